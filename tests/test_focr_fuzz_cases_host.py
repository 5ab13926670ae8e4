"""The cases of tests/focr_fuzz_cases.py on the models alone: every mode accepts every case (none may be left out on the
device), the committed seed reaches every property the cases are for, each asserted by name, and off the default font
setup the fast models still equal one FreeType raster per candidate.  No GPU needed."""
import numpy as np

import focr_fuzz_cases as FC
import focr_line_model as M
import focr_margins_model as MM
import focr_scores_model as SC
import focr_search_model as S
import focr_slack_model as K
import focr_whole_model as W
from font_ocr_amd.decoder import raster_glyph

F32 = np.float32
ALL = range(FC.N_CASES)


def _lines(c, mode):
    return [r for pg in FC.want(c, mode) for _, r in pg]


def test_every_mode_accepts_every_case():
    """The refusals of include/focr_decode.h, restated: none applies to any case, and every model returns an answer."""
    for i in ALL:
        c = FC.case(i)
        fm, p = FC.model(c), FC.plan(c)
        assert float(fm.ox) == int(fm.ox) >= 0, c.name
        assert p["lo"] >= 1 and 64 * p["w"] + p["hi"] < 1 << 24, c.name
        assert p["batch"] + p["hi"] <= FC.WHOLE_RING_MAX and p["ring"] <= FC.WHOLE_RING_MAX, c.name
        assert 1 <= c.radius <= min(64, S.max_radius(fm.incs)) and 1 <= c.slack <= min(16, K.max_slack(fm.incs)), c.name
        g = fm.font.s.glyphs
        T = max(g[k].stride * g[k].box_h * 2 * 255 * 255 for k in range(len(c.alphabet)))
        assert K.char_bound(fm.incs, p["w"], c.slack) * T < 1 << 47, c.name
        assert 2 <= len(set(c.alphabet)) == len(c.alphabet) <= 12 and set(c.alphabet) <= set(FC.ASCII95), c.name
        for mode in FC.MODES:
            want = FC.want(c, mode)
            assert len(want) == len(c.pages), (c.name, mode)
            assert [[y for y, _ in pg] for pg in want] == [[y for y, _ in pg] for pg in FC.want(c, "plain")], (c.name, mode)


def test_fixed_cases_are_what_they_are_named():
    fixed = {FC.case(i).name.split("-", 1)[1]: FC.case(i) for i in range(FC.N_RANDOM, FC.N_CASES)}
    assert list(fixed) == [name for name, _ in FC.FIXED]
    c = fixed["x-at-page-width"]
    assert all(c.geo[0] == p.shape[1] and c.geo[1] < p.shape[0] and (p != 255).any() for p in c.pages) and FC.plan(c)["w"] == 0
    assert all(len(FC.crops(c, p)) >= 2 for p in c.pages) and all(pg == [] for pg in FC.want(c, "plain"))
    c = fixed["y-past-page"]
    assert all(c.geo[1] >= p.shape[0] and FC.crops(c, p) == [] for p in c.pages)
    c = fixed["one-column"]
    assert FC.plan(c)["w"] == 1 and _lines(c, "whole") and all(len(t) >= 1 for t in _lines(c, "plain"))
    c = fixed["line-height-1"]
    assert c.geo[3] == 1 and _lines(c, "whole")
    # glyphs that miss the one row cost nothing anywhere, so states tie between glyphs of different advances and the lower
    # index decides (where the slack model once kept the lower pen's glyph): the reversed alphabet reads another text
    rev = FC.fast(c.font, c.size, c.alphabet[::-1], c.hinting, c.kerning)
    refs = [ref for page in c.pages for _, ref in FC.crops(c, page) if not np.all(ref == 255)]
    assert any(K.slack_line(rev, ref, c.slack).text != s.text for ref, s in zip(refs, _lines(c, "slack")))
    c = fixed["advance-1-height-12"]
    assert c.geo[3:] == (12, 1) and len(FC.want(c, "whole")[0]) >= 12
    c = fixed["min-inc64-above-512"]
    assert FC.plan(c)["lo"] == 1202 and FC.plan(c)["batch"] == FC.plan(c)["slack_batch"] == 512 and _lines(c, "slack")
    c = fixed["min-inc64-below-64"]
    assert FC.plan(c)["lo"] == 63 and _lines(c, "slack")


def test_the_cases_reach_what_they_are_for():
    """Each property has at least one case under the committed seed; a change to the generator that loses one fails here
    by name."""
    reach = {}

    def note(name, i, hit):
        reach.setdefault(name, [])
        if hit:
            reach[name].append(i)

    for i in ALL:
        c = FC.case(i)
        fm, p = FC.model(c), FC.plan(c)
        x, y, width, lh, adv = c.geo
        font = {FC.SANS: "sans", FC.SERIF: "serif", FC.MONO: "mono"}[c.font]
        for f in ("sans", "serif", "mono"):
            note(f + " hinted", i, font == f and c.hinting)
            note(f + " unhinted", i, font == f and not c.hinting)
        inked = any((p_ != 255).any() for p_ in c.pages) and bool(_lines(c, "plain"))
        note("kerning below 1", i, inked and c.kerning < 1)
        note("kerning above 1", i, inked and c.kerning > 1)
        note("origin_x 1", i, inked and float(fm.ox) == 1)
        note("line_advance below line_height", i, inked and adv < lh)
        note("line_advance equal to line_height", i, inked and adv == lh)
        note("line_advance above line_height", i, inked and adv > lh)
        note("width clipped by the page", i, inked and any(0 < pg.shape[1] - x < width for pg in c.pages))
        note("last slot cut by the bottom edge", i, inked and any(
            FC.crops(c, pg) and 0 < FC.crops(c, pg)[-1][1].shape[0] < lh and FC.crops(c, pg)[-1][1].shape[1] > 0 for pg in c.pages))
        note("a cut last slot with ink", i, any(pg and pg[-1][0] + lh > page.shape[0] for pg, page in zip(FC.want(c, "plain"), c.pages)))
        note("pages of two sizes", i, inked and len({pg.shape for pg in c.pages}) == 2)
        note("a blank page between inked ones", i, len(c.pages) == 3 and [bool((pg != 255).any()) for pg in c.pages] == [True, False, True])
        note("a blank slot between non-blank ones", i, any(
            len(pg) >= 2 and len(pg) < (pg[-1][0] - pg[0][0]) // adv + 1 for pg in FC.want(c, "plain")))
        note("batch capped at 512", i, inked and p["batch"] == 512 and p["lo"] > 512)
        note("batch below 100", i, inked and p["slack_batch"] < p["batch"] < 100)
        note("whole-line text differs from greedy", i, any(
            a.text != b for pa, pb in zip(FC.want(c, "whole"), FC.want(c, "plain")) for (_, a), (_, b) in zip(pa, pb)))
        note("slack takes a non-zero offset", i, any(s.offsets.any() for s in _lines(c, "slack")))
        note("slack text differs from whole-line", i, [s.text for s in _lines(c, "slack")] != [s.text for s in _lines(c, "whole")])
        note("search takes a non-zero offset", i, any(s.offsets.any() for s in _lines(c, "search")))
        note("search takes offsets of both signs", i, any((s.offsets < 0).any() and (s.offsets > 0).any() for s in _lines(c, "search")))
        note("a doubtful margin", i, any(
            len(m.margin) and ((m.runner != MM.NO_RUNNER) & ((m.margin == 0) | (m.margin < np.abs(m.term.astype(np.int64)).min()))).any()
            for m in _lines(c, "margins")))
        note("scores with a runner", i, any((s.runner != SC.NO_RUNNER).any() for s in _lines(c, "scores")))
        note("more than one character a line", i, any(len(t) > 8 for t in _lines(c, "plain")))
    print({k: len(v) for k, v in reach.items()})
    for name, hits in reach.items():
        assert hits, "no case reaches: " + name
    assert [name for name, hits in reach.items() if not [i for i in hits if i < FC.N_RANDOM]] == [], "only a fixed case reaches it"


def pinned_cases():
    """Six random cases that between them cover Serif, hinting on, kerning 0.6 and kerning 1.3: for each of the four the
    cheapest case that has it, then the cheapest others.  The cost is the brute-force search's rasters."""
    cs = [FC.case(i) for i in range(FC.N_RANDOM)]
    cs = [c for c in cs if _lines(c, "plain")]
    cost = {c.index: sum(len(t) for t in _lines(c, "plain")) * (2 * c.radius + 1) * len(c.alphabet) for c in cs}
    cs.sort(key=lambda c: (cost[c.index], c.index))
    picked = []
    for has in (lambda c: c.font == FC.SERIF, lambda c: c.hinting, lambda c: c.kerning == 0.6, lambda c: c.kerning == 1.3):
        first = next(c for c in cs if has(c))
        if first not in picked:
            picked.append(first)
    picked += [c for c in cs if c not in picked][: 6 - len(picked)]
    return picked


def test_fast_models_equal_freetype_off_the_default_setup():
    """On every line of six cases: FastModel.decode_line is the brute-force decode_line, line_scores is
    brute_line_scores, search_line is brute_search_line, each with the case's kerning and hinting; and a sample of the
    terms the whole-line model asks for equal one FreeType raster of the candidate each."""
    picked = pinned_cases()
    assert len(picked) == 6
    assert any(c.font == FC.SERIF for c in picked) and any(c.hinting for c in picked) and any(not c.hinting for c in picked)
    assert any(c.kerning == 0.6 for c in picked) and any(c.kerning == 1.3 for c in picked)
    n_lines = n_terms = 0
    for c in picked:
        fm = FC.model(c)
        ox, oy = fm.font.origin
        assert (ox, oy) == M.origin(c.font, c.size, c.alphabet), c.name
        for page in c.pages:
            for y, ref in FC.crops(c, page):
                if np.all(ref == 255):
                    continue
                where = (c.name, y)
                n_lines += 1
                assert fm.decode_line(ref) == M.decode_line(ref, c.font, c.size, c.alphabet, c.kerning, c.hinting), where
                for a, b in ((SC.line_scores(fm, ref), SC.brute_line_scores(ref, c.font, c.size, c.alphabet, c.kerning, c.hinting)),
                             (S.search_line(fm, ref, c.radius), S.brute_search_line(ref, c.font, c.size, c.alphabet, c.radius, c.kerning, c.hinting))):
                    assert type(a) is type(b) and all(np.array_equal(u, v) for u, v in zip(a, b)), where
                h, w = ref.shape
                calls = [0]

                def pinned(fm_, r, total, s):
                    got = W.term_from_scores(fm_, r, total, s)
                    calls[0] += 1
                    if calls[0] % 3 == 1:
                        for k, ch in enumerate(c.alphabet):
                            canvas = np.zeros((h, w), dtype=np.uint8)
                            raster_glyph(c.font, c.size, ch, F32(ox + F32(s) / F32(64)), oy, canvas, c.hinting)
                            assert got[k] == int(((r - canvas.astype(np.int64)) ** 2).sum()) - total, where + (s, ch)
                    return got

                W.whole_line(fm, ref, term=pinned)
                n_terms += (calls[0] + 2) // 3
    assert n_lines >= 6 and n_terms >= 60

"""The cases of tests/focr_fonts_fuzz.py on the models alone: neither form refuses any candidate of any case (none may be
left out on the device), the committed seed reaches every property the cases are for, each asserted by name and by a
random case, the FIXED cases are what they are named, and off the default font setup the model's per-candidate cost still
equals one FreeType raster per chosen character.  No GPU needed."""
import numpy as np

import focr_fonts_fuzz as FZ
import focr_fonts_model as FM
import focr_whole_model as W
from focr_fast_model import line_cap
from font_ocr_amd.decoder import raster_glyph

F32 = np.float32
ALL = range(FZ.N_CASES)


def _lines(c, form):
    return [r for pg in FZ.want(c, form) for _, r in pg]


def test_neither_form_refuses_any_candidate():
    """The checks of focr_decoder_set_font_candidates and of whole_font_plan, restated per candidate of every case, on the
    case's widest crop; and both models answer for every page."""
    for i in ALL:
        c = FZ.case(i)
        ms, w = FZ.models(c), FZ.crop_width(c)
        assert 1 <= len(c.cands) <= 15 and len(ms) == len(c.cands) + 1, c.name
        assert 2 <= len(set(c.alphabet)) == len(c.alphabet) <= 12, c.name
        s0 = ms[0].font.s
        for k, m in enumerate(ms):
            who, s = (c.name, k), m.font.s
            assert s.n_glyphs == s0.n_glyphs == len(c.alphabet), who
            assert [s.glyphs[j].codepoint for j in range(s.n_glyphs)] == [s0.glyphs[j].codepoint for j in range(s.n_glyphs)], who
            assert all(s.glyphs[j].increment > 0 for j in range(s.n_glyphs)), who
            assert float(m.ox) == int(m.ox) >= 0 and float(s.origin_x) == float(m.ox), who
            inc = W.inc64(m.incs)
            lo, hi = int(inc.min()), int(inc.max())
            assert lo >= 1 and 64 * w + hi < 1 << 24, who
            T = max(s.glyphs[j].stride * s.glyphs[j].box_h * 2 * 255 * 255 for j in range(s.n_glyphs))
            assert T < 1 << 31 and max(-(-64 * w // lo), 1) * T < 1 << 47, who
            assert min(lo, FZ.WHOLE_BATCH_MAX) + hi <= FZ.WHOLE_RING_MAX, who
            p = FZ.font_plan(m, w)
            assert p is not None and (p["lo"], p["hi"]) == (lo, hi) and p["batch"] + hi <= p["ring"] <= FZ.WHOLE_RING_MAX, who
        for form in FZ.FORMS:
            want = FZ.want(c, form)
            assert len(want) == len(c.pages), (c.name, form)
            assert [[y for y, _ in pg] for pg in want] == [[y for y, ref in FZ.crops(c, p) if not np.all(ref == 255)] for p in c.pages], (c.name, form)
            assert all(0 <= r.k <= len(c.cands) and r.trail[-1] == (r.k, r.cost) for r in _lines(c, form)), (c.name, form)


def test_the_cases_reach_what_they_are_for():
    """Each property has at least one random case under the committed seed; a change to the generator that loses one fails
    here by name."""
    reach = {}

    def note(name, i, hit):
        reach.setdefault(name, [])
        if hit:
            reach[name].append(i)

    for i in ALL:
        c = FZ.case(i)
        ms, K = FZ.models(c), len(c.cands)
        x, y, width, lh, adv = c.geo
        plans = [FZ.font_plan(m, FZ.crop_width(c)) for m in ms]
        pen, whole = FZ.want(c, "pen"), FZ.want(c, "whole")
        inked = bool(_lines(c, "pen"))
        for form in FZ.FORMS:
            ks = [r.k for r in _lines(c, form)]
            note(form + ": the decode font wins", i, 0 in ks)
            note(form + ": the last candidate wins", i, K in ks)
            note(form + ": a candidate strictly between wins", i, any(0 < k < K for k in ks))
        note("the two forms pick different winners for a line", i, any(a.k != b.k for a, b in zip(_lines(c, "pen"), _lines(c, "whole"))))
        for v in range(4):
            note("n_fonts & 3 == %d" % v, i, inked and (K + 1) & 3 == v)
        note("K = 1", i, inked and K == 1)
        note("K = 15", i, inked and K == 15)
        note("a winner that is not the first candidate of its wave (k >= 4)", i, any(r.k >= 4 for r in _lines(c, "pen")))
        note("a decode font at origin_x 1 loses to a candidate at 0", i, float(ms[0].ox) == 1 and any(r.k and float(ms[r.k].ox) == 0 for r in _lines(c, "pen")))
        note("a decode font at origin_x 0 loses to a candidate at 1", i, float(ms[0].ox) == 0 and any(r.k and float(ms[r.k].ox) == 1 for r in _lines(c, "pen")))
        note("a winner's text is longer than the decode font's line_cap", i, any(
            r.k and len(r.text) > line_cap(ms[0].incs, ref.shape[1])
            for pg, page in zip(pen, c.pages) for (_, r), (_, ref) in zip(pg, [cr for cr in FZ.crops(c, page) if not np.all(cr[1] == 255)])))
        trails = [len(r.trail) for r in _lines(c, "whole")]
        note("whole: the best changes three times or more", i, any(t >= 3 for t in trails))
        note("whole: the winner lies in half 1", i, any(t % 2 == 0 for t in trails))
        note("whole: the winner lies in half 0 after a swap", i, any(t % 2 == 1 and t >= 3 for t in trails))
        note("whole: a batch capped at 512 beside one below 512", i, inked and any(p["lo"] > 512 for p in plans) and any(p["lo"] < 512 for p in plans))
        note("whole: a candidate's ring exceeds the decode font's", i, inked and any(p["ring"] > plans[0]["ring"] for p in plans[1:]))
        note("width clipped by the page", i, inked and any(0 < pg.shape[1] - x < width for pg in c.pages))
        note("a cut last slot with ink won by k > 0", i, any(pg and pg[-1][0] + lh > page.shape[0] and pg[-1][1].k > 0 for pg, page in zip(pen, c.pages)))
        note("line_advance below line_height", i, inked and adv < lh)
        note("line_advance equal to line_height", i, inked and adv == lh)
        note("line_advance above line_height", i, inked and adv > lh)
        note("x off 2 and y off 0", i, inked and x != 2 and y != 0)
        note("pages of two sizes", i, inked and len({pg.shape for pg in c.pages}) == 2)
        note("a blank page between inked ones", i, len(c.pages) == 3 and [bool((pg != 255).any()) for pg in c.pages] == [True, False, True])
        note("a blank slot between inked ones", i, any(len(pg) >= 2 and len(pg) < (pg[-1][0] - pg[0][0]) // adv + 1 for pg in pen))
        note("hinted and unhinted candidates in one case", i, inked and len({h for _, _, h, _ in c.cands} | {c.hinting}) == 2)
        note("three faces in one case", i, inked and len({f for f, _, _, _ in c.cands} | {c.font}) == 3)
        note("a candidate at least twice the size of another", i, inked and max(t for _, t, _, _ in c.cands) >= 2 * min(t for _, t, _, _ in c.cands))
    print({k: len(v) for k, v in reach.items()})
    for name, hits in reach.items():
        assert hits, "no case reaches: " + name
    assert [name for name, hits in reach.items() if not [i for i in hits if i < FZ.N_RANDOM]] == [], "only a fixed case reaches it"


def test_fixed_cases_are_what_they_are_named():
    fixed = {FZ.case(i).name.split("-", 1)[1]: FZ.case(i) for i in range(FZ.N_RANDOM, FZ.N_CASES)}
    assert list(fixed) == [name for name, _ in FZ.FIXED]
    for c in fixed.values():  # none is on the geometry of tests/test_gpu_focr_fonts.py: clipped, overlapping, cut
        x, y, width, lh, adv = c.geo
        assert all(0 < p.shape[1] - x < width for p in c.pages) and adv < lh, c.name
        assert all(0 < FZ.crops(c, p)[-1][1].shape[0] < lh for p in c.pages), c.name
        assert sum(len(pg) for pg in FZ.want(c, "pen")) >= 3, c.name

    def tie(c, first, twin):
        """The twins are one font, the first wins a line in both forms, and on that line the twin's own cost is the winner's."""
        ms = FZ.models(c)
        assert ms[first] is ms[twin] and first < twin, c.name
        n = 0
        for form in FZ.FORMS:
            for page, pg in zip(c.pages, FZ.want(c, form)):
                refs = dict(FZ.crops(c, page))
                for y, r in pg:
                    assert r.k != twin, (c.name, form, y)
                    if r.k == first:
                        n += 1
                        own = FM.pen_loop(ms[twin], refs[y])[1] if form == "pen" else W.whole_line(ms[twin], refs[y]).cost
                        assert own == r.cost, (c.name, form, y)
        assert n >= 2, c.name

    c = fixed["tie-with-the-decode-font"]
    assert c.cands[1] == (c.font, c.size, c.hinting, c.kerning)
    tie(c, 0, 2)
    c = fixed["tie-in-two-waves"]
    assert (1 & 3, 2 & 3) == (1, 2)
    tie(c, 1, 2)
    c = fixed["tie-in-one-wave"]
    assert 1 & 3 == 5 & 3
    tie(c, 1, 5)
    c = fixed["last-of-fifteen"]
    assert len(c.cands) == 15 and len(set(c.cands) | {(c.font, c.size, c.hinting, c.kerning)}) == 16
    assert {k for pg in c.ink for _, k in pg} == {15}
    for form in FZ.FORMS:
        assert sum(r.k == 15 for r in _lines(c, form)) >= 2, form
    c = fixed["cap-is-the-candidate's"]
    ms, w = FZ.models(c), FZ.crop_width(c)
    assert ms[0].incs.min() > 2 * min(m.incs.min() for m in ms[1:])
    caps = [line_cap(m.incs, w) for m in ms]
    assert max(caps[1:]) > 2 * caps[0]
    assert any(r.k and len(r.text) > caps[0] for r in _lines(c, "pen"))
    c = fixed["whole-batches-and-rings"]
    plans = [FZ.font_plan(m, FZ.crop_width(c)) for m in FZ.models(c)]
    assert plans[0]["lo"] < 512 and sorted(p["batch"] for p in plans)[-2:] == [512, 512] and len({p["batch"] for p in plans}) == 3
    assert max(p["ring"] for p in plans[1:]) > plans[0]["ring"] and len({r.k for r in _lines(c, "whole")}) >= 3


def pinned_lines():
    """Six inked lines of the random cases, the cheapest by crop area that between them have a Serif candidate, a hinted one
    and kernings below and above 1 among the fonts scored."""
    cs = [FZ.case(i) for i in range(FZ.N_RANDOM)]
    lines = [(c, p, y, ref) for c in cs for p, page in enumerate(c.pages) for y, ref in FZ.crops(c, page) if not np.all(ref == 255)]
    lines.sort(key=lambda l: (l[3].size * (len(l[0].cands) + 1), l[0].index, l[1], l[2]))
    specs = lambda c: [(c.font, c.size, c.hinting, c.kerning)] + list(c.cands)
    picked = []
    for has in (lambda s: s[0] == FZ.SERIF, lambda s: s[2], lambda s: s[3] < 1, lambda s: s[3] > 1):
        first = next(l for l in lines if any(has(s) for s in specs(l[0])))
        if not any(first is l for l in picked):
            picked.append(first)
    picked += [l for l in lines if not any(l is q for q in picked)][: 6 - len(picked)]
    return picked


def test_model_costs_equal_freetype_off_the_default_setup():
    """On six lines: every candidate's pen-loop cost is the brute-force sum, per chosen character, of one raster_glyph term at
    the model's own pen, with the candidate's face, size and hinting; its kerning is in the pens."""
    picked = pinned_lines()
    assert len(picked) == 6
    seen = set()
    n = 0
    for c, p, y, ref in picked:
        h, w = ref.shape
        r = 255 - ref.astype(np.int64)
        total = int((r * r).sum())
        for k, (m, (face, size, hinting, kerning)) in enumerate(zip(FZ.models(c), [(c.font, c.size, c.hinting, c.kerning)] + list(c.cands))):
            idx, cost, base = FM.pen_loop(m, ref)
            assert base == total
            ox, oy = m.font.origin
            pos, brute = F32(0), 0
            for i in idx:
                canvas = np.zeros((h, w), dtype=np.uint8)
                raster_glyph(face, size, c.alphabet[i], F32(ox + pos), oy, canvas, hinting)
                brute += int(((r - canvas.astype(np.int64)) ** 2).sum()) - total
                pos = F32(pos + m.incs[i])
            assert brute == cost, (c.name, p, y, k)
            seen |= {("serif", face == FZ.SERIF), ("hinted", hinting), ("below", kerning < 1), ("above", kerning > 1)}
            n += len(idx)
    assert {("serif", True), ("hinted", True), ("below", True), ("above", True)} <= seen and n >= 60

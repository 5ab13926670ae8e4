"""What makes tests/test_gpu_focr_text_fuzz.py mean something, on the CPU and with the committed models only
(tests/focr_text_fuzz.py): the references agree with each other on every seeded case, so a device test built on them can
fail only because of the device; the cases and the random readings reach the edges they are there for; and the two pictures
of a reading, focr_verify_text_model.verify_text and the mode's own verify_image, are one picture.

The identity runs every family, case, mode and line but the modes that return no number of their own ("plain" and "search"
of "cases": their texts and offsets are those of "scores" and "search_scores"); nothing else is thinned.  The seed of the
random readings (focr_text_fuzz.SEED) was chosen so that the last test holds."""
import numpy as np
import pytest

import focr_fuzz_cases as FC
import focr_line_model as M
import focr_score_text_model as SM
import focr_search_model as S
import focr_text_fuzz as T
import focr_verify_text_model as VT
import focr_whole_model as W
from font_ocr_amd import VerifyFont

NUMBERED = [(f, m) for f in T.FAMILIES for m in T.MODES[f] if m not in ("plain", "search")]


def _note(seen, s, got, kw):
    """What the lines fed back from one run reach, added to seen."""
    x, _, width, lh, _ = s.geo
    if len({p.shape for p in s.pages}) > 1:
        seen.add("two page sizes in one call")
    if len(s.fonts) == 16:
        seen.add("K = 15")
    n_lines = [len(pg) for pg in got["lines"]]
    if len(n_lines) == 3 and n_lines[0] and not n_lines[1] and n_lines[2]:
        seen.add("a blank page between two others")
    for p, pg in enumerate(got["lines"]):
        H, Wp = s.pages[p].shape
        w = min(width, Wp - min(x, Wp))
        for n, (y, text) in enumerate(pg):
            k = kw["fonts"][p][n] if "fonts" in kw else 0
            f = s.fonts[k]
            offs = kw["offsets"][p][n] if "offsets" in kw else None
            pens = kw["pens"][p][n] if "pens" in kw else None
            ds = SM.deltas(f, [s.alphabet.index(c) for c in text], pens, offs)
            q = kw["baselines"][p][n] if "baselines" in kw else 0
            for on, what in ((w < width, "a crop clipped at the right"), (H - y < lh, "a crop cut at the bottom"), (f.hinting, "hinting on"),
                             (float(f.kerning) != 1.0, "kerning != 1"), (offs is not None and np.any(np.asarray(offs) != 0), "a non-zero offset"),
                             (any(d >= 64 * w for d in ds), "a glyph wholly past the crop"),
                             (q != 0 and q & ((1 << s.y_bits) - 1), "q != 0 with a non-zero phase"), (k != 0, "k != 0")):
                if on:
                    seen.add(what)


@pytest.mark.parametrize("family,mode", NUMBERED, ids=["%s-%s" % fm for fm in NUMBERED])
def test_a_model_run_fed_back_costs_what_it_returned(family, mode):
    """The references' identity on every case and line of a (family, mode): score.cost == want.cost; with scores
    score.base == want.base and terms == want.score - want.base; for margins terms == want.term."""
    n = 0
    for i in T.IDS[family]:
        s = T.setup(family, i, mode)
        got = T.model_run(s)
        kw = T.feed(s, got)
        T.identity(s, got, T.reference_scores(s, got["lines"], **kw))
        n += sum(len(pg) for pg in got["lines"])
    assert n > 0, (family, mode)


def test_the_fed_back_lines_reach_their_edges():
    """Asserted, not printed: every edge below is reached by at least one line fed back from a run."""
    seen = set()
    for family, mode in NUMBERED:
        for i in T.IDS[family]:
            s = T.setup(family, i, mode)
            got = T.model_run(s)
            _note(seen, s, got, T.feed(s, got))
    want = {"a crop clipped at the right", "a crop cut at the bottom", "hinting on", "kerning != 1", "a non-zero offset", "a glyph wholly past the crop",
            "q != 0 with a non-zero phase", "k != 0", "K = 15", "two page sizes in one call", "a blank page between two others"}
    assert want - seen == set(), sorted(want - seen)


def test_geometries_without_a_crop_score_zeros():
    """x-at-page-width and y-past-page: no run returns a line.  Where the crop has no column every random reading has
    line_base 0 and every term 0, as include/focr_decode.h says of an empty crop (score_text has no y_start, so the readings of
    y-past-page lie on the page like any other's; those at a y of page_h or more score zeros as well)."""
    names = {FC.case(i).name.split("-", 1)[1]: i for i in range(FC.N_RANDOM, FC.N_CASES)}
    for name in ("x-at-page-width", "y-past-page"):
        s = T.setup("cases", names[name])
        assert not any(T.model_run(T.setup("cases", s.index, m))["lines"][p] for m in FC.MODES for p in range(len(s.pages))), name
        for p in range(len(s.pages)):
            r = T.random_reading("cases", s.index, p)
            for rec, sc in zip(r.recs, T.reading_scores(s, r)):
                if name == "x-at-page-width" or rec[0] >= s.pages[p].shape[0]:
                    assert (sc.base, sc.cost, sc.shift) == (0, 0, 0) and not sc.terms.any(), (name, p)


def test_the_random_readings_reach_their_edges():
    """Every edge the random readings are there for is reached by at least one of them."""
    seen = set()
    for family in T.FAMILIES:
        for i in T.IDS[family]:
            s = T.setup(family, i)
            x, _, width, _, _ = s.geo
            for p in range(len(s.pages)):
                r = T.random_reading(family, i, p)
                assert r == T.random_reading(family, i, p)  # a function of its arguments alone
                w = min(width, s.pages[p].shape[1] - min(x, s.pages[p].shape[1]))
                scores = T.reading_scores(s, r)
                spans = [(first, first + n) for _, first, n, _, _ in r.recs]
                for on, what in ((any(d < 0 for ds in T.reading_deltas(s, r, scores) for d in ds), "a negative delta"),
                                 (r.placement == "pens" and any(v >= 64 * w for v in r.along), "a pen past the crop"),
                                 (len(set(r.recs)) < len(r.recs), "a repeated line"),
                                 (any(a[0] < b[1] and b[0] < a[1] and r.recs[m] != r.recs[n] for m, a in enumerate(spans) for n, b in enumerate(spans) if m < n),
                                  "two lines sharing characters"),
                                 (any(sc.shift != 0 for sc in scores), "a winner at a shift != 0"),
                                 (r.with_q and any(rec[3] != 0 for rec in r.recs), "a whole-row q in a candidate font"),
                                 (r.y_bits and any(rec[4] & ((1 << r.y_bits) - 1) for rec in r.recs), "a fractional-phase q")):
                    if on:
                        seen.add(what)
    want = {"a negative delta", "a pen past the crop", "a repeated line", "two lines sharing characters", "a winner at a shift != 0",
            "a whole-row q in a candidate font", "a fractional-phase q"}
    assert want - seen == set(), sorted(want - seen)


_vfonts = {}


def _verify_font(c):
    if c.index not in _vfonts:
        _vfonts[c.index] = VerifyFont(c.font, c.size, c.alphabet, c.hinting, c.kerning)
    return _vfonts[c.index]


@pytest.mark.parametrize("mode", FC.MODES)
def test_the_two_pictures_agree(mode):
    """focr_verify_text_model.verify_text of a model reading is the mode's existing verify_image of it, image bytes and sum, on
    every third case of tests/focr_fuzz_cases.py: M.verify_image (the pen loop), S.verify_image (the pen search) or
    W.verify_image (the whole kinds)."""
    for i in range(0, FC.N_CASES, 3):
        s = T.setup("cases", i, mode)
        c, x = s.case, s.geo[0]
        got = T.model_run(s)
        kw = T.picture_feed(T.feed(s, got))
        want = FC.want(c, mode)
        for p, (img, sq) in enumerate(T.reference_pictures(s, got["lines"], **kw)):
            page, want_pg = c.pages[p], want[p]
            if mode in ("plain", "scores"):
                old = M.verify_image(page, got["lines"][p], c.font, c.size, x, c.kerning, c.hinting)  # (image, the MSE as an f32)
                assert old[1].tobytes() == VT.mse(sq, page.shape[1], page.shape[0]).tobytes(), (c.name, mode, p)
                old = (old[0], sq)
            elif mode in ("search", "search_scores"):
                old = S.verify_image(page, [(y, r.text, r.pens) for y, r in want_pg], FC.model(c).font, _verify_font(c), x)
            else:
                old = W.verify_image(page, [(y, r.text, r.pens) for y, r in want_pg], FC.model(c).font, _verify_font(c), x)
            assert img.tobytes() == old[0].tobytes() and sq == old[1], (c.name, mode, p)

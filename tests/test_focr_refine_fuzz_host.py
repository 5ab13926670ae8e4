"""What makes tests/test_gpu_focr_refine_fuzz.py mean something, on the CPU and with the committed models only
(tests/focr_refine_fuzz.py): the seeded cases and readings, at their drawn (radius, sweeps, glyphs), reach the steps and crops the
device test is there for; the kernel's neighbour bound (the others that can reach a step's window are found from the INPUT pens and
a slack of radius * sweeps, decode_refine.hip step (1)) is the definition on every one of them, and a slack of radius alone is not;
and the phase tables' model is the brute force of one FreeType raster per candidate on six short seeded lines.

The first test goes three cases at a time, so that their model answers cost a few seconds each; the tests over all of them read
the same answers (computed once, focr_refine_fuzz.model_fed and reading_reference).  The floors below are well under what the model gives at
focr_refine_fuzz.SEED, which was chosen so that they hold (the figures behind each floor)."""
import collections

import numpy as np
import pytest

import focr_refine_fuzz as RF
import focr_refine_model as R
import focr_text_fuzz as TF
from focr_fast_model import FastModel, crop
from focr_fuzz_cases import SANS


def same(a, b):
    return a[:6] == b[:6] and np.array_equal(a.pens, b.pens)


def every_line(family, ids):
    """(setup, page, y, idx, pens, k, (radius, sweeps, glyphs), Refine, notes, what) of every fed-back line and every reading's record."""
    for i in ids:
        for mode in RF.MODES[family]:
            s, _, (lines, pens, fonts, *par), ref = RF.model_fed(family, i, mode)
            for p, pg in enumerate(lines):
                for n, (y, text) in enumerate(pg):
                    k = fonts[p][n] if fonts is not None else 0
                    yield (s, p, y, [s.alphabet.index(c) for c in text], pens[p][n], k, tuple(par)) + ref[p][n] + (mode,)
        s = TF.setup(family, i)
        for p in range(len(s.pages)):
            s, r, par, ref = RF.reading_reference(family, i, p)
            for (y, first, m, k), (res, notes) in zip(r.recs, ref):
                yield s, p, y, r.chars[first: first + m], r.pens[first: first + m], k, par, res, notes, "reading"


# three cases a test (half a group of the device module), so that each stays at a few seconds
CHUNKS = [(f, list(RF.IDS[f][a: a + 3])) for f in RF.FAMILIES for a in range(0, len(RF.IDS[f]), 3)]


@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=["%s%s-%s" % (f, g[0], g[-1]) for f, g in CHUNKS])
def test_the_neighbour_bound_is_the_definition(chunk):
    """refine_crop on the canvas of the characters the kernel's scan admits (slack = radius * sweeps) equals refine_crop on the canvas
    of every character, field for field, on every fed-back line and every reading's record of the chunk."""
    family, ids = CHUNKS[chunk]
    n = 0
    for s, p, y, idx, pens, k, (radius, sweeps, glyphs), want, _, what in every_line(family, ids):
        x, _, width, lh, _ = s.geo
        got, _ = RF.refine_within(RF.models(s)[k], crop(s.pages[p], x, y, width, lh), idx, pens, radius, sweeps, glyphs, radius * sweeps)
        assert same(got, want), (family, s.name, what, p, y)
        n += 1
    assert n > 0 or all(not any(TF.model_run(TF.setup(family, i, m))["lines"]) for i in ids for m in RF.MODES[family])


@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=["%s%s-%s" % (f, g[0], g[-1]) for f, g in CHUNKS])
def test_no_seeded_line_tells_a_slack_of_one_radius_apart(chunk):
    """Why the other half of the argument needs a directed line: on every seeded line and record with two sweeps or more and a
    radius (1122 of them), the scan with slack = radius gives the definition's result too."""
    family, ids = CHUNKS[chunk]
    for s, p, y, idx, pens, k, (radius, sweeps, glyphs), want, _, what in every_line(family, ids):
        if sweeps >= 2 and radius:
            x, _, width, lh, _ = s.geo
            got, _ = RF.refine_within(RF.models(s)[k], crop(s.pages[p], x, y, width, lh), idx, pens, radius, sweeps, glyphs, radius)
            assert same(got, want), (family, s.name, what, p, y)


def ramp_line():
    """Two `m` of Sans 13 px, 24 px apart, on a page that darkens over columns 10 .. 15, stays dark up to column 26 and is white from
    there: the left one climbs the ramp by a whole pixel in each of eight sweeps, the right one hides its ink under it.  (No seeded
    line does it, the test above; nor did dense lines on noise at radius 64 and 3 and 8 sweeps that were tried: a step's window starts 3 .. 6 columns left of the first column a candidate touches, as whole strip dwords, and a box has
    blank columns, so a character has to come some 8 px closer than its input pen says before the scan leaves it out wrongly.)"""
    fm = FastModel(SANS, 13.0, "m")
    r = np.minimum(148, np.maximum(0, 29 * (np.arange(90) - 10)))
    r[27:] = 0
    return fm, (255 - r).astype(np.uint8)[None, :].repeat(17, 0), [0, 0], [93, 1619]


def test_a_slack_of_one_radius_is_not_enough():
    """The other half of the argument: with slack = radius the scan leaves out a character that has moved into reach, and the result
    differs; with radius * sweeps it is the definition's again."""
    fm, ref, idx, pens = ramp_line()
    want = R.refine_crop(fm, ref, idx, pens, 64, 8, False)
    assert want.sweeps == 8 and want.pens.tolist() == [596, 1279]  # both have moved further than one radius
    assert same(RF.refine_within(fm, ref, idx, pens, 64, 8, False, 64 * 8)[0], want)
    short = RF.refine_within(fm, ref, idx, pens, 64, 8, False, 64)[0]
    assert not same(short, want) and short.pens.tolist() == [596, 1107] and short.cost != want.cost
    fm.close()


def test_the_draws_and_the_line_counts():
    """draw() and reading() are functions of their arguments alone and cover every radius, every sweep count and both glyphs; the
    radii above 7 go to cut lines or to at most two sweeps; every mode returns focr_refine_fuzz.LINES lines and the readings RECORDS
    records (what the device module counts); 16 characters of pen-search runs lie left of pen 0 and go in at 0."""
    seen, lines, below, records = set(), collections.Counter(), 0, 0
    for family in RF.FAMILIES:
        for i in RF.IDS[family]:
            s = TF.setup(family, i)
            for mode in RF.MODES[family] + tuple(range(len(s.pages))):
                par = RF.draw(family, i, mode)
                assert par == RF.draw(family, i, mode) and par[0] in RF.RADII and par[1] in RF.SWEEPS
                assert par[0] <= 7 or par[1] <= 2 or RF.cut(family, i, mode) == RF.CUT
                seen.update([("radius", par[0]), ("sweeps", par[1]), ("glyphs", par[2])])
            for mode in RF.MODES[family]:
                s, got, (fed_lines, pens, _, *_), _ = RF.model_fed(family, i, mode)
                lines[family, mode] += sum(len(pg) for pg in fed_lines)
                below += RF.below_zero(s, got)
                assert all(len(t) == len(ps) for pg, pp in zip(fed_lines, pens) for (_, t), ps in zip(pg, pp))
            for p in range(len(s.pages)):
                r = RF.reading(family, i, p)
                assert r == RF.reading(family, i, p)
                tf = TF.random_reading(family, i, p)
                assert r.chars == list(tf.chars) and r.recs == [rec[:4] for rec in tf.recs]  # records, characters, ys and fonts as they are
                records += len(r.recs)
    assert seen == {("radius", v) for v in RF.RADII} | {("sweeps", v) for v in RF.SWEEPS} | {("glyphs", True), ("glyphs", False)}
    assert lines == {(f, m): RF.LINES[f] for f in RF.FAMILIES for m in RF.MODES[f]} and records == RF.RECORDS
    assert below == 16


def test_the_cases_reach_what_the_device_test_relies_on():
    """Asserted, not printed, each as a count of lines above a floor (the model's count at SEED in brackets)."""
    n = collections.Counter()
    for family in RF.FAMILIES:
        for s, p, y, idx, pens, k, (radius, sweeps, glyphs), res, notes, what in every_line(family, RF.IDS[family]):
            pre = "reading: " if what == "reading" else ""
            x, _, width, lh, _ = s.geo
            H, Wp = s.pages[p].shape
            w = min(width, Wp - min(x, Wp))
            f = s.fonts[k]
            if sweeps:
                n[pre + ("converged" if res.sweeps < sweeps else "at the cap")] += 1
                if res.sweeps < sweeps and np.any(np.diff(res.pens.astype(np.int64)) < 0):
                    n["converged with decreasing output pens"] += 1
            for note in RF.NOTES:
                n[pre + note] += notes[note] > 0
            for on, name in ((res.changed > 0, "changed"), (radius and sweeps and len(pens) and pens[0] == 0, "a character at pen 0 with a radius"),
                             (w == 0 or y >= H, "an empty crop"), (w == 1 and y < H, "a one-column crop"), (0 < w < width, "a crop cut at the right"),
                             (0 < H - y < lh, "a crop cut at the bottom"), (f.hinting, "a hinted font"), (f.text_size == 6.0, "size 6"),
                             (f.text_size == 24.0, "size 24"), (k >= 2, "a candidate font k >= 2"), (pens and pens[-1] >= 64 * max(w, 1), "a glyph wholly right of the crop")):
                n[pre + name] += bool(on)
    for family in RF.FAMILIES:
        for i in RF.IDS[family]:
            for p in range(len(TF.setup(family, i).pages)):
                recs = RF.reading(family, i, p).recs
                spans = [(first, first + m) for _, first, m, _ in recs]
                n["a repeated line"] += len(set(recs)) < len(recs)
                n["two lines sharing characters"] += any(a[0] < b[1] and b[0] < a[1] and recs[u] != recs[v] for u, a in enumerate(spans) for v, b in enumerate(spans) if u < v)
    # the model's counts at SEED, of 1796 fed-back lines: converged 435, at the cap 1066, changed 1128, late 25, glyph 342, pen 1067,
    # tie_rank 130, tie_glyph 39, tie_inc 74, neg_pen 952, pen 0 with a radius 891, cut at the right 669, at the bottom 542, hinted 842,
    # size 6 277, size 24 335, k >= 2 173, one column 14; of 313 records: converged 91, at the cap 154, glyph 154, pen 129,
    # tie_rank 54, tie_glyph 27, tie_inc 91, neg_pen 88, empty crops 12, one column 5, k >= 2 70, wholly right of the crop 157;
    # of the readings 60 repeat a line and 55 share characters; no converged line's output pens decrease
    floors = {"converged": 200, "at the cap": 500, "changed": 500, "late": 10, "glyph": 150, "pen": 500, "tie_rank": 50, "tie_glyph": 15, "tie_inc": 30,
              "neg_pen": 400, "a character at pen 0 with a radius": 100, "a crop cut at the right": 100, "a crop cut at the bottom": 100, "a hinted font": 200,
              "size 6": 20, "size 24": 20, "a candidate font k >= 2": 50, "a one-column crop": 5,
              "reading: converged": 40, "reading: at the cap": 70, "reading: glyph": 70, "reading: pen": 60, "reading: tie_rank": 25, "reading: tie_glyph": 10,
              "reading: tie_inc": 40, "reading: neg_pen": 40, "reading: an empty crop": 10, "reading: a one-column crop": 1, "reading: a candidate font k >= 2": 20,
              "reading: a glyph wholly right of the crop": 50, "a repeated line": 20, "two lines sharing characters": 40}
    short = {k: (n[k], v) for k, v in floors.items() if n[k] < v}
    assert not short, (short, dict(n))
    # the one omission the device module is allowed (feeding a converged line's output back needs pens that do not decrease):
    assert n["converged with decreasing output pens"] * 2 < n["converged"] + n["reading: converged"]


_short = []


def short_lines():
    """Six seeded lines cut to five characters, across the families: a hinted font, 24 px, a kerning off 1, and three lines of font
    searches (one in a candidate font)."""
    def first(family, mode, ok):
        for i in RF.IDS[family]:
            s = TF.setup(family, i, mode)
            got = TF.model_run(s)
            pens = RF.pens_of(s, got)
            for p, pg in enumerate(got["lines"]):
                for q, (y, text) in enumerate(pg):
                    k = got["fonts"][p][q] if "fonts" in got else 0
                    if len(text) >= 3 and s.geo[3] >= 4 and ok(s, s.fonts[k], k):
                        return s, p, y, [s.alphabet.index(c) for c in text[:5]], pens[p][q][:5], k
        raise AssertionError((family, mode))
    if _short:
        return _short
    _short.extend([first("cases", "plain", lambda s, f, k: f.hinting), first("cases", "slack", lambda s, f, k: f.text_size == 24.0 and len(s.alphabet) <= 6),
            first("cases", "search", lambda s, f, k: float(f.kerning) != 1.0 and not f.hinting), first("fonts", "pen", lambda s, f, k: k >= 1),
            first("fonts", "whole", lambda s, f, k: k == 0), first("fonts", "whole", lambda s, f, k: k >= 1 and f.hinting)])
    return _short


@pytest.mark.parametrize("n", range(6))
def test_the_model_is_the_brute_force_on_seeded_lines(n):
    """R.brute (one FreeType raster per candidate, the canvas composed anew from rasters) == R.refine_crop over the phase tables."""
    s, p, y, idx, pens, k = short_lines()[n]
    x, _, width, lh, _ = s.geo
    fm, ref = RF.models(s)[k], crop(s.pages[p], x, y, width, lh)
    radius, sweeps = (2, 2) if n % 2 == 0 else (1, 2)
    want = R.brute(fm, ref, idx, pens, radius, sweeps, n != 3)
    assert same(R.refine_crop(fm, ref, idx, pens, radius, sweeps, n != 3), want), (s.name, p, y)

"""tests/focr_line_frac_model.py: the integers of the fractional line grid at their edges, what the grid is for (pages whose
leading is not a whole number of pixels, which the two baseline modes lose after a few lines on the whole-pixel grid and
read to the end on the fractional one), its scores against FreeType, and proof that the cases of
tests/focr_line_frac_cases.py, which tests/test_gpu_focr_line_frac.py runs on the device, reach what their names say.
No GPU."""
import functools

import numpy as np
import pytest

import focr_baseline_model as B
import focr_line_frac_cases as K
import focr_line_frac_model as LF
import focr_whole_baseline_model as WB
from focr_fast_model import F32

B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/="


@functools.lru_cache(maxsize=None)
def model(font, size, alphabet, y_bits):
    return B.BaselineModel(font, size, alphabet, y_bits=y_bits)


def test_centre_at_its_edges():
    """c = ((f << B) + 32) >> 6, halves up: it reaches 2^B, one whole row, from f = 64 - (32 >> B) on, that is from 60 at
    B = 3, 56 at B = 2 and 32 at B = 0; it is 0 with f != 0 below 32 >> B (and always for f < 4 at B = 3)."""
    assert [LF.centre(f, 3) for f in (0, 3, 4, 59, 60, 63)] == [0, 0, 1, 7, 8, 8]
    assert [LF.centre(f, 2) for f in (0, 7, 8, 55, 56, 63)] == [0, 0, 1, 3, 4, 4]
    assert [LF.centre(f, 1) for f in (0, 15, 16, 47, 48, 63)] == [0, 0, 1, 1, 2, 2]
    assert [LF.centre(f, 0) for f in (0, 31, 32, 63)] == [0, 0, 1, 1]
    for y_bits in range(4):
        cs = [LF.centre(f, y_bits) for f in range(64)]
        assert cs == sorted(cs) and cs[0] == 0 and cs[-1] == 1 << y_bits
        assert all(abs(c / (1 << y_bits) - f / 64) <= 0.5 / (1 << y_bits) for f, c in enumerate(cs))  # the nearest step
        assert LF.candidates(cs[-1], 2) == [cs[-1] + o for o in (0, -1, 1, -2, 2)]
    # the widest returned q: -32 ..= 2^B + 32 <= 40 fits an int8
    assert min(LF.candidates(0, 32)) == -32 and max(LF.candidates(8, 32)) == 40 < 128


def test_slots_at_the_page_edges():
    """The slot whose crop row is the page's last row, and the next one, which does not exist; a last slot the page cuts; the
    closed form of the slot count against a walk of the grid; (0, 0) is the whole-pixel grid."""
    # Y_i = 64 * 3 + 20 + i * 998: slot 7 has Y = 7198, row 112; a page of 113 rows keeps it with one row, one of 112 does not
    s7 = LF.slot(7, 113, 3, 20, 14, 15, 38)
    assert (s7.Y, s7.yc, s7.h, s7.f) == (7198, 112, 1, 30)
    assert len(LF.slots(113, 3, 20, 14, 15, 38)) == 8 == LF.n_slots(113, 3, 20, 14, 15, 38)
    assert len(LF.slots(112, 3, 20, 14, 15, 38)) == 7 == LF.n_slots(112, 3, 20, 14, 15, 38)
    s8 = LF.slot(8, 113, 3, 20, 14, 15, 38)  # clamped as image::crop_imm clamps it: an empty crop
    assert (s8.yc, s8.h) == (113, 0)
    cut = LF.slots(120, 3, 20, 14, 15, 38)[-1]
    assert (cut.i, cut.yc, cut.h) == (7, 112, 8)
    # a crop row that the fraction alone pushes onto / off the page: Y_0 = 64 * 9 + 63 is still row 9
    assert LF.n_slots(10, 9, 63, 4, 1, 1) == 1 and [s.yc for s in LF.slots(10, 9, 63, 4, 1, 1)] == [9]
    assert LF.n_slots(10, 10, 0, 4, 1, 1) == 0 and LF.n_slots(10, 0, 0, 0, 1, 1) == 0
    rng = np.random.default_rng(0)
    for _ in range(300):
        H, y, yf, lh, la, af = (int(v) for v in (rng.integers(1, 200), rng.integers(0, 210), rng.integers(0, 64), rng.integers(1, 20),
                                                 rng.integers(1, 40), rng.integers(0, 64)))
        sl = LF.slots(H, y, yf, lh, la, af)
        assert len(sl) == LF.n_slots(H, y, yf, lh, la, af)
        assert all(s.yc < H and 1 <= s.h <= lh and s.yc + s.h <= H and 64 * s.yc + s.f == s.Y for s in sl)
        if (yf, af) == (0, 0) or rng.integers(0, 4) == 0:
            whole = LF.slots(H, y, 0, lh, la, 0)
            assert [(s.yc, s.f) for s in whole] == [(y + i * la, 0) for i in range(-(-(H - y) // la) if y < H else 0)]


def _drift_page(advance_frac):
    rng = np.random.default_rng(13)
    texts = ["".join(B64[k] for k in rng.integers(0, 64, 14)) for _ in range(14)]
    H = 3 + 16 + int(14 * (15 + advance_frac / 64)) + 4
    return texts, LF.draw_page(np.full((H, 112), 255, dtype=np.uint8), K.MONO, 13.0, B64, texts, 0, 3, 20, 15, advance_frac)


@pytest.mark.parametrize("advance_frac,whole_pixel_reads", [(38, 4), (54, 3)], ids=["998/64", "1014/64"])
def test_mono_page_with_a_fractional_leading(advance_frac, whole_pixel_reads):
    """DejaVu Sans Mono 13 px, the 65-character base64 alphabet, 14 lines of 14 random characters in 16-row crops, the first
    line's top at 3 + 20/64 px, a leading of 998/64 (15.594) and 1014/64 (15.844) px, B = 2.  On the whole-pixel grid
    (line_advance 15) the baseline search at N = 8 reads 4 and 3 of the 14 lines: the drift eats the radius, q saturates
    at +-8.  On the fractional grid it reads all 14 at N = 1, and N = 2 changes nothing; every chosen q lies within one
    step of its line's centre."""
    m = model(K.MONO, 13.0, B64, 2)
    texts, page = _drift_page(advance_frac)
    whole = m.search_image(page, 0, 3, 112, 16, 15, 8)
    assert sum(b.text[:14] == t for (_, b), t in zip(whole, texts)) == whole_pixel_reads
    assert sum(abs(b.q) == 8 for _, b in whole) >= 5
    slots = LF.slots(page.shape[0], 3, 20, 16, 15, advance_frac)[:14]
    found = LF.search_image(m, page, 0, 3, 112, 16, 15, 1, 20, advance_frac)
    assert [y for y, _ in found] == [s.yc for s in slots] != [3 + 15 * i for i in range(14)]
    assert [b.text[:14] for _, b in found] == texts
    assert all(abs(b.q - LF.centre(s.f, 2)) <= 1 for (_, b), s in zip(found, slots))
    wider = LF.search_image(m, page, 0, 3, 112, 16, 15, 2, 20, advance_frac)
    assert [(y, b.text, b.q) for y, b in wider] == [(y, b.text, b.q) for y, b in found]
    # y + q * 2^-B stays the line's true top, to the nearest step
    assert all(abs(64 * y + 16 * b.q - s.Y) <= 16 + 8 for (y, b), s in zip(found, slots))


SANS_AL, SANS_TEXT = " burnclipfHv", "burn clip ffH vvill rnrn cl"


def test_sans_page_under_whole_line_candidates():
    """DejaVu Sans 13 px, three lines of `burn clip ffH vvill rnrn cl` cropped to 150 columns (the crop cuts the final l), the
    leading 998/64 px, B = 2.  The whole-line decode under candidates reads every line at N = 1 on the fractional grid; on
    the whole-pixel grid at N = 2 the third line, 1.5 px off its crop, is already lost."""
    m = model(K.SANS, 13.0, SANS_AL, 2)
    frac = (20, 38)
    page = K.grid_page(K.SANS, 13.0, SANS_AL, 3 + 2 * 16 + 14, 150, [SANS_TEXT] * 3, 0, 3, frac, 15)
    found = LF.search_image(m, page, 0, 3, 150, 14, 15, 1, *frac, whole=True)
    assert [(y, b.q, b.text) for y, b in found] == [(3, 1, SANS_TEXT[:-1]), (18, 4, SANS_TEXT[:-1]), (34, 2, SANS_TEXT[:-1])]
    assert [b.q for _, b in found] == [LF.centre(s.f, 2) for s in LF.slots(page.shape[0], 3, 20, 14, 15, 38)]
    whole = WB.search_image(m, page, 0, 3, 150, 14, 15, 2)
    assert [y for y, _ in whole] == [3, 18, 33]
    assert [b.text == SANS_TEXT[:-1] for _, b in whole] == [True, True, False] and whole[2][1].q == 2  # saturated


@pytest.mark.parametrize("y_bits", [2, 3])
def test_scores_beyond_one_row_equal_one_raster_per_candidate(y_bits):
    """A centre of 2^B and an offset above it give q > 2^B: one score per y-phase, q = 2^B + 1 ..= 2^(B + 1), each against
    one FreeType raster per glyph at ty_q itself."""
    al = K.MONO_AL
    m = model(K.MONO, 13.0, al, y_bits)
    r = np.random.default_rng(y_bits).integers(0, 256, (14, 40)).astype(np.int64)
    qs = list(range((1 << y_bits) + 1, (2 << y_bits) + 1))
    assert {q & ((1 << y_bits) - 1) for q in qs} == set(range(1 << y_bits)) and min(qs) > 1 << y_bits
    for q in qs:
        for pos in (F32(0), F32(17.3)):
            assert np.array_equal(m.scores_q(r, pos, q), B.brute_scores(K.MONO, 13.0, al, r, F32(m.ox + pos), m.ty(q))), (q, pos)


def test_a_dropped_candidate_beside_a_centre():
    """The 6 px font whose origin_y is 5, B = 0, N = 8: around the centre 1 the offsets -7 and -8 give q < -5 and are dropped,
    around the centre 0 the offsets -6 to -8; the line drawn 3 px above its slot takes q = -2, the lowest (cost, rank) over
    the candidates that remain."""
    for whole in (False, True):
        c = K.dropped_case(whole)
        m = K.model(c.font, c.size, c.alphabet, c.y_bits)
        assert float(m.oy) == 5.0 and (c.y_bits, c.n) == (0, 8)
        slots = LF.slots(c.pages[0].shape[0], c.geo[1], c.frac[0], c.geo[3], c.geo[4], c.frac[1])
        assert [LF.centre(s.f, 0) for s in slots[:3]] == [0, 1, 0] and [s.f for s in slots[:3]] == [20, 44, 4]
        assert [q for q in LF.candidates(1, 8) if m.dropped(q)] == [-6, -7] and [q for q in LF.candidates(0, 8) if m.dropped(q)] == [-6, -7, -8]
        (_, a), (y, b), (_, d) = K.expected(c)[0]
        assert (y, b.q) == (12, -2) and a.q == 0 and d.q == 0 and [r.text[:4] for r in (b, d)] == ["baAB", "ABab"]
        line = c.pages[0][12:24, :40]
        one = (lambda q: WB.whole_line_q(m, line, q).cost) if whole else (lambda q: m.decode_line_q(line, q)[1])
        best = min((one(q), rank, q) for rank, q in enumerate(LF.candidates(1, 8)) if not m.dropped(q))
        assert (b.cost, b.q) == (best[0], best[2])


def _slots(c, page):
    return LF.slots(page.shape[0], c.geo[1], c.frac[0], c.geo[3], c.geo[4], c.frac[1])


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
@pytest.mark.parametrize("y_bits", [0, 2, 3])
def test_standard_cases_reach_their_edges(whole, y_bits):
    """The standard grid at N = 1: a centre of 2^B (slot 0, f = 60), crop rows off the whole-pixel grid, a blank slot between
    inked ones, and for the baseline search's page a last slot that the page cuts to 8 rows; the model reads every inked
    line at its centre or one step beside it."""
    c = K.std_case(whole, y_bits, 1)
    for p, (page, found) in enumerate(zip(c.pages, K.expected(c))):
        slots = _slots(c, page)
        assert slots[0].f == 60 and LF.centre(60, y_bits) == 1 << y_bits and found[0][1].q >= (1 << y_bits) - 1
        assert [s.yc for s in slots[:4]] == [3, 19, 35, 50] != [3, 18, 33, 48]
        inked = [y for y, _ in found]
        blank = [s.yc for s in slots if s.yc not in inked]
        assert blank[0] in ((19,) if whole else (50,)) and min(inked) < blank[0] < max(inked)
        by_row = {s.yc: s for s in slots}
        assert all(abs(b.q - LF.centre(by_row[y].f, y_bits)) <= 1 for y, b in found)
        if not whole:
            assert (slots[-1].yc, slots[-1].h) == (128, 8) and inked[-1] == 128 and len(slots) == 9 == LF.n_slots(136, 3, 60, 14, 15, 38)
            assert [b.text[:11] for _, b in found] == [t for t in K._texts(c.alphabet, 9, 11, 7 + y_bits + 1 + p, blank=(3,)) if t]


def test_named_cases_reach_what_they_name():
    """advance-one: many slots per tile row; moved-off-page: canvases moved above row 0 and past the last row; wide: a strip
    past LDS; two-sizes: grids of different slot counts in one call."""
    c = K.advance_one_case()
    slots = _slots(c, c.pages[0])
    assert c.geo[4] == 1 and c.frac[1] and c.geo[3] == 12 and len(slots) == 34 and sum(s.yc < 16 for s in slots) == 12
    assert len(K.expected(c)[0]) > 20 and len({s.f for s in slots}) > 20
    for whole in (False, True):
        c = K.moved_off_page_case(whole)
        found = K.expected(c)[0]
        H = c.pages[0].shape[0]
        assert (found[0][0], B.row_shift(found[0][1].q, 0)) == (0, -3) and c.y_bits == 0
        y, last = found[-1]
        assert B.row_shift(last.q, 0) == 3 and y + 3 + 13 > H and _slots(c, c.pages[0])[-1].h < c.geo[3]
        c = K.wide_case(whole)
        assert K.strip_bytes(c.pages[0].shape[1], c.geo[0], c.geo[2], c.geo[3]) > 65536 and len(c.pages) == 1
        assert len(K.expected(c)[0]) >= 1 and any(s.f for s in _slots(c, c.pages[0]))
        c = K.two_sizes_case(whole)
        assert len({p.shape for p in c.pages}) == 2 and len({len(_slots(c, p)) for p in c.pages}) == 2


def test_far_below_reaches_the_largest_q():
    """far-below: the centre 2^B = 1 and the offset +32 give q = 33 = 2^B + FOCR_BASELINE_MAX at B = 0, and the verify draws
    the canvas FOCR_BASELINE_MAX + 1 = 33 rows below its slot; at one y of the sweep its last row is row 0 of a 16-row tile,
    so only the full lower reach of the moved compose finds the slot from that tile."""
    from font_ocr_amd import VerifyFont
    vf = VerifyFont(K.MONO, 13.0, K.MONO_AL)
    last = []
    for y in range(16):
        c = K.far_below_case(y)
        m = K.model(c.font, c.size, c.alphabet, 0)
        (yc, b), = K.expected(c)[0]
        s = _slots(c, c.pages[0])[0]  # (a second slot, four blank rows at the page's end, follows)
        assert (yc, s.f, LF.centre(s.f, 0), b.q, B.row_shift(b.q, 0)) == (y, 40, 1, 33, 33) and b.text[:6] == "Ab01+a"
        img, _ = LF.verify_image(c.pages[0], [(yc, b)], m.font, vf, c.geo[0], 0)
        rows = np.nonzero(img[..., 2].any(axis=1))[0]
        assert rows.min() >= y + 33
        last.append(int(rows.max()))
    assert sum(r % 16 == 0 for r in last) == 1
    vf.close()


def test_cases_at_zero_fraction_reach_their_edges():
    """K.off(case), the hand-built cases at (0, 0) on their own pages, which tests/test_gpu_focr_line_frac.py's
    *_at_zero_fraction tests run: the expectation is the two whole-pixel models' (not the fractional model at (0, 0), which is
    compared with it here), every case has a non-blank line and a line whose winning q is not 0, and each edge is still reached."""
    from font_ocr_amd import VerifyFont

    def held(c):
        want = K.expected(c)
        m = K.model(c.font, c.size, c.alphabet, c.y_bits)
        frac = [LF.search_image(m, p, *c.geo, c.n, 0, 0, whole=c.whole) for p in c.pages]
        assert c.frac == (0, 0) and [[(y, r.text, r.q, r.cost) for y, r in pg] for pg in want] == [[(y, r.text, r.q, r.cost) for y, r in pg] for pg in frac]
        assert all((y - c.geo[1]) % c.geo[4] == 0 for pg in want for y, _ in pg)  # the rows y_start + i * line_advance
        assert sum(len(pg) for pg in want) >= 1 and any(r.q != 0 for pg in want for _, r in pg), c.name
        return want

    c = K.off(K.advance_one_case())
    found = held(c)[0]
    assert len(found) > 20 and sum(y < 16 for y, _ in found) >= 10  # many slots per tile row
    for whole in (False, True):
        c = K.off(K.moved_off_page_case(whole))
        found = held(c)[0]
        y, last = found[-1]
        assert (found[0][0], found[0][1].q, last.q) == (0, -3, 4) and y + 4 + 13 > c.pages[0].shape[0]
        c = K.off(K.wide_case(whole))
        assert K.strip_bytes(c.pages[0].shape[1], c.geo[0], c.geo[2], c.geo[3]) > 65536 and held(c)
        c = K.std_case(whole, 2, 1)
        want = held(K.off(c._replace(pages=K.std_pages(whole, 31, 2))))
        assert len(want) == 2 and all(len(pg) >= 2 for pg in want) and {r.q for pg in want for _, r in pg} <= {-1, 0, 1}
    vf = VerifyFont(K.MONO, 13.0, K.MONO_AL)
    last = []
    for y in range(16):  # the largest q of the whole-pixel grid, FOCR_BASELINE_MAX = 32, and a canvas whose last row opens a tile once
        c = K.off(K.far_below_case(y))
        (yc, b), = held(c)[0]
        assert (yc, b.q, B.row_shift(b.q, 0)) == (y, 32, 32)
        img, _ = LF.verify_image(c.pages[0], [(yc, b)], K.model(c.font, c.size, c.alphabet, 0).font, vf, c.geo[0], 0)
        last.append(int(np.nonzero(img[..., 2].any(axis=1))[0].max()))
    assert sum(r % 16 == 0 for r in last) == 1
    vf.close()


def test_verify_model_takes_the_crop_row_and_the_absolute_q():
    """The verify of a fractional run is the baseline run's with (yc_i, text, q): with the centre 2^B of slot 0 the canvas is
    drawn one row below the crop row, where the line's top (f = 60) is nearest."""
    from font_ocr_amd import VerifyFont
    c = K.std_case(False, 2, 1)
    m = K.model(c.font, c.size, c.alphabet, 2)
    found = K.expected(c)[0]
    assert found[0][1].q == 4 and B.row_shift(4, 2) == 1
    vf = VerifyFont(c.font, c.size, c.alphabet)
    img, sq = LF.verify_image(c.pages[0], found, m.font, vf, c.geo[0], 2)
    flat, sq0 = B.verify_image(c.pages[0], [(y, b.text, 0) for y, b in found], m.font, vf, c.geo[0], 2)
    assert sq < sq0 and not np.array_equal(img, flat)
    vf.close()


def test_the_seeded_fractions_are_what_they_promise():
    """fuzz_frac is a function of its arguments, stays in 0 .. 63, is never (0, 0), and over many indices draws y_frac = 63
    and advance_frac = 0 about one time in four each."""
    draws = [K.fuzz_frac(w, i) for w in (False, True) for i in range(400)]
    assert draws == [K.fuzz_frac(w, i) for w in (False, True) for i in range(400)]
    assert all(0 <= a <= 63 and 0 <= b <= 63 and (a, b) != (0, 0) for a, b in draws)
    assert 0.2 < sum(a == 63 for a, _ in draws) / 800 < 0.32 and 0.2 < sum(b == 0 for _, b in draws) / 800 < 0.32
    assert all(LF.centre(63, y_bits) == 1 << y_bits for y_bits in range(4))


def test_fuzz_cases_reach_their_edges():
    """What the seeded cases of tests/test_gpu_focr_line_frac.py::test_fuzz_cases reach on their seeded fractions, each
    property asserted by name.  The fractional grid lies between two whole-pixel grids: (y_start, line_advance), whose rows
    it never passes, so that a page has at most as many slots as on that one, and the next one down, (y_start + 1 where
    y_frac > 0, line_advance + 1 where advance_frac > 0), on which a page has at most as many slots as on the fractional
    one.  "Fewer" is against the first and "more" against the second."""
    reach = {}

    def note(name, who, hit):
        reach.setdefault(name, [])
        if hit:
            reach[name].append(who)

    for whole in (False, True):
        for i in K.FUZZ_IDS:
            c = K.fuzz_case(whole, i)
            m, top = K.fuzz_model(c), 1 << c.y_bits
            x, y, width, lh, adv = c.geo
            for page, found in zip(c.pages, K.fuzz_expected(c)):
                H = page.shape[0]
                slots = _slots(c, page)
                by_row = {s.yc: s for s in slots}
                assert len(by_row) == len(slots) or adv == 1
                below = LF.slots(H, y, 0, lh, adv, 0)
                above = LF.slots(H, y + (c.frac[0] > 0), 0, lh, adv + (c.frac[1] > 0), 0)
                assert len(above) <= len(slots) <= len(below), c.name
                note("a page with fewer slots than the whole-pixel grid above it", c.name, len(slots) < len(below))
                note("a page with more slots than the whole-pixel grid below it", c.name, len(slots) > len(above))
                for yc, r in found:
                    s = by_row[yc]
                    ci = LF.centre(s.f, c.y_bits)
                    assert 0 <= ci <= top and not m.dropped(r.q) and abs(r.q - ci) <= c.n, (c.name, yc)
                    note("a crop row off the whole-pixel grid", c.name, yc != y + s.i * adv)
                    note("a centre of 0", c.name, ci == 0)
                    note("a centre of 2^B", c.name, ci == top)
                    note("a centre strictly between", c.name, 0 < ci < top)
                    note("a centre that only the half rounds up", c.name, ((s.f << c.y_bits) & 63) == 32)
                    note("a winning q below its centre", c.name, r.q < ci)
                    note("a winning q at its centre", c.name, r.q == ci)
                    note("a winning q above its centre", c.name, r.q > ci)
                    note("a dropped candidate beside a kept winner", c.name, any(m.dropped(q) for q in LF.candidates(ci, c.n)))
                    note("a cut last slot with ink", c.name, s is slots[-1] and s.h < lh)
            note("hinting on", c.name, c.hinting)
            note("kerning off 1", c.name, c.kerning != 1.0)
            note("y_frac 63", c.name, c.frac[0] == 63)
            note("advance_frac 0", c.name, c.frac[1] == 0)
    print({k: len(v) for k, v in reach.items()})
    for name, hits in reach.items():
        assert hits, "no case reaches: " + name
    for form in ("base", "whole"):  # the centres and the winners in both forms (the slot count is the shared prepass's)
        for name, hits in reach.items():
            assert "page with" in name or [h for h in hits if h.startswith(form)], (form, name)
    # the seeded cases cannot drop a candidate (an origin_y of 5 px or more, a radius of 1.5 px at most): the low-origin case does
    assert reach["a dropped candidate beside a kept winner"] == ["base-low", "base-low", "whole-low", "whole-low"]

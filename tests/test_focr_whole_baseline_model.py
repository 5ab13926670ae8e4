"""tests/focr_whole_baseline_model.py against FreeType, and what the mode is for.  The model's term_q comes from y-phase
v = q & (2^B - 1) of the font moved by d = q >> B rows at pos = s / 64; here it is compared with one focr_raster_glyph per
glyph at (origin_x + s / 64, ty_q) itself.  Then the line of DejaVu Sans and Serif 13 px that neither the baseline search
nor the whole-line decode reads is pinned: the programme under every candidate takes the true offset and reads it, where
the greedy search takes a wrong offset in four of the eight cases.  No GPU."""
import functools
import os
import string

import numpy as np
import pytest

import focr_baseline_model as B
import focr_whole_baseline_model as WB
import focr_whole_model as WM

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
SERIF = os.path.join(GOLD, "DejaVuSerif.ttf")
AL65 = " " + string.ascii_lowercase + string.ascii_uppercase + string.digits + "+/"
TEXT = "burn clip ffH vvill rnrn cl"


@functools.lru_cache(maxsize=None)
def model(font, alphabet, y_bits):
    return B.BaselineModel(font, 13.0, alphabet, y_bits=y_bits)


@pytest.mark.parametrize("y_bits", [1, 2])
def test_term_q_equals_one_raster_per_candidate(y_bits):
    """Every glyph's term under candidates on both sides of 0, at states with several x phases and a clipped last glyph,
    on a short Sans noise line: term_q(i, s) is the full-canvas SSD of one FreeType raster at (origin_x + s / 64, ty_q)
    less the canvas's sum of r^2."""
    al = "burn clipfH"
    m = model(SANS, al, y_bits)
    r = np.random.default_rng(40 + y_bits).integers(0, 256, (16, 44)).astype(np.int64)
    total = int((r * r).sum())
    for q in (-(3 << y_bits) - 1, -3, -1, 0, 1, 2, (2 << y_bits) + 1):
        term = WB.term_q(q)
        for s in (0, 501, 64 * 41 + 19):
            want = B.brute_scores(SANS, 13.0, al, r, F32(m.ox + F32(s) / F32(64)), m.ty(q)) - total
            assert np.array_equal(term(m, r, total, s), want), (q, s)
    assert np.array_equal(WB.term_q(0)(m, r, total, 777), WM.term_from_scores(m, r, total, 777))  # candidate 0 is the plain term


# font, offset in px, the radius that still holds the true q, the greedy search's (q, text) at N = 8, the whole-line text
# and cost at q = 0, and the programme under every candidate: q, text, cost
TABLE = [
    (SANS, 1.0, 4, (4, "bunY dm+Tl vvillmmY+"), "hurn cllp ffH vvlll rnrn r", (4, "burn clip ffH vvill rnrn c", -15774179)),
    (SANS, -1.0, 4, (-2, "bunY dm+zf vvM mrn m"), "burn cllp ffH vvlll rnrn G", (-4, "burn clip ffH vvill rnrn c", -15304401)),
    (SANS, 0.75, 3, (6, "bunY dm 4H vvM mrn 4"), "burn clip ffH vvill rnrn c", (3, "burn clip ffH vvill rnrn c", -15149741)),
    (SANS, -2.0, 8, (-8, "bunT1Mi HH Vw47nm v"), "IAIt0 FllI/ RU Yxlll lTT I G", (-8, "burn clip ffH vvill rnrn c", -14826736)),
    (SERIF, 1.0, 4, (4, "bmxi Gm BH vvm Huzm"), "6urn clip /JH vvill rnrnJ", (4, "burn clip ffH vvill rnrn ", -16462938)),
    (SERIF, -1.0, 4, (-5, "mnT  Sm RH vvm HuzA"), "buru vlu/ lIH vvlll rur/u", (-4, "burn clip ffH vvill rnrn ", -15833625)),
    (SERIF, 0.75, 3, (4, "bmxi Gm BH vvm Huzn"), "burn clip ffH vvill rnrnJ", (3, "burn clip ffH vvill rnrn ", -16398083)),
    (SERIF, -2.0, 8, (-8, "mnT TEo3BT zGh31Tm"), "l80T   B0 lIU 7Ull DlDW", (-8, "burn clip ffH vvill rnrn ", -15242966)),
]


def _page(font, offset):
    page = np.full((16, 150), 255, dtype=np.uint8)
    return B.draw_offset(page, font, 13.0, AL65, TEXT, 0, 0, offset)


@pytest.mark.parametrize("font,offset,n,greedy,whole0,want", TABLE, ids=["%s%+g" % ("sans" if f == SANS else "serif", o) for f, o, *_ in TABLE])
def test_proportional_lines_off_the_baseline(font, offset, n, greedy, whole0, want):
    """DejaVu Sans and Serif 13 px, unhinted, the 65-glyph alphabet, `burn clip ffH vvill rnrn cl` on a 16 x 150 page (the
    crop cuts the final l), B = 2.  The programme under every candidate takes the true offset and reads the line; the
    whole-line decode at q = 0 misreads it unless the offset is small, and the greedy search at N = 8 loses the text.  Two
    rows search the full N = 8, the others a radius that still holds the true q."""
    m = model(font, AL65, 2)
    page = _page(font, offset)
    g = m.search_line(page, 8)
    assert (g.q, g.text) == greedy
    assert WB.whole_line_q(m, page, 0).text == whole0
    got = WB.search_line(m, page, n)
    assert (got.q, got.text, got.cost) == want and got.q == round(offset * 4) and abs(got.q) <= n
    assert got.text[:-1].rstrip() == TEXT[: len(got.text) - 1].rstrip() and len(got.text) >= 25


def test_the_greedy_search_picks_another_offset_in_four_rows():
    """So "let the greedy search pick q, then run the programme once" is not the definition: the programme's own cost
    has to choose."""
    wrong = [(f, o) for f, o, _, (gq, _), _, (q, _, _) in TABLE if gq != q]
    assert wrong == [(SANS, -1.0), (SANS, 0.75), (SERIF, -1.0), (SERIF, 0.75)]


def test_ties_take_the_offset_nearest_zero():
    """Ink out of every glyph's reach (the crop's last row only) and a space in the alphabet: every candidate's line costs
    the same, so q = 0 wins and the trail of improvements holds it alone."""
    m = B.BaselineModel(MONO, 13.0, " AB", y_bits=2)
    page = np.full((16, 40), 255, dtype=np.uint8)
    page[15, :] = 0
    assert {WB.whole_line_q(m, page, q).cost for q in range(-4, 5)} == {0}
    trail = []
    got = WB.search_line(m, page, 4, trail)
    assert got.q == 0 and got.cost == 0 and set(got.text) == {" "} and trail == [0]
    m.close()


def test_radius_zero_is_the_whole_line_decode():
    m = model(SANS, "burn clipfH", 2)
    page = np.full((16, 60), 255, dtype=np.uint8)
    B.draw_offset(page, SANS, 13.0, "burn clipfH", "burn clip", 0, 0, 0.5)
    got, plain = WB.search_line(m, page, 0), WM.whole_line(m, page)
    assert got.q == 0 and (got.text, got.cost) == (plain.text, plain.cost)
    assert np.array_equal(got.pens, plain.pens) and np.array_equal(got.idx, plain.idx)
    (y, b), = WB.search_image(m, page, 0, 0, 60, 16, 16, 0)
    assert y == 0 and b.text == plain.text


def test_dropped_candidates_and_the_verify_model():
    """A 6 px font's origin_y is 5: at B = 0 the candidates below -5 are dropped.  The verify model draws the line at its
    pens, row_shift(q) rows down."""
    from font_ocr_amd import VerifyFont
    al = " ABab"  # with a space: the blank rest of the crop costs nothing
    m = B.BaselineModel(MONO, 6.0, al, y_bits=0)
    page = np.full((12, 40), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 6.0, al, "AbBa", 0, 0, 2.0)
    trail = []
    got = WB.search_line(m, page, 32, trail)
    assert got.q == 2 and got.text.startswith("AbBa") and all(q >= -5 for q in trail)
    best = min((WB.whole_line_q(m, page, q).cost, B.rank(q), q) for q in range(-5, 33))
    assert (got.cost, got.q) == (best[0], best[2])
    vf = VerifyFont(MONO, 6.0, al)
    moved, sq = WB.verify_image(page, [(0, got.text, got.pens, got.q)], m.font, vf, 0, 0)
    unmoved, sq0 = WB.verify_image(page, [(0, got.text, got.pens, 0)], m.font, vf, 0, 0)
    assert np.array_equal(moved[2:, :, 2], unmoved[:-2, :, 2]) and sq < sq0
    vf.close()
    m.close()

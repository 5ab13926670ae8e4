"""The pages and geometries that tests/test_gpu_focr_line_frac.py runs on the device and that
tests/test_focr_line_frac_model.py proves, on the CPU model, to reach the cases their names promise.  Small on purpose:
pages of about 100 x 130 px, lines of 12 to 16 rows, alphabets of 4 to 12 glyphs (the whole-line programme on the CPU costs
0.3 s per candidate of a 100 px line of 11 glyphs), except where the case itself is a size (the strip past LDS).
Behind the hand-built cases: the seeded cases of the two baseline fuzzes on a seeded fraction (fuzz_frac, fuzz_case).
"""
import collections
import functools
import os

import numpy as np

import focr_baseline_model as B
import focr_line_frac_model as LF
import focr_whole_baseline_model as WB

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
MONO_AL = " ABab01+"      # the baseline search's: 8 glyphs, with a space, so that the blank rest of a line costs nothing
SANS_AL = " burnclip"     # the whole-line candidates': 9 glyphs of `burn clip`

# name, whole (the whole-line decode under candidates, else the baseline search), font, size, alphabet, B, N, pages,
# (x, y, width, line_height, line_advance), (y_frac, advance_frac)
Case = collections.namedtuple("Case", "name whole font size alphabet y_bits n pages geo frac")


@functools.lru_cache(maxsize=None)
def model(font, size, alphabet, y_bits):
    return B.BaselineModel(font, size, alphabet, y_bits=y_bits)


def _texts(alphabet, n_lines, n_chars, seed, blank=()):
    rng = np.random.default_rng(seed)
    ink = [c for c in alphabet if not c.isspace()]
    return [None if i in blank else "".join(rng.choice(ink, n_chars)) for i in range(n_lines)]


def grid_page(font, size, alphabet, H, W, texts, x, y, frac, line_advance, shift=None):
    """A white page with texts[i] on slot i of the grid; shift[i] px (a float, default 0) moves line i off its slot."""
    page = np.full((H, W), 255, dtype=np.uint8)
    for i, text in enumerate(texts):
        Y = 64 * y + frac[0] + i * LF.step(line_advance, frac[1])
        if text and (Y >> 6) < H:
            B.draw_offset(page, font, size, alphabet, text, x, Y >> 6, (Y & 63) / 64.0 + (shift[i] if shift else 0.0))
    return page


# The standard grid: y = 3 + 60/64 px and a leading of 15 + 38/64 px on a page of 136 rows.  Nine slots at rows 3, 19, 35,
# 50, 66, 81, 97, 113 and 128 (the whole-pixel grid's are 3, 18, 33, ...), with f = 60, 34, 8, 46, 20, 58, 32, 6, 44: slot 0
# has the centre 2^B at every B, slot 3 is left blank between inked ones, and the page cuts slot 8 to 8 rows.
STD_GEO, STD_FRAC, STD_H = (2, 3, 96, 14, 15), (60, 38), 136


def std_pages(whole, seed, n_pages=1):
    if whole:  # three lines of 58 columns: slots 0 and 2 inked, slot 1 blank, and nothing below
        return [grid_page(SANS, 13.0, SANS_AL, 60, 62, _texts(SANS_AL, 3, 7, seed + p, blank=(1,)), 2, 3, STD_FRAC, 15) for p in range(n_pages)]
    return [grid_page(MONO, 13.0, MONO_AL, STD_H, 100, _texts(MONO_AL, 9, 11, seed + p, blank=(3,)), 2, 3, STD_FRAC, 15) for p in range(n_pages)]


def std_case(whole, y_bits, n):
    if whole:
        return Case(f"std-whole-B{y_bits}-N{n}", True, SANS, 13.0, SANS_AL, y_bits, n, std_pages(True, 7 + y_bits + n), (2, 3, 58, 14, 15), STD_FRAC)
    return Case(f"std-base-B{y_bits}-N{n}", False, MONO, 13.0, MONO_AL, y_bits, n, std_pages(False, 7 + y_bits + n, 2), STD_GEO, STD_FRAC)


def dropped_case(whole):
    """A 6 px font's origin_y is 5: at B = 0 and N = 8 the candidates q < -5 are dropped, beside centres of 0 and 1; the middle line sits 3 px above its slot."""
    al = " ABab"
    geo, frac = (0, 0, 40, 12, 12), (20, 24)  # f = 20, 44, 4: centres 0, 1, 0
    page = grid_page(MONO, 6.0, al, 40, 44, ["AbBa", "baAB", "ABab"], 0, 0, frac, 12, shift=[0.0, -3.0, 0.0])
    return Case("dropped-" + ("whole" if whole else "base"), whole, MONO, 6.0, al, 0, 8, [page], geo, frac)


def advance_one_case():
    """line_advance 1 with a fraction under a line_height of 12: a slot every 1 + 21/64 rows, about twelve per tile row of
    the moved compose, two text lines among them."""
    frac = (5, 21)
    page = np.full((44, 100), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, MONO_AL, "Ab01+aB", 2, 4, 0.25)
    B.draw_offset(page, MONO, 13.0, MONO_AL, "+10bA", 2, 24, 0.75)
    return Case("advance-one", False, MONO, 13.0, MONO_AL, 2, 1, [page], (2, 0, 96, 12, 1), frac)


def moved_off_page_case(whole):
    """The first line sits 3 px above its slot at row 0 and the last one 3 px below a slot the page cuts: at B = 0, N = 4
    the verify moves the first canvas above row 0 and the last one past the page's last row."""
    al, font = (SANS_AL, SANS) if whole else (MONO_AL, MONO)
    frac, W = (0, 38), 62 if whole else 100
    texts = _texts(al, 3, 6 if whole else 11, 3)
    page = grid_page(font, 13.0, al, 42, W, texts, 2, 0, frac, 15, shift=[-3.0, 0.0, 3.0])
    return Case("moved-off-page-" + ("whole" if whole else "base"), whole, font, 13.0, al, 0, 4, [page], (2, 0, W - 4, 14, 15), frac)


def far_below_case(y):
    """The far end of the verify's lower reach: B = 0, N = 32, a slot of 48 rows at row y with f = 40, so the centre is 2^B = 1,
    and a line drawn 33 rows below the slot's top: q = 1 + 32 = 33, the largest q there is, and the canvas is moved 33 rows
    down.  Over y = 0 .. 15 the moved canvas's last row is the first row of a compose tile once."""
    page = np.full((y + 64, 60), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, MONO_AL, "Ab01+a", 2, y, 33.0)
    return Case(f"far-below-y{y}", False, MONO, 13.0, MONO_AL, 0, 32, [page], (2, y, 56, 48, 60), (40, 0))


def wide_case(whole):
    """One wide page whose strip does not fit in LDS: stride * line_height > 65536."""
    if whole:  # 128 rows of 512 columns, two glyphs: 32768 states per candidate on the CPU
        al, geo, frac = " l", (0, 2, 512, 128, 100), (50, 30)
        page = np.full((140, 512), 255, dtype=np.uint8)
        B.draw_offset(page, SANS, 13.0, al, "l ll l", 0, 2, 50 / 64.0)
        return Case("wide-whole", True, SANS, 13.0, al, 2, 1, [page], geo, frac)
    geo, frac = (0, 1, 4200, 16, 15), (40, 38)
    page = grid_page(MONO, 13.0, MONO_AL, 34, 4200, _texts(MONO_AL, 2, 60, 5), 0, 1, frac, 15)
    return Case("wide-base", False, MONO, 13.0, MONO_AL, 2, 1, [page], geo, frac)


def two_sizes_case(whole):
    """A batch of two page sizes through decode(): the second page is narrower and shorter, so its grid has fewer slots."""
    a, = std_pages(whole, 21)
    b = std_pages(whole, 22)[0][: (44 if whole else 90), : (50 if whole else 80)].copy()
    c = std_case(whole, 2, 1)
    return c._replace(name="two-sizes-" + ("whole" if whole else "base"), pages=[a, b, a.copy()])


# ---- the seeded cases of the two baseline fuzzes on a seeded fraction -------------------------------------------------------

FUZZ_SEED = 0x1F4C
N_FUZZ = 12  # of each form

# as Case, with the hinting and kerning the seeded cases bring
Fuzz = collections.namedtuple("Fuzz", "name whole font size hinting kerning alphabet y_bits n pages geo frac")


def fuzz_frac(whole, i):
    """(y_frac, advance_frac) of seeded case i of a form, a function of FUZZ_SEED, the form and i alone: each in 0 .. 63 and
    not both 0; y_frac is 63 in about one draw of four (the centre ((f << B) + 32) >> 6 then reaches 2^B at every B), and
    advance_frac is 0 in about one of four (every slot keeps slot 0's sub-pixel part)."""
    rng = np.random.default_rng([FUZZ_SEED, int(whole), i])
    while True:
        y_frac = 63 if rng.random() < 0.25 else int(rng.integers(0, 64))
        advance_frac = 0 if rng.random() < 0.25 else int(rng.integers(0, 64))
        if y_frac or advance_frac:
            return y_frac, advance_frac


FUZZ_IDS = tuple(range(N_FUZZ)) + ("low",)


def _low_case(whole):
    """The seeded cases' fonts have an origin_y of 5 px or more and their radius reaches 1.5 px at most, so none of them can
    drop a candidate.  This one can: the alphabet `.,_` has an origin_y of 1 px, and the radius reaches 2 px (N = 8 at B = 2,
    N = 4 at B = 1), so that q below -2^B is dropped around a low centre; the middle line sits 1 px above its slot.
    Hinted Serif at kerning 0.85 for the baseline search, Sans (origin_x 1) at kerning 1.07 for the whole-line candidates."""
    font, hinting, kerning, y_bits, n = (SANS, False, 1.07, 1, 4) if whole else (os.path.join(GOLD, "DejaVuSerif.ttf"), True, 0.85, 2, 8)
    al, size, geo, frac = ".,_", 7.15, (1, 2, 30, 6, 7), fuzz_frac(whole, N_FUZZ)
    texts = _texts(al, 3, 9, 17 + whole)
    page = np.full((2 + 2 * 7 + 12, 33), 255, dtype=np.uint8)
    for i, (text, shift) in enumerate(zip(texts, (0.0, -1.0, 0.25))):
        Y = 64 * geo[1] + frac[0] + i * LF.step(geo[4], frac[1])
        B.draw_offset(page, font, size, al, text, geo[0], Y >> 6, (Y & 63) / 64.0 + shift, hinting, kerning)
    H = ((64 * geo[1] + frac[0] + 2 * LF.step(geo[4], frac[1])) >> 6) + 4  # the page cuts the third slot to four rows
    return Fuzz("whole-low" if whole else "base-low", whole, font, size, hinting, kerning, al, y_bits, n, [page[:H].copy()], geo, frac)


def fuzz_case(whole, i):
    """Case i of tests/focr_fuzz_cases.py at B = 2, N = 4 (the baseline search), or of tests/focr_whole_baseline_fuzz.py at
    its own y_bits and n (the whole-line decode under candidates), on the grid of fuzz_frac(whole, i); "low" is _low_case."""
    if i == "low":
        return _low_case(whole)
    if whole:
        import focr_whole_baseline_fuzz as WF
        c = WF.case(i)
        return Fuzz(f"whole-{i}", True, c.font, c.size, c.hinting, c.kerning, c.alphabet, c.y_bits, c.n, [c.page], c.geo, fuzz_frac(True, i))
    import focr_fuzz_cases as FC
    c = FC.case(i)
    return Fuzz(f"base-{i}", False, c.font, c.size, c.hinting, c.kerning, c.alphabet, 2, 4, c.pages, c.geo, fuzz_frac(False, i))


@functools.lru_cache(maxsize=None)
def _fuzz_model(font, size, alphabet, hinting, kerning, y_bits):
    return B.BaselineModel(font, size, alphabet, hinting, kerning, y_bits)


def fuzz_model(c):
    return _fuzz_model(c.font, c.size, c.alphabet, c.hinting, c.kerning, c.y_bits)


_fuzz_expected = {}


def fuzz_expected(c):
    """expected() of a Fuzz case, with the model of its hinting and kerning; computed once."""
    if c.name not in _fuzz_expected:
        _fuzz_expected[c.name] = [LF.search_image(fuzz_model(c), p, *c.geo, c.n, *c.frac, whole=c.whole) for p in c.pages]
    return _fuzz_expected[c.name]


def strip_bytes(page_w, x, width, line_height):
    w = min(width, page_w - min(x, page_w))
    return ((w + 7) // 4 + 2) * 4 * line_height


def off(case):
    """The case at the fraction (0, 0), the whole-pixel grid, on the same pages: the baseline search's kernel and the
    verify's layout kernel are the same ones on both grids, so the edges the hand-built cases aim at are run on each.  The
    lines were drawn for the fractional grid, so they sit off these slots and the searches answer with q != 0."""
    return case._replace(name=case.name + "-off", frac=(0, 0))


def expected(case):
    """The model's [[(yc_i, Baseline or WholeBaseline)] per page] of a case: the fractional grid's model, or at (0, 0) the two
    whole-pixel baseline models' own walk of the page."""
    m = model(case.font, case.size, case.alphabet, case.y_bits)
    if tuple(case.frac) == (0, 0):
        if case.whole:
            return [WB.search_image(m, p, *case.geo, case.n) for p in case.pages]
        return [m.search_image(p, *case.geo, case.n) for p in case.pages]
    return [LF.search_image(m, p, *case.geo, case.n, *case.frac, whole=case.whole) for p in case.pages]

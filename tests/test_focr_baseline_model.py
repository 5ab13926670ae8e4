"""tests/focr_baseline_model.py against FreeType, and what the baseline search is for.  The model takes candidate q's
rendering from y-phase v = q & (2^B - 1) of the font moved by d = q >> B rows; here every score it gives is compared with
one focr_raster_glyph per glyph at the vertical translation ty_q itself.  Then the lines of DejaVu Sans Mono 13 px whose
baseline sits off the crop's are pinned: the plain loop loses them, the search finds the offset and the text.  No GPU."""
import functools
import os

import numpy as np
import pytest

import focr_baseline_model as B
from focr_fast_model import F32, FastModel

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
SERIF = os.path.join(GOLD, "DejaVuSerif.ttf")
B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/="
TEXT = "egw8CJ08PT3bR0QapjFB3w1i0"  # 25 characters: 195.7 px of Mono 13 px, so a 200 px line decodes one character more


@functools.lru_cache(maxsize=None)
def model(font, size, hinting, y_bits):
    return B.BaselineModel(font, size, B64, hinting=hinting, y_bits=y_bits)


def _noisy_line(seed, h=16, w=48):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.int64)


@pytest.mark.parametrize("y_bits", [0, 2, 3])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
@pytest.mark.parametrize("font,size", [(MONO, 13.0), (SANS, 13.0), (SERIF, 9.0)], ids=["mono", "sans", "serif"])
def test_scores_equal_one_raster_per_candidate(font, size, hinting, y_bits):
    """Every glyph's score under candidates on both sides of 0, at pens with several x phases and a clipped last glyph,
    on a 16-row noise line: the largest |q| push boxes past the crop's top and bottom rows."""
    m = model(font, size, hinting, y_bits)
    r = _noisy_line(int(size) + y_bits + hinting)
    n = 8 << y_bits  # up to 8 px either way
    qs = sorted({-n, -(5 << y_bits) - 1, -3, -1, 0, 1, 2, (1 << y_bits) + 1, (4 << y_bits) + 3, n})
    qs = [q for q in qs if not m.dropped(q)]  # Serif 9 px has origin_y 7: its candidates more than 7 px up do not exist
    assert sum(q < 0 for q in qs) >= 3 and sum(q > 0 for q in qs) >= 4
    for q in qs:
        for pos in (F32(0), F32(7.83), F32(41.3)):
            want = B.brute_scores(font, size, B64, r, F32(m.ox + pos), m.ty(q), hinting)
            assert np.array_equal(m.scores_q(r, pos, q), want), (q, pos)
    assert np.array_equal(m.scores_q(r, F32(3.5), 0), FastModel.scores(m, r, F32(3.5)))  # candidate 0 is the plain model


def test_dropped_candidates():
    """A 6 px font's origin_y is 5: at B = 0 the candidates below -5 have ty_q < 0 and are dropped, and the search's
    answer is the search over the rest."""
    m = B.BaselineModel(MONO, 6.0, B64, y_bits=0)
    assert float(m.oy) == 5.0 and not m.dropped(-5) and m.dropped(-6) and not m.dropped(32)
    page = np.full((12, 60), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 6.0, B64, "base64", 0, 0, 2.0)
    got = m.search_line(page, 32)
    assert got.q == 2 and got.text.startswith("base64")
    best = min(((m.decode_line_q(page, q)[1], B.rank(q), q) for q in range(-5, 33)))
    assert (got.cost, got.q) == (best[0], best[2])
    m.close()


@pytest.mark.parametrize("offset,q,plain_wrong", [(0.75, 3, 6), (1.0, 4, 13), (-1.0, -4, 17), (1.6, 6, 21), (-2.0, -8, 23)])
def test_mono_lines_off_the_baseline(offset, q, plain_wrong):
    """Mono 13 px, the 65-character base64 alphabet, a 25-character line of 16 x 200 px drawn `offset` px below the
    crop's baseline.  The plain pen loop loses `plain_wrong` of the 25 characters; the search at B = 2, N = 8 takes the
    true offset (1.5 px for 1.6) and reads the whole text, then one character past its end."""
    m = model(MONO, 13.0, False, 2)
    page = np.full((16, 200), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, B64, TEXT, 0, 0, offset)
    plain = m.decode_line(page)
    assert len(plain) == 26 and sum(a != b for a, b in zip(plain, TEXT)) == plain_wrong
    got = m.search_line(page, 8)
    assert got.q == q and got.text[:25] == TEXT and len(got.text) == 26
    assert got.cost == m.decode_line_q(page, q)[1] < m.decode_line_q(page, 0)[1]
    assert m.decode_line_q(page, 0)[0] == plain


def test_mono_long_line():
    m = model(MONO, 13.0, False, 2)
    text = TEXT + "VcyHTHd+IYZ5NgQBwDRffH+v9FuSi7RuKU+"
    page = np.full((16, 480), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, B64, text, 0, 0, 1.0)
    plain = m.decode_line(page)
    assert sum(a != b for a, b in zip(plain, text)) == 28
    got = m.search_line(page, 8)
    assert got.q == 4 and got.text[:60] == text


def test_sans_offset_found_text_lost():
    """Sans 13 px at +1 px: the search takes q = 4, the true offset, and the text is still lost, to the greedy loop:
    that is the whole-line decode's to cure, not this search's."""
    m = model(SANS, 13.0, False, 2)
    page = np.full((16, 200), 255, dtype=np.uint8)
    B.draw_offset(page, SANS, 13.0, B64, TEXT, 0, 0, 1.0)
    got = m.search_line(page, 8)
    assert got.q == 4 and got.cost == -23640810
    assert got.text != TEXT and len(got.text) == 24 and got.text[:2] == TEXT[:2]
    assert sum(a != b for a, b in zip(m.decode_line(page), TEXT)) == 21


def test_ties_take_the_offset_nearest_zero():
    """Ink out of every glyph's reach (the crop's last row only) and a space in the alphabet: every candidate's cost is
    the same, so q = 0 wins; rank orders 0, -1, +1, -2, ..."""
    assert B.candidates(2) == [0, -1, 1, -2, 2]
    m = B.BaselineModel(MONO, 13.0, " AB", y_bits=2)
    page = np.full((16, 40), 255, dtype=np.uint8)
    page[15, :] = 0  # below every glyph at every candidate within a pixel: a blank scores 0 everywhere
    costs = {q: m.decode_line_q(page, q)[1] for q in range(-4, 5)}
    assert set(costs.values()) == {0}
    got = m.search_line(page, 4)
    assert got.q == 0 and got.cost == 0 and set(got.text) == {" "}
    m.close()

"""The pen-search model (tests/focr_search_model.py) against brute force and against the pages it is for.  The model is
the definition of include/focr_decode.h on FastModel.scores; here it must equal a walk that rasterises every (glyph,
offset) candidate with FreeType at origin_x + p_j, and it must decode the lines the plain decoder loses: glyphs snapped
to the pixel grid, and an advance one percent larger than the font's.  No GPU needed."""
import os

import numpy as np
import pytest

import focr_search_model as S
from focr_fast_model import FastModel
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, VerifyFont
from font_ocr_amd.decoder import render_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")


def test_rank_orders_offsets_from_zero_outwards():
    assert [S.rank(j) for j in (0, -1, 1, -2, 2, -64, 64)] == [0, 1, 2, 3, 4, 127, 128]
    assert sorted(range(-5, 6), key=S.rank) == [0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5]


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("n", [1, 4])
def test_model_equals_brute_force(font, n):
    """A 12-character line drawn with its pens floored to whole pixels, so that the search has offsets to find: text,
    offsets, pens, scores and other-glyph runners equal one FreeType raster per candidate."""
    size, al = 13.0, FOCR_DEFAULT_ALPHABET
    rng = np.random.default_rng(11 + n)
    text = "".join(rng.choice(list(al), 12))
    page = np.full((16, 100), 255, dtype=np.uint8)
    S.draw_snapped(page, font, size, al, text, 0, 0, "floor")
    fm = FastModel(font, size, al)
    got, want = S.search_line(fm, page, n), S.brute_search_line(page, font, size, al, n)
    fm.close()
    assert got.text == want.text and len(got.text) >= 12
    for name in ("offsets", "pens", "score", "runner", "runner_score", "second_is_own"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert got.base == want.base
    assert np.any(got.offsets != 0) and np.all(np.abs(got.offsets) <= n)
    best = np.array([al.index(c) for c in got.text])
    assert np.all(got.runner != best) and np.all(got.runner_score >= got.score)


def test_radius_zero_is_the_plain_decoder():
    size, al = 13.0, FOCR_DEFAULT_ALPHABET
    page = np.full((16, 120), 255, dtype=np.uint8)
    S.draw_snapped(page, MONO, size, al, "Plain 0 decode", 0, 0, "round")
    fm = FastModel(MONO, size, al)
    got = S.search_line(fm, page, 0)
    assert got.text == fm.decode_line(page) and not got.offsets.any()
    fm.close()


def _wrong(got, want):
    return sum(a != b for a, b in zip(got[: len(want)], want)) + max(0, len(want) - len(got))


@pytest.fixture(scope="module")
def table():
    """One 640x16 line of 60 random characters of the default alphabet in Mono 13 px, drawn four ways, and the number of
    its characters decoded wrong by the plain walk and by searches of 8, 32 and 48 sixty-fourths."""
    size, al = 13.0, FOCR_DEFAULT_ALPHABET
    rng = np.random.default_rng(5)
    text = "".join(al[i] for i in rng.integers(0, len(al), 60))
    fm = FastModel(MONO, size, al)
    out = {}
    for name, snap, adv in (("exact", "exact", 1.0), ("round", "round", 1.0), ("floor", "floor", 1.0), ("advance", "exact", 1.01)):
        page = np.full((16, 640), 255, dtype=np.uint8)
        S.draw_snapped(page, MONO, size, al, text, 0, 0, snap, adv)
        out[name] = [_wrong(fm.decode_line(page), text)] + [_wrong(S.search_line(fm, page, n).text, text) for n in (8, 32, 48)]
    fm.close()
    return out


def test_accuracy_on_snapped_and_stretched_lines(table):
    """Wrong characters of 60: plain, then radius 8, 32, 48."""
    assert table["floor"][2] == 0      # floored pens: radius 32 decodes the whole line
    assert table["advance"][1] == 0    # advance 1 % too large: radius 8 decodes the whole line
    assert table["floor"][0] > 10 and table["advance"][0] > 10
    assert table == {"exact": [0, 0, 0, 0], "round": [1, 2, 1, 0], "floor": [18, 3, 0, 0], "advance": [48, 0, 0, 0]}


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
def test_verify_model_at_the_plain_pens_is_render(font):
    """compose_line_at with the running sum of the increments is render(): what pins the verify model of a searched run
    to the reference when no offset is taken."""
    size, al = 13.0, FOCR_DEFAULT_ALPHABET
    df, vf = DecodeFont(font, size, al), VerifyFont(font, size, al)
    rng = np.random.default_rng(2)
    for text in ["J", "jTY", "".join(rng.choice(list(al), 25)), "".join(rng.choice(list(al), 7))]:
        idx = [al.index(c) for c in text]
        assert np.array_equal(S.compose_line_at(df, vf, idx, S.plain_pens(df, idx)), render_text(font, size, text)), text
    df.close()
    vf.close()


def test_cap_and_radius_limits():
    """The largest radius a font takes is half its smallest increment in sixty-fourths; the searched cap counts steps of
    (q - N / 64) + min_increment and is never below the plain cap."""
    from focr_fast_model import line_cap
    df = DecodeFont(MONO, 13.0, FOCR_DEFAULT_ALPHABET)
    inc = df.increments()
    df.close()
    n = S.max_radius(inc)
    assert n == 64 and np.float32(n) / 64 <= inc.min() / 2
    assert S.max_radius(np.array([0.9], dtype=np.float32)) == 28  # 28 / 64 <= 0.45 < 29 / 64
    assert S.search_cap(inc, 200, 8) >= line_cap(inc, 200)
    assert S.search_cap(inc, 200, 64) >= S.search_cap(inc, 200, 8)


def test_ramp_line_crawls_under_the_searched_cap():
    """Sans 'i' alone at 7.15 px on a line that fades from black to paper: nearly every step takes j = -63, the pen
    crawls by a pixel, and the line runs to 116 characters, past the plain cap of 61 and under the searched cap of 120
    (tests/test_gpu_focr_search.py decodes the same line on the device)."""
    from focr_fast_model import line_cap
    fm = FastModel(SANS, 7.15, "i")
    n = S.max_radius(fm.incs)
    line = np.tile(np.linspace(0, 254, 120).round().astype(np.uint8), (16, 1))
    s = S.search_line(fm, line, n)
    assert n == 63 and line_cap(fm.incs, 120) == 61 and S.search_cap(fm.incs, 120, n) == 120
    assert len(s.text) == 116 and int((s.offsets == -63).sum()) == 112
    fm.close()

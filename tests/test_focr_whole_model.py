"""The whole-line model (tests/focr_whole_model.py) against FreeType and against the pages it is for.  The model is the
definition of include/focr_decode.h on FastModel.scores; here every term it uses must equal one FreeType raster of the
candidate on the line canvas, it must decode the proportional lines the greedy pen loop loses ("rn" -> "m", "cl" -> "d",
"ff" -> "m", and a line of forty "i"), and on monospace lines it must return what the greedy loop returns.  No GPU needed."""
import os

import numpy as np
import pytest

import focr_whole_model as W
from focr_fast_model import FastModel
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont
from font_ocr_amd.decoder import raster_glyph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
SERIF = os.path.join(GOLD, "DejaVuSerif.ttf")
F32 = np.float32
TEXT = "burn clip ffH vvill rnrn cl"
# what the greedy pen loop makes of the lines below at 13 px, unhinted, kerning 1, the default alphabet
GREEDY = {(SANS, TEXT): "bunY dm+Tl vvillmmY d>", (SERIF, TEXT): "bmxi Gm BH vvm Huzi O>",
          (SANS, "i" * 40): "+ii+ii+ii++ii+ii++ii+o", (SERIF, "i" * 40): "mmmmEmmmmmmmmB>"}


def test_inc64_rounds_to_nearest_even():
    got = W.inc64(np.array([1.0, 0.0078125, 0.0234375, 7.826660, 3.611328], dtype=F32))  # 64, 0.5, 1.5, 500.9, 231.1
    assert got.tolist() == [64, 0, 2, 501, 231]
    assert W.char_bound(np.array([3.611328, 7.8], dtype=F32), 145) == -(-64 * 145 // 231) == 41


def test_every_term_is_one_freetype_raster():
    """Sans 13 px, four glyphs, a crop about 20 px wide: each term(i, s) the programme asks for equals the full-canvas SSD of
    one raster_glyph canvas at origin + s / 64, less the canvas's sum of r^2; the text comes back with one character
    over the right edge, and the cost is the sum of the terms along it."""
    font, size, al = SANS, 13.0, "rnmi"
    page = W.draw_line(font, size, al, "rni")
    h, w = page.shape
    assert 18 <= w <= 24
    fm = FastModel(font, size, al)
    ox, oy = fm.font.origin
    seen = {}

    def pinned(fm_, r, total, s):
        got = W.term_from_scores(fm_, r, total, s)
        for i, ch in enumerate(al):
            canvas = np.zeros((h, w), dtype=np.uint8)
            raster_glyph(font, size, ch, F32(ox + F32(s) / F32(64)), oy, canvas)
            assert got[i] == int(((r - canvas.astype(np.int64)) ** 2).sum()) - total, (s, ch)
            seen[(s, i)] = int(got[i])
        return got

    got = W.whole_line(fm, page, term=pinned)
    fm.close()
    assert len(seen) >= 4 * 16 and len({s for s, _ in seen}) * 4 == len(seen)  # every glyph at every state reached
    assert got.text[:3] == "rni" and len(got.text) == 4
    assert got.cost == sum(seen[(int(s), int(i))] for s, i in zip(got.pens, got.idx))
    assert got.pens[0] == 0 and np.array_equal(np.diff(got.pens.astype(np.int64)), W.inc64(fm.incs)[got.idx[:-1]])
    assert got.pens[-1] < 64 * w <= got.pens[-1] + W.inc64(fm.incs)[got.idx[-1]]


@pytest.mark.parametrize("font,text", list(GREEDY), ids=["sans", "serif", "sans-i40", "serif-i40"])
def test_proportional_lines_the_greedy_loop_loses(font, text):
    """The greedy model returns exactly the wrong string recorded above; the programme returns the text and one trailing
    character that hangs over the right edge, as the reference's loop would also produce.  Forty "i" fill the character
    bound to the last place."""
    al = FOCR_DEFAULT_ALPHABET
    page = W.draw_line(font, 13.0, al, text)
    fm = FastModel(font, 13.0, al)
    assert fm.decode_line(page) == GREEDY[(font, text)]
    got = W.whole_line(fm, page)
    bound = W.char_bound(fm.incs, page.shape[1])
    fm.close()
    assert got.text[:-1] == text and len(got.text) == len(text) + 1 <= bound
    assert got.cost < 0 and abs(got.base + got.cost) < got.base // 100  # near zero: exact only while footprints do not overlap
    if font == SANS and text[0] == "i":
        assert len(got.text) == bound == 41


@pytest.mark.parametrize("text", [TEXT, "i" * 40, None], ids=["words", "i40", "random60"])
def test_monospace_lines_decode_as_the_greedy_loop_does(text):
    al = FOCR_DEFAULT_ALPHABET
    if text is None:
        text = "".join(al[i] for i in np.random.default_rng(7).integers(0, len(al), 60))
    page = W.draw_line(MONO, 13.0, al, text)
    fm = FastModel(MONO, 13.0, al)
    greedy, got = fm.decode_line(page), W.whole_line(fm, page)
    fm.close()
    assert got.text == greedy and got.text[: len(text)] == text


def test_draw_line_is_the_decoders_own_placement():
    """draw_line's first glyph sits where the decoder's phase table puts it at pen 0."""
    df = DecodeFont(SANS, 13.0, "bi")
    page = W.draw_line(SANS, 13.0, "bi", "b", width=12)
    bm, ox, oy = df.phase(0, int(df.origin[0] * 64) & 63)
    ox += int(df.origin[0] * 64) >> 6
    df.close()
    want = np.zeros(page.shape, dtype=np.uint8)
    want[oy: oy + bm.shape[0], ox: ox + bm.shape[1]] = bm
    assert np.array_equal(255 - page, want)

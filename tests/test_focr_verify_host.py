"""Host side of the focr verify (include/focr_decode.h, focr_verify_font_build): the verify table against direct
rasterisation, and a restatement of render() from the decode and verify tables alone that must equal
focr_render_text byte for byte.  The restatement is what the device's verify kernels compute.  No GPU needed."""
import os

import numpy as np
import pytest

from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, VerifyFont
from font_ocr_amd.decoder import DecoderError, glyph_metrics, raster_glyph, render_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
ASCII95 = "".join(chr(c) for c in range(32, 127))
F32 = np.float32


def compose_line(df, vf, idx):
    """render() of the alphabet indices idx from the two tables: f32 pen, union of round_out boxes from the empty rect
    at (0, 0), each glyph's true phase rectangle copied in text order at delta trunc((-ox + pos) * 64), clipped."""
    incs = df.increments()
    pos, pen = [], F32(0)
    for c in idx:
        pos.append(pen)
        pen = F32(pen + incs[c])
    ox = oy = lx = ly = 0
    for c, p in zip(idx, pos):
        b = vf.box(c)
        ox, lx = min(ox, int(np.floor(F32(b[0] + p)))), max(lx, int(np.ceil(F32(b[2] + p))))
        oy, ly = min(oy, int(np.floor(F32(b[1] + F32(0))))), max(ly, int(np.ceil(F32(b[3] + F32(0)))))
    cw, ch = lx - ox, ly - oy
    canvas = np.zeros((ch, cw), dtype=np.uint8)
    dy = -oy - int(vf.s.origin_y)  # the phases are rendered at ty = origin_y, the line at ty = -oy: whole pixels
    for c, p in zip(idx, pos):
        d = int(F32(F32(F32(-ox) + p) * F32(64)))
        phase, shift = d & 63, d >> 6
        bm, offx, offy = df.phase(c, phase)
        rx, ry, rw, rh = vf.rect(c, phase)
        x0, y0 = shift + offx + rx, offy + ry + dy
        src = bm[ry: ry + rh, rx: rx + rw]
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x0 + rw, cw), min(y0 + rh, ch)
        if cx0 < cx1 and cy0 < cy1:
            canvas[cy0:cy1, cx0:cx1] = src[cy0 - y0: cy1 - y0, cx0 - x0: cx1 - x0]
    return canvas


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
@pytest.mark.parametrize("size", [13.0, 24.0])
def test_phase_rectangles_equal_direct_rasterisation(font, hinting, size):
    """Rendered over two canvases filled with different values, the pixels FreeType's bitmap covers (zeros included)
    are the ones that agree: they must be exactly the table's rectangle, with the decode font's bytes."""
    df = DecodeFont(font, size, FOCR_DEFAULT_ALPHABET, hinting)
    vf = VerifyFont(font, size, FOCR_DEFAULT_ALPHABET, hinting)
    oy = df.origin[1]
    assert F32(vf.s.origin_y) == oy
    M, S = 16, 64 + 16
    for i, ch in enumerate(FOCR_DEFAULT_ALPHABET):
        for p in range(64):
            a = np.full((S, S), 1, dtype=np.uint8)
            b = np.full((S, S), 2, dtype=np.uint8)
            for c in (a, b):  # M whole pixels right and down of the phase, so that nothing is clipped
                raster_glyph(font, size, ch, F32((64 * M + p) / 64.0), F32(oy + M), c, hinting)
            covered = a == b
            bm, offx, offy = df.phase(i, p)
            rx, ry, rw, rh = vf.rect(i, p)
            want = np.zeros((S, S), dtype=bool)
            x0, y0 = M + offx + rx, M + offy + ry
            want[y0: y0 + rh, x0: x0 + rw] = True
            assert np.array_equal(covered, want), (ch, p)
            assert np.array_equal(a[y0: y0 + rh, x0: x0 + rw], bm[ry: ry + rh, rx: rx + rw]), (ch, p)
            assert rx + rw <= bm.shape[1] and ry + rh <= bm.shape[0]
    df.close()
    vf.close()


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("size", [13.0, 24.0])
def test_boxes_round_out_to_the_identity_bounds(font, size):
    vf = VerifyFont(font, size, ASCII95)
    df = DecodeFont(font, size, ASCII95)
    assert vf.s.n_glyphs == len(ASCII95)
    for i, ch in enumerate(ASCII95):
        g = vf.s.glyphs[i]
        assert g.codepoint == ord(ch)
        assert F32(g.increment).tobytes() == df.increments()[i].tobytes()
        b = vf.box(i)
        got = (int(np.floor(F32(b[0] + F32(0)))), int(np.floor(F32(b[1] + F32(0)))), int(np.ceil(F32(b[2] + F32(0)))),
               int(np.ceil(F32(b[3] + F32(0)))))
        assert got == glyph_metrics(font, size, ch)[2], ch
    vf.close()
    df.close()


def _strings(rng, alphabet, n):
    out = ["", "J", "jJ", "Tj", "Y  y", "j" * 7]
    out += [c + "".join(rng.choice(list(alphabet), int(rng.integers(0, 30)))) for c in "JTYj"]
    out += ["".join(rng.choice(list(alphabet), int(rng.integers(1, 45)))) for _ in range(n)]
    return out


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("kerning", [0.85, 1.0, 1.07])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
def test_composed_line_equals_render_text(font, kerning, hinting):
    """Kerning 0.85 makes neighbouring glyph boxes overlap, so a later glyph's zeros overwrite an earlier one's ink."""
    size = 13.0
    df = DecodeFont(font, size, ASCII95, hinting, kerning)
    vf = VerifyFont(font, size, ASCII95, hinting, kerning)
    rng = np.random.default_rng(int(kerning * 100) + 7 * hinting + (font == SANS))
    for text in _strings(rng, ASCII95, 40):
        want = render_text(font, size, text, kerning, hinting)
        got = compose_line(df, vf, [ASCII95.index(c) for c in text])
        assert got.shape == want.shape and np.array_equal(got, want), text
    df.close()
    vf.close()


def test_composed_line_at_24px_and_the_default_alphabet():
    size, alpha = 24.0, FOCR_DEFAULT_ALPHABET
    rng = np.random.default_rng(3)
    for font in (MONO, SANS):
        df, vf = DecodeFont(font, size, alpha, True, 0.85), VerifyFont(font, size, alpha, True, 0.85)
        for text in _strings(rng, alpha, 15):
            want = render_text(font, size, text, 0.85, True)
            assert np.array_equal(compose_line(df, vf, [alpha.index(c) for c in text]), want), text
        df.close()
        vf.close()


def test_verify_builder_refusals():
    for k in (0.0, -1.0):
        with pytest.raises(DecoderError, match="kerning"):
            VerifyFont(MONO, 13.0, FOCR_DEFAULT_ALPHABET, False, k)
    with pytest.raises(DecoderError, match="missing"):
        VerifyFont(MONO, 13.0, "AB一", False, 1.0)

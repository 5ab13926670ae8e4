"""focr_decoder_score_text (include/focr_decode.h, LineDecoder.score_text), restated for the tests.

The definition with one FreeType raster per glyph: a line's characters are placed by the pen loop's f32 walk, by the pen
search's offsets or by a whole-line run's pens; each glyph is rasterised by raster_glyph on the line's own crop at the
translation its delta names (tx = delta / 64, exact; a negative delta is what FreeType receives) and at the vertical
translation ty = origin_y + q * 2^-B of the line's baseline candidate q; its term is the sum of c * (c - 2 r) over the crop
(raster_glyph clips to the canvas on all four sides); the line's cost is the sum of its terms, and with a shift radius N the
lowest (cost_j, rank(j)) over the rigid shifts j in -N ..= N.  A font is a DecodeFont, of which only the numbers are read
(path, size, hinting, alphabet, increments, origin): nothing comes from the phase table, and nothing from the device path.
FreeType refuses a translation near 2^15 px (a pen near 2^21); such a glyph lies wholly right of any crop of the tests and
its term is 0 by the definition, which terms() checks before it takes the 0.
"""
import collections

import numpy as np

from focr_fast_model import crop
from focr_search_model import rank
from font_ocr_amd.decoder import DecoderError, raster_glyph

F32 = np.float32
STEP = F32(0.015625)

Score = collections.namedtuple("Score", "base cost shift terms")


def deltas(font, idx, pens=None, offsets=None, j=0):
    """FreeType's delta of every glyph of the line idx (alphabet indices) in `font` with the whole line moved by j / 64 px."""
    assert pens is None or offsets is None
    ox = font.origin[0]
    if pens is not None:  # the whole-line programme's: 64 * origin_x + s_g
        assert float(ox) == int(ox) >= 0 and all(0 <= int(s) < 1 << 24 for s in pens)
        return [64 * int(ox) + int(s) + j for s in pens]
    incs = font.increments()
    out, pos = [], F32(0)
    for g, i in enumerate(idx):  # the pen loop's one add, or the pen search's two; p_0 = (j_0 + j) / 64
        jg = (int(offsets[g]) if offsets is not None else 0) + (j if g == 0 else 0)
        p = F32(pos + F32(jg) * STEP)
        out.append(int(F32(F32(ox + p) * F32(64))))  # trunc, towards zero
        pos = F32(p + incs[i])
    return out


def terms(font, ref, idx, ds, q=0, y_bits=0):
    """The footprint term of every glyph of idx at the deltas ds against the cropped luma line ref, under baseline
    candidate q in steps of 2^-y_bits px: one FreeType raster each."""
    r = 255 - ref.astype(np.int64)
    oy = font.origin[1]
    assert float(oy) == int(oy) >= 0 or q == 0
    ty = F32(oy + F32(q) / F32(1 << y_bits))
    out = np.zeros(len(idx), dtype=np.int64)
    if ref.size == 0:
        return out  # an empty crop: every term 0
    canvas = np.zeros(ref.shape, dtype=np.uint8)
    for g, (i, d) in enumerate(zip(idx, ds)):
        canvas[:] = 0
        try:
            raster_glyph(font.font_path, font.text_size, font.alphabet[i], F32(d) / F32(64), ty, canvas, font.hinting)
        except DecoderError:  # FreeType refuses a translation near 2^15 px: such a glyph lies wholly right of the crop, term 0
            assert d >= 1 << 20 and (d >> 6) - 2 * int(np.ceil(font.text_size)) - 2 >= ref.shape[1], (d, ref.shape)
            continue
        c = canvas.astype(np.int64)
        out[g] = int((c * (c - 2 * r)).sum())
    return out


def score_crop(font, ref, idx, pens=None, offsets=None, q=0, y_bits=0, radius=0):
    """Score of the line idx in `font` against the cropped luma line ref."""
    r = 255 - ref.astype(np.int64)
    base = int((r * r).sum())
    best = None
    for j in sorted(range(-radius, radius + 1), key=rank):  # in rank order: a strict < keeps the lowest rank of equal costs
        t = terms(font, ref, idx, deltas(font, idx, pens, offsets, j), q, y_bits)
        if best is None or int(t.sum()) < best.cost:
            best = Score(base, int(t.sum()), j, t)
    return best


def score_text(font, page, x, y, width, line_height, text, pens=None, offsets=None, q=0, y_bits=0, radius=0):
    """Score of `text` in `font` at line slot (x, y) of a luma page, the crop clamped as image::crop_imm clamps it."""
    idx = [font.alphabet.index(c) for c in text]
    return score_crop(font, crop(page, x, y, width, line_height), idx, pens, offsets, q, y_bits, radius)


def draw_text(font, text, width, height, shift64=0):
    """A luma line of `text` in `font`, each glyph drawn by FreeType at the pen loop's own position moved right by
    shift64 / 64 px (the delta's translation, so a page drawn with shift64 = 0 costs -line_base in its own font)."""
    idx = [font.alphabet.index(c) for c in text]
    page = np.full((height, width), 255, dtype=np.uint8)
    for i, d in zip(idx, deltas(font, idx)):
        g = np.zeros((height, width), dtype=np.uint8)
        raster_glyph(font.font_path, font.text_size, font.alphabet[i], F32(d + shift64) / F32(64), font.origin[1], g, font.hinting)
        page = np.minimum(page, 255 - g)
    return page

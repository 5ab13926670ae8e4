"""CPU model of focr_decoder_verify_text (include/focr_decode.h), for the tests: the verify image of a page under a list of
lines the caller supplies, each in a font of its own.

A line without pens or offsets is rasterised by FreeType through render_text with the line's own font path, size, hinting and
kerning, and shares nothing else with the product.  With pens or offsets the glyphs are placed the way the search and
whole-line models place theirs (focr_search_model.compose_line_at: glyph q at an f32 pen of its own), with the tables of the
line's font.  The lines are composed in list order, as focr_line_model.verify_image composes them.
"""
import collections
import functools

import numpy as np

import focr_search_model as S
from font_ocr_amd.decoder import DecodeFont, VerifyFont, render_text

F32 = np.float32

# One font of a call: what render_text takes beside the text.
Font = collections.namedtuple("Font", "path size hinting kerning", defaults=(False, 1.0))
# One line of a call: y, its text, the index of its font, and (neither or one of) its pens or its offsets in 1/64 px.
Line = collections.namedtuple("Line", "y text font pens offsets", defaults=(0, None, None))


@functools.lru_cache(maxsize=None)
def tables(font, alphabet):
    """(DecodeFont, VerifyFont) of a Font over an alphabet: what compose_line_at reads."""
    return (DecodeFont(font.path, font.size, alphabet, font.hinting, font.kerning),
            VerifyFont(font.path, font.size, alphabet, font.hinting, font.kerning))


def offset_pens(df, idx, offsets):
    """The f32 pens of a pen search: the pen moves by j / 64 before glyph q is placed, and advances from there."""
    incs, pens, pen = df.increments(), [], F32(0)
    for c, j in zip(idx, offsets):
        pen = F32(pen + F32(F32(int(j)) * F32(0.015625)))
        pens.append(pen)
        pen = F32(pen + incs[c])
    return pens


def line_canvas(font, alphabet, line):
    """The coverage canvas (h x w uint8) of one line in its font, or None for an empty line."""
    if not line.text:
        return None
    if line.pens is None and line.offsets is None:
        return render_text(font.path, font.size, line.text, font.kerning, font.hinting)
    df, vf = tables(font, alphabet)
    idx = [alphabet.index(ch) for ch in line.text]
    if line.pens is not None:
        at = [F32(int(s)) / F32(64) for s in line.pens]  # a whole-line run's pens: pos = s / 64, exact
    else:
        at = offset_pens(df, idx, line.offsets)
    return S.compose_line_at(df, vf, idx, at)


def verify_text(page, lines, fonts, alphabet, x):
    """(image, exact sum of (R - B)^2) of one page under lines (Line records, in drawing order) in fonts (Font records):
    red is the page's luma where it is not 255, blue 255 - v where the last line over the pixel has v != 0."""
    H, W = page.shape
    out = np.zeros((H, W, 3), dtype=np.uint8)
    out[..., 0] = np.where(page != 255, page, 0)
    for line in lines:
        c = line_canvas(fonts[line.font], alphabet, Line(*line))
        if c is None:
            continue
        hh, ww = min(c.shape[0], H - line.y), min(c.shape[1], W - x)
        if hh > 0 and ww > 0:
            c = c[:hh, :ww]
            np.copyto(out[line.y: line.y + hh, x: x + ww, 2], 255 - c, where=c != 0)
    d = out[..., 0].astype(np.int64) - out[..., 2].astype(np.int64)
    return out, int((d * d).sum())


def mse(sq_sum, W, H):
    """red_blue_mse of the reference: (sum as f32) / (w * h as u32 as f32)."""
    return F32(F32(int(sq_sum)) / F32((W * H) & 0xFFFFFFFF))


def draw_lines(page, lines, fonts, x):
    """Darken `page` with every line rendered by render_text in its own font at (x, y), clipped: a page to verify against."""
    H, W = page.shape
    for line in lines:
        line = Line(*line)
        if not line.text:
            continue
        f = fonts[line.font]
        c = render_text(f.path, f.size, line.text, f.kerning, f.hinting)
        hh, ww = min(c.shape[0], H - line.y), min(c.shape[1], W - x)
        if hh > 0 and ww > 0:
            region = page[line.y: line.y + hh, x: x + ww]
            region[:] = np.minimum(region, 255 - c[:hh, :ww])
    return page

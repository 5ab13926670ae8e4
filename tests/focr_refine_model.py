"""focr_decoder_refine_text (include/focr_decode.h, LineDecoder.refine_text), restated for the tests in numpy.

The definition, step by step, over a FastModel's phase tables: a character's clipped bitmap c_g is DecodeFont.phase at
delta = 64 * origin_x + pen (phase delta & 63, whole-pixel shift delta >> 6), clipped to the crop on all four sides; the composed
canvas is the max of the characters' bitmaps; with r = 255 - luma and f(v) = v * (v - 2 r) the composed cost is the sum of f over the
crop.  One step for character g: o is the canvas of all the others, D(a, j) the sum of f(max(c, o)) - f(o) for glyph a at pen
s_g + j; the lowest (D, rank(j), a) replaces the character if its D is strictly below the incumbent's.  A step scores all glyphs of
one pen at once from FastModel._phase's stack (one frame that holds every glyph of the phase; outside a glyph's own bitmap the frame
is 0, and a pixel with c = 0 adds nothing to D).  brute() is the same with one FreeType raster per candidate and the whole canvas
composed anew.  Nothing here comes from the device path.
"""
import collections

import numpy as np

from focr_search_model import rank
from font_ocr_amd.decoder import DecoderError, raster_glyph

F32 = np.float32
PEN_END = 1 << 24

Refine = collections.namedtuple("Refine", "base cost_in cost sweeps changed idx pens")


def f_of(v, r):
    return v * (v - 2 * r)


def clipped(font, i, pen, h, w):
    """(ya, yb, xa, xb, c): glyph i of the DecodeFont at `pen`, clipped to an h x w crop; None when nothing of it is on the crop."""
    ox = font.origin[0]
    assert float(ox) == int(ox) >= 0
    d = 64 * int(ox) + int(pen)
    bm, fx, fy = font.phase(i, d & 63)
    x0, y0 = (d >> 6) + fx, fy
    ya, yb, xa, xb = max(y0, 0), min(y0 + bm.shape[0], h), max(x0, 0), min(x0 + bm.shape[1], w)
    if ya >= yb or xa >= xb:
        return None
    return ya, yb, xa, xb, bm[ya - y0: yb - y0, xa - x0: xb - x0].astype(np.int64)


def compose(font, idx, pens, h, w, skip=None):
    """The composed canvas (h x w int64) of the line but character `skip`."""
    v = np.zeros((h, w), dtype=np.int64)
    for g, (i, s) in enumerate(zip(idx, pens)):
        box = None if g == skip else clipped(font, i, s, h, w)
        if box is not None:
            ya, yb, xa, xb, c = box
            np.maximum(v[ya:yb, xa:xb], c, out=v[ya:yb, xa:xb])
    return v


def composed_cost(font, ref, idx, pens):
    """C of the line against the cropped luma line ref."""
    r = 255 - ref.astype(np.int64)
    h, w = ref.shape if ref.size else (0, 0)
    return int(f_of(compose(font, idx, pens, h, w), r.reshape(h, w)).sum())


def stack_terms(fm, r, o, pen):
    """D of every glyph of the FastModel at `pen` over the canvas o of the others: an int64 array of len(alphabet)."""
    h, w = r.shape
    d = 64 * int(fm.ox) + int(pen)
    st, fy0, fx0 = fm._phase(d & 63)
    sx = (d >> 6) + fx0
    y0, y1, x0, x1 = max(0, fy0), min(h, fy0 + st.shape[1]), max(0, sx), min(w, sx + st.shape[2])
    if y0 >= y1 or x0 >= x1:
        return np.zeros(st.shape[0], dtype=np.int64)
    c = st[:, y0 - fy0: y1 - fy0, x0 - sx: x1 - sx].astype(np.int64)
    ow, rw = o[y0:y1, x0:x1], r[y0:y1, x0:x1]
    return (f_of(np.maximum(c, ow), rw) - f_of(ow, rw)).sum(axis=(1, 2))


def raster_terms(font):
    """stack_terms from one FreeType raster per candidate on the crop itself: for brute()."""
    def terms(fm, r, o, pen):
        h, w = r.shape
        out = np.zeros(len(font.alphabet), dtype=np.int64)
        canvas = np.zeros((h, w), dtype=np.uint8)
        for a, ch in enumerate(font.alphabet):
            canvas[:] = 0
            raster_glyph(font.font_path, font.text_size, ch, F32(64 * int(font.origin[0]) + pen) / F32(64), font.origin[1], canvas, font.hinting)
            c = canvas.astype(np.int64)
            out[a] = int((f_of(np.maximum(c, o), r) - f_of(o, r)).sum())
        return out
    return terms


def refine_crop(fm, ref, idx, pens, radius=4, sweeps=4, glyphs=True, terms=stack_terms, canvas=None):
    """Refine of the line idx (alphabet indices) at `pens` against the cropped luma line ref by the FastModel fm.  `terms` scores the
    glyphs of one pen (stack_terms, or raster_terms for the brute force); `canvas` composes the others (compose over the phase
    tables, or the brute force's)."""
    font = fm.font
    h, w = ref.shape if ref.size else (0, 0)
    r = 255 - ref.astype(np.int64).reshape(h, w)
    base = int((r * r).sum())
    idx, pens = [int(i) for i in idx], [int(s) for s in pens]
    idx_in, pens_in = list(idx), list(pens)
    assert all(0 <= s < PEN_END for s in pens) and all(a <= b for a, b in zip(pens, pens[1:]))
    canvas = canvas or (lambda idx, pens, skip=None: compose(font, idx, pens, h, w, skip))
    cost_in = int(f_of(canvas(idx, pens), r).sum())
    js = sorted(range(-radius, radius + 1), key=rank)
    run = 0
    for _ in range(sweeps):
        moved = False
        for g in range(len(idx)):
            if h == 0 or w == 0:
                continue  # an empty crop: every D is 0
            o = canvas(idx, pens, g)
            inc = int(terms(fm, r, o, pens[g])[idx[g]])
            best = None
            for j in js:
                if not 0 <= pens[g] + j < PEN_END:
                    continue
                t = terms(fm, r, o, pens[g] + j)
                for a in (range(len(t)) if glyphs else [idx[g]]):
                    key = (int(t[a]), rank(j), a)
                    if best is None or key < best[0]:
                        best = (key, a, j)
            if best[0][0] < inc:  # strictly: among equal D the incumbent stays
                idx[g], pens[g] = best[1], pens[g] + best[2]
                moved = True
        run += 1
        if not moved:
            break
    cost = int(f_of(canvas(idx, pens), r).sum())
    changed = sum(a != b or s != t for a, b, s, t in zip(idx, idx_in, pens, pens_in))
    return Refine(base, cost_in, cost, run, changed, idx, np.array(pens, dtype=np.uint32))


def brute(fm, ref, idx, pens, radius=4, sweeps=4, glyphs=True):
    """refine_crop with nothing from the phase tables: every candidate and every character of the canvas is one FreeType raster on the
    crop (raster_glyph clips to the canvas on all four sides), and the canvas is composed anew for every step."""
    font = fm.font
    h, w = ref.shape if ref.size else (0, 0)

    def canvas(idx, pens, skip=None):
        v = np.zeros((h, w), dtype=np.uint8)
        for g, (i, s) in enumerate(zip(idx, pens)):
            if g == skip or h == 0 or w == 0:
                continue
            one = np.zeros((h, w), dtype=np.uint8)
            try:
                raster_glyph(font.font_path, font.text_size, font.alphabet[i], F32(64 * int(font.origin[0]) + s) / F32(64), font.origin[1], one, font.hinting)
            except DecoderError:  # FreeType refuses a translation near 2^15 px: such a glyph lies wholly right of the crop
                assert s >= 1 << 20
                continue
            v = np.maximum(v, one)
        return v.astype(np.int64)

    return refine_crop(fm, ref, idx, pens, radius, sweeps, glyphs, terms=raster_terms(font), canvas=canvas)


def text_of(fm, idx):
    return "".join(fm.alphabet[i] for i in idx)

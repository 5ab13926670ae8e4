"""focr_decoder_learn_text and focr_decode_font_learn (include/focr_decode.h; LineDecoder.learn_text, DecodeFont.learned), restated
for the tests in numpy.

The definition, one character at a time: the placement is focr_score_text_model.deltas' (the pen loop's f32 walk, the pen search's
offsets or a whole-line run's pens, at shift 0); a character's box is box_w x box_h at crop column (delta >> 6) + off_x[p] and crop
row off_y[p], p = delta & 63, read from DecodeFont.phase; it contributes iff it is in use, its line is in the font that is learned,
the crop is not empty and the box lies wholly inside it; it then adds 1 to counts[i * 64 + p] and r = 255 - luma under the box to
the cell's block of sums, which has the font's own `bitmaps` layout.  The learned font is restated from the base font's phases:
the bounding rectangle of a phase's ink, grown and clipped, takes the means rounded half up.  Nothing comes from the device path,
and nothing from the native learn_font.h.
"""
import collections

import numpy as np

from focr_fast_model import crop
from focr_score_text_model import deltas

Learned = collections.namedtuple("Learned", "sums counts used")


def layout(font):
    """Per glyph (offset, stride, box_h, box_w) of the font's `bitmaps`, and the table's length."""
    gs = [font.s.glyphs[i] for i in range(font.s.n_glyphs)]
    return [(int(g.offset), int(g.stride), int(g.box_h), int(g.box_w)) for g in gs], int(font.s.bitmaps_len)


def empty(font):
    lay, n = layout(font)
    return Learned(np.zeros(n, dtype=np.uint64), np.zeros(64 * len(lay), dtype=np.uint64), [])


def boxes(font, idx, ds):
    """Per character (phase, x0, y0, box_w, box_h) of its box on the crop."""
    out = []
    for i, d in zip(idx, ds):
        bm, ox, oy = font.phase(i, d & 63)
        out.append((d & 63, (d >> 6) + ox, oy, bm.shape[1], bm.shape[0]))
    return out


def learn_crop(font, acc, ref, idx, pens=None, offsets=None, use=None):
    """One line idx (alphabet indices) of `font` against its cropped luma line ref, added to acc (a Learned); its used flags."""
    lay, _ = layout(font)
    r = 255 - ref.astype(np.int64)
    h, w = ref.shape if ref.size else (0, 0)
    used = np.zeros(len(idx), dtype=np.uint8)
    for g, (i, (p, x0, y0, bw, bh)) in enumerate(zip(idx, boxes(font, idx, deltas(font, idx, pens, offsets)))):
        if use is not None and not use[g]:
            continue
        if h == 0 or w == 0 or x0 < 0 or y0 < 0 or x0 + bw > w or y0 + bh > h:
            continue  # no partial boxes; an empty crop holds none
        used[g] = 1
        acc.counts[i * 64 + p] += 1
        off, stride, box_h, box_w = lay[i]
        assert (box_h, box_w) == (bh, bw)
        cell = acc.sums[off + p * stride * box_h: off + (p + 1) * stride * box_h].reshape(box_h, stride)
        cell[:, :box_w] += r[y0: y0 + bh, x0: x0 + bw].astype(np.uint64)
    return used


def learn_text(font, pages, lines, x, width, line_height, fonts=None, pens=None, offsets=None, use=None, k=0):
    """LineDecoder.learn_text for the font `font` = font k: pages a list of luma pages, lines [[(y, text), ...] per page]; fonts,
    pens, offsets and use per [page][line] as there.  A Learned with used[page][line]."""
    acc = empty(font)
    for pi, pg in enumerate(lines):
        row = []
        for q, (y, text) in enumerate(pg):
            if (fonts[pi][q] if fonts is not None else 0) != k:
                row.append(np.zeros(len(text), dtype=np.uint8))
                continue
            idx = [font.alphabet.index(c) for c in text]
            row.append(learn_crop(font, acc, crop(pages[pi], x, y, width, line_height), idx, pens[pi][q] if pens is not None else None,
                                  offsets[pi][q] if offsets is not None else None, use[pi][q] if use is not None else None))
        acc.used.append(row)
    return acc


def support(bm, grow):
    """The bounding rectangle (y0, y1, x0, x1) of bm's non-zero pixels grown by `grow` a side and clipped to bm; None without ink."""
    ys, xs = np.nonzero(bm)
    if ys.size == 0:
        return None
    return (max(int(ys.min()) - grow, 0), min(int(ys.max()) + 1 + grow, bm.shape[0]), max(int(xs.min()) - grow, 0),
            min(int(xs.max()) + 1 + grow, bm.shape[1]))


def learned_phases(font, acc, min_count=1, grow=0):
    """{(i, p): bitmap} of every learned cell of `font` (count >= min_count and ink in the base phase), and the number of cells with ink."""
    lay, _ = layout(font)
    out, inked = {}, 0
    for i, (off, stride, box_h, box_w) in enumerate(lay):
        for p in range(64):
            bm = font.phase(i, p)[0]
            s = support(bm, grow)
            if s is None:
                continue
            inked += 1
            n = int(acc.counts[i * 64 + p])
            if n < min_count:
                continue
            cell = acc.sums[off + p * stride * box_h: off + (p + 1) * stride * box_h].reshape(box_h, stride)[:, :box_w].astype(np.int64)
            y0, y1, x0, x1 = s
            new = bm.copy()
            new[y0:y1, x0:x1] = ((2 * cell[y0:y1, x0:x1] + n) // (2 * n)).astype(np.uint8)  # the mean, half up
            out[(i, p)] = new
    return out, inked


class Tables:
    """The phases of a font with some cells replaced: what focr_score_text's terms and the pen loop read of a font."""

    def __init__(self, font, cells=None):
        self.font, self.cells = font, cells or {}

    def phase(self, i, p):
        bm, ox, oy = self.font.phase(i, p)
        return self.cells.get((i, p), bm), ox, oy


def table_terms(tables, ref, idx, ds):
    """The footprint term of every glyph of idx at the deltas ds against the cropped luma line ref, from phase tables: the sum
    of c * (c - 2 r) over the bitmap clipped to the crop on all four sides."""
    r = 255 - ref.astype(np.int64)
    h, w = ref.shape if ref.size else (0, 0)
    out = np.zeros(len(idx), dtype=np.int64)
    for g, (i, d) in enumerate(zip(idx, ds)):
        bm, ox, oy = tables.phase(i, d & 63)
        x0, y0 = (d >> 6) + ox, oy
        ya, yb, xa, xb = max(y0, 0), min(y0 + bm.shape[0], h), max(x0, 0), min(x0 + bm.shape[1], w)
        if ya >= yb or xa >= xb:
            continue
        c = bm[ya - y0: yb - y0, xa - x0: xb - x0].astype(np.int64)
        out[g] = int((c * (c - 2 * r[ya:yb, xa:xb])).sum())
    return out


def decode_line(tables, ref, n_glyphs, incs, origin_x):
    """The plain pen loop on one cropped luma line from phase tables: alphabet indices (the first minimum of the terms per step)."""
    F32 = np.float32
    w = ref.shape[1] if ref.size else 0
    pos, out = F32(0), []
    while pos < F32(w):
        d = int(F32(F32(origin_x + pos) * F32(64)))
        t = table_terms(tables, ref, list(range(n_glyphs)), [d] * n_glyphs)
        i = int(np.argmin(t))
        out.append(i)
        pos = F32(pos + incs[i])
    return out

"""The focr decoder's fractional line grid, restated for the tests (focr_decoder_set_line_frac,
LineDecoder.decode(..., y_frac=, line_advance_frac=)).

The definition of include/focr_decode.h in plain integers: L = 64 * line_advance + advance_frac, slot i's top at
Y_i = 64 * y_start + y_frac + i * L, its crop row yc_i = Y_i >> 6, its rows h_i = min(line_height, page_h - yc_i), its
sub-pixel part f_i = Y_i & 63 and its centre c_i = ((f_i << B) + 32) >> 6; a page has the slots with yc_i < page_h.  The
candidates of line i are q = c_i + offset, the offsets -N ..= N in rank order, and the two searches are the two baseline
models' own per-candidate decodes (BaselineModel.decode_line_q; focr_whole_baseline_model.whole_line_q) under those q: the
lowest (cost_q, rank) of the candidates not dropped.  The verify is the two models' verify_image with (yc_i, text, q).
Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_baseline_model as B
import focr_whole_baseline_model as WB
from focr_fast_model import crop

Slot = collections.namedtuple("Slot", "i Y yc h f")


def step(line_advance, advance_frac):
    return 64 * line_advance + advance_frac


def slot(i, page_h, y_start, y_frac, line_height, line_advance, advance_frac):
    """Slot i of the grid, whether or not the page has it (yc is clamped as image::crop_imm clamps it)."""
    Y = 64 * y_start + y_frac + i * step(line_advance, advance_frac)
    yc = min(Y >> 6, page_h)
    return Slot(i, Y, yc, min(line_height, page_h - yc), Y & 63)


def n_slots(page_h, y_start, y_frac, line_height, line_advance, advance_frac):
    """The closed form of the header: ceil((64 * page_h - Y_0) / L), or 0 when the first crop is empty."""
    if line_height == 0 or y_start >= page_h:
        return 0
    L = step(line_advance, advance_frac)
    return -((64 * y_start + y_frac - 64 * page_h) // L)


def slots(page_h, y_start, y_frac, line_height, line_advance, advance_frac):
    """The slots of a page, by walking the grid while the crop row is on the page (not by the closed form)."""
    out = []
    while line_height:
        s = slot(len(out), page_h, y_start, y_frac, line_height, line_advance, advance_frac)
        if (s.Y >> 6) >= page_h:
            break
        out.append(s)
    return out


def centre(f, y_bits):
    """c_i: f / 64 px in steps of 2^-B px, halves up."""
    return ((f << y_bits) + 32) >> 6


def candidates(c, n):
    """The candidates of a line with centre c and radius n, in rank order: c, c - 1, c + 1, ..."""
    return [c + o for o in B.candidates(n)]


def search_line(m, ref, c, n):
    """focr_baseline_model.Baseline of one cropped luma line around the centre c: BaselineModel.search_line with the
    centred candidate list."""
    best = None
    for q in candidates(c, n):  # in rank order: a strict < keeps the lowest rank of equal costs
        if m.dropped(q):
            continue
        text, cost = m.decode_line_q(ref, q)
        if best is None or cost < best.cost:
            best = B.Baseline(text, q, cost)
    return best


def whole_search_line(m, ref, c, n):
    """focr_whole_baseline_model.WholeBaseline of one cropped luma line around the centre c."""
    best = None
    for q in candidates(c, n):
        if m.dropped(q):
            continue
        w = WB.whole_line_q(m, ref, q)
        if best is None or w.cost < best.cost:
            best = WB.WholeBaseline(w.text, w.idx, w.pens, w.cost, q)
    return best


def search_image(m, page, x, y, width, line_height, line_advance, n, y_frac, advance_frac, whole=False):
    """[(yc_i, Baseline or WholeBaseline)] of every non-blank slot of a page on the fractional grid."""
    out = []
    for s in slots(page.shape[0], y, y_frac, line_height, line_advance, advance_frac):
        line = crop(page, x, s.yc, width, line_height)
        if not np.all(line == 255):
            c = centre(s.f, m.y_bits)
            out.append((s.yc, (whole_search_line if whole else search_line)(m, line, c, n)))
    return out


def verify_image(page, found, df, vf, x, y_bits, whole=False):
    """The verify image and squared error after a run on the grid: found is search_image's result; the two models'
    verify_image with yc_i as the line's y and the absolute q."""
    if whole:
        return WB.verify_image(page, [(y, r.text, r.pens, r.q) for y, r in found], df, vf, x, y_bits)
    return B.verify_image(page, [(y, r.text, r.q) for y, r in found], df, vf, x, y_bits)


def draw_page(page, font, size, alphabet, texts, x, y, y_frac, line_advance, advance_frac, hinting=False, kerning=1.0):
    """Darken `page` with texts[i] on slot i of the grid (None or "": nothing): each glyph rasterised by FreeType with its
    line's top at Y_i / 64 px, i.e. f_i / 64 px below row Y_i >> 6.  Slots whose crop row is off the page are skipped."""
    H = page.shape[0]
    for i, text in enumerate(texts):
        Y = 64 * y + y_frac + i * step(line_advance, advance_frac)
        if text and (Y >> 6) < H:
            B.draw_offset(page, font, size, alphabet, text, x, Y >> 6, (Y & 63) / 64.0, hinting, kerning)
    return page

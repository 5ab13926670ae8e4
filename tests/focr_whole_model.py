"""The focr decoder's whole-line decode, restated for the tests (focr_decoder_set_whole_line,
LineDecoder.decode(whole_line=True)).

The definition of include/focr_decode.h on FastModel.scores (tests/focr_fast_model.py): states are pens s in 1/64 px from
0; the rendering at s is the plain decoder's at pos = s / 64 (exact in f32 below 2^24, and origin_x is a whole number,
so the delta is 64 * origin_x + s); term(i, s) is glyph i's full-canvas SSD there less the canvas's sum of r^2, the
footprint term; cost[0] = 0 and cost[t] is the minimum of cost[s] + term(i, s) over glyphs i and reachable states
s = t - inc64[i] with 0 <= s < 64 * w, the glyph remembered for t the one with the lowest (cost, i); the line ends in
the reachable state t >= 64 * w with the lowest (cost[t], t) and the text is read back along the remembered glyphs.
draw_line draws the pages the tests decode, and verify_image is draw_verify with every character at its returned pen.
Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_search_model as S
from font_ocr_amd.decoder import DecodeFont, raster_glyph, render_text

F32 = np.float32
INF = np.iinfo(np.int64).max

Whole = collections.namedtuple("Whole", "text idx pens cost base")


def inc64(increments):
    """(int)rintf(increment * 64) of every glyph: the multiply is exact in f32, the rounding is to nearest even."""
    return np.rint(np.asarray(increments, dtype=F32) * F32(64)).astype(np.int64)


def char_bound(increments, w):
    """The exact bound on a whole-line result's characters: ceil(64 * w / min inc64)."""
    m = int(inc64(increments).min())
    return max(-(-64 * w // m), 1)


def term_from_scores(fm, r, total, s):
    """term(i, s) of every glyph i: FastModel.scores at pos = s / 64 less the canvas's sum of r^2."""
    return fm.scores(r, F32(s) / F32(64)) - total


def whole_line(fm, ref, term=term_from_scores):
    """Whole of one cropped luma line (h x w uint8) by the FastModel fm.  idx: alphabet indices; pens: each character's
    state s (uint32, 1/64 px); cost: the sum of the terms along the text; base: the crop's sum of r^2."""
    h, w = ref.shape
    r = 255 - ref.astype(np.int64)
    total = int((r * r).sum())
    inc = inc64(fm.incs)
    assert inc.min() >= 1 and float(fm.ox) == int(fm.ox) >= 0
    n_live = 64 * w
    # glyphs that share an increment reach the same state from s: of each such group only the lowest (term, i) matters
    perm = np.lexsort((np.arange(len(inc)), inc))
    starts = np.flatnonzero(np.r_[True, np.diff(inc[perm]) != 0])
    sizes = np.diff(np.r_[starts, len(inc)])
    step = inc[perm][starts]
    at = np.arange(len(inc))
    cost = np.full(n_live + int(inc.max()), INF, dtype=np.int64)
    glyph = np.full(len(cost), -1, dtype=np.int64)
    cost[0] = 0
    for s in range(n_live):
        if cost[s] == INF:
            continue
        c = term(fm, r, total, s)[perm]
        low = np.minimum.reduceat(c, starts)
        first = np.minimum.reduceat(np.where(c == np.repeat(low, sizes), at, len(inc)), starts)
        gi = perm[first]  # within a group perm ascends, so the first minimum is the lowest index
        cand, t = cost[s] + low, s + step
        better = (cand < cost[t]) | ((cand == cost[t]) & (gi < glyph[t]))
        cost[t[better]], glyph[t[better]] = cand[better], gi[better]
    end = n_live + int(np.argmin(cost[n_live:]))  # the first minimum: the lowest (cost, t)
    assert cost[end] != INF
    idx, pens, t = [], [], end
    while t > 0:
        i = int(glyph[t])
        t -= int(inc[i])
        idx.append(i)
        pens.append(t)
    idx, pens = idx[::-1], pens[::-1]
    return Whole("".join(fm.alphabet[i] for i in idx), np.array(idx, dtype=np.uint16), np.array(pens, dtype=np.uint32),
                 int(cost[end]), total)


def whole_image(fm, page, x, y, width, line_height, line_advance):
    """[(y, Whole)] of every non-blank line of a page, as FastModel.decode_image walks it."""
    from focr_fast_model import crop
    out = []
    i = 0
    while True:
        ly = y + i * line_advance
        i += 1
        line = crop(page, x, ly, width, line_height)
        if line.shape[0] == 0:
            return out
        if not np.all(line == 255):
            out.append((ly, whole_line(fm, line)))


# ---- the pages of the tests ------------------------------------------------------------------------------------------

def alphabet_height(font, size, alphabet):
    """Rows of render_text of the whole alphabet: a line canvas that holds every glyph at the decoder's origin."""
    return render_text(font, size, alphabet).shape[0]


def draw_line(font, size, alphabet, text, width=None, height=None):
    """A luma line of `text`, each glyph drawn with FreeType at the decoder's own origin and f32 pens (kerning 1,
    unhinted), as focr_fast_model.narrowest_glyph_line draws its line.  The canvas is as tall as render_text of the
    alphabet and, without a width, as wide as the last pen rounded up: the pen loop's `pos < width` then ends on the
    text's last character, give or take one."""
    f = DecodeFont(font, size, alphabet)
    inc, (ox, oy) = f.increments(), f.origin
    f.close()
    pens, pos = [], F32(0)
    for ch in text:
        pens.append(pos)
        pos = F32(pos + inc[alphabet.index(ch)])
    w = int(np.ceil(pos)) if width is None else width
    h = alphabet_height(font, size, alphabet) if height is None else height
    page = np.full((h, w), 255, dtype=np.uint8)
    for ch, p in zip(text, pens):
        g = np.zeros((h, w), dtype=np.uint8)
        raster_glyph(font, size, ch, F32(ox + p), oy, g)
        page = np.minimum(page, 255 - g)
    return page


# ---- draw_verify at the returned pens --------------------------------------------------------------------------------

def verify_image(page, lines, df, vf, x):
    """focr_search_model.verify_image with every character of a line at pos = s / 64 of its returned pen s: lines is
    [(y, text, uint32 pens)].  Returns (image, exact sum of (R - B)^2)."""
    return S.verify_image(page, [(y, t, [F32(int(s)) / F32(64) for s in pens]) for y, t, pens in lines], df, vf, x)

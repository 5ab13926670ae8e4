"""The focr decoder's per-character scores, restated for the tests (focr_decoder_get_scores, LineDecoder.decode(scores=True)).

Along the fast model's pen walk (tests/focr_fast_model.py), every step ranks all glyphs by (full-canvas SSD, alphabet
index): the first is the decoded character and its score, the second the runner-up and its score.  base is the sum of
r^2 over the crop.  brute_line_scores is the same ranking with every candidate rasterised by FreeType at its float
translation (tests/focr_line_model.py's primitives): it pins the ranking to the reference's score_glyph, at a cost that
only a tiny line can pay.  Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_line_model as M
from focr_fast_model import crop

F32 = np.float32
NO_RUNNER = 0xFFFF
INT64_MAX = np.iinfo(np.int64).max

Scored = collections.namedtuple("Scored", "text base score runner runner_score")


def _top2(s):
    """(best, its score, runner, its score) of one step's int64 scores: lowest (score, index) first."""
    order = np.lexsort((np.arange(len(s)), s))
    if len(s) == 1:
        return int(order[0]), int(s[order[0]]), NO_RUNNER, INT64_MAX
    return int(order[0]), int(s[order[0]]), int(order[1]), int(s[order[1]])


def _scored(alphabet, r, steps):
    best = [t[0] for t in steps]
    return Scored("".join(alphabet[i] for i in best), int((r * r).sum()), np.array([t[1] for t in steps], dtype=np.int64),
                  np.array([t[2] for t in steps], dtype=np.uint16), np.array([t[3] for t in steps], dtype=np.int64))


def line_scores(fm, ref):
    """Scored of one cropped luma line (h x w uint8) by the FastModel fm."""
    r = 255 - ref.astype(np.int64)
    pos, steps = F32(0), []
    while pos < F32(ref.shape[1]):
        steps.append(_top2(fm.scores(r, pos)))
        pos = F32(pos + fm.incs[steps[-1][0]])
    return _scored(fm.alphabet, r, steps)


def image_scores(fm, page, x, y, width, line_height, line_advance):
    """[(y, Scored)] of every non-blank line of a page, as FastModel.decode_image walks it."""
    out = []
    i = 0
    while True:
        ly = y + i * line_advance
        i += 1
        line = crop(page, x, ly, width, line_height)
        if line.shape[0] == 0:
            return out
        if not np.all(line == 255):
            out.append((ly, line_scores(fm, line)))


def brute_line_scores(ref, font, size, alphabet, kerning=1.0, hinting=False):
    """Scored of one cropped luma line with one FreeType raster per candidate per step and the full-canvas int64 SSD."""
    h, w = ref.shape
    r = 255 - ref.astype(np.int64)
    ox, oy = M.origin(font, size, alphabet)
    incs = [M.increment(font, size, ch, kerning) for ch in alphabet]
    pos, steps = F32(0), []
    canvas = np.zeros((h, w), dtype=np.uint8)
    while pos < F32(w):
        s = np.zeros(len(alphabet), dtype=np.int64)
        for i, ch in enumerate(alphabet):
            canvas[:] = 0
            M.raster_glyph(font, size, ch, F32(ox + pos), oy, canvas, hinting)
            s[i] = int(((r - canvas.astype(np.int64)) ** 2).sum())
        steps.append(_top2(s))
        pos = F32(pos + incs[steps[-1][0]])
    return _scored(alphabet, r, steps)


def draw(page, font, size, text, x, y, kerning=1.0, hinting=False):
    """Darken `page` with render() of text at (x, y), clipped to the page."""
    c = M.render_text(font, size, text, kerning, hinting)
    H, W = page.shape
    hh, ww = min(c.shape[0], H - y), min(c.shape[1], W - x)
    if hh > 0 and ww > 0:
        page[y: y + hh, x: x + ww] = np.minimum(page[y: y + hh, x: x + ww], 255 - c[:hh, :ww])

"""The focr decoder's font search, restated for the tests (focr_decoder_set_font_candidates / _set_font_search,
LineDecoder.decode(font_search=True)).

The definition of include/focr_decode.h on a list of FastModels over one alphabet (tests/focr_fast_model.py); models[0] is the
decode font, models[1:] the uploaded candidates.  Pen-loop form: every candidate decodes the line by the plain pen loop with
its own tables, increments and origin_x, and cost_k is the sum of the chosen glyphs' footprint terms (FastModel.scores less
the crop's sum of r^2).  Whole-line form: every candidate decodes the line by focr_whole_model.whole_line, and cost_k is its
end state's cost.  The line is the candidate with the lowest (cost_k, k).  Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_whole_model as W
from focr_fast_model import crop

F32 = np.float32

# text, alphabet indices, the winner k and its cost, the crop's sum of r^2; pens: the winner's (whole-line form; else None);
# trail: [(k, cost)] of every candidate that became the best so far, in order (the last one is the winner)
Fonts = collections.namedtuple("Fonts", "text idx k cost base pens trail")


def pen_loop(fm, ref):
    """The plain pen loop of the FastModel fm on one cropped luma line -> (alphabet indices, cost, base)."""
    r = 255 - ref.astype(np.int64)
    total = int((r * r).sum())
    pos, idx, cost = F32(0), [], 0
    while pos < F32(ref.shape[1]):
        s = fm.scores(r, pos)
        i = int(np.argmin(s))  # the first minimum
        idx.append(i)
        cost += int(s[i]) - total
        pos = F32(pos + fm.incs[i])
    return idx, cost, total


def _same_alphabet(models):
    assert len(models) >= 1 and all(m.alphabet == models[0].alphabet for m in models)
    return models[0].alphabet


def search_line(models, ref):
    """Fonts of one cropped luma line under the pen loop of every model: the lowest (cost_k, k)."""
    alphabet = _same_alphabet(models)
    best, trail = None, []
    for k, fm in enumerate(models):  # in index order: a strict < keeps the first of equal costs
        idx, cost, base = pen_loop(fm, ref)
        if best is None or cost < best[2]:
            best = (idx, k, cost, base)
            trail.append((k, cost))
    idx, k, cost, base = best
    return Fonts("".join(alphabet[i] for i in idx), np.array(idx, dtype=np.uint16), k, cost, base, None, trail)


def whole_search_line(models, ref):
    """Fonts of one cropped luma line under the whole-line programme of every model: the lowest (cost_k, k)."""
    _same_alphabet(models)
    best, trail = None, []
    for k, fm in enumerate(models):
        w = W.whole_line(fm, ref)
        if best is None or w.cost < best[1].cost:
            best = (k, w)
            trail.append((k, w.cost))
    k, w = best
    return Fonts(w.text, w.idx, k, w.cost, w.base, w.pens, trail)


def search_image(models, page, x, y, width, line_height, line_advance, whole=False):
    """[(y, Fonts)] of every non-blank line of a page, as FastModel.decode_image walks it."""
    out = []
    i = 0
    while True:
        ly = y + i * line_advance
        i += 1
        line = crop(page, x, ly, width, line_height)
        if line.shape[0] == 0:
            return out
        if not np.all(line == 255):
            out.append((ly, (whole_search_line if whole else search_line)(models, line)))

"""The focr decoder's whole-line decode under every baseline candidate, restated for the tests
(focr_decoder_set_whole_baseline, LineDecoder.decode(whole_line=True, whole_baseline=N)).

The definition of include/focr_decode.h composed from the two models it names: candidates, y-phases, the row shift d, the
four-sided clipping, dropped candidates and rank are tests/focr_baseline_model.py's (BaselineModel.scores_q is the
full-canvas SSD of every glyph under candidate q); states, inc64, cost, the end state and the read-back are
tests/focr_whole_model.py's (whole_line(fm, ref, term=...)).  term_q(i, s) is scores_q at pos = s / 64 less the canvas's
sum of r^2; under candidate q the line is whole_line with term_q in term's place, and the line is the candidate with the
lowest (cost_q, rank(q)).  The verify model draws compose_line_at at the returned pens, row_shift(q) rows down, clipped as
focr_baseline_model.verify_image clips.  tests/test_focr_whole_baseline_model.py pins term_q to one FreeType raster per
candidate.  Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_baseline_model as B
import focr_whole_model as WM
from focr_fast_model import crop
from focr_search_model import compose_line_at

F32 = np.float32

WholeBaseline = collections.namedtuple("WholeBaseline", "text idx pens cost q")


def term_q(q):
    """The `term` of focr_whole_model.whole_line under candidate q, for a BaselineModel fm."""
    return lambda fm, r, total, s: fm.scores_q(r, F32(s) / F32(64), q) - total


def whole_line_q(m, ref, q):
    """focr_whole_model.Whole of one cropped luma line by the BaselineModel m under candidate q."""
    return WM.whole_line(m, ref, term=term_q(q))


def search_line(m, ref, n, trail=None):
    """WholeBaseline of one cropped luma line with radius n: the lowest (cost_q, rank(q)) of the candidates not dropped.
    trail (a list) receives, in rank order, every q that was the best so far when it was decoded."""
    best = None
    for q in B.candidates(n):  # in rank order: a strict < keeps the lowest rank of equal costs
        if m.dropped(q):
            continue
        w = whole_line_q(m, ref, q)
        if best is None or w.cost < best.cost:
            best = WholeBaseline(w.text, w.idx, w.pens, w.cost, q)
            if trail is not None:
                trail.append(q)
    return best


def search_image(m, page, x, y, width, line_height, line_advance, n, trails=None):
    """[(y, WholeBaseline)] of every non-blank line of a page, as FastModel.decode_image walks it.  trails (a list)
    receives one trail per line (search_line)."""
    out = []
    i = 0
    while True:
        ly = y + i * line_advance
        i += 1
        line = crop(page, x, ly, width, line_height)
        if line.shape[0] == 0:
            return out
        if not np.all(line == 255):
            trail = []
            out.append((ly, search_line(m, line, n, trail)))
            if trails is not None:
                trails.append(trail)


def verify_image(page, lines, df, vf, x, y_bits):
    """draw_verify after such a run: lines is [(y, text, uint32 pens, q)]; each line's canvas is composed with every
    character at pos = s / 64 of its pen s, drawn row_shift(q) rows below y and clipped to the page at its top as well as
    its bottom and right.  Returns (image, exact sum of (R - B)^2)."""
    H, W = page.shape
    out = np.zeros((H, W, 3), dtype=np.uint8)
    out[..., 0] = np.where(page != 255, page, 0)
    for ly, text, pens, q in lines:
        idx = [df.alphabet.index(ch) for ch in text]
        c = compose_line_at(df, vf, idx, [F32(int(s)) / F32(64) for s in pens])
        top = ly + B.row_shift(q, y_bits)
        skip = max(0, -top)
        hh, ww = min(c.shape[0], H - top), min(c.shape[1], W - x)
        if hh > skip and ww > 0:
            c = c[skip:hh, :ww]
            np.copyto(out[top + skip: top + hh, x: x + ww, 2], 255 - c, where=c != 0)
    d = out[..., 0].astype(np.int64) - out[..., 2].astype(np.int64)
    return out, int((d * d).sum())

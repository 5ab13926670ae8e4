"""The focr decoder's whole-line decode with pen slack, restated for the tests (focr_decoder_set_whole_slack,
LineDecoder.decode(whole_line=True, pen_slack=N)).

The definition of include/focr_decode.h on FastModel.scores (tests/focr_fast_model.py), in the names of
tests/focr_whole_model.py: states are pens in 1/64 px; a step moves the pen by an offset j, -N <= j <= N, before the
glyph is rendered, and the offset is carried forward.  cost[0] = 0.  A render pen p < 64 * w takes G[p], the lowest
(cost[p - j], rank(j)) over the reachable states p - j in [0, 64 * w), rank the pen search's (0, -1, +1, -2, ...), and
remembers that j; cost[t] is the minimum over glyphs i of G[t - inc64[i]] + term(i, t - inc64[i]), the glyph remembered
for t the one with the lowest (cost, i); the line ends in the reachable t >= 64 * w with the lowest (cost[t], t), and
the read-back alternates glyph, render pen and offset.  A state t is final once every render pen below t - min inc64
has been visited, and a window reaches N <= min inc64 / 2 past its pen, so visiting the render pens in ascending order
sees only final costs.  Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_whole_model as W
from focr_search_model import rank

INF = W.INF

Slack = collections.namedtuple("Slack", "text idx pens offsets cost base states")


def max_slack(increments):
    """The largest N focr_decoder_run accepts for a font: 2 * N <= min inc64, at most 64."""
    return min(64, int(W.inc64(increments).min()) // 2)


def char_bound(increments, w, n):
    """The exact bound on a result's characters: ceil(64 * w / (min inc64 - N))."""
    m = int(W.inc64(increments).min()) - n
    return max(-(-64 * w // m), 1)


def batch(increments, n):
    """B of DESIGN.md 4b-4: render pens per batch on the device."""
    return min(int(W.inc64(increments).min()) - n, 512)


def slack_line(fm, ref, n, term=W.term_from_scores):
    """Slack of one cropped luma line (h x w uint8) by the FastModel fm with slack radius n.  idx: alphabet indices;
    pens: each character's render pen p (uint32, 1/64 px); offsets: its j (int8); cost: the sum of the terms along the
    text; base: the crop's sum of r^2; states: how many render pens rendered anything."""
    h, w = ref.shape
    r = 255 - ref.astype(np.int64)
    total = int((r * r).sum())
    inc = W.inc64(fm.incs)
    assert inc.min() >= 1 and float(fm.ox) == int(fm.ox) >= 0 and 0 <= 2 * n <= inc.min()
    n_live = 64 * w
    js = sorted(range(-n, n + 1), key=rank)
    cost = np.full(n_live + int(inc.max()), INF, dtype=np.int64)
    glyph = np.full(len(cost), -1, dtype=np.int64)
    off = np.zeros(n_live, dtype=np.int64)
    cost[0] = 0
    states = 0
    for p in range(n_live):
        g, gj = INF, 0
        for j in js:  # rank order and a strict compare: the lowest (cost, rank)
            s = p - j
            if 0 <= s < n_live and cost[s] < g:
                g, gj = int(cost[s]), j
        if g == INF:
            continue
        states += 1
        off[p] = gj
        c = term(fm, r, total, p)
        for i in range(len(inc)):  # the lowest (cost, i), also against a glyph of another advance pushed from a lower pen
            t = p + int(inc[i])
            if (g + int(c[i]), i) < (int(cost[t]), int(glyph[t]) if glyph[t] >= 0 else len(inc)):
                cost[t], glyph[t] = g + int(c[i]), i
    end = n_live + int(np.argmin(cost[n_live:]))  # the first minimum: the lowest (cost, t)
    assert cost[end] != INF
    idx, pens, offs, t = [], [], [], end
    while t > 0:
        i = int(glyph[t])
        p = t - int(inc[i])
        j = int(off[p])
        idx.append(i), pens.append(p), offs.append(j)
        t = p - j
    idx, pens, offs = idx[::-1], pens[::-1], offs[::-1]
    return Slack("".join(fm.alphabet[i] for i in idx), np.array(idx, dtype=np.uint16), np.array(pens, dtype=np.uint32),
                 np.array(offs, dtype=np.int8), int(cost[end]), total, states)


def check_invariants(fm, s):
    """pens[0] == offsets[0], and pens[q + 1] - offsets[q + 1] == pens[q] + inc64[idx[q]]."""
    inc = W.inc64(fm.incs)
    p, j = s.pens.astype(np.int64), s.offsets.astype(np.int64)
    assert len(p) == len(j) == len(s.idx) == len(s.text)
    if len(p):
        assert p[0] == j[0]
        assert np.array_equal(p[1:] - j[1:], p[:-1] + inc[s.idx[:-1]])


# ---- the pages of the tests ------------------------------------------------------------------------------------------

def draw_at(font, size, alphabet, text, pens64, width, height=None):
    """A luma line of `text` with character q drawn by FreeType at the pen pens64[q] / 64 px on the decoder's own line
    canvas (origin of `alphabet`; kerning 1, unhinted), as focr_whole_model.draw_line draws at the font's own pens."""
    from font_ocr_amd.decoder import DecodeFont, raster_glyph
    f = DecodeFont(font, size, alphabet)
    ox, oy = f.origin
    f.close()
    h = W.alphabet_height(font, size, alphabet) if height is None else height
    page = np.full((h, width), 255, dtype=np.uint8)
    for ch, p in zip(text, pens64):
        g = np.zeros((h, width), dtype=np.uint8)
        raster_glyph(font, size, ch, W.F32(ox + W.F32(int(p)) / W.F32(64)), oy, g)
        page = np.minimum(page, 255 - g)
    return page


def font_pens(fm, text, start=0):
    """The states the whole-line programme gives `text`: the running sum of inc64 from `start`."""
    inc = W.inc64(fm.incs)
    return start + np.concatenate([[0], np.cumsum([int(inc[fm.alphabet.index(c)]) for c in text[:-1]])]).astype(np.int64)

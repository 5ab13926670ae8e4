"""The per-character margins of the focr whole-line decode, restated for the tests (focr_decoder_set_whole_margins,
LineDecoder.decode(whole_line=True, margins=True)).

The definition of include/focr_decode.h with two tables on FastModel.scores (tests/focr_fast_model.py), in the names of
tests/focr_whole_model.py: F[t] is the whole-line programme's forward cost (F[0] = 0, the glyph remembered for t the one
with the lowest (cost, i), the line's end the reachable t >= 64 * w with the lowest (F[t], t)); B[t] = 0 for t >= 64 * w
and B[s] = min over i of term(i, s) + B[s + inc64[i]] below; character k (glyph i_k, pen s_k) has the midpoint
m_k = s_k + (inc64[i_k] >> 1); an edge (s, i) covers it when s is reachable and s <= m_k < s + inc64[i], and costs
T = F[s] + term(i, s) + B[s + inc64[i]]; the runner is the glyph i != i_k with the lowest (T, i) over the covering edges
and the margin that T less the line's cost (0xFFFF and -1 without such an edge).  forbid() is the other side of the cut
identity: a term for focr_whole_model.whole_line that takes glyph i_k out of every state that covers m_k.
Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_whole_model as W

NO_RUNNER = 0xFFFF
INF = np.iinfo(np.int64).max
DEAR = 1 << 40  # a term no path can afford: far above any line's cost, far below int64's end

Margins = collections.namedtuple("Margins", "text idx pens cost base term runner margin b0 runner_pen")


def margins_line(fm, ref):
    """Margins of one cropped luma line (h x w uint8) by the FastModel fm.  text, idx, pens, cost and base are the
    whole-line result (focr_whole_model.Whole); term (int32), runner (uint16 alphabet indices) and margin (int64) are per
    character; b0 is B[0]; runner_pen is, for the tests' own assertions (the decoder does not report it), the lowest state
    s of an edge (s, runner) that covers the midpoint at the runner's through-cost (-1 without a runner)."""
    h, w = ref.shape
    r = 255 - ref.astype(np.int64)
    total = int((r * r).sum())
    inc = W.inc64(fm.incs)
    assert inc.min() >= 1 and float(fm.ox) == int(fm.ox) >= 0
    n_live, top, at = 64 * w, int(inc.max()), np.arange(len(inc))
    # forward: F, the remembered glyphs, and every reachable state's terms
    F = np.full(n_live + top, INF, dtype=np.int64)
    glyph = np.full(len(F), -1, dtype=np.int64)
    terms = {}
    F[0] = 0
    for s in range(n_live):
        if F[s] == INF:
            continue
        terms[s] = W.term_from_scores(fm, r, total, s)
        cand, t = F[s] + terms[s], s + inc
        order = np.lexsort((at, cand, t))  # by target, then (cost, i): the first of every target is the one to push
        first = order[np.r_[True, np.diff(t[order]) != 0]]
        c1, t1 = cand[first], t[first]
        better = (c1 < F[t1]) | ((c1 == F[t1]) & (first < glyph[t1]))
        F[t1[better]], glyph[t1[better]] = c1[better], first[better]
    end = n_live + int(np.argmin(F[n_live:]))  # the first minimum: the lowest (F[t], t)
    assert F[end] != INF
    cost = int(F[end])
    idx, pens, t = [], [], end
    while t > 0:
        i = int(glyph[t])
        t -= int(inc[i])
        idx.append(i)
        pens.append(t)
    idx, pens = idx[::-1], pens[::-1]
    # backward: B over the reachable states (the targets of a reachable state are reachable)
    B = np.zeros(n_live + top, dtype=np.int64)
    for s in range(n_live - 1, -1, -1):
        if s in terms:
            B[s] = int((terms[s] + B[s + inc]).min())
    # per character: the lowest (T, i) over the covering edges of another glyph
    term, runner, margin, runner_pen = [], [], [], []
    for i_k, s_k in zip(idx, pens):
        m = s_k + (int(inc[i_k]) >> 1)
        best = None
        for s in range(max(0, m - top + 1), m + 1):
            if s not in terms:
                continue
            covers = (s + inc > m) & (at != i_k)
            if not covers.any():
                continue
            T = np.where(covers, F[s] + terms[s] + B[s + inc], INF)
            i = int(np.lexsort((at, T))[0])
            if best is None or (int(T[i]), i) < best[:2]:
                best = (int(T[i]), i, s)
        term.append(int(terms[s_k][i_k]))
        runner.append(best[1] if best else NO_RUNNER)
        margin.append(best[0] - cost if best else -1)
        runner_pen.append(best[2] if best else -1)
    return Margins("".join(fm.alphabet[i] for i in idx), np.array(idx, dtype=np.uint16), np.array(pens, dtype=np.uint32), cost, total,
                   np.array(term, dtype=np.int32), np.array(runner, dtype=np.uint16), np.array(margin, dtype=np.int64), int(B[0]),
                   np.array(runner_pen, dtype=np.int64))


def runner_text(fm, runner):
    """The runners as LineDecoder returns them: one character each, "\\0" where there is none."""
    return "".join("\0" if i == NO_RUNNER else fm.alphabet[i] for i in runner)


def forbid(fm, i_k, m_k):
    """A term for focr_whole_model.whole_line: term_from_scores, with glyph i_k prohibitively dear at every state s that
    covers the point m_k (s <= m_k < s + inc64[i_k])."""
    span = int(W.inc64(fm.incs)[i_k])

    def term(fm_, r, total, s):
        out = W.term_from_scores(fm_, r, total, s).copy()
        if s <= m_k < s + span:
            out[i_k] = DEAR
        return out

    return term

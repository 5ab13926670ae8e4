"""focr_decoder_align_text (include/focr_decode.h, LineDecoder.align_text), restated for the tests.

The definition, state by state: character g of the line has the nominal pen m_g = start + the running sum of inc64 (the
whole-line programme's rint(increment * 64)); a state (g, e), -W <= e <= W, is live when m_g + e >= 0 and its term T(g, e) is the
footprint term of the glyph at the pen m_g + e; F(0, e) = T(0, e), F(g, e) = T(g, e) + the lowest (F(g - 1, e - d), rank(d)) over
d in -N ..= N among the reachable states of the band; the line ends in the lowest (F(n - 1, e), rank(e)) and is walked back.
The terms come from focr_whole_model.term_from_scores on a FastModel (fast_term: the full-canvas SSD at pos = pen / 64 less
the crop's sum of r^2), computed once per pen and kept; raster_term is the same number from one FreeType raster per glyph and
pen (focr_score_text_model.terms), for a candidate font or a baseline candidate q.  Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_score_text_model as S
import focr_whole_model as W
from focr_search_model import rank

Align = collections.namedtuple("Align", "base cost first last pens terms")


def nominal(increments, idx, start=0):
    """m_g of the line idx (alphabet indices): start + the running sum of inc64."""
    inc = W.inc64(increments)
    out, pen = [], int(start)
    for i in idx:
        out.append(pen)
        pen += int(inc[i])
    return out


def fast_term(fm, ref, idx):
    """term(g, pen) of the line idx on the cropped luma line ref by the FastModel fm: every glyph's term at a pen is worked out
    once and kept."""
    r = 255 - ref.astype(np.int64)
    total = int((r * r).sum())
    assert float(fm.ox) == int(fm.ox) >= 0
    kept = {}

    def term(g, pen):
        if pen not in kept:
            kept[pen] = W.term_from_scores(fm, r, total, pen)
        return int(kept[pen][idx[g]])

    return term


def raster_term(font, ref, idx, q=0, y_bits=0):
    """term(g, pen) from one FreeType raster per (glyph, pen): any DecodeFont, under baseline candidate q."""
    ox = font.origin[0]
    assert float(ox) == int(ox) >= 0
    kept = {}

    def term(g, pen):
        key = (idx[g], pen)
        if key not in kept:
            kept[key] = int(S.terms(font, ref, [idx[g]], [64 * int(ox) + pen], q, y_bits)[0])
        return kept[key]

    return term


def base_of(ref):
    r = 255 - ref.astype(np.int64)
    return int((r * r).sum())


def align(term, nom, drift, step, base=0):
    """Align of a line with the nominal pens nom under term(g, pen), drift radius W and step radius N."""
    n = len(nom)
    if n == 0:
        return Align(base, 0, 0, 0, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64))
    ds = sorted(range(-step, step + 1), key=rank)  # in rank order: a strict < keeps the lowest rank of equal costs
    rows, backs = [], []
    for g in range(n):
        row, back = {}, {}
        for e in range(-drift, drift + 1):
            if nom[g] + e < 0:
                continue  # not live
            if g == 0:
                best, bd = 0, 0
            else:
                best, bd = None, 0
                for d in ds:
                    v = rows[-1].get(e - d)
                    if v is not None and (best is None or v < best):
                        best, bd = v, d
                if best is None:
                    continue  # unreachable
            row[e], back[e] = best + term(g, nom[g] + e), bd
        rows.append(row)
        backs.append(back)
    last = min(rows[-1], key=lambda e: (rows[-1][e], rank(e)))
    es, e = [0] * n, last
    for g in range(n - 1, -1, -1):
        es[g] = e
        e -= backs[g][e]
    pens = [nom[g] + es[g] for g in range(n)]
    terms = [term(g, pens[g]) for g in range(n)]
    assert sum(terms) == rows[-1][last]
    return Align(base, rows[-1][last], es[0], last, np.array(pens, dtype=np.uint32), np.array(terms, dtype=np.int64))


def align_crop(fm, ref, idx, start, drift, step, term=None, increments=None):
    """Align of the line idx against the cropped luma line ref by the FastModel fm (or under `term` with `increments`)."""
    return align(term or fast_term(fm, ref, idx), nominal(fm.incs if increments is None else increments, idx, start), drift, step, base_of(ref))


def brute(term, nom, drift, step, base=0):
    """The same line by enumeration of every offset path e_0 .. e_{n-1}: the lowest cost, and among equal costs the path the
    definition's tie rules pick: the lowest rank(e_{n-1}), then walking back the lowest rank(e_g - e_{g-1}) at every step among
    the paths that are cheapest up to there."""
    n = len(nom)
    if n == 0:
        return Align(base, 0, 0, 0, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64))
    band = range(-drift, drift + 1)

    def paths(g, e):  # every path that ends in (g, e) with its cost
        if nom[g] + e < 0:
            return
        t = term(g, nom[g] + e)
        if g == 0:
            yield (e,), t
            return
        for p in band:
            if abs(e - p) <= step:
                for path, c in paths(g - 1, p):
                    yield path + (e,), c + t

    def best(g, e):  # the lowest cost of a path to (g, e), None when there is none
        return min((c for _, c in paths(g, e)), default=None)

    ends = {e: best(n - 1, e) for e in band}
    last = min((e for e in band if ends[e] is not None), key=lambda e: (ends[e], rank(e)))
    es, e = [0] * n, last
    for g in range(n - 1, 0, -1):
        es[g] = e
        cands = [(best(g - 1, e - d), rank(d), d) for d in range(-step, step + 1) if -drift <= e - d <= drift and best(g - 1, e - d) is not None]
        e -= min(cands)[2]
    es[0] = e
    pens = [nom[g] + es[g] for g in range(n)]
    terms = [term(g, pens[g]) for g in range(n)]
    assert sum(terms) == ends[last]
    return Align(base, ends[last], es[0], last, np.array(pens, dtype=np.uint32), np.array(terms, dtype=np.int64))

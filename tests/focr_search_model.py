"""The focr decoder's pen search, restated for the tests (focr_decoder_set_pen_search, LineDecoder.decode(pen_search=N)).

The definition of include/focr_decode.h on FastModel.scores (tests/focr_fast_model.py): at a step with the f32 pen pos,
the candidates are (glyph i, offset j) for j in -N ..= N at the pen p_j = pos + j / 64 (one f32 add), dropped where
origin_x + p_j is negative; a candidate's score is the full-canvas SSD with the pen at p_j; the step takes the lowest
(score, rank(j), i), rank(0) = 0, rank(-1) = 1, rank(+1) = 2, ..., and the pen becomes p_j + increment[i].  The runner
of a step is the best candidate, at any offset, of another glyph.  brute_search_line is the same walk with every
candidate rasterised by FreeType at origin_x + p_j (tests/focr_line_model.py's primitives), and verify_image is
draw_verify with every character at the pen the search chose for it, composed from the decode and verify tables as
tests/test_focr_verify_host.py's compose_line does for the plain pens.  Nothing here comes from the device path.
"""
import collections

import numpy as np

import focr_line_model as M
from focr_fast_model import crop
from font_ocr_amd.decoder import DecodeFont, raster_glyph

F32 = np.float32
NO_RUNNER = 0xFFFF
INT64_MAX = np.iinfo(np.int64).max
STEP = F32(0.015625)

Searched = collections.namedtuple("Searched", "text offsets pens base score runner runner_score second_is_own")


def rank(j):
    return 0 if j == 0 else (2 * -j - 1 if j < 0 else 2 * j)


def max_radius(increments):
    """The largest N focr_decoder_run accepts for a font: N / 64 <= min_increment / 2, at most 64."""
    return min(64, int(np.floor(F32(np.min(increments)) * F32(0.5) * F32(64))))


def search_cap(increments, w, n):
    """The decoder's characters-per-line bound with a search radius n > 0: steps of (q - n / 64) + min_increment in f32."""
    m, reach, p, steps = F32(np.min(increments)), F32(n) * STEP, F32(0), 0
    while p < F32(w):
        p = F32(F32(p - reach) + m)
        steps += 1
    return max(steps, 1)


def _offsets(n):
    """-n ..= n in rank order: 0, -1, 1, -2, 2, ..."""
    return sorted(range(-n, n + 1), key=rank)


def _step(js, pens, s):
    """js, pens: a step's offsets in rank order and their pens (None: dropped); s[k]: the int64 scores of every glyph
    at js[k].  Returns (the best, the best of another glyph or None, whether the second lowest key of all is another
    offset of the best's glyph), each candidate as (score, rank, glyph, j, pen).  In rank-major order the first minimum
    of the flat array is the lowest (score, rank, glyph)."""
    a = np.full((len(js), len(next(v for v in s if v is not None))), INT64_MAX, dtype=np.int64)
    for k, v in enumerate(s):
        if v is not None:
            a[k] = v
    G = a.shape[1]

    def lowest(m):
        k, i = divmod(int(np.argmin(m)), G)
        return (int(m[k, i]), k, i, js[k], pens[k]) if m[k, i] != INT64_MAX else None

    best = lowest(a)
    rest = a.copy()
    rest[best[1], best[2]] = INT64_MAX
    second = lowest(rest)
    rest[:, best[2]] = INT64_MAX
    return best, lowest(rest), second is not None and second[2] == best[2]


def _searched(alphabet, r, steps):
    return Searched("".join(alphabet[b[2]] for b, _, _ in steps), np.array([b[3] for b, _, _ in steps], dtype=np.int8),
                    np.array([b[4] for b, _, _ in steps], dtype=np.float32), int((r * r).sum()),
                    np.array([b[0] for b, _, _ in steps], dtype=np.int64),
                    np.array([o[2] if o else NO_RUNNER for _, o, _ in steps], dtype=np.uint16),
                    np.array([o[0] if o else INT64_MAX for _, o, _ in steps], dtype=np.int64),
                    np.array([own for _, _, own in steps], dtype=bool))


def search_line(fm, ref, n):
    """Searched of one cropped luma line (h x w uint8) by the FastModel fm with radius n."""
    r = 255 - ref.astype(np.int64)
    pos, steps = F32(0), []
    while pos < F32(ref.shape[1]):
        js = _offsets(n)
        pens = [F32(pos + F32(j) * STEP) for j in js]
        pens = [pj if F32(fm.ox + pj) >= 0 else None for pj in pens]
        steps.append(_step(js, pens, [fm.scores(r, pj) if pj is not None else None for pj in pens]))
        best = steps[-1][0]
        pos = F32(best[4] + fm.incs[best[2]])
    return _searched(fm.alphabet, r, steps)


def search_image(fm, page, x, y, width, line_height, line_advance, n):
    """[(y, Searched)] of every non-blank line of a page, as FastModel.decode_image walks it."""
    out = []
    i = 0
    while True:
        ly = y + i * line_advance
        i += 1
        line = crop(page, x, ly, width, line_height)
        if line.shape[0] == 0:
            return out
        if not np.all(line == 255):
            out.append((ly, search_line(fm, line, n)))


def brute_search_line(ref, font, size, alphabet, n, kerning=1.0, hinting=False):
    """Searched of one cropped luma line with one FreeType raster per candidate per step and the full-canvas int64 SSD."""
    h, w = ref.shape
    r = 255 - ref.astype(np.int64)
    ox, oy = M.origin(font, size, alphabet)
    incs = [M.increment(font, size, ch, kerning) for ch in alphabet]
    pos, steps = F32(0), []
    canvas = np.zeros((h, w), dtype=np.uint8)
    while pos < F32(w):
        js = _offsets(n)
        pens = [F32(pos + F32(j) * STEP) for j in js]
        pens = [pj if F32(ox + pj) >= 0 else None for pj in pens]
        s = []
        for pj in pens:
            s.append(None if pj is None else np.zeros(len(alphabet), dtype=np.int64))
            for i, ch in enumerate(alphabet if pj is not None else ""):
                canvas[:] = 0
                M.raster_glyph(font, size, ch, F32(ox + pj), oy, canvas, hinting)
                s[-1][i] = int(((r - canvas.astype(np.int64)) ** 2).sum())
        steps.append(_step(js, pens, s))
        best = steps[-1][0]
        pos = F32(best[4] + incs[best[2]])
    return _searched(alphabet, r, steps)


# ---- pages whose text does not sit where the font's advances put it --------------------------------------------------

def draw_snapped(page, font, size, alphabet, text, x, y, snap="exact", advance=1.0):
    """Darken rows y .. of `page` from column x with `text`, each glyph rasterised by FreeType on the decoder's own
    line canvas (origin of `alphabet`) at a pen that advances by increment * advance in f32 and is drawn "exact",
    rounded to whole pixels ("round") or floored ("floor").  Clipped to the page."""
    f = DecodeFont(font, size, alphabet)
    inc, (ox, oy) = f.increments(), f.origin
    f.close()
    H, W = page.shape
    h, w = min(int(np.ceil(size)) + 3, H - y), W - x
    pen = F32(0)
    for ch in text:
        at = {"exact": pen, "round": F32(np.floor(pen + F32(0.5))), "floor": F32(np.floor(pen))}[snap]
        g = np.zeros((h, w), dtype=np.uint8)
        raster_glyph(font, size, ch, F32(ox + at), oy, g)
        page[y: y + h, x: x + w] = np.minimum(page[y: y + h, x: x + w], 255 - g)
        pen = F32(pen + F32(inc[alphabet.index(ch)] * F32(advance)))
    return page


# ---- draw_verify at the searched pens --------------------------------------------------------------------------------

def compose_line_at(df, vf, idx, pens):
    """render() of the alphabet indices idx with glyph q at the f32 pen pens[q] instead of the running sum of the
    increments: the union of round_out boxes from the empty rect at (0, 0), each glyph's true phase rectangle copied in
    text order at delta trunc((-ox + pen) * 64), clipped to the canvas."""
    ox = oy = lx = ly = 0
    for c, p in zip(idx, pens):
        b = vf.box(c)
        ox, lx = min(ox, int(np.floor(F32(b[0] + p)))), max(lx, int(np.ceil(F32(b[2] + p))))
        oy, ly = min(oy, int(np.floor(F32(b[1] + F32(0))))), max(ly, int(np.ceil(F32(b[3] + F32(0)))))
    cw, ch = lx - ox, ly - oy
    canvas = np.zeros((ch, cw), dtype=np.uint8)
    dy = -oy - int(vf.s.origin_y)
    for c, p in zip(idx, pens):
        d = int(F32(F32(F32(-ox) + p) * F32(64)))
        phase, shift = d & 63, d >> 6
        bm, offx, offy = df.phase(c, phase)
        rx, ry, rw, rh = vf.rect(c, phase)
        x0, y0 = shift + offx + rx, offy + ry + dy
        src = bm[ry: ry + rh, rx: rx + rw]
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x0 + rw, cw), min(y0 + rh, ch)
        if cx0 < cx1 and cy0 < cy1:
            canvas[cy0:cy1, cx0:cx1] = src[cy0 - y0: cy1 - y0, cx0 - x0: cx1 - x0]
    return canvas


def plain_pens(df, idx):
    """The pens render() gives the alphabet indices idx: the running f32 sum of their increments."""
    incs, pens, pen = df.increments(), [], F32(0)
    for c in idx:
        pens.append(pen)
        pen = F32(pen + incs[c])
    return pens


def verify_image(page, lines, df, vf, x):
    """tests/focr_line_model.py's verify_image with every line composed at its own pens: lines is [(y, text, pens)].
    Returns (image, exact sum of (R - B)^2)."""
    H, W = page.shape
    out = np.zeros((H, W, 3), dtype=np.uint8)
    out[..., 0] = np.where(page != 255, page, 0)
    for ly, text, pens in lines:
        c = compose_line_at(df, vf, [df.alphabet.index(ch) for ch in text], pens)
        hh, ww = min(c.shape[0], H - ly), min(c.shape[1], W - x)
        if hh > 0 and ww > 0:
            c = c[:hh, :ww]
            np.copyto(out[ly: ly + hh, x: x + ww, 2], 255 - c, where=c != 0)
    d = out[..., 0].astype(np.int64) - out[..., 2].astype(np.int64)
    return out, int((d * d).sum())

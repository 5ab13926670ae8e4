"""Cases and plain-numpy references for the phase-by-phase tests of the MFMA prefilter (tests/test_gpu_prefilter_model.py on the
device, tests/test_prefilter_host.py on the CPU).  A case is a small bank, a few ink-high pages and a threshold, built from a seed;
`vacuity` says, from the host model alone, whether the case has what makes the device checks mean something (emitting pairs,
candidates that do not emit, pairs just under the threshold, blank and live statistics tiles), so that is known before any GPU time
is spent.  Pairs just under / just over the threshold are too rare to wait for (a band of S = 32 .. 512 in sums of ~1e5): `tune`
builds one of each by bisection between a template and its negative and single-pixel steps, asking the model for d = G + C-in."""
import os

import numpy as np

from font_ocr_amd import synth_page
from font_ocr_amd.bank import SYNTH_SEED_BASE, TEMPLATE_DTYPE, Bank
from font_ocr_amd.searcher import PREFILTER_AUTO, PREFILTER_LEGACY, prefilter_page_model

NEVER = -32768
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bank_of(needles):
    tm, flat, off = [], [], 0
    for nd in needles:
        t = np.zeros(1, TEMPLATE_DTYPE)
        t["letter"], t["n_w"], t["n_h"], t["offset"] = 33 + len(tm), nd.shape[1], nd.shape[0], off
        tm.append(t)
        flat.append(nd.reshape(-1).astype(np.uint8))
        off += nd.size
    return Bank(np.concatenate(tm), np.concatenate(flat), len(tm), 0, 0, 13.0, 8.0)


# id -> classes [(n_w, n_h, templates, indices of constant templates)], (pages, r_w, r_h), threshold, options
#   blank: pages left blank; drop: column drop; prefilter; pages: "noise" (default) / "saturated" / "bench"
# (Thresholds at or below 0 go with narrow pages or few templates: most pairs emit there, and a page row with more than 4096 hits sends
# the scan with estimated sizes to the legacy tail, which leaves no candidate list to read back.)
CASES = {
    # LAYOUT_W8 at 1, 2, 3, 4 K-steps, one class per pass, register form (kept width 8 / 4); 1 / 15 / 16 / 17 templates per class
    "w8-ksteps": dict(classes=[(8, 8, 1, ()), (8, 16, 15, ()), (8, 24, 16, ()), (8, 32, 17, ()), (4, 7, 3, ())], geom=(3, 97, 40), thr=0.8),
    # LAYOUT_W16 at 1 .. 4 K-steps and 16x17 (n > 256, 5 K-steps: the legacy kernel's int32 tables); 33 templates = three N-tiles
    "w16-ksteps": dict(classes=[(16, 4, 17, ()), (16, 8, 33, ()), (14, 12, 1, ()), (16, 16, 16, ()), (16, 17, 15, ())], geom=(3, 65, 50), thr=0.3),
    # LAYOUT_W12 (3 K-steps, the only count the plane kernel has for it): four classes in one pass, the 8-wide one riding the 12-byte rows
    "w12-four": dict(classes=[(12, 15, 17, ()), (10, 16, 5, ()), (11, 7, 16, ()), (8, 15, 4, ())], geom=(3, 301, 37), thr=0.3),
    "drop9": dict(classes=[(9, 15, 17, ())], geom=(3, 64, 24), thr=0.8),                       # DROP alone; a page below one 32-row band
    "drop13": dict(classes=[(13, 16, 17, ())], geom=(3, 97, 40), thr=0.8),                                 # 13 -> 12 kept columns alone: DROP with no kept box beside it, on the planes
    # n > 256 on the planes (32-bit multiplies in the statistics): 9x32 keeps 8 columns, 4 K-steps; alone (DROP) and beside 8x32 (PAIR)
    "drop9-tall": dict(classes=[(9, 32, 5, ())], geom=(3, 97, 70), thr=0.3),
    "pair9-tall": dict(classes=[(9, 32, 5, ()), (8, 32, 4, ())], geom=(3, 97, 70), thr=0.3),
    "pair9": dict(classes=[(9, 15, 17, ()), (8, 15, 16, ())], geom=(3, 1021, 40), thr=0.3),              # PAIR; strips of 240 columns
    "pair9-neg": dict(classes=[(9, 15, 5, ()), (8, 15, 5, ())], geom=(3, 97, 34), thr=-0.9),
    "pair13": dict(classes=[(13, 16, 17, ()), (12, 16, 3, ())], geom=(3, 97, 70), thr=0.8),                # 13 -> 12 kept columns, PAIR on 12-byte rows
    "drop13-n416": dict(classes=[(13, 32, 4, ())], geom=(3, 65, 66), thr=0.3),                             # 13x32: n > 256, 6 K-steps -> legacy kernel, DROP into int32 tables
    "nodrop": dict(classes=[(9, 15, 17, ()), (13, 14, 6, ())], geom=(3, 65, 40), thr=0.3, drop=False),     # every column multiplied: 9 -> 12-byte rows, 13 -> 16
    # kept widths the register form does not take (LDS form): 5, 7, 6 (8-byte rows, 2 / 2 / 4 K-steps) and 15 (16-byte rows)
    "lds-widths": dict(classes=[(5, 9, 6, ()), (7, 12, 17, ()), (6, 30, 3, ()), (15, 10, 5, ())], geom=(3, 97, 50), thr=0.0),
    # six classes that share one pass: more than the plane kernel's four values -> the legacy kernel for all of them
    "six-in-a-pass": dict(classes=[(8, 9, 3, ()), (7, 10, 3, ()), (6, 11, 3, ()), (5, 12, 3, ()), (4, 13, 3, ()), (3, 16, 3, ())], geom=(3, 65, 34), thr=0.3),
    # constant templates in the middle of the caller's order and enough of them to fill a whole N-tile (live ones take the first slots)
    "dead": dict(classes=[(8, 15, 40, (5, 20, 21)), (9, 15, 33, tuple(range(8, 25)))], geom=(3, 40, 40), thr=-0.25),
    # more N-tiles than one launch stages in LDS: 38 tiles of 4 K-steps (mfma2_chunk_tiles(4) = 37)
    "two-launches": dict(classes=[(16, 16, 600, ())], geom=(3, 48, 24), thr=0.3),
    "w17": dict(classes=[(8, 8, 5, ()), (16, 16, 5, ())], geom=(4, 17, 40), thr=0.0),           # one window column for the 16-wide class
    "saturated": dict(classes=[(16, 16, 9, ()), (9, 15, 9, ())], geom=(6, 97, 70), thr=0.3, pages="saturated"),
    "bench": dict(classes=None, geom=(1, 608, 720), thr=0.8, pages="bench"),                               # the benchmark's page shape, 40 templates of its bank
    "clamp-hi": dict(classes=[(9, 15, 5, ()), (8, 15, 5, ())], geom=(3, 64, 24), thr=1000.0, vacuous_ok=True),   # planes at -32767: nothing passes
    "clamp-lo": dict(classes=[(9, 15, 5, ()), (8, 15, 5, ())], geom=(3, 64, 24), thr=-1000.0, vacuous_ok=True),  # planes at +32767: every pair passes
    "legacy-prefilter": dict(classes=[(9, 15, 17, ()), (8, 15, 16, ())], geom=(3, 97, 40), thr=0.8, prefilter=PREFILTER_LEGACY),
}


# What each case is there for, pinned: per class (n_w, n_h) -> (kept width, K layout (1: 16-byte rows, 2: 8, 3: 12), K-steps, pass, True if the
# pass takes the threshold planes / False: the legacy kernel's int32 tables).  A change to layout_supers or pass_planes that moves a case
# onto another path fails tests/test_prefilter_host.py::test_gpu_prefilter_cases_are_not_vacuous instead of passing unnoticed.
EXPECT = {
    'w8-ksteps': {(4, 7): (4, 2, 1, 3, True), (8, 8): (8, 2, 1, 3, True), (8, 16): (8, 2, 2, 0, True), (8, 24): (8, 2, 3, 1, True), (8, 32): (8, 2, 4, 2, True)},
    'w16-ksteps': {(14, 12): (14, 1, 3, 4, True), (16, 4): (16, 1, 1, 1, True), (16, 8): (16, 1, 2, 0, True), (16, 16): (16, 1, 4, 3, True), (16, 17): (16, 1, 5, 2, False)},
    'w12-four': {(8, 15): (8, 3, 3, 0, True), (10, 16): (10, 3, 3, 0, True), (11, 7): (11, 3, 3, 0, True), (12, 15): (12, 3, 3, 0, True)},
    'drop9': {(9, 15): (8, 2, 2, 0, True)},
    'drop13': {(13, 16): (12, 3, 3, 0, True)},
    'drop9-tall': {(9, 32): (8, 2, 4, 0, True)},
    'pair9-tall': {(8, 32): (8, 2, 4, 0, True), (9, 32): (8, 2, 4, 0, True)},
    'pair9': {(8, 15): (8, 2, 2, 0, True), (9, 15): (8, 2, 2, 0, True)},
    'pair9-neg': {(8, 15): (8, 2, 2, 0, True), (9, 15): (8, 2, 2, 0, True)},
    'pair13': {(12, 16): (12, 3, 3, 0, True), (13, 16): (12, 3, 3, 0, True)},
    'drop13-n416': {(13, 32): (12, 3, 6, 0, False)},
    'nodrop': {(9, 15): (9, 3, 3, 0, True), (13, 14): (13, 1, 4, 1, True)},
    'lds-widths': {(5, 9): (5, 2, 2, 0, True), (6, 30): (6, 2, 4, 1, True), (7, 12): (7, 2, 2, 0, True), (15, 10): (15, 1, 3, 2, True)},
    'six-in-a-pass': {(3, 16): (3, 2, 2, 0, False), (4, 13): (4, 2, 2, 0, False), (5, 12): (5, 2, 2, 0, False), (6, 11): (6, 2, 2, 0, False), (7, 10): (7, 2, 2, 0, False), (8, 9): (8, 2, 2, 0, False)},
    'dead': {(8, 15): (8, 2, 2, 0, True), (9, 15): (8, 2, 2, 0, True)},
    'two-launches': {(16, 16): (16, 1, 4, 0, True)},
    'w17': {(8, 8): (8, 2, 1, 0, True), (16, 16): (16, 1, 4, 1, True)},
    'saturated': {(9, 15): (8, 2, 2, 0, True), (16, 16): (16, 1, 4, 1, True)},
    'bench': {(8, 15): (8, 2, 2, 0, True), (9, 15): (8, 2, 2, 0, True)},
    'clamp-hi': {(8, 15): (8, 2, 2, 0, True), (9, 15): (8, 2, 2, 0, True)},
    'clamp-lo': {(8, 15): (8, 2, 2, 0, True), (9, 15): (8, 2, 2, 0, True)},
    'legacy-prefilter': {(8, 15): (8, 2, 2, 0, False), (9, 15): (8, 2, 2, 0, False)},
}
ODD_MTILES = ("saturated", "dead")  # cases with a pass whose live M-tile count is no multiple of the scan kernel's four M-tiles per item


def model(case, bank, page, want=("V", "W_upper", "L", "plane", "G", "sim")):
    return prefilter_page_model(bank, page, case["thr"], case.get("drop", True), case.get("prefilter", PREFILTER_AUTO), want)


def d_of(m, t):
    """G + C-in of template t over the page, int64 (negative beyond reach where the pair can never pass)."""
    k = int(m["templates"][t, 0])
    return m["G"][t].astype(np.int64) + (m["plane"][k].astype(np.int64) << int(m["classes"][k]["shift"]))


def tune(case, bank, t, rng, lo, hi):
    """An n_h x n_w window whose d for template t lies in (lo, hi]."""
    nd = bank.needle(t).astype(np.float64)
    h, w = nd.shape
    noise = rng.uniform(-15.0, 15.0, nd.shape)

    def win(b):
        return np.clip(np.rint(b * nd + (1.0 - b) * (255.0 - nd) + noise), 0, 255).astype(np.uint8)

    def d(wn):
        page = np.zeros((h + 1, w + 1), np.uint8)
        page[1:, 1:] = wn
        return int(d_of(model(case, bank, page, ("G", "plane")), t)[1, 1])

    a, b = 0.0, 1.0
    assert d(win(a)) <= lo and d(win(b)) > hi, (d(win(a)), d(win(b)), lo, hi)
    for _ in range(50):
        mid = 0.5 * (a + b)
        if d(win(mid)) <= lo:
            a = mid
        else:
            b = mid
    cur = win(a)
    dc = d(cur)
    centre = 0.5 * (lo + hi)
    for _ in range(40):
        if lo < dc <= hi:
            return cur
        best = None
        for i in range(h * w):
            for step in (1, -1):
                v = int(cur.flat[i]) + step
                if not 0 <= v <= 255:
                    continue
                trial = cur.copy()
                trial.flat[i] = v
                dt = d(trial)
                if lo < dt <= hi:
                    return trial
                if best is None or abs(dt - centre) < abs(best[0] - centre):
                    best = (dt, trial)
        dc, cur = best
    raise AssertionError(f"tune: no window with d in ({lo}, {hi}] for template {t}: stuck at {dc}")


def _saturated_pages(n_pages, r_w, r_h, rng):
    """The integer edges the statistics' 24-bit multiplies are sized for: maximal s and s2 with the smallest non-zero V (an all-255
    page with single pixels of 254 / 0), the largest V (0 / 255 checkerboards, half-planes), a one-pixel line that is a dropped
    column carrying all the ink of its window."""
    pg = np.zeros((n_pages, r_h, r_w), np.uint8)
    pg[0] = 255
    ys, xs = rng.integers(0, r_h, 24), rng.integers(0, r_w, 24)
    pg[0, ys[:12], xs[:12]] = 254
    pg[0, ys[12:], xs[12:]] = 0
    yy, xx = np.mgrid[0:r_h, 0:r_w]
    pg[1] = np.where((yy + xx) % 2 == 0, 255, 0)
    pg[1, :, r_w // 2:] = np.where((yy // 2 + xx // 3) % 2 == 0, 255, 0)[:, r_w // 2:]
    pg[2, :, : r_w // 3] = 255                    # half-planes: a vertical and a horizontal edge
    pg[2, r_h // 2:, r_w // 2:] = 255
    pg[3, :, 10::23] = 255                        # one-pixel lines on blank paper, and one of 254 on full ink
    pg[3, r_h // 2:, :] = 255
    pg[3, r_h // 2:, 17::29] = 254
    return pg                                     # (the last page is left to the textured content below)


def build(case_id):
    """-> (case, bank, pages): ink-high uint8 pages (n, r_h, r_w)."""
    case = CASES[case_id]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id)))
    n_pages, r_w, r_h = case["geom"]
    blank = case.get("blank", (1,) if n_pages >= 3 else ())  # a fully blank page between two others
    if case.get("pages") == "saturated":
        blank = tuple(range(n_pages - 1))  # (filled below; the fifth stays blank, the last is textured)
    if case.get("pages") == "bench":
        full = Bank.load(os.path.join(GOLD, "bank_dejavu13_ascii95_x2.bin"))
        bank = full.subset(list(range(33, 53)) + list(range(95 + 33, 95 + 53)))  # 20 glyphs at both sub-pixel shifts: 8x15 and 9x15
        pages = (255 - synth_page(full, SYNTH_SEED_BASE + 1, r_w, r_h))[None].copy()
        pages[0, r_h - 100:, r_w - 200:] = 0
        pages[0, :40, :40] = 0
    else:
        needles = []
        for n_w, n_h, count, dead in case["classes"]:
            for i in range(count):
                nd = rng.integers(0, 256, (n_h, n_w), dtype=np.uint8)
                if i % 3 == 1:
                    nd[rng.random(nd.shape) < 0.5] = 0  # glyph-like: half of it paper
                if i in dead:
                    nd[:] = int(rng.integers(0, 256))
                needles.append(nd)
        order = rng.permutation(len(needles))  # the classes interleaved, as a caller's bank may have them
        bank = bank_of([needles[i] for i in order])
        pages = np.zeros((n_pages, r_h, r_w), np.uint8)
        if case.get("pages") == "saturated":
            pages = _saturated_pages(n_pages, r_w, r_h, rng)
        for p in range(n_pages):
            if p in blank:
                continue
            pages[p] = rng.integers(0, 256, (r_h, r_w), dtype=np.uint8)
            pages[p][rng.random((r_h, r_w)) < 0.5] = 0
            if r_w >= 200:
                pages[p, :, 100:190] = 0  # blank paper under whole statistics tiles
    info = prefilter_page_model(bank, None, case["thr"], case.get("drop", True), case.get("prefilter", PREFILTER_AUTO))
    live = [t for t in range(len(bank)) if info["templates"][t, 2]]
    max_w, max_h = int(bank.templates["n_w"].max()), int(bank.templates["n_h"].max())
    textured = [p for p in range(n_pages) if p not in blank]
    spots = [(p, y, x) for p in textured for y in range(1, r_h - max_h + 1, max_h + 1) for x in range(1, r_w - max_w + 1, max_w + 1)]
    if case.get("pages") == "bench":
        spots = [(0, 1, 1), (0, 1, 12), (0, 20, 1)]
    plant = []
    if not case.get("vacuous_ok"):
        t0 = live[0]
        S = 1 << int(info["classes"][int(info["templates"][t0, 0])]["shift"])
        plant = [(t0, tune(case, bank, t0, rng, -S, 0)), (t0, tune(case, bank, t0, rng, 0, S))]
    for i, t in enumerate(live[: max(0, len(spots) - len(plant))][:24]):  # the templates themselves, increasingly blended with noise
        nd = bank.needle(t).astype(np.float64)
        b = 1.0 - 0.04 * (i % 12)
        plant.append((t, np.clip(np.rint(b * nd + (1.0 - b) * rng.uniform(0, 255, nd.shape)), 0, 255).astype(np.uint8)))
    for (p, y, x), (t, wn) in zip(spots, plant):
        pages[p, y:y + wn.shape[0], x:x + wn.shape[1]] = wn
    return case, bank, pages


def window_sums(page, n_w, n_h, keep_w, rows, cols):
    """Exact int64 statistics of the n_w x n_h windows at y < rows, x < cols of a page continued with blank paper: V = n*s2 - s^2 and
    W = n_k^2*q2 - 2*n_k*s_k*q1 + D*s_k^2 (q1, q2: sums over the columns from keep_w on; 0 if nothing is dropped), plain numpy."""
    big = np.zeros((rows + n_h, cols + n_w), np.int64)
    h, w = min(page.shape[0], big.shape[0]), min(page.shape[1], big.shape[1])
    big[:h, :w] = page[:h, :w]

    def box(a, x0, x1):  # sums over rows y .. y + n_h - 1, columns x + x0 .. x + x1 - 1
        c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
        c[1:, 1:] = a.cumsum(0).cumsum(1)
        return c[n_h:n_h + rows, x1:x1 + cols] - c[:rows, x1:x1 + cols] - c[n_h:n_h + rows, x0:x0 + cols] + c[:rows, x0:x0 + cols]

    s, s2 = box(big, 0, n_w), box(big * big, 0, n_w)
    n, n_k, D = n_w * n_h, keep_w * n_h, (n_w - keep_w) * n_h
    V = n * s2 - s * s
    W = np.zeros_like(V)
    if D:
        q1, q2 = box(big, keep_w, n_w), box(big * big, keep_w, n_w)
        s_k = s - q1
        W = n_k * n_k * q2 - 2 * n_k * s_k * q1 + D * s_k * s_k
    return V, W


def vacuity(case, bank, pages, models):
    """What the case holds, from the model alone: pairs that emit, candidates that do not, pairs with -S < d <= 0, blank and live 64x32
    statistics tiles (a tile is blank if the paper under it and under every window that starts in it is)."""
    thr = case["thr"]
    out = dict(emit=0, cand_no_emit=0, near=0, blank_tiles=0, live_tiles=0, missed=0)
    max_w, max_h = int(bank.templates["n_w"].max()), int(bank.templates["n_h"].max())
    for p, m in enumerate(models):
        for t in range(len(bank)):
            if not m["templates"][t, 2]:
                continue
            k = int(m["templates"][t, 0])
            S = 1 << int(m["classes"][k]["shift"])
            d = d_of(m, t)
            ok = m["plane"][k] != NEVER
            with np.errstate(invalid="ignore"):
                emit = m["sim"][t] > thr
            out["emit"] += int(emit.sum())
            out["missed"] += int((emit & ~(d > 0)).sum())
            out["cand_no_emit"] += int((ok & (d > 0) & ~emit).sum())
            out["near"] += int((ok & (d > -S) & (d <= 0)).sum())
        pg = pages[p]
        for y0 in range(0, pg.shape[0], 32):
            for x0 in range(0, pg.shape[1], 64):
                blank = not pg[y0:y0 + 32 + max_h - 1, x0:x0 + 64 + max_w].any()
                out["blank_tiles" if blank else "live_tiles"] += 1
    # live 16-window M-tiles per pass (the scan kernel takes them four at a time): those with a window that can emit in a class of the pass
    cl = models[0]["classes"]
    out["live_mtiles"] = []
    for su in sorted({int(c["super"]) for c in cl}):
        cnt = 0
        for m in models:
            some = np.zeros(m["plane"].shape[1:], bool)
            for k, c in enumerate(cl):
                if int(c["super"]) == su:
                    some |= m["plane"][k] != NEVER
            pad = np.zeros((some.shape[0], (some.shape[1] + 15) // 16 * 16), bool)
            pad[:, : some.shape[1]] = some
            cnt += int(pad.reshape(pad.shape[0], -1, 16).any(2).sum())
        out["live_mtiles"].append(cnt)
    return out

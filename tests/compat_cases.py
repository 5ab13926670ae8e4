"""Cases for the drop-in symbols ncc_8_u8 / ncc_16_u8 (csrc/hip/compat.hip) at the places where compat_call branches: more hits than
its page-locked block holds (PIN_HITS = 65 536: device sort, pack, truncation to n_out, grow and rescan), window tables that
prepare_for_size would never produce, inputs that change between two calls of one geometry (residency by content hash), and
geometries with nothing to search.  tests/test_compat_cases_host.py proves on the CPU that each case has the property it is there for;
tests/test_gpu_compat_edges.py holds the device against the oracle, byte for byte.

A call is a dict: page (r_h, r_w) uint8 ink-high, needle (n_h, n_w), stats = (patch_sum, patch_rnorm, start_end), thr, n_out.
"""
import functools

import numpy as np

from oracle import oracle as O

PIN_HITS = 1 << 16   # CompatState::PIN_HITS
N_OUT_ALL = 1 << 17  # an n_out no call here reaches


def call(page, needle, stats, thr, n_out):
    return dict(page=page, needle=needle, stats=stats, thr=float(thr), n_out=int(n_out))


def oracle(c, use_ref=False):
    """The expected list of a call.  n_out == 0 has no reference behaviour (src/ncc.cpp:45 requires n_out >= 1, and the reference
    kernel would write past `out`): the expected list is empty, and the restatement alone says so."""
    r_h, r_w = c["page"].shape
    return O.ncc_u8(O.padded(c["page"]), r_w, r_h, c["needle"], c["stats"], c["thr"], c["n_out"], use_ref=use_ref and c["n_out"] > 0)


def windows(start_end, r_h, n_h):
    """Windows the tables select: the sum of end - start over the searched rows y = 1 .. r_h - n_h."""
    se = start_end.astype(np.int64)
    return int(sum(se[2 * y + 1] - se[2 * y] for y in range(1, r_h - n_h + 1)))


# ---- more than PIN_HITS hits: a 300 x 240 noise page at threshold -1.0, where every window of a noise needle emits
BIG_W, BIG_H = 300, 240
BIG_NEEDLES = {"n8": (8, 8), "n16": (13, 11)}  # (n_w, n_h): (300 - 8) * (240 - 8) = 67 744 and (300 - 13) * (240 - 11) = 65 723 windows
BIG_N_OUT = (1, 1024, N_OUT_ALL)               # a fresh thread's first call (n_out = 1: 65 536 slots) grows its hit arrays and rescans


@functools.lru_cache(maxsize=None)
def big(which):
    """-> (page, needle, stats) of the big case `which`."""
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (BIG_H, BIG_W), dtype=np.uint8)
    needles = {k: rng.integers(0, 256, (h, w), dtype=np.uint8) for k, (w, h) in sorted(BIG_NEEDLES.items())}
    n_w, n_h = BIG_NEEDLES[which]
    return page, needles[which], O.prepare_for_size(page, n_w, n_h)


def big_calls(which):
    page, needle, stats = big(which)
    return [call(page, needle, stats, -1.0, n_out) for n_out in BIG_N_OUT]


def trimmed(stats, r_h, n_h, keep):
    """The same tables with start_end cut from the bottom rows upwards until `keep` windows remain."""
    ps, pr, se = stats
    se = se.copy()
    excess = windows(se, r_h, n_h) - keep
    assert excess >= 0
    y = r_h - n_h
    while excess > 0:
        cut = min(excess, int(se[2 * y + 1]) - int(se[2 * y]))
        se[2 * y + 1] -= cut
        excess -= cut
        y -= 1
    return ps, pr, se


def boundary_calls():
    """The last call of the page-locked path (exactly PIN_HITS hits) and the first of the device path (one more)."""
    page, needle, stats = big("n8")
    n_h = needle.shape[0]
    return {n: call(page, needle, trimmed(stats, BIG_H, n_h, n), -1.0, N_OUT_ALL) for n in (PIN_HITS, PIN_HITS + 1)}


# ---- caller tables: another [start, end) in every row, and table entries no window statistics would give
TAB_W, TAB_H = 97, 41
TAB_NEEDLES = {"n8": (7, 9), "n16": (13, 6)}
TAB_THR = (-1.0, 0.0, 0.2)
TAB_LENGTHS = (1, 2, 3, 0, 17, 22, 35, 4, None)  # end - start by row (None: up to the last window the page has); % 4 and % 16 take every tail length


@functools.lru_cache(maxsize=None)
def tables_case(which, edited=True):
    """-> (page, needle, stats).  edited=False: the per-row ranges only, without the overwritten entries."""
    n_w, n_h = TAB_NEEDLES[which]
    rng = np.random.default_rng(0xC0DE + n_w)
    page = rng.integers(0, 256, (TAB_H, TAB_W), dtype=np.uint8)
    needle = rng.integers(0, 256, (n_h, n_w), dtype=np.uint8)
    page[10:10 + n_h, 12:12 + n_w] = needle  # an exact match inside a row's range, a near one two rows down
    page[21:21 + n_h, 14:14 + n_w] = needle ^ (rng.random((n_h, n_w)) < 0.1).astype(np.uint8) * 0x40
    ps, pr, se = O.prepare_for_size(page, n_w, n_h)
    x_searches = TAB_W - n_w + 1
    se = se.copy()
    for y in range(1, TAB_H - n_h + 1):
        start = 1 + (5 * y) % 11
        length = TAB_LENGTHS[y % len(TAB_LENGTHS)]
        se[2 * y], se[2 * y + 1] = start, x_searches if length is None else start + length
    if edited:
        ps, pr = ps.copy(), pr.copy()
        live = [(y, x) for y in range(1, TAB_H - n_h + 1) for x in range(int(se[2 * y]), int(se[2 * y + 1]))]
        pick = [live[i] for i in rng.choice(len(live), 8, replace=False)]
        for (y, x), v in zip(pick[:4], (np.inf, np.nan, 0.0, None)):
            pr[y, x] = -0.5 * pr[y, x] if v is None else v
        for k, (y, x) in enumerate(pick[4:]):  # (all below 2^31: the reference's vector path reads the sums as i32)
            ps[y, x] = (0, int(ps[1, 1]) + 1, int(ps[y, x]) + 1000, 0x7FFFFFFF)[k]
    return page, needle, (ps, pr, se)


def tables_calls(which, edited=True):
    page, needle, stats = tables_case(which, edited)
    return [call(page, needle, stats, thr, 8192) for thr in TAB_THR]


# ---- residency: call with A, call with B of the same geometry; B's result must be B's.  One input changes per case, the others stay A's.
# 113 x 53: every input's last n % 64 bytes (the part the hash once XOR-folded, bytes 8 apart onto each other) lie in the last page rows —
# 37 page bytes, 5 patch_sum entries, 5 patch_rnorm entries (x = 108 .. 112 of row 52) and the start_end rows 48 .. 52 — which a needle
# one pixel high and three wide reads (windows x < 111 of rows y <= 52).
RES_W, RES_H = 113, 53
RES_CASES = ("page-body", "page-tail", "page-tail-swap", "page-tail-mask", "sum-tail-swap", "rnorm-tail-swap", "start-end-tail-swap")


@functools.lru_cache(maxsize=None)
def _residency_base():
    rng = np.random.default_rng(0x5E51DE)
    page = rng.integers(1, 256, (RES_H, RES_W), dtype=np.uint8)
    page[52, 100], page[52, 108] = 17, 201
    needle = np.array([[10, 200, 77]], np.uint8)
    ps, pr, se = O.prepare_for_size(page, 3, 1)
    se = se.copy()
    x_searches = RES_W - 3 + 1
    for y in range(1, RES_H):
        se[2 * y], se[2 * y + 1] = 1 + y % 7, x_searches - y % 5
    return page, needle, (ps, pr, se)


def residency(case_id):
    """-> (call A, call B, (index of the changed input in [page, patch_sum, patch_rnorm, start_end], its changed byte offsets))."""
    page, needle, (ps, pr, se) = _residency_base()
    page, ps, pr, se = page.copy(), ps.copy(), pr.copy(), se.copy()
    a = call(page.copy(), needle, (ps.copy(), pr.copy(), se.copy()), -1.0, 8192)
    if case_id == "page-body":
        page[20, 40] ^= 0x55
        which = 0
    elif case_id == "page-tail":
        page[52, 100] ^= 0x55
        which = 0
    elif case_id == "page-tail-swap":
        page[52, 100], page[52, 108] = page[52, 108], page[52, 100]
        which = 0
    elif case_id == "page-tail-mask":
        page[52, 100] ^= 0x5A
        page[52, 108] ^= 0x5A
        which = 0
    elif case_id == "sum-tail-swap":
        ps[52, 108], ps[52, 110] = ps[52, 110], ps[52, 108]
        which = 1
    elif case_id == "rnorm-tail-swap":
        pr[52, 108], pr[52, 109] = pr[52, 109], pr[52, 108]
        which = 2
    elif case_id == "start-end-tail-swap":
        se[2 * 49: 2 * 49 + 2], se[2 * 51: 2 * 51 + 2] = se[2 * 51: 2 * 51 + 2].copy(), se[2 * 49: 2 * 49 + 2].copy()
        which = 3
    else:
        raise KeyError(case_id)
    b = call(page, needle, (ps, pr, se), -1.0, 8192)
    return a, b, which


def inputs_of(c):
    """The four hashed inputs of a call as bytes, in the order [page, patch_sum, patch_rnorm, start_end]."""
    ps, pr, se = c["stats"]
    return [np.ascontiguousarray(c["page"], np.uint8).tobytes(), np.ascontiguousarray(ps, np.uint32).tobytes(),
            np.ascontiguousarray(pr, np.float64).tobytes(), np.ascontiguousarray(se, np.uint16).tobytes()]


def xor_fold(tail):
    """What the content hash once made of an input's last n % 64 bytes: tail ^= b[i] << (8 * i & 63) — bytes 8 apart fold onto each other."""
    v = 0
    for i, b in enumerate(tail):
        v ^= b << (8 * i & 63)
    return v


# ---- geometries with nothing, or one row, to search
DEG_W, DEG_H = 16, 12
DEG_CASES = {"n_h == r_h": ((5, 12), 1024), "n_h == r_h - 1": ((5, 11), 1024), "n_w == r_w": ((16, 4), 1024), "n_out == 0": ((5, 4), 0)}


def degenerate(case_id):
    (n_w, n_h), n_out = DEG_CASES[case_id]
    rng = np.random.default_rng(0xDE6)
    page = rng.integers(0, 256, (DEG_H, DEG_W), dtype=np.uint8)
    needle = rng.integers(0, 256, (n_h, n_w), dtype=np.uint8)
    return call(page, needle, O.prepare_for_size(page, n_w, n_h), -1.0, n_out)

"""Cases for the exact scan (csrc/hip/scan_direct.hip: scan_direct_kernel, scan_tall_kernel) in both arithmetics: FOCR_SCAN_DIRECT (the
reference kernel's fma epilogue) and FOCR_SCAN_RUST (the scalar Rust scan's division, square root and skips).  Most GPU tests take
SCAN_DIRECT as their expected value; this is where it is held against the oracle at the shapes its own code branches on.
tests/test_exact_cases_host.py proves the cases' properties on the CPU, tests/test_gpu_exact_modes.py runs them on the device.

The banks are test_gpu_parity's `_random_bank` over the shape sets of test_random_banks_all_layouts, plus sets that launch
scan_tall_kernel<1> (n_h > 32, n_w <= 4) and <7> (25 .. 28 px wide), classes of 8, 9 and 16 templates (TALL_TC = 8: a full pass, a tail of
one, two full passes) and templates of the limit height 255.  In every set two templates of the first class are replaced:
  ZERO   all zero (s_n == 0: the Rust scan yields nothing, the C arithmetic divides by a zero norm)
  CONST  constant 200 (norm2_n == 0: den == 0 in every window); 255 at the limit height, where a saturated window under it has the largest dot
         product the limits allow, 255 * 255 * 32 * 255 = 530 604 000 < 2^31
and in every class of 300 px or more
  HEAVY  noise in 200 .. 255, planted on page 0: s_n * s_p = s_n^2 >= 2^32 in an emitted window — the product the Rust scan forms in u64.
Pages (ink-high here; the Scanner takes 255 - ink): page 0 is noise with the first template of each class planted where there is room;
page 1 is column bands — noise | paper (windows with s_p == 0 inside a row's [start, end)) | ink 255 (uniform windows: norm2_p == 0, the
largest s_p) — so that every template height sees every band.
"""
import functools
import math
import zlib

import numpy as np

from oracle import oracle as O
from test_gpu_parity import _random_bank

THRESHOLDS = (0.25, 0.9, -0.3)
CAP_C = 1024          # the reference kernel's cap (MAX_MATCHES): part of the C arithmetic's lists
CAP_RUST = 1 << 14    # the Rust scan has none: a buffer no count here reaches
ZERO, CONST, HEAVY_K = 1, 2, 3  # index inside its class of the replaced templates (k = 0 stays `_random_bank`'s noise and is planted)
HEAVY_AREA = 300      # 200 * 300 = 60 000 ... 255 * 300: s_n^2 >= 2^32 needs s_n >= 65 536; noise in 200 .. 255 averages 227 per pixel

# id -> shapes [(n_w, n_h)], templates per shape, (pages, r_h, r_w)
SETS = {
    "w16": ([(16, 16), (13, 7), (14, 20)], 7, (2, 61, 97)),
    "w8": ([(8, 15), (5, 9), (3, 3), (1, 1), (8, 32)], 7, (2, 61, 97)),
    "w12": ([(9, 15), (8, 15), (12, 16), (10, 3)], 7, (2, 61, 97)),
    "tall": ([(9, 17), (11, 32), (4, 30), (16, 32)], 7, (2, 61, 97)),
    "taller": ([(9, 33), (16, 48), (5, 40), (13, 64), (9, 15)], 7, (2, 61, 97)),      # 64 > 61 rows: never searchable
    "tallest": ([(7, 58), (16, 70)], 7, (2, 61, 97)),
    "wide": ([(17, 5), (24, 20), (32, 33), (20, 40), (9, 15)], 7, (2, 61, 97)),
    "drop": ([(13, 15), (12, 15), (9, 14), (8, 14), (9, 30), (13, 32)], 7, (2, 61, 97)),
    "tall1": ([(3, 40), (4, 35), (2, 16)], [8, 9, 7], (2, 61, 97)),                    # scan_tall_kernel<1>: one full pass / a tail of one
    "tall7": ([(27, 9), (25, 12), (28, 34)], [16, 9, 8], (2, 61, 97)),                 # scan_tall_kernel<7>: two full passes / a tail / one
    "h255": ([(32, 255), (1, 255)], [4, 9], (2, 300, 40)),                             # the limit height, in <8> and <1>
}
# the properties each set must show (the host test computes them from the oracle's lists and window statistics):
#   u64       an emitted window of the Rust scan with s_n * s_p >= 2^32
#   sp0 / neg / sn0   windows inside [start, end) the Rust scan skips for s_p == 0 / num < 0 / s_n == 0
#   den0      a window with den == 0 and s_p != 0
# (u64 needs a class of HEAVY_AREA px or more: w16, w8, w12 and tall1 have none)
PROPS = {k: ("sp0", "neg", "sn0", "den0") + (("u64",) if k not in ("w16", "w8", "w12", "tall1") else ()) for k in SETS}


def searchable(shape, geom):
    return shape[0] < geom[2] and shape[1] < geom[1]  # a window with x, y >= 1 fits


def launches(set_id):
    """The scan kernels a direct scan of the set launches, as focr_last_launches names them."""
    shapes, _, geom = SETS[set_id]
    out = set()
    for n_w, n_h in shapes:
        if searchable((n_w, n_h), geom):
            ndw = (n_w + 3) // 4
            out.add(f"scan_tall_kernel<{ndw}>" if n_h > 32 or n_w > 16 else f"scan_direct_kernel<{ndw},{16 if n_h <= 16 else 32}>")
    return out


def bands(r_w):
    """Page 1's columns: (noise end, paper end); ink 255 from there to the last column but one, which is noise again (so that a row's
    [start, end) reaches across for every width)."""
    return (28, 62) if r_w == 97 else (2, 6)


@functools.lru_cache(maxsize=None)
def build(set_id):
    """-> (bank, luma pages (n, r_h, r_w) as Scanner.set_pages takes them, info): info['zero'], info['const'] template indices,
    info['heavy'] list of them, info['first'] the first template of each class, info['planted'] [(t, y, x)] on page 0."""
    shapes, per, geom = SETS[set_id]
    rng = np.random.default_rng(zlib.crc32(("exact " + set_id).encode()))
    bank = _random_bank(rng, shapes, per)
    counts = per if isinstance(per, list) else [per] * len(shapes)
    first = [int(sum(counts[:k])) for k in range(len(shapes))]
    info = dict(zero=first[0] + ZERO, const=first[0] + CONST, heavy=[], first=first, planted=[])
    bank.needle(info["zero"])[:] = 0
    bank.needle(info["const"])[:] = 200
    n_pages, r_h, r_w = geom
    ink = rng.integers(0, 256, (n_pages, r_h, r_w), dtype=np.uint8)
    if set_id == "h255":
        # 255s with one pixel changed: under a saturated window the largest dot product but for that pixel, a variance of about 1 out of sums
        # near 5e8, and windows that differ from it in one pixel only
        bank.needle(info["const"])[:] = 255
        t = first[0] + HEAVY_K
        bank.needle(t)[:] = 255
        bank.needle(t)[0, 0] = 254
        info["heavy"].append(t)
    else:
        for k, (n_w, n_h) in enumerate(shapes):
            if n_w * n_h >= HEAVY_AREA and searchable((n_w, n_h), geom):
                t = first[k] + HEAVY_K
                bank.needle(t)[:] = rng.integers(200, 256, (n_h, n_w), dtype=np.uint8)
                info["heavy"].append(t)
    # page 0: shelves of planted templates, the heavy ones first
    x, y, shelf = 1, 1, 0
    for t in info["heavy"] + first:
        if set_id == "h255" and t in info["heavy"]:
            continue
        nd = bank.needle(t)
        n_h, n_w = nd.shape
        if not searchable((n_w, n_h), geom):
            continue
        if x + n_w > r_w:
            x, y, shelf = 1, y + shelf + 1, 0
        if y + n_h > r_h or x + n_w > r_w:
            continue  # no room: noise finds this class its matches
        ink[0, y:y + n_h, x:x + n_w] = nd
        info["planted"].append((t, y, x))
        x, shelf = x + n_w + 1, max(shelf, n_h)
    # page 1: noise | paper | ink 255 | one column of noise
    a, b = bands(r_w)
    ink[1, :, a:b] = 0
    ink[1, :, b:r_w - 1] = 255
    if set_id == "h255":
        ink[1, 5, b] = 254  # the window at (x = b, y = 5) IS the changed template; the 32-wide windows around it hold the pixel elsewhere
    return bank, (255 - ink).astype(np.uint8), info


@functools.lru_cache(maxsize=None)
def oracle_c(set_id, thr):
    """The reference kernel's lists (cap 1024) -> [page][template] MATCH_DTYPE arrays; computed once, left unchanged."""
    bank, luma, _ = build(set_id)
    out = []
    for pg in luma:
        counts, m = O.scan_page(O.invert(pg), bank, thr, CAP_C, use_ref=O.have_ref())
        out.append([m[t, : counts[t]].copy() for t in range(len(bank))])
    return out


@functools.lru_cache(maxsize=None)
def _page_tables(set_id, p):
    bank, luma, _ = build(set_id)
    ink = O.invert(luma[p])
    tabs = O.tables(ink)
    shapes = {(int(t["n_w"]), int(t["n_h"])) for t in bank.templates}
    se = {s: O.prepare_for_size(ink, s[0], s[1], tabs)[2] for s in shapes if s[0] <= ink.shape[1] and s[1] <= ink.shape[0]}
    return ink, tabs, se


@functools.lru_cache(maxsize=None)
def oracle_rust(set_id, thr):
    """The scalar Rust scan's lists, template by template through O.search_rust_u8 (any width) -> [page][template] arrays (no cap)."""
    bank, luma, _ = build(set_id)
    out = []
    for p in range(len(luma)):
        ink, tabs, se = _page_tables(set_id, p)
        row = []
        for t in range(len(bank)):
            nd = bank.needle(t)
            c, m = O.search_rust_u8(ink, nd, thr, CAP_RUST, tabs, se.get((nd.shape[1], nd.shape[0])))
            assert c < CAP_RUST, "no oracle count reaches its buffer"
            row.append(m)
        out.append(row)
    return out


def window_ints(ink, needle):
    """Exact integers of every window position: (acc, s_p, s2_p) as int64 arrays indexed [y, x]."""
    n_h, n_w = needle.shape
    w = np.lib.stride_tricks.sliding_window_view(ink.astype(np.int64), (n_h, n_w))
    nd = needle.astype(np.int64)
    return np.einsum("yxij,ij->yx", w, nd), w.sum((2, 3)), (w * w).sum((2, 3))


def rust_witness(ink, needle, start_end):
    """Second witness of the Rust arithmetic (src/ncc.rs:406-483) in plain Python: integers for acc, s_p, s2_p and the u64 products, Python
    floats (IEEE double) and math.sqrt for the rest.  -> (candidates [(x, y, similarity as a double, s_n * s_p)] before the threshold, in
    (y, x) order — a match is one with similarity > (double)(f32)threshold, narrowed to f32 — and the windows skipped per rule
    {'sp0', 'neg', 'sn0', 'den0'}: den0 counts windows that reached the division with den == 0)."""
    n_h, n_w = needle.shape
    r_h, r_w = ink.shape
    n = n_w * n_h
    s_n = sum(int(v) for v in needle.reshape(-1))
    s2_n = sum(int(v) * int(v) for v in needle.reshape(-1))
    skipped = dict(sp0=0, neg=0, sn0=0, den0=0)
    rows = [(y, int(start_end[2 * y]), int(start_end[2 * y + 1])) for y in range(1, r_h - n_h + 1)]
    if s_n == 0:
        skipped["sn0"] = sum(e - s for _, s, e in rows)
        return [], skipped
    acc, sp, s2p = window_ints(ink, needle)
    out = []
    for y, start, end in rows:
        for x in range(start, end):
            a, s_p, s2_p = int(acc[y, x]), int(sp[y, x]), int(s2p[y, x])
            assert a < 1 << 32 and s_n * s_p < 1 << 64
            if s_p == 0:
                skipped["sp0"] += 1
                continue
            num = float(a) - float(s_n * s_p) / float(n)
            if num < 0.0:
                skipped["neg"] += 1
                continue
            norm2_n = float(s2_n) - float(s_n * s_n) / float(n)
            norm2_p = float(s2_p) - float(s_p * s_p) / float(n)
            prod = norm2_n * norm2_p
            den = math.sqrt(prod) if prod >= 0.0 else math.nan
            if den == 0.0:
                skipped["den0"] += 1
                continue  # num / 0 is +inf or NaN: neither is a match
            sim = num / den
            if sim != math.inf and not math.isnan(sim):
                out.append((x, y, sim, s_n * s_p))
    return out, skipped


def witness_templates(set_id):
    """The templates the witness walks (pure Python is slow): the replaced ones and the first of every class."""
    _, _, info = build(set_id)
    return sorted({info["zero"], info["const"], *info["heavy"], *info["first"]})

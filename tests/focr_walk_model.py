"""walk_lines (font_ocr_amd/csrc/hip/post.hip) restated as the fixed kernel runs it, with mark_anchor_rows in front of it.

The device marks the anchored (page, row) entries and every row's extent in the (page, y, x, t)-sorted hit list; then a
wave walks each anchored row 64 elements at a time: a ballot of the open group's members inside the chunk, a max of their
f32::total_cmp order, a ballot of the lanes that reach it (the highest lane wins), and a group still open at the end of a
chunk carried into the next with its best order and index (later elements win ties: `>=`).  Hits cut off by their call's
cap are invalid lanes.  walk_row does the same steps on 64-lane numpy vectors, statement for statement, and counts the
trips of the `while (pos < 64)` loop: more than TRIP_BOUND in one chunk raises TripBoundExceeded where the kernel would
not finish.  Which wave walks a row (WALK_ROWS entries per wave) does not change what the walk of that row gives, so the
model walks the anchored rows one after the other.

The module also builds the hit lists that tests/test_walk_model.py proves on the model against the reference's
process_hits (oracle.process_hits) and that tests/test_gpu_process_hits.py then feeds the device through
focr_debug_process_hits.
"""
import numpy as np

LANES = 64
TRIP_BOUND = LANES + 1  # a chunk's first trip may close a carried group without consuming anything; every other trip consumes
WALK_ROWS = 16
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
OVERLAPS = (I32_MIN, -5, -1, 0, 1, 64, 65535, I32_MAX)
N_TEMPLATES = 380  # the configs[1] bank (tests/golden/bank_dejavu13_ascii95_x2.bin) that the GPU test uploads
_ALL = (1 << LANES) - 1


class TripBoundExceeded(AssertionError):
    """The walk made more trips in one chunk than the kernel's termination argument allows."""


def _ballot(pred):
    return int(np.packbits(pred, bitorder="little").view("<u8")[0])


def _ctz(mask):
    return (mask & -mask).bit_length() - 1


def order_key(sims):
    """f32::total_cmp as an unsigned order: post.hip's total_key(s) ^ 0x80000000."""
    b = np.asarray(sims, np.float32).view(np.int32).astype(np.int64)
    return (np.where(b < 0, b ^ 0x7FFFFFFF, b) & 0xFFFFFFFF) ^ 0x80000000


def walk_row(x, order, kept, overlap):
    """walk_lines on one anchored row: x, order (order_key) and kept of the row's extent of the sorted list.  Returns the
    winning element of each group, as indices into the extent."""
    e = len(x)
    lane = np.arange(LANES)
    choice = []
    open_ = False
    anchor = 0
    best_ord = best_idx = 0
    for base in range(0, e, LANES):
        i = np.minimum(base + lane, e - 1)
        valid = (base + lane < e) & kept[i]
        xl = np.where(valid, x[i], 0x7FFFFFFF)
        ordl = np.where(valid, order[i], 0)
        vmask = _ballot(valid)
        pos = 0
        opened_at = -1
        trips = 0
        while pos < 64:
            trips += 1
            if trips > TRIP_BOUND:
                raise TripBoundExceeded(f"chunk at element {base}: more than {TRIP_BOUND} trips (overlap {overlap})")
            if not open_:
                cand = vmask & (_ALL << pos) & _ALL
                if not cand:
                    break
                pos = _ctz(cand)
                anchor = int(xl[pos])
                opened_at = pos
                best_ord = best_idx = 0
                open_ = True
            inn = valid & (lane >= pos) & ((lane == opened_at) | ((xl - anchor <= overlap) & (anchor - xl <= overlap)))
            inmask = _ballot(inn)
            brk = vmask & ~inmask & (_ALL << pos) & _ALL
            stop = _ctz(brk) if brk else 64
            member = inn & (lane < stop)
            mx = int(np.where(member, ordl, 0).max())
            top = _ballot(member & (ordl == mx))
            if top and mx >= best_ord:
                best_ord = mx
                best_idx = base + top.bit_length() - 1
            if stop < 64:
                choice.append(best_idx)
                open_ = False
            pos = stop
    if open_:
        choice.append(best_idx)
    return choice


def model_lines(case):
    """mark_anchor_rows + walk_lines + emit_chars over a Case -> per page, its lines as lists of element indices."""
    sim = case.sim
    kept = case.keep != 0
    row = case.page.astype(np.int64) * case.r_h + case.y
    keep_row = np.zeros(case.n_pages * case.r_h, bool)
    keep_row[row[kept & (sim >= np.float32(case.anchor))]] = True  # f32 >=: a NaN anchor marks nothing
    order = order_key(sim)
    x = case.x.astype(np.int64)
    lines = [[] for _ in range(case.n_pages)]
    starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]]) if len(row) else np.zeros(0, np.int64)
    for b, e in zip(starts, np.r_[starts[1:], len(row)]):
        r = int(row[b])
        if keep_row[r]:
            lines[r // case.r_h].append([int(b) + k for k in walk_row(x[b:e], order[b:e], kept[b:e], case.overlap)])
    return lines


def reference_lines(case):
    """The reference's process_hits (oracle.process_hits) page by page, fed the kept hits in get_hits order (template-major,
    then (y, x)) -> per page, its lines as lists of element indices (carried through as a tag in `w`)."""
    from oracle import oracle as O

    out = []
    for p in range(case.n_pages):
        sel = np.flatnonzero((case.page == p) & (case.keep != 0))
        sel = sel[np.lexsort((case.x[sel], case.y[sel], case.t[sel]))]
        hits = np.zeros(len(sel), O.HIT_DTYPE)
        hits["x"], hits["y"], hits["similarity"], hits["letter"] = case.x[sel], case.y[sel], case.sim[sel], case.t[sel]
        hits["w"], hits["h"] = sel, 1
        out.append([[int(c["w"]) for c in line] for line in O.process_hits(hits, case.anchor, case.overlap)])
    return out


class Case:
    """One hit list in (page, y, x, t) order, its geometry and the process_hits arguments it runs with.  parts: rows given as
    (page, y, x, t, similarity, keep), each field a scalar or an array of the row's length."""

    def __init__(self, name, parts, anchor=0.95, overlap=5, n_pages=1, r_w=400, r_h=8, expect_lines=None):
        self.name, self.anchor, self.overlap = name, float(anchor), int(overlap)
        self.n_pages, self.r_w, self.r_h, self.n_templates = n_pages, r_w, r_h, N_TEMPLATES
        self.expect_lines = expect_lines  # the number of lines the case must give, where the case is about that number
        cols = [[] for _ in range(6)]
        for part in parts:
            n = len(np.atleast_1d(part[4]))
            for c, v in zip(cols, part):
                c.append(np.broadcast_to(np.asarray(v), (n,)))
        dtypes = (np.int64, np.int64, np.int64, np.int64, np.float32, np.uint8)
        page, y, x, t, sim, keep = (np.concatenate(c).astype(d) if c else np.zeros(0, d) for c, d in zip(cols, dtypes))
        key = ((page * r_h + y) * r_w + x) * N_TEMPLATES + t
        o = np.argsort(key, kind="stable")
        assert (np.diff(key[o]) > 0).all(), f"{name}: two hits share (page, y, x, t)"
        assert len(o) == 0 or (page.max() < n_pages and y.max() < r_h and x.max() < r_w and t.max() < N_TEMPLATES and
                               min(page.min(), y.min(), x.min(), t.min()) >= 0), name
        self.page, self.y, self.x, self.t = (a[o].astype(np.uint32) for a in (page, y, x, t))
        self.sim, self.keep = sim[o], keep[o]

    def __repr__(self):
        return f"Case({self.name}: {len(self.sim)} hits, anchor {self.anchor}, overlap {self.overlap})"


def _sims(rng, n, lo=0.5, hi=0.9):
    return rng.uniform(lo, hi, n).astype(np.float32)


TIES = np.array([0.96, 0.97, 0.97, 0.98, 0.98, 0.98], np.float32)
POOL = np.array([0.5, 0.8, 0.9, 0.95, 0.95, 0.97, 0.97, 0.99, 1.0], np.float32)
FUZZ_POOL = np.array([0.5, 0.8, 0.9, 0.95, 0.95, 0.97, 0.97, 0.99, 1.0, -0.0, 0.0, 1e-45, -0.25], np.float32)


def chunk_rows():
    """One group per row, of 63 .. 129 hits: its maximum first, last, at element 63, at 64, tied across 63 / 64, tied across
    three chunks, every element tied.  The group is made by equal x (overlap 0) and by a huge overlap over distinct x."""
    rng = np.random.default_rng(63)
    out = []
    for n in (63, 64, 65, 127, 128, 129):
        k = np.arange(n)
        peaks = {"first": [0], "last": [n - 1], "alltied": list(k)}
        if n > 63:
            peaks["at63"] = [63]
        if n > 64:
            peaks.update(at64=[64], tie63_64=[63, 64])
        if n > 128:
            peaks["tie3chunks"] = [5, 64 + 5, 128]
        for name, where in peaks.items():
            s = _sims(rng, n)
            s[where] = 0.99
            out.append(Case(f"{n}-samex-{name}", [(0, 3, 9, k, s, 1)], overlap=0))
            out.append(Case(f"{n}-wide-{name}", [(0, 3, k, k % 7, s, 1)], overlap=I32_MAX))
    return out


def big_rows():
    """A row of 100 000 kept hits, (x, t) = divmod(k, 380): one group under overlap INT32_MAX with its maximum at element 63,
    at 64, tied across 63 / 64 and across three distant chunks; a group per x under overlap 0; a character per hit under -1."""
    rng = np.random.default_rng(100_000)
    n = 100_000
    k = np.arange(n)
    x, t = k // N_TEMPLATES, k % N_TEMPLATES
    out = []
    for name, where, overlap in (("at63", [63], I32_MAX), ("at64", [64], I32_MAX), ("tie63_64", [63, 64], I32_MAX),
                                 ("tie3chunks", [64 * 400 + 63, 64 * 900, n - 1], I32_MAX), ("perx", [63, 64, 379, 380], 0),
                                 ("each", [64], -1)):
        s = _sims(rng, n)
        s[where] = 0.99
        out.append(Case(f"100000-{name}", [(0, 1, x, t, s, 1)], overlap=overlap, r_w=300, r_h=2))
    return out


def boundary_rows():
    """The first non-member of a row's first group lands on element 63, 64 (element 0 of the next chunk), 65, 127, 128 or
    129; similarities from a pool of ties, so that maxima tie inside groups and across chunk edges."""
    rng = np.random.default_rng(64)
    out = []
    for first in (63, 64, 65, 127, 128, 129):
        for overlap in (0, 3):
            xs, ts, x0 = [], [], 20
            for size in (first, 70, 9, 64):
                j = np.arange(size)
                xs.append(x0 + (j * (overlap + 1)) // size)  # x0 .. x0 + overlap: one group anchored on x0
                ts.append(j)
                x0 += overlap + 1
            x, t = np.concatenate(xs), np.concatenate(ts)
            s = TIES[rng.integers(0, len(TIES), len(x))]
            out.append(Case(f"break{first}-ov{overlap}", [(0, 5, x, t, s, 1)], overlap=overlap))
    return out


def capped_rows():
    """Hits cut off by their call's cap (keep = 0) are invisible: straddling a chunk edge, a whole chunk of them inside one
    group, 64 of them before a row's first kept hit, a group that ends in capped hits at a chunk edge, and a row whose only
    hit at or above the anchor is capped (that row gives no line)."""
    rng = np.random.default_rng(65)
    n = 200
    k = np.arange(n)
    out = []
    for overlap in (0, 2, -1):
        for name, capped, peaks, capped_peak in (("straddle", slice(60, 68), [59, 68], 62), ("chunk", slice(64, 128), [63, 128], 100),
                                                 ("lead", slice(0, 64), [64, 99], 10), ("tail", slice(56, 64), [40, 64], 60)):
            keep = np.ones(n, np.uint8)
            keep[capped] = 0
            s = _sims(rng, n)
            s[peaks] = 0.99
            s[capped_peak] = 0.999
            x = np.where(k < 64, 11, 13) if name == "tail" else 11  # "tail": the first group ends where its capped hits end
            out.append(Case(f"capped-{name}-ov{overlap}", [(0, 2, x, k, s, keep)], overlap=overlap))
        s = _sims(rng, n)
        s[77] = 0.99
        keep = np.ones(n, np.uint8)
        keep[77] = 0
        s2 = _sims(rng, 30)
        s2[29] = 0.99
        out.append(Case(f"capped-unanchored-ov{overlap}", [(0, 2, 11, k, s, keep), (0, 4, 3, np.arange(30), s2, 1)], overlap=overlap,
                        expect_lines=1))
    return out


def _mixed(rng, n_rows=6, r_w=160, pool=POOL, keep_p=0.9, page=0):
    """Rows of 1 .. 300 hits clustered around x positions 9 px apart: groups of every size for small overlaps."""
    parts = []
    for y in range(n_rows):
        n = int(rng.integers(1, 300))
        x = np.clip(rng.choice(np.arange(5, r_w - 5, 9), n) + rng.integers(-3, 4, n), 0, r_w - 1)
        u = np.unique(x.astype(np.int64) * N_TEMPLATES + rng.integers(0, N_TEMPLATES, n))
        parts.append((page, y, u // N_TEMPLATES, u % N_TEMPLATES, pool[rng.integers(0, len(pool), len(u))],
                      (rng.random(len(u)) < keep_p).astype(np.uint8)))
    return parts


def overlap_rows():
    """Every overlap from INT32_MIN to INT32_MAX on the same rows of up to 300 hits."""
    rng = np.random.default_rng(66)
    out = []
    for it in range(2):
        parts = _mixed(rng)
        for overlap in OVERLAPS:
            out.append(Case(f"overlap{overlap}-{it}", parts, overlap=overlap, r_w=160))
    return out


def anchor_rows():
    """Anchors NaN and +inf (no line), -inf and -1 (every row with a kept hit), exactly a kept hit's similarity and the next
    f32 above it."""
    rng = np.random.default_rng(67)
    parts = _mixed(rng, pool=np.r_[POOL, np.float32(0.9731)])
    kept = np.concatenate([np.broadcast_to(p[4], len(p[5]))[p[5] != 0] for p in parts])
    s = np.float32(0.9731) if (kept == np.float32(0.9731)).any() else np.float32(kept.max())
    rows_with_kept = sum(int((p[5] != 0).any()) for p in parts)
    out = []
    for anchor, lines in ((float("nan"), 0), (float("inf"), 0), (float("-inf"), rows_with_kept), (-1.0, rows_with_kept),
                          (float(s), None), (float(np.nextafter(s, np.float32(np.inf))), None)):
        for overlap in (5, -1):
            out.append(Case(f"anchor{anchor!r}-ov{overlap}", parts, anchor=anchor, overlap=overlap, r_w=160, expect_lines=lines))
    return out


def similarity_rows():
    """f32::total_cmp inside groups: +0.0 beats -0.0 wherever it sits, negatives, subnormals, 1.0; the groups start at a chunk's
    first element or straddle a chunk edge behind filler hits."""
    groups = [[0.0, -0.0, -0.0], [-0.0, 0.0, -0.0], [-0.0, -0.0, 0.0], [0.0, 0.0, -0.0], [-0.5, -0.25, -0.75],
              [1e-45, 2e-45, -1e-45, 0.0], [1.0, 0.99, 1.0], [-0.0, -1e-45, -0.0], [-0.25, -0.0, -1e-45]]
    out = []
    for lead in (0, 61, 62, 63):
        xs, ts, ss = [np.zeros(lead, np.int64)], [np.arange(lead)], [np.full(lead, 0.5, np.float32)]
        for g, vals in enumerate(groups):
            xs.append(np.full(len(vals), 3 + 3 * g))
            ts.append(np.arange(len(vals)))
            ss.append(np.array(vals, np.float32))
        part = (0, 1, np.concatenate(xs), np.concatenate(ts), np.concatenate(ss), 1)
        for anchor, overlap in ((-1.0, 1), (1.0, 1), (-1.0, -1)):
            out.append(Case(f"sims-lead{lead}-a{anchor}-ov{overlap}", [part], anchor=anchor, overlap=overlap))
    return out


def walk_row_edges():
    """A wave takes WALK_ROWS = 16 (page, row) entries: with r_h = 17 or 31 its rows span two pages.  Anchored rows at random,
    every row anchored, the last row of the last page anchored; 1, 3 and 300 pages."""
    rng = np.random.default_rng(16)
    out = []
    for r_h, n_pages in ((17, 1), (17, 3), (31, 1), (31, 3), (17, 300)):
        for every in (False, True):
            parts = []
            for p in range(n_pages):
                for y in range(r_h):
                    last = p == n_pages - 1 and y == r_h - 1
                    if not (every or last or rng.random() < (0.3 if n_pages > 3 else 0.6)):
                        continue
                    n = int(rng.integers(1, 6))
                    s = rng.uniform(0.5, 0.94, n).astype(np.float32)
                    if every or last or rng.random() < 0.5:
                        s[rng.integers(0, n)] = 0.97
                    parts.append((p, y, np.sort(rng.choice(64, n, replace=False)), rng.integers(0, N_TEMPLATES, n), s, 1))
            out.append(Case(f"rows{r_h}x{n_pages}-{'all' if every else 'some'}", parts, overlap=2, n_pages=n_pages, r_w=64,
                            r_h=r_h, expect_lines=n_pages * r_h if every else None))
    return out


def empty_lists():
    """No hits at all, and hits that are all capped: zero lines."""
    k = np.arange(100)
    s = np.full(100, 0.99, np.float32)
    return [Case("no-hits", [], n_pages=2, expect_lines=0),
            Case("all-capped", [(0, 1, 3, k, s, 0), (1, 2, k, 5, s, 0)], n_pages=2, expect_lines=0),
            Case("all-capped-ov-1", [(0, 1, 3, k, s, 0), (1, 2, k, 5, s, 0)], n_pages=2, overlap=-1, expect_lines=0)]


def fuzz(n_lists=300, seed=0xF0C5):
    """Seeded lists mixing the above: rows of 1 .. 250 hits, narrow and wide x spreads, tied and signed-zero similarities, runs
    of capped hits, every anchor and overlap edge, geometries whose waves span pages."""
    out = []
    for i in range(n_lists):
        rng = np.random.default_rng(seed + i)
        n_pages, r_h, r_w = int(rng.integers(1, 4)), int(rng.choice([3, 16, 17, 31, 40])), int(rng.integers(8, 260))
        parts = []
        for p in range(n_pages):
            for y in rng.choice(r_h, size=int(rng.integers(0, min(r_h, 6) + 1)), replace=False):
                n = int(rng.choice([1, 3, 63, 64, 65, 128, 129, 250]))
                x0, spread = int(rng.integers(0, r_w)), int(rng.choice([1, 3, r_w]))
                x = np.minimum(x0 + rng.integers(0, spread, n), r_w - 1)
                u = np.unique(x.astype(np.int64) * N_TEMPLATES + rng.integers(0, N_TEMPLATES, n))
                m = len(u)
                s = FUZZ_POOL[rng.integers(0, len(FUZZ_POOL), m)] if rng.random() < 0.7 else rng.uniform(-0.2, 1.0, m).astype(np.float32)
                keep = np.ones(m, np.uint8)
                mode = int(rng.integers(0, 3))
                if mode == 1:
                    keep = (rng.random(m) < 0.8).astype(np.uint8)
                elif mode == 2:
                    a = int(rng.integers(0, m))
                    keep[a:a + int(rng.integers(1, 80))] = 0
                parts.append((p, int(y), u // N_TEMPLATES, u % N_TEMPLATES, s, keep))
        anchors = [0.95, 0.97, 0.5, -1.0, float("-inf"), float("inf"), float("nan")]
        if parts and rng.random() < 0.3:
            pp = parts[int(rng.integers(0, len(parts)))]
            anchors = [float(pp[4][int(rng.integers(0, len(pp[4])))])]
        anchor = anchors[int(rng.integers(0, len(anchors)))]
        overlap = int(rng.choice(OVERLAPS + (2, 5, 8, 12)))
        out.append(Case(f"fuzz{i}", parts, anchor=anchor, overlap=overlap, n_pages=n_pages, r_w=r_w, r_h=r_h))
    return out


FAMILIES = {"chunk_rows": chunk_rows, "big_rows": big_rows, "boundaries": boundary_rows, "capped": capped_rows,
            "overlaps": overlap_rows, "anchors": anchor_rows, "similarities": similarity_rows, "walk_rows": walk_row_edges,
            "empty": empty_lists, "fuzz": fuzz}

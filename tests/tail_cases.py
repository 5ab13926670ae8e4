"""Cases for the tail of the MFMA scan at its capacity edges (tests/test_tail_cases_host.py on the CPU, tests/test_gpu_tail_edges.py on the
device).  Everything behind the scan kernels picks its code path from a count: the hits of one bucket (a page row, or an x-segment of
one: rows.hip), the hits of one page (order.hip: units of 2048), the templates of the bank (4096: row tail and counting form, above:
legacy tail and sorting form), the number of buckets (the prefix's 16 x 256 pieces).  A case puts exact counts there.

The construction: a page of noise bytes 1 .. 255 against a bank of T noise templates of one size at threshold -1.0 emits every
(window, template) pair with 1 <= x <= r_w - n_w, 1 <= y <= r_h - n_h whose window touches ink, so a page whose pixel row j carries
noise in columns [0, L_j + 1) — L non-increasing — has exactly L_y * T hits in page row y ("stairs").  Where a case needs few
hits it plants templates on paper at a positive threshold instead.  The targets below are written out, not computed: the host test
holds the oracle's lists against them (a case that misses its targets fails there, before any device sees it), `plan` restates the
host's choice of path (scan_mfma.hip: launch_scan_mfma, row_tail; results.hip: SizeEstimate::update) from the oracle's hits, and the
device test asserts the path the library reports (focr_debug_tail_path) against the same table.

Every case has a seed of its own and hence bank content no other test uses: size estimates are shared per process, keyed by the
bank's content, and a case's first scan must run with exact sizes.
"""
import zlib

import numpy as np

from oracle import oracle as O
from prefilter_cases import bank_of

SEED0 = 0x7A110000


def _c(group, classes, geom, thr, cap, pages, rows, seg, row_max, path, verify="lds12", chunks=0, capped=0, caps=(), post=False, grids=False,
       witness=False, buckets=None):
    return dict(group=group, classes=classes, geom=geom, thr=thr, cap=cap, pages=pages, rows=rows, seg=seg, row_max=row_max, path=path, verify=verify,
                chunks=chunks, capped=capped, caps=caps, post=post, grids=grids, witness=witness, buckets=buckets or {})


def stairs(*live):
    return ("stairs", list(live))


def block(cols, rows):
    return ("stairs", [cols] * rows)


def plant(*tyx):
    return ("plant", list(tyx))


R, RB, RL, LG = "rows", "rows+big", "rows+lib", "legacy"

# id -> group; classes [(n_w, n_h, templates)] in bank order; (pages, r_w, r_h); threshold; cap of the main run;
#   pages  {page: recipe}: stairs(L_1, L_2, ...) = live windows of page rows y = 1, 2, ...; block(cols, rows); plant((t, y, x), ...); others paper
#   rows   {page: hits of page rows y = 1, 2, ... (all templates) | {y: hits}}: the TARGETS; a page's total is their sum
#   seg    (log2 of the segment width, segments per row) of the three MFMA scans of one context: exact sizes, estimated sizes,
#          estimated sizes after any re-segmentation; (0, 0) where the scan takes the legacy tail
#   row_max  the largest bucket under each of those three layouts (the layout the row tail would use, also where the scan goes legacy: a
#          largest bucket above 2048 halves the segments for the setup's next scan whichever tail that scan takes)
#   path   of the three scans: rows (one sort launch) / rows+big (second launch, buckets 1025 .. 4096) / rows+lib (library sort of the placed
#          hits: a bucket above 4096 under exact sizes) / legacy (estimated: the previous largest bucket + 25 % + 16 exceeds 4096, or the previous
#          scan did not sort rows; any: more than 4096 templates)
#   verify, chunks  the row tail's verify form; capped: (page, template) calls the main cap cuts; caps: further caps (two scans each)
#   buckets  {(scan, page, y, segment): hits} spot targets; post / grids / witness: the group's case for process_hits, the grid hook, the second witness
CASES = {
    # ---- (a) bucket sizes around 64: readlane ranking up to 64, counting sort from 65; a pure-paper page in the batch
    "a-64": _c("a", [(8, 8, 1)], (6, 80, 11), -1.0, 100,
               {0: stairs(1, 1), 1: stairs(2, 1, 1), 3: stairs(63, 62, 2), 4: stairs(64, 64, 63), 5: stairs(65, 64, 1)},
               {0: [1, 1], 1: [2, 1, 1], 3: [63, 62, 2], 4: [64, 64, 63], 5: [65, 64, 1]},
               [(7, 1)] * 3, [65] * 3, [R, R, R], capped=3, witness=True),
    # ---- (a) around 1024: the first launch's capacity; 1033 px: one segment of 2048 px, two x per bin
    "a-1024-t1": _c("a", [(8, 8, 1)], (3, 1033, 11), -1.0, 1024,
                    {0: stairs(1023, 1023, 1022), 1: stairs(1024, 1023, 65), 2: stairs(1025, 1024, 64)},
                    {0: [1023, 1023, 1022], 1: [1024, 1023, 65], 2: [1025, 1024, 64]},
                    [(11, 1)] * 3, [1025] * 3, [RB, RB, RB], capped=3),
    # 1024 is the batch's largest: exact sizes plan no second launch, the estimate (1296) does and finds its list empty; 16 t per bin
    "a-1024-t16": _c("a", [(8, 8, 16)], (2, 72, 11), -1.0, 100,
                     {0: stairs(64, 64, 63), 1: stairs(64, 4)}, {0: [1024, 1024, 1008], 1: [1024, 64]},
                     [(7, 1)] * 3, [1024] * 3, [R, RB, RB], capped=16),
    "a-1025-t5": _c("a", [(8, 8, 5)], (2, 213, 11), -1.0, 1024,
                    {0: stairs(205, 205, 204), 1: stairs(205, 13, 1)}, {0: [1025, 1025, 1020], 1: [1025, 65, 5]},
                    [(8, 1)] * 3, [1025] * 3, [RB, RB, RB]),
    "a-1025-t41": _c("a", [(8, 8, 41)], (2, 33, 11), -1.0, 60,
                     {0: stairs(25, 25, 24), 1: stairs(25, 1)}, {0: [1025, 1025, 984], 1: [1025, 41]},
                     [(6, 1)] * 3, [1025] * 3, [RB, RB, RB], capped=41),
    # ---- (a) around 4096: the second launch's capacity; 4105 px: one segment of 8192 px, eight x per bin.  A 4096-hit bucket sends the next
    # scan of the setup to the legacy tail (4096 + 25 % + 16 > 4096), which leaves no largest bucket: the third stays there
    "a-4096-t1": _c("a", [(8, 8, 1)], (2, 4105, 11), -1.0, 5000,
                    {0: stairs(4095, 4095, 1025), 1: stairs(4096, 4095, 1024)}, {0: [4095, 4095, 1025], 1: [4096, 4095, 1024]},
                    [(13, 1), (0, 0), (0, 0)], [4096, 4095, 4095], [RB, LG, LG], capped=2),
    "a-4097-t1": _c("a", [(8, 8, 1)], (3, 4105, 11), -1.0, 5000,
                    {0: stairs(4095, 4095, 1025), 1: stairs(4096, 4095, 1024), 2: stairs(4097, 4096, 64)},
                    {0: [4095, 4095, 1025], 1: [4096, 4095, 1024], 2: [4097, 4096, 64]},
                    [(13, 1), (0, 0), (0, 0)], [4097, 4095, 4095], [RL, LG, LG], capped=3),
    "a-4096-t64": _c("a", [(8, 8, 64)], (2, 72, 11), -1.0, 100,
                     {0: stairs(64, 64, 63), 1: stairs(64, 17, 1)}, {0: [4096, 4096, 4032], 1: [4096, 1088, 64]},
                     [(7, 1), (0, 0), (0, 0)], [4096, 4032, 4032], [RB, LG, LG], capped=64),
    "a-4097-t17": _c("a", [(8, 8, 17)], (2, 249, 11), -1.0, 1024,
                     {0: stairs(241, 241, 240), 1: stairs(241, 61, 3)}, {0: [4097, 4097, 4080], 1: [4097, 1037, 51]},
                     [(8, 1), (0, 0), (0, 0)], [4097, 2159, 2159], [RL, LG, LG]),
    # ---- (a) mixed: <= 64, 65 .. 1024 and 1025 .. 4096 in neighbouring rows and on different pages, six buckets on the `big` list; 2060 > 2048
    # halves the segments once (512 -> 256 px: 255 x 5 = 1275 is then the largest)
    "a-mixed": _c("a", [(8, 8, 5)], (4, 420, 12), -1.0, 300,
                  {0: stairs(412, 205, 13, 1), 1: stairs(300, 204, 12), 3: stairs(410, 206, 205, 2)},
                  {0: [2060, 1025, 65, 5], 1: [1500, 1020, 60], 3: [2050, 1030, 1025, 10]},
                  [(9, 1), (8, 2), (8, 2)], [2060, 1275, 1275], [RB, RB, RB], capped=15, post=True, grids=True,
                  buckets={(0, 0, 1, 0): 2060, (1, 0, 1, 0): 1275, (1, 0, 1, 1): 785, (1, 3, 2, 0): 1030, (1, 3, 2, 1): 0}),
    # ---- (b) segments.  4096 templates take 128 px segments from the first scan: two on a 200 px page, the last one partial (72 px); planted
    # hits at x = 127 | 128 and at r_w - n_w = 196, with template indices at both ends of the bank
    "b-seg-t4096": _c("b", [(4, 7, 4096)], (2, 200, 24), 0.95, 1024,
                      {0: plant((0, 1, 127), (4095, 9, 128), (7, 1, 196), (2048, 9, 1), (100, 17, 120), (101, 17, 124), (102, 17, 132)),
                       1: plant((4095, 17, 196), (1, 1, 1))},
                      {0: {1: 2, 9: 2, 17: 3}, 1: {1: 1, 17: 1}},
                      [(7, 2)] * 3, [2, 2, 2], [R, R, R], verify="chunks", chunks=4,
                      buckets={(0, 0, 1, 0): 1, (0, 0, 1, 1): 1, (0, 0, 9, 0): 1, (0, 0, 9, 1): 1, (0, 0, 17, 0): 2, (0, 0, 17, 1): 1, (0, 1, 17, 1): 1}),
    # 2400 hits per row in one 512 px segment, then 256 px segments of 1530 and 870
    "b-halve": _c("b", [(8, 8, 6)], (2, 408, 11), -1.0, 1024,
                  {0: stairs(400, 400, 399), 1: stairs(400, 171, 10)}, {0: [2400, 2400, 2394], 1: [2400, 1026, 60]},
                  [(9, 1), (8, 2), (8, 2)], [2400, 1530, 1530], [RB, RB, RB], capped=6, post=True, grids=True, witness=True,
                  buckets={(0, 0, 1, 0): 2400, (1, 0, 1, 0): 1530, (1, 0, 1, 1): 870, (2, 1, 2, 0): 1026, (2, 1, 2, 1): 0}),
    # halves twice: 520 px = one 1024 px segment; all 2400 hits of a row lie left of x = 512, so the first halving changes nothing
    "b-halve2": _c("b", [(8, 8, 6)], (2, 520, 11), -1.0, 1024,
                   {0: stairs(400, 400, 399), 1: stairs(400, 300, 2)}, {0: [2400, 2400, 2394], 1: [2400, 1800, 12]},
                   [(10, 1), (9, 2), (8, 3)], [2400, 2400, 1530], [RB, RB, RB], capped=6,
                   buckets={(1, 0, 1, 0): 2400, (1, 0, 1, 1): 0, (2, 0, 1, 0): 1530, (2, 0, 1, 1): 870, (2, 0, 1, 2): 0}),
    # ---- (c) ordering units of 2048 hits per page; empty pages between; caps at a call's count, one less, the unit, 1, inside the second unit
    "c-units": _c("c", [(8, 8, 1)], (13, 692, 73), -1.0, 3000,
                  {1: block(1, 1), 3: block(89, 23), 5: block(64, 32), 7: block(683, 3), 9: block(64, 64), 11: block(241, 17)},
                  {1: [1], 3: [89] * 23, 5: [64] * 32, 7: [683] * 3, 9: [64] * 64, 11: [241] * 17},
                  [(10, 1)] * 3, [683] * 3, [R, R, R], capped=2, caps=(4097, 4096, 2049, 2048, 2047, 1), post=True, grids=True),
    # three templates interleaved across the unit boundaries (a hit's rank in its call = its unit's base rank + the unit's earlier hits of that t):
    # pages of 2049 = 3 x 683 and 4098 hits, calls of 683 and 1366 hits, the cap inside the second page's calls
    "c-units-t3": _c("c", [(8, 8, 3)], (3, 692, 12), -1.0, 1000, {0: block(683, 1), 2: block(683, 2)}, {0: [2049], 2: [2049, 2049]},
                     [(10, 1), (9, 2), (9, 2)], [2049, 1533, 1533], [RB, RB, RB], capped=3, buckets={(1, 2, 2, 0): 1533, (1, 2, 2, 1): 516}),
    # order_units_kernel walks the pages 1024 at a time
    "c-pages-1023": _c("c", [(8, 8, 1)], (1023, 24, 12), 0.95, 1024, {0: plant((0, 1, 1), (0, 4, 16)), 1022: plant((0, 2, 9))},
                       {0: {1: 1, 4: 1}, 1022: {2: 1}}, [(5, 1)] * 3, [1] * 3, [R, R, R], witness=True),
    "c-pages-1024": _c("c", [(8, 8, 1)], (1024, 24, 12), 0.95, 1024, {0: plant((0, 1, 1)), 1022: plant((0, 2, 9)), 1023: plant((0, 4, 16), (0, 4, 1))},
                       {0: {1: 1}, 1022: {2: 1}, 1023: {4: 2}}, [(5, 1)] * 3, [2] * 3, [R, R, R]),
    "c-pages-1025": _c("c", [(8, 8, 1)], (1025, 24, 12), 0.95, 1, {0: plant((0, 1, 1)), 1022: plant((0, 2, 9)), 1023: plant((0, 3, 5)), 1024: plant((0, 4, 16), (0, 4, 1))},
                       {0: {1: 1}, 1022: {2: 1}, 1023: {3: 1}, 1024: {4: 2}}, [(5, 1)] * 3, [2] * 3, [R, R, R], capped=1),
    # ---- (d) banks around 4096 templates.  -1.0: 44 x T hits per row — library sort under exact sizes, then the legacy tail; 4097 (with an 8 x 8
    # class in the middle of the bank): legacy tail and the sorting form throughout.  The cap (500) cuts the 748-window calls of page 0
    "d-t4095": _c("d", [(4, 7, 4095)], (2, 48, 24), -1.0, 500, {0: block(44, 17), 1: block(19, 11)},
                  {0: [44 * 4095] * 17, 1: [19 * 4095] * 11}, [(6, 1), (0, 0), (0, 0)], [44 * 4095, 31 * 4095, 31 * 4095], [RL, LG, LG], verify="chunks", chunks=4, capped=4095),
    "d-t4096": _c("d", [(4, 7, 4096)], (2, 48, 24), -1.0, 500, {0: block(44, 17), 1: block(19, 11)},
                  {0: [44 * 4096] * 17, 1: [19 * 4096] * 11}, [(6, 1), (0, 0), (0, 0)], [44 * 4096, 31 * 4096, 31 * 4096], [RL, LG, LG], verify="chunks", chunks=4, capped=4096,
                  grids=True),
    "d-t4097": _c("d", [(4, 7, 2000), (8, 8, 1), (4, 7, 2096)], (2, 48, 24), -1.0, 500, {0: block(44, 17), 1: block(19, 11)},
                  {0: [44 * 4096 + 40] * 16 + [44 * 4096], 1: [19 * 4096 + 19] * 11}, [(0, 0)] * 3, [44 * 4096 + 40] * 3, [LG, LG, LG], verify="none", capped=4097),
    "d-t4095-plant": _c("d", [(4, 7, 4095)], (2, 48, 24), 0.95, 1024, {0: plant((0, 1, 1), (4094, 1, 44), (2047, 9, 20), (2048, 17, 44)), 1: plant((4094, 17, 1))},
                        {0: {1: 2, 9: 1, 17: 1}, 1: {17: 1}}, [(6, 1)] * 3, [2] * 3, [R, R, R], verify="chunks", chunks=4, witness=True),
    "d-t4096-plant": _c("d", [(4, 7, 4096)], (2, 48, 24), 0.95, 1024, {0: plant((0, 1, 1), (4095, 1, 44), (2047, 9, 20), (2048, 17, 44)), 1: plant((4095, 17, 1))},
                        {0: {1: 2, 9: 1, 17: 1}, 1: {17: 1}}, [(6, 1)] * 3, [2] * 3, [R, R, R], verify="chunks", chunks=4, post=True),
    "d-t4097-plant": _c("d", [(4, 7, 2000), (8, 8, 1), (4, 7, 2096)], (2, 48, 24), 0.95, 1024,
                        {0: plant((0, 1, 1), (4096, 1, 44), (2000, 9, 20), (2001, 17, 44)), 1: plant((4096, 17, 1), (2000, 1, 40))},
                        {0: {1: 2, 9: 1, 17: 1}, 1: {1: 1, 17: 1}}, [(0, 0)] * 3, [2] * 3, [LG, LG, LG], verify="none"),
    # ---- (e) bucket counts at the edges of the prefix's pieces (16 waves, multiples of 256): 11, 256, 257, 4096, 4097 buckets, hits only in the first
    # bucket that can hold one (page 0, y = 1: row 0 never emits) and in the very last (a template one pixel high reaches y = r_h - 1)
    "e-11": _c("e", [(8, 1, 1)], (1, 24, 11), 0.95, 1024, {0: plant((0, 1, 1), (0, 10, 16))}, {0: {1: 1, 10: 1}}, [(5, 1)] * 3, [1] * 3, [R, R, R], witness=True),
    "e-256": _c("e", [(8, 1, 1)], (4, 24, 64), 0.95, 1024, {0: plant((0, 1, 1)), 3: plant((0, 63, 16))}, {0: {1: 1}, 3: {63: 1}}, [(5, 1)] * 3, [1] * 3, [R, R, R]),
    "e-257": _c("e", [(8, 1, 1)], (1, 24, 257), 0.95, 1024, {0: plant((0, 1, 1), (0, 256, 16))}, {0: {1: 1, 256: 1}}, [(5, 1)] * 3, [1] * 3, [R, R, R], post=True),
    "e-4096": _c("e", [(8, 1, 1)], (16, 24, 256), 0.95, 1024, {0: plant((0, 1, 1)), 15: plant((0, 255, 16))}, {0: {1: 1}, 15: {255: 1}}, [(5, 1)] * 3, [1] * 3, [R, R, R]),
    "e-4097": _c("e", [(8, 1, 1)], (17, 24, 241), 0.95, 1024, {0: plant((0, 1, 1)), 16: plant((0, 240, 16))}, {0: {1: 1}, 16: {240: 1}}, [(5, 1)] * 3, [1] * 3, [R, R, R],
                 grids=True),
}
GROUPS = ("a", "b", "c", "d", "e")


def seed_of(case_id):
    return SEED0 ^ zlib.crc32(case_id.encode())  # of the id alone: a new case leaves the others' banks as they are


def row_targets(case):
    """-> {(page, y): hits} of the non-empty page rows."""
    out = {}
    for p, r in case["rows"].items():
        for y, n in (r.items() if isinstance(r, dict) else enumerate(r, 1)):
            if n:
                out[(p, y)] = n
    return out


def build(case_id):
    """-> (case, bank, luma pages (n, r_h, r_w): 255 = paper, what Scanner.set_pages takes; the oracle takes O.invert of one)."""
    case = CASES[case_id]
    rng = np.random.default_rng(seed_of(case_id))
    needles = []
    for n_w, n_h, count in case["classes"]:
        for _ in range(count):
            nd = rng.integers(0, 256, (n_h, n_w), dtype=np.uint8)
            nd[0, 0], nd[-1, -1] = 255, 0  # never constant
            needles.append(nd)
    bank = bank_of(needles)
    n_pages, r_w, r_h = case["geom"]
    ink = np.zeros((n_pages, r_h, r_w), np.uint8)
    for p, (kind, arg) in case["pages"].items():
        if kind == "stairs":
            assert all(a >= b for a, b in zip(arg, arg[1:])), "stairs: live counts must not increase"
            for y, live in enumerate(arg, 1):
                if live:
                    ink[p, y, : live + 1] = rng.integers(1, 256, live + 1, dtype=np.uint8)
            ink[p, 0] = ink[p, 1]  # (row 0 belongs to no window that emits: y >= 1)
        else:
            for t, y, x in arg:
                nd = bank.needle(t)
                assert not ink[p, y:y + nd.shape[0], x:x + nd.shape[1]].any(), "planted templates overlap"
                ink[p, y:y + nd.shape[0], x:x + nd.shape[1]] = nd
    return case, bank, (255 - ink).astype(np.uint8)


def cap_full(case):
    """A cap no call of the case reaches: its lists are the uncapped ones."""
    n_pages, r_w, r_h = case["geom"]
    return 64 if case["thr"] > 0 else r_w * r_h


_ORACLE = {}


def oracle_lists(case_id, cap=None):
    """The oracle's lists of the whole batch at `cap` (None: uncapped), computed once per process and left unchanged:
    (counts (n_pages, T) uint32, lists [page][template] of MATCH_DTYPE arrays)."""
    key = (case_id, cap)
    if key not in _ORACLE:
        case, bank, luma = build(case_id)
        c = cap_full(case) if cap is None else cap
        seen, counts, lists = {}, [], []
        for pg in luma:
            k = pg.tobytes()
            if k not in seen:  # (the paper pages of a batch are one page)
                cnt, m = O.scan_page(O.invert(pg), bank, case["thr"], c, use_ref=False)
                seen[k] = (cnt.copy(), [m[t, : cnt[t]].copy() for t in range(len(cnt))])
            counts.append(seen[k][0])
            lists.append(seen[k][1])
        _ORACLE[key] = (np.array(counts, np.uint32), lists)
    return _ORACLE[key]


def hits_of(lists):
    """Uncapped lists -> (page, y, x, t) int64 arrays of every hit."""
    P, Y, X, TT = [], [], [], []
    for p, pl in enumerate(lists):
        for t, m in enumerate(pl):
            if len(m):
                P.append(np.full(len(m), p, np.int64))
                Y.append(m["y"].astype(np.int64))
                X.append(m["x"].astype(np.int64))
                TT.append(np.full(len(m), t, np.int64))
    if not P:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    return np.concatenate(P), np.concatenate(Y), np.concatenate(X), np.concatenate(TT)


def first_shift(r_w, T):
    """row_segments on a setup's first scan: one segment per 2^19 window-templates, no narrower than 32 px."""
    sh = 0
    while (1 << sh) < r_w:
        sh += 1
    while sh > 5 and (1 << sh) * T > (1 << 19):
        sh -= 1
    return sh


def bucket_sizes(case, P, Y, X, sh):
    """-> hits per bucket, index (page * r_h + y) * n_seg + (x >> sh)."""
    n_pages, r_w, r_h = case["geom"]
    n_seg = (r_w + (1 << sh) - 1) >> sh
    return np.bincount((P * r_h + Y) * n_seg + (X >> sh), minlength=n_pages * r_h * n_seg), n_seg


def plan(case, P, Y, X):
    """The host's choices for three scans of one context (exact sizes, then estimated twice), restated from the hits: list of dicts
    (path, seg, row_max: the largest bucket under the layout the row tail has or would have, stat: size_estimate_stats()['row_max'] after it)."""
    n_pages, r_w, r_h = case["geom"]
    T = sum(c[2] for c in case["classes"])
    est = None  # (row_max, seg_shift) of the previous scan
    out = []
    for i in range(3):
        sh = est[1] if est and est[1] else first_shift(r_w, T)
        sizes, n_seg = bucket_sizes(case, P, Y, X, sh)
        largest = int(sizes.max()) if len(P) else 0
        rows = T <= 4096 and len(sizes) <= (1 << 22)
        bound = largest
        if rows and est is not None:
            bound = est[0] + est[0] // 4 + 16
            rows = est[0] != 0 and bound <= 4096
            assert not rows or largest <= bound, "the case would be redone with exact sizes: not what it is there for"
        if not rows:
            path, row_cap, seg, seen = "legacy", 0, (0, 0), 0  # (the legacy tail leaves no largest bucket: the segments stay)
        else:
            row_cap = 4096 if bound <= 4096 else 0
            path = "rows+lib" if not row_cap else "rows+big" if bound > 1024 else "rows"
            seg, seen = (sh, n_seg), largest
        stat = max(seen, 1) if row_cap else 0
        out.append(dict(path=path, seg=seg, row_max=largest, stat=stat))
        est = (stat, sh - 1 if seen > 2048 and sh > 5 else sh)
    return out

"""focr_get_runners (font_ocr_amd/csrc/hip/post.hip, walk_kernel<true>) stated twice, and the hit lists that test it.

brute_force is the definition (include/focr_ncc.h): for every output character of process_hits its overlap group G -- the kept hits
of its anchored row that partition_by puts together, anchored on the group's first element, which is always a member --, `members`
= |G|, and the runner = what max_by(f32::total_cmp) returns over {h in G : letter(h) != letter(W)}, W the winner: the LAST maximum
in (x, t) order.  No such hit: template_index = letter = NO_RUNNER, similarity = -inf, x = 0.  Its winners must be those of
focr_walk_model.reference_lines (oracle.process_hits), which pins the grouping to the reference.

walk_row_runners is the kernel's walk of one row on 64-lane numpy vectors, statement for statement, in the manner of
focr_walk_model.walk_row: per open group it carries `members` and a top-2 over distinct letters, a1 = (order, index, letter) of the
best member and a2 = the best member whose letter differs from a1's; a chunk gives (m1, m2) the same way and the merge keeps, as
a2, the last maximum of {the loser of a1 / m1, a2, m2} whose letter differs from the new a1's.  "No value" is a flag (None here),
not order 0: order 0 is the similarity 0xFFFFFFFF.  (The kernel carries a member's template and x beside its index and
turns its order back into the similarity's bits; the model keeps the index and reads the three from the list.)

The Case families put winners and runners on chunk edges and lanes 0 / 63, demote carried bests, hide capped hits of another
letter, and use every odd similarity as a runner.  Letters come from the x2 bank (95 glyphs x 4 shifts)."""
import os

import numpy as np

import focr_walk_model as W
from focr_walk_model import I32_MAX, I32_MIN, LANES, N_TEMPLATES, OVERLAPS, Case, order_key

NO_RUNNER = 0xFFFFFFFF
RUNNER_DTYPE = np.dtype([("members", "<u4"), ("letter", "<u4"), ("template_index", "<u4"), ("similarity", "<f4"), ("x", "<u2"), ("reserved", "<u2")])
_ALL = (1 << LANES) - 1
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bank_letters():
    from font_ocr_amd import Bank

    letters = Bank.load(os.path.join(_GOLD, "bank_dejavu13_ascii95_x2.bin")).templates["letter"].astype(np.uint32)
    assert len(letters) == N_TEMPLATES
    return letters


LETTERS = bank_letters()
_GLYPHS = np.unique(LETTERS)
TI = [np.flatnonzero(LETTERS == g) for g in _GLYPHS]  # glyph -> its four template indices (one per shift)
assert len(TI) == 95 and all(len(t) == 4 for t in TI)
A, B, C, D = 40, 17, 63, 80  # four glyphs of the bank


def bits(*words):
    return np.array(words, np.uint32).view(np.float32)


def _records(case, members, runners):
    """RUNNER_DTYPE records of groups with these sizes and runners (element indices; -1: none)."""
    members, runners = np.asarray(members, np.int64), np.asarray(runners, np.int64)
    out = np.zeros(len(members), RUNNER_DTYPE)
    has = runners >= 0
    i = runners[has]
    out["members"] = members
    out["letter"], out["template_index"], out["similarity"] = NO_RUNNER, NO_RUNNER, -np.inf
    out["letter"][has], out["template_index"][has], out["x"][has] = LETTERS[case.t[i]], case.t[i], case.x[i]
    sim = out["similarity"].copy()
    sim.view(np.uint32)[has] = case.sim.view(np.uint32)[i]  # the bits, whatever a NaN does on its way
    out["similarity"] = sim
    return out


def _rows(case):
    """(page, first, end) of the anchored rows, in output order."""
    kept = case.keep != 0
    row = case.page.astype(np.int64) * case.r_h + case.y
    keep_row = np.zeros(case.n_pages * case.r_h, bool)
    keep_row[row[kept & (case.sim >= np.float32(case.anchor))]] = True
    starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]]) if len(row) else np.zeros(0, np.int64)
    return [(int(row[b]) // case.r_h, int(b), int(e)) for b, e in zip(starts, np.r_[starts[1:], len(row)]) if keep_row[row[b]]]


def _last_max(order, idx):
    """max_by(total_cmp) over the elements idx (ascending): the last maximum."""
    best = None
    for i in idx:
        if best is None or order[i] >= order[best]:
            best = i
    return best


def brute_force(case):
    """-> (lines, records): per page its lines as lists of winning element indices (as focr_walk_model.reference_lines), and one
    RUNNER_DTYPE record per output character, in output order."""
    order = order_key(case.sim)
    lines = [[] for _ in range(case.n_pages)]
    members, runners = [], []
    letter = LETTERS[case.t]
    for page, b, e in _rows(case):
        kept = [i for i in range(b, e) if case.keep[i]]
        line, k = [], 0
        while k < len(kept):
            x0 = int(case.x[kept[k]])
            group = [kept[k]]
            k += 1
            while k < len(kept) and abs(int(case.x[kept[k]]) - x0) <= case.overlap:
                group.append(kept[k])
                k += 1
            w = _last_max(order, group)
            runner = _last_max(order, [i for i in group if letter[i] != letter[w]])
            line.append(w)
            members.append(len(group))
            runners.append(-1 if runner is None else runner)
        lines[page].append(line)
    return lines, _records(case, members, runners)


def _beats(a, b):
    """top_beats: b takes a's place as the last maximum.  A value is (order, index, letter) or None."""
    return b is not None and (a is None or b[0] > a[0] or (b[0] == a[0] and b[1] > a[1]))


def walk_row_runners(x, order, kept, letter, overlap):
    """walk_kernel<true> on one anchored row -> per group (winner index, members, runner index or None), indices into the extent."""
    e = len(x)
    lane = np.arange(LANES)
    out = []
    open_ = False
    anchor = 0
    a1 = a2 = None
    members = 0
    for base in range(0, e, LANES):
        i = np.minimum(base + lane, e - 1)
        valid = (base + lane < e) & kept[i]
        xl = np.where(valid, x[i], 0x7FFFFFFF)
        ordl = np.where(valid, order[i], 0)
        let = np.where(valid, letter[i], 0)
        vmask = W._ballot(valid)
        pos = 0
        opened_at = -1
        trips = 0
        while pos < 64:
            trips += 1
            if trips > W.TRIP_BOUND:
                raise W.TripBoundExceeded(f"chunk at element {base}: more than {W.TRIP_BOUND} trips (overlap {overlap})")
            if not open_:
                cand = vmask & (_ALL << pos) & _ALL
                if not cand:
                    break
                pos = W._ctz(cand)
                anchor = int(xl[pos])
                opened_at = pos
                open_ = True
                a1 = a2 = None
                members = 0
            inn = valid & (lane >= pos) & ((lane == opened_at) | ((xl - anchor <= overlap) & (anchor - xl <= overlap)))
            inmask = W._ballot(inn)
            brk = vmask & ~inmask & (_ALL << pos) & _ALL
            stop = W._ctz(brk) if brk else 64
            member = inn & (lane < stop)
            mx = int(np.where(member, ordl, 0).max())
            top = W._ballot(member & (ordl == mx))
            members += bin(W._ballot(member)).count("1")
            if top:
                l1 = top.bit_length() - 1
                m1 = (mx, base + l1, int(let[l1]))
                m2 = None
                other = member & (let != m1[2])
                if W._ballot(other):
                    mx2 = int(np.where(other, ordl, 0).max())
                    l2 = W._ballot(other & (ordl == mx2)).bit_length() - 1
                    m2 = (mx2, base + l2, int(let[l2]))
                lose = m1
                if a1 is None or m1[0] >= a1[0]:
                    lose, a1 = a1, m1
                s = None
                if lose is not None and lose[2] != a1[2]:
                    s = lose
                if a2 is not None and a2[2] != a1[2] and _beats(s, a2):
                    s = a2
                if m2 is not None and m2[2] != a1[2] and _beats(s, m2):
                    s = m2
                a2 = s
            if stop < 64:
                out.append((a1[1], members, None if a2 is None else a2[1]))
                open_ = False
            pos = stop
    if open_:
        out.append((a1[1], members, None if a2 is None else a2[1]))
    return out


def model(case):
    """mark_anchor_rows + walk_kernel<true> over a Case -> (lines, records), as brute_force gives them."""
    order = order_key(case.sim)
    x = case.x.astype(np.int64)
    kept = case.keep != 0
    letter = LETTERS[case.t].astype(np.int64)
    lines = [[] for _ in range(case.n_pages)]
    members, runners = [], []
    for page, b, e in _rows(case):
        groups = walk_row_runners(x[b:e], order[b:e], kept[b:e], letter[b:e], case.overlap)
        lines[page].append([b + w for w, _, _ in groups])
        members += [m for _, m, _ in groups]
        runners += [-1 if r is None else b + r for _, _, r in groups]
    return lines, _records(case, members, runners)


def same_records(got, want):
    """Field by field, the similarity as bytes.  Returns the name of the first field that differs, or None."""
    if len(got) != len(want):
        return "length"
    for f in ("members", "letter", "template_index", "x", "reserved"):
        if not np.array_equal(got[f], want[f]):
            return f
    return None if np.ascontiguousarray(got["similarity"]).tobytes() == np.ascontiguousarray(want["similarity"]).tobytes() else "similarity"


# ---- the hit lists -------------------------------------------------------------------------------------------------------------

def _t(glyph, shift=0):
    return int(TI[glyph][shift])


def small_groups():
    """Groups of one; four shifts of one glyph (no runner); two letters at equal similarity (the later wins, margin 0); a winner
    letter with several members above the runner."""
    one = [(0, 1, 10 * k + 3, _t(k), 0.96 + 0.001 * k, 1) for k in range(8)]
    shifts = [(0, 2, 20 * j + 3, TI[g], np.array([0.96, 0.99, 0.97, 0.99], np.float32), 1) for j, g in enumerate((A, B, C))]
    # equal similarity, both orders of the letters in (x, t): the later element wins, the earlier one is the runner
    s2, s3 = np.full(2, 0.97, np.float32), np.full(3, 0.97, np.float32)
    ties = [(0, 3, 10, [_t(A), _t(B)], s2, 1), (0, 3, 40, [_t(B, 1), _t(A, 1)], s2, 1), (0, 3, [70, 71], [_t(B), _t(A)], s2, 1),
            (0, 3, [100, 100, 101], [_t(A), _t(B), _t(A, 2)], s3, 1)]
    above = [(0, 4, 10, np.r_[TI[A], TI[B]], np.array([0.99, 0.985, 0.98, 0.975, 0.97, 0.96, 0.97, 0.5], np.float32), 1),
             (0, 4, [50, 50, 51, 51, 52, 52], [_t(B), _t(A), _t(A, 1), _t(C), _t(A, 2), _t(B, 3)],
              np.array([0.96, 0.99, 0.98, 0.97, 0.985, 0.97], np.float32), 1)]
    return [Case("groups-of-one", one, overlap=2), Case("four-shifts", shifts, overlap=2), Case("equal-two-letters", ties, overlap=5),
            Case("several-above-runner", above, overlap=5), Case("small-all", one + shifts + ties + above, overlap=5)]


def placed_groups():
    """One group per row of 63 .. 200 members; the winner (0.99) and the runner (0.98) on every ordered pair of the elements 0, 63,
    64, 127, 128 and the last: (chunk 0, chunk 1) and (chunk 1, chunk 0), lanes 0 and 63.  The group is made by equal x (the
    templates 0 .. n-1 in turn, so every letter occurs) and by a huge overlap over distinct x (letters of three glyphs)."""
    rng = np.random.default_rng(200)
    out = []
    t3 = np.r_[TI[A], TI[B], TI[C]]
    for n in (63, 64, 65, 127, 128, 129, 200):
        spots = sorted({p for p in (0, 63, 64, 127, 128, n - 1) if p < n})
        pairs = [(w, r) for w in spots for r in spots if w != r]
        same, wide = [], []
        k = np.arange(n)
        assert all(LETTERS[w] != LETTERS[r] for w, r in pairs)  # (same x: element k is template k)
        for y, (w, r) in enumerate(pairs):
            s = W._sims(rng, n)
            s[w], s[r] = 0.99, 0.98
            same.append((0, y, 9, k, s, 1))
            t = t3[rng.integers(0, 12, n)]
            t[w], t[r] = _t(A, w % 4), _t(B, r % 4)
            wide.append((0, y, k, t, s, 1))
        out.append(Case(f"placed{n}-samex", same, overlap=0, r_h=len(pairs)))
        out.append(Case(f"placed{n}-wide", wide, overlap=I32_MAX, r_h=len(pairs)))
    return out


def demotions():
    """What the merge must demote.  One wide group per row over two or three chunks, fillers of four letters below 0.8:
    (1) carried best A and second B, then a later, higher B': the runner is A;  (2) the later chunk's second C beats the carried A;
    (3) a chunk whose best shares the carried best's letter while its second beats the carried second -- with the chunk's best
    below and above the carried one;  (4) the same across three chunks, and with ties between the candidates."""
    rng = np.random.default_rng(3)
    t4 = np.r_[TI[A], TI[B], TI[C], TI[D]]
    plans = [
        {3: (A, 0.97), 10: (B, 0.96), 70: (B, 0.99)},
        {3: (A, 0.97), 10: (B, 0.96), 70: (B, 0.99), 90: (C, 0.98)},
        {3: (A, 0.99), 10: (B, 0.90), 70: (A, 0.95), 90: (C, 0.93)},
        {3: (A, 0.99), 10: (B, 0.90), 70: (A, 0.995), 90: (C, 0.93)},
        {3: (A, 0.97), 10: (B, 0.96), 70: (C, 0.98), 90: (A, 0.975), 130: (B, 0.99), 140: (C, 0.985)},
        {63: (A, 0.97), 64: (B, 0.97), 127: (A, 0.97), 128: (B, 0.97)},                 # every candidate tied: the last of each letter
        {0: (B, 0.97), 63: (A, 0.97), 64: (C, 0.97), 129: (A, 0.97)},
        {5: (A, 0.99), 6: (B, 0.98), 70: (B, 0.98), 135: (C, 0.98)},                    # tied seconds: the last one
        {5: (A, 0.99), 70: (A, 0.99), 135: (A, 0.99), 136: (B, 0.5)},                   # the only other letter sits below every filler's rank
    ]
    parts = []
    for y, plan in enumerate(plans):
        n = 150
        t = t4[rng.integers(0, 16, n)]
        s = rng.uniform(0.5, 0.8, n).astype(np.float32)
        if y == len(plans) - 1:
            t = TI[A][rng.integers(0, 4, n)]  # nothing but A and one B
        for p, (g, v) in plan.items():
            t[p], s[p] = _t(g, p % 4), v
        parts.append((0, y, np.arange(n), t, s, 1))
    return [Case("demotions", parts, overlap=I32_MAX, r_h=len(plans)), Case("demotions-a0.5", parts, anchor=0.5, overlap=I32_MAX, r_h=len(plans))]


def capped_others():
    """Hits cut off by the cap (keep = 0) of ANOTHER letter at similarity 1.0, inside groups and on chunk edges: neither the runner
    nor counted.  Also a capped opener, and a group whose only other-letter hits are capped (no runner)."""
    n = 130
    k = np.arange(n)
    parts = []
    for y, capped in enumerate(([63, 64], [127, 128], [0, 1, 62, 63, 64, 65], [20, 100], list(range(60, 70)), [0])):
        t = TI[A][k % 4].copy()
        s = np.full(n, 0.6, np.float32)
        keep = np.ones(n, np.uint8)
        t[30], s[30] = _t(A, 1), 0.99
        t[110], s[110] = _t(B), 0.9
        t[capped], s[capped], keep[capped] = _t(C, 2), 1.0, 0
        parts.append((0, y, k, t, s, keep))
    t = TI[A][k % 4].copy()  # every other-letter hit is capped: no runner
    s = np.full(n, 0.6, np.float32)
    s[5] = 0.99
    keep = np.ones(n, np.uint8)
    t[[10, 63, 64, 129]], s[[10, 63, 64, 129]], keep[[10, 63, 64, 129]] = _t(B), 1.0, 0
    parts.append((0, 6, k, t, s, keep))
    same = [(0, 0, 7, np.arange(n), np.where(k == 50, 0.99, 0.6).astype(np.float32), (k % 3 != 0).astype(np.uint8))]
    return [Case("capped-others", parts, overlap=I32_MAX, r_h=7), Case("capped-others-ov3", parts, overlap=3, r_h=7),
            Case("capped-samex", same, overlap=0, r_h=1)]


def lone_overlaps():
    """overlap -1 and INT32_MIN: every kept hit of an anchored row is a character: members 1, no runner."""
    rng = np.random.default_rng(11)
    parts = W._mixed(rng, n_rows=4)
    return [Case(f"lone-ov{ov}", parts, overlap=ov, r_w=160) for ov in (-1, I32_MIN)]


SPECIALS = np.r_[np.array([-0.0, 0.0, 1e-45, -0.25, np.inf, -np.inf], np.float32),
                 bits(0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF)]


def special_runners():
    """Runner candidates -0.0, 0.0, a subnormal, a negative value, +-inf, NaNs of both signs, and 0xFFFFFFFF as the only other-letter
    member (order 0: it comes back as a runner with its bits intact).  +inf and the positive NaNs rank above every finite
    similarity, so there the odd value wins and the finite one is the runner.  Behind 0, 62 or 63 filler hits of a group of their
    own, so that the groups also straddle a chunk edge."""
    out = []
    for lead in (0, 62, 63):
        xs, ts, ss = [np.zeros(lead, np.int64)], [np.arange(lead)], [np.full(lead, 0.5, np.float32)]
        for g, v in enumerate(SPECIALS):
            x0 = 10 + 9 * g
            xs.append(np.array([x0, x0, x0 + 1, x0 + 1]))
            ts.append(np.array([_t(A), _t(B), _t(A, 1), _t(A, 2)]))
            ss.append(np.r_[np.float32(0.97), v, np.float32(0.5), np.float32(0.96)].astype(np.float32))
            x0 += 3  # two other-letter members: the odd value and one of its letter's shifts below / above it
            xs.append(np.array([x0, x0, x0 + 1]))
            ts.append(np.array([_t(B, 1), _t(A, 3), _t(B, 2)]))
            ss.append(np.r_[v, np.float32(0.98), np.float32(-0.5)].astype(np.float32))
            x0 += 3  # under the highest similarity there is, so that +inf and the positive NaNs are runners too
            xs.append(np.array([x0, x0]))
            ts.append(np.array([_t(A), _t(B, 3)]))
            ss.append(np.r_[bits(0x7FFFFFFF), v].astype(np.float32))
        part = (0, 1, np.concatenate(xs), np.concatenate(ts), np.concatenate(ss), 1)
        out.append(Case(f"specials-lead{lead}", [part], anchor=0.95, overlap=1))
    # every member an odd value: pairs of two letters, all of them runners of each other
    xs = np.repeat(10 + 4 * np.arange(len(SPECIALS) - 1), 2)
    ts = np.tile([_t(A), _t(B)], len(SPECIALS) - 1)
    ss = np.stack([SPECIALS[:-1], SPECIALS[1:]], 1).ravel()
    out.append(Case("specials-pairs", [(0, 1, xs, ts, ss, 1)], anchor=float("-inf"), overlap=1))
    return out


def row_edges():
    """17 consecutive anchored rows (one wave takes 16, the next 1), and rows of two pages with unanchored rows between them: the
    records stay aligned with the characters."""
    def row(p, y, anchored, seed):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(2, 9))
        x = np.sort(rng.choice(60, n, replace=False))
        s = rng.uniform(0.5, 0.94, n).astype(np.float32)
        if anchored:
            s[rng.integers(0, n)] = 0.97
        return (p, y, x, np.r_[TI[A], TI[B], TI[C]][rng.integers(0, 12, n)], s, 1)

    seventeen = [row(0, y, True, y) for y in range(17)]
    pages = [row(p, y, (p * 17 + y) % 3 != 1, 100 + p * 17 + y) for p in range(2) for y in (0, 3, 5, 6, 15, 16)]
    return [Case("rows17", seventeen, overlap=4, r_w=64, r_h=17, expect_lines=17), Case("rows17-of-40", seventeen, overlap=4, r_w=64, r_h=40),
            Case("two-pages", pages, overlap=4, n_pages=2, r_w=64, r_h=17, expect_lines=10)]


def fuzz(n_lists=300, seed=0x4E55):
    """Seeded lists whose templates are 3 glyphs x 4 shifts, so that letters collide inside every group."""
    t12 = np.r_[TI[A], TI[B], TI[C]]
    pool = np.r_[W.FUZZ_POOL, bits(0xFFFFFFFF, 0x7FC00000), np.float32(-np.inf)]
    out = []
    for i in range(n_lists):
        rng = np.random.default_rng(seed + i)
        n_pages, r_h, r_w = int(rng.integers(1, 4)), int(rng.choice([3, 16, 17, 31, 40])), int(rng.integers(8, 260))
        parts = []
        for p in range(n_pages):
            for y in rng.choice(r_h, size=int(rng.integers(0, min(r_h, 6) + 1)), replace=False):
                n = int(rng.choice([1, 3, 63, 64, 65, 128, 129, 250]))
                x0, spread = int(rng.integers(0, r_w)), int(rng.choice([1, 3, 8, r_w]))
                x = np.minimum(x0 + rng.integers(0, spread, n), r_w - 1)
                u = np.unique(x.astype(np.int64) * N_TEMPLATES + t12[rng.integers(0, 12, n)])
                m = len(u)
                s = pool[rng.integers(0, len(pool), m)] if rng.random() < 0.7 else rng.uniform(-0.2, 1.0, m).astype(np.float32)
                keep = np.ones(m, np.uint8)
                mode = int(rng.integers(0, 3))
                if mode == 1:
                    keep = (rng.random(m) < 0.8).astype(np.uint8)
                elif mode == 2:
                    a = int(rng.integers(0, m))
                    keep[a:a + int(rng.integers(1, 80))] = 0
                parts.append((p, int(y), u // N_TEMPLATES, u % N_TEMPLATES, s, keep))
        anchor = [0.95, 0.97, 0.5, -1.0, float("-inf"), float("inf"), float("nan")][int(rng.integers(0, 7))]
        overlap = int(rng.choice(OVERLAPS + (2, 5, 8, 12)))
        out.append(Case(f"rfuzz{i}", parts, anchor=anchor, overlap=overlap, n_pages=n_pages, r_w=r_w, r_h=r_h))
    return out


FAMILIES = {"small_groups": small_groups, "placed_groups": placed_groups, "demotions": demotions, "capped_others": capped_others,
            "lone_overlaps": lone_overlaps, "special_runners": special_runners, "row_edges": row_edges, "runner_fuzz": fuzz}

"""The cases of tests/compat_cases.py have the properties they are there for, by the oracle alone (no device): hit counts on either side of
compat_call's 65 536-hit block, per-row tables that reach every row-tail length of the reference kernel, A/B pairs whose lists differ (a
stale upload cannot pass) and whose changed bytes lie where the content hash once folded them together.  Where the compiled reference
kernel is present the restatement is held against it on every call."""
import numpy as np
import pytest

import compat_cases as CC
from oracle import oracle as O


def _want(c):
    """The restatement's list; equal to the compiled reference's where that exists."""
    want = CC.oracle(c, use_ref=False)
    if O.have_ref():
        assert CC.oracle(c, use_ref=True).tobytes() == want.tobytes()
    return want


def _in_yx_order(m):
    key = m["y"].astype(np.int64) << 16 | m["x"].astype(np.int64)
    return bool((np.diff(key) > 0).all())


@pytest.mark.parametrize("which", sorted(CC.BIG_NEEDLES))
def test_big_calls_emit_more_than_the_pinned_block_holds(which):
    page, needle, stats = CC.big(which)
    n_w, n_h = CC.BIG_NEEDLES[which]
    assert needle.shape == (n_h, n_w) and page.shape == (CC.BIG_H, CC.BIG_W)
    calls = CC.big_calls(which)
    assert [c["n_out"] for c in calls] == [1, 1024, 1 << 17]
    full = _want(calls[-1])
    assert CC.PIN_HITS < len(full) < CC.N_OUT_ALL
    assert len(full) == (CC.BIG_W - n_w) * (CC.BIG_H - n_h) == CC.windows(stats[2], CC.BIG_H, n_h)  # every window emits
    assert _in_yx_order(full)
    for c in calls[:-1]:  # the reference stops at n_out: the first n_out of the full list
        assert _want(c).tobytes() == full[: c["n_out"]].tobytes()
    # a fresh thread's first call (n_out = 1) sizes the hit arrays at max(65 536, 4 * n_out) < the hits: it grows and rescans
    assert max(1 << 16, 4 * calls[0]["n_out"]) < len(full)


def test_boundary_calls_sit_on_either_side_of_the_pinned_block():
    calls = CC.boundary_calls()
    page, needle, stats = CC.big("n8")
    full = _want(CC.big_calls("n8")[-1])
    for n, c in calls.items():
        assert CC.windows(c["stats"][2], CC.BIG_H, needle.shape[0]) == n
        got = _want(c)
        assert len(got) == n
        assert got.tobytes() == full[:n].tobytes()  # rows are cut from the bottom: the list is a prefix
    assert sorted(calls) == [CC.PIN_HITS, CC.PIN_HITS + 1]


@pytest.mark.parametrize("which", sorted(CC.TAB_NEEDLES))
def test_caller_tables_reach_every_row_tail_and_change_the_lists(which):
    page, needle, (ps, pr, se) = CC.tables_case(which)
    n_w, n_h = CC.TAB_NEEDLES[which]
    ps0, pr0, se0 = O.prepare_for_size(page, n_w, n_h)
    x_searches = CC.TAB_W - n_w + 1
    rows = range(1, CC.TAB_H - n_h + 1)
    start = np.array([int(se[2 * y]) for y in rows])
    end = np.array([int(se[2 * y + 1]) for y in rows])
    # inside what prepare_for_size filled (the other entries of its tables are stale), never past the last window the page has
    for y, s, e in zip(rows, start, end):
        assert int(se0[2 * y]) <= s <= e <= int(se0[2 * y + 1]) == x_searches
    assert (start > 1).any() and (end < x_searches).any() and (end == x_searches).any() and (start == end).any()
    assert {int(v) for v in (end - start) % 4} == {0, 1, 2, 3}
    assert {1, 2, 3} <= {int(v) for v in (end - start) % 16} and ((end - start) >= 32).any()  # ncc_8_u8: two 16-window blocks, then the scalar tail
    assert len({(s, e) for s, e in zip(start, end)}) > len(start) // 2  # a different table per row
    # the overwritten entries: the four special rnorms and four foreign sums, all inside the rows' ranges
    d_pr = np.argwhere(~((pr == pr0) | (np.isnan(pr) & np.isnan(pr0))))
    d_ps = np.argwhere(ps != ps0)
    assert len(d_pr) == 4 and len(d_ps) == 4
    for y, x in list(d_pr) + list(d_ps):
        assert int(se[2 * y]) <= x < int(se[2 * y + 1])
    vals = [pr[y, x] for y, x in d_pr]
    assert sum(np.isposinf(v) for v in vals) == 1 and sum(np.isnan(v) for v in vals) == 1 and sum(v == 0.0 for v in vals) == 1 and sum(v < 0 for v in vals) == 1
    assert int(ps.max()) < 1 << 31
    # every call: restatement == reference; each edit shows in a list, so a kernel that recomputed its statistics would differ
    plain = [CC.oracle(c) for c in CC.tables_calls(which, edited=False)]
    edited = [_want(c) for c in CC.tables_calls(which)]
    full = [CC.oracle(dict(c, stats=(ps0, pr0, se0))) for c in CC.tables_calls(which)]
    assert [c["thr"] for c in CC.tables_calls(which)] == [-1.0, 0.0, 0.2]
    for p, e, f in zip(plain, edited, full):
        assert 0 < len(e) < 8192 and len(p) < len(f)
        assert p.tobytes() != e.tobytes()
    assert len(edited[0]) > len(edited[1]) > len(edited[2])
    # at -1.0 the four rnorm edits are visible one by one: +inf, NaN and 0.0 take their windows out (or leave a 0), the negative one flips a sign
    p0 = {(int(m["y"]), int(m["x"])): float(m["similarity"]) for m in plain[0]}
    e0 = {(int(m["y"]), int(m["x"])): float(m["similarity"]) for m in edited[0]}
    changed = {k for k in p0 if e0.get(k) != p0[k]}
    assert {(int(y), int(x)) for y, x in list(d_pr) + list(d_ps)} == changed | {k for k in e0 if k not in p0}
    # the planted needle is found where its row's range covers it
    assert any(m["similarity"] > 0.999 for m in edited[2])


@pytest.mark.parametrize("case_id", CC.RES_CASES)
def test_residency_pairs_differ_where_the_hash_looks_last(case_id):
    a, b, which = CC.residency(case_id)
    assert a["page"].shape == (CC.RES_H, CC.RES_W) == b["page"].shape
    npx = CC.RES_W * CC.RES_H
    assert npx % 64 >= 9 and 4 * npx % 64 >= 16 and 8 * npx % 64 >= 16 and 4 * CC.RES_H % 64 >= 12
    ia, ib = CC.inputs_of(a), CC.inputs_of(b)
    for k in range(4):
        assert (ia[k] != ib[k]) == (k == which)  # one input changes, the other three stay
    xa, xb = ia[which], ib[which]
    diff = [i for i in range(len(xa)) if xa[i] != xb[i]]
    body = len(xa) - len(xa) % 64
    if case_id == "page-body":
        assert len(diff) == 1 and diff[0] < body
    elif case_id == "page-tail":
        assert len(diff) == 1 and diff[0] >= body
    else:  # the changed bytes lie in the last n % 64 bytes, pairwise 8 apart, and the former fold of those bytes cannot tell A from B
        assert diff and min(diff) >= body
        assert all((i + 8 in diff) != (i - 8 in diff) for i in diff)
        assert CC.xor_fold(xa[body:]) == CC.xor_fold(xb[body:])
    # B's list is not A's: a second call that scanned A's stale copy fails the device test
    wa, wb = _want(a), _want(b)
    assert 0 < len(wb) < b["n_out"] and 0 < len(wa) < a["n_out"]
    assert wa.tobytes() != wb.tobytes()


def test_degenerate_calls_have_nothing_or_one_row_to_search():
    want = {k: _want(CC.degenerate(k)) for k in CC.DEG_CASES}
    for k in ("n_h == r_h", "n_w == r_w", "n_out == 0"):
        assert len(want[k]) == 0, k
    c = CC.degenerate("n_h == r_h")
    assert c["needle"].shape[0] == CC.DEG_H
    c = CC.degenerate("n_w == r_w")
    assert c["needle"].shape[1] == CC.DEG_W and c["needle"].shape[0] < CC.DEG_H - 1
    c = CC.degenerate("n_out == 0")
    assert len(CC.oracle(dict(c, n_out=1024))) > 0  # only n_out keeps it empty
    one = want["n_h == r_h - 1"]
    assert len(one) > 0 and set(one["y"].tolist()) == {1}

"""The cases of tests/tail_cases.py reach their targets by the oracle alone (no device): bucket sizes, page totals, per-call counts against the
cap and the path the host will choose — known before any GPU time is spent, and a case that misses a target fails here, it is never skipped."""
import numpy as np
import pytest

import tail_cases as TC
from oracle import oracle as O

IDS = sorted(TC.CASES)


@pytest.mark.parametrize("case_id", IDS)
def test_case_reaches_its_targets_on_the_oracle(case_id):
    case, bank, luma = TC.build(case_id)
    n_pages, r_w, r_h = case["geom"]
    T = len(bank)
    assert T == sum(c[2] for c in case["classes"]) and luma.shape == (n_pages, r_h, r_w)
    counts, lists = TC.oracle_lists(case_id)
    assert int(counts.max()) < TC.cap_full(case)  # the lists are uncapped
    P, Y, X, _ = TC.hits_of(lists)
    # hits per page row, and hence per page
    got = {}
    for key, n in zip(*np.unique(P * r_h + Y, return_counts=True)):
        got[(int(key) // r_h, int(key) % r_h)] = int(n)
    assert got == TC.row_targets(case)
    want_pages = np.zeros(n_pages, np.int64)
    for (p, y), n in TC.row_targets(case).items():
        want_pages[p] += n
    assert np.array_equal(counts.sum(1), want_pages)
    # the three scans of one context: segmentation, largest bucket, path
    plans = TC.plan(case, P, Y, X)
    assert [pl["path"] for pl in plans] == case["path"]
    assert [pl["seg"] for pl in plans] == case["seg"]
    assert [pl["row_max"] for pl in plans] == case["row_max"]
    # spot buckets under the layout of the scan they name
    for (scan, p, y, s), n in case["buckets"].items():
        sh, n_seg = case["seg"][scan]
        sizes, ns = TC.bucket_sizes(case, P, Y, X, sh)
        assert ns == n_seg and int(sizes[(p * r_h + y) * n_seg + s]) == n, (scan, p, y, s, int(sizes[(p * r_h + y) * n_seg + s]))
    if case["path"][0] != "legacy":  # in the first layout a page row's segments add up to the row
        sizes, n_seg = TC.bucket_sizes(case, P, Y, X, case["seg"][0][0])
        per_row = sizes.reshape(n_pages * r_h, n_seg).sum(1)
        for (p, y), n in TC.row_targets(case).items():
            assert per_row[p * r_h + y] == n
        assert per_row.sum() == sum(TC.row_targets(case).values())
    # the caps: the reference stops a call at `cap` matches, which are the first `cap` of the uncapped list
    assert int((counts > case["cap"]).sum()) == case["capped"]
    for cap in (case["cap"],) + tuple(case["caps"]):
        c_counts, c_lists = TC.oracle_lists(case_id, cap)
        assert np.array_equal(c_counts, np.minimum(counts, cap))
        for p in range(n_pages):
            for t in range(T):
                if counts[p, t]:
                    assert c_lists[p][t].tobytes() == lists[p][t][:cap].tobytes()
    if case["caps"]:  # a cap at a call's count, one below, 1, and one first reached inside a call's second ordering unit
        biggest = int(counts.max())
        assert biggest in case["caps"] and biggest - 1 in case["caps"] and 1 in case["caps"]
        assert 2048 < case["cap"] < biggest and 2048 in case["caps"]


def test_every_group_has_its_special_cases():
    for g in TC.GROUPS:
        for flag in ("post", "grids", "witness"):
            assert sum(1 for c in TC.CASES.values() if c["group"] == g and c[flag]) == 1, (g, flag)
    assert len({TC.seed_of(k) for k in TC.CASES}) == len(TC.CASES)


@pytest.mark.parametrize("case_id", [k for k in IDS if TC.CASES[k]["witness"]])
def test_second_witness_agrees_on_the_smallest_case_of_each_group(case_id):
    """oracle/rust_witness.py (a literal transliteration of the reference's Rust) against oracle/ncc_oracle.c on a group's smallest case: the live
    ranges and window statistics the construction rests on (prepare_for_size: a row's live windows are [start, end)), and process_hits."""
    from oracle import rust_witness as W

    case, bank, luma = TC.build(case_id)
    n_pages, r_w, r_h = case["geom"]
    counts, lists = TC.oracle_lists(case_id, case["cap"])
    sizes = sorted({(int(t["n_w"]), int(t["n_h"])) for t in bank.templates})
    pages = sorted(case["pages"])[:2] + [p for p in range(n_pages) if p not in case["pages"]][:1]  # two with ink, one of paper
    for p in pages:
        ink = O.invert(luma[p])
        a2 = W.array2_from(ink.tolist())
        for n_w, n_h in sizes:
            ps, pr, se = O.prepare_for_size(ink, n_w, n_h)
            wps, wpr, wse = W.prepare_for_size(a2, n_w, n_h)
            assert list(se) == list(wse), (p, n_w, n_h)
            for y in range(1, r_h - n_h + 1):
                s, e = int(se[2 * y]), int(se[2 * y + 1])
                assert [int(v) for v in ps[y, s:e]] == [wps[(x, y)] for x in range(s, e)]
                assert np.array(pr[y, s:e]).tobytes() == np.array([wpr[(x, y)] for x in range(s, e)], np.float64).tobytes()
                if case["thr"] < 0 and len(sizes) == 1:  # every live window emits for every template: the row's hits are its live range x T
                    assert (e - s) * len(bank) == TC.row_targets(case).get((p, y), 0), (p, y, s, e)
        mm = np.zeros((len(bank), case["cap"]), O.MATCH_DTYPE)
        for t, m in enumerate(lists[p]):
            mm[t, : len(m)] = m
        hits = O.raw_hits(counts[p], mm, bank)
        for anchor, overlap in ((0.3, 5), (0.99, 0)):
            want = O.process_hits(hits, anchor, overlap)
            dicts = [dict(x=int(h["x"]), y=int(h["y"]), similarity=float(h["similarity"]), i=i) for i, h in enumerate(hits)]
            if not (hits["similarity"] >= np.float32(anchor)).any():  # no anchor: the Rust panics on the empty list (partition_by), the oracle returns no line
                with pytest.raises(IndexError):
                    W.process_hits(dicts, anchor, overlap)
                assert want == []
                continue
            got = W.process_hits(dicts, anchor, overlap)
            assert [[(h["x"], h["y"]) for h in ln] for ln in got] == [[(int(h["x"]), int(h["y"])) for h in ln] for ln in want]
            assert [[np.float32(h["similarity"]).tobytes() for h in ln] for ln in got] == [[h["similarity"].tobytes() for h in ln] for ln in want]

"""The tail of the MFMA scan at its capacity edges, on the device (cases and targets: tests/tail_cases.py; that every case reaches its targets
is shown on the CPU by tests/test_tail_cases_host.py).  Per case: three MFMA scans in one context without re-uploading — exact sizes,
estimated sizes, estimated sizes after any re-segmentation — then the legacy tail and the direct scan; every scan's lists equal the
oracle's bit for bit (x, y, f32 bits, order, cap) and every scan took the path the table names (focr_debug_tail_path)."""
import ctypes as C

import numpy as np
import pytest

import tail_cases as TC
from font_ocr_amd.searcher import SCAN_DIRECT, SCAN_MFMA, FocrError, Scanner
from oracle import oracle as O
from test_gpu_parity import _assert_same, _csr_to_lists

pytestmark = pytest.mark.gpu

_FLAT = {}


def _want(case_id, cap):
    """The oracle's lists at `cap`, and their (offsets, flat bytes) form — computed once, shared, never changed."""
    key = (case_id, cap)
    if key not in _FLAT:
        counts, lists = TC.oracle_lists(case_id, cap)
        parts = [m for pl in lists for m in pl if len(m)]
        flat = np.concatenate(parts) if parts else np.zeros(0, O.MATCH_DTYPE)
        _FLAT[key] = (counts, lists, np.concatenate([[0], np.cumsum(counts.reshape(-1).astype(np.uint64))]).astype(np.uint64), flat.tobytes())
    return _FLAT[key]


def _same_as_oracle(sc, case_id, cap, what):
    counts, lists, offsets_w, flat_w = _want(case_id, cap)
    offsets, m = sc.matches()
    if not (np.array_equal(offsets, offsets_w) and m.tobytes() == flat_w):  # (the whole batch at once; on a difference, the call that differs)
        _assert_same(_csr_to_lists(offsets, m, counts.shape[0], counts.shape[1]), lists, f"{case_id} {what}")
        raise AssertionError(f"{case_id} {what}: offsets differ")
    assert np.array_equal(sc.counts(), counts), f"{case_id} {what}: counts"
    return offsets, m


def _path(sc):
    tp = sc.tail_path()
    name = {"rows": "rows", "legacy": "legacy", "none": "none"}[tp["tail"]] + ("+big" if tp["big_launch"] else "") + ("+lib" if tp["library_sort"] else "")
    return name, (tp["seg_shift"], tp["n_seg"]), tp


def _check_mfma_scan(sc, case_id, case, cap, i, what):
    """Scan i (0: exact sizes, 1, 2: estimated) of a setup just ran: lists, path, segmentation, verify and ordering form, the largest bucket."""
    T = sum(c[2] for c in case["classes"])
    _same_as_oracle(sc, case_id, cap, what)
    name, seg, tp = _path(sc)
    assert (name, seg) == (case["path"][i], case["seg"][i]), (case_id, what, tp)
    assert tp["order"] == ("counting" if T <= 4096 else "sorting"), (case_id, what, tp)
    rows = name != "legacy"
    assert tp["verify"] == (case["verify"] if rows else "none") and tp["verify_chunks"] == (case["chunks"] if rows else 0), (case_id, what, tp)
    st = sc.size_estimate_stats()
    assert st["redone"] == 0, (case_id, what, st)  # no estimate of a case is too small: nothing is redone behind the test's back
    assert st["row_max"] == (max(case["row_max"][i], 1) if name in ("rows", "rows+big") else 0), (case_id, what, st)  # the device's prefix and maximum
    if rows:
        n = C.c_size_t(0)  # the row tail leaves the candidate list in place (their number only: a case may hold millions)
        sc._ck(sc._lib.focr_debug_candidates(sc._h, None, 0, C.byref(n)))
        assert n.value == sc.counters()["candidates"]
    else:
        with pytest.raises(FocrError):
            sc.candidates()


def _check_lines(sc, case_id, case, bank, offsets, m):
    n_pages, T, cap = case["geom"][0], len(bank), case["cap"]
    anchor = 0.3 if case["thr"] < 0 else 0.95
    sc.process_hits(anchor, 5)
    lines = sc.lines()
    got = _csr_to_lists(offsets, m, n_pages, T)
    some = 0
    for p in range(n_pages):
        counts = np.array([len(x) for x in got[p]], np.uint32)
        if not counts.any():
            assert lines[p] == []
            continue
        mm = np.zeros((T, cap), O.MATCH_DTYPE)
        for t, x in enumerate(got[p]):
            mm[t, : len(x)] = x
        want = O.process_hits(O.raw_hits(counts, mm, bank), anchor, 5)
        assert len(lines[p]) == len(want), (case_id, p)
        for lg, lw in zip(lines[p], want):
            for f in ("x", "y"):
                assert np.array_equal(lg[f].astype(np.int64), lw[f].astype(np.int64)), (case_id, p, f)
            assert np.array_equal(lg["letter"], lw["letter"]) and lg["similarity"].tobytes() == lw["similarity"].tobytes(), (case_id, p)
        some += len(want)
    assert some, f"{case_id}: no line to compare"


@pytest.mark.parametrize("case_id", sorted(TC.CASES))
def test_tail_case(case_id):
    case, bank, luma = TC.build(case_id)
    thr, cap = case["thr"], case["cap"]
    T = len(bank)
    order = "counting" if T <= 4096 else "sorting"
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(luma)
        for i in range(3):
            sc.scan(thr, cap, SCAN_MFMA)
            _check_mfma_scan(sc, case_id, case, cap, i, f"mfma scan {i}")
        if case["post"]:
            _check_lines(sc, case_id, case, bank, *sc.matches())
        sc.set_row_tail(0)
        sc.scan(thr, cap, SCAN_MFMA)
        _same_as_oracle(sc, case_id, cap, "legacy tail")
        name, seg, tp = _path(sc)
        assert (name, seg, tp["order"], tp["verify"]) == ("legacy", (0, 0), order, "none"), tp
        assert sc.size_estimate_stats()["row_max"] == 0
        with pytest.raises(FocrError):
            sc.candidates()
        sc.set_row_tail(1)
        sc.scan(thr, cap, SCAN_DIRECT)
        _same_as_oracle(sc, case_id, cap, "direct")
        name, seg, tp = _path(sc)
        assert (name, seg, tp["order"]) == ("none", (0, 0), order), tp
        for c2 in case["caps"]:  # a cap is part of the setup: exact sizes, then estimated
            for i in range(2):
                sc.scan(thr, c2, SCAN_MFMA)
                _check_mfma_scan(sc, case_id, case, c2, i, f"cap {c2} scan {i}")
        if case["grids"]:
            for num, den in ((1, 64), (3, 1)):
                sc.set_tail_grid(num, den)
                sc.set_row_tail(1)             # forgets the context's estimates ...
                sc.set_size_estimates(False)   # ... and this scan adopts none: exact sizes, the first scan's layout
                sc.scan(thr, cap, SCAN_MFMA)
                _check_mfma_scan(sc, case_id, case, cap, 0, f"grid {num}/{den} exact")
                sc.set_size_estimates(True)
                sc.scan(thr, cap, SCAN_MFMA)
                _check_mfma_scan(sc, case_id, case, cap, 1, f"grid {num}/{den} estimated")
            sc.set_tail_grid(0, 0)

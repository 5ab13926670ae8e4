"""The drop-in symbols ncc_8_u8 / ncc_16_u8 on the device at compat_call's branch points (tests/compat_cases.py; the cases' properties are
proved on the CPU by tests/test_compat_cases_host.py): lists equal to the oracle's byte for byte — x, y, the f32 similarity bits, order and
truncation at n_out."""
import threading

import numpy as np
import pytest

import compat_cases as CC
from font_ocr_amd.searcher import Searcher
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _device(c):
    s = Searcher(c["page"])
    s.acc_u32[:] = 0xDEADBEEF
    got = s.search_c_u8(c["needle"], c["stats"], c["thr"], c["n_out"])
    assert not s.acc_u32.any()  # src/ncc.cpp:67, 272: the call zeroes the caller's accumulator, whatever else it does
    return got


def _want(c):
    return CC.oracle(c, use_ref=O.have_ref())


def _same(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} matches, the oracle has {len(want)}"
    assert got.tobytes() == want.tobytes(), what


def _in_fresh_thread(calls):
    """The calls, in order, on a thread of its own: compat_call's state is thread_local, so the thread starts without hit arrays and its
    first call above the page-locked block has to grow them and scan again.  (Its context stays alive for the rest of the process: the
    file starts two such threads.)"""
    out = []

    def work():
        try:
            for c in calls:
                out.append(_device(c))
        except BaseException as e:  # noqa: BLE001 — handed to the test's thread
            out.append(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    for r in out:
        if isinstance(r, BaseException):
            raise r
    assert len(out) == len(calls)
    return out


@pytest.mark.parametrize("which", sorted(CC.BIG_NEEDLES))
def test_more_hits_than_the_pinned_block_take_the_device_path(which):
    """More than 65 536 hits: device sort, pack, then the first n_out in (y, x) order — the first hit, the first 1024, all of them.  The
    thread's first call (n_out = 1) finds 65 536 slots too few: grow and rescan; the later calls reuse the arrays.  The 8 x 8 thread goes
    on to the boundary: exactly 65 536 hits (the last call the page-locked block serves) and 65 537 (the first it cannot)."""
    calls = CC.big_calls(which)
    names = [f"{which} n_out={c['n_out']}" for c in calls]
    if which == "n8":
        for n, c in sorted(CC.boundary_calls().items()):
            calls.append(c)
            names.append(f"{n} windows")
    for got, c, name in zip(_in_fresh_thread(calls), calls, names):
        _same(got, _want(c), name)


@pytest.mark.parametrize("which", sorted(CC.TAB_NEEDLES))
def test_caller_tables_are_honoured_as_the_reference_reads_them(which):
    """Another [start, end) per row (interior starts, early ends, empty rows, every row-tail length) and patch_rnorm / patch_sum entries no
    page would give (+inf, NaN, 0.0, negative; foreign sums): both sides do the same IEEE operations on the caller's numbers."""
    for edited in (False, True):
        for c in CC.tables_calls(which, edited):
            _same(_device(c), _want(c), f"{which} edited={edited} thr={c['thr']}")


@pytest.mark.parametrize("case_id", CC.RES_CASES)
def test_second_call_of_a_geometry_scans_its_own_inputs(case_id):
    """Residency: inputs A, then inputs B of the same geometry — B's list is the oracle's for B, also where B differs from A by one byte, or
    only in the last n % 64 bytes of one input by bytes 8 apart (swapped, or XOR-ed with one mask), which the content hash once folded
    onto each other: the second call then scanned A's stale copy."""
    a, b, _ = CC.residency(case_id)
    _same(_device(a), _want(a), f"{case_id}: A")
    _same(_device(b), _want(b), f"{case_id}: B after A")
    _same(_device(a), _want(a), f"{case_id}: A after B")


@pytest.mark.parametrize("case_id", sorted(CC.DEG_CASES))
def test_degenerate_calls(case_id):
    c = CC.degenerate(case_id)
    got = _device(c)
    _same(got, _want(c), case_id)
    assert (len(got) == 0) == (case_id != "n_h == r_h - 1")

"""The model of the fixed line walk (tests/focr_walk_model.py) equals the reference's process_hits (oracle.process_hits) on
every hit list that tests/test_gpu_process_hits.py feeds the device, negative and huge overlaps included, and stays within
the kernel's bound on trips of its chunk loop.  The device runs those lists only once this passes.  No GPU."""
import numpy as np
import pytest

import focr_walk_model as M


@pytest.mark.parametrize("family", list(M.FAMILIES))
def test_walk_model_equals_reference(family):
    cases = M.FAMILIES[family]()
    assert cases
    for case in cases:
        got = M.model_lines(case)
        assert got == M.reference_lines(case), case
        if case.expect_lines is not None:
            assert sum(len(p) for p in got) == case.expect_lines, case


def test_fuzz_reaches_the_edges():
    """The seeded fuzz is not vacuous: it walks negative overlaps, capped hits, chunk-crossing rows and every anchor edge."""
    cases = M.fuzz()
    assert len(cases) == 300
    assert sum(c.overlap < 0 for c in cases) > 30
    assert sum(int((c.keep == 0).any()) for c in cases) > 100
    assert sum(int(np.isnan(c.anchor)) for c in cases) > 5
    assert sum(sum(len(l) for l in p) for c in cases for p in M.model_lines(c)) > 10_000


def test_walk_row_groups_and_trips():
    """Hand-checked walks: overlap -1 makes every kept hit a group (capped ones skipped); one group across three chunks keeps
    its LAST maximum; INT32_MIN and INT32_MAX stay within the trip bound."""
    x = np.array([5, 5, 6, 9, 9], np.int64)
    order = M.order_key(np.array([0.9, 0.95, 0.9, 0.99, 0.99], np.float32))
    kept = np.array([True, True, False, True, True])
    assert M.walk_row(x, order, kept, -1) == [0, 1, 3, 4]
    assert M.walk_row(x, order, kept, 1) == [1, 4]
    assert M.walk_row(x, order, kept, 0) == [1, 4]
    assert M.walk_row(x, order, kept, M.I32_MAX) == [4]
    n = 200
    order = M.order_key(np.full(n, 0.5, np.float32))
    assert M.walk_row(np.zeros(n, np.int64), order, np.ones(n, bool), M.I32_MAX) == [n - 1]
    assert M.walk_row(np.arange(n), order, np.ones(n, bool), M.I32_MIN) == list(range(n))
    # +0.0 beats -0.0 (f32::total_cmp) wherever it sits
    assert M.walk_row(np.zeros(3, np.int64), M.order_key(np.array([0.0, -0.0, -0.0], np.float32)), np.ones(3, bool), 0) == [0]

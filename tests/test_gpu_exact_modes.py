"""The exact scan on the device (scan_direct_kernel, scan_tall_kernel) in both arithmetics against the oracle, byte for byte, on the sets
of tests/exact_cases.py (whose properties tests/test_exact_cases_host.py proves on the CPU): FOCR_SCAN_DIRECT against the reference
kernel's lists with its cap of 1024, FOCR_SCAN_RUST (cap = UINT32_MAX: that path has none) against the scalar Rust scan restated per
template — templates 17 .. 32 px wide included, which the reference's dispatch leaves as todo!() and the device scans with the same
arithmetic.  Each scan must also have launched exactly the kernels its set is there for."""
import numpy as np
import pytest

import exact_cases as EC
from font_ocr_amd.searcher import SCAN_DIRECT, SCAN_RUST, Scanner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scanner():
    s = Scanner(0)
    yield s
    s.close()


@pytest.mark.parametrize("mode", [pytest.param(SCAN_DIRECT, id="direct"), pytest.param(SCAN_RUST, id="rust")])
@pytest.mark.parametrize("set_id", sorted(EC.SETS))
def test_exact_scan_equals_the_oracle(scanner, set_id, mode):
    bank, luma, _ = EC.build(set_id)
    T, n_pages = len(bank), len(luma)
    scanner.set_bank(bank)
    scanner.set_pages(luma)
    for thr in EC.THRESHOLDS:
        want = EC.oracle_c(set_id, thr) if mode == SCAN_DIRECT else EC.oracle_rust(set_id, thr)
        scanner.scan(thr, EC.CAP_C if mode == SCAN_DIRECT else 0xFFFFFFFF, mode)
        counts = scanner.counts()
        offsets, m = scanner.matches()
        assert np.array_equal(counts, np.array([[len(w) for w in pl] for pl in want], np.uint32)), (set_id, thr)
        assert np.array_equal(np.diff(offsets.astype(np.int64)), counts.reshape(-1))
        for p in range(n_pages):
            for t in range(T):
                got = m[int(offsets[p * T + t]): int(offsets[p * T + t + 1])]
                assert got.tobytes() == want[p][t].tobytes(), (set_id, thr, p, t)
        assert {li["name"] for li in scanner.launches()} == EC.launches(set_id), (set_id, thr)

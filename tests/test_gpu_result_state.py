"""Which results stand, and when: the getters of a Scanner after every call that withdraws a batch's results, from every state a scan
can leave the context in (common.h: the context's validity flags and their transitions).  Python API only.  Fixture of
test_gpu_lazy_matches.py: 2 pages of 96x64, 124 templates, threshold 0.8 (the oracle has hits, and a cap of 1 bites)."""
import ctypes as C
import re

import numpy as np
import pytest

from font_ocr_amd import _native as N
from font_ocr_amd import synth_page
from font_ocr_amd.bank import SYNTH_SEED_BASE
from font_ocr_amd.searcher import SCAN_DIRECT, SCAN_MFMA, FocrError, Scanner, prefilter_page_model
from oracle import oracle as O

pytestmark = pytest.mark.gpu

R_W, R_H, N_PAGES = 96, 64, 2
THR = 0.8
POST = (0.95, 5)        # process_hits' anchor threshold and overlap
POST_OTHER = (0.99, 12)  # ... and a pair that gives other lines (asserted on the oracle)


@pytest.fixture(scope="module")
def bank(bank_x2):
    return bank_x2.subset(list(range(33, 95)) + list(range(95 + 33, 95 + 95)))  # 124 templates


@pytest.fixture(scope="module")
def pages(bank_x2):
    return np.ascontiguousarray(np.stack([synth_page(bank_x2, SYNTH_SEED_BASE + 4100 + p, 256, 160)[32:32 + R_H, 40:40 + R_W] for p in range(N_PAGES)]))


def _flat_lines(lines):
    """lines (pages of lines of hit records) -> what identifies them: per page and line (x, y, letter, similarity bits)"""
    return [[(l["x"].astype(np.int64).tolist(), l["y"].astype(np.int64).tolist(), l["letter"].astype(np.int64).tolist(), l["similarity"].astype(np.float32).tobytes())
             for l in page] for page in lines]


@pytest.fixture(scope="module")
def want(bank, pages):
    """The reference, computed once and never changed: per cap (counts, offsets, flat list); per process_hits setting the lines."""
    out = {"post": {}}
    for cap in (1024, 1):
        counts, flat, hits = [], [], []
        for pg in pages:
            c, m = O.scan_page(O.invert(pg), bank, THR, cap, use_ref=O.have_ref())
            counts.append(np.asarray(c, np.uint32))
            flat.extend(m[t, : c[t]] for t in range(len(c)))
            hits.append(O.raw_hits(c, m, bank))
        counts = np.stack(counts)
        out[cap] = (counts, np.concatenate([[0], np.cumsum(counts.reshape(-1), dtype=np.uint64)]), np.concatenate(flat))
        if cap == 1024:
            for post in (POST, POST_OTHER):
                out["post"][post] = _flat_lines([O.process_hits(h, *post) for h in hits])
    assert out[1024][0].max() >= 2 and out[1][0].max() == 1 and out[1][0].sum() < out[1024][0].sum()  # hits, and a cap of 1 bites
    assert sum(len(p) for p in out["post"][POST]) > 0
    assert out["post"][POST] != out["post"][POST_OTHER], "the second process_hits setting must change the lines"
    return out


@pytest.fixture(scope="module")
def fresh(bank, pages, want):
    """Lines and runners of a context that has done nothing else, per process_hits setting (cap 1024)."""
    out = {}
    for post in (POST, POST_OTHER):
        with Scanner(0) as sc:
            sc.set_bank(bank)
            sc.set_pages(pages)
            sc.scan(THR, 1024, SCAN_MFMA)
            sc.process_hits(*post)
            out[post] = (sc.lines_flat().copy(), sc.runners().copy())
            assert _flat_lines(sc.lines()) == want["post"][post]
    return out


def _check_results(sc, want_cap, what):
    counts, offsets, flat = want_cap
    got_off, got_m = sc.matches()
    assert np.array_equal(sc.counts(), counts), f"{what}: counts"
    assert np.array_equal(got_off, offsets), f"{what}: offsets"
    assert got_m.tobytes() == flat.tobytes(), f"{what}: match list"
    assert sc.total_matches() == int(counts.sum()), f"{what}: total_matches"


def _refuses(call, text, what):
    with pytest.raises(FocrError, match=text):
        call()
        pytest.fail(f"{what}: no error")


def _no_post_results(sc, what):
    """every getter of process_hits' results gives its "no results" answer"""
    _refuses(sc.lines, "focr_get_lines: call focr_process_hits first", what)
    _refuses(sc.runners, "focr_get_runners: call focr_process_hits first", what)
    _refuses(sc.verify_images, "focr_verify_images: call focr_process_hits first", what)
    assert sc.total_chars() == 0 and sc.device_chars() == (0, 0), what


def _no_scan_results(sc, what):
    """... and every getter of the scan's"""
    for name in ("counts", "matches", "candidates", "tail_path"):
        _refuses(getattr(sc, name), "no scan results", f"{what}: {name}")
    assert sc.total_matches() == 0, what
    _no_post_results(sc, what)


# start states: (id, scan mode, forced split, size estimates, scans before process_hits).  Size estimates are kept per context AND shared
# between the contexts of a process that scan one setup (this module's fixtures and test_gpu_lazy_matches.py scan this very one), so
# only a context with estimates switched off is sure to scan with exact sizes: nothing is pending when its scan returns.
STARTS = [("exact", SCAN_MFMA, False, False, 1), ("estimated", SCAN_MFMA, False, True, 2), ("split", SCAN_MFMA, True, False, 1), ("direct", SCAN_DIRECT, False, False, 1)]
CALLS = ["set_bank", "alloc_same", "alloc_larger", "upload_pages", "upload_pages_device", "scan", "debug_process_hits"]


@pytest.mark.parametrize("start", STARTS, ids=[s[0] for s in STARTS])
def test_getters_after_every_invalidating_call(bank, pages, want, fresh, start):
    name, mode, split, estimates, n_scans = start
    cap = 1024
    hip = N.hip()  # the library's handle also resolves the HIP runtime it is linked to: a device copy of the pages for upload_pages_device
    d_pages = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_pages), C.c_size_t(pages.nbytes)) == 0
    try:
        assert hip.hipMemcpy(d_pages, C.c_void_p(pages.ctypes.data), C.c_size_t(pages.nbytes), 1) == 0  # hipMemcpyHostToDevice
        assert hip.hipDeviceSynchronize() == 0
        with Scanner(0) as sc:
            sc.force_split(split)
            sc.set_size_estimates(estimates)
            sc.set_bank(bank)
            for call in CALLS:
                what = f"{name}, {call}"
                sc.set_pages(pages)
                for _ in range(n_scans):  # (the second scan of a setup runs on estimated sizes; nothing has waited for it when process_hits is queued)
                    sc.scan(THR, cap, mode)
                sc.process_hits(*POST)
                if call == "set_bank":
                    sc.set_bank(bank)
                elif call == "alloc_same":
                    sc.alloc_pages(N_PAGES, R_W, R_H)
                elif call == "alloc_larger":
                    sc.alloc_pages(N_PAGES + 1, R_W, R_H)
                elif call == "upload_pages":
                    sc.upload_pages(pages[:1], 0)
                elif call == "upload_pages_device":
                    sc.upload_pages_device(d_pages.value, N_PAGES, 0)
                elif call == "scan":
                    sc.scan(THR, cap, mode)
                else:  # one hit, cut off by its call's cap
                    sc.debug_process_hits([0], [10], [10], [0], [0.99], [0])
                if call == "scan":  # the new scan's results stand, the previous batch's lines do not
                    _no_post_results(sc, what)
                    _check_results(sc, want[cap], what)
                    assert sc.tail_path()["tail"] == ("none" if mode == SCAN_DIRECT else "rows"), what
                elif call == "debug_process_hits":  # hits stand, but no lists, candidates or lines
                    for getter in ("counts", "matches", "candidates"):
                        _refuses(getattr(sc, getter), "the hits came from focr_debug_process_hits", f"{what}: {getter}")
                    assert sc.total_matches() == 0, what
                    sc.tail_path()  # (the last scan's: documented as readable whenever hits stand)
                    _no_post_results(sc, what)
                else:
                    _no_scan_results(sc, what)
                sc.sync()
                if call not in ("scan", "debug_process_hits"):
                    _no_scan_results(sc, what + ", after sync")
                # the context recovers: a whole batch again
                sc.set_pages(pages)
                sc.scan(THR, cap, mode)
                sc.process_hits(*POST)
                _check_results(sc, want[cap], what + ": next batch")
                assert sc.lines_flat().tobytes() == fresh[POST][0].tobytes(), what + ": next batch's lines"
                assert sc.runners().tobytes() == fresh[POST][1].tobytes(), what + ": next batch's runners"
                if not estimates:  # no scan of this context ran on estimates: none can have been redone
                    assert sc.size_estimate_stats()["redone"] == 0, what
    finally:
        hip.hipFree(d_pages)


def test_cap_of_one_after_results_were_withdrawn(bank, pages, want):
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.scan(THR, 1024, SCAN_MFMA)
        sc.process_hits(*POST)
        sc.alloc_pages(N_PAGES, R_W, R_H)
        _no_scan_results(sc, "alloc_pages")
        sc.set_pages(pages)
        sc.scan(THR, 1, SCAN_MFMA)
        _check_results(sc, want[1], "cap 1")


@pytest.mark.parametrize("mode", [pytest.param(SCAN_MFMA, id="mfma"), pytest.param(SCAN_DIRECT, id="direct")])
def test_second_process_hits_owns_lines_and_runners(bank, pages, want, fresh, mode):
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.scan(THR, 1024, mode)
        sc.process_hits(*POST)
        assert _flat_lines(sc.lines()) == want["post"][POST]
        assert sc.runners().tobytes() == fresh[POST][1].tobytes()  # (both are now cached: lines on the host, runners on the device)
        sc.process_hits(*POST_OTHER)
        assert _flat_lines(sc.lines()) == want["post"][POST_OTHER]
        assert sc.lines_flat().tobytes() == fresh[POST_OTHER][0].tobytes() != fresh[POST][0].tobytes()
        assert sc.runners().tobytes() == fresh[POST_OTHER][1].tobytes()
        assert sc.last_runners()["launches"] == 1  # computed for this process_hits, not copied from the previous one's
        assert len(sc.runners()) == sc.total_chars() == len(fresh[POST_OTHER][0])


def test_launch_records_carry_no_private_data(bank, pages):
    """n_templates of a launch record is a template count and nothing else; the issued MACs add up to the counter."""
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.scan(THR, 1024, SCAN_MFMA)
        launches = sc.launches()
        assert launches and all(l["name"].startswith("scan_mfma") for l in launches), launches
        assert all(0 < l["n_templates"] <= len(bank) for l in launches), launches
        per_name = {}
        for l in launches:
            per_name[l["name"]] = per_name.get(l["name"], 0) + l["n_templates"]
        assert sum(per_name.values()) == len(bank), per_name  # every template of the bank is scanned by exactly one launch
        # per kernel: the templates of the size classes that share its pass (same K-steps, same K layout: the name's first two arguments)
        want_per_pass = {}
        for k in prefilter_page_model(bank, None, THR)["classes"]:
            key = (int(k["ksteps"]), int(k["layout"]))
            want_per_pass[key] = want_per_pass.get(key, 0) + int(k["n_templates"])
        got_per_pass = {tuple(int(v) for v in re.search(r"<(\d+),(\d+),", name).groups()): n for name, n in per_name.items()}
        assert got_per_pass == want_per_pass, (per_name, want_per_pass)
        assert sc.counters()["issued_macs"] == sum(l["issued_macs"] for l in launches) > 0


def test_timings_and_stamps_are_consistent(bank, pages):
    with Scanner(0) as sc:
        sc.set_size_estimates(False)  # exact sizes, whatever this process has scanned before
        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.scan(THR, 1024, SCAN_MFMA)
        sc.process_hits(*POST)
        ms = list(sc.timings().values())
        stamps = list(sc.phase_stamps().values())
        assert sc.size_estimate_stats()["redone"] == 0
    print("timings", ms, "stamps", stamps)
    assert all(v >= 0 for v in ms[:5]), ms
    # ms[0..3] and ms[5] are differences of the same five event times, each delivered as a float32: the parts add up to the whole but
    # for the rounding of those five values, at most 1.5 float32 spacings at the whole's magnitude each (the tick difference converted
    # to float, then to milliseconds), 7.5 in all
    allowance = 8 * float(np.spacing(np.float32(ms[5])))
    parts = ms[0] + ms[1] + ms[2] + ms[3]
    print("total", ms[5], "parts", parts, "allowance", allowance)
    assert ms[5] >= parts - allowance, (ms, allowance)
    have = [v for v in stamps[:7] if v >= 0]
    assert len(have) >= 2 and all(a <= b for a, b in zip(have, have[1:])), stamps

"""The executor's host results against the oracle, byte for byte: what `complete()` (pipe.hip) leaves in a context's page-locked
buffers with fetch on — the last step before the `ncc` binary's output — and the page layer under it (pages.hip).  Batches and
their expected records: tests/executor_cases.py (oracle only; proved on the CPU by tests/test_executor_cases_host.py).  Everything
compares with ==.

  A  every batch kind through Pipeline.host_results, MFMA and direct scans, without process_hits, a resident rescan, device-pointer
     pages; the record equals the oracle and what wait()'s Scanner view reports
  B  buffer life: on one slot the result buffers grow (new addresses) and are then kept (same addresses, nothing of the larger
     batch visible); four slots hold four records at once at sixteen different addresses
  C  size estimates and the redo under fetch, with chars_out
  D  order and states: tickets read out of order, twice, after wait, released unread; the refusals
  E  the fleet: eleven mixed batches over one and two executors, with and without the end-of-stream hints
  F  releases out of order (tools/host_results_check.py, a child process: focr_fleet_submit must refuse, not wait)
  G  pages in memory locked with RegisteredPages, announced and not
  H  page sources on a plain Scanner: pieces out of order, mixed inversion, device pointers at byte offsets 0 / 1 / 2, a smaller
     batch in a kept buffer — for a page width that is a multiple of four and one that is not
  I  Scanner.lines_into

The scenarios that could block (a failed batch, F, two consumer threads) run in tools/host_results_check.py under a time limit.
The batch that fails before its scan is a rescan in a context without pages, as tools/gate_check.py provokes it (a page narrower
than the bank's widest template would not do: it is no error in this library, it gives zero matches).

Teeth, as measured on an MI355X with one-line mutations of the library that change values only (no size, address or launch
bound), each built apart and run once.  Which test of this module failed first, what else of it failed, and which of the older GPU
tests run against the same build noticed (the CLI, process_hits, result-state and lazy-match modules and the parity module without
its soak, fuzz and full-size cases: 163 tests):
  1  ingest_pages ignoring `first`: H, test_upload_in_pieces_out_of_order[dword-width] first, then all ten piecewise uploads (out of
     order, mixed inversion, device pointers); nothing else here, and none of the older tests
  2  complete() taking R.n_chars from focr_total_lines (set after the buffers are sized): A, test_host_results_equal_the_oracle
     [text-mfma] first, then every test that reads a record with lines (34 of 58); of the older tests only
     test_cli_verify_and_scores_while_the_ring_wraps
  3  complete() not clearing chars_queued after a redo: C, test_estimated_and_redone_batches_under_fetch ("#2 dense: chars_out"),
     and nothing else; of the older tests test_pipeline_chars_out_with_estimated_and_redone_batches
  4  focr_get_lines_into copying n_pages instead of n_pages + 1 page offsets: A, test_host_results_equal_the_oracle[text-mfma] first
     (every kind with a line; `blank` and `no-lines` take the branch that fills the offsets on the host), H's smaller batch and I
     (text, one-blank-page, debug hits: Scanner.lines_into hands the call buffers filled with a pattern); of the older tests five
     of test_gpu_cli.py and test_cli_forwards_overlap_and_anchor
  5  focr_fleet_host_results passing the fleet ticket as the executor's: the child process first (release-order-2: "ticket 4, out
     of order"), then E on two executors (fleet ticket 2 delivers ticket 3's record); one executor passes, as it must; none of the
     older tests
The same runs showed this module's own flaw: the address of a grown buffer was compared with its predecessor's while PinBuf::ensure
freed before it allocated, and twice in five runs the allocator handed the line offsets' old address back.  ensure allocates first
now (pipe.hip), which makes the comparison sound.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import executor_cases as EC
from font_ocr_amd import _native as N
from font_ocr_amd.bank import HIT_DTYPE
from font_ocr_amd.searcher import SCAN_DIRECT, SCAN_MFMA, Fleet, FocrError, HostResults, PinnedPages, Pipeline, RegisteredPages, Scanner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("text", "blank", "no-lines", "one-blank-page", "small", "big", "sparse", "dense", "cap1", "odd-width", "dword-width")


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\ntest_gpu_host_results: {time.time() - t0:.1f} s of wall time")


@pytest.fixture(scope="module")
def built():
    """(bank, cases, expected): the oracle's records, computed once and never changed."""
    return EC.all_expected()


@pytest.fixture(scope="module")
def pipe3(built):
    """The default executor (three lanes of two contexts) with fetch on, shared by the tests that release whatever they submit."""
    pipe = Pipeline(0, 3)
    pipe.set_bank(built[0])
    pipe.set_fetch(True)
    yield pipe
    pipe.close()


def _pipe(bank, *shape, fetch=True):
    pipe = Pipeline(0, *shape)
    pipe.set_bank(bank)
    if fetch:
        pipe.set_fetch(True)
    return pipe


def _args(case, mode=SCAN_MFMA, post=True):
    return (case["thr"], case["cap"], mode, post, case["anchor"], case["overlap"])


def _assert_record(rec, e, what):
    """A host record equals the oracle's, field by field and byte by byte."""
    assert isinstance(rec, HostResults)
    got = (rec.n_pages, rec.n_templates, rec.n_matches, rec.n_lines, rec.n_chars)
    assert got == (e.n_pages, e.n_templates, e.n_matches, e.n_lines, e.n_chars), (what, got)
    assert rec.counts.shape == e.counts.shape and rec.counts.dtype == np.uint32 and rec.counts.tobytes() == e.counts.tobytes(), f"{what}: counts"
    assert rec.addresses["counts"] != 0
    assert np.isfinite(rec.device_ms) and rec.device_ms >= 0.0, (what, rec.device_ms)
    if not e.post:
        assert rec.page_line_off is None and rec.line_char_off is None and rec.chars is None, what
        assert [rec.addresses[k] for k in ("page_line_off", "line_char_off", "chars")] == [0, 0, 0], what
        assert rec.lines_flat_bytes() == b""
        return
    assert rec.page_line_off.shape == (e.n_pages + 1,) and rec.line_char_off.shape == (e.n_lines + 1,) and rec.chars.shape == (e.n_chars,), what
    assert int(rec.line_char_off[rec.n_lines]) == rec.n_chars and int(rec.page_line_off[rec.n_pages]) == rec.n_lines, what
    assert rec.page_line_off.tobytes() == e.page_line_off.tobytes(), f"{what}: page_line_off"
    assert rec.line_char_off.tobytes() == e.line_char_off.tobytes(), f"{what}: line_char_off"
    assert rec.chars.dtype == HIT_DTYPE and rec.lines_flat_bytes() == e.chars.tobytes(), f"{what}: chars"


def _assert_scanner(sc, rec, e, what):
    """... and what wait()'s Scanner view reports for the same ticket."""
    assert sc.total_matches() == rec.n_matches == e.n_matches, what
    assert sc.counts().tobytes() == rec.counts.tobytes(), f"{what}: Scanner.counts"
    if e.post:
        assert sc.lines_flat().tobytes() == rec.lines_flat_bytes(), f"{what}: Scanner.lines_flat"
        assert sc.total_chars() == rec.n_chars


def _roundtrip(pipe, case, e, what, mode=SCAN_MFMA, post=True, pages="host", **submit_kw):
    """One batch through the executor: submit, host results, the Scanner view, release."""
    if pages == "host":
        t = pipe.submit(case["pages"], *_args(case, mode, post), **submit_kw)
    else:  # resident
        t = pipe.submit(None, *_args(case, mode, post), **submit_kw)
    try:
        rec = pipe.host_results(t)
        _assert_record(rec, e, what)
        _assert_scanner(pipe.wait(t), rec, e, what)
        return rec.copy()
    finally:
        pipe.release(t)


# ---- A. host results equal the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [SCAN_MFMA, SCAN_DIRECT], ids=["mfma", "direct"])
@pytest.mark.parametrize("kind", KINDS)
def test_host_results_equal_the_oracle(pipe3, built, kind, mode):
    _, cases, exp = built
    rec = _roundtrip(pipe3, cases[kind], exp[kind], f"{kind} mode {mode}", mode)
    assert rec.lines_flat_bytes() == exp[kind].chars.tobytes()  # the detached copy outlives the release


@pytest.mark.parametrize("kind", ["text", "blank", "dense"])
def test_host_results_without_process_hits(pipe3, built, kind):
    bank, cases, _ = built
    e = EC.expected(cases[kind], bank, post=False)
    _roundtrip(pipe3, cases[kind], e, f"{kind} without process_hits", post=False)


def test_host_results_of_a_resident_rescan(built):
    """submit() without pages after a batch with pages rescans what the context holds — with the new ticket's own threshold, cap and
    anchor: the same pages give the records of `text`, `cap1` and `no-lines`."""
    bank, cases, exp = built
    pipe = _pipe(bank, 1, 1)
    try:
        _roundtrip(pipe, cases["text"], exp["text"], "with pages")
        _roundtrip(pipe, cases["text"], exp["text"], "resident", pages="resident")
        _roundtrip(pipe, cases["cap1"], exp["cap1"], "resident, cap 1", pages="resident")
        _roundtrip(pipe, cases["no-lines"], exp["no-lines"], "resident, no anchor", pages="resident")
        _roundtrip(pipe, cases["text"], EC.expected(cases["text"], bank, post=False), "resident, no process_hits", pages="resident", post=False)
    finally:
        pipe.close()


@pytest.mark.parametrize("kind,offset", [("text", 0), ("dword-width", 1), ("odd-width", 0), ("odd-width", 3)])
def test_host_results_from_device_pointer_pages(pipe3, built, kind, offset):
    """Pages the executor ingests straight from a device pointer (page-locked host memory is device-accessible: a device buffer as
    far as the library is concerned) — also from a pointer that is not dword-aligned."""
    _, cases, exp = built
    case = cases[kind]
    pin = PinnedPages(1, 1, case["pages"].size + 8)
    try:
        flat = pin.array.reshape(-1)
        flat[:] = 0x5A
        flat[offset: offset + case["pages"].size] = case["pages"].reshape(-1)
        t = pipe3.submit(None, *_args(case), device_ptr=flat.ctypes.data + offset, shape=case["pages"].shape)
        try:
            rec = pipe3.host_results(t)
            _assert_record(rec, exp[kind], f"{kind} from a device pointer + {offset}")
            _assert_scanner(pipe3.wait(t), rec, exp[kind], kind)
        finally:
            pipe3.release(t)
    finally:
        pin.close()


# ---- B. buffer life ----------------------------------------------------------------------------------------------------------------------

def test_result_buffers_grow_and_are_kept(built):
    bank, cases, exp = built
    pipe = _pipe(bank, 1, 1)
    try:
        recs = [_roundtrip(pipe, cases[k], exp[k], f"#{i} {k}") for i, k in enumerate(("small", "big", "small", "blank", "text"))]
        small, big, small2 = recs[:3]
        for field in ("chars", "line_char_off"):
            assert big.addresses[field] != small.addresses[field], f"{field}: the buffer should have grown for `big`"
            assert small2.addresses[field] == big.addresses[field], f"{field}: the grown buffer should have been kept"
        assert small2.lines_flat_bytes() == small.lines_flat_bytes() and small2.line_char_off.tobytes() == small.line_char_off.tobytes()
        for r in recs[3:]:  # smaller requests never move a buffer
            assert r.addresses["chars"] == big.addresses["chars"] and r.addresses["line_char_off"] == big.addresses["line_char_off"]
    finally:
        pipe.close()


def test_four_slots_hold_four_records_at_once(built):
    bank, cases, exp = built
    kinds = ("text", "one-blank-page", "big", "odd-width")
    pipe = _pipe(bank, 2, 2)
    try:
        assert len(pipe.scanners) == 4
        tickets = [pipe.submit(cases[k]["pages"], *_args(cases[k])) for k in kinds]
        recs = [pipe.host_results(t) for t in tickets]  # views; nothing is read before the last batch has completed
        for k, rec in zip(kinds, recs):
            _assert_record(rec, exp[k], f"{k}, all four outstanding")
        addresses = [a for rec in recs for a in rec.addresses.values()]
        assert 0 not in addresses and len(set(addresses)) == 16, addresses
        for t in tickets:
            pipe.release(t)
    finally:
        pipe.close()


# ---- C. estimates and redo under fetch ---------------------------------------------------------------------------------------------------

def test_estimated_and_redone_batches_under_fetch(built):
    """One slot: every batch meets its predecessor's estimates.  The first `dense` overflows them (tests/executor_cases.py proves it
    must) and is redone; its characters reach chars_out after the redo, not from the first attempt."""
    bank, cases, exp = built
    pipe = _pipe(bank, 1, 1)
    pin = PinnedPages(1, 1, 1 << 16)
    try:
        buf = pin.array.reshape(-1)
        assert (exp["dense"].n_chars + 1) * HIT_DTYPE.itemsize < buf.size
        redone = [pipe.scanners[0].size_estimate_stats()["redone"]]
        for i, k in enumerate(("sparse", "sparse", "dense", "dense", "sparse")):
            buf[:] = 0xEE
            t = pipe.submit(cases[k]["pages"], *_args(cases[k]), chars_out=(buf.ctypes.data, buf.size))
            try:
                rec = pipe.host_results(t)
                _assert_record(rec, exp[k], f"#{i} {k}")
                n = rec.n_chars * HIT_DTYPE.itemsize
                assert buf[:n].tobytes() == rec.lines_flat_bytes(), f"#{i} {k}: chars_out"
                _assert_scanner(pipe.wait(t), rec, exp[k], f"#{i} {k}")
                redone.append(pipe.scanners[0].size_estimate_stats()["redone"])
            finally:
                pipe.release(t)
        assert redone[1] == redone[2] == redone[0], redone      # the sparse batches fit their bounds
        assert redone[3] == redone[0] + 1, redone               # the first dense one does not
        assert redone[4] == redone[5] == redone[3], redone      # its successor has dense bounds; sparse fits them
    finally:
        pipe.close()
        pin.close()


# ---- D. order and states -----------------------------------------------------------------------------------------------------------------

def test_tickets_read_out_of_order_twice_and_after_wait(pipe3, built):
    _, cases, exp = built
    ta = pipe3.submit(cases["big"]["pages"], *_args(cases["big"]))
    tb = pipe3.submit(cases["text"]["pages"], *_args(cases["text"]))
    tc = pipe3.submit(cases["cap1"]["pages"], *_args(cases["cap1"]))
    try:
        rb = pipe3.host_results(tb)  # ticket k + 1 before ticket k
        _assert_record(rb, exp["text"], "ticket k + 1 first")
        ra = pipe3.host_results(ta)
        _assert_record(ra, exp["big"], "ticket k second")
        rb2 = pipe3.host_results(tb)  # twice: the same record
        assert rb2.addresses == rb.addresses
        _assert_record(rb2, exp["text"], "asked twice")
        _assert_record(rb, exp["text"], "the first view after the second call")
        sc = pipe3.wait(tc)  # wait first, then host_results
        rc = pipe3.host_results(tc)
        _assert_record(rc, exp["cap1"], "after wait")
        _assert_scanner(sc, rc, exp["cap1"], "after wait")
    finally:
        for t in (ta, tb, tc):
            pipe3.release(t)
    for t in (ta, tb, tc):
        with pytest.raises(FocrError, match="not outstanding"):
            pipe3.host_results(t)


def test_release_without_reading(built):
    bank, cases, exp = built
    pipe = _pipe(bank, 1, 1)
    try:
        t = pipe.submit(cases["big"]["pages"], *_args(cases["big"]))
        pipe.release(t)  # completes the batch unseen
        with pytest.raises(FocrError, match="not outstanding"):
            pipe.host_results(t)
        _roundtrip(pipe, cases["text"], exp["text"], "the slot's next batch")
    finally:
        pipe.close()


def test_fetch_off_and_fetch_switched_on_late(built):
    """Fetch is read when a batch is completed: off, host_results refuses; switched on after a batch has completed, that batch still
    refuses and the next one delivers."""
    bank, cases, exp = built
    pipe = _pipe(bank, 3, fetch=False)
    try:
        t1 = pipe.submit(cases["text"]["pages"], *_args(cases["text"]))
        with pytest.raises(FocrError, match="call focr_pipe_set_fetch first"):
            pipe.host_results(t1)
        sc = pipe.wait(t1)  # the batch itself is fine
        assert sc.counts().tobytes() == exp["text"].counts.tobytes() and sc.lines_flat().tobytes() == exp["text"].chars.tobytes()
        t2 = pipe.submit(cases["cap1"]["pages"], *_args(cases["cap1"]))
        pipe.wait(t2)  # completed with fetch off ...
        pipe.set_fetch(True)
        with pytest.raises(FocrError, match="call focr_pipe_set_fetch first"):
            pipe.host_results(t2)  # ... so it stays without a record
        pipe.release(t1)
        pipe.release(t2)
        _roundtrip(pipe, cases["one-blank-page"], exp["one-blank-page"], "the first batch completed with fetch on")
        pipe.set_fetch(False)
        t4 = pipe.submit(cases["text"]["pages"], *_args(cases["text"]))
        with pytest.raises(FocrError, match="call focr_pipe_set_fetch first"):
            pipe.host_results(t4)
        pipe.release(t4)
    finally:
        pipe.close()


def test_scenarios_that_could_block_run_in_a_child_process():
    """tools/host_results_check.py: a failed batch between good ones, releases out of order on one and two executors (section F: the
    refusal that fleet.hip's count of releases missed), two consumer threads.  A deadlock fails at the time limit."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_results_check.py")], capture_output=True, text=True, timeout=90)
    lines = r.stdout.splitlines()
    for name in ("error-batch", "release-order-1", "release-order-2", "two-consumers"):
        assert f"ok {name}" in lines, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])


# ---- E. the fleet ------------------------------------------------------------------------------------------------------------------------

def _fleet_stream(fl, cases, exp, kinds, hints):
    """Submit `kinds` in order, retire in submission order through Fleet.host_results -> detached records."""
    inflight, got = [], []

    def retire():
        t, k = inflight.pop(0)
        rec = fl.host_results(t)
        _assert_record(rec, exp[k], f"fleet ticket {t} ({k}), {fl.n_devices} executors, hints {hints}")
        got.append(rec.copy())
        fl.release(t)

    try:
        for i, k in enumerate(kinds):
            if len(inflight) == fl.slots:
                retire()
            if hints and i == len(kinds) - min(fl.n_devices, len(kinds)):
                fl.announce_last()  # before the last n_devices submits
            inflight.append((fl.submit(cases[k]["pages"], *_args(cases[k])), k))
        if hints:
            fl.end_of_stream()
    finally:
        while inflight:
            retire()
    return got


@pytest.mark.parametrize("devices", [[0], [0, 0]], ids=["one", "two"])
def test_fleet_host_results_with_and_without_stream_hints(built, devices):
    bank, cases, exp = built
    fl = Fleet(devices, lanes=2)
    try:
        fl.set_bank(bank)
        fl.set_fetch(True)
        lib = N.hip()
        for i in range(fl.n_devices):  # Fleet.pipe: the executors are the fleet's own
            assert lib.focr_pipe_contexts(fl.pipe(i)) * fl.n_devices == fl.slots and lib.focr_pipe_lanes(fl.pipe(i)) == 2
        assert fl.n_devices == 1 or fl.pipe(0) != fl.pipe(1)
        with pytest.raises(IndexError):
            fl.pipe(fl.n_devices)
        assert len(KINDS) == 11
        plain = _fleet_stream(fl, cases, exp, KINDS, hints=False)
        hinted = _fleet_stream(fl, cases, exp, KINDS, hints=True)
        for a, b in zip(plain, hinted):
            assert a.counts.tobytes() == b.counts.tobytes() and a.page_line_off.tobytes() == b.page_line_off.tobytes()
            assert a.line_char_off.tobytes() == b.line_char_off.tobytes() and a.lines_flat_bytes() == b.lines_flat_bytes()
        # a stream of one batch: on two executors the second keeps its "last" mark until the next stream's second batch takes it
        _fleet_stream(fl, cases, exp, ("dense",), hints=True)
        again = _fleet_stream(fl, cases, exp, KINDS, hints=False)
        for a, b in zip(plain, again):
            assert a.counts.tobytes() == b.counts.tobytes() and a.lines_flat_bytes() == b.lines_flat_bytes()
    finally:
        fl.close()


# ---- G. registered memory ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("announce", [True, False], ids=["prefetch", "submit-only"])
def test_pages_in_registered_memory(pipe3, built, announce):
    _, cases, exp = built
    arr = cases["one-blank-page"]["pages"].copy()  # a plain numpy array, page-locked where it lies
    with RegisteredPages(arr) as reg:
        assert reg.array is arr
        if announce:
            pipe3.prefetch(arr)
        t = pipe3.submit(arr, *_args(cases["one-blank-page"]))
        try:
            rec = pipe3.host_results(t)
            _assert_record(rec, exp["one-blank-page"], "registered pages")
            _assert_scanner(pipe3.wait(t), rec, exp["one-blank-page"], "registered pages")
        finally:
            pipe3.release(t)
    # unregistered only now, after the batch's wait; the array is ordinary memory again and still intact
    assert arr.tobytes() == cases["one-blank-page"]["pages"].tobytes()
    with pytest.raises(ValueError):
        RegisteredPages(arr[:, :, ::2])


# ---- H. page sources on a plain Scanner ---------------------------------------------------------------------------------------------------

def _csr(e):
    return np.concatenate([[0], np.cumsum(e.counts.reshape(-1), dtype=np.uint64)]).astype(np.uint64)


def _scan_all(sc, case):
    sc.scan(case["thr"], case["cap"], SCAN_MFMA)
    planes = sc.planes().tobytes()
    offsets, m = sc.matches()
    sc.process_hits(case["anchor"], case["overlap"])
    return planes, sc.counts().tobytes(), offsets.tobytes(), m.tobytes(), sc.lines_flat().tobytes()


@pytest.fixture(scope="module")
def source_scanner(built):
    sc = Scanner(0)
    sc.set_bank(built[0])
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def whole_batch(built, source_scanner):
    """kind -> what set_pages of the whole batch gives (planes, counts, offsets, matches, lines), the matches held to the oracle."""
    bank, cases, exp = built
    out = {}
    for kind in ("dword-width", "odd-width"):
        source_scanner.set_pages(cases[kind]["pages"])
        out[kind] = _scan_all(source_scanner, cases[kind])
        e = exp[kind]
        assert out[kind][1:] == (e.counts.tobytes(), _csr(e).tobytes(), e.matches_flat(bank).tobytes(), e.chars.tobytes()), kind
    return out


def _fresh_slots(sc, pages):
    """Four allocated slots that hold other pages than the scenario will upload: a piece that lands in the wrong slot, or nowhere,
    cannot go unnoticed behind what an earlier scenario left there."""
    sc.set_pages(np.ascontiguousarray(pages[::-1]))
    sc.sync()
    sc.alloc_pages(*pages.shape[:1], pages.shape[2], pages.shape[1])


@pytest.mark.parametrize("kind", ["dword-width", "odd-width"])
def test_upload_in_pieces_out_of_order(built, source_scanner, whole_batch, kind):
    pages = built[1][kind]["pages"]
    _fresh_slots(source_scanner, pages)
    source_scanner.upload_pages(pages[2:4], first=2)
    source_scanner.upload_pages(pages[0:2], first=0)
    assert _scan_all(source_scanner, built[1][kind]) == whole_batch[kind]


@pytest.mark.parametrize("kind", ["dword-width", "odd-width"])
def test_upload_in_pieces_with_different_inversion(built, source_scanner, whole_batch, kind):
    pages = built[1][kind]["pages"]
    _fresh_slots(source_scanner, pages)
    source_scanner.upload_pages(255 - pages[0:1], first=0, invert=False)  # ink-high bytes as they are
    source_scanner.upload_pages(pages[1:3], first=1, invert=True)
    source_scanner.upload_pages(255 - pages[3:4], first=3, invert=False)
    assert _scan_all(source_scanner, built[1][kind]) == whole_batch[kind]


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("kind", ["dword-width", "odd-width"])
def test_upload_from_a_device_pointer_at_byte_offsets(built, source_scanner, whole_batch, kind, offset):
    """r_w % 4 == 0 with a pointer that is not dword-aligned must take ingest_pages' byte path; in two pieces, the second first."""
    pages = built[1][kind]["pages"]
    page_bytes = pages[0].size
    pin = PinnedPages(1, 1, pages.size + 8)
    try:
        flat = pin.array.reshape(-1)
        flat[:] = 0x5A
        flat[offset: offset + pages.size] = pages.reshape(-1)
        _fresh_slots(source_scanner, pages)
        source_scanner.upload_pages_device(flat.ctypes.data + offset + 2 * page_bytes, 2, first=2)
        source_scanner.upload_pages_device(flat.ctypes.data + offset, 2, first=0)
        assert _scan_all(source_scanner, built[1][kind]) == whole_batch[kind]  # (matches() has waited for the ingest: the buffer may go)
    finally:
        pin.close()


@pytest.mark.parametrize("kind", ["dword-width", "odd-width"])
def test_smaller_batch_in_a_kept_page_buffer(built, source_scanner, whole_batch, kind):
    """Two pages after four of the same geometry: the buffer is kept, and nothing of the larger batch's other pages shows."""
    bank, cases, exp = built
    pages, e = cases[kind]["pages"], exp[kind]
    source_scanner.set_pages(pages)
    assert _scan_all(source_scanner, cases[kind]) == whole_batch[kind]
    source_scanner.set_pages(pages[2:4])
    _, counts, offsets, m, lines = _scan_all(source_scanner, cases[kind])
    assert source_scanner.counts().shape == (2, len(bank))
    want_m = np.concatenate([np.zeros(0, EC.O.MATCH_DTYPE)] + [e.matches_flat(bank)[int(e.counts[:p].sum()): int(e.counts[:p + 1].sum())] for p in (2, 3)])
    first_char = int(e.line_char_off[int(e.page_line_off[2])])
    assert counts == e.counts[2:4].tobytes() and m == want_m.tobytes() and lines == e.chars[first_char:].tobytes()
    assert offsets == np.concatenate([[0], np.cumsum(e.counts[2:4].reshape(-1), dtype=np.uint64)]).astype(np.uint64).tobytes()
    p_off, l_off, chars = source_scanner.lines_into()
    assert len(p_off) == 3 and int(p_off[2]) == len(l_off) - 1 == e.n_lines - int(e.page_line_off[2]) and chars.tobytes() == lines


# ---- I. lines_into -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["text", "blank", "no-lines", "one-blank-page"])
def test_lines_into_equals_lines_flat_and_the_oracle(built, source_scanner, kind):
    _, cases, exp = built
    case, e = cases[kind], exp[kind]
    source_scanner.set_pages(case["pages"])
    source_scanner.scan(case["thr"], case["cap"], SCAN_MFMA)
    with pytest.raises(FocrError, match="call focr_process_hits first"):
        source_scanner.lines_into()  # before any process_hits of this scan
    source_scanner.process_hits(case["anchor"], case["overlap"])
    p_off, l_off, chars = source_scanner.lines_into()
    assert chars.tobytes() == source_scanner.lines_flat().tobytes() == e.chars.tobytes()
    assert p_off.tobytes() == e.page_line_off.tobytes() and l_off.tobytes() == e.line_char_off.tobytes()
    assert int(l_off[-1]) == len(chars) and int(p_off[-1]) == len(l_off) - 1


def test_lines_into_after_debug_process_hits(built, source_scanner):
    bank, cases, _ = built
    source_scanner.set_pages(cases["text"]["pages"])
    page, y, x, t = [0, 0, 0, 1], [10, 10, 10, 20], [5, 7, 30, 50], [1, 2, 3, 0]
    sims = np.array([0.96, 0.97, 0.9, 0.99], np.float32)
    source_scanner.debug_process_hits(page, y, x, t, sims, [1, 1, 1, 1])
    source_scanner.process_hits(0.95, 5)
    p_off, l_off, chars = source_scanner.lines_into()
    assert chars.tobytes() == source_scanner.lines_flat().tobytes()
    assert p_off.tolist() == [0, 1, 2] and l_off.tolist() == [0, 2, 3]
    assert chars["x"].tolist() == [7, 30, 50] and chars["template_index"].tolist() == [2, 3, 0] and chars["similarity"].tobytes() == sims[[1, 2, 3]].tobytes()
    assert np.array_equal(chars["letter"], bank.templates["letter"][[2, 3, 0]])

"""The per-call match lists are written on demand (order.hip, materialise_matches): whatever a caller does between a scan and its first
matches() — nothing, process_hits, lines(), a second matches(), an executor batch submitted with process_hits — the lists and counts
must be the oracle's, bit for bit, and equal to those of a context that never called process_hits."""
import numpy as np
import pytest

from font_ocr_amd import synth_page
from font_ocr_amd.bank import MATCH_DTYPE, SYNTH_SEED_BASE
from font_ocr_amd.searcher import SCAN_DIRECT, SCAN_MFMA, Pipeline, Scanner
from oracle import oracle as O

pytestmark = pytest.mark.gpu

R_W, R_H, N_PAGES = 96, 64, 2
THR = 0.8
CAPS = (1024, 1)


@pytest.fixture(scope="module")
def bank(bank_x2):
    sub = bank_x2.subset(list(range(33, 95)) + list(range(95 + 33, 95 + 95)))  # 124 templates
    widths = {int(t["n_w"]) for t in sub.templates}
    assert {8, 9} <= widths, widths  # both an 8- and a 9-wide class (the 9-wide one scans with its last column bounded)
    return sub


@pytest.fixture(scope="module")
def pages(bank_x2):
    # (the synthetic pages keep 45 px of margin: a 96x64 page is cut out of the text area of a larger one)
    return np.ascontiguousarray(np.stack([synth_page(bank_x2, SYNTH_SEED_BASE + 4100 + p, 256, 160)[32:32 + R_H, 40:40 + R_W] for p in range(N_PAGES)]))


def _oracle(pages, bank, thr, cap):
    """(counts[n_pages, T], flat matches in (page, template, y, x) order) from the CPU oracle"""
    counts, flat = [], []
    for pg in pages:
        c, m = O.scan_page(O.invert(pg), bank, thr, cap, use_ref=O.have_ref())
        counts.append(np.asarray(c, np.uint32))
        flat.extend(m[t, : c[t]] for t in range(len(c)))
    return np.stack(counts), np.concatenate(flat)


@pytest.fixture(scope="module")
def want(bank, pages):
    """The reference, computed once: per cap (counts, flat list).  The cap of 1 must bite: some call has two or more hits."""
    out = {cap: _oracle(pages, bank, THR, cap) for cap in CAPS}
    assert out[1024][0].max() >= 2, "no (page, template) call with two hits: a cap of 1 would cut nothing"
    assert out[1][0].max() == 1 and out[1][0].sum() < out[1024][0].sum()
    return out


def _results(sc):
    offsets, m = sc.matches()
    return sc.counts().copy(), offsets.copy(), m.copy()


def _check(got, want, what):
    counts, offsets, m = got
    w_counts, w_flat = want
    assert np.array_equal(counts, w_counts), f"{what}: counts"
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(w_counts.reshape(-1), dtype=np.uint64)])), f"{what}: offsets"
    assert m.tobytes() == w_flat.tobytes(), f"{what}: match list"


@pytest.mark.parametrize("cap", CAPS)
def test_matches_in_every_order_a_caller_can_reach(bank, pages, want, cap):
    with Scanner(0) as plain, Scanner(0) as sc:
        plain.set_bank(bank)
        plain.set_pages(pages)
        plain.scan(THR, cap, SCAN_MFMA)
        base = _results(plain)  # a context that never calls process_hits
        _check(base, want[cap], "no process_hits")
        plain.scan(THR, cap, SCAN_DIRECT)
        _check(_results(plain), want[cap], "direct scan")

        def same(what):
            got = _results(sc)
            _check(got, want[cap], what)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base)), what

        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.scan(THR, cap, SCAN_MFMA)  # first scan of the setup: exact sizes
        same("before process_hits")
        sc.process_hits(0.95, 5)
        same("after process_hits, lists already written")
        sc.scan(THR, cap, SCAN_MFMA)  # estimated sizes: nothing has waited when process_hits is queued
        sc.process_hits(0.95, 5)
        same("after process_hits")
        same("called twice")
        sc.scan(THR, cap, SCAN_MFMA)
        sc.process_hits(0.95, 5)
        lines = sc.lines_flat().copy()
        same("after lines()")
        assert sc.lines_flat().tobytes() == lines.tobytes() and len(lines) > 0
        sc.scan(THR, cap, SCAN_DIRECT)
        sc.process_hits(0.95, 5)
        assert sc.lines_flat().tobytes() == lines.tobytes()
        same("direct scan, after lines()")
        sc.scan(THR, cap, SCAN_MFMA)
        sc.process_hits(0.95, 5)
        assert sc.total_matches() == int(want[cap][0].sum())
        assert np.array_equal(sc.counts(), want[cap][0])  # counts alone never need the lists
        same("after counts()")


@pytest.mark.parametrize("cap", CAPS)
def test_executor_batch_with_process_hits_then_late_matches(bank, pages, want, cap):
    """Pipeline.submit(process_hits=True): the lists are asked for on the waited ticket, before its release, while later batches
    of the same lanes are queued or running behind it."""
    pipe = Pipeline(0, 2, 2)
    try:
        pipe.set_bank(bank)
        n = len(pipe.scanners)
        tickets = [pipe.submit(pages, THR, cap, process_hits=True) for _ in range(n)]
        for k in range(2 * n):  # every context twice: its second batch runs on estimated sizes
            t = tickets[k]
            sc = pipe.wait(t)
            assert sc.total_chars() > 0
            lines = sc.lines_flat().copy()
            _check(_results(sc), want[cap], f"ticket {t}")
            _check(_results(sc), want[cap], f"ticket {t}, again")
            assert sc.lines_flat().tobytes() == lines.tobytes()
            pipe.release(t)
            if len(tickets) < 2 * n:
                tickets.append(pipe.submit(pages, THR, cap, process_hits=True))
    finally:
        pipe.close()


def test_no_hits_and_nothing_launched(bank, pages):
    blank = np.full_like(pages, 255)
    empty = (np.zeros((N_PAGES, len(bank)), np.uint32), np.zeros(0, MATCH_DTYPE))
    with Scanner(0) as sc:
        sc.set_bank(bank)
        for what, pg, thr in (("blank pages", blank, THR), ("threshold +inf", pages, float("inf"))):
            sc.set_pages(pg)
            for mode in (SCAN_MFMA, SCAN_MFMA, SCAN_DIRECT):  # exact sizes, estimated sizes, the direct scan
                sc.scan(thr, 1024, mode)
                sc.process_hits(0.95, 5)
                assert sc.total_chars() == 0 and sc.lines() == [[] for _ in range(N_PAGES)]
                _check(_results(sc), empty, what)
                _check(_results(sc), empty, what + ", again")


@pytest.mark.parametrize("cap", CAPS)
def test_forced_split_then_late_matches(bank, pages, want, cap):
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.force_split(True)  # page sub-ranges, as after a candidate overflow: every sub-range's lists are appended
        sc.scan(THR, cap, SCAN_MFMA)
        sc.process_hits(0.95, 5)
        lines = sc.lines_flat().copy()
        _check(_results(sc), want[cap], "split")
        _check(_results(sc), want[cap], "split, again")
        sc.force_split(False)
        sc.scan(THR, cap, SCAN_MFMA)
        sc.process_hits(0.95, 5)
        assert sc.lines_flat().tobytes() == lines.tobytes()
        _check(_results(sc), want[cap], "whole batch after a split one")


@pytest.mark.parametrize("mode", [pytest.param(SCAN_MFMA, id="mfma"), pytest.param(SCAN_DIRECT, id="direct")])
def test_redo_on_overflow_and_pages_of_several_units_then_late_matches(bank, pages, mode):
    """A batch whose estimated sizes prove too small is redone with exact sizes when somebody first waits for it — here lines(), with
    process_hits queued behind the first attempt; the lists asked for afterwards are the redone batch's.  At a threshold of 0.2 a
    96x64 page has far more than 2 048 hits (several units of the ordering pass) and a cap of 3 cuts calls in every unit."""
    thr, cap = 0.2, 3
    sparse = np.full_like(pages, 255)
    sparse[:, 20:40, 10:40] = pages[:, 20:40, 10:40]  # a few glyphs only
    w_sparse, w_dense = _oracle(sparse, bank, thr, cap), _oracle(pages, bank, thr, 1 << 20)
    per_page = w_dense[0].sum(axis=1)
    assert per_page.min() > 2 * 2048, per_page                     # more than two units on every page
    assert w_dense[0].sum() > 1.2 * _oracle(sparse, bank, thr, 1 << 20)[0].sum() + 8192  # beyond any margin of the sparse batch's counts
    w_dense = _oracle(pages, bank, thr, cap)
    assert (w_dense[0] == cap).any()
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(sparse)
        sc.scan(thr, cap, mode)
        _check(_results(sc), w_sparse, "sparse")
        redone = sc.size_estimate_stats()["redone"]
        sc.upload_pages(pages, 0)  # same setup, many times the hits
        sc.scan(thr, cap, mode)
        sc.process_hits(0.9, 5)
        lines = sc.lines_flat().copy()
        if mode == SCAN_MFMA:  # (the direct scan always knows its sizes)
            assert sc.size_estimate_stats()["redone"] == redone + 1
        _check(_results(sc), w_dense, "dense, redone")
        sc.scan(thr, cap, mode)    # estimates from the dense batch now
        sc.process_hits(0.9, 5)
        assert sc.lines_flat().tobytes() == lines.tobytes()
        _check(_results(sc), w_dense, "dense, estimated")
        _check(_results(sc), w_dense, "dense, again")

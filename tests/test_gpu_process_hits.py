"""process_hits on the device (post.hip: mark_anchor_rows, walk_lines, emit_chars, page_offsets) against the reference's
process_hits (oracle.process_hits), page by page: x, y, letter and the similarity bits of every character, in order.

The first half feeds the kernels chosen hit lists through focr_debug_process_hits (Scanner.debug_process_hits), so that ties,
group boundaries and capped hits land on the line walk's 64-element chunk edges on purpose (tests/focr_walk_model.py builds
the lists, tests/test_walk_model.py proves them on the model of the walk first).  The second half goes through the scan:
BASELINE configs[1] at full size, configs[2]'s bank, the executor and the fleet, the size-estimate redo and the `ncc` CLI,
with anchors and overlaps other than the defaults."""
import os
import subprocess

import numpy as np
import pytest

import focr_walk_model as M
from font_ocr_amd import ASCII95, Bank, save_pgm, synth_page, synth_pages
from font_ocr_amd.bank import SYNTH_SEED_BASE
from font_ocr_amd.searcher import SCAN_MFMA, Fleet, FocrError, Pipeline, Scanner
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCC = os.path.join(ROOT, "font_ocr_amd", "bin", "ncc")
FONT = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")


@pytest.fixture(scope="module")
def scanner(bank_x2):
    s = Scanner(0)
    s.set_bank(bank_x2)
    yield s
    s.close()


def _assert_case(sc, bank, case):
    sc.alloc_pages(case.n_pages, case.r_w, case.r_h)
    sc.debug_process_hits(case.page, case.y, case.x, case.t, case.sim, case.keep)
    sc.process_hits(case.anchor, case.overlap)
    got = sc.lines()
    want = M.reference_lines(case)
    letters = bank.templates["letter"]
    for p in range(case.n_pages):
        assert len(got[p]) == len(want[p]), (case, p, len(got[p]), len(want[p]))
        for k, (lg, lw) in enumerate(zip(got[p], want[p])):
            i = np.asarray(lw, np.int64)
            what = (case, p, k)
            assert len(lg) == len(i), what
            assert np.array_equal(lg["x"].astype(np.int64), case.x[i].astype(np.int64)), what
            assert np.array_equal(lg["y"].astype(np.int64), case.y[i].astype(np.int64)), what
            assert np.array_equal(lg["letter"], letters[case.t[i]]), what
            assert lg["similarity"].tobytes() == case.sim[i].tobytes(), what
            assert np.array_equal(lg["template_index"], case.t[i]), what  # the very hit the reference picked
    if case.expect_lines is not None:
        assert sum(len(p) for p in got) == case.expect_lines, case


@pytest.mark.parametrize("family", list(M.FAMILIES))
def test_chosen_hit_lists_vs_reference(scanner, bank_x2, family):
    """Rows of 63 .. 129 and 100 000 hits with their maximum or ties on chunk edges (the later element wins), group boundaries
    and capped hits on chunk edges, every overlap edge (INT32_MIN, -1 ..), every anchor edge (NaN, +-inf ..), signed zeros and
    subnormals, waves whose rows span pages, empty lists, and a seeded fuzz of 300 lists."""
    for case in M.FAMILIES[family]():
        _assert_case(scanner, bank_x2, case)


def test_debug_entry_checks_its_list_and_the_next_scan_replaces_it(scanner, bank_x2):
    sc = scanner
    sc.alloc_pages(2, 64, 17)
    ok = dict(page=[0, 0, 1], y=[3, 3, 0], x=[5, 5, 9], t=[1, 2, 0], similarity=[0.97, 0.99, 0.96], keep=[1, 1, 1])
    for field, bad in (("page", [0, 0, 2]), ("y", [3, 3, 17]), ("x", [5, 5, 64]), ("t", [1, 2, 380]),  # outside pages / bank
                       ("t", [2, 1, 0]), ("t", [1, 1, 0]), ("x", [5, 4, 9]), ("page", [1, 1, 0])):    # not strictly increasing
        with pytest.raises(FocrError):
            sc.debug_process_hits(**dict(ok, **{field: bad}))
    sc.debug_process_hits(**ok)
    sc.process_hits(0.95, 5)
    lines = sc.lines()
    assert [[list(l["template_index"]) for l in p] for p in lines] == [[[2]], [[0]]]
    with pytest.raises(FocrError):
        sc.counts()  # no per-call lists stand behind such hits
    with pytest.raises(FocrError):
        sc.matches()
    page = synth_page(bank_x2, SYNTH_SEED_BASE + 5, 300, 130)
    sc.set_pages(page)
    sc.scan(0.8, 1024, SCAN_MFMA)
    _assert_scan_lines(sc, bank_x2, 1, [(0.95, 5), (0.95, -1)], "scan after the hook")


def _scan_hits(sc, bank, n_pages):
    """The device's own match lists, page by page, as the reference's all_hits (O.raw_hits)."""
    counts = sc.counts()
    offsets, m = sc.matches()
    T = len(bank)
    mm = np.zeros((T, int(max(1, counts.max()))), O.MATCH_DTYPE)
    out = []
    for p in range(n_pages):
        for t in np.flatnonzero(counts[p]):
            s = int(offsets[p * T + t])
            mm[t, : counts[p, t]] = m[s: s + int(counts[p, t])]
        out.append(O.raw_hits(counts[p], mm, bank))
    return out


def _assert_lines(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (lg, lw) in enumerate(zip(got, want)):
        assert len(lg) == len(lw), (what, k)
        assert np.array_equal(lg["x"].astype(np.int64), lw["x"].astype(np.int64)), (what, k)
        assert np.array_equal(lg["y"].astype(np.int64), lw["y"].astype(np.int64)), (what, k)
        assert np.array_equal(lg["letter"], lw["letter"]), (what, k)
        assert lg["similarity"].tobytes() == lw["similarity"].tobytes(), (what, k)


def _assert_scan_lines(sc, bank, n_pages, params, what):
    hits = _scan_hits(sc, bank, n_pages)
    for anchor, overlap in params:
        sc.process_hits(anchor, overlap)
        got = sc.lines()
        n_chars = 0
        for p in range(n_pages):
            want = O.process_hits(hits[p], anchor, overlap)
            _assert_lines(got[p], want, (what, anchor, overlap, p))
            n_chars += sum(len(l) for l in want)
        assert n_chars > 0, (what, anchor, overlap)


def test_c2_full_size_lines_vs_reference(bank_x2):
    """BASELINE configs[1]: 128 pages of 608x720, 380 templates, MFMA scan at 0.8 — every page's lines equal the reference's."""
    n_pages = 128
    with Scanner(0) as sc:
        sc.set_bank(bank_x2)
        sc.set_pages(synth_pages(bank_x2, n_pages, 608, 720))
        sc.scan(0.8, 1024, SCAN_MFMA)
        _assert_scan_lines(sc, bank_x2, n_pages, [(0.95, 5), (0.7, 0), (0.95, -1), (0.5, 1 << 20)], "configs[1]")


def test_c3_bank_lines_vs_reference(bank_x2y2):
    """configs[2]'s bank (1520 templates) on 16 pages of 1200x1600."""
    n_pages = 16
    with Scanner(0) as sc:
        sc.set_bank(bank_x2y2)
        sc.set_pages(synth_pages(bank_x2y2, n_pages, 1200, 1600))
        sc.scan(0.8, 1024, SCAN_MFMA)
        _assert_scan_lines(sc, bank_x2y2, n_pages, [(0.95, 5), (0.95, -1)], "configs[2] bank")


def test_executor_and_fleet_forward_anchor_and_overlap(bank_x2):
    """Pipeline.submit and Fleet.submit hand anchor and overlap to the batch's process_hits: the same characters, byte for byte,
    as Scanner.process_hits with the same arguments."""
    bank = bank_x2.subset(list(range(33, 80)) + list(range(95 + 33, 95 + 80)))
    batches = [synth_pages(bank_x2, 2, 300, 130, first=7000 + 10 * k) for k in range(3)]
    params = [(0.7, 0), (0.95, -1)]
    want = {}
    with Scanner(0) as sc:
        sc.set_bank(bank)
        for k, pg in enumerate(batches):
            sc.set_pages(pg)
            sc.scan(0.8, 1024, SCAN_MFMA)
            _assert_scan_lines(sc, bank, 2, params, f"batch {k}")
            for a, o in params:
                sc.process_hits(a, o)
                want[k, a, o] = sc.lines_flat().tobytes()
            assert want[k, 0.7, 0] != want[k, 0.95, -1]
    pipe = Pipeline(0, 2)
    try:
        pipe.set_bank(bank)
        for a, o in params:
            for k, pg in enumerate(batches):
                t = pipe.submit(pg, 0.8, 1024, SCAN_MFMA, True, a, o)
                got = pipe.wait(t).lines_flat().tobytes()
                pipe.release(t)
                assert got == want[k, a, o], ("pipeline", k, a, o)
    finally:
        pipe.close()
    fl = Fleet([0], lanes=2)
    try:
        fl.set_bank(bank)
        for a, o in params:
            for k, pg in enumerate(batches):
                t = fl.submit(pg, 0.8, 1024, SCAN_MFMA, True, a, o)
                got = fl.wait(t).lines_flat().tobytes()
                fl.release(t)
                assert got == want[k, a, o], ("fleet", k, a, o)
    finally:
        fl.close()


def test_size_estimate_redo_keeps_anchor_and_overlap(bank_x2):
    """A process_hits queued behind a scan that overflows its estimated sizes is re-run with the stored anchor and overlap
    (results.hip: the redo): its lines equal an exact-size run's and the reference's."""
    bank = bank_x2.subset(list(range(33, 80)) + list(range(95 + 33, 95 + 80)))
    dense = synth_pages(bank_x2, 2, 608, 720, first=7100)  # ~18 000 hits a page: far above the sparse batch's bounds (+8192)
    sparse = np.full_like(dense, 255)
    sparse[:, 20:40, 30:120] = dense[:, 20:40, 30:120]
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(sparse)
        for overlap in (-1, 1 << 20):
            sc.upload_pages(sparse, 0)
            sc.scan(0.7, 1024, SCAN_MFMA)
            sc.scan(0.7, 1024, SCAN_MFMA)  # estimated from the sparse batch
            redone = sc.size_estimate_stats()["redone"]
            sc.upload_pages(dense, 0)
            sc.scan(0.7, 1024, SCAN_MFMA)
            sc.process_hits(0.9, overlap)  # queued behind a scan whose bounds are far too small
            got = sc.lines_flat().copy()
            assert sc.size_estimate_stats()["redone"] == redone + 1, overlap
            sc.set_size_estimates(False)
            sc.scan(0.7, 1024, SCAN_MFMA)
            sc.process_hits(0.9, overlap)
            assert sc.lines_flat().tobytes() == got.tobytes() and len(got) > 0, overlap
            _assert_scan_lines(sc, bank, 2, [(0.9, overlap)], "exact run")
            sc.set_size_estimates(True)


@pytest.mark.skipif(not os.path.exists(FONT), reason="DejaVu Sans Mono not installed")
def test_cli_forwards_overlap_and_anchor(tmp_path):
    """`ncc --overlap -1 --anchor-threshold 0.7` and `--overlap=2147483647` print the text of the reference's lines."""
    alphabet = ASCII95[1:60]
    bank = Bank.rasterize(FONT, 13, 1, 0, alphabet=alphabet)
    pages = [synth_page(bank, SYNTH_SEED_BASE + 400 + p, 300 + 20 * p, 130) for p in range(2)]
    paths = []
    for p, pg in enumerate(pages):
        paths.append(str(tmp_path / f"p{p}.pgm"))
        save_pgm(paths[-1], pg)
    hits = [O.raw_hits(*O.scan_page(O.invert(pg), bank, 0.8, use_ref=O.have_ref()), bank) for pg in pages]
    common = [NCC, "-f", FONT, "-t", "13", "--x-bits", "1", "-a", alphabet]
    for flags, anchor, overlap in ((["--overlap", "-1", "--anchor-threshold", "0.7"], 0.7, -1), (["--overlap=2147483647"], 0.95, 2**31 - 1)):
        r = subprocess.run(common + flags + ["-i"] + paths, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want = "".join("".join(chr(int(c)) for c in l["letter"]) + "\n" for h in hits for l in O.process_hits(h, anchor, overlap))
        assert r.stdout == want and len(want) > 20, flags

"""focr_get_runners on the device (post.hip, walk_kernel<true>) against the brute-force definition of tests/ncc_runners_model.py:
members, letter, template_index and x with ==, the similarity as bytes.

The first half feeds the kernel chosen hit lists through focr_debug_process_hits: the families of ncc_runners_model (winners and
runners on chunk edges, demotions, capped hits of another letter, odd similarities) and every family of focr_walk_model.  The
second half goes through the scan -- plain, on size estimates, split --, the executor and the fleet, the other getters in both
orders, the state errors, device memory and `ncc --scores`."""
import csv
import os
import subprocess

import numpy as np
import pytest

import focr_walk_model as W
import ncc_runners_model as R
from font_ocr_amd import ASCII95, Bank, _native as N, save_pgm, synth_page, synth_pages
from font_ocr_amd.bank import SYNTH_SEED_BASE
from font_ocr_amd.searcher import NO_RUNNER, RUNNER_DTYPE, SCAN_MFMA, Fleet, FocrError, Pipeline, Scanner
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCC = os.path.join(ROOT, "font_ocr_amd", "bin", "ncc")
FONT = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FAMILIES = {**R.FAMILIES, **W.FAMILIES}


@pytest.fixture(scope="module")
def scanner(bank_x2):
    s = Scanner(0)
    s.set_bank(bank_x2)
    yield s
    s.close()


def _assert_against(sc, case, what):
    """The scanner's characters and runner records against the definition over `case` (the hits the scanner holds)."""
    want_lines, want = R.brute_force(case)
    chars, got = sc.lines_flat(), sc.runners()
    win = np.array([i for page in want_lines for line in page for i in line], np.int64)
    assert len(chars) == len(win) == len(got), (what, len(chars), len(win), len(got))
    assert np.array_equal(chars["template_index"], case.t[win]) and np.array_equal(chars["x"], case.x[win]), what  # aligned with the characters
    assert chars["similarity"].tobytes() == case.sim[win].tobytes(), what
    assert R.same_records(got, want) is None, (what, R.same_records(got, want))
    return got


@pytest.mark.parametrize("family", list(FAMILIES))
def test_chosen_hit_lists_vs_definition(scanner, family):
    sc = scanner
    for case in FAMILIES[family]():
        sc.alloc_pages(case.n_pages, case.r_w, case.r_h)
        sc.debug_process_hits(case.page, case.y, case.x, case.t, case.sim, case.keep)
        sc.process_hits(case.anchor, case.overlap)
        _assert_against(sc, case, case)


def _case_of_scan(sc, bank, n_pages, anchor, overlap):
    """The device's own match lists as a Case: the reference's all_hits page by page (O.raw_hits), with their template indices."""
    counts = sc.counts()
    offsets, m = sc.matches()
    T = len(bank)
    mm = np.zeros((T, int(max(1, counts.max()))), O.MATCH_DTYPE)
    parts = []
    for p in range(n_pages):
        for t in np.flatnonzero(counts[p]):
            s = int(offsets[p * T + t])
            mm[t, : counts[p, t]] = m[s: s + int(counts[p, t])]
        hits = O.raw_hits(counts[p], mm, bank)
        if len(hits):
            parts.append((p, hits["y"], hits["x"], np.repeat(np.arange(T), counts[p]), hits["similarity"], 1))
    assert (counts < 1024).all()  # nothing capped: every hit is kept
    return W.Case("scan", parts, anchor=anchor, overlap=overlap, n_pages=n_pages, r_w=sc.r_w, r_h=sc.r_h)


PAGE = None


def _page(bank):
    global PAGE
    if PAGE is None:
        PAGE = synth_page(bank, SYNTH_SEED_BASE + 5, 300, 130)
    return PAGE


def test_through_the_scan(scanner, bank_x2):
    """The counts were computed with the CPU oracle: at 0.8 / (0.95, 5) 78 characters, 44 with a runner; at 0.6 / (0.9, 2) 159
    characters, 128 with a runner, groups of up to 101 members (the walk crosses a chunk edge); (0.95, -1): no runners."""
    sc = scanner
    sc.set_pages(_page(bank_x2))
    for thr, anchor, overlap, n_chars, n_with, max_members in ((0.8, 0.95, 5, 78, 44, None), (0.6, 0.9, 2, 159, 128, 101)):
        sc.scan(thr, 1024, SCAN_MFMA)
        sc.process_hits(anchor, overlap)
        got = _assert_against(sc, _case_of_scan(sc, bank_x2, 1, anchor, overlap), (thr, anchor, overlap))
        has = got["template_index"] != NO_RUNNER
        print(f"threshold {thr} ({anchor}, {overlap}): {len(got)} characters, {int(has.sum())} with a runner, members up to {int(got['members'].max())}")
        assert (len(got), int(has.sum())) == (n_chars, n_with)
        assert has.any() and not has.all()
        if max_members:
            assert int(got["members"].max()) == max_members > 64
    sc.scan(0.8, 1024, SCAN_MFMA)
    sc.process_hits(0.95, -1)
    got = _assert_against(sc, _case_of_scan(sc, bank_x2, 1, 0.95, -1), "(0.95, -1)")
    assert len(got) > 78 and (got["template_index"] == NO_RUNNER).all() and (got["members"] == 1).all()
    assert np.isneginf(got["similarity"]).all() and not got["x"].any() and (got["letter"] == NO_RUNNER).all()


def test_rerun_estimates_and_split(bank_x2):
    """A new process_hits replaces the records; a second scan on size estimates and a split scan give the same records; a second
    call copies without a launch."""
    with Scanner(0) as sc:
        sc.set_bank(bank_x2)
        sc.set_pages(_page(bank_x2))
        sc.scan(0.8, 1024, SCAN_MFMA)  # exact sizes
        sc.process_hits(0.95, 5)
        first = sc.runners()
        assert sc.last_runners()["launches"] == 1 and sc.last_runners()["ms"] > 0
        again = sc.runners()
        assert sc.last_runners() == {"ms": 0.0, "launches": 0} and again.tobytes() == first.tobytes()
        sc.process_hits(0.9, 1)
        other = _assert_against(sc, _case_of_scan(sc, bank_x2, 1, 0.9, 1), "(0.9, 1)")
        assert sc.last_runners()["launches"] == 1
        assert len(other) != len(first)
        sc.process_hits(0.95, 5)
        assert sc.runners().tobytes() == first.tobytes()
        sc.scan(0.8, 1024, SCAN_MFMA)  # on the first scan's size estimates, everything queued
        sc.process_hits(0.95, 5)
        assert sc.runners().tobytes() == first.tobytes()
        lines, nested = sc.lines(runners=True)
        assert [[len(l) for l in p] for p in lines] == [[len(l) for l in p] for p in nested]
        assert np.concatenate([l for p in nested for l in p]).tobytes() == first.tobytes()
        sc.force_split(True)
        sc.scan(0.8, 1024, SCAN_MFMA)
        sc.process_hits(0.95, 5)
        assert sc.runners().tobytes() == first.tobytes()
        sc.force_split(False)


def test_estimates_redo(bank_x2):
    """runners() as the first wait for a batch whose counts exceed the estimates taken from the scan before it: the batch and the
    process_hits queued behind it are redone on exact sizes, and the records are those of an exact run."""
    bank = bank_x2.subset(list(range(33, 80)) + list(range(95 + 33, 95 + 80)))
    dense = synth_pages(bank_x2, 2, 608, 720, first=7100)  # ~18 000 hits a page: far above the sparse batch's bounds
    sparse = np.full_like(dense, 255)
    sparse[:, 20:40, 30:120] = dense[:, 20:40, 30:120]
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(sparse)
        sc.scan(0.7, 1024, SCAN_MFMA)
        sc.scan(0.7, 1024, SCAN_MFMA)  # estimated from the sparse batch
        sc.process_hits(0.9, 5)
        few = sc.runners()
        redone = sc.size_estimate_stats()["redone"]
        sc.upload_pages(dense, 0)
        sc.scan(0.7, 1024, SCAN_MFMA)
        sc.process_hits(0.9, 5)  # queued behind a scan whose bounds are far too small
        buf = np.zeros(1 << 18, RUNNER_DTYPE)  # (Scanner.runners() would ask for the number of characters first, and that would be the wait)
        sc._ck(sc._lib.focr_get_runners(sc._h, buf.ctypes.data))
        got = buf[: sc.total_chars()].copy()
        assert not buf[len(got):].view(np.uint8).any()
        assert sc.size_estimate_stats()["redone"] == redone + 1
        assert sc.lines_flat().shape == got.shape
        sc.set_size_estimates(False)
        sc.scan(0.7, 1024, SCAN_MFMA)
        sc.process_hits(0.9, 5)
        want = sc.runners()
        assert len(few) < len(got) and got.tobytes() == want.tobytes()
        assert (got["template_index"] != NO_RUNNER).any() and (got["template_index"] == NO_RUNNER).any()


def test_executor_and_fleet(bank_x2):
    batches = [synth_pages(bank_x2, 2, 300, 130, first=5300 + 2 * b) for b in range(3)]
    want = []
    with Scanner(0) as sc:
        sc.set_bank(bank_x2)
        for luma in batches:
            sc.set_pages(luma)
            sc.scan(0.8)
            sc.process_hits(0.95, 5)
            want.append((sc.lines_flat(), sc.runners()))
    assert want[0][1].tobytes() != want[1][1].tobytes() and all((w[1]["template_index"] != NO_RUNNER).any() for w in want)
    for make in (lambda: Pipeline(0, 2), lambda: Fleet([0], lanes=2)):
        ex = make()
        try:
            ex.set_bank(bank_x2)
            tickets = [ex.submit(luma, threshold=0.8, anchor_threshold=0.95, overlap=5) for luma in batches]
            for t, (chars, runners) in zip(tickets, want):  # later batches are queued behind the one that is read
                view = ex.wait(t)
                assert view.runners().tobytes() == runners.tobytes()
                assert view.lines_flat().tobytes() == chars.tobytes()
                lines, nested = view.lines(runners=True)
                assert sum(len(l) for p in nested for l in p) == len(runners)
                ex.release(t)
        finally:
            ex.close()


def test_order_independence(bank_x2):
    """runners(), verify_images(), lines() and matches() in both orders: each gives what it gives alone."""
    calls = {"runners": lambda s: s.runners().tobytes(), "verify": lambda s: b"".join(a.tobytes() for a in s.verify_images()),
             "lines": lambda s: s.lines_flat().tobytes(), "matches": lambda s: b"".join(a.tobytes() for a in s.matches())}
    with Scanner(0) as sc:
        sc.set_bank(bank_x2)
        sc.set_pages(_page(bank_x2))

        def fresh():
            sc.scan(0.8, 1024, SCAN_MFMA)
            sc.process_hits(0.95, 5)

        alone = {}
        for name, f in calls.items():
            fresh()
            alone[name] = f(sc)
        names = list(calls)
        for order in (names, names[::-1]):
            fresh()
            for name in order:
                assert calls[name](sc) == alone[name], (order, name)
        assert len(alone["runners"]) == 78 * RUNNER_DTYPE.itemsize


def test_state_and_zero_characters(bank_x2):
    with Scanner(0) as sc:
        sc.set_bank(bank_x2)
        sc.set_pages(_page(bank_x2))
        with pytest.raises(FocrError, match=r"\[3\]"):  # FOCR_ERR_STATE: before any scan
            sc.runners()
        sc.scan(0.8)
        with pytest.raises(FocrError, match=r"\[3\]"):  # a scan without process_hits
            sc.runners()
        sc.process_hits(0.95, 5)
        assert len(sc.runners()) == 78
        sc.scan(0.8)
        with pytest.raises(FocrError, match=r"\[3\]"):  # the next scan: again until process_hits has run
            sc.runners()
        sc.process_hits(2.0, 5)  # no row reaches the anchor: hits, but no characters
        assert sc.total_chars() == 0 and len(sc.runners()) == 0 and sc.last_runners()["launches"] == 0
        sc.set_pages(np.full((1, 130, 300), 255, np.uint8))  # no hits at all: process_hits launches nothing
        sc.scan(0.8)
        sc.process_hits(0.95, 5)
        r = sc.runners()
        assert r.dtype == RUNNER_DTYPE and len(r) == 0


def test_scanner_gives_back_every_byte(bank_x2):
    live = lambda: int(N.hip().focr_debug_device_bytes())  # noqa: E731
    before = live()
    sc = Scanner(0)
    sc.set_bank(bank_x2)
    sc.set_pages(_page(bank_x2))
    sc.scan(0.8)
    sc.process_hits(0.95, 5)
    held = live()
    assert len(sc.runners()) == 78
    assert live() > held  # the record buffer exists only once somebody has asked
    sc.scan(0.6)
    sc.process_hits(0.9, 2)
    assert len(sc.runners()) == 159
    sc.close()
    assert live() == before


@pytest.mark.skipif(not os.path.exists(FONT), reason="DejaVu Sans Mono not installed")
def test_cli_scores(tmp_path):
    if not os.path.exists(NCC):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    alphabet = ASCII95[1:60]
    bank = Bank.rasterize(FONT, 13, 1, 0, alphabet=alphabet)
    pages = np.stack([synth_page(bank, SYNTH_SEED_BASE + 800 + p, 300, 100) for p in range(2)])
    paths = []
    for p in range(2):
        paths.append(str(tmp_path / f"page{p}.pgm"))
        save_pgm(paths[-1], pages[p])
    out = tmp_path / "scores.csv"
    cmd = [NCC, "-f", FONT, "-t", "13", "--x-bits", "1", "-a", alphabet, "-i"] + paths
    plain = subprocess.run(cmd, capture_output=True)
    scored = subprocess.run(cmd + ["--scores", str(out)], capture_output=True)
    assert plain.returncode == 0 and scored.returncode == 0, scored.stderr
    assert scored.stdout == plain.stdout and len(plain.stdout) > 50
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.scan(0.8)
        sc.process_hits(0.95, 5)
        lines, runners = sc.lines(runners=True)
    rows = list(csv.reader(open(out)))
    assert rows[0] == "image_index,line,column,codepoint,x,y,similarity,members,runner_codepoint,runner_x,runner_similarity,margin".split(",")
    want = []
    for p in range(2):
        for l, (line, rl) in enumerate(zip(lines[p], runners[p])):
            for k, (c, r) in enumerate(zip(line, rl)):
                head = [p, l, k, int(c["letter"]), int(c["x"]), int(c["y"]), c["similarity"], int(r["members"])]
                want.append(head + ([None] * 4 if r["template_index"] == NO_RUNNER else
                                    [int(r["letter"]), int(r["x"]), r["similarity"], float(c["similarity"]) - float(r["similarity"])]))
    assert len(rows) - 1 == len(want) > 20
    kinds = set()
    for row, w in zip(rows[1:], want):
        assert [int(v) for v in row[:6]] == w[:6] and np.float32(row[6]) == w[6] and int(row[7]) == w[7], (row, w)
        kinds.add(w[8] is None)
        if w[8] is None:
            assert row[8:] == ["", "", "", ""], row
        else:
            assert (int(row[8]), int(row[9])) == (w[8], w[9]) and np.float32(row[10]) == w[10], (row, w)
            assert float(row[11]) == float(f"{w[11]:.9g}"), (row, w)  # the double difference, printed as %.9g
    assert kinds == {True, False}

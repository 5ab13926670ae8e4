"""Row pairs in the MFMA scan (scan_mfma2.hip, PAIR: two window rows per fragment load against two operand images of the bank; the work
list of row pairs: stats.hip) on the device, at the shapes where pairing can go wrong.  Every scan's match lists equal the oracle's bit for
bit (x, y, f32 bits, order), the direct scan gives the same lists, the library reports the form it took (focr_debug_scan_paired), and the
candidate list of the paired form equals, as a set and without duplicates, that of the unpaired form on the same context — forced through
focr_debug_set_stats_form(1): the LDS-tiled statistics leave mark bytes, and a work list made from mark bytes is never paired.

Pages are at most 3 x (96 x 64); banks are at most 40 templates of the committed one (8x15 and 9x15, 15 of LAYOUT_W8's 16 rows), except
where a case needs what that bank does not have: a 16-row class, the other two K layouts, and 37 N-tiles (a bank whose two images do not
fit one launch cannot be smaller than 577 templates)."""
import os

import numpy as np
import pytest

import prefilter_cases as PC
from font_ocr_amd.bank import Bank
from font_ocr_amd.searcher import PREFILTER_AUTO, SCAN_DIRECT, SCAN_MFMA, Scanner
from oracle import oracle as O
from test_gpu_parity import _assert_same, _csr_to_lists

pytestmark = pytest.mark.gpu

CAP = 1024
N_H = 15  # both size classes of the committed bank


@pytest.fixture(scope="module")
def full():
    return Bank.load(os.path.join(PC.GOLD, "bank_dejavu13_ascii95_x2.bin"))


@pytest.fixture(scope="module")
def bank40(full):
    return full.subset(list(range(33, 53)) + list(range(95 + 33, 95 + 53)))  # 20 glyphs at both sub-pixel shifts: 8x15 and 9x15


def _oracle(ink_pages, bank, thr):
    out = []
    for pg in ink_pages:
        counts, matches = O.scan_page(np.ascontiguousarray(pg), bank, thr, CAP, use_ref=O.have_ref())
        out.append([matches[t, : counts[t]] for t in range(len(counts))])
    return out


def _lists(sc, n_pages, T):
    offsets, m = sc.matches()
    return _csr_to_lists(offsets, m, n_pages, T)


def _cand_set(sc, shape):
    """The candidate list as a set of (page, y, x, t); no duplicates, every key inside the batch."""
    cand = sc.candidates()
    assert len(cand) == sc.counters()["candidates"]
    n_pages, r_h, r_w, T = shape
    assert (cand[:, 0] < n_pages).all() and (cand[:, 1] < r_h).all() and (cand[:, 2] < r_w).all() and (cand[:, 3] < T).all()
    keys = set(map(tuple, cand.tolist()))
    assert len(keys) == len(cand), "duplicates in the candidate list"
    return keys


def _both_forms(bank, ink, thr, want_paired, what, direct=True):
    """Paired (where the pass can) and unpaired scans of one context: lists against the oracle, exact and estimated sizes; candidate sets against
    each other.  Returns the paired form's candidate set."""
    ink = np.ascontiguousarray(ink)
    n_pages, r_h, r_w = ink.shape
    T = len(bank)
    want = _oracle(ink, bank, thr)
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(ink, invert=False)
        sets = []
        for form in (0, 1):
            sc.set_stats_form(form)
            for which in ("exact sizes", "estimated sizes"):
                sc.scan(thr, CAP, SCAN_MFMA)
                _assert_same(_lists(sc, n_pages, T), want, f"{what}, statistics form {form}, {which}")
                launches, paired = sc.scan_paired()
                assert launches >= 1 and paired == (want_paired if form == 0 else 0), (what, form, which, launches, paired, sc.launches())
                sets.append(_cand_set(sc, (n_pages, r_h, r_w, T)))
        assert sets[0] == sets[1] == sets[2] == sets[3], (what, [len(s) for s in sets], sorted(sets[0] ^ sets[2])[:8])
        if direct:
            sc.set_stats_form(0)
            sc.scan(thr, CAP, SCAN_DIRECT)
            _assert_same(_lists(sc, n_pages, T), want, f"{what}, direct scan")
    return sets[0], want


def _plant(ink, bank, t, p, y, x, rng, blend=1.0):
    nd = bank.needle(t).astype(np.float64)
    wn = np.clip(np.rint(blend * nd + (1.0 - blend) * rng.uniform(0, 255, nd.shape)), 0, 255).astype(np.uint8)
    ink[p, y:y + wn.shape[0], x:x + wn.shape[1]] = wn


@pytest.mark.parametrize("rows", [1, 2, 3, 16, 17, 31, 32, 33])
def test_row_parity_and_page_bottom(bank40, rows):
    """r_h - n_h searched rows: a lone last row, a last pair whose partner is not searched, band edges.  Glyphs sit in the first row, the last
    row and the row above it (where there is one), on three pages: planted glyphs, blank, texture."""
    r_w, r_h = 96, rows + N_H
    rng = np.random.default_rng(rows)
    ink = np.zeros((3, r_h, r_w), np.uint8)
    spots = [(1, 1), (rows, 12), (max(rows - 1, 1), 30), ((rows + 1) // 2, 48), (rows, 70)]
    for i, (y, x) in enumerate(spots):
        _plant(ink, bank40, i % 20 + 20 * (i % 2), 0, y, x, rng, 1.0 - 0.03 * i)
    ink[2] = rng.integers(0, 256, (r_h, r_w), dtype=np.uint8)
    ink[2][rng.random((r_h, r_w)) < 0.5] = 0
    _plant(ink, bank40, 3, 2, rows, 50, rng)
    cands, want = _both_forms(bank40, ink, 0.8, 1, f"{rows} searched rows")
    hits = sum(len(m) for pl in want for m in pl)
    last = sum(int((m["y"] == rows).sum()) for pl in want for m in pl)
    assert hits > 0 and last > 0, (hits, last)  # the last searched row holds a match
    assert all(1 <= y <= rows for _, y, _, _ in cands)


@pytest.mark.parametrize("speck_row", [20, 21, 34, 35])
def test_single_live_pairs(bank40, speck_row):
    """One pixel of ink on blank paper: the live window rows are speck_row - 14 .. speck_row.  An even speck row ends them with the UPPER row
    of a pair alone (its partner below sees only paper), an odd one starts them with the LOWER row of a pair alone.  At threshold -1 every
    live window is a candidate for every live template, so a key of the dead row of such a pair would show."""
    r_w, r_h = 96, 64
    ink = np.zeros((2, r_h, r_w), np.uint8)
    ink[0, speck_row, 50] = 200
    ink[1, speck_row, 3] = 90  # at the left edge: the M-tile of x = 0 (never searched) is live through its other windows
    top, bottom = speck_row - 14, speck_row
    assert (bottom % 2 == 0) or (top % 2 == 1)
    for thr in (-1.0, 0.3):
        cands, want = _both_forms(bank40, ink, thr, 1, f"speck at row {speck_row}, threshold {thr}", direct=thr < 0)
        rows = sorted({y for _, y, _, _ in cands})
        assert all(top <= y <= bottom for y in rows), (speck_row, rows)
        if thr < 0:
            assert rows[0] == top and rows[-1] == bottom, (speck_row, rows)  # both lone rows did emit; their dead partners did not
            assert sum(len(m) for pl in want for m in pl) > 0


@pytest.mark.parametrize("case_id", ["drop9", "dead", "clamp-lo"])
def test_candidate_sets_of_the_prefilter_cases(case_id):
    """Cases of tests/prefilter_cases.py whose passes pair and whose pages are small (DROP alone; PAIR statistics, dead slots and a negative
    threshold; every pair a candidate): the same candidate set in both forms — tests/test_gpu_prefilter_model.py holds that set against the
    host model, for these and for the larger cases that pair ("pair9", "pair9-neg", "bench", "saturated")."""
    case, bank, pages = PC.build(case_id)
    assert case.get("prefilter", PREFILTER_AUTO) == PREFILTER_AUTO and case.get("drop", True)
    cands, _ = _both_forms(bank, pages, case["thr"], 1, case_id, direct=False)
    assert len(cands) > 0


@pytest.mark.parametrize("thr", [0.0, -1.0])
def test_thresholds_at_and_below_zero_emit_no_dead_slot(full, thr):
    """Dead slots (the space glyph at both shifts) and the padding of a class's last N-tile pass G + C-in > 0 at thresholds <= 0; neither
    image may emit them (the segment's dead-tile offset is the same in both)."""
    idx = [0, 95] + list(range(33, 52)) + list(range(95 + 33, 95 + 52))  # 2 + 19 + 19 templates: the classes end in partly filled tiles
    bank = full.subset(idx)
    dead = [i for i in range(len(bank)) if bank.needle(i).min() == bank.needle(i).max()]
    assert len(dead) == 2 and len(bank) == 40
    rng = np.random.default_rng(5)
    ink = np.zeros((1, 34, 48), np.uint8)
    ink[0, 4:30, 6:40] = rng.integers(0, 256, (26, 34), dtype=np.uint8)
    _plant(ink, bank, 7, 0, 2, 20, rng)
    cands, want = _both_forms(bank, ink, thr, 1, f"threshold {thr}")
    assert len(cands) > 0 and not any(t in dead for _, _, _, t in cands)
    assert all(len(want[0][t]) == 0 for t in dead)


def test_other_layouts_pair_too():
    """LAYOUT_W16 at 4 and 2 K-steps (15 of 16 rows, 7 of 8) and LAYOUT_W12 (15 and 14 of 16 rows): the committed bank has neither."""
    rng = np.random.default_rng(11)
    for classes, n_passes in (([(16, 15, 17), (16, 7, 5)], 2), ([(12, 15, 17), (8, 14, 4)], 1)):
        needles = [rng.integers(0, 256, (n_h, n_w), dtype=np.uint8) for n_w, n_h, count in classes for _ in range(count)]
        bank = PC.bank_of([needles[i] for i in rng.permutation(len(needles))])
        ink = np.zeros((3, 49, 96), np.uint8)
        ink[0] = rng.integers(0, 256, (49, 96), dtype=np.uint8)
        ink[0][rng.random((49, 96)) < 0.5] = 0
        ink[2, 20:, :40] = rng.integers(0, 256, (29, 40), dtype=np.uint8)
        for i in range(6):
            nd = bank.needle(i)
            y = (1, 49 - nd.shape[0], 48 - nd.shape[0], 17, 18, 2)[i]
            ink[2, y:y + nd.shape[0], 2 + 15 * i:2 + 15 * i + nd.shape[1]] = nd
        cands, want = _both_forms(bank, ink, 0.3, n_passes, f"classes {classes}")
        assert len(cands) > 0 and sum(len(m) for pl in want for m in pl) > 0


def test_passes_that_cannot_pair_stay_single():
    """A 16-row class fills its K block; 37 N-tiles fit a launch once, not twice: both scans take the unpaired kernel and give the oracle's lists."""
    rng = np.random.default_rng(3)
    for classes, geom in (([(8, 16, 20), (8, 15, 6)], (2, 40, 96)), ([(8, 15, 16 * 36 + 1)], (1, 24, 48))):
        needles = [rng.integers(0, 256, (n_h, n_w), dtype=np.uint8) for n_w, n_h, count in classes for _ in range(count)]
        bank = PC.bank_of(needles)
        n_pages, r_h, r_w = geom
        ink = rng.integers(0, 256, geom, dtype=np.uint8)
        ink[rng.random(geom) < 0.5] = 0
        for i in range(3):
            nd = bank.needle(i * 7)
            ink[0, 1 + i:1 + i + nd.shape[0], 1 + 12 * i:1 + 12 * i + nd.shape[1]] = nd
        cands, want = _both_forms(bank, ink, 0.3, 0, f"classes {[c[:2] for c in classes]}")
        assert len(cands) > 0 and sum(len(m) for pl in want for m in pl) > 0

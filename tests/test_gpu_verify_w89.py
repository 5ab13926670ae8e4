"""The exact verify's form for banks of 8- and 9-wide templates of one height (verify_candidate_w89, verify.h; verify_list_kernel<3>,
verify.hip: template rows of 8 bytes, the ninth column packed four rows to a dword) on the device.  The form computes the same integers as
the 12-byte form and shares its f64 epilogue, so everything a scan returns must be the same bit for bit: per context, the 8-byte form (as
designed) and the 12-byte form (focr_debug_set_verify_form(1)) give the same offsets, match lists (x, y, f32 bits, order), counts and
candidate sets, with exact and with estimated sizes, and both equal the exact scan (SCAN_DIRECT) on the same pages; the library reports the
form each scan took (focr_debug_tail_path).  A hit's slot inside its bucket is handed out by an atomic and differs from run to run in
either form; the row sort behind it makes the lists independent of it, and the lists are what is compared.

Pages are at most 2 x (160 x 96), banks at most 32 templates: glyphs of the committed bank (8x15 and 9x15) or noise templates where a case
needs another height or width."""
import os

import numpy as np
import pytest

import prefilter_cases as PC
from font_ocr_amd import synth_page
from font_ocr_amd.bank import SYNTH_SEED_BASE, Bank
from font_ocr_amd.searcher import SCAN_MFMA, Scanner
from verify_cases import CAP, noise_bank as _noise_bank, noise_pages as _noise_pages, scan_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bank32():
    full = Bank.load(os.path.join(PC.GOLD, "bank_dejavu13_ascii95_x2.bin"))
    bank = full.subset(list(range(33, 49)) + list(range(95 + 33, 95 + 49)))  # 16 glyphs at both sub-pixel shifts
    widths = sorted({bank.needle(t).shape[1] for t in range(len(bank))})
    heights = {bank.needle(t).shape[0] for t in range(len(bank))}
    assert widths == [8, 9] and heights == {15}, (widths, heights)
    return bank


def _scan_all(sc, thr, form_designed, what):
    """Both verify forms of one context, then the exact scan: all results equal (verify_cases.scan_all)."""
    return scan_all(sc, thr, ((0, form_designed), (1, "lds12")), what)


@pytest.mark.parametrize("thr", [0.8, 0.3])
def test_both_forms_bit_identical_on_text(bank32, thr):
    """Synthetic text of the bank's glyphs: at 0.8 a few candidates per wave, at 0.3 every wave of the verify full, both widths inside it."""
    luma = np.stack([synth_page(bank32, SYNTH_SEED_BASE + 40 + i, 160, 96) for i in range(2)])
    with Scanner(0) as sc:
        sc.set_bank(bank32)
        sc.set_pages(luma)
        m, cands = _scan_all(sc, thr, "lds8", f"text, threshold {thr}")
    assert len(m) > 0
    by_width = {w: sum(1 for *_, t in cands if bank32.needle(t).shape[1] == w) for w in (8, 9)}
    assert by_width[8] > 0 and by_width[9] > 0, by_width
    if thr < 0.5:
        assert len(cands) > 64 * 16, len(cands)  # more than one step of a whole workgroup


def test_last_row_and_column_odd_count_blank_page(bank32):
    """A match at x = r_w - n_w, y = r_h - n_h for a template of either width (the last readable row and column of two pages), a candidate
    count that is no multiple of 64, and a blank page between them."""
    r_w, r_h = 97, 47
    t8 = next(t for t in range(len(bank32)) if bank32.needle(t).shape[1] == 8)
    t9 = next(t for t in range(len(bank32)) if bank32.needle(t).shape[1] == 9)
    ink = np.zeros((3, r_h, r_w), np.uint8)
    for p, t in ((0, t8), (2, t9)):
        nd = bank32.needle(t)
        ink[p, r_h - 15:, r_w - nd.shape[1]:] = nd
        ink[p, 1:16, 1:1 + nd.shape[1]] = nd
    with Scanner(0) as sc:
        sc.set_bank(bank32)
        sc.set_pages(ink, invert=False)
        m, cands = _scan_all(sc, 0.8, "lds8", "page corners")
        assert len(cands) % 64 != 0 and not any(p == 1 for p, *_ in cands), len(cands)
        offsets = sc.matches()[0]
        counts = sc.counts()
    assert counts[1].sum() == 0
    for p, t, n_w in ((0, t8, 8), (2, t9, 9)):
        mm = m[int(offsets[p * len(bank32) + t]):int(offsets[p * len(bank32) + t + 1])]
        at = {(int(a["x"]), int(a["y"])) for a in mm}
        assert (r_w - n_w, r_h - 15) in at and (1, 1) in at, (p, t, at)


def test_zero_candidates(bank32):
    with Scanner(0) as sc:
        sc.set_bank(bank32)
        sc.set_pages(np.zeros((2, 40, 64), np.uint8), invert=False)
        for form in (0, 1):
            sc.set_verify_form(form)
            sc.scan(0.8, CAP, SCAN_MFMA)
            assert sc.counters()["candidates"] == 0 and sc.counts().sum() == 0 and len(sc.matches()[1]) == 0


@pytest.mark.parametrize("n_h", [1, 4, 5, 8, 9, 12, 13, 16])
def test_heights_around_the_row_groups(n_h):
    """The form's row loop runs in two groups of eight page rows, its ninth column in dwords of four: one height per bank at every edge of
    both, noise templates of both widths on noise, every template planted once."""
    bank = _noise_bank([(8, n_h, 5), (9, n_h, 6)], 100 + n_h)
    shape = (2, 2 * n_h + 7, 96)
    plants = [(t, t % 2, 1 if (t // 2) % 2 == 0 else shape[1] - n_h, 1 + 8 * t) for t in range(len(bank))]  # the first and the last searched row
    ink = _noise_pages(bank, shape, 200 + n_h, plants)
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(ink, invert=False)
        m, cands = _scan_all(sc, 0.3, "lds8", f"n_h = {n_h}")
    assert len(m) >= len(bank) and len(cands) >= len(m)


def test_threshold_ties(bank32):
    """Thresholds at a returned similarity and at its two neighbours (the threshold is an f32 in the interface, so the neighbours are f32s):
    the emit test is a strict `>` in f64, and both forms draw the line where the exact scan does."""
    luma = np.stack([synth_page(bank32, SYNTH_SEED_BASE + 50, 160, 96)])
    with Scanner(0) as sc:
        sc.set_bank(bank32)
        sc.set_pages(luma)
        sc.scan(0.8, CAP, SCAN_MFMA)
        sims = np.unique(sc.matches()[1]["similarity"])
        assert len(sims) >= 3
        s = np.float32(sims[len(sims) // 2])  # neither the lowest nor the highest: hits on both sides of it
        n_at = []
        for thr in (np.nextafter(s, np.float32(0)), s, np.nextafter(s, np.float32(2))):
            m, _ = _scan_all(sc, float(thr), "lds8", f"threshold {float(thr)!r}")
            n_at.append(len(m))
            assert (m["similarity"].astype(np.float64) >= float(thr)).all()  # (the f64 similarity is above; its f32 rounding may be equal)
    # the hit whose f32 similarity is s lies above the lower neighbour and not above the upper one; at s itself its f64 value decides
    assert n_at[0] >= n_at[1] >= n_at[2] > 0 and n_at[0] > n_at[2], n_at


@pytest.mark.parametrize("classes", [[(8, 15, 6), (9, 15, 6), (7, 15, 2)], [(8, 15, 6), (9, 15, 6), (10, 15, 2)], [(9, 15, 8), (12, 15, 2)],
                                     [(8, 15, 6), (9, 14, 6)], [(8, 15, 12)]],
                         ids=["w7", "w10", "w12", "two-heights", "w8-alone"])
def test_other_banks_keep_the_12_byte_form(classes):
    """A template of another width, two heights, or no nine-wide template at all: the 12-byte form whatever the hook says, same results."""
    bank = _noise_bank(classes, 7 + len(classes[0]) + classes[-1][0])
    shape = (2, 40, 128)
    plants = [(t, t % 2, 1 + 11 * (t % 3), 1 + 9 * t) for t in range(min(len(bank), 13))]
    ink = _noise_pages(bank, shape, 9 + classes[-1][0], plants)
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(ink, invert=False)
        m, cands = _scan_all(sc, 0.3, "lds12", f"classes {classes}")
    assert len(m) >= len(plants) and len(cands) >= len(m)


def test_nine_wide_alone_takes_the_8_byte_form():
    bank = _noise_bank([(9, 15, 9)], 31)
    ink = _noise_pages(bank, (1, 48, 96), 32, [(t, 0, 1 + 16 * (t % 2), 1 + 10 * t) for t in range(len(bank))])
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(ink, invert=False)
        m, _ = _scan_all(sc, 0.3, "lds8", "9 x 15 alone")
    assert len(m) >= len(bank)

"""The second operand image of the MFMA bank (row pairs: scan_mfma2.hip, PAIR) on the CPU: it is a pure function of the first.

Where every size class of a pass leaves the last row of its K block empty and both images fit one launch, the bank holds every template a
second time, one row lower in its K block (bank_mfma.hip: layout_supers, quantise_bank).  Checked here against a plain-Python form of the
K layouts (mfma_common.h: kgroup_of), for all three layouts: byte (K-step, lane group, byte) of row j in the second image is the first
image's byte of row j, found where row j + 1 lies; nothing else is set in the second image; dead and padding slots are empty in both; and
a pass that cannot pair has one image only.  No device."""
import numpy as np

import prefilter_cases as PC
from font_ocr_amd.searcher import bank_images, prefilter_page_model

W16, W8, W12 = 1, 2, 3


def kgroup_of(layout, j, x):
    """(row j, column x) of a template -> (K-step, lane group, byte in the 16-byte group): mfma_common.h, written out again."""
    if layout == W16:
        return j // 4, j % 4, x
    if layout == W8:
        q = j // 2
        return q // 4, q % 4, 8 * (j % 2) + x
    m = j // 4
    return 3 * (m // 4) + x // 4, m % 4, 4 * (j % 4) + x % 4


def block_rows(layout, ksteps):
    return {W16: 4 * ksteps, W8: 8 * ksteps, W12: 16 * (ksteps // 3)}[layout]


def _bank(classes, seed):
    rng = np.random.default_rng(seed)
    needles = []
    for n_w, n_h, count in classes:
        for i in range(count):
            nd = rng.integers(0, 256, (n_h, n_w), dtype=np.uint8)
            if i % 5 == 3:
                nd[:] = 77  # a constant needle: dead slot
            needles.append(nd)
    order = rng.permutation(len(needles))
    return PC.bank_of([needles[i] for i in order])


# (classes, column drop) -> per (layout, K-steps): pairable?
BANKS = [
    # LAYOUT_W8: 2 K-steps = 16 rows with 15- and 12-row classes (the benchmark's shape: 9x15 keeps 8 columns), 1 K-step = 8 rows with 7 rows,
    # 3 K-steps = 24 rows with a class that fills them (not pairable)
    ([(8, 15, 19), (9, 15, 17), (5, 12, 3), (8, 7, 5), (4, 6, 2), (8, 24, 4)], True, {(W8, 2): 1, (W8, 1): 1, (W8, 3): 0}),
    # LAYOUT_W12 (16 rows, 3 K-steps): 15, 14 and 9 rows, an 8-wide class riding the 12-byte rows; LAYOUT_W16: 4 K-steps with 15 rows, 3 with 11, 1 with 3
    ([(12, 15, 17), (10, 14, 5), (8, 9, 3), (16, 15, 18), (14, 11, 6), (16, 3, 2)], True, {(W12, 3): 1, (W16, 4): 1, (W16, 3): 1, (W16, 1): 1}),
    # one 16-row class among 15-row ones: the whole pass stays single; W16 at 2 K-steps with 8 rows: single
    ([(8, 15, 6), (8, 16, 3), (16, 8, 4)], True, {(W8, 2): 0, (W16, 2): 0}),
    # every column multiplied: 9 -> 12-byte rows
    ([(9, 15, 17), (13, 15, 6)], False, {(W12, 3): 1, (W16, 4): 1}),
]


def _check(bank, drop, expect):
    supers, q = bank_images(bank, drop)
    info = prefilter_page_model(bank, None, 0.5, drop)
    classes, templates = info["classes"], info["templates"]
    seen = {}
    at = 0
    for si, su in enumerate(supers):
        ks, n_tiles = su["ksteps"], su["n_tiles"]
        size = n_tiles * ks * 1024
        assert su["q_offset"] == at, (si, su, at)  # images lie back to back, in pass order
        seen[(su["layout"], ks)] = su["pairable"]
        rows = block_rows(su["layout"], ks)
        heights = [int(c["n_h"]) for c in classes if int(c["super"]) == si]
        assert heights and su["pairable"] == int(max(heights) <= rows - 1 and 2 * n_tiles <= su["chunk_tiles"]), (si, su, heights)
        img0 = q[at:at + size].reshape(n_tiles, ks, 4, 16, 16)  # [N-tile][K-step][lane group][slot][byte]
        at += size
        if not su["pairable"]:
            continue
        img1 = q[at:at + size].reshape(n_tiles, ks, 4, 16, 16)
        at += size
        want = np.zeros_like(img1)  # the second image, built from the first alone
        live_slots = set()
        for t in range(len(bank)):
            k, slot, live, nt = (int(v) for v in templates[t])
            c = classes[k]
            if int(c["super"]) != si:
                continue
            n_h, kw = int(c["n_h"]), int(c["keep_w"])
            if live:
                live_slots.add((nt, slot % 16))
            for j in range(n_h):
                for x in range(kw):
                    a, g, b = kgroup_of(su["layout"], j, x)
                    a1, g1, b1 = kgroup_of(su["layout"], j + 1, x)
                    assert a1 < ks, (si, j, x)  # row j + 1 is inside the K block
                    want[nt, a1, g1, slot % 16, b1] = img0[nt, a, g, slot % 16, b]
                    if live:  # the first image holds the template the model reads back out of it
                        assert img0[nt, a, g, slot % 16, b] == info["q"][t, j, x], (t, j, x)
        assert np.array_equal(img1, want), f"super-class {si}: the second image is not the first one row lower"
        # sums agree slot by slot (same int8 values, nothing added), and slots without a live template are empty in both images
        assert np.array_equal(img0.astype(np.int64).sum((1, 2, 4)), img1.astype(np.int64).sum((1, 2, 4)))
        assert np.array_equal(np.abs(img0.astype(np.int64)).sum((1, 2, 4)), np.abs(img1.astype(np.int64)).sum((1, 2, 4)))
        for nt in range(n_tiles):
            for s in range(16):
                if (nt, s) not in live_slots:
                    assert not img0[nt, :, :, s].any() and not img1[nt, :, :, s].any(), (si, nt, s)
        assert live_slots and any(img1[nt, :, :, s].any() for nt, s in live_slots)
    assert at == q.size, (at, q.size)
    assert seen == expect, (seen, expect)


def test_second_image_is_the_first_one_row_lower_in_every_layout():
    for i, (classes, drop, expect) in enumerate(BANKS):
        _check(_bank(classes, 100 + i), drop, expect)


def test_a_bank_whose_two_images_do_not_fit_one_launch_keeps_one():
    """37 N-tiles of 2 K-steps fit a launch once (73) but not twice."""
    bank = _bank([(8, 15, 16 * 36 + 1)], 7)
    supers, q = bank_images(bank, True)
    assert len(supers) == 1 and supers[0]["n_tiles"] == 37 and supers[0]["chunk_tiles"] == 73 and not supers[0]["pairable"]
    assert q.size == 37 * 2 * 1024
    bank = _bank([(8, 15, 16 * 36)], 7)  # 36 tiles: 72 <= 73
    supers, q = bank_images(bank, True)
    assert supers[0]["n_tiles"] == 36 and supers[0]["pairable"] and q.size == 2 * 36 * 2 * 1024


def test_the_benchmark_bank_pairs():
    case, bank, _ = PC.build("bench")
    supers, q = bank_images(bank, True)
    assert len(supers) == 1 and supers[0] == dict(layout=W8, ksteps=2, n_tiles=4, pairable=1, q_offset=0, chunk_tiles=73), supers

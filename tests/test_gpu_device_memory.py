"""Every device allocation of the library has one owner (csrc/hip/devmem.h), and focr_debug_device_bytes counts what the
owners hold.  Each test reads the count, drives one kind of object through the paths that allocate — every tail of the scan,
a replaced bank, a change of page geometry, the decoder's verify and test images, an executor's two page sets per context —
closes it, and reads the count again: whatever the object held is gone, whichever buffers a later change adds.  Only
differences are compared, so objects other tests keep alive do not matter.

Not asserted on: the state of the compat symbols (ncc_8_u8 / ncc_16_u8) is per thread and deliberately stays live, and
counted, past its thread's end (compat.hip); nothing here calls them.  Page-locked host memory is not device memory."""
import os

import numpy as np
import pytest

import focr_line_model as M
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineDecoder, _native as N, synth_pages
from font_ocr_amd.searcher import SCAN_DIRECT, SCAN_MFMA, Fleet, PinnedPages, Pipeline, Scanner

pytestmark = pytest.mark.gpu

MONO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "DejaVuSansMono.ttf")
INK = "".join(c for c in FOCR_DEFAULT_ALPHABET if not c.isspace())


def _live():
    return int(N.hip().focr_debug_device_bytes())


def test_scanner_gives_back_every_byte(bank_x2):
    before = _live()
    s = Scanner(0)
    created = _live()
    assert created > before  # the counters and the result block
    s.set_bank(bank_x2)
    s.set_pages(synth_pages(bank_x2, 3, 256, 96, first=4100))
    s.scan(0.8, 1024, SCAN_MFMA)  # hits-first tail, exact sizes
    s.scan(0.8, 1024, SCAN_MFMA)  # ... on size estimates
    s.process_hits(0.95, 5)
    assert s.total_chars() > 0
    with_tail = _live()
    s.set_row_tail(0)  # the legacy tail: the second candidate list, flags and positions
    s.scan(0.8, 1024, SCAN_MFMA)
    assert s.counts().sum() > 0 and _live() > with_tail
    s.set_row_tail(1)
    s.force_split(True)  # page sub-ranges, results appended
    s.scan(0.8, 1024, SCAN_MFMA)
    s.process_hits(0.95, 5)
    s.lines()
    s.force_split(False)
    s.scan(0.8, 1024, SCAN_DIRECT)
    s.process_hits(0.95, 5)
    held = _live()
    s.set_bank(bank_x2.subset(list(range(33, 95))))  # the old bank's arrays go, the new one's come
    assert _live() < held
    s.scan(0.8, 1024, SCAN_MFMA)
    s.set_pages(synth_pages(bank_x2, 2, 200, 80, first=4200))  # another geometry: a new page set replaces the old
    s.scan(0.8, 1024, SCAN_MFMA)
    s.process_hits(0.95, 5)
    assert _live() > created
    s.close()
    assert _live() == before


def test_line_decoder_gives_back_every_byte():
    rng = np.random.default_rng(7)
    pages = [M.synth_page(rng, MONO, 13.0, INK, W, H, 3, 2, 15, max(1, (H - 2) // 15), blank_every=2)[0] for W, H in ((150, 62), (150, 62), (110, 47))]
    before = _live()
    dec = LineDecoder(0)
    dec.set_font(MONO, 13.0)
    lines, mse, images = dec.decode(pages, 3, 2, 120, 13, 15, verify="image")
    assert sum(len(l) for l in lines) > 0 and images[0].shape == (62, 150, 3)
    rects, texts = dec.test_images(pages, 3, 2, 120, 13, 15)
    assert rects[0].shape == (62, 150, 4) and texts[2].shape == (47, 110, 4)
    bg = rng.integers(0, 256, (1000, 4), dtype=np.uint8)
    dec.debug_blend(bg, bg[::-1].copy())  # its temporary is gone when the call returns
    dec.set_font(MONO, 11.0)  # a replaced font
    dec.decode(pages[:2], 3, 2, 120, 11, 13, verify="mse")
    assert _live() > before
    dec.close()
    assert _live() == before


def _pinned_batches(bank, n_batches, first):
    pins = []
    for b in range(n_batches):
        pin = PinnedPages(2, 96, 288)
        pin.array[:] = synth_pages(bank, 2, 288, 96, first=first + 2 * b)
        pins.append(pin)
    return pins


def test_pipeline_gives_back_every_byte(bank_x2):
    """Announced batches are ingested into a context's alternate page set, which then becomes its current one: after two
    such batches a context owns two sets, and the third re-uses the first.  Three per context here."""
    before = _live()
    pipe = Pipeline(0, 2)
    pins = _pinned_batches(bank_x2, 3 * len(pipe.scanners), 4300)
    try:
        pipe.set_bank(bank_x2)
        held = []
        for pin in pins:
            pipe.prefetch(pin.array)
            t = pipe.submit(pin.array, 0.8)
            assert len(pipe.wait(t).lines_flat()) > 0
            pipe.release(t)
            held.append(_live())
        n = len(pipe.scanners)
        assert held[2 * n - 1] > held[n - 1] > before  # the second round of the ring allocated every context's second set
    finally:
        pipe.close()
        for pin in pins:
            pin.close()
    assert _live() == before


def test_fleet_gives_back_every_byte(bank_x2):
    if N.hip().focr_device_count() < 2:
        pytest.skip("one device visible: the fleet's contexts are the executor's of test_pipeline_gives_back_every_byte")
    before = _live()
    fl = Fleet(None, lanes=2)
    pins = _pinned_batches(bank_x2, 3 * fl.slots, 4400)
    try:
        fl.set_bank(bank_x2)
        for pin in pins:
            t = fl.submit(pin.array, 0.8)
            assert len(fl.wait(t).lines_flat()) > 0
            fl.release(t)
        assert _live() > before
    finally:
        fl.close()
        for pin in pins:
            pin.close()
    assert _live() == before

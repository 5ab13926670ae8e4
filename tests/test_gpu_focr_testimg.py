"""focr --test on the device (focr_decoder_test_images) against the model (tests/focr_testimg_model.py), byte for byte:
the blend exhaustively through the debug entry, the line boxes over the geometry that changes their blend counts and
clipping, the alphabet canvas with both fonts and hinting, batches, device memory, the last run left untouched,
refusals, the launch count, and the `focr --test` CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_line_model as M
import focr_testimg_model as T
from focr_fast_model import ALPHABET_319
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineDecoder, load_image, load_image_rgba, save_pgm
from font_ocr_amd.decoder import DecoderError, render_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
INK = "".join(c for c in FOCR_DEFAULT_ALPHABET if not c.isspace())

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def _page(seed, W, H, font=MONO, size=13.0, adv=15, n_lines=None, blank_every=2, x=3, y=2):
    rng = np.random.default_rng(seed)
    n = n_lines if n_lines is not None else max(1, (H - y) // adv)
    page, _ = M.synth_page(rng, font, size, INK, W, H, x, y, adv, n, blank_every=blank_every)
    return page


def _check(dec, pages, geo, rgba=None, font=MONO, size=13.0, alphabet=FOCR_DEFAULT_ALPHABET, hinting=False, kerning=1.0):
    rects, texts = dec.test_images(pages, *geo, rgba=rgba)
    canvas = render_text(font, size, alphabet, kerning, hinting)
    for i, p in enumerate(pages):
        base = T.grey_rgba(p) if rgba is None else rgba[i]
        want_r = T.draw_test_rectangles(p, *geo, rgba=base)
        want_t = T.draw_test_text(canvas, base)
        assert rects[i].shape == p.shape + (4,) and rects[i].dtype == np.uint8
        assert np.array_equal(rects[i], want_r), (i, np.argwhere(np.any(rects[i] != want_r, axis=-1))[:5])
        assert np.array_equal(texts[i], want_t), (i, np.argwhere(np.any(texts[i] != want_t, axis=-1))[:5])
    assert dec._lib.focr_decoder_last_test_launches(dec._h) == 3
    return rects, texts


def test_blend_exhaustive(dec):
    """Every (bg channel, bg alpha, fg red) triple with the drawings' fg alpha 128, then random pixels of any fg alpha."""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    bg = np.stack([c, c, c, a], axis=-1).reshape(-1, 4)
    for r in range(0, 256, 64):  # 64 fg reds per call
        bgs = np.tile(bg, (64, 1))
        fg = np.zeros_like(bgs)
        fg[:, 0] = np.repeat(np.arange(r, r + 64, dtype=np.uint8), len(bg))
        fg[:, 3] = 128
        got = dec.debug_blend(bgs, fg)
        want = T.blend(bgs, fg)
        assert np.array_equal(got, want), np.argwhere(np.any(got != want, axis=-1))[:5]
    rng = np.random.default_rng(11)
    bg = rng.integers(0, 256, (1 << 20, 4), dtype=np.uint8)
    fg = rng.integers(0, 256, (1 << 20, 4), dtype=np.uint8)
    fg[::7, 3] = 0
    fg[1::7, 3] = 255
    bg[2::7, 3] = 0
    assert np.array_equal(dec.debug_blend(bg, fg), T.blend(bg, fg))


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
def test_default_geometry_batch_two_sizes(dec, font, hinting):
    """Several pages of two sizes, blank slots skipped, the text canvas at the top-left corner."""
    pages = [_page(1, 150, 62, font), _page(2, 150, 62, font, blank_every=3), _page(3, 110, 47, font), _page(4, 150, 62, font)]
    dec.set_font(font, 13.0, FOCR_DEFAULT_ALPHABET, hinting)
    _check(dec, pages, (3, 2, 120, 13, 15), font=font, hinting=hinting)


@pytest.mark.parametrize("lh,adv", [(12, 5), (12, 12), (9, 3), (7, 2)])
def test_overlapping_boxes(dec, lh, adv):
    """line_advance <= line_height: boxes share rows, and pixels take four or more blends."""
    pages = [_page(5, 90, 40, adv=8, blank_every=0), _page(6, 90, 40, adv=8, blank_every=2)]
    dec.set_font(MONO, 13.0)
    _check(dec, pages, (4, 1, 60, lh, adv))
    assert T.rect_counts(pages[0], 4, 1, 60, lh, adv).max() >= 4


def test_every_pixel_on_an_edge(dec):
    """line_height = line_advance = 1 and nothing blank, over a base of all 65 536 (colour, alpha) pairs."""
    W = H = 256
    rng = np.random.default_rng(9)
    page = rng.integers(0, 255, (H, W), dtype=np.uint8)  # no 255 anywhere: every one-row crop has ink
    x, yy = np.meshgrid(np.arange(W, dtype=np.uint8), np.arange(H, dtype=np.uint8))
    base = np.stack([x, 255 - x, x // 3, yy], axis=-1).astype(np.uint8)
    assert T.rect_counts(page, 0, 0, W - 1, 1, 1).min() >= 1
    dec.set_font(MONO, 13.0)
    _check(dec, [page], (0, 0, W - 1, 1, 1), rgba=[base])


@pytest.mark.parametrize("geo", [(100, 2, 80, 13, 15), (3, 2, 120, 70, 15), (3, 30, 500, 40, 9), (150, 0, 10, 12, 15),
                                 (200, 0, 10, 12, 15), (3, 2, 1, 13, 15), (0, 0, 0, 13, 15), (3, 62, 50, 13, 15), (3, 2, 50, 0, 15)],
                         ids=["right", "bottom", "both", "x_eq_w", "x_past_w", "width1", "width0", "y_past_h", "height0"])
def test_clipping_and_thin_geometry(dec, geo):
    """Boxes clipped at the right and bottom edges, x_start >= W (every crop empty, no box), width 1 and 0."""
    pages = [_page(7, 150, 62), _page(8, 150, 62)]
    dec.set_font(MONO, 13.0)
    rects, _ = _check(dec, pages, geo)
    if geo[0] >= 150 or geo[1] >= 62 or geo[3] == 0 or geo[2] == 0:
        assert all(np.array_equal(r, T.grey_rgba(p)) for r, p in zip(rects, pages))


@pytest.mark.parametrize("W", [256, 257, 513])
def test_tile_boundaries(dec, W):
    """The compose tile is 16 rows by 256 columns: 17 rows make a second tile row one row high, 257 and 513 columns a
    last tile column one column wide.  Boxes of height 5 every 5 rows from y = 1 put a bottom edge and a top edge on
    row 16 and vertical edges across rows 15 / 16; the right edge is the page's last column; the 24 px alphabet canvas
    crosses every seam.  Both images at once, then each alone."""
    H, size, geo = 17, 24.0, (2, 1, W - 3, 5, 5)
    rng = np.random.default_rng(27)
    pages = [rng.integers(0, 255, (H, W), dtype=np.uint8) for _ in range(2)]
    pages[1][6:11] = 255  # the second slot of the second page is blank
    canvas = render_text(MONO, size, FOCR_DEFAULT_ALPHABET)
    want_r = [T.draw_test_rectangles(p, *geo) for p in pages]
    want_t = [T.draw_test_text(canvas, T.grey_rgba(p)) for p in pages]
    last = (W - 1) // 256 * 256  # first column of the last tile column
    for p, r, t in zip(pages, want_r, want_t):  # the expectation itself reaches the second tile row and the last tile column
        for img in (r, t):
            changed = np.any(img != T.grey_rgba(p), axis=-1)
            assert changed[16].any() and changed[:16].any() and changed[:, last:].any()
    assert T.rect_counts(pages[0], *geo)[8, 2] == 1 and T.rect_counts(pages[1], *geo)[8, 2] == 0  # row 8 is the second box's alone
    dec.set_font(MONO, size)
    lib, h = dec._lib, dec._h
    for rect, text, launches in ((True, True, 3), (True, False, 2), (False, True, 2)):
        rects, texts = dec.test_images(pages, *geo, rect=rect, text=text)
        assert lib.focr_decoder_last_test_launches(h) == launches
        assert (rects is None) == (not rect) and (texts is None) == (not text)
        for i in range(2):
            if rect:
                assert np.array_equal(rects[i], want_r[i]), (i, np.argwhere(np.any(rects[i] != want_r[i], axis=-1))[:5])
            if text:
                assert np.array_equal(texts[i], want_t[i]), (i, np.argwhere(np.any(texts[i] != want_t[i], axis=-1))[:5])


@pytest.mark.parametrize("alphabet,font,size", [(FOCR_DEFAULT_ALPHABET, MONO, 24.0), (ALPHABET_319, SANS, 13.0),
                                                (ALPHABET_319, MONO, 20.0)], ids=["default24", "319sans", "319mono"])
def test_alphabet_larger_than_the_page(dec, alphabet, font, size):
    """The alphabet canvas is wider and taller than the page; 319 glyphs run past the decode line cap."""
    canvas = render_text(font, size, alphabet)
    page = _page(10, 140, canvas.shape[0] - 3, font, 13.0, adv=15, n_lines=1)
    assert canvas.shape[0] > page.shape[0] and canvas.shape[1] > page.shape[1]
    dec.set_font(font, size, alphabet)
    _check(dec, [page], (3, 2, 100, 14, 15), font=font, size=size, alphabet=alphabet)
    big = _page(12, canvas.shape[1] + 40, canvas.shape[0] + 20, font, 13.0)  # and a page larger than the canvas
    _check(dec, [big], (3, 2, 300, 14, 15), font=font, size=size, alphabet=alphabet)


def test_kerning_and_colour_base(dec):
    """A colour RGBA base with varying alpha (transparent pixels included) and kerning != 1."""
    pages = [_page(13, 150, 62, SANS), _page(14, 150, 62, SANS)]
    rng = np.random.default_rng(15)
    rgba = [rng.integers(0, 256, p.shape + (4,), dtype=np.uint8) for p in pages]
    rgba[0][::3, :, 3] = 0
    dec.set_font(SANS, 13.0, FOCR_DEFAULT_ALPHABET, True, 1.07)
    _check(dec, pages, (3, 2, 120, 13, 15), rgba=rgba, font=SANS, hinting=True, kerning=1.07)


def test_device_memory(dec):
    pages = np.ascontiguousarray(np.stack([_page(16, 150, 62), _page(17, 150, 62)]))
    rng = np.random.default_rng(18)
    rgba = rng.integers(0, 256, pages.shape + (4,), dtype=np.uint8)
    geo = (3, 2, 120, 13, 15)
    dec.set_font(MONO, 13.0)
    want_r, want_t = dec.test_images(pages, *geo, rgba=list(rgba))
    assert np.array_equal(want_r[1], T.draw_test_rectangles(pages[1], *geo, rgba=rgba[1]))
    hip = C.CDLL("libamdhip64.so.7")
    bufs = [C.c_void_p() for _ in range(4)]
    sizes = [pages.nbytes, rgba.nbytes, rgba.nbytes, rgba.nbytes]
    try:
        for b, n in zip(bufs, sizes):
            assert hip.hipMalloc(C.byref(b), C.c_size_t(n)) == 0
        assert hip.hipMemcpy(bufs[0], C.c_void_p(pages.ctypes.data), C.c_size_t(pages.nbytes), 1) == 0
        assert hip.hipMemcpy(bufs[1], C.c_void_p(rgba.ctypes.data), C.c_size_t(rgba.nbytes), 1) == 0
        assert hip.hipDeviceSynchronize() == 0
        dec.test_images_device(bufs[0].value, 2, 62, 150, *geo, rgba_ptr=bufs[1].value, rect_ptr=bufs[2].value, text_ptr=bufs[3].value)
        for b, want in ((bufs[2], want_r), (bufs[3], want_t)):
            out = np.empty_like(rgba)
            assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), b, C.c_size_t(out.nbytes), 2) == 0
            assert np.array_equal(out, np.stack(want))
        with pytest.raises(DecoderError, match="aligned"):
            dec.test_images_device(bufs[0].value, 2, 62, 150, *geo, rect_ptr=bufs[2].value + 1)
    finally:
        for b in bufs:
            if b.value:
                hip.hipFree(b)


def test_last_run_unchanged(dec):
    """A test_images call between a decode and its verify changes neither: lines, last_ms and the verify images."""
    font, size = SANS, 13.0
    pages = [_page(19, 150, 62, font), _page(20, 150, 62, font)]
    dec.set_font(font, size)
    lines, mse, images = dec.decode(pages, 1, 2, 200, 13, 15, verify="image")
    lib, h = dec._lib, dec._h
    ms, n_lines, n_chars = lib.focr_decoder_last_ms(h), lib.focr_decoder_n_lines(h), lib.focr_decoder_n_chars(h)
    other = [_page(21, 120, 50, font), _page(22, 120, 50, font)]
    dec.test_images(other, 0, 0, 100, 12, 5)
    assert lib.focr_decoder_last_ms(h) == ms and lib.focr_decoder_n_lines(h) == n_lines and lib.focr_decoder_n_chars(h) == n_chars
    assert lib.focr_decoder_last_launches(h) == 3
    sums, again = dec.verify()
    assert all(np.array_equal(a, b) for a, b in zip(again, images))
    assert (sums.astype(np.float32) / np.float32(150 * 62)).tobytes() == mse.tobytes()
    assert dec.decode(pages, 1, 2, 200, 13, 15) == lines


def test_refusals_and_launch_count(dec):
    lib, h = dec._lib, dec._h
    page = _page(23, 80, 30)
    out = np.empty(page.shape + (4,), np.uint8)
    dec.set_font(MONO, 13.0)  # drops the verify table
    args = (C.c_void_p(page.ctypes.data), None, 0, 1, 80, 30, 0, 0, 80, 12, 15)
    assert lib.focr_decoder_test_images(h, *args, None, C.c_void_p(out.ctypes.data), 0) != 0
    assert b"verify table" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_test_images(h, *args, C.c_void_p(out.ctypes.data), None, 0) == 0  # the boxes need no table
    assert lib.focr_decoder_last_test_launches(h) == 2
    assert np.array_equal(out, T.draw_test_rectangles(page, 0, 0, 80, 12, 15))
    with pytest.raises(DecoderError, match="line_advance 0"):
        dec.test_images([page], 0, 0, 80, 12, 0)
    # the count is the same for one slot and for hundreds
    for geo in ((0, 0, 80, 12, 15), (0, 0, 80, 1, 1), (0, 29, 80, 12, 15), (0, 40, 80, 12, 15)):
        dec.test_images([page] * 3, *geo)
        assert lib.focr_decoder_last_test_launches(h) == 3, geo
        assert dec.last_test_ms > 0
    rects, texts = dec.test_images([page], 0, 0, 80, 12, 15, rect=False)
    assert rects is None and lib.focr_decoder_last_test_launches(h) == 2


def _png_rgba_header(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    return data[24], data[25]  # bit depth, colour type


def test_cli_test(tmp_path):
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    from PIL import Image

    font, size = SANS, 13.0
    a, b = _page(24, 150, 62, font), _page(25, 110, 47, font)
    pa, pb = str(tmp_path / "a.pgm"), str(tmp_path / "b.pgm")
    save_pgm(pa, a)
    save_pgm(pb, b)
    geo = ["-x", "3", "-y", "2", "-w", "120", "--line-height", "13", "--line-advance", "15"]
    cmd = [FOCR, "-f", font, "-t", str(size), "--hinting"] + geo
    r = subprocess.run(cmd + ["--test", str(tmp_path / "P"), "-i", pa, pb], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ""
    canvas = render_text(font, size, FOCR_DEFAULT_ALPHABET, 1.0, True)
    want = {"rect": T.draw_test_rectangles(a, 3, 2, 120, 13, 15), "text": T.draw_test_text(canvas, T.grey_rgba(a))}
    for kind, img in want.items():  # the first -i image only
        path = str(tmp_path / f"P-{kind}.png")
        assert _png_rgba_header(path) == (8, 6)
        assert np.array_equal(load_image_rgba(path), img)  # the RGBA writer round-trips through the loader
        assert np.array_equal(np.asarray(Image.open(path).convert("RGBA")), img)

    # a colour source keeps its colour; its luma decides the blank slots
    rng = np.random.default_rng(26)
    col = rng.integers(0, 256, (40, 90, 4), dtype=np.uint8)
    col[::2] = 255
    pc = str(tmp_path / "c.png")
    Image.fromarray(col, "RGBA").save(pc)
    r = subprocess.run([FOCR, "-f", font, "-t", str(size), "-x", "2", "-y", "1", "-w", "50", "--line-height", "3",
                        "--line-advance", "4", "--test", str(tmp_path / "C"), "-i", pc], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    base, luma = load_image_rgba(pc), load_image(pc)
    assert np.array_equal(base, col)
    assert np.array_equal(load_image_rgba(str(tmp_path / "C-rect.png")), T.draw_test_rectangles(luma, 2, 1, 50, 3, 4, base))
    assert np.array_equal(load_image_rgba(str(tmp_path / "C-text.png")),
                          T.draw_test_text(render_text(font, size, FOCR_DEFAULT_ALPHABET), base))

    # the --verify directory check still comes first
    r = subprocess.run(cmd + ["--verify", str(tmp_path / "nodir"), "--test", str(tmp_path / "Q"), "-i", pa], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--verify should be a dir" in r.stderr
    assert not os.path.exists(tmp_path / "Q-rect.png") and not os.path.exists(tmp_path / "Q-text.png")

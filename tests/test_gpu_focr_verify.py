"""focr --verify on the device (focr_decoder_verify) against the model's draw_verify (tests/focr_line_model.py) on the
device's own decoded lines: images byte for byte and MSE as f32, over the decoder's test grid and awkward geometry;
device-memory pages and images; refusals; and the `focr --verify` CLI."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import focr_line_model as M
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineDecoder, VerifyFont, save_pgm
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
ASCII95 = "".join(chr(c) for c in range(32, 127))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def _ink(alphabet):
    return "".join(c for c in alphabet if not c.isspace())


def _pages(font, size, alphabet, kerning, hinting, seed):
    """As tests/test_gpu_focr.py: pages of two sizes, blank lines, a partial last line, one page with noise."""
    adv = int(size * 1.2) + 2
    lh = int(size) + 2
    rng = np.random.default_rng(seed)
    a, _ = M.synth_page(rng, font, size, _ink(alphabet), 150, 3 * adv + lh // 2 + 3, 3, 2, adv, 4, kerning, hinting, blank_every=2)
    b, _ = M.synth_page(rng, font, size, _ink(alphabet), 150, 3 * adv + lh // 2 + 3, 3, 2, adv, 4, kerning, hinting, noise=20)
    c, _ = M.synth_page(rng, font, size, _ink(alphabet), 110, 2 * adv + 4, 3, 2, adv, 3, kerning, hinting)
    return [a, b, c], adv, lh


def _check(pages, got, mse, images, font, size, x, kerning=1.0, hinting=False):
    """The model's verify image and MSE of each page's decoded lines."""
    assert mse.dtype == np.float32 and len(mse) == len(pages)
    for i, (p, lines) in enumerate(zip(pages, got)):
        img, m = M.verify_image(p, lines, font, size, x, kerning, hinting)
        if images is not None:
            assert images[i].shape == img.shape and images[i].dtype == np.uint8
            assert np.array_equal(images[i], img), i
        assert mse[i].tobytes() == np.float32(m).tobytes(), (i, mse[i], m)


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("kerning", [1.0, 1.07])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
@pytest.mark.parametrize("size", [13.0, 24.0])
@pytest.mark.parametrize("alphabet", [FOCR_DEFAULT_ALPHABET, ASCII95], ids=["default", "ascii95"])
def test_verify_equals_model(dec, font, kerning, hinting, size, alphabet):
    seed = zlib.crc32(repr((os.path.basename(font), kerning, hinting, size, len(alphabet))).encode())
    pages, adv, lh = _pages(font, size, alphabet, kerning, hinting, seed)
    dec.set_font(font, size, alphabet, hinting, kerning)
    geo = (1, 2, 200, lh, adv)  # the rendered text runs past the right edge of every page
    plain = dec.decode(pages, *geo)
    got, mse, images = dec.decode(pages, *geo, verify="image")
    assert got == plain and any(got)
    _check(pages, got, mse, images, font, size, geo[0], kerning, hinting)
    assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    got2, mse2, none = dec.decode(pages, *geo, verify="mse")
    assert got2 == got and none is None and mse2.tobytes() == mse.tobytes()


def test_verify_geometry_edges(dec):
    """Text clipped at the right and bottom edges, overlapping canvases, thin crops, lines past the page."""
    font, size = SANS, 13.0
    pages, adv, lh = _pages(font, size, FOCR_DEFAULT_ALPHABET, 1.0, False, 11)
    dec.set_font(font, size)
    for geo in [(0, 0, 60, lh, adv), (120, 2, 40, lh, adv), (5, 7, 90, lh + 5, adv), (2, 0, 200, 3, 4),
                (1, 2, 200, lh, 6),      # line_advance well below the canvas height: neighbouring canvases overlap
                (1, 30, 200, lh, adv)]:  # the last line's canvas runs past the bottom of the page
        got, mse, images = dec.decode(pages, *geo, verify="image")
        _check(pages, got, mse, images, font, size, geo[0])


@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
def test_negative_left_bounds(dec, hinting):
    """DejaVu Sans J, T, Y and j reach left of the pen: their lines' canvases start at bounds.ox < 0."""
    font, size = SANS, 24.0
    W, H, adv, lh = 220, 120, 28, 26
    rng = np.random.default_rng(4)
    page = np.full((H, W), 255, dtype=np.uint8)
    for i, first in enumerate("JTYj"):
        text = first + "".join(rng.choice(list(_ink(FOCR_DEFAULT_ALPHABET)), 8))
        c = M.render_text(font, size, text, 1.0, hinting)
        ly = 2 + i * adv
        hh, ww = min(c.shape[0], H - ly), min(c.shape[1], W - 4)
        page[ly: ly + hh, 4: 4 + ww] = np.minimum(page[ly: ly + hh, 4: 4 + ww], 255 - c[:hh, :ww])
    dec.set_font(font, size, FOCR_DEFAULT_ALPHABET, hinting)
    got, mse, images = dec.decode(page, 4, 2, 200, lh, adv, verify="image")
    assert any(M.glyph_metrics(font, size, t[0])[2][0] < 0 for _, t in got[0])  # some line's canvas starts left of 0
    _check([page], got, mse, images, font, size, 4, 1.0, hinting)


def test_blank_batch_is_red_only(dec):
    font, size = MONO, 13.0
    dec.set_font(font, size)
    pages = [np.full((40, 90), 255, dtype=np.uint8), np.full((40, 90), 255, dtype=np.uint8)]
    pages[1][3, 5] = 10  # ink outside every crop
    got, mse, images = dec.decode(pages, 20, 10, 50, 12, 15, verify="image")
    assert got == [[], []]
    _check(pages, got, mse, images, font, size, 20)
    assert not images[0].any() and images[1][3, 5, 0] == 10
    # no line slot at all (y past the page): nothing decoded, the pages are still drawn
    got, mse, images = dec.decode(pages, 0, 500, 50, 12, 15, verify="image")
    assert got == [[], []] and dec._lib.focr_decoder_last_launches(dec._h) == 0
    _check(pages, got, mse, images, font, size, 0)


def test_device_pages_and_device_images(dec):
    pages, adv, lh = _pages(MONO, 13.0, FOCR_DEFAULT_ALPHABET, 1.07, False, 3)
    batch = np.ascontiguousarray(np.stack([pages[0], pages[1]]))
    geo = (1, 2, 200, lh, adv)
    dec.set_font(MONO, 13.0, FOCR_DEFAULT_ALPHABET, False, 1.07)
    want_lines, want_mse, want_images = dec.decode(batch, *geo, verify="image")
    hip = C.CDLL("libamdhip64.so.7")
    src, dst = C.c_void_p(), C.c_void_p()
    nbytes = batch.nbytes * 3
    assert hip.hipMalloc(C.byref(src), C.c_size_t(batch.nbytes)) == 0
    try:
        assert hip.hipMalloc(C.byref(dst), C.c_size_t(nbytes)) == 0
        try:
            assert hip.hipMemcpy(src, C.c_void_p(batch.ctypes.data), C.c_size_t(batch.nbytes), 1) == 0  # host to device
            assert hip.hipDeviceSynchronize() == 0
            lines, mse, images = dec.decode_device(src.value, *batch.shape, *geo, verify="image")
            assert lines == want_lines and mse.tobytes() == want_mse.tobytes()
            assert all(np.array_equal(a, b) for a, b in zip(images, want_images))
            sums, none = dec.verify(rgb_device=dst.value)
            assert none is None
            out = np.empty((2,) + batch.shape[1:] + (3,), dtype=np.uint8)
            assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), dst, C.c_size_t(nbytes), 2) == 0  # device to host
            assert np.array_equal(out, np.stack(want_images))
            assert (sums.astype(np.float32) / np.float32(batch.shape[1] * batch.shape[2])).tobytes() == want_mse.tobytes()
        finally:
            hip.hipFree(dst)
    finally:
        hip.hipFree(src)


def test_refusals(dec):
    lib, h = dec._lib, dec._h
    sums = np.zeros(4, dtype=np.uint64)
    dec.set_font(MONO, 13.0)
    # no run since the font was set
    assert lib.focr_decoder_verify(h, None, 0, sums.ctypes.data) != 0
    assert b"no successful" in lib.focr_decoder_last_error(h)
    with pytest.raises(DecoderError, match="no decode"):
        dec.verify()
    page = np.full((30, 80), 255, dtype=np.uint8)
    page[5:9, 5:20] = 0
    dec.decode(page, 0, 0, 80, 12, 15)
    # no verify table (the set_font above dropped it)
    assert lib.focr_decoder_verify(h, None, 0, sums.ctypes.data) != 0
    assert b"no verify table" in lib.focr_decoder_last_error(h)
    # mismatched tables: other size, kerning, hinting, alphabet
    for args in [(MONO, 14.0, FOCR_DEFAULT_ALPHABET, False, 1.0), (MONO, 13.0, FOCR_DEFAULT_ALPHABET, False, 1.07),
                 (MONO, 13.0, FOCR_DEFAULT_ALPHABET, True, 1.0), (MONO, 13.0, FOCR_DEFAULT_ALPHABET[::-1], False, 1.0),
                 (MONO, 13.0, FOCR_DEFAULT_ALPHABET[:-1], False, 1.0)]:
        vf = VerifyFont(*args)
        assert lib.focr_decoder_set_verify_font(h, C.byref(vf.s)) != 0, args
        assert b"does not match" in lib.focr_decoder_last_error(h)
        vf.close()
    # increments that differ in one bit
    vf = VerifyFont(MONO, 13.0)
    vf.s.glyphs[3].increment = np.nextafter(np.float32(vf.s.glyphs[3].increment), np.float32(100))
    assert lib.focr_decoder_set_verify_font(h, C.byref(vf.s)) != 0
    assert b"increments" in lib.focr_decoder_last_error(h)
    vf.close()
    # a failed run leaves nothing to verify
    with pytest.raises(DecoderError):
        dec.decode(page, 0, 0, 80, 12, 0)  # line_advance 0 is refused
    assert lib.focr_decoder_verify(h, None, 0, sums.ctypes.data) != 0


def test_second_run_then_verify(dec):
    """verify always draws the last run, whatever ran before it, also with another geometry and page size."""
    font, size = SANS, 13.0
    pages, adv, lh = _pages(font, size, FOCR_DEFAULT_ALPHABET, 1.0, False, 17)
    dec.set_font(font, size)
    dec.decode(pages[:2], 1, 2, 200, lh, adv, verify="image")
    got = dec.decode([pages[2]], 3, 1, 100, lh, adv)
    sums, images = dec.verify()
    img, m = M.verify_image(pages[2], got[0], font, size, 3)
    assert np.array_equal(images[0], img)
    assert np.float32(np.float32(sums[0]) / np.float32(pages[2].size)) == m
    assert dec.last_verify_ms > 0


def test_cli_verify(tmp_path):
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    from PIL import Image

    font, size, kern = SANS, 13.0, 1.07
    rng = np.random.default_rng(8)
    pages = []
    for i in range(40):  # three sizes, interleaved
        W, H = [(150, 60), (110, 45), (180, 75)][i % 3]
        p, _ = M.synth_page(rng, font, size, _ink(FOCR_DEFAULT_ALPHABET), W, H, 1, 2, 17, H // 17, kern, False,
                            blank_every=3 if i % 4 == 0 else 0)
        pages.append(p)
    paths = []
    for i, p in enumerate(pages):
        paths.append(str(tmp_path / f"p{i:02d}.pgm"))
        save_pgm(paths[-1], p)
    vdir = tmp_path / "verify"
    vdir.mkdir()
    base = [FOCR, "-f", font, "-t", str(size), "-k", str(kern), "-x", "1", "-y", "2", "-w", "200", "--line-height", "15",
            "--line-advance", "17"]
    r = subprocess.run(base + ["--verify", str(vdir), "-i"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run(base + ["-i"] + paths, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and plain.stderr == ""
    assert r.stdout == plain.stdout
    with LineDecoder(0) as d:
        d.set_font(font, size, FOCR_DEFAULT_ALPHABET, False, kern)
        lines = d.decode(pages, 1, 2, 200, 15, 17)
    assert r.stdout == "".join(t + "\n" for pg in lines for _, t in pg)
    want_err = {}
    for path, p, ls in zip(paths, pages, lines):
        img, mse = M.verify_image(p, ls, font, size, 1, kern, False)
        got = np.asarray(Image.open(str(vdir / (os.path.splitext(os.path.basename(path))[0] + ".png"))).convert("RGB"))
        assert np.array_equal(got, img), path
        want_err[path] = f"{path} {float(mse):.6f}"
    # the reference's order: size groups (W, H ascending), pages of a group in -i order
    order = sorted(range(len(pages)), key=lambda i: (pages[i].shape[1], pages[i].shape[0], i))
    assert r.stderr.splitlines() == [want_err[paths[i]] for i in order]

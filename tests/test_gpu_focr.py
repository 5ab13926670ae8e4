"""The focr line decoder on the device against the brute-force model of the reference (tests/focr_line_model.py):
list for list over fonts, kernings, hinting, sizes, alphabets and awkward geometry; ties; truth on clean pages; pages
given in device memory; and the `focr` CLI end to end."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import focr_line_model as M
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineDecoder, save_pgm

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
    """Pages of two sizes: blank lines in between, a partial last line, one with noise (near-ties)."""
    adv = int(size * 1.2) + 2
    lh = int(size) + 2
    rng = np.random.default_rng(seed)
    a, _ = M.synth_page(rng, font, size, _ink(alphabet), 150, 3 * adv + lh // 2 + 3, 3, 2, adv, 4, kerning, hinting, blank_every=2)
    b, _ = M.synth_page(rng, font, size, _ink(alphabet), 150, 3 * adv + lh // 2 + 3, 3, 2, adv, 4, kerning, hinting, noise=20)
    c, _ = M.synth_page(rng, font, size, _ink(alphabet), 110, 2 * adv + 4, 3, 2, adv, 3, kerning, hinting)
    return [a, b, c], adv, lh


def _model(pages, font, size, alphabet, geo, kerning, hinting):
    return [M.decode_image(p, font, size, alphabet, *geo, kerning, hinting) for p in pages]


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("kerning", [1.0, 1.07])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
@pytest.mark.parametrize("size", [13.0, 24.0])
@pytest.mark.parametrize("alphabet", [FOCR_DEFAULT_ALPHABET, ASCII95], ids=["default", "ascii95"])
def test_decoder_equals_model(dec, font, kerning, hinting, size, alphabet):
    seed = zlib.crc32(repr((os.path.basename(font), kerning, hinting, size, len(alphabet))).encode())
    pages, adv, lh = _pages(font, size, alphabet, kerning, hinting, seed)
    dec.set_font(font, size, alphabet, hinting, kerning)
    # x + width past the page edge (widths 150 and 110, both clipped)
    geo = (1, 2, 200, lh, adv)
    got = dec.decode(pages, *geo)
    want = _model(pages, font, size, alphabet, geo, kerning, hinting)
    assert got == want
    assert any(got) and all(isinstance(t, str) for pg in got for _, t in pg)


def test_decoder_geometry_edges(dec):
    font, size = SANS, 13.0
    pages, adv, lh = _pages(font, size, FOCR_DEFAULT_ALPHABET, 1.0, False, 11)
    dec.set_font(font, size)
    for geo in [(0, 0, 60, lh, adv),       # narrow crop, lines not aligned to the text
                (150, 2, 40, lh, adv),     # x_start >= W for the 150-px pages: empty crops count as blank
                (500, 2, 40, lh, adv),     # x_start >= W for every page
                (5, 7, 90, lh + 5, adv),   # tall crops that overlap the next line
                (2, 0, 200, 3, 4)]:        # thin crops every 4 rows
        assert dec.decode(pages, *geo) == _model(pages, font, size, FOCR_DEFAULT_ALPHABET, geo, 1.0, False), geo


@pytest.mark.parametrize("alphabet", ["\u0020\u00a0AB", "\u00a0\u0020AB", "AB\u00a0\u0020"], ids=["sp-nbsp", "nbsp-sp", "AB-nbsp-sp"])
def test_ties_go_to_the_first_listed(dec, alphabet):
    """U+0020 and U+00A0 are both blank: on paper the first one listed must win every time."""
    font, size = MONO, 13.0
    page = np.full((20, 80), 255, dtype=np.uint8)
    c = M.render_text(font, size, "AB  BA", 1.0, False)
    hh, ww = min(c.shape[0], 18), min(c.shape[1], 79)
    page[2: 2 + hh, 1: 1 + ww] = 255 - c[:hh, :ww]
    dec.set_font(font, size, alphabet)
    got = dec.decode(page, 0, 0, 80, 16, 20)
    assert got == [M.decode_image(page, font, size, alphabet, 0, 0, 80, 16, 20)]
    first_blank = next(ch for ch in alphabet if ch.isspace())
    other = "\u00a0" if first_blank == " " else " "
    text = got[0][0][1]
    assert first_blank in text and other not in text


def test_truth_on_clean_monospace_pages(dec):
    """Glyphs drawn at the decoder's own pen positions (kerning 1.0, monospace) decode to the drawn text."""
    font, size, alpha = MONO, 13.0, FOCR_DEFAULT_ALPHABET
    ox, oy = M.origin(font, size, alpha)
    inc = {ch: M.increment(font, size, ch, 1.0) for ch in alpha}
    rng = np.random.default_rng(5)
    W, H, adv, lh = 300, 80, 16, 14
    pages, truths = [], []
    for _ in range(3):
        page = np.full((H, W), 255, dtype=np.uint8)
        truth = []
        for ly in range(0, H - lh + 1, adv):
            text = "".join(rng.choice(list(_ink(alpha)), int(rng.integers(5, 30))))
            cov = np.zeros((lh, W), dtype=np.uint8)
            pos = np.float32(0)
            for ch in text:
                g = np.zeros((lh, W), dtype=np.uint8)
                M.raster_glyph(font, size, ch, np.float32(ox + pos), oy, g)
                cov = np.maximum(cov, g)
                pos = np.float32(pos + inc[ch])
            page[ly: ly + lh] = 255 - cov
            truth.append((ly, text))
        pages.append(page)
        truths.append(truth)
    dec.set_font(font, size, alpha)
    got = dec.decode(pages, 0, 0, W, lh, adv)
    assert [[(y, t.rstrip(" ")) for y, t in pg] for pg in got] == truths


def test_device_pages_decode_like_host_pages(dec):
    """The same batch from device memory (allocated through the HIP runtime the library itself uses)."""
    import ctypes as C

    pages, adv, lh = _pages(MONO, 13.0, FOCR_DEFAULT_ALPHABET, 1.07, False, 3)
    batch = np.ascontiguousarray(np.stack([pages[0], pages[1]]))
    dec.set_font(MONO, 13.0, FOCR_DEFAULT_ALPHABET, False, 1.07)
    host = dec.decode(batch, 1, 2, 200, lh, adv)
    hip = C.CDLL("libamdhip64.so.7")
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(batch.nbytes)) == 0
    try:
        assert hip.hipMemcpy(ptr, C.c_void_p(batch.ctypes.data), C.c_size_t(batch.nbytes), 1) == 0  # hipMemcpyHostToDevice
        assert hip.hipDeviceSynchronize() == 0
        assert dec.decode_device(ptr.value, *batch.shape, 1, 2, 200, lh, adv) == host
    finally:
        hip.hipFree(ptr)
    assert any(host)


def test_cli_end_to_end(tmp_path):
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    from PIL import Image

    font, size, kern = SANS, 13.0, 1.07
    pages, adv, lh = _pages(font, size, FOCR_DEFAULT_ALPHABET, kern, False, 21)
    pages = [pages[2], pages[0], pages[1], pages[2][::-1].copy()]  # two sizes, interleaved
    paths = []
    for i, p in enumerate(pages):
        path = str(tmp_path / f"page{i}.pgm")
        save_pgm(path, p)
        paths.append(path)
    vdir = tmp_path / "verify"
    vdir.mkdir()
    geo = (1, 2, 200, lh, adv)
    cmd = [FOCR, "-f", font, "-t", str(size), "-k", str(kern), "-x", "1", "-y", "2", "-w", "200", "--line-height", str(lh),
           "--line-advance", str(adv), "--verify", str(vdir), "-i"] + paths
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = _model(pages, font, size, FOCR_DEFAULT_ALPHABET, geo, kern, False)
    assert r.stdout == "".join(t + "\n" for pg in want for _, t in pg)
    mse_lines = set()
    for path, p, lines in zip(paths, pages, want):
        img, mse = M.verify_image(p, lines, font, size, geo[0], kern, False)
        got = np.asarray(Image.open(str(vdir / (os.path.splitext(os.path.basename(path))[0] + ".png"))).convert("RGB"))
        assert np.array_equal(got, img), path
        mse_lines.add(f"{path} {float(mse):.6f}")
    assert set(r.stderr.splitlines()) == mse_lines
    # one image, no --verify: the streaming path prints the same lines
    r1 = subprocess.run(cmd[: cmd.index("--verify")] + ["-i", paths[1]], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0 and r1.stdout == "".join(t + "\n" for _, t in want[1])

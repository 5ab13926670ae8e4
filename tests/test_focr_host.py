"""Host side of the focr line decoder (include/focr_decode.h): the 64-phase table against direct rasterisation, the f32
increments, the decode-font builder's refusals, the ABI tables and the CLI's usage errors.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import focr_line_model as M
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError, raster_glyph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
ASCII95 = "".join(chr(c) for c in range(32, 127))


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
def test_phase_table_equals_direct_rasterisation(font, hinting):
    """Every glyph, every 26.6 phase, at whole-pixel shifts from -2 to the far end of a 64-px line: the table's bitmap
    placed at (shift + off_x, off_y) is what focr_raster_glyph draws at translation (delta / 64, origin_y)."""
    size = 13.0
    f = DecodeFont(font, size, FOCR_DEFAULT_ALPHABET, hinting)
    ox, oy = f.origin
    W, H = 96, 24
    rng = np.random.default_rng(7)
    for i, ch in enumerate(FOCR_DEFAULT_ALPHABET):
        shifts = sorted({-2, -1, 0, 1, 17} | set(int(s) for s in rng.integers(2, 64, 2)))
        for p in range(64):
            bm, offx, offy = f.phase(i, p)
            for s in shifts:
                d = 64 * s + p
                want = np.zeros((H, W), dtype=np.uint8)
                raster_glyph(font, size, ch, np.float32(d / 64.0), oy, want, hinting)
                got = np.zeros((H + 64, W + 64), dtype=np.uint8)  # margin of 32 px on every side, cropped after placing
                y0, x0 = 32 + offy, 32 + s + offx
                got[y0: y0 + bm.shape[0], x0: x0 + bm.shape[1]] = bm
                assert np.array_equal(got[32: 32 + H, 32: 32 + W], want), (ch, p, s)
    f.close()


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("kerning", [1.0, 1.07, 0.93])
@pytest.mark.parametrize("size", [13.0, 24.0])
def test_increments_and_origin_match_the_model(font, kerning, size):
    f = DecodeFont(font, size, ASCII95, False, kerning)
    want = np.array([M.increment(font, size, ch, kerning) for ch in ASCII95], dtype=np.float32)
    assert f.increments().tobytes() == want.tobytes()
    assert np.float32(f.s.min_increment) == want.min()
    ox, oy = M.origin(font, size, ASCII95)
    assert (f.origin[0], f.origin[1]) == (ox, oy)
    f.close()


def test_builder_refusals():
    for k in (0.0, -1.0):
        with pytest.raises(DecoderError, match="kerning"):
            DecodeFont(MONO, 13.0, FOCR_DEFAULT_ALPHABET, False, k)
    with pytest.raises(DecoderError, match="missing"):
        DecodeFont(MONO, 13.0, "AB一", False, 1.0)  # no CJK in DejaVu


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(focr_[a-z0-9_]+)\s*\(", src))


def test_decode_header_equals_symbol_tables_and_exports():
    declared = _declared("focr_decode.h")
    bound = set(N.DECODE_RASTER_SYMBOLS) | set(N.DECODE_HIP_SYMBOLS)
    assert declared == bound, declared ^ bound
    assert not declared & (set(N.HIP_SYMBOLS) | set(N.HOST_SYMBOLS) | set(N.RASTER_SYMBOLS))
    N.decode_raster()
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    for lib, table in (("libfocr_raster.so", N.DECODE_RASTER_SYMBOLS), ("libfocr_hip.so", N.DECODE_HIP_SYMBOLS)):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(N.LIB_DIR, lib)], capture_output=True, text=True,
                             check=True).stdout
        assert set(table) <= set(re.findall(r" T (focr_\w+)", out)), lib


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_usage_errors_and_test_refused(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--img", "--font", "--alphabet", "--hinting", "--text-size", "--kerning", "--x", "--y", "--width",
                 "--line-height", "--line-advance", "--test", "--verify"):
        assert flag in r.stdout, flag
    assert FOCR_DEFAULT_ALPHABET in r.stdout
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    for argv in ([], ["-t", "13"], base[:-2], base + ["--bogus"], base + ["-x", "-3"], base + ["-t", "abc"],
                 base + ["--line-advance"]):
        r = subprocess.run([focr_bin] + argv, capture_output=True, text=True)
        assert r.returncode == 2, (argv, r.returncode, r.stderr)
        assert "error:" in r.stderr and "Usage: focr" in r.stderr
    # the u32 flags follow Rust's u32::from_str: a leading '+' is taken, blanks and trailing characters are not
    r = subprocess.run([focr_bin] + base + ["-x", "+3", "--bogus"], capture_output=True, text=True)
    assert r.returncode == 2 and "unexpected argument '--bogus'" in r.stderr, r.stderr
    for v in (" 3", "3x"):
        r = subprocess.run([focr_bin] + base + ["-x", v], capture_output=True, text=True)
        assert r.returncode == 2 and f"invalid value '{v}' for '-x'" in r.stderr, r.stderr
    r = subprocess.run([focr_bin] + base + ["--test", "out", "-i", "x.png"], capture_output=True, text=True)
    assert r.returncode != 0 and "--test" in r.stderr

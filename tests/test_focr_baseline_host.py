"""Host side of the focr baseline search (include/focr_decode.h): the y-phase font build against the plain build and
against FreeType, the new entry points declared, bound and exported, the Python refusals, and the CLI's usage errors
before it touches a device.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import raster_glyph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
NEW_HIP = ("focr_decoder_set_baseline_fonts", "focr_decoder_set_baseline_search", "focr_decoder_get_baselines",
           "focr_decoder_debug_set_baseline_grid")
F32 = np.float32


def _bitmaps(f):
    return bytes(np.ctypeslib.as_array(f.bitmaps, shape=(f.bitmaps_len,)))


def _glyph_fields(g):
    return (g.codepoint, F32(g.increment).tobytes(), g.box_w, g.box_h, g.stride, g.offset, tuple(g.off_x), tuple(g.off_y))


@pytest.mark.parametrize("font,size,hinting,kerning", [(MONO, 13.0, False, 1.0), (SANS, 9.5, True, 1.25)], ids=["mono", "sans-hinted-kerned"])
@pytest.mark.parametrize("y_bits", [1, 3])
def test_phase_zero_is_the_plain_build_and_the_rest_share_its_frame(font, size, hinting, kerning, y_bits):
    plain = DecodeFont(font, size, FOCR_DEFAULT_ALPHABET, hinting, kerning)
    y = DecodeFont(font, size, FOCR_DEFAULT_ALPHABET, hinting, kerning, y_bits=y_bits)
    assert len(y.fonts) == 1 << y_bits and len(plain.fonts) == 1
    G = len(FOCR_DEFAULT_ALPHABET)
    a, b = plain.s, y.fonts[0]
    assert _bitmaps(a) == _bitmaps(b) and a.n_glyphs == b.n_glyphs == G
    assert [_glyph_fields(a.glyphs[i]) for i in range(G)] == [_glyph_fields(b.glyphs[i]) for i in range(G)]
    for f in y.fonts:  # glyph order, increments (bitwise), origin, size, kerning, hinting; its own int32 bound
        assert f.n_glyphs == G
        for name in ("origin_x", "origin_y", "text_size", "kerning", "min_increment"):
            assert F32(getattr(f, name)).tobytes() == F32(getattr(a, name)).tobytes(), name
        assert f.hinting == a.hinting
        for i in range(G):
            g = f.glyphs[i]
            assert g.codepoint == a.glyphs[i].codepoint and F32(g.increment).tobytes() == F32(a.glyphs[i].increment).tobytes()
            assert g.stride % 4 == 0 and g.stride >= g.box_w and g.stride * g.box_h * 2 * 255 * 255 < 2 ** 31
            assert g.offset + 64 * g.stride * g.box_h <= f.bitmaps_len
    assert len({f.bitmaps_len for f in y.fonts}) > 1  # box sizes do differ between the y-phases
    plain.close()
    y.close()


@pytest.mark.parametrize("font,size,hinting", [(MONO, 13.0, False), (SANS, 13.0, True)], ids=["mono", "sans-hinted"])
def test_every_phase_is_its_freetype_raster(font, size, hinting):
    """Glyph i's phase (p, v) is FreeType's bitmap at the translation (origin_x + p / 64, origin_y + v / 8), placed at
    its (off_x, off_y) on the line canvas; nothing of it lies outside the box.  (Drawn four whole pixels right and down:
    a hinted glyph's box starts a row above the canvas at some v.)"""
    al = FOCR_DEFAULT_ALPHABET
    f = DecodeFont(font, size, al, hinting, y_bits=3)
    ox, oy = f.origin
    pad = 4
    for v in range(8):
        ty = F32(F32(oy + pad) + F32(v) / F32(8))
        for p in (0, 21, 63):
            for i in range(0, len(al), 3):
                bm, off_x, off_y = f.phase(i, p, v)
                want = np.zeros((int(size) * 2 + 8 + pad, int(size) * 2 + 8 + pad), dtype=np.uint8)
                raster_glyph(font, size, al[i], F32(F32(ox + pad) + F32(p) / F32(64)), ty, want, hinting)
                got = np.zeros_like(want)
                x0, y0 = int(ox) + pad + off_x, pad + off_y
                assert y0 >= 0 and x0 >= 0
                got[y0: y0 + bm.shape[0], x0: x0 + bm.shape[1]] = bm
                assert np.array_equal(got, want), (v, p, al[i])
    f.close()


def test_build_refusals():
    with pytest.raises(ValueError, match="y_bits"):
        DecodeFont(MONO, 13.0, y_bits=4)
    lib = N.decode_raster()
    fonts = (N.DecodeFontStruct * 16)()
    cps = (C.c_uint32 * 2)(65, 66)
    e = C.create_string_buffer(256)
    assert lib.focr_decode_font_build_y(MONO.encode(), 13.0, 0, 1.0, cps, 2, 4, fonts, e, len(e)) != 0 and b"y_bits" in e.value
    assert lib.focr_decode_font_build_y(MONO.encode(), 13.0, 0, 0.0, cps, 2, 1, fonts, e, len(e)) != 0 and b"kerning" in e.value
    assert all(not f.glyphs and not f.bitmaps for f in fonts)


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    assert "FOCR_BASELINE_MAX = 32" in header and "FOCR_BASELINE_Y_BITS_MAX = 3" in header
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (focr_\w+)", out))
    for sym in NEW_HIP:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in N.DECODE_HIP_SYMBOLS and sym in exported, sym
    assert re.search(r"\bfocr_decode_font_build_y\s*\(", header) and "focr_decode_font_build_y" in N.DECODE_RASTER_SYMBOLS


def test_python_refusals():
    check = LineDecoder._check_baseline_search
    assert check(0, True, 8, True, True, 8) == 0 and check(32, False, 0, False, False, 0) == 32
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="0 .. 32"):
            check(bad, False, 0, False, False, 0)
    for args, what in (((True, 0, False, False, 0), "scores=True"), ((False, 8, False, False, 0), "pen_search"),
                       ((False, 0, True, False, 0), "whole_line=True"), ((False, 0, True, True, 0), "whole_line=True"),
                       ((False, 0, False, True, 0), "margins=True"), ((False, 0, False, False, 8), "pen_slack")):
        with pytest.raises(ValueError, match="baseline_search does not go with " + re.escape(what)):
            check(4, *args)
    for fn in (LineDecoder.decode, LineDecoder.decode_device):
        assert inspect.signature(fn).parameters["baseline_search"].default == 0
    assert inspect.signature(LineDecoder.set_font).parameters["y_bits"].default == 0
    assert list(inspect.signature(DecodeFont.phase).parameters) == ["self", "i", "p", "v"]
    dec = object.__new__(LineDecoder)  # no device: the refusals come before anything touches the library
    dec.font = object()
    page = np.full((16, 40), 255, dtype=np.uint8)
    with pytest.raises(ValueError, match="baseline_search does not go with scores=True"):
        dec.decode([page], 0, 0, 40, 16, 16, scores=True, baseline_search=4)
    with pytest.raises(ValueError, match="baseline_search does not go with whole_line=True"):
        dec.decode_device(0, 1, 16, 40, 0, 0, 40, 16, 16, whole_line=True, baseline_search=4)
    with pytest.raises(ValueError, match="0 .. 32"):
        dec.decode([page], 0, 0, 40, 16, 16, baseline_search=33)
    dec._h = None


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt, arg in (("--baseline-search", "<N>"), ("--y-bits", "<B>"), ("--baselines", "<BASELINES>")):
        line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith(opt + " ")]
        assert "[extension]" in line and arg in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    img = ["-i", "/nonexistent/page.pgm"]  # a run that got past the arguments would fail on it with another exit code
    for extra, words in ((["--baseline-search", "33"], ("--baseline-search", "at most 32")), (["--baseline-search", "x"], ("--baseline-search",)),
                         (["--baseline-search", "4", "--y-bits", "4"], ("--y-bits", "at most 3")),
                         (["--y-bits", "2"], ("--y-bits", "--baseline-search")), (["--baselines", "/dev/null"], ("--baselines", "--baseline-search")),
                         (["--baseline-search", "4", "--scores", "/dev/null"], ("--baseline-search", "--scores")),
                         (["--baseline-search", "4", "--pen-search", "4"], ("--baseline-search", "--pen-search")),
                         (["--baseline-search", "4", "--whole-line"], ("--baseline-search", "--whole-line"))):
        r = subprocess.run([focr_bin] + base + extra + img, capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "Usage: focr" in r.stderr and r.stdout == "", extra
        assert all(w in r.stderr for w in words), (extra, r.stderr)
    r = subprocess.run([focr_bin] + base + ["--baseline-search", "32", "--y-bits", "3"], capture_output=True, text=True)  # no -i: nothing to do
    assert r.returncode == 0 and r.stdout == ""

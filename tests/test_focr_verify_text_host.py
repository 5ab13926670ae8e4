"""Host side of focr_decoder_verify_text (include/focr_decode.h): the entry points declared, bound and exported, the header's
definition, LineDecoder.verify_text's signature and the refusals it makes before it touches the library, and the CLI's usage
errors and --help line before it touches a device.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from font_ocr_amd import LineDecoder
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
SYMBOLS = {"focr_decoder_set_verify_font_candidates": (r"int", r"\(focr_decoder_t \*dec, const focr_verify_font_t \*fonts, uint32_t n\);"),
           "focr_decoder_verify_text": (r"int", r"\(focr_decoder_t \*dec, const uint8_t \*pages, int pages_on_device, size_t n_pages,\s*"
                                        r"size_t page_w, size_t page_h, uint32_t x_start,\s*const focr_text_line_t \*lines, size_t n_lines,\s*"
                                        r"const uint16_t \*chars, const uint32_t \*pens, const int8_t \*offsets, size_t n_chars,\s*"
                                        r"uint8_t \*rgb, int rgb_on_device, uint64_t \*sq_sums\);"),
           "focr_decoder_last_verify_text_ms": (r"float", r"\(const focr_decoder_t \*dec\);"),
           "focr_decoder_last_verify_text_launches": (r"uint32_t", r"\(const focr_decoder_t \*dec\);")}


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (focr_\w+)", out))
    for name, (ret, args) in SYMBOLS.items():
        assert re.search(r"\b%s\s+%s\s*%s" % (ret, name, args), header), name
        assert name in N.DECODE_HIP_SYMBOLS and len(N.DECODE_HIP_SYMBOLS[name][1]) == args.count(",") + 1, name
        assert name in exported, name
    # focr_text_line_t is focr_decoded_line_t with the font in pad's place, in the header and in the binding
    assert re.search(r"typedef struct focr_text_line \{\s*uint32_t page, y;\s*uint64_t first;\s*uint32_t n_chars;\s*uint32_t font;\s*\} focr_text_line_t;", header)
    assert [f[0] for f in N.TextLine._fields_] == ["page", "y", "first", "n_chars", "font"] and C.sizeof(N.TextLine) == C.sizeof(N.DecodedLine) == 24
    assert all(getattr(N.TextLine, a).offset == getattr(N.DecodedLine, b).offset for a, b in zip(("page", "y", "first", "n_chars", "font"), ("page", "y", "first", "n_chars", "pad")))
    # the definition: fonts, placement, order, the image, every refusal, what stays as it was
    section = header[header.index("device: verify images of a caller's text"): header.index("int focr_decoder_verify_text")]
    for word in ("lines[l].font", "focr_decoder_set_verify_font_candidates", "focr_decoder_set_font_candidates", "render() renders a string",
                 "clipped at the page's right and bottom edges", "n_chars == 0 or y >= page_h", "pens[first + q] / 64", "offsets[first + q] / 64",
                 "pens and offsets together are refused", "non-decreasing page order", "list order is the drawing order", "exact sum of (R - B)^2",
                 "without a line still gets its image", "before anything is launched", "no decode font", "names the line's index",
                 "names the setter to call", "2^24", "buffers of its own", "needs no run", "What it does not do"):
        assert word in section, word
    # the older refusals keep their sentences, each with a pointer to the new entry point beside it
    for pinned in ("focr_decoder_verify after a font-search run is refused", "focr --verify of a mixed-font run"):
        at = header.index(pinned)
        assert "focr_decoder_verify_text" in header[at: at + 420], pinned


def test_python_signature_and_refusals():
    sig = inspect.signature(LineDecoder.verify_text)
    assert list(sig.parameters) == ["self", "luma_pages", "lines", "x", "fonts", "pens", "offsets", "images"]
    assert [sig.parameters[p].default for p in ("fonts", "pens", "offsets", "images")] == [None, None, None, True]
    assert list(inspect.signature(LineDecoder.set_font_candidates).parameters) == ["self", "fonts"]
    dec = object.__new__(LineDecoder)  # no device: these refusals come before anything touches the library

    class Font:
        alphabet = "ab c"

    dec.font, dec._candidates, dec._vfont, dec._vcands = Font(), [object()], object(), object()
    page = np.full((16, 40), 255, dtype=np.uint8)
    with pytest.raises(ValueError, match="pens or offsets, not both"):
        dec.verify_text([page], [[(0, "ab")]], 0, pens=[[[0, 64]]], offsets=[[[0, 0]]])
    with pytest.raises(ValueError, match="one list per page"):
        dec.verify_text([page], [[(0, "ab")], []], 0)
    for name in ("fonts", "pens", "offsets"):
        with pytest.raises(ValueError, match=name + " must hold one entry per line"):
            dec.verify_text([page], [[(0, "ab"), (8, "c")]], 0, **{name: [[0]]})
    with pytest.raises(ValueError, match=r"fonts must be 0 \.\. 1"):
        dec.verify_text([page], [[(0, "ab")]], 0, fonts=[[2]])
    with pytest.raises(ValueError, match=r"'x' \(page 0, line 1\) is not in the alphabet"):
        dec.verify_text([page], [[(0, "ab"), (8, "axb")]], 0)
    with pytest.raises(ValueError, match="1 pens or offsets for 2 characters"):
        dec.verify_text([page], [[(0, "ab")]], 0, pens=[[[0]]])
    # the existing refusals keep their words
    dec._batch, dec._font_search = (1, 16, 40), True
    with pytest.raises(RuntimeError, match="searched fonts"):
        dec.verify()
    with pytest.raises(ValueError, match="font_search=True does not go with verify yet"):
        dec.decode([page], 0, 0, 40, 16, 16, font_search=True, verify="mse")
    dec._h = None


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin, tmp_path):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--verify-fonts ")]
    assert "[extension]" in line and "<DIR>" in line and "winning font" in line and "only with --font-candidate" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    img = ["-i", "/nonexistent/page.pgm"]  # a run that got past the arguments would fail on it with another exit code
    cand = ["--font-candidate", "t=12"]
    for extra, words in ((["--verify-fonts", str(tmp_path)], ("--verify-fonts <DIR>", "--font-candidate <SPEC>", "cannot be used without")),
                         (cand + ["--verify", str(tmp_path)], ("--font-candidate", "--verify <VERIFY>")),
                         (cand + ["--verify-fonts", str(tmp_path), "--verify", str(tmp_path)], ("--font-candidate", "--verify <VERIFY>"))):
        r = subprocess.run([focr_bin] + base + extra + img, capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "Usage: focr" in r.stderr and r.stdout == "", (extra, r.stderr)
        assert all(w in r.stderr for w in words), (extra, r.stderr)
    r = subprocess.run([focr_bin] + base + cand + ["--verify-fonts", str(tmp_path / "missing")] + img, capture_output=True, text=True)
    assert r.returncode == 101 and "--verify-fonts should be a dir" in r.stderr and r.stdout == ""
    for extra in (cand + ["--verify-fonts", str(tmp_path)], cand + ["--whole-line", "--verify-fonts", str(tmp_path), "--fonts", "/dev/null"]):
        r = subprocess.run([focr_bin] + base + extra, capture_output=True, text=True)  # no -i: nothing to do
        assert r.returncode == 0 and r.stdout == "", (extra, r.stderr)

"""Host side of focr_decoder_score_text (include/focr_decode.h): the entry points declared, bound and exported, the header's
definition, LineDecoder.score_text's and rank_text's signatures and the refusals they make before they touch the library, and
the CLI's usage errors and --help lines before it touches a device.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from font_ocr_amd import LineDecoder
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import TextScore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
SYMBOLS = {"focr_decoder_score_text": (r"int", r"\(focr_decoder_t \*dec, const uint8_t \*pages, int pages_on_device, size_t n_pages,\s*"
                                       r"size_t page_w, size_t page_h, uint32_t x_start, uint32_t width, uint32_t line_height,\s*"
                                       r"const focr_text_line_t \*lines, size_t n_lines,\s*"
                                       r"const uint16_t \*chars, const uint32_t \*pens, const int8_t \*offsets, size_t n_chars,\s*"
                                       r"const int8_t \*line_q, uint32_t y_bits, uint32_t shift_radius,\s*"
                                       r"int32_t \*terms, focr_text_score_t \*out\);"),
           "focr_decoder_last_score_text_ms": (r"float", r"\(const focr_decoder_t \*dec\);"),
           "focr_decoder_last_score_text_launches": (r"uint32_t", r"\(const focr_decoder_t \*dec\);")}


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
    assert re.search(r"typedef struct focr_text_score \{\s*uint64_t line_base;[^}]*int64_t\s+cost;[^}]*int32_t\s+shift;[^}]*uint32_t pad;\s*\} focr_text_score_t;",
                     header)
    assert [f[0] for f in N.TextScoreStruct._fields_] == ["line_base", "cost", "shift", "pad"] and C.sizeof(N.TextScoreStruct) == 24
    assert (N.TextScoreStruct.cost.offset, N.TextScoreStruct.shift.offset) == (8, 16)
    # the definition: crop, fonts, the three placements, rendering, the vertical position, terms, the shift, refusals, state, scope
    section = header[header.index("device: the cost of a caller's text"): header.index("typedef struct focr_text_score")]
    for word in ("any page order", "repeat and share characters", "image::crop_imm", "line_base 0 and every term 0", "lines[l].font",
                 "no verify table is needed", "trunc((origin_x_k + pos) * 64)", "(float)offsets[g] * 0.015625f", "64 * origin_x_k + pens[g]",
                 "pens and offsets together are refused", "delta & 63", "delta >> 6", "nothing is dropped", "wholly outside the crop",
                 "q & (2^B - 1)", "q >> B", "clipped to the crop on all four", "c * (c - 2 r)", "running sum of n_chars", "FOCR_PEN_SEARCH_MAX",
                 "(cost_j, rank(j))", "N = 0 scores once", "before anything is launched", "width 0 or line_height 0", "fractional or negative",
                 "one vertical phase", "origin_y is not a whole number", "2^24", "buffers of its own", "needs no run", "What it does not do",
                 "a per-line x", "a vertical search", "forced alignment", "true composed error", "any change to focr_decoder_run"):
        assert word in section, word
    # verify_text's own "what it does not do" now points here
    at = header.index("lines at sub-pixel rows, per-line sums")
    assert "focr_decoder_score_text" in header[at: at + 200]


def test_python_signatures_and_refusals():
    sig = inspect.signature(LineDecoder.score_text)
    assert list(sig.parameters) == ["self", "luma_pages", "lines", "x", "width", "line_height", "fonts", "pens", "offsets", "baselines", "y_bits",
                                    "shift", "terms"]
    assert [sig.parameters[p].default for p in ("fonts", "pens", "offsets", "baselines", "y_bits", "shift", "terms")] == [None, None, None, None, 0, 0, True]
    sig = inspect.signature(LineDecoder.rank_text)
    assert list(sig.parameters) == ["self", "page", "y", "text", "x", "width", "line_height", "shift"] and sig.parameters["shift"].default == 0
    assert TextScore._fields == ("base", "cost", "shift", "terms")
    dec = object.__new__(LineDecoder)  # no device: these refusals come before anything touches the library

    class Font:
        alphabet = "ab c"

    dec.font, dec._candidates = None, []
    page = np.full((16, 40), 255, dtype=np.uint8)
    with pytest.raises(RuntimeError, match=r"set_font\(\) first"):
        dec.score_text([page], [[(0, "ab")]], 0, 40, 16)
    dec.font, dec._candidates = Font(), [object()]
    with pytest.raises(ValueError, match="pens or offsets, not both"):
        dec.score_text([page], [[(0, "ab")]], 0, 40, 16, pens=[[[0, 64]]], offsets=[[[0, 0]]])
    for bad in (-1, 65):
        with pytest.raises(ValueError, match=r"shift must be 0 \.\. 64"):
            dec.score_text([page], [[(0, "ab")]], 0, 40, 16, shift=bad)
    with pytest.raises(ValueError, match=r"y_bits must be 0 \.\. 3"):
        dec.score_text([page], [[(0, "ab")]], 0, 40, 16, baselines=[[0]], y_bits=4)
    for w, lh in ((0, 16), (40, 0)):
        with pytest.raises(ValueError, match="width and line_height must be positive"):
            dec.score_text([page], [[(0, "ab")]], 0, w, lh)
    with pytest.raises(ValueError, match="one list per page"):
        dec.score_text([page], [[(0, "ab")], []], 0, 40, 16)
    for name in ("fonts", "pens", "offsets", "baselines"):
        with pytest.raises(ValueError, match=name + " must hold one entry per line"):
            dec.score_text([page], [[(0, "ab"), (8, "c")]], 0, 40, 16, **{name: [[0]]})
    with pytest.raises(ValueError, match=r"fonts must be 0 \.\. 1"):
        dec.score_text([page], [[(0, "ab")]], 0, 40, 16, fonts=[[2]])
    with pytest.raises(ValueError, match=r"'x' \(page 0, line 1\) is not in the alphabet"):
        dec.score_text([page], [[(0, "ab"), (8, "axb")]], 0, 40, 16)
    with pytest.raises(ValueError, match="1 pens or offsets for 2 characters"):
        dec.score_text([page], [[(0, "ab")]], 0, 40, 16, offsets=[[[0]]])
    with pytest.raises(ValueError, match=r"one luma page \(H, W\)"):
        dec.rank_text(np.stack([page, page]), 0, "ab", 0, 40, 16)
    with pytest.raises(ValueError, match=r"'x' \(page 0, line 0\) is not in the alphabet"):
        dec.rank_text(page, 0, "ax", 0, 40, 16)
    dec._h = None


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--rank-text ")]
    assert "[extension]" in line and "<TEXT>" in line and "Decode nothing" in line and "--font-candidate" in line
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--rank-shift ")]
    assert "[extension]" in line and "<N>" in line and "N <= 64" in line and "only with --rank-text" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    img = ["-i", "/nonexistent/page.pgm"]  # a run that got past the arguments would fail on it with another exit code
    for extra, words in ((["--rank-shift", "3"], ("--rank-shift <N>", "cannot be used without", "--rank-text <TEXT>")),
                         (["--rank-text", "ab~c"], ("invalid value 'ab~c'", "--rank-text <TEXT>", "'~' is not in the alphabet")),
                         (["--rank-text", "ab", "--rank-shift", "65"], ("--rank-shift", "at most 64")),
                         (["--rank-text", "ab", "--rank-shift", "x"], ("--rank-shift",)),
                         (["--rank-text"], ("--rank-text",))):
        r = subprocess.run([focr_bin] + base + extra + (img if extra[-1] != "--rank-text" else []), capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "Usage: focr" in r.stderr and r.stdout == "", (extra, r.stderr)
        assert all(w in r.stderr for w in words), (extra, r.stderr)
    # past the arguments: the image is read before any device is asked for, and the text may be empty
    for text in ("ab", ""):
        r = subprocess.run([focr_bin] + base + ["--rank-text", text, "--rank-shift", "64"] + img, capture_output=True, text=True)
        assert r.returncode == 101 and "--rank-text:" in r.stderr and "/nonexistent/page.pgm" in r.stderr and r.stdout == "", r.stderr
    r = subprocess.run([focr_bin] + base + ["--rank-text", "ab"], capture_output=True, text=True)  # no -i: nothing to score against
    assert r.returncode == 101 and "--rank-text: no -i image" in r.stderr and r.stdout == ""

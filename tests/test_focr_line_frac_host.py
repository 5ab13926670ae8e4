"""Host side of the focr decoder's fractional line grid (include/focr_decode.h): the setter declared, bound and exported and
its refusal without a decoder, the definition's words in the header, the Python signatures and checks, and the CLI's usage
errors before it touches a device.  No GPU needed.  (The setter's bounds and focr_decoder_run's refusals need a decoder, and
a decoder needs a device: tests/test_gpu_focr_line_frac.py::test_refusals has them, each with its message.)"""
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
SYMBOL = "focr_decoder_set_line_frac"


def test_symbol_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    assert re.search(r"\bint %s\s*\(focr_decoder_t \*dec, uint32_t y_frac, uint32_t advance_frac\);" % SYMBOL, header)
    assert SYMBOL in N.DECODE_HIP_SYMBOLS and len(N.DECODE_HIP_SYMBOLS[SYMBOL][1]) == 3
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    assert SYMBOL in set(re.findall(r" T (focr_\w+)", out))
    # the definition states the grid's integers, the candidates, the returned q, the verify, and the refusal
    section = header[header.index("a fractional line grid for the two baseline modes"): header.index("int %s" % SYMBOL)]
    for word in ("L = 64 * line_advance + advance_frac", "Y_i = 64 * y_start + y_frac + i * L", "yc_i = Y_i >> 6", "f_i = Y_i & 63",
                 "n_slots = ceil((64 * page_h - Y_0) / L)", "c_i = ((f_i << B) + 32) >> 6", "q = c_i + rank_offset(rank)", "(cost_q, rank)",
                 "fits the int8_t", "FOCR_BASELINE_MAX + 1", "launch count stays 3", "radius >= 1", "line_advance == 0", "focr_decoder_test_images",
                 "What it does not cure"):
        assert word in section, word


def test_setter_refuses_a_null_decoder():
    lib = N.decode_hip()
    assert lib.focr_decoder_set_line_frac(None, 0, 0) != 0
    assert lib.focr_decoder_last_error(None) == b"focr_decoder_set_line_frac: null decoder"


def test_python_signatures_and_checks():
    check = LineDecoder._check_line_frac
    assert check(0, 0, 0, 0) == (0, 0) and check(63, 63, 1, 0) == (63, 63) and check(5, 0, 0, 32) == (5, 0) and check(0, 1, 4, 0) == (0, 1)
    for bad, name in (((64, 0), "y_frac"), ((-1, 0), "y_frac"), ((0, 64), "line_advance_frac"), ((0, -1), "line_advance_frac")):
        with pytest.raises(ValueError, match=name + r" must be 0 \.\. 63"):
            check(*bad, 4, 0)
    for fr in ((1, 0), (0, 1), (63, 63)):
        with pytest.raises(ValueError, match="need baseline_search or whole_baseline"):
            check(*fr, 0, 0)
    for fn in (LineDecoder.decode, LineDecoder.decode_device):
        p = inspect.signature(fn).parameters
        assert p["y_frac"].default == 0 and p["line_advance_frac"].default == 0
    dec = object.__new__(LineDecoder)  # no device: the checks come before anything touches the library
    dec.font = object()
    page = np.full((16, 40), 255, dtype=np.uint8)
    with pytest.raises(ValueError, match="need baseline_search or whole_baseline"):
        dec.decode([page], 0, 0, 40, 16, 16, y_frac=20)
    with pytest.raises(ValueError, match="need baseline_search or whole_baseline"):
        dec.decode([page], 0, 0, 40, 16, 16, whole_line=True, line_advance_frac=38)  # the whole-line decode without candidates
    with pytest.raises(ValueError, match="need baseline_search or whole_baseline"):
        dec.decode_device(0, 1, 16, 40, 0, 0, 40, 16, 16, scores=True, y_frac=1)
    with pytest.raises(ValueError, match="line_advance_frac must be 0 .. 63"):
        dec.decode_device(0, 1, 16, 40, 0, 0, 40, 16, 16, baseline_search=4, line_advance_frac=64)
    # what the mode refuses anyway is still refused, with its own words
    with pytest.raises(ValueError, match="whole_baseline needs whole_line=True"):
        dec.decode([page], 0, 0, 40, 16, 16, whole_baseline=4, y_frac=20)
    with pytest.raises(ValueError, match="baseline_search does not go with scores=True"):
        dec.decode([page], 0, 0, 40, 16, 16, baseline_search=4, scores=True, y_frac=20)
    dec._h = None


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--y-frac", "--line-advance-frac"):
        line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith(opt + " ")]
        assert "[extension]" in line and "<N>" in line and "N <= 63" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    img = ["-i", "/nonexistent/page.pgm"]  # a run that got past the arguments would fail on it with another exit code
    for extra, words in ((["--y-frac", "20"], ("--y-frac", "--baseline-search", "--whole-baseline")),
                         (["--line-advance-frac", "38"], ("--line-advance-frac", "--baseline-search", "--whole-baseline")),
                         (["--whole-line", "--y-frac", "20"], ("--y-frac", "--whole-baseline")),
                         (["--pen-search", "4", "--line-advance-frac", "1"], ("--line-advance-frac", "--baseline-search")),
                         (["--baseline-search", "1", "--y-frac", "64"], ("--y-frac", "at most 63")),
                         (["--baseline-search", "1", "--line-advance-frac", "64"], ("--line-advance-frac", "at most 63")),
                         (["--baseline-search", "1", "--y-frac", "x"], ("--y-frac",)),
                         (["--baseline-search", "1", "--y-frac", "-1"], ("--y-frac",)),
                         (["--whole-line", "--whole-baseline", "1", "--line-advance-frac", "38", "--test", "out"], ("--line-advance-frac", "--test")),
                         (["--baseline-search", "1", "--y-frac", "0", "--test", "out"], ("--y-frac", "--test")),
                         (["--whole-baseline", "1", "--y-frac", "20"], ("--whole-baseline", "--whole-line"))):
        r = subprocess.run([focr_bin] + base + extra + img, capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "Usage: focr" in r.stderr and r.stdout == "", extra
        assert all(w in r.stderr for w in words), (extra, r.stderr)
    for mode in (["--baseline-search", "1"], ["--whole-line", "--whole-baseline", "1"]):
        r = subprocess.run([focr_bin] + base + mode + ["--y-bits", "2", "--y-frac", "63", "--line-advance-frac", "63"],
                           capture_output=True, text=True)  # no -i: nothing to do
        assert r.returncode == 0 and r.stdout == ""


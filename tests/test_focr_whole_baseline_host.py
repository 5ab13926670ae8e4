"""Host side of the focr whole-line decode under baseline candidates (include/focr_decode.h): the new entry point declared,
bound and exported, the Python signatures and refusals, and the CLI's usage errors before it touches a device.  No GPU
needed."""
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
SYMBOL = "focr_decoder_set_whole_baseline"


def test_symbol_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    assert re.search(r"\bint %s\s*\(focr_decoder_t \*dec, uint32_t y_bits, uint32_t n\);" % SYMBOL, header)
    assert SYMBOL in N.DECODE_HIP_SYMBOLS and len(N.DECODE_HIP_SYMBOLS[SYMBOL][1]) == 3
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    assert SYMBOL in set(re.findall(r" T (focr_\w+)", out))
    # the definition names what it takes from its two parents, and every refusal
    section = header[header.index("baseline candidates of a whole-line run"): header.index("int %s" % SYMBOL)]
    for word in ("ty_q = origin_y + q * 2^-B", "term_q", "(cost_q, rank(q))", "focr_decoder_get_baselines", "launch count stays 3",
                 "whole-line decode off", "margins on", "pen slack", "focr_decoder_set_baseline_fonts", "whole number >= 0", "2^47"):
        assert word in section, word


def test_python_signatures_and_refusals():
    check = LineDecoder._check_whole_baseline
    assert check(0, False, True, 8) == 0 and check(32, True, False, 0) == 32 and check(1, True, False, 0) == 1
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="whole_baseline must be 0 .. 32"):
            check(bad, True, False, 0)
    with pytest.raises(ValueError, match="whole_baseline needs whole_line=True"):
        check(4, False, False, 0)
    for args, what in (((True, True, 0), "margins=True"), ((True, False, 8), "pen_slack")):
        with pytest.raises(ValueError, match="whole_baseline does not go with " + re.escape(what)):
            check(4, *args)
    for fn in (LineDecoder.decode, LineDecoder.decode_device):
        assert inspect.signature(fn).parameters["whole_baseline"].default == 0
    dec = object.__new__(LineDecoder)  # no device: the refusals come before anything touches the library
    dec.font = object()
    page = np.full((16, 40), 255, dtype=np.uint8)
    with pytest.raises(ValueError, match="whole_baseline needs whole_line=True"):
        dec.decode([page], 0, 0, 40, 16, 16, whole_baseline=4)
    with pytest.raises(ValueError, match="whole_baseline does not go with margins=True"):
        dec.decode([page], 0, 0, 40, 16, 16, whole_line=True, margins=True, whole_baseline=4)
    with pytest.raises(ValueError, match="whole_baseline does not go with pen_slack"):
        dec.decode_device(0, 1, 16, 40, 0, 0, 40, 16, 16, whole_line=True, pen_slack=4, whole_baseline=4)
    with pytest.raises(ValueError, match="0 .. 32"):
        dec.decode_device(0, 1, 16, 40, 0, 0, 40, 16, 16, whole_line=True, whole_baseline=33)
    # the pen loop's search stays refused beside the whole-line decode, whatever this switch says
    with pytest.raises(ValueError, match="baseline_search does not go with whole_line=True"):
        dec.decode([page], 0, 0, 40, 16, 16, whole_line=True, baseline_search=4, whole_baseline=4)
    dec._h = None


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--whole-baseline ")]
    assert "[extension]" in line and "<N>" in line and "only with the whole-line decode" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    img = ["-i", "/nonexistent/page.pgm"]  # a run that got past the arguments would fail on it with another exit code
    for extra, words in ((["--whole-line", "--whole-baseline", "33"], ("--whole-baseline", "at most 32")),
                         (["--whole-line", "--whole-baseline", "x"], ("--whole-baseline",)),
                         (["--whole-baseline", "4"], ("--whole-baseline", "--whole-line")),
                         (["--whole-line", "--whole-baseline", "4", "--y-bits", "4"], ("--y-bits", "at most 3")),
                         (["--whole-line", "--whole-baseline", "4", "--margins", "/dev/null"], ("--whole-baseline", "--margins")),
                         (["--whole-line", "--whole-baseline", "4", "--pen-slack", "4"], ("--whole-baseline", "--pen-slack")),
                         (["--whole-line", "--whole-baseline", "4", "--baseline-search", "4"], ("--baseline-search", "--whole-line")),
                         (["--whole-line", "--y-bits", "2"], ("--y-bits", "--baseline-search")),
                         (["--whole-line", "--baselines", "/dev/null"], ("--baselines", "--baseline-search"))):
        r = subprocess.run([focr_bin] + base + extra + img, capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "Usage: focr" in r.stderr and r.stdout == "", extra
        assert all(w in r.stderr for w in words), (extra, r.stderr)
    r = subprocess.run([focr_bin] + base + ["--whole-line", "--whole-baseline", "32", "--y-bits", "3", "--baselines", "/dev/null"],
                       capture_output=True, text=True)  # no -i: nothing to do
    assert r.returncode == 0 and r.stdout == ""

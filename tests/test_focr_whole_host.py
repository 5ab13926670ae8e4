"""Host side of the focr whole-line decode (include/focr_decode.h): the new entry points are declared, bound and
exported, the CLI knows --whole-line and refuses it beside --scores and --pen-search before it touches a device, and the
Python API refuses the same combinations.  No GPU needed."""
import os
import re
import subprocess

import pytest

from font_ocr_amd import LineDecoder
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
NEW = ("focr_decoder_set_whole_line", "focr_decoder_get_pens", "focr_decoder_debug_set_whole_grid")


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (focr_\w+)", out))
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in N.DECODE_HIP_SYMBOLS and sym in exported, sym
    for word in ("inc64[i] = (int)rintf(increment[i] * 64)", "lowest (cost, i)", "lowest (cost[t], t)", "2^24", "2^47"):
        assert word in header, word


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    line, = [ln for ln in r.stdout.splitlines() if "--whole-line" in ln]
    assert r.returncode == 0 and "[extension]" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15", "--whole-line"]
    # no such image: a run that got past the arguments would fail on it with another exit code
    for other, named in ((["--scores", "/nonexistent/dir/scores.csv"], "--scores"), (["--pen-search", "4"], "--pen-search"),
                         (["--pen-search=64"], "--pen-search")):
        for args in (base + other, other + base):
            r = subprocess.run([focr_bin] + args + ["-i", "/nonexistent/page.pgm"], capture_output=True, text=True)
            assert r.returncode == 2 and "error:" in r.stderr and "--whole-line" in r.stderr and named in r.stderr, args
            assert "cannot be used with" in r.stderr and "Usage: focr" in r.stderr and r.stdout == ""
    r = subprocess.run([focr_bin] + base + ["--pen-search", "0"], capture_output=True, text=True)  # radius 0 is no search; no -i: nothing to do
    assert r.returncode == 0 and r.stdout == ""
    r = subprocess.run([focr_bin] + base[:-1] + ["--whole-lines"], capture_output=True, text=True)
    assert r.returncode == 2 and "unexpected argument" in r.stderr


def test_python_argument_checks():
    """whole_line goes with neither scores nor a pen search; the check comes before any device work."""
    check = LineDecoder._check_whole_line
    assert check(True, False, 0) is True and check(False, True, 8) is False and check(0, False, 0) is False
    with pytest.raises(ValueError, match="scores"):
        check(True, True, 0)
    with pytest.raises(ValueError, match="pen_search"):
        check(True, False, 1)
    import inspect
    for fn in (LineDecoder.decode, LineDecoder.decode_device):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "whole_line" and p["whole_line"].default is False

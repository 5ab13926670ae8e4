"""Host side of the focr pen search (include/focr_decode.h): the new entry points are declared, bound and exported, and
the CLI knows --pen-search and refuses a radius above 64 before it touches a device.  No GPU needed."""
import os
import re
import subprocess

import pytest

from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
NEW = ("focr_decoder_set_pen_search", "focr_decoder_get_offsets")


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    assert "FOCR_PEN_SEARCH_MAX = 64" in header
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (focr_\w+)", out))
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in N.DECODE_HIP_SYMBOLS and sym in exported, sym


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_error(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    line, = [ln for ln in r.stdout.splitlines() if "--pen-search" in ln]
    assert r.returncode == 0 and "[extension]" in line and "<N>" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    # no such image: a run that got past the arguments would fail on it with another exit code
    for bad in ("65", "1000", "-1", "x"):
        r = subprocess.run([focr_bin] + base + ["--pen-search", bad, "-i", "/nonexistent/page.pgm"], capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "--pen-search" in r.stderr and "Usage: focr" in r.stderr, bad
        assert r.stdout == ""
    r = subprocess.run([focr_bin] + base + ["--pen-search", "65"], capture_output=True, text=True)
    assert r.returncode == 2 and "at most 64" in r.stderr
    r = subprocess.run([focr_bin] + base + ["--pen-search", "64"], capture_output=True, text=True)  # no -i: nothing to do
    assert r.returncode == 0 and r.stdout == ""

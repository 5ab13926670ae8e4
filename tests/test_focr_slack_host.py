"""Host side of the focr whole-line pen slack (include/focr_decode.h): the new entry point is declared, bound and
exported, the library's refusals name both switches, the CLI knows --pen-slack and refuses its misuse before it touches
a device, and the Python API refuses the same combinations before any device work.  No GPU needed."""
import inspect
import os
import re
import subprocess

import pytest

from font_ocr_amd import LineDecoder
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
NEW = ("focr_decoder_set_whole_slack",)


@pytest.fixture(scope="module")
def hip_lib():
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    return hip


def test_symbols_declared_bound_and_exported(hip_lib):
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (focr_\w+)", out))
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in N.DECODE_HIP_SYMBOLS and sym in exported, sym
    assert N.DECODE_HIP_SYMBOLS["focr_decoder_set_whole_slack"][1][1] is __import__("ctypes").c_uint32
    for word in ("lowest (cost[p - j], rank(j))", "0 <= p - j < n_live", "G[t - inc64[i]].cost + term(i, t - inc64[i])",
                 "continue from t = p - j", "pens[q + 1] - offsets[q + 1] == pens[q] + inc64[idx[q]]",
                 "ceil(64 * width / (min inc64 - N))", "2 * N > min inc64"):
        assert word in header, word
    # the pen loop's search stays refused beside the whole-line decode
    assert "a pen search radius" in header


def test_refusal_messages_name_both_switches(hip_lib):
    """The two refusals of a combination of switches, as the library holds them: each names both setters."""
    text = open(hip_lib, "rb").read()
    msgs = [m.decode() for m in re.findall(rb"focr_decoder_run: pen slack on[^\0]*", text)]
    assert len(msgs) == 2 and len(set(msgs)) == 2, msgs
    off, = [m for m in msgs if "whole-line decode off" in m]
    both, = [m for m in msgs if "margins on" in m]
    assert "focr_decoder_set_whole_slack" in off and "focr_decoder_set_whole_line" in off
    assert "focr_decoder_set_whole_slack" in both and "focr_decoder_set_whole_margins" in both
    for word in (b"focr_decoder_set_whole_slack: the slack radius is at most 64", b"the pen slack is more than half the smallest inc64",
                 b"whole-line decode with pen slack: the widest advance and the slack are too large"):
        assert word in text, word


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin, tmp_path):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    line, = [ln for ln in r.stdout.splitlines() if "--pen-slack" in ln]
    assert r.returncode == 0 and "[extension]" in line and "<N>" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    csv = str(tmp_path / "margins.csv")
    # no such image: a run that got past the arguments would fail on it with another exit code
    cases = ((["--pen-slack", "8"], "cannot be used without", "--whole-line"),
             (["--pen-slack=8"], "cannot be used without", "--whole-line"),
             (["--whole-line", "--pen-slack", "8", "--margins", csv], "cannot be used with", "--margins"),
             (["--pen-slack", "8", "--pen-search", "4"], "cannot be used with", "--pen-search"))
    for extra, phrase, named in cases:
        for args in (base + extra, extra + base):
            r = subprocess.run([focr_bin] + args + ["-i", "/nonexistent/page.pgm"], capture_output=True, text=True)
            assert r.returncode == 2 and "error:" in r.stderr and "--pen-slack" in r.stderr and named in r.stderr, (args, r.stderr)
            assert phrase in r.stderr and "Usage: focr" in r.stderr and r.stdout == ""
            assert not os.path.exists(csv)
    for bad in ("65", "-1", "x"):
        r = subprocess.run([focr_bin] + base + ["--whole-line", "--pen-slack", bad, "-i", "/nonexistent/page.pgm"], capture_output=True, text=True)
        assert r.returncode == 2 and "invalid value '%s' for '--pen-slack'" % bad in r.stderr, bad
    r = subprocess.run([focr_bin] + base + ["--whole-line", "--pen-slack"], capture_output=True, text=True)
    assert r.returncode == 2 and "a value is required for '--pen-slack'" in r.stderr
    # a radius of 0 is no slack and passes everywhere; with --whole-line a radius passes, and no -i means nothing to do
    for extra in (["--pen-slack", "0"], ["--pen-slack", "0", "--pen-search", "4"], ["--whole-line", "--pen-slack", "8"]):
        r = subprocess.run([focr_bin] + base + extra, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == "", extra
    # with --whole-line the arguments pass and the missing image is what fails
    r = subprocess.run([focr_bin] + base + ["--whole-line", "--pen-slack", "8", "-i", "/nonexistent/page.pgm"], capture_output=True, text=True)
    assert r.returncode not in (0, 2)


def test_python_argument_checks():
    """pen_slack needs whole_line and refuses margins; both checks, and the old ones, come before any device work (a
    decoder needs a device, and none is made here)."""
    check = LineDecoder._check_pen_slack
    assert check(0, False, False) == 0 and check(8, True, False) == 8 and check(64, True, False) == 64 and check(0, True, True) == 0
    with pytest.raises(ValueError, match="pen_slack.*whole_line"):
        check(8, False, False)
    with pytest.raises(ValueError, match="pen_slack.*margins"):
        check(8, True, True)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="0 .. 64"):
            check(bad, True, False)
    # whole_line=True, pen_search=8 still raises the old error, from the old check with its old signature
    assert list(inspect.signature(LineDecoder._check_whole_line).parameters) == ["whole_line", "scores", "pen_search"]
    with pytest.raises(ValueError, match=r"whole_line=True does not go with pen_search \(the dynamic programme does not search offsets\)"):
        LineDecoder._check_whole_line(True, False, 8)
    for fn in (LineDecoder.decode, LineDecoder.decode_device):
        p = inspect.signature(fn).parameters
        assert p["pen_slack"].default == 0 and list(p).index("pen_slack") == list(p).index("pen_search") + 1
    # decode() itself checks before it touches the library: an object with no library behind it gets as far as the checks
    dec = object.__new__(LineDecoder)
    dec.font, dec._h = object(), None
    with pytest.raises(ValueError, match="pen_slack.*whole_line"):
        dec.decode([], 0, 0, 10, 10, 10, pen_slack=8)
    with pytest.raises(ValueError, match="pen_slack.*margins"):
        dec.decode([], 0, 0, 10, 10, 10, whole_line=True, margins=True, pen_slack=8)
    with pytest.raises(ValueError, match="does not go with pen_search"):
        dec.decode([], 0, 0, 10, 10, 10, whole_line=True, pen_search=8, pen_slack=8)
    with pytest.raises(ValueError, match="pen_slack.*whole_line"):
        dec.decode_device(0, 1, 10, 10, 0, 0, 10, 10, 10, pen_slack=8)

"""Host side of the focr whole-line margins (include/focr_decode.h): the new entry points are declared, bound and
exported, the CLI knows --margins and refuses it without --whole-line before it touches a device, and the Python API
refuses the same combination before any device work.  No GPU needed."""
import inspect
import os
import re
import subprocess

import pytest

import font_ocr_amd
from font_ocr_amd import LineDecoder, LineMargins
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
NEW = ("focr_decoder_set_whole_margins", "focr_decoder_get_margins")


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
    struct = re.search(r"typedef struct focr_char_margin \{(.*?)\} focr_char_margin_t;", header, re.S).group(1)
    assert [f.split()[-1] for f in struct.split(";") if f.strip()] == ["term", "runner", "pad", "margin"]
    for word in ("m_k = s_k + (inc64[i_k] >> 1)", "s <= m_k < s + inc64[i]", "T(s, i) = F[s] + term(i, s) + B[s + inc64[i]]",
                 "lowest (T, i)", "0xFFFF and margin = -1"):
        assert word in header, word
    # whole-line with scores stays refused as it was
    assert "scores on (a runner-up has no definition under a dynamic programme yet)" in header


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin, tmp_path):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    line, = [ln for ln in r.stdout.splitlines() if "--margins" in ln]
    assert r.returncode == 0 and "[extension]" in line and "<MARGINS>" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    csv = str(tmp_path / "margins.csv")
    # no such image: a run that got past the arguments would fail on it with another exit code
    for margins in (["--margins", csv], ["--margins=" + csv]):
        for args in (base + margins, margins + base):
            r = subprocess.run([focr_bin] + args + ["-i", "/nonexistent/page.pgm"], capture_output=True, text=True)
            assert r.returncode == 2 and "error:" in r.stderr and "--margins" in r.stderr and "--whole-line" in r.stderr, args
            assert "cannot be used without" in r.stderr and "Usage: focr" in r.stderr and r.stdout == ""
            assert not os.path.exists(csv)
    # with --whole-line, in either order, the arguments pass and the missing image is what fails
    for args in (base + ["--whole-line", "--margins", csv], ["--margins", csv, "--whole-line"] + base):
        r = subprocess.run([focr_bin] + args + ["-i", "/nonexistent/page.pgm"], capture_output=True, text=True)
        assert r.returncode not in (0, 2) and "Usage: focr" not in r.stderr, args
    r = subprocess.run([focr_bin] + base + ["--whole-line", "--margins"], capture_output=True, text=True)
    assert r.returncode == 2 and "a value is required for '--margins'" in r.stderr
    # whole-line with scores is still the usage error it was
    r = subprocess.run([focr_bin] + base + ["--whole-line", "--margins", csv, "--scores", csv + "2", "-i", "/nonexistent/page.pgm"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "'--whole-line' cannot be used with '--scores <SCORES>'" in r.stderr


def test_python_argument_checks():
    """margins needs whole_line; the check comes before any device work; _check_whole_line is what it was."""
    check = LineDecoder._check_margins
    assert check(True, True) is True and check(False, True) is False and check(0, False) is False
    with pytest.raises(ValueError, match="whole_line"):
        check(True, False)
    assert list(inspect.signature(LineDecoder._check_whole_line).parameters) == ["whole_line", "scores", "pen_search"]
    with pytest.raises(ValueError, match="a runner-up has no definition under the dynamic programme"):
        LineDecoder._check_whole_line(True, True, 0)
    for fn in (LineDecoder.decode, LineDecoder.decode_device):
        p = inspect.signature(fn).parameters
        assert p["margins"].default is False and list(p)[-2:] == ["margins", "whole_line"]
    # a decoder that was never created: the refusal must come before anything touches it
    dec = LineDecoder.__new__(LineDecoder)
    dec.font, dec._h = object(), None
    with pytest.raises(ValueError, match="margins=True needs whole_line=True"):
        dec.decode([], 0, 0, 10, 10, 10, margins=True)
    with pytest.raises(ValueError, match="margins=True needs whole_line=True"):
        dec.decode_device(0, 1, 10, 10, 0, 0, 10, 10, 10, margins=True)
    assert LineMargins._fields == ("term", "runner", "margin") and LineMargins.NO_RUNNER == "\0"
    assert font_ocr_amd.LineMargins is LineMargins

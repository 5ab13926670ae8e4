"""Host side of the focr decoder's font search (include/focr_decode.h): the new entry points declared, bound and exported, the
Python signatures and refusals, and the CLI's spec parser and usage errors before it touches a device.  No GPU needed."""
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
SYMBOLS = {"focr_decoder_set_font_candidates": r"\(focr_decoder_t \*dec, const focr_decode_font_t \*fonts, uint32_t n\);",
           "focr_decoder_set_font_search": r"\(focr_decoder_t \*dec, int on\);",
           "focr_decoder_get_fonts": r"\(const focr_decoder_t \*dec, uint8_t \*font, int64_t \*cost\);",
           "focr_decoder_debug_set_fonts_grid": r"\(focr_decoder_t \*dec, uint32_t grid\);"}


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (focr_\w+)", out))
    for name, args in SYMBOLS.items():
        assert re.search(r"\bint %s\s*%s" % (name, args), header), name
        assert name in N.DECODE_HIP_SYMBOLS and len(N.DECODE_HIP_SYMBOLS[name][1]) == args.count(",") + 1, name
        assert name in exported, name
    assert re.search(r"enum \{ FOCR_FONT_CANDIDATES_MAX = 16 \};", header)
    # the definition names both forms, the winner's rule, every refusal and what it does not cure
    section = header[header.index("device: font candidates"): header.index("int focr_decoder_set_font_candidates")]
    for word in ("Candidate 0 is the decode", "trunc((origin_x_k + pos) * 64)", "focr_decoder_set_whole_line", "(cost_k, k)", "focr_decoder_get_fonts",
                 "focr_decoder_get_pens", "launch count stays 3", "no candidates uploaded", "scores, a pen search, margins, a pen slack, a baseline search",
                 "\"yet\"", "candidate's index", "2^24", "2^47", "focr_decoder_verify after a font-search run is refused", "What it does not cure",
                 "monospace tool", "focr --verify of a mixed-font run", "different alphabets"):
        assert word in section, word


def test_python_signatures_and_refusals():
    for fn in (LineDecoder.decode, LineDecoder.decode_device):
        assert inspect.signature(fn).parameters["font_search"].default is False
    assert list(inspect.signature(LineDecoder.set_font_candidates).parameters) == ["self", "fonts"]
    dec = object.__new__(LineDecoder)  # no device: the refusals come before anything touches the library
    dec.font = object()
    dec._candidates = [object()]
    page = np.full((16, 40), 255, dtype=np.uint8)
    geo = (0, 0, 40, 16, 16)
    for kw, what in ((dict(scores=True), "scores=True"), (dict(pen_search=4), "pen_search"), (dict(whole_line=True, margins=True), "margins=True"),
                     (dict(whole_line=True, pen_slack=4), "pen_slack"), (dict(baseline_search=2), "baseline_search"),
                     (dict(whole_line=True, whole_baseline=2), "whole_baseline"), (dict(verify="mse"), "verify"), (dict(verify="image"), "verify")):
        with pytest.raises(ValueError, match="font_search=True does not go with " + re.escape(what) + " yet"):
            dec.decode([page], *geo, font_search=True, **kw)
        with pytest.raises(ValueError, match="font_search=True does not go with " + re.escape(what) + " yet"):
            dec.decode_device(0, 1, 16, 40, *geo, font_search=True, **kw)
    # a fractional grid is refused by its own rule, and the older refusals keep their words
    with pytest.raises(ValueError, match="y_frac and line_advance_frac need baseline_search or whole_baseline"):
        dec.decode([page], *geo, font_search=True, y_frac=3)
    with pytest.raises(ValueError, match="margins=True needs whole_line=True"):
        dec.decode([page], *geo, font_search=True, margins=True)
    dec._candidates = []
    with pytest.raises(ValueError, match=r"font_search=True needs candidates \(set_font_candidates\)"):
        dec.decode([page], *geo, font_search=True)
    with pytest.raises(ValueError, match="at most 15 font candidates"):
        dec.set_font_candidates([object()] * 16)
    dec._h = None


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--font-candidate ")]
    assert "[extension]" in line and "<SPEC>" in line and "f=PATH,t=SIZE,k=KERNING,h=0|1" in line and "at most 15" in line
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--fonts ")]
    assert "[extension]" in line and "only with --font-candidate" in line
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    img = ["-i", "/nonexistent/page.pgm"]  # a run that got past the arguments would fail on it with another exit code
    cand = ["--font-candidate", "t=12"]
    for extra, words in ((["--font-candidate", ""], ("--font-candidate",)),
                         (["--font-candidate", "t="], ("--font-candidate", "'t' has no value")),
                         (["--font-candidate", "t=12,,h=1"], ("--font-candidate",)),
                         (["--font-candidate", "t=12,"], ("--font-candidate",)),
                         (["--font-candidate", "t=12,t=13"], ("--font-candidate", "'t' is given twice")),
                         (["--font-candidate", "f=a.ttf,h=1,f=b.ttf"], ("--font-candidate", "'f' is given twice")),
                         (["--font-candidate", "s=12"], ("--font-candidate", "s=12")),
                         (["--font-candidate", "h=2"], ("--font-candidate", "'h'")),
                         (["--font-candidate", "t=big"], ("--font-candidate", "'t'")),
                         (["--font-candidate", "k=1.0x"], ("--font-candidate", "'k'")),
                         (cand * 16, ("--font-candidate", "more than 15 times")),
                         (["--fonts", "/dev/null"], ("--fonts", "--font-candidate")),
                         (cand + ["--scores", "/dev/null"], ("--font-candidate", "--scores")),
                         (cand + ["--pen-search", "4"], ("--font-candidate", "--pen-search")),
                         (cand + ["--whole-line", "--pen-slack", "4"], ("--font-candidate", "--pen-slack")),
                         (cand + ["--whole-line", "--margins", "/dev/null"], ("--font-candidate", "--margins")),
                         (cand + ["--baseline-search", "4"], ("--font-candidate", "--baseline-search")),
                         (cand + ["--whole-line", "--whole-baseline", "4"], ("--font-candidate", "--whole-baseline")),
                         (cand + ["--verify", "/tmp"], ("--font-candidate", "--verify"))):
        r = subprocess.run([focr_bin] + base + extra + img, capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "Usage: focr" in r.stderr and r.stdout == "", (extra, r.stderr)
        assert all(w in r.stderr for w in words), (extra, r.stderr)
    for extra in (cand * 15 + ["--fonts", "/dev/null"], ["--font-candidate", "f=%s,t=12.5,k=1.05,h=1" % MONO, "--whole-line"]):
        r = subprocess.run([focr_bin] + base + extra, capture_output=True, text=True)  # no -i: nothing to do
        assert r.returncode == 0 and r.stdout == "", (extra, r.stderr)

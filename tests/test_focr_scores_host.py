"""Host side of the focr decoder's scores: the C ABI and its ctypes mirror, the CLI flag, and the yardstick of the GPU
tests (tests/focr_scores_model.py) pinned to the reference's score_glyph by a brute-force ranking."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import focr_scores_model as S
from focr_fast_model import FastModel
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineScores
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
CSRC = os.path.join(ROOT, "font_ocr_amd", "csrc")


def test_library_exports_scores():
    hip = os.path.join(N.LIB_DIR, "libfocr_hip.so")
    if not os.path.exists(hip):
        subprocess.run(["make", "-s", "-C", CSRC, "hip"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", hip], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (focr_\w+)", out))
    assert {"focr_decoder_set_scores", "focr_decoder_get_scores"} <= exported
    assert {"focr_decoder_set_scores", "focr_decoder_get_scores"} <= set(N.DECODE_HIP_SYMBOLS)


def test_char_score_layout():
    assert C.sizeof(N.CharScore) == 24
    assert [(n, getattr(N.CharScore, n).offset) for n, _ in N.CharScore._fields_] == [("score", 0), ("runner_score", 8), ("runner", 16),
                                                                                     ("pad", 18)]
    assert LineScores._fields == ("base", "score", "runner", "runner_score")


def test_cli_help_names_scores():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", CSRC, "cli"], check=True)
    r = subprocess.run([FOCR, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    line, = [ln for ln in r.stdout.splitlines() if "--scores" in ln]
    assert "[extension]" in line


def test_cli_unwritable_scores_path(tmp_path):
    """An unwritable --scores path is a usage error (exit code 2), before the font is even read."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", CSRC, "cli"], check=True)
    r = subprocess.run([FOCR, "-f", str(tmp_path / "no-such-font.ttf"), "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15",
                        "--scores", str(tmp_path / "no-such-dir" / "out.csv"), "-i", str(tmp_path / "no-such-page.pgm")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--scores" in r.stderr and r.stdout == ""


def test_scores_model_equals_brute_force():
    """One 120x16 line of Mono 13 px, default alphabet: the fast model's top-2 by (score, index) is the top-2 of one
    FreeType raster per candidate with the full-canvas SSD, and base is the crop's sum of r^2."""
    size = 13.0
    page = np.full((16, 120), 255, dtype=np.uint8)
    S.draw(page, MONO, size, "l1I O0 ab+/=", 0, 0)
    fm = FastModel(MONO, size, FOCR_DEFAULT_ALPHABET)
    got = S.line_scores(fm, page)
    fm.close()
    want = S.brute_line_scores(page, MONO, size, FOCR_DEFAULT_ALPHABET)
    assert got.text == want.text and len(got.text) > 12
    assert got.base == want.base == int(((255 - page.astype(np.int64)) ** 2).sum())
    for a, b in zip(got[2:], want[2:]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.all(got.runner_score >= got.score) and np.all(got.runner != [FOCR_DEFAULT_ALPHABET.index(c) for c in got.text])
    assert "l1I" in got.text

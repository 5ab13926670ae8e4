"""The verify images of the `ncc` path without a device: the numpy model (tests/ncc_verify_model.py) on three cases whose images
are written out here, the host library's PNG writer, and the `ncc` CLI's --verify surface."""
import os
import subprocess

import numpy as np
import pytest

from font_ocr_amd import Bank
from font_ocr_amd import _native as N
from font_ocr_amd.bank import HIT_DTYPE, TEMPLATE_DTYPE, load_image, load_image_rgba
from font_ocr_amd.searcher import verify_mse
from ncc_verify_model import triple_of, verify_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCC = os.path.join(ROOT, "font_ocr_amd", "bin", "ncc")


def _bank(needles):
    tm = np.zeros(len(needles), TEMPLATE_DTYPE)
    off = 0
    for i, nd in enumerate(needles):
        tm[i]["letter"], tm[i]["n_w"], tm[i]["n_h"], tm[i]["offset"] = 65 + i, nd.shape[1], nd.shape[0], off
        off += nd.size
    return Bank(tm, np.concatenate([np.asarray(nd, np.uint8).reshape(-1) for nd in needles]), len(needles), 0, 0, 13.0, 8.0)


def _chars(rows):
    out = np.zeros(len(rows), HIT_DTYPE)
    for i, (x, y, w, h, t) in enumerate(rows):
        out[i] = (x, y, w, h, 0.99, 65 + t, t)
    return out


def test_one_character_on_a_6x5_page():
    bank = _bank([np.array([[255, 0, 10], [1, 128, 0]], np.uint8)])
    ink = np.zeros((1, 5, 6), np.uint8)
    ink[0, 1, 2] = 255  # black under the glyph's full ink: red 0, blue 0
    ink[0, 1, 3] = 55   # grey under a glyph hole: red 200 stays alone
    ink[0, 4, 0] = 5    # grey away from the glyph
    rgb, sums = verify_model(ink, bank, [0, 1], [0, 1], _chars([(2, 1, 3, 2, 0)]))
    red = [[0, 0, 0, 0, 0, 0], [0, 0, 0, 200, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [250, 0, 0, 0, 0, 0]]
    blue = [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 245, 0], [0, 0, 254, 127, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    assert rgb[0, :, :, 0].tolist() == red and rgb[0, :, :, 2].tolist() == blue and not rgb[..., 1].any()
    assert sums.dtype == np.uint64 and sums.tolist() == [200 ** 2 + 245 ** 2 + 254 ** 2 + 127 ** 2 + 250 ** 2]


def test_a_later_character_wins_only_where_it_has_ink():
    bank = _bank([np.full((2, 3), 100, np.uint8), np.array([[200, 0, 200], [0, 200, 0]], np.uint8)])
    ink = np.zeros((1, 3, 5), np.uint8)
    chars = _chars([(0, 0, 3, 2, 0), (1, 0, 3, 2, 1)])  # one line, x ascending: the second overlaps the first by two columns
    rgb, sums = verify_model(ink, bank, [0, 1], [0, 2], chars)
    assert rgb[0, :, :, 2].tolist() == [[155, 55, 155, 55, 0], [155, 155, 55, 0, 0], [0, 0, 0, 0, 0]]  # the hole shows 155
    assert sums.tolist() == [4 * 155 ** 2 + 3 * 55 ** 2]
    back, _ = verify_model(ink, bank, [0, 1], [0, 2], chars, reverse=True)
    assert back[0, :, :, 2].tolist() == [[155, 155, 155, 55, 0], [155, 155, 155, 0, 0], [0, 0, 0, 0, 0]]


def test_an_uncovered_pixel_of_luma_0_adds_nothing():
    bank = _bank([np.full((1, 1), 255, np.uint8)])
    ink = np.zeros((2, 2, 2), np.uint8)
    ink[0, 0, 0] = 255  # luma 0, uncovered: red 0, blue 0 (the reference's quirk, kept)
    ink[0, 1, 1] = 254  # luma 1
    rgb, sums = verify_model(ink, bank, [0, 0, 0], [0], _chars([]))
    assert rgb[0, :, :, 0].tolist() == [[0, 0], [0, 1]] and not rgb[..., 1:].any()
    assert sums.tolist() == [1, 0]
    assert verify_mse(sums, 2, 2).dtype == np.float32 and verify_mse(sums, 2, 2).tolist() == [0.25, 0.0]
    assert verify_mse(np.array([2 ** 40 + 1], np.uint64), 3, 1)[0] == np.float32(2 ** 40 + 1) / np.float32(3)


def test_triple_of_lines():
    lines = [[_chars([(1, 2, 3, 2, 0)]), _chars([(1, 9, 3, 2, 0), (5, 9, 3, 2, 0)])], [], [_chars([(0, 0, 3, 2, 0)])]]
    po, lo, ch = triple_of(lines)
    assert po.tolist() == [0, 2, 2, 3] and lo.tolist() == [0, 1, 3, 4] and ch["y"].tolist() == [2, 9, 9, 0]


def test_png_writer_round_trips_grey_rgb_and_rgba(tmp_path):
    """focr_image_save_png (the writer `ncc` and `focr` share) against the host library's own decoder."""
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (7, 3), (301, 5)):
        for ch in (1, 3, 4):
            px = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
            path = str(tmp_path / f"p{w}_{ch}.png")
            assert N.host().focr_image_save_png(path.encode(), px.ctypes.data, w, h, ch) == 0
            got = load_image_rgba(path)
            want = np.concatenate([np.repeat(px, 3, axis=2), np.full((h, w, 1), 255, np.uint8)], axis=2) if ch == 1 else \
                np.concatenate([px, np.full((h, w, 1), 255, np.uint8)], axis=2) if ch == 3 else px
            assert np.array_equal(got, want), (w, h, ch)
            if ch == 1:
                assert np.array_equal(load_image(path), px[..., 0])
    px = np.zeros((2, 2, 3), np.uint8)
    assert N.host().focr_image_save_png(str(tmp_path / "x.png").encode(), px.ctypes.data, 2, 2, 2) != 0  # no such pixel format
    assert N.host().focr_image_save_png(str(tmp_path / "no" / "x.png").encode(), px.ctypes.data, 2, 2, 3) != 0


@pytest.fixture(scope="module")
def ncc_bin():
    if not os.path.exists(NCC):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return NCC


def test_cli_help_lists_verify(ncc_bin):
    r = subprocess.run([ncc_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if "--verify" in l]
    assert len(line) == 1 and "[extension]" in line[0]


def test_cli_verify_is_refused_before_a_device_is_touched(ncc_bin, tmp_path):
    """--verify with --raw, and a DIR that is no directory: exit 2 with the flag named, before the font is even opened (the font
    does not exist: reaching the rasteriser would exit 101)."""
    base = [ncc_bin, "-f", "/nonexistent.ttf", "-t", "13"]
    r = subprocess.run(base + ["--verify", str(tmp_path), "--raw", "-i", "x.pgm"], capture_output=True, text=True)
    assert r.returncode == 2 and "--verify" in r.stderr and "--raw" in r.stderr and "unexpected argument" not in r.stderr
    r = subprocess.run(base + ["--verify", "/nonexistent", "-i", "x.pgm"], capture_output=True, text=True)
    assert r.returncode == 2 and "--verify should be a dir" in r.stderr
    file = tmp_path / "plain"
    file.write_text("x")
    r = subprocess.run(base + ["--verify=" + str(file), "-i", "x.pgm"], capture_output=True, text=True)
    assert r.returncode == 2 and "--verify should be a dir" in r.stderr
    r = subprocess.run(base + ["--verify", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 101  # accepted: the run goes on to the font, which is not there

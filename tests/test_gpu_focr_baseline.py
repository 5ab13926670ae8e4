"""The focr decoder's baseline search (line_baseline_kernel, focr_decoder_set_baseline_fonts / _set_baseline_search /
_get_baselines, LineDecoder.decode(baseline_search=N), focr --baseline-search) against tests/focr_baseline_model.py, the
definition of include/focr_decode.h restated on the fast model and pinned to FreeType by
tests/test_focr_baseline_model.py.  Every quantity is an exact integer or an f32 computed by stated operations, so every
comparison is ==.  Each test asserts from its geometry, or from the model's answer, that it reaches the case it names."""
import csv
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import focr_baseline_model as B
import focr_fuzz_cases as FZ
from focr_fast_model import permuted_319
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder, VerifyFont, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536   # decode_line.h: a strip of up to this many bytes is staged in LDS
BASE_RED_BYTES = 64     # decode_baseline.hip: the waves' (cost, rank) pairs share that LDS with the strip
B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/="
ALPHABETS = {"2": "AB", "64": B64[:64], "65": B64, "319": permuted_319()}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


@functools.lru_cache(maxsize=None)
def model(font, size, alphabet, y_bits, hinting=False, kerning=1.0):
    return B.BaselineModel(font, size, alphabet, hinting, kerning, y_bits)


def strip_bytes(page_w, x, width, line_height):
    w = min(width, page_w - min(x, page_w))
    return ((w + 7) // 4 + 2) * 4 * line_height


def _check(dec, m, pages, geo, n):
    """Decode with radius n in steps of 2^-m.y_bits px: line order, texts, q and costs equal to the model's.  Returns
    the model's [[(y, Baseline)] per page]."""
    want = [m.search_image(p, *geo, n) for p in pages]
    lines, qs, costs = dec.decode(pages, *geo, baseline_search=n)
    assert lines == [[(y, b.text) for y, b in pg] for pg in want]
    assert qs == [[b.q for _, b in pg] for pg in want]
    assert costs == [[b.cost for _, b in pg] for pg in want]
    return want


def _offset_pages(font, size, alphabet, offsets, W=120, seed=0, n_chars=13):
    """One page per row of `offsets`: 16-row slots, slot s inked with random text `offsets[p][s]` px below the crop's
    baseline (None: blank), and three rows of a further slot that the page's bottom cuts."""
    rng = np.random.default_rng(seed)
    ink = [c for c in alphabet if not c.isspace()]
    pages = []
    for row in offsets:
        page = np.full((16 * len(row) + 3, W), 255, dtype=np.uint8)
        for s, off in enumerate(row):
            if off is not None:
                B.draw_offset(page, font, size, alphabet, "".join(rng.choice(ink, n_chars)), 2, 16 * s, off)
        pages.append(page)
    return pages


@pytest.mark.parametrize("n,y_bits,alphabet", [(1, 0, "2"), (1, 2, "65"), (2, 2, "64"), (4, 3, "65"), (4, 2, "319"), (32, 0, "64"), (32, 2, "2"),
                                                (32, 3, "65")])
def test_parity(dec, n, y_bits, alphabet):
    """3 candidates (one wave idle), 5 (uneven), 9 and 65, at B = 0, 2 and 3, with 2, 64, 65 and 319 glyphs (a partial, a
    full, a second and a fifth stripe of the wave's glyph loop).  Lines sit up to 1.3 px off the baseline either way,
    between blank slots; the page's bottom cuts the last slot to three rows."""
    al = ALPHABETS[alphabet]
    pages = _offset_pages(MONO, 13.0, al, [(0.75, -1.0, None, 1.3), (-0.25, 0.0, 0.5, None)], seed=n + y_bits)
    m = model(MONO, 13.0, al, y_bits)
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, pages, (2, 0, 118, 16, 16), n)
    assert [[y for y, _ in pg if y < 64] for pg in want] == [[0, 16, 48], [0, 16, 32]]
    # the three rows of the first page's last slot, cut by the page's bottom, take ink only from the 319's deepest glyphs
    assert [y for y, _ in want[0] if y >= 64] == ([64] if alphabet == "319" else [])
    qs = [b.q for pg in want for _, b in pg]
    assert min(qs) < 0 < max(qs) and all(abs(q) <= n for q in qs)
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3


def test_ties_in_the_319_glyph_alphabet(dec):
    """The tie alphabet: where a group of identical glyphs wins a step, its first member by index does, under every
    candidate; device and model agree on text, q and cost."""
    al = ALPHABETS["319"]
    page = np.full((32, 100), 255, dtype=np.uint8)
    B.draw_offset(page, SANS, 13.0, al, "AoxAo oA", 0, 0, 1.0)
    B.draw_offset(page, SANS, 13.0, al, "oAAo xA", 0, 16, -0.5)
    m = model(SANS, 13.0, al, 2)
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, [page], (0, 0, 100, 16, 16), 4)[0]
    text = "".join(b.text for _, b in want)
    assert [b.q for _, b in want] == [4, -2]
    for grp in ("AΑА", "oοо"):
        first = min(grp, key=al.index)
        assert first in text and not set(grp) - {first} & set(text), grp


@pytest.mark.parametrize("y_bits", [0, 2])
def test_dropped_candidates(dec, y_bits):
    """Mono 6 px has origin_y 5: with N = 32 the candidates with ty_q < 0 (q < -5 at B = 0, q < -20 at B = 2) are dropped,
    and a line drawn 4 px above the baseline takes one of the last negative q that remain."""
    m = model(MONO, 6.0, B64, y_bits)
    assert float(m.oy) == 5.0 and m.dropped(-(5 << y_bits) - 1) and not m.dropped(-(5 << y_bits)) and (5 << y_bits) < 32
    page = np.full((24, 80), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 6.0, B64, "dropped+cands", 0, 0, -4.0)
    B.draw_offset(page, MONO, 6.0, B64, "kept/below=", 0, 12, 3.0)
    dec.set_font(m.font, 6.0)
    want = _check(dec, m, [page], (0, 0, 80, 12, 12), 32)[0]
    up, down = (b.q / (1 << y_bits) for _, b in want)
    assert -5 <= up <= -3.5 and 2.5 <= down <= 3.5


def test_every_glyph_pushed_off_the_crop(dec):
    """Mono 13 px without descenders, 16-row crops, B = 0, N = 32: origin_y is 10, so q = -10 is the last candidate upwards
    and moves every box above row 0, and q >= 16 moves every box below the last row: those candidates cost 0 and read the
    first glyph all along, on the device as in the model, and the search still finds the lines at +2 and -3."""
    al = "ABx0"
    m = model(MONO, 13.0, al, 0)
    page = np.full((32, 60), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, al, "ABxB0A", 0, 0, 2.0)
    B.draw_offset(page, MONO, 13.0, al, "x0ABBA", 0, 16, -3.0)
    assert float(m.oy) == 10.0
    for q in (-10, 16, 32):
        assert m.decode_line_q(page[:16], q) == ("A" * 8, 0)
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, [page], (0, 0, 60, 16, 16), 32)[0]
    assert [b.q for _, b in want] == [2, -3] and [b.text[:6] for _, b in want] == ["ABxB0A", "x0ABBA"]
    # a crop of three rows: only the rows a candidate leaves inside it count, whichever way it is pushed
    _check(dec, m, [page], (0, 5, 60, 3, 16), 32)


def test_all_tie_line(dec):
    """Ink out of every glyph's reach and a space in the alphabet: every candidate costs the same, so q = 0 wins."""
    m = model(MONO, 13.0, " AB", 2)
    page = np.full((16, 40), 255, dtype=np.uint8)
    page[15, :] = 0
    dec.set_font(m.font, 13.0)
    (_, b), = _check(dec, m, [page], (0, 0, 40, 16, 16), 4)[0]
    assert b.q == 0 and b.cost == 0 and set(b.text) == {" "}


def test_line_height_one_and_a_cut_last_slot(dec):
    """line_height 1 with line_advance 3: every crop is one row.  Then 16-row slots on a page of 37 rows: the third
    slot keeps five rows."""
    m = model(MONO, 13.0, B64, 2)
    page = _offset_pages(MONO, 13.0, B64, [(0.5, -0.75)], W=90, n_chars=10)[0]
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, [page], (2, 0, 88, 1, 3), 8)[0]
    assert len(want) >= 8 and len({b.q for _, b in want}) > 2
    tall = np.full((37, 90), 255, dtype=np.uint8)
    B.draw_offset(tall, MONO, 13.0, B64, "cut+by+the", 2, 32, -6.0)  # moved up so that its ink lies in the five rows
    B.draw_offset(tall, MONO, 13.0, B64, "whole/line", 2, 0, 0.25)
    want = _check(dec, m, [tall], (2, 0, 88, 16, 16), 32)[0]
    assert [y for y, _ in want] == [0, 32] and want[0][1].q == 1 and want[1][1].q < -8


@pytest.mark.parametrize("width", [1008, 1012])
def test_lds_and_global_strip(dec, width):
    """Sans 24 px in 64-row slots.  The strip shares LDS with the waves' pairs: 1008 columns are the last strip staged in
    LDS (65280 + 64 bytes), 1012 already read global memory (65536 + 64)."""
    font, size, lh = SANS, 24.0, 64
    sb = strip_bytes(1013, 0, width, lh)
    assert (sb + BASE_RED_BYTES <= LDS_STRIP_MAX) == (width == 1008) and sb <= LDS_STRIP_MAX
    rng = np.random.default_rng(31)
    page = np.full((2 * lh, 1013), 255, dtype=np.uint8)
    for s, off in enumerate((1.0, -1.0)):
        B.draw_offset(page, font, size, FOCR_DEFAULT_ALPHABET, "".join(rng.choice(list(B64), 85)), 0, s * lh + 20, off)
    page[:, 1007:] = np.minimum(page[:, 1007:], 200)  # ink in the columns the widths differ by
    m = model(font, size, FOCR_DEFAULT_ALPHABET, 0)
    dec.set_font(m.font, size)
    want = _check(dec, m, [page], (0, 20, width, lh, lh), 1)[0]
    assert [(y, b.q) for y, b in want] == [(20, 1), (84, -1)] and all(len(b.text) > 60 for _, b in want)


def test_several_lines_per_workgroup_and_a_blank_page(dec):
    """Three pages, the middle one blank, six lines in all: with the debug grid at 1, 2 and 4 a workgroup takes six, three
    and two or one lines in turn, and the result is the one-line-per-workgroup run's."""
    m = model(MONO, 13.0, B64, 2)
    pages = _offset_pages(MONO, 13.0, B64, [(0.5, -0.5, 1.0, None), (None, None, None, None), (-1.25, None, 0.25, 1.5)], W=100, n_chars=11, seed=5)
    dec.set_font(m.font, 13.0)
    geo = (2, 0, 98, 16, 16)
    want = _check(dec, m, pages, geo, 6)
    assert [len(pg) for pg in want] == [3, 0, 3]
    free = dec.decode(pages, *geo, baseline_search=6)
    try:
        for grid in (1, 2, 4):
            assert dec._lib.focr_decoder_debug_set_baseline_grid(dec._h, grid) == 0
            assert dec.decode(pages, *geo, baseline_search=6) == free
    finally:
        assert dec._lib.focr_decoder_debug_set_baseline_grid(dec._h, 0) == 0


@pytest.mark.parametrize("i", range(12))
def test_fuzz_cases(dec, i):
    """The first dozen cases of tests/focr_fuzz_cases.py (fonts, sizes, kernings, hinting, crops that the page clips,
    pages of two sizes, salted ink up to 0.4 px off the baseline), at B = 2, N = 4."""
    c = FZ.case(i)
    m = model(c.font, c.size, c.alphabet, 2, c.hinting, c.kerning)
    dec.set_font(m.font, c.size)
    want = _check(dec, m, c.pages, c.geo, 4)
    assert sum(len(pg) for pg in want) > 0


def _baselines(d):
    n = d._lib.focr_decoder_n_lines(d._h)
    q, cost = np.full(max(n, 1), 99, dtype=np.int8), np.zeros(max(n, 1), dtype=np.int64)
    rc = d._lib.focr_decoder_get_baselines(d._h, q.ctypes.data, cost.ctypes.data)
    return rc, q[:n], cost[:n]


def test_radius_zero_is_the_plain_decoder(dec):
    """N = 0 with y-phase fonts uploaded, before and after a searched run, against a decoder that never heard of them:
    lines, verify images and sums and the launch count are the same, and focr_decoder_get_baselines fails."""
    font, size, geo = MONO, 13.0, (2, 0, 118, 16, 16)
    pages = _offset_pages(font, size, FOCR_DEFAULT_ALPHABET, [(0.75, -1.0, None, 1.3)], seed=3)
    with LineDecoder(0) as fresh:
        fresh.set_font(font, size)
        lines, mse, images = fresh.decode(pages, *geo, verify="image")
        launches = fresh._lib.focr_decoder_last_launches(fresh._h)
    dec.set_font(font, size, y_bits=2)
    assert dec._lib.focr_decoder_set_baseline_search(dec._h, 2, 0) == 0
    dec._baseline = (2, 0)
    for again in (False, True):
        got = dec.decode(pages, *geo, verify="image", baseline_search=0)
        assert len(got) == 3 and got[0] == lines and got[1].tobytes() == mse.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(got[2], images))
        assert dec._lib.focr_decoder_last_launches(dec._h) == launches == 3
        rc, _, _ = _baselines(dec)
        assert rc != 0 and b"focr_decoder_set_baseline_search" in dec._lib.focr_decoder_last_error(dec._h)
        if not again:
            searched, qs, _ = dec.decode(pages, *geo, baseline_search=8)
            assert searched != lines and qs == [[3, -4, 5]] and _baselines(dec)[0] == 0
            assert list(_baselines(dec)[1]) == [3, -4, 5]


def _raw_run(dec, page, x, y, width, line_height, line_advance):
    """focr_decoder_run of one page with whatever state the library is in: (return code, its message)."""
    page = np.ascontiguousarray(page)
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], x, y, width, line_height,
                                   line_advance)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def test_refusals(dec):
    """Every refusal of include/focr_decode.h, before anything is launched and each with a message that names both
    setters; the decoder decodes afterwards."""
    m = model(MONO, 13.0, B64, 2)
    page = _offset_pages(MONO, 13.0, B64, [(0.5,)], W=60, n_chars=6)[0]
    geo = (2, 0, 58, 16, 16)
    lib, h = dec._lib, dec._h
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, [page], geo, 4)

    def refused(*words):
        rc, msg = _raw_run(dec, page, *geo)
        assert rc != 0 and all(w in msg for w in words + ("focr_decoder_set_baseline_search",)), msg
        assert lib.focr_decoder_last_launches(h) == 0 and lib.focr_decoder_n_lines(h) == 0 and _baselines(dec)[0] != 0

    # the setters' own bounds
    assert lib.focr_decoder_set_baseline_search(h, 4, 4) != 0 and b"focr_decoder_set_baseline_search: y_bits" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_baseline_search(h, 2, 33) != 0 and b"at most 32" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_baseline_search(h, 2, 4) == 0
    # states of the library the Python API never makes
    for on, off, name in ((lambda: lib.focr_decoder_set_scores(h, 1), lambda: lib.focr_decoder_set_scores(h, 0), "focr_decoder_set_scores"),
                          (lambda: lib.focr_decoder_set_pen_search(h, 4), lambda: lib.focr_decoder_set_pen_search(h, 0), "focr_decoder_set_pen_search"),
                          (lambda: lib.focr_decoder_set_whole_line(h, 1), lambda: lib.focr_decoder_set_whole_line(h, 0), "focr_decoder_set_whole_line"),
                          (lambda: lib.focr_decoder_set_whole_margins(h, 1), lambda: lib.focr_decoder_set_whole_margins(h, 0), "focr_decoder_set_whole_margins"),
                          (lambda: lib.focr_decoder_set_whole_slack(h, 4), lambda: lib.focr_decoder_set_whole_slack(h, 0), "focr_decoder_set_whole_slack")):
        assert on() == 0
        refused(name)
        assert off() == 0
    # B > 0 without y-phase fonts of that B
    assert lib.focr_decoder_set_baseline_search(h, 3, 4) == 0
    refused("y_bits", "focr_decoder_set_baseline_fonts")
    assert lib.focr_decoder_set_baseline_search(h, 2, 4) == 0
    plain = DecodeFont(MONO, 13.0, B64)
    dec.set_font(plain, 13.0)  # set_font drops the y-phase fonts
    refused("y_bits", "focr_decoder_set_baseline_fonts")
    # fonts that do not match the decode font: another alphabet, another size, and a fonts[0] with other bitmaps
    for other, words in ((DecodeFont(MONO, 13.0, B64[1:] + "A", y_bits=2), b"code points"), (DecodeFont(MONO, 12.0, B64, y_bits=2), b"size"),
                         (DecodeFont(MONO, 13.0, B64[:64], y_bits=2), b"glyph count")):
        assert lib.focr_decoder_set_baseline_fonts(h, other.fonts, 2) != 0
        assert b"focr_decoder_set_baseline_fonts" in lib.focr_decoder_last_error(h) and words in lib.focr_decoder_last_error(h)
        other.close()
    forged = DecodeFont(MONO, 13.0, B64, y_bits=2)
    forged.s.bitmaps[forged.s.glyphs[3].offset + 40] ^= 1
    assert lib.focr_decoder_set_baseline_fonts(h, forged.fonts, 2) != 0 and b"fonts[0]" in lib.focr_decoder_last_error(h)
    forged.s.bitmaps[forged.s.glyphs[3].offset + 40] ^= 1
    assert lib.focr_decoder_set_baseline_fonts(h, forged.fonts, 4) != 0 and b"y_bits" in lib.focr_decoder_last_error(h)
    refused("focr_decoder_set_baseline_fonts")  # a failed upload leaves none
    assert lib.focr_decoder_set_baseline_fonts(h, forged.fonts, 2) == 0
    dec.font, dec._baseline = forged, (2, 4)
    assert dec.decode([page], *geo, baseline_search=4)[0] == [[(y, b.text) for y, b in pg] for pg in want]
    # an origin_y that is not a whole number (a caller-built font: the builder's always is)
    bent = DecodeFont(MONO, 13.0, B64)
    bent.s.origin_y = 10.5
    dec.set_font(bent, 13.0)
    assert lib.focr_decoder_set_baseline_search(h, 0, 4) == 0
    refused("origin_y", "whole number")
    assert lib.focr_decoder_set_baseline_search(h, 0, 0) == 0
    dec._baseline = (0, 0)
    assert _raw_run(dec, page, *geo)[0] == 0  # the plain run takes that font
    with pytest.raises(ValueError):
        dec.decode([page], *geo, baseline_search=4, pen_search=4)
    with pytest.raises(DecoderError, match="focr_decoder_get_baselines|did not search"):
        dec._check(lib.focr_decoder_get_baselines(h, None, None))
    for f in (plain, forged, bent):
        f.close()
    dec.set_font(m.font, 13.0)
    _check(dec, m, [page], geo, 4)


def test_verify_moves_each_canvas(dec):
    """The verify image and sums after a baseline run: draw_verify with each line's canvas moved by the nearest whole
    row of its offset, clipped at the page's top (the first line, a row and a half up) and bottom (the last)."""
    font, size, al, geo = MONO, 13.0, B64, (2, 0, 118, 16, 16)
    pages = _offset_pages(font, size, al, [(-1.5, 0.25, 2.0, None, 1.75)], seed=9)
    pages[0] = pages[0][:78]  # the last line's moved canvas reaches past the page's bottom
    m = model(font, size, al, 2)
    dec.set_font(m.font, size)
    want = m.search_image(pages[0], *geo, 8)
    assert [b.q for _, b in want] == [-6, 1, 8, 7]
    assert [B.row_shift(b.q, 2) for _, b in want] == [-1, 0, 2, 2]
    lines, mse, images, qs, costs = dec.decode(pages, *geo, verify="image", baseline_search=8)
    assert lines[0] == [(y, b.text) for y, b in want] and qs[0] == [b.q for _, b in want] and costs[0] == [b.cost for _, b in want]
    vf = VerifyFont(font, size, al)
    img, sq = B.verify_image(pages[0], [(y, b.text, b.q) for y, b in want], m.font, vf, geo[0], 2)
    assert np.array_equal(images[0], img)
    sums, _ = dec.verify(images=False)
    assert int(sums[0]) == sq and mse[0].tobytes() == (np.float32(sq) / np.float32(pages[0].size)).tobytes()
    assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
    unmoved, _ = B.verify_image(pages[0], [(y, b.text, 0) for y, b in want], m.font, vf, geo[0], 2)
    assert not np.array_equal(img, unmoved)
    plain, plain_mse, _ = dec.decode(pages, *geo, verify="mse")
    assert plain != lines and mse[0] < plain_mse[0]
    vf.close()


def test_cli(dec, tmp_path):
    """focr --baseline-search 8 --y-bits 2 --baselines --verify on two PGMs of different sizes: stdout is the Python API's
    text, the CSV its q, offset and cost per line, the MSEs on stderr its verify's."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    font, size, al, geo = MONO, 13.0, FOCR_DEFAULT_ALPHABET, (2, 0, 118, 16, 16)
    a, b = _offset_pages(font, size, al, [(0.75, -1.0, None, 1.3), (-0.25, 0.0, 0.5, None)], seed=13)
    pages = [a, b[:48, :110].copy()]
    paths = []
    for i, pg in enumerate(pages):
        paths.append(str(tmp_path / f"page{i}.pgm"))
        save_pgm(paths[-1], pg)
    out, vdir = tmp_path / "baselines.csv", tmp_path / "v"
    vdir.mkdir()
    cmd = [FOCR, "-f", font, "-t", str(size), "-x", "2", "-y", "0", "-w", "118", "--line-height", "16", "--line-advance", "16"]
    r = subprocess.run(cmd + ["--baseline-search", "8", "--y-bits", "2", "--baselines", str(out), "--verify", str(vdir), "-i"] + paths,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    dec.set_font(font, size, y_bits=2)
    lines, mse, _, qs, costs = dec.decode(pages, *geo, verify="mse", baseline_search=8)
    assert r.stdout == "".join(t + "\n" for pg in lines for _, t in pg) and len(r.stdout) > 60
    assert sorted(r.stderr.splitlines()) == sorted("%s %.6f" % (p, m) for p, m in zip(paths, mse))
    assert sorted(os.listdir(vdir)) == ["page0.png", "page1.png"]
    with open(out, newline="") as f:
        got = list(csv.reader(f))
    rows = [[str(i), str(y), str(q), "%g" % (q / 4), str(c)] for i, (pg, q_pg, c_pg) in enumerate(zip(lines, qs, costs))
            for (y, _), q, c in zip(pg, q_pg, c_pg)]
    assert got == [["image_index", "y", "q", "offset_px", "cost"]] + rows
    assert {row[3] for row in rows} >= {"0.75", "-1", "1.25"}
    r = subprocess.run(cmd + ["-i"] + paths, capture_output=True, text=True, timeout=300)  # without the search: today's text
    assert r.returncode == 0 and r.stdout == "".join(t + "\n" for pg in dec.decode(pages, *geo) for _, t in pg) != ""


def test_memory_returns():
    """A decoder that uploaded y-phase fonts and searched, with a verify, gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    page = _offset_pages(MONO, 13.0, FOCR_DEFAULT_ALPHABET, [(0.75, -1.0)], seed=1)[0]
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0)
        d.decode([page], 2, 0, 118, 16, 16)
        off = N.hip().focr_debug_device_bytes()
        d.set_font(MONO, 13.0, y_bits=2)
        fonts = N.hip().focr_debug_device_bytes()
        d.decode([page], 2, 0, 118, 16, 16, baseline_search=8, verify="mse")
        searched = N.hip().focr_debug_device_bytes()
        assert before < off < fonts < searched
        d.set_font(MONO, 13.0)  # drops the y-phase tables
        assert N.hip().focr_debug_device_bytes() < searched
    assert N.hip().focr_debug_device_bytes() == before

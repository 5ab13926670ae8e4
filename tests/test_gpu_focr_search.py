"""The focr decoder's pen search (line_search_kernel, focr_decoder_set_pen_search / focr_decoder_get_offsets,
LineDecoder.decode(pen_search=N), focr --pen-search) against tests/focr_search_model.py, the definition of
include/focr_decode.h restated on the fast model and pinned to FreeType by tests/test_focr_search_model.py.  Every
quantity is an exact integer or an f32 computed by stated operations, so every comparison is ==.  Each test asserts from
its geometry, or from the model's answer, that it reaches the case it names."""
import csv
import functools
import os
import subprocess

import numpy as np
import pytest

import focr_scores_model as SC
import focr_search_model as S
from focr_fast_model import ASCII95, TIE_GROUPS, FastModel, line_cap, narrowest_glyph_line, permuted_319
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder, LineScores, VerifyFont, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536      # decode.hip: the plain kernel stages a strip of up to this many bytes in LDS
SEARCH_RED_BYTES = 128     # decode.hip: the search kernel's reduction pairs share that LDS with the strip
ALPHABETS = {"default": FOCR_DEFAULT_ALPHABET, "ascii95": ASCII95}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


@functools.lru_cache(maxsize=None)
def model(font, size, alphabet):
    return FastModel(font, size, alphabet)


def strip_bytes(page_w, x, width, line_height):
    w = min(width, page_w - min(x, page_w))
    return ((w + 7) // 4 + 2) * 4 * line_height


def _ink(alphabet):
    return "".join(c for c in alphabet if not c.isspace())


def _text(rng, alphabet, n):
    return "".join(rng.choice(list(alphabet), n))


def _want(fm, pages, geo, n):
    return [S.search_image(fm, p, *geo, n) for p in pages]


def _check(dec, fm, pages, geo, n):
    """Decode with radius n: line order, texts, n_chars and offsets equal to the model's.  Returns the model's
    [[(y, Searched)] per page]."""
    want = _want(fm, pages, geo, n)
    lines, offsets = dec.decode(pages, *geo, pen_search=n)
    assert lines == [[(y, s.text) for y, s in pg] for pg in want]
    assert [len(pg) for pg in offsets] == [len(pg) for pg in lines]
    for p, (got_pg, want_pg) in enumerate(zip(offsets, want)):
        for got, (y, s) in zip(got_pg, want_pg):
            assert got.dtype == np.int8 and got.shape == s.offsets.shape and np.array_equal(got, s.offsets), (p, y)
    return want


def _snapped_pages(font, size, alphabet, W=200, seed=0):
    """Two pages of four 16-row slots and a clipped fifth: three lines of text each and a blank slot, drawn with the
    pens floored to whole pixels on the first page and with an advance 1 % too large on the second."""
    rng = np.random.default_rng(seed)
    pages = []
    for snap, adv in (("floor", 1.0), ("exact", 1.01)):
        page = np.full((67, W), 255, dtype=np.uint8)
        for slot in (0, 1, 3):
            S.draw_snapped(page, font, size, alphabet, _text(rng, alphabet, 22), 2, slot * 16, snap, adv)
        pages.append(page)
    return pages


@pytest.mark.parametrize("n", [1, 8, 32, 64])
@pytest.mark.parametrize("alphabet", ["default", "ascii95"])
@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
def test_parity(dec, font, alphabet, n):
    al = ALPHABETS[alphabet]
    pages = _snapped_pages(font, 13.0, al, seed=len(al) + (font == SANS))
    fm = model(font, 13.0, al)
    dec.set_font(fm.font, 13.0)
    want = _check(dec, fm, pages, (2, 0, 198, 16, 16), n)
    assert [[y for y, _ in pg] for pg in want] == [[0, 16, 48]] * 2
    offs = np.concatenate([s.offsets for pg in want for _, s in pg])
    assert np.any(offs < 0) and np.any(offs > 0) and np.all(np.abs(offs) <= n)
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    assert dec._lib.focr_decoder_n_chars(dec._h) == len(offs)


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
def test_ties(dec, font):
    """319 glyphs with each group of identical glyphs on one lane of the plain kernel's stripes, radius 4.  Glyph ties:
    where a group wins, its first member by index does, at whatever offset.  Offset ties: a blank scores the same at
    every offset, so a run of spaces between inked glyphs decodes at j = 0."""
    al = permuted_319()
    assert [al.index(c) for c in "АAΑ"] == [5, 69, 133]
    rng = np.random.default_rng(7)
    page = np.full((32, 150), 255, dtype=np.uint8)
    for ly, gap in ((0, "   "), (16, "  ")):
        text = gap.join("".join(rng.choice(list("AAoo" + "xyzéŁź"), 4)) for _ in range(3))
        S.draw_snapped(page, font, 13.0, al, text, 0, ly, "floor")
    fm = model(font, 13.0, al)
    dec.set_font(fm.font, 13.0)
    want = _check(dec, fm, [page], (0, 0, 150, 16, 16), 4)[0]
    text = "".join(s.text for _, s in want)
    offs = np.concatenate([s.offsets for _, s in want])
    blank = np.array([c in " \u00a0" for c in text])
    assert blank.sum() >= 5 and not offs[blank].any() and offs[~blank].any()
    for grp in TIE_GROUPS:
        first = min(grp, key=al.index)
        assert first in text and not set(grp) - {first} & set(text), grp


@pytest.mark.parametrize("font,origin_x", [(MONO, 0.0), (SANS, 1.0)], ids=["origin0", "origin1"])
def test_line_start(dec, font, origin_x):
    """A line whose ink starts one column left of where the pen at 0 puts it.  With origin_x = 0 every negative offset of
    the first step is dropped (origin_x + p_j < 0) and the step has to do with j >= 0; with origin_x = 1 they are
    candidates down to a whole pixel and the first step takes one."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(font, 13.0, al)
    assert float(fm.ox) == origin_x
    page = np.full((16, 120), 255, dtype=np.uint8)
    S.draw_snapped(page, font, 13.0, al, "HEADofLINE", 0, 0)
    page = np.concatenate([page[:, 1:], np.full((16, 1), 255, dtype=np.uint8)], axis=1)  # one column to the left
    dec.set_font(fm.font, 13.0)
    (_, s), = _check(dec, fm, [page], (0, 0, 120, 16, 16), 64)[0]
    assert s.offsets[0] >= 0 if origin_x == 0 else s.offsets[0] < 0
    assert np.float32(origin_x) + s.pens[0] >= 0


@pytest.mark.parametrize("width,n", [(1008, 2), (1012, 2), (1013, 8)])
def test_lds_and_global_strip(dec, width, n):
    """Sans 24 px in 64-row slots.  Width 1013 is where the plain kernel's strip leaves LDS (65792 bytes); the search
    kernel shares LDS with its reduction pairs, so its own last LDS strip is 1008 wide and 1012 already reads global."""
    font, size, lh = SANS, 24.0, 64
    sb = strip_bytes(1013, 0, width, lh)
    assert {1008: sb + SEARCH_RED_BYTES <= LDS_STRIP_MAX, 1012: sb <= LDS_STRIP_MAX < sb + SEARCH_RED_BYTES, 1013: sb > LDS_STRIP_MAX}[width]
    rng = np.random.default_rng(31)
    page = np.full((2 * lh, 1013), 255, dtype=np.uint8)
    for s in range(2):
        for dy in (3, 33):
            SC.draw(page, font, size, _text(rng, FOCR_DEFAULT_ALPHABET, 85), 0, s * lh + dy)
    page[:, 1007:] = np.minimum(page[:, 1007:], 200)  # ink in the columns the widths differ by
    fm = model(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    want = _check(dec, fm, [page], (0, 0, width, lh, lh), n)[0]
    assert [y for y, _ in want] == [0, 64] and all(len(s.text) > 60 for _, s in want)


def test_refusals(dec):
    """Sans 6 px: the smallest increment is 1.667 px, so 53 / 64 is the largest radius the run takes.  A line of the
    narrowest glyph decodes to the model's length at it; 54 is refused at run, with a message, and 65 where it is set."""
    font, size, al, W = SANS, 6.0, FOCR_DEFAULT_ALPHABET, 120
    line, ch, plain_cap = narrowest_glyph_line(font, size, al, W)
    fm = model(font, size, al)
    n = S.max_radius(fm.incs)
    assert n == 53 and plain_cap == line_cap(fm.incs, W)
    dec.set_font(fm.font, size)
    (_, s), = _check(dec, fm, [line], (0, 0, W, 16, 16), n)[0]
    assert 0 < len(s.text) <= S.search_cap(fm.incs, W, n) and np.any(s.offsets == -n)
    with pytest.raises(DecoderError, match="pen search radius.*smallest pen increment"):
        dec.decode([line], 0, 0, W, 16, 16, pen_search=n + 1)
    assert dec.decode([line], 0, 0, W, 16, 16, pen_search=n)[0] == [[(0, s.text)]]
    with pytest.raises(ValueError):
        dec.decode([line], 0, 0, W, 16, 16, pen_search=65)
    assert dec._lib.focr_decoder_set_pen_search(dec._h, 65) != 0
    assert b"focr_decoder_set_pen_search" in dec._lib.focr_decoder_last_error(dec._h)
    assert dec.decode([line], 0, 0, W, 16, 16, pen_search=n)[0] == [[(0, s.text)]]  # the refused radius changed nothing


def _ramp_line(W):
    """A line whose ink fades from black at the left to paper at the right: a lone glyph always scores best as far left
    as the search lets it go, so every step pulls the pen back."""
    return np.tile(np.linspace(0, 254, W).round().astype(np.uint8), (16, 1))


@pytest.mark.parametrize("size,n,want_len,plain_cap,cap", [(7.15, 63, 116, 61, 120), (6.0, 53, 119, 72, 144)])
def test_cap_edge(dec, size, n, want_len, plain_cap, cap):
    """The searched line cap, on the lines that need it: Sans 'i' alone on the ramp, at the largest radius the refusal
    allows.  At 7.15 px (increment 1.986, radius 63 / 64) 112 of the 116 steps take j = -63 and the pen crawls by a
    whole pixel: 116 characters under a searched cap of 120, where the plain cap is 61.  At 6 px (1.667, 53 / 64) the
    crawl settles at j = -43 / -42: 119 characters, plain cap 72, searched cap 144.  A decoder that kept the plain cap,
    or any cap below the model's length, would cut these lines; n_chars must equal the model's.  One radius more is
    refused at run."""
    font, al, W = SANS, "i", 120
    fm = model(font, size, al)
    assert n == S.max_radius(fm.incs) < 64 and plain_cap == line_cap(fm.incs, W) and cap == S.search_cap(fm.incs, W, n)
    line = _ramp_line(W)
    dec.set_font(fm.font, size)
    (_, s), = _check(dec, fm, [line], (0, 0, W, 16, 16), n)[0]
    assert len(s.text) == want_len and plain_cap < want_len <= cap
    assert dec._lib.focr_decoder_n_chars(dec._h) == want_len
    if size == 7.15:
        assert cap - want_len <= 4 and int((s.offsets == -n).sum()) == 112
    assert len(dec.decode([line], 0, 0, W, 16, 16)[0][0][1]) <= plain_cap  # the plain run keeps its own cap
    with pytest.raises(DecoderError, match="pen search radius.*smallest pen increment"):
        dec.decode([line], 0, 0, W, 16, 16, pen_search=n + 1)


def test_font_that_drops_every_candidate(dec):
    """A caller-built font with origin_x < 0 (the project's builder never makes one): origin_x + p_j is negative for
    every candidate of the first step, so the searched line ends there with no character."""
    df = DecodeFont(MONO, 13.0, "AB")
    df.s.origin_x = -2.0
    page = np.full((16, 60), 255, dtype=np.uint8)
    S.draw_snapped(page, MONO, 13.0, "AB", "ABBA", 0, 0)
    dec.set_font(df, 13.0)
    lines, offsets = dec.decode([page], 0, 0, 60, 16, 16, pen_search=8)
    assert lines == [[(0, "")]] and len(offsets[0][0]) == 0
    df.close()


def _offsets(d):
    js = np.full(d._lib.focr_decoder_n_chars(d._h), 99, dtype=np.int8)
    assert d._lib.focr_decoder_get_offsets(d._h, js.ctypes.data) == 0
    return js


def test_radius_zero_is_the_plain_decoder(dec):
    """Radius 0 through the new entry points, before and after a searched run, against a decoder that never heard of
    them: lines, scores, verify images and sums, and the launch count are the same, and the offsets read all zero."""
    font, size, geo = MONO, 13.0, (2, 0, 198, 16, 16)
    pages = _snapped_pages(font, size, FOCR_DEFAULT_ALPHABET, seed=3)
    with LineDecoder(0) as fresh:
        fresh.set_font(font, size)
        lines, mse, images, scores = fresh.decode(pages, *geo, verify="image", scores=True)
        launches = fresh._lib.focr_decoder_last_launches(fresh._h)
        assert not _offsets(fresh).any() and len(_offsets(fresh)) == sum(len(t) for pg in lines for _, t in pg)
    dec.set_font(font, size)
    assert dec._lib.focr_decoder_set_pen_search(dec._h, 0) == 0
    for again in (False, True):
        got = dec.decode(pages, *geo, verify="image", scores=True, pen_search=0)
        assert len(got) == 4 and got[0] == lines and got[1].tobytes() == mse.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(got[2], images))
        for a_pg, b_pg in zip(got[3], scores):
            assert len(a_pg) == len(b_pg)
            for a, b in zip(a_pg, b_pg):
                assert a.base == b.base and all(np.array_equal(a[f], b[f]) for f in (1, 2, 3))
        assert dec._lib.focr_decoder_last_launches(dec._h) == launches == 3
        assert not _offsets(dec).any()
        if not again:
            searched, offs = dec.decode(pages, *geo, pen_search=8)
            assert searched != lines and any(o.any() for pg in offs for o in pg) and _offsets(dec).any()


def test_scores(dec):
    """Radius 8 with scores on: score is the chosen candidate's, runner and runner_score the best candidate of another
    glyph at any offset.  On clean text the second lowest key of nearly every step is the winner's own glyph one offset
    away, which the rule must pass over."""
    font, size, al, geo = MONO, 13.0, FOCR_DEFAULT_ALPHABET, (2, 0, 198, 16, 16)
    pages = _snapped_pages(font, size, al, seed=5)
    fm = model(font, size, al)
    dec.set_font(fm.font, size)
    want = _want(fm, pages, geo, 8)
    lines, scores, offsets = dec.decode(pages, *geo, scores=True, pen_search=8)
    assert lines == [[(y, s.text) for y, s in pg] for pg in want]
    own = 0
    for got_pg, off_pg, want_pg in zip(scores, offsets, want):
        assert len(got_pg) == len(off_pg) == len(want_pg)
        for got, off, (y, s) in zip(got_pg, off_pg, want_pg):
            assert isinstance(got, LineScores) and got.base == s.base and np.array_equal(off, s.offsets)
            for name, dtype in (("score", np.int64), ("runner", np.uint16), ("runner_score", np.int64)):
                g, w = getattr(got, name), getattr(s, name)
                assert g.dtype == dtype and np.array_equal(g, w), (y, name)
            assert np.all(got.runner != np.array([al.index(c) for c in s.text]))
            own += int(s.second_is_own.sum())
    assert own > 20
    one = "A"  # a one-glyph alphabet has no other glyph, whatever the offsets
    dec.set_font(font, size, one)
    _, sc, _ = dec.decode(pages[:1], *geo, scores=True, pen_search=8)
    assert all(np.all(s.runner == SC.NO_RUNNER) and np.all(s.runner_score == SC.INT64_MAX) for s in sc[0])


def test_verify_follows_the_search(dec):
    """The 1.01-advance page, radius 8: the verify image and sums are draw_verify with every character at the pen the
    search chose, and the page's error is below the plain run's, whose text drifts off the ink."""
    font, size, al, geo = MONO, 13.0, FOCR_DEFAULT_ALPHABET, (2, 0, 198, 16, 16)
    page = _snapped_pages(font, size, al, seed=9)[1]
    fm = model(font, size, al)
    dec.set_font(fm.font, size)
    want = _want(fm, [page], geo, 8)[0]
    lines, mse, images, offsets = dec.decode([page], *geo, verify="image", pen_search=8)
    assert lines[0] == [(y, s.text) for y, s in want] and all(np.array_equal(o, s.offsets) for o, (_, s) in zip(offsets[0], want))
    df, vf = fm.font, VerifyFont(font, size, al)
    img, sq = S.verify_image(page, [(y, s.text, s.pens) for y, s in want], df, vf, geo[0])
    assert np.array_equal(images[0], img)
    sums, _ = dec.verify(images=False)
    assert int(sums[0]) == sq and mse[0].tobytes() == (np.float32(sq) / np.float32(page.size)).tobytes()
    assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
    plain, plain_mse, plain_img = dec.decode([page], *geo, verify="image")
    pimg, psq = S.verify_image(page, [(y, t, S.plain_pens(df, [al.index(c) for c in t])) for y, t in plain[0]], df, vf, geo[0])
    assert np.array_equal(plain_img[0], pimg) and plain != lines
    assert mse[0] < plain_mse[0]
    vf.close()


def test_cli(dec, tmp_path):
    """focr --pen-search 8 --scores --verify on two PGMs of different sizes: stdout is the Python API's text, the CSV is
    its scores with a trailing pen_offset column, the MSEs on stderr are its verify's; without --pen-search the CSV has
    today's header and eight columns."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    font, size, al, geo = MONO, 13.0, FOCR_DEFAULT_ALPHABET, (2, 0, 198, 16, 16)
    a, b = _snapped_pages(font, size, al, seed=13)
    pages = [a, b[:48, :180].copy()]
    paths = []
    for i, pg in enumerate(pages):
        paths.append(str(tmp_path / f"page{i}.pgm"))
        save_pgm(paths[-1], pg)
    out, vdir = tmp_path / "out.csv", tmp_path / "v"
    vdir.mkdir()
    cmd = [FOCR, "-f", font, "-t", str(size), "-x", "2", "-y", "0", "-w", "198", "--line-height", "16", "--line-advance", "16"]
    r = subprocess.run(cmd + ["--pen-search", "8", "--scores", str(out), "--verify", str(vdir), "-i"] + paths, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    dec.set_font(font, size)
    lines, mse, _, scores, offsets = dec.decode(pages, *geo, verify="mse", scores=True, pen_search=8)
    assert r.stdout == "".join(t + "\n" for pg in lines for _, t in pg) and len(r.stdout) > 100
    assert sorted(r.stderr.splitlines()) == sorted("%s %.6f" % (p, m) for p, m in zip(paths, mse))
    assert sorted(os.listdir(vdir)) == ["page0.png", "page1.png"]
    header = ["image_index", "y", "column", "codepoint", "score", "runner_codepoint", "runner_score", "margin"]

    def rows(scores, offsets):
        for i, (pg, sc_pg) in enumerate(zip(lines_, scores)):
            for k, ((y, text), sc) in enumerate(zip(pg, sc_pg)):
                for c, ch in enumerate(text):
                    row = [i, y, c, ord(ch), sc.score[c], ord(al[sc.runner[c]]), sc.runner_score[c], sc.runner_score[c] - sc.score[c]]
                    yield [str(v) for v in row + ([offsets[i][k][c]] if offsets else [])]

    lines_ = lines
    with open(out, newline="") as f:
        got = list(csv.reader(f))
    assert got == [header + ["pen_offset"]] + list(rows(scores, offsets))
    assert any(row[-1] not in ("0",) for row in got[1:])
    r = subprocess.run(cmd + ["--scores", str(out), "-i"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines_, scores = dec.decode(pages, *geo, scores=True)
    assert r.stdout == "".join(t + "\n" for pg in lines_ for _, t in pg)
    want = "".join(",".join(row) + "\n" for row in [header] + list(rows(scores, None)))
    with open(out, "rb") as f:
        assert f.read() == want.encode()


def test_memory_returns():
    """A decoder that ran with a search, with and without scores, gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    page = _snapped_pages(MONO, 13.0, FOCR_DEFAULT_ALPHABET, seed=1)[0]
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0)
        d.decode([page], 2, 0, 198, 16, 16)
        off = N.hip().focr_debug_device_bytes()
        d.decode([page], 2, 0, 198, 16, 16, pen_search=8)
        on = N.hip().focr_debug_device_bytes()
        d.decode([page], 2, 0, 198, 16, 16, scores=True, pen_search=8, verify="mse")
        assert before < off < on < N.hip().focr_debug_device_bytes()
    assert N.hip().focr_debug_device_bytes() == before

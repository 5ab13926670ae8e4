"""The focr decoder's whole-line decode under every baseline candidate (line_whole_baseline_kernel,
focr_decoder_set_whole_baseline, LineDecoder.decode(whole_line=True, whole_baseline=N), focr --whole-line --whole-baseline)
against tests/focr_whole_baseline_model.py, the definition of include/focr_decode.h composed from the baseline and the
whole-line models and pinned to FreeType by tests/test_focr_whole_baseline_model.py.  Every quantity is an exact integer,
so every comparison is ==.  Each test asserts from its geometry, or from the model's answer, that it reaches the case it
names.  The CPU model is what takes the time: crops are 40 to 120 columns and alphabets 2 to 12 glyphs, and the 65
candidates of N = 32 run in Mono, where one state in an advance is reachable."""
import csv
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import focr_baseline_model as B
import focr_whole_baseline_fuzz as FZ
import focr_whole_baseline_model as WB
import focr_whole_model as WM
from focr_fast_model import permuted_319
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder, VerifyFont, load_image_rgba, save_pgm
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
SERIF = os.path.join(GOLD, "DejaVuSerif.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536     # decode_line.h: strip, cost ring and live list share this much LDS, else the strip is read from global
WHOLE_MISC_BYTES = 1088   # decode_whole.h: the head and the live list in front of the ring
WHOLE_BATCH_MAX = 512     # decode_whole.h: states per batch at most
AL = "burn clipfH"        # 11 glyphs of Sans with narrow and wide advances

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


@functools.lru_cache(maxsize=None)
def model(font, size, alphabet, y_bits, hinting=False, kerning=1.0):
    return B.BaselineModel(font, size, alphabet, hinting, kerning, y_bits)


def ring_length(m):
    inc = WM.inc64(m.incs)
    need, n = min(int(inc.min()), WHOLE_BATCH_MAX) + int(inc.max()), 64
    while n < need:
        n *= 2
    return n


def strip_bytes(w, line_height):
    return ((w + 7) // 4 + 2) * 4 * line_height


def _check(dec, m, pages, geo, n, trails=None):
    """Decode whole lines with radius n in steps of 2^-m.y_bits px: line order, texts, pens, costs and q equal to the
    model's, in 3 launches.  Returns the model's [[(y, WholeBaseline)] per page]."""
    want = [WB.search_image(m, p, *geo, n, trails) for p in pages]
    lines, pens, costs, qs = dec.decode(pages, *geo, whole_line=True, whole_baseline=n)
    assert lines == [[(y, b.text) for y, b in pg] for pg in want]
    assert qs == [[b.q for _, b in pg] for pg in want]
    assert costs == [[b.cost for _, b in pg] for pg in want]
    assert [len(pg) for pg in pens] == [len(pg) for pg in want]
    for pen_pg, want_pg in zip(pens, want):
        for got, (y, b) in zip(pen_pg, want_pg):
            assert got.dtype == np.uint32 and np.array_equal(got, b.pens), y
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    return want


def _texts(alphabet, rng, n_chars):
    ink = [c for c in alphabet if not c.isspace()]
    return "".join(rng.choice(ink, n_chars))


def _offset_pages(font, size, alphabet, offsets, W, seed=0, n_chars=8, cut=None):
    """One page per row of `offsets`: 16-row slots, slot s inked with random text `offsets[p][s]` px below the crop's
    baseline (None: blank), and three rows of a further slot that the page's bottom cuts, inked from a line `cut` px
    above the baseline when given."""
    rng = np.random.default_rng(seed)
    pages = []
    for row in offsets:
        page = np.full((16 * len(row) + 3, W), 255, dtype=np.uint8)
        for s, off in enumerate(row):
            if off is not None:
                B.draw_offset(page, font, size, alphabet, _texts(alphabet, rng, n_chars), 2, 16 * s, off)
        if cut is not None:
            B.draw_offset(page, font, size, alphabet, _texts(alphabet, rng, n_chars), 2, 16 * len(row), -cut)
        pages.append(page)
    return pages


@pytest.mark.parametrize("n,y_bits,font,rows", [
    (1, 0, SANS, [(1.0, None, 0.0), (-1.0,)]),
    (2, 2, SANS, [(0.5, None, 0.0), (-0.25,)]),
    (4, 3, SANS, [(0.5, None, 0.0), (-0.25,)]),
    (32, 0, MONO, [(1.0, None, 0.0, -2.0), (3.0, 2.0)]),
    (32, 2, MONO, [(1.25, None, 0.0, -0.75), (8.0, -2.5)]),
    (32, 3, MONO, [(4.0, None, 0.0, -1.0), (0.5, -0.125)]),
], ids=["n1b0", "n2b2", "n4b3", "n32b0", "n32b2", "n32b3"])
def test_parity(dec, n, y_bits, font, rows):
    """3, 5, 9 and 65 candidates at B = 0, 2 and 3.  Lines above and below the baseline in one batch of two pages, blank
    slots between them, and a last slot that the page's bottom cuts to three rows.  Of the winners one is the first
    candidate (q = 0, half 0 of the scratch), one the last in rank order (q = +N; but at N = 32, B = 0, where 32 px down
    leaves nothing of a line in its crop) and one lies between; the trail of improvements says which half of the scratch
    each winner's backpointers were in, and both halves hold one."""
    sans = font == SANS
    al = AL if sans else "ABx0+/"
    W = 44 if sans else 60
    rows = [r + (None,) * (len(rows[0]) - len(r)) for r in rows]
    pages = _offset_pages(font, 13.0, al, rows, W, seed=n + y_bits, n_chars=5 if sans else 7, cut=8.0)
    m = model(font, 13.0, al, y_bits)
    dec.set_font(m.font, 13.0)
    trails = []
    want = _check(dec, m, pages, (2, 0, W - 2, 16, 16), n, trails)
    ys = [[y for y, _ in pg] for pg in want]
    assert all(16 * len(rows[0]) in pg for pg in ys)  # the cut slot is decoded from its three rows
    assert [y for y in ys[0] if y < 16 * len(rows[0])] == [16 * s for s, off in enumerate(rows[0]) if off is not None]
    qs = [b.q for pg in want for _, b in pg]
    assert 0 in qs and (n in qs or n >> y_bits >= 16) and any(q not in (0, n) for q in qs) and all(abs(q) <= n for q in qs)
    assert {(len(t) - 1) & 1 for t in trails} == {0, 1}  # the half of each winner: improvements after the first swap it


@pytest.mark.parametrize("offset", [1.0, -1.0])
def test_proportional_line_off_the_baseline(dec, offset):
    """What the mode is for, on 110 columns of Sans 13 px with the letters of `burn clip ffH vvill` and the wide glyphs the
    greedy loop confuses them with: the line sits 1 px low or 1 px high, the programme under nine candidates at B = 2
    takes the true offset and reads it, and the plain whole-line run of the same page reads another text."""
    al = "burn clipfHvmd"
    m = model(SANS, 13.0, al, 2)
    page = np.full((16, 110), 255, dtype=np.uint8)
    B.draw_offset(page, SANS, 13.0, al, "burn clip ffH vvill", 0, 0, offset)
    dec.set_font(m.font, 13.0)
    (_, b), = _check(dec, m, [page], (0, 0, 110, 16, 16), 4)[0]
    assert b.q == int(offset * 4) and b.text.startswith("burn clip ffH vvill")
    plain, _, _ = dec.decode([page], 0, 0, 110, 16, 16, whole_line=True)
    assert plain[0][0][1] != b.text and plain[0][0][1] == WB.whole_line_q(m, page, 0).text


@pytest.mark.parametrize("y_bits", [0, 2])
def test_dropped_candidates(dec, y_bits):
    """Mono 6 px has origin_y 5: with N = 32 the candidates with ty_q < 0 (q < -5 at B = 0, q < -20 at B = 2) are dropped,
    and a line drawn 4 px above the baseline takes one of the last negative q that remain."""
    al = "ABCDEFabcdef"
    m = model(MONO, 6.0, al, y_bits)
    assert float(m.oy) == 5.0 and m.dropped(-(5 << y_bits) - 1) and not m.dropped(-(5 << y_bits)) and (5 << y_bits) < 32
    page = np.full((24, 80), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 6.0, al, "dEcAfbbADe", 0, 0, -4.0)
    B.draw_offset(page, MONO, 6.0, al, "FaCeBdEdca", 0, 12, 3.0)
    dec.set_font(m.font, 6.0)
    want = _check(dec, m, [page], (0, 0, 80, 12, 12), 32)[0]
    up, down = (b.q / (1 << y_bits) for _, b in want)
    assert -5 <= up <= -3.5 and 2.5 <= down <= 3.5


def test_every_glyph_pushed_off_the_crop(dec):
    """Mono 13 px without descenders, 16-row crops, B = 0, N = 32: origin_y is 10, so q = -10 is the last candidate upwards
    and moves every box above row 0, and q >= 16 moves every box below the last row: those candidates cost 0 whatever
    they read, on the device as in the model, and the search still finds the lines at +2 and -3.  A third slot holds one
    grey pixel: the candidates that push every glyph off the crop cost 0, and so do the others, which read spaces over
    it: all costs are equal, and q = 0 wins."""
    al = "ABx0 "
    m = model(MONO, 13.0, al, 0)
    page = np.full((48, 60), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, al, "ABxB0A", 0, 0, 2.0)
    B.draw_offset(page, MONO, 13.0, al, "x0ABBA", 0, 16, -3.0)
    page[38, 59] = 200  # in the third slot of either geometry below
    assert float(m.oy) == 10.0
    for q in (-10, 16, 32):
        assert WB.whole_line_q(m, page[:16], q).cost == 0
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, [page], (0, 0, 60, 16, 16), 32)[0]
    assert [b.q for _, b in want][:2] == [2, -3] and [b.text[:6] for _, b in want][:2] == ["ABxB0A", "x0ABBA"]
    assert len(want) == 3 and (want[2][1].q, want[2][1].cost) == (0, 0)
    # crops of three rows: only the rows a candidate leaves inside them count, whichever way it is pushed
    want = _check(dec, m, [page], (0, 5, 60, 3, 16), 32)[0]
    assert len(want) == 3 and (want[2][1].q, want[2][1].cost) == (0, 0)


@pytest.mark.parametrize("alphabet", ["3", "65"])
def test_all_tie_line(dec, alphabet):
    """Ink out of every glyph's reach and a space in the alphabet (3 glyphs, and the 65 of the default alphabet, on 60
    columns): every candidate costs the same, so the lower rank, q = 0, wins."""
    al = " AB" if alphabet == "3" else FOCR_DEFAULT_ALPHABET
    m = model(MONO, 13.0, al, 2)
    page = np.full((16, 60), 255, dtype=np.uint8)
    page[15, :] = 0
    assert {WB.whole_line_q(m, page, q).cost for q in (-4, -1, 0, 3)} == {0}
    dec.set_font(m.font, 13.0)
    (_, b), = _check(dec, m, [page], (0, 0, 60, 16, 16), 4)[0]
    assert b.q == 0 and b.cost == 0


def test_ties_in_the_319_glyph_alphabet(dec):
    """The tie alphabet on 60 columns: identical glyphs tie in cost at every state under every candidate, and the first
    member of a group by index is the one remembered; device and model agree on text, pens, q and cost."""
    al = permuted_319()
    page = np.full((16, 60), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, al, "AoxAo A", 0, 0, 0.5)
    m = model(MONO, 13.0, al, 1)
    dec.set_font(m.font, 13.0)
    (_, b), = _check(dec, m, [page], (0, 0, 60, 16, 16), 2)[0]
    assert b.q == 1 and len(b.text) >= 7 and b.text[2] == "x"
    for grp in ("AΑА", "oοо"):
        first = min(grp, key=al.index)
        assert first in b.text and not set(grp) - {first} & set(b.text), grp


def test_several_lines_per_workgroup(dec):
    """Six lines on two pages whose winners sit in different halves of the scratch (the trails' parities differ from one
    line to the next), on a grid of one and of two workgroups: a workgroup takes six and three lines in turn, and neither
    a stale half nor a stale saved end state leaks from one line into the next.  Then the decoder's own grid."""
    m = model(SANS, 13.0, AL, 1)
    pages = _offset_pages(SANS, 13.0, AL, [(0.0, -0.5, 1.0), (0.5, 0.0, -1.0)], 44, seed=7, n_chars=5)
    geo = (2, 0, 42, 16, 16)
    dec.set_font(m.font, 13.0)
    trails = []
    want = _check(dec, m, pages, geo, 2, trails)
    assert [len(pg) for pg in want] == [3, 3] and [b.q for pg in want for _, b in pg] == [0, -1, 2, 1, 0, -2]
    halves = [(len(t) - 1) & 1 for t in trails]
    assert {0, 1} == set(halves) and any(a != b for a, b in zip(halves, halves[1:]))
    free = dec.decode(pages, *geo, whole_line=True, whole_baseline=2)
    try:
        for grid in (1, 2):
            assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, grid) == 0
            got = dec.decode(pages, *geo, whole_line=True, whole_baseline=2)
            assert got[0] == free[0] and got[2] == free[2] and got[3] == free[3]
            assert all(np.array_equal(a, b) for pa, pb in zip(got[1], free[1]) for a, b in zip(pa, pb))
    finally:
        assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 0) == 0


@pytest.mark.parametrize("line_height", [1081, 1082])
def test_strip_in_lds_and_in_global_memory(dec, line_height):
    """Mono 13 px, four glyphs, 40 columns: with 1081 rows strip, ring and live list are the last to fit the LDS budget;
    with 1082 the strip is read from global memory, by every candidate."""
    al = "AB >"
    m = model(MONO, 13.0, al, 2)
    lds = strip_bytes(40, line_height) + WHOLE_MISC_BYTES + 8 * ring_length(m)
    assert (lds <= LDS_STRIP_MAX) == (line_height == 1081) and strip_bytes(40, 1081) + WHOLE_MISC_BYTES + 8 * ring_length(m) > LDS_STRIP_MAX - 52
    page = np.full((1082, 40), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, al, "AB>BA", 0, 0, 0.75)
    page[1081, :] = np.minimum(page[1081, :], 200)  # ink in the row the heights differ by
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, [page], (0, 0, 40, line_height, line_height), 4)[0]
    assert [y for y, _ in want] == [0, line_height][: 1082 - line_height + 1]  # the last row is a slot of its own at 1081 rows
    assert want[0][1].q == 3 and want[0][1].text[:5] == "AB>BA"


def test_batch_capped_below_the_smallest_advance(dec):
    """Sans 32 px, "il m": the smallest inc64 is above the 512 states a batch may hold, so batches are shorter than every
    step, under every candidate."""
    al = "il m"
    m = model(SANS, 32.0, al, 1)
    inc = WM.inc64(m.incs)
    assert int(inc.min()) > WHOLE_BATCH_MAX and len(set(inc.tolist())) >= 3
    page = np.full((40, 80), 255, dtype=np.uint8)
    B.draw_offset(page, SANS, 32.0, al, "lim il", 0, 0, -0.5)
    dec.set_font(m.font, 32.0)
    (_, b), = _check(dec, m, [page], (0, 0, 80, 40, 40), 2)[0]
    assert b.q == -1 and b.text.startswith("lim il")


def test_narrow_font_with_a_ring_of_64_keys(dec):
    """Mono 1 px at kerning 0.8: every advance is 31/64 px, so batch and widest advance fit the shortest ring there is."""
    al = "AB"
    m = model(MONO, 1.0, al, 2, False, 0.8)
    assert ring_length(m) == 64 and set(WM.inc64(m.incs).tolist()) == {31}
    page = np.full((4, 40), 255, dtype=np.uint8)
    page[1:3, 3:30] = np.random.default_rng(2).integers(100, 256, (2, 27)).astype(np.uint8)
    dec.set_font(m.font, 1.0)
    (_, b), = _check(dec, m, [page], (0, 0, 40, 4, 4), 4)[0]
    assert len(b.text) == -(-64 * 40 // 31)


@pytest.mark.parametrize("font,hinting", [(SERIF, False), (MONO, True)], ids=["serif", "hinted"])
def test_y_phases_with_different_boxes(dec, font, hinting):
    """Serif unhinted and Mono hinted at B = 2: box_h differs between the y-phases of some glyph, and the alphabet's last
    glyph, whose bitmaps end the y-phase table, is on the line, so the table's last rows are read."""
    al = "gjpqy bdfHQ"
    m = model(font, 13.0, al, 2, hinting)
    heights = {v: [m.font.fonts[v].glyphs[i].box_h for i in range(len(al))] for v in range(4)}
    assert any(heights[v] != heights[0] for v in (1, 2, 3))
    page = np.full((19, 100), 255, dtype=np.uint8)
    B.draw_offset(page, font, 13.0, al, "Qjdg QQ", 0, 0, 0.75, hinting)
    dec.set_font(m.font, 13.0)
    (_, b), = _check(dec, m, [page], (0, 0, 100, 19, 19), 3)[0]
    assert b.q == 3 and "Q" in b.text and al[-1] == "Q"


def _raw_run(dec, page, x, y, width, line_height, line_advance):
    """focr_decoder_run of one page with whatever state the library is in: (return code, its message)."""
    page = np.ascontiguousarray(page)
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], x, y, width, line_height,
                                   line_advance)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def _baselines(d):
    n = d._lib.focr_decoder_n_lines(d._h)
    q, cost = np.full(max(n, 1), 99, dtype=np.int8), np.zeros(max(n, 1), dtype=np.int64)
    rc = d._lib.focr_decoder_get_baselines(d._h, q.ctypes.data, cost.ctypes.data)
    return rc, q[:n], cost[:n]


def test_refusals(dec):
    """Every refusal of include/focr_decode.h, through ctypes for the states the Python API never makes: before anything
    is launched, each with a message that names the setters involved; the decoder decodes afterwards."""
    m = model(MONO, 13.0, "ABx0+/", 2)
    page = _offset_pages(MONO, 13.0, "ABx0+/", [(0.5,)], 60, n_chars=6)[0]
    geo = (2, 0, 58, 16, 16)
    lib, h = dec._lib, dec._h
    dec.set_font(m.font, 13.0)
    want = _check(dec, m, [page], geo, 4)

    def refused(*words):
        rc, msg = _raw_run(dec, page, *geo)
        assert rc != 0 and all(w in msg for w in words + ("focr_decoder_set_whole_baseline",)), msg
        assert lib.focr_decoder_last_launches(h) == 0 and lib.focr_decoder_n_lines(h) == 0 and _baselines(dec)[0] != 0

    # the setter's own bounds
    assert lib.focr_decoder_set_whole_baseline(h, 4, 4) != 0 and b"focr_decoder_set_whole_baseline: y_bits" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_whole_baseline(h, 2, 33) != 0 and b"at most 32" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_whole_baseline(h, 2, 4) == 0
    # beside margins, beside slack, and with the whole-line decode off
    for on, off, name in ((lambda: lib.focr_decoder_set_whole_margins(h, 1), lambda: lib.focr_decoder_set_whole_margins(h, 0), "focr_decoder_set_whole_margins"),
                          (lambda: lib.focr_decoder_set_whole_slack(h, 4), lambda: lib.focr_decoder_set_whole_slack(h, 0), "focr_decoder_set_whole_slack"),
                          (lambda: lib.focr_decoder_set_whole_line(h, 0), lambda: lib.focr_decoder_set_whole_line(h, 1), "focr_decoder_set_whole_line")):
        assert on() == 0
        refused(name)
        assert off() == 0
    # the pen loop's search stays refused beside the whole-line decode, with its own message
    assert lib.focr_decoder_set_whole_baseline(h, 2, 0) == 0 and lib.focr_decoder_set_baseline_search(h, 2, 4) == 0
    rc, msg = _raw_run(dec, page, *geo)
    assert rc != 0 and "focr_decoder_set_baseline_search" in msg and "focr_decoder_set_whole_line" in msg
    assert lib.focr_decoder_set_baseline_search(h, 0, 0) == 0
    # B > 0 without y-phase fonts of that B
    assert lib.focr_decoder_set_whole_baseline(h, 3, 4) == 0
    refused("y_bits", "focr_decoder_set_baseline_fonts")
    assert lib.focr_decoder_set_whole_baseline(h, 2, 4) == 0
    plain = DecodeFont(MONO, 13.0, "ABx0+/")
    dec.set_font(plain, 13.0)  # set_font drops the y-phase fonts
    refused("y_bits", "focr_decoder_set_baseline_fonts")
    # an origin_y that is not a whole number (a caller-built font: the builder's always is)
    bent = DecodeFont(MONO, 13.0, "ABx0+/")
    bent.s.origin_y = 10.5
    dec.set_font(bent, 13.0)
    assert lib.focr_decoder_set_whole_baseline(h, 0, 4) == 0
    refused("origin_y", "whole number")
    assert lib.focr_decoder_set_whole_baseline(h, 0, 0) == 0
    assert _raw_run(dec, page, *geo)[0] == 0  # the plain whole-line run takes that font
    dec._whole, dec._whole_baseline = True, (0, 0)
    for kw in ({"whole_line": False}, {"whole_line": True, "margins": True}, {"whole_line": True, "pen_slack": 4}):
        with pytest.raises(ValueError, match="whole_baseline"):
            dec.decode([page], *geo, whole_baseline=4, **kw)
    for f in (plain, bent):
        f.close()
    dec.set_font(m.font, 13.0)
    again = _check(dec, m, [page], geo, 4)
    assert [b.q for _, b in again[0]] == [b.q for _, b in want[0]]


def test_modes_follow_each_other_on_one_handle(dec):
    """Plain, whole-line, baseline_search and whole_baseline runs follow each other on one decoder, twice over, and each
    returns what it did alone on a fresh one; focr_decoder_get_baselines fails after a plain whole-line run and succeeds
    after this mode's."""
    al, geo = AL, (2, 0, 42, 16, 16)
    pages = _offset_pages(SANS, 13.0, al, [(0.5, None, -0.5)], 44, seed=3, n_chars=5)
    modes = [{}, {"whole_line": True}, {"baseline_search": 2}, {"whole_line": True, "whole_baseline": 2}]

    def same(a, b):
        return repr(a) == repr(b)

    alone = []
    for kw in modes:
        with LineDecoder(0) as fresh:
            fresh.set_font(SANS, 13.0, al, y_bits=1)
            alone.append(fresh.decode(pages, *geo, verify="mse", **kw))
    dec.set_font(SANS, 13.0, al, y_bits=1)
    for _ in range(2):
        for kw, want in zip(modes, alone):
            got = dec.decode(pages, *geo, verify="mse", **kw)
            assert same(got, want), kw
            rc = _baselines(dec)[0]
            assert (rc == 0) == ("baseline_search" in kw or "whole_baseline" in kw), kw
            if kw == {"whole_line": True}:
                assert b"focr_decoder_set_whole_baseline" in dec._lib.focr_decoder_last_error(dec._h)
    assert alone[3][-1] == [[1, -1]] and all(a < b for a, b in zip(alone[3][4][0], alone[1][4][0]))  # q, and a lower cost than at q = 0
    # N = 0 is the plain whole-line run
    got = dec.decode(pages, *geo, verify="mse", whole_line=True, whole_baseline=0)
    assert same(got, alone[1]) and dec._lib.focr_decoder_last_launches(dec._h) == 3


def test_verify_draws_pens_on_a_moved_canvas(dec):
    """The verify image and sums after such a run: every character at pos = s / 64 of its pen, each line's canvas moved
    by the nearest whole row of its offset and clipped at the page's top (the first line, a row and a half up) and
    bottom (the last)."""
    al = "burn clipfHvmd"
    geo = (0, 0, 60, 16, 16)
    m = model(SANS, 13.0, al, 1)
    assert float(m.ox) == 0
    page = np.full((43, 60), 255, dtype=np.uint8)
    for s, (text, off) in enumerate((("burn clip", -1.5), ("fill Hrn", 0.5), ("club dim", 2.0))):
        B.draw_offset(page, SANS, 13.0, al, text, 0, 16 * s, off)
    dec.set_font(m.font, 13.0)
    want = WB.search_image(m, page, *geo, 4)
    assert [b.q for _, b in want] == [-3, 1, 4] and [B.row_shift(b.q, 1) for _, b in want] == [-1, 1, 2]
    lines, mse, images, pens, costs, qs = dec.decode([page], *geo, verify="image", whole_line=True, whole_baseline=4)
    assert lines[0] == [(y, b.text) for y, b in want] and qs[0] == [b.q for _, b in want] and costs[0] == [b.cost for _, b in want]
    assert all(np.array_equal(p, b.pens) for p, (_, b) in zip(pens[0], want))
    vf = VerifyFont(SANS, 13.0, al)
    img, sq = WB.verify_image(page, [(y, b.text, b.pens, b.q) for y, b in want], m.font, vf, geo[0], 1)
    assert np.array_equal(images[0], img)
    sums, _ = dec.verify(images=False)
    assert int(sums[0]) == sq and mse[0].tobytes() == (np.float32(sq) / np.float32(page.size)).tobytes()
    assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
    unmoved, _ = WB.verify_image(page, [(y, b.text, b.pens, 0) for y, b in want], m.font, vf, geo[0], 1)
    assert not np.array_equal(img, unmoved)
    vf.close()


def test_cli(dec, tmp_path):
    """focr --whole-line --whole-baseline 4 --y-bits 2 --baselines --verify on one small page: stdout is the model's
    text, the CSV its q, offset and cost per line, the PNG byte-equal to the model's verify image."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    al = FOCR_DEFAULT_ALPHABET
    page = np.full((35, 64), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, al, "Whole+0", 2, 0, 0.75)
    B.draw_offset(page, MONO, 13.0, al, "line/q=", 2, 16, -1.0)
    path = str(tmp_path / "page.pgm")
    save_pgm(path, page)
    out, vdir = tmp_path / "baselines.csv", tmp_path / "v"
    vdir.mkdir()
    cmd = [FOCR, "-f", MONO, "-t", "13", "-x", "2", "-y", "0", "-w", "62", "--line-height", "16", "--line-advance", "16", "--whole-line"]
    r = subprocess.run(cmd + ["--whole-baseline", "4", "--y-bits", "2", "--baselines", str(out), "--verify", str(vdir), "-i", path],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = model(MONO, 13.0, al, 2)
    want = WB.search_image(m, page, 2, 0, 62, 16, 16, 4)
    assert [b.q for _, b in want[:2]] == [3, -4]
    assert r.stdout == "".join(b.text + "\n" for _, b in want)
    with open(out, newline="") as f:
        got = list(csv.reader(f))
    assert got == [["image_index", "y", "q", "offset_px", "cost"]] + [["0", str(y), str(b.q), "%g" % (b.q / 4), str(b.cost)] for y, b in want]
    vf = VerifyFont(MONO, 13.0, al)
    img, sq = WB.verify_image(page, [(y, b.text, b.pens, b.q) for y, b in want], m.font, vf, 2, 2)
    vf.close()
    assert os.listdir(vdir) == ["page.png"]
    assert np.array_equal(load_image_rgba(str(vdir / "page.png"))[..., :3], img)
    assert r.stderr.split() == [path, "%.6f" % (np.float32(sq) / np.float32(page.size))]
    r = subprocess.run(cmd + ["--whole-baseline", "4", "--pen-slack", "2", "-i", path], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--whole-baseline" in r.stderr


@pytest.mark.parametrize("i", range(12))
def test_fuzz_cases(dec, i):
    """The dozen seeded cases of tests/focr_whole_baseline_fuzz.py: Sans, Serif and Mono, 6 to 16 px, kerning 0.8 to 1.2,
    hinting on and off, an x and a y that are not 0 and a width that the page clips, ink up to 0.75 px off the baseline."""
    c = FZ.case(i)
    m = model(c.font, c.size, c.alphabet, c.y_bits, c.hinting, c.kerning)
    dec.set_font(m.font, c.size)
    want = _check(dec, m, [c.page], c.geo, c.n)
    assert sum(len(pg) for pg in want) > 0


def test_memory_returns():
    """A decoder that uploaded y-phase fonts and ran the mode, with a verify, gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    page = _offset_pages(MONO, 13.0, "ABx0+/", [(0.75, -1.0)], 60, seed=1)[0]
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, "ABx0+/", y_bits=2)
        d.decode([page], 2, 0, 58, 16, 16, whole_line=True)
        whole = N.hip().focr_debug_device_bytes()
        d.decode([page], 2, 0, 58, 16, 16, whole_line=True, whole_baseline=4, verify="mse")
        searched = N.hip().focr_debug_device_bytes()
        assert before < whole < searched  # the second half of the scratch, the lines' q and the verify's buffers
    assert N.hip().focr_debug_device_bytes() == before

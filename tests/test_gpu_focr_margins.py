"""The per-character margins of the focr whole-line decode (line_whole_margins_kernel, focr_decoder_set_whole_margins /
focr_decoder_get_margins, LineDecoder.decode(whole_line=True, margins=True), focr --whole-line --margins) against
tests/focr_margins_model.py, the definition of include/focr_decode.h restated with a forward and a backward table and
pinned by tests/test_focr_margins_model.py.  Every quantity is an exact integer, so terms, runners and margins are
compared with ==, and the texts, pens and costs of a margins run with those of a whole-line run without margins.  Each
test asserts from its geometry, or from the model's answer, that it reaches the case it names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_margins_model as MM
import focr_whole_model as W
from focr_fast_model import ALPHABET_319, TIE_GROUPS, FastModel, crop
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineDecoder, LineMargins, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536      # decode_line.h: strip, cost ring, live list and the characters' keys share this much LDS
WHOLE_MISC_BYTES = 1088    # decode_whole.hip: the end keys, the counts and the live list
WHOLE_BATCH_MAX = 512      # decode_whole.hip: states per batch at most
TEXT = "burn clip ffH vvill rnrn cl"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


_models, _lines = {}, {}


def model(font, size, alphabet):
    key = (font, size, alphabet)
    if key not in _models:
        _models[key] = FastModel(font, size, alphabet)
    return _models[key]


def want_line(fm, line):
    """The model's Margins of one crop, computed once per (model, crop)."""
    key = (id(fm), line.shape, line.tobytes())
    if key not in _lines:
        _lines[key] = MM.margins_line(fm, line)
    return _lines[key]


def want_pages(fm, pages, x, y, width, line_height, line_advance):
    """[[(y, Margins)] per page], over the crops FastModel.decode_image walks."""
    out = []
    for page in pages:
        out.append([])
        i = 0
        while True:
            ly = y + i * line_advance
            i += 1
            line = crop(page, x, ly, width, line_height)
            if line.shape[0] == 0:
                break
            if not np.all(line == 255):
                out[-1].append((ly, want_line(fm, np.ascontiguousarray(line))))
    return out


def ring_length(fm):
    inc = W.inc64(fm.incs)
    need, n = min(int(inc.min()), WHOLE_BATCH_MAX) + int(inc.max()), 64
    while n < need:
        n *= 2
    return n


def strip_bytes(w, line_height):
    return ((w + 7) // 4 + 2) * 4 * line_height


def chars_bytes(fm, w):
    """decode_whole.hip's whole_chars_dwords: a 64-bit key and a midpoint per character of the bound, in whole 16 bytes."""
    return ((3 * W.char_bound(fm.incs, w) + 3) & ~3) * 4


def same_margins(got, want, fm, where=None):
    assert isinstance(got, LineMargins) and got.term.dtype == np.int32 and got.margin.dtype == np.int64 and isinstance(got.runner, str), where
    assert np.array_equal(got.term, want.term), where
    assert got.runner == MM.runner_text(fm, want.runner), where
    assert np.array_equal(got.margin, want.margin), where


def check(dec, fm, pages, geo):
    """Decode whole lines without and with margins: the margins run's texts, pens and costs are the other run's and the
    model's, its margins the model's, in 3 launches.  Returns the model's pages."""
    want = want_pages(fm, pages, *geo)
    plain = dec.decode(pages, *geo, whole_line=True)
    lines, pens, costs, margins = dec.decode(pages, *geo, whole_line=True, margins=True)
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    assert lines == plain[0] == [[(y, s.text) for y, s in pg] for pg in want]
    assert costs == plain[2] == [[s.cost for _, s in pg] for pg in want]
    assert [len(pg) for pg in margins] == [len(pg) for pg in lines]
    for p, want_pg in enumerate(want):
        for k, (y, s) in enumerate(want_pg):
            assert np.array_equal(pens[p][k], plain[1][p][k]) and np.array_equal(pens[p][k], s.pens), (p, y)
            same_margins(margins[p][k], s, fm, (p, y))
            assert int(margins[p][k].term.astype(np.int64).sum()) == costs[p][k]
    return want


def put(page, line, y, x=0):
    h, w = min(line.shape[0], page.shape[0] - y), min(line.shape[1], page.shape[1] - x)
    page[y: y + h, x: x + w] = np.minimum(page[y: y + h, x: x + w], line[:h, :w])


def test_proportional_lines_in_a_batch(dec):
    """Sans 13 px, the default alphabet: the README's line and "Il1 O0o" in a 3-page batch of four slots a page, with blank
    slots between the inked ones and a blank page.  The smallest margins are the ones a reader would check."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(SANS, 13.0, al)
    a, b = W.draw_line(SANS, 13.0, al, TEXT), W.draw_line(SANS, 13.0, al, "Il1 O0o", width=157)
    h, w = a.shape
    assert (h, w) == (13, 157) and 64 * w > 4 * ring_length(fm)
    pages = np.full((3, 4 * h, w), 255, dtype=np.uint8)
    put(pages[0], a, 0), put(pages[0], b, 2 * h), put(pages[2], a, 3 * h)
    dec.set_font(fm.font, 13.0)
    want = check(dec, fm, pages, (0, 0, w, h, h))
    assert [[y for y, _ in pg] for pg in want] == [[0, 2 * h], [], [3 * h]]
    s, t = want[0][0][1], want[0][1][1]
    assert s.text[:-1] == TEXT and t.text[:7] == "Il1 O0o"
    assert {TEXT[k] for k in np.argsort(s.margin[: len(TEXT)])[:6]} <= set("li")
    assert MM.runner_text(fm, t.runner)[:2] == "lI" and t.margin[0] == t.margin[1] == t.margin[:7].min()


@pytest.mark.parametrize("size", [13.0, 32.0])
def test_monospace_line_and_the_plain_scores(dec, size):
    """Mono: one state in inc64 is reachable and most batches are empty.  Margins equal the model's, and, where the plain
    decoder renders the character at the same 26.6 delta (its f32 pen truncates to the character's state: the first
    character at 13 px, where the increment is 500.906 / 64 px and inc64 is 501; every character at 32 px, where it is
    1233 / 64 exactly: tests/test_focr_margins_model.py), runner and margin are the plain run's runner and
    runner_score - score, and term is its score - base."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(MONO, size, al)
    inc, = set(W.inc64(fm.incs).tolist())
    assert inc == (501 if size == 13.0 else 1233)
    line = W.draw_line(MONO, size, al, TEXT if size == 13.0 else "Il1 O0o")
    geo = (0, 0, line.shape[1], line.shape[0], line.shape[0])
    dec.set_font(fm.font, size)
    (_, s), = check(dec, fm, [line], geo)[0]
    assert np.all(s.pens % inc == 0)
    pos, same = np.float32(0), []
    for i, pen in zip(s.idx, s.pens):
        same.append(int(np.float32(np.float32(fm.ox + pos) * np.float32(64))) == 64 * int(fm.ox) + int(pen))
        pos = np.float32(pos + fm.incs[i])
    same = np.array(same)
    assert same[0] and (same.all() if size == 32.0 else not same[1:].any())
    plain, scores = dec.decode([line], *geo, scores=True)
    assert plain == [[(0, s.text)]]
    sc = scores[0][0]
    assert np.array_equal(sc.runner[same], s.runner[same]) and np.array_equal((sc.runner_score - sc.score)[same], s.margin[same])
    assert np.array_equal((sc.score - sc.base)[same], s.term.astype(np.int64)[same])


def test_ties_between_identical_glyphs(dec):
    """ALPHABET_319 in Mono 13 px with every tie group on the page: a chosen glyph with an identical twin has margin 0, and
    its runner is the lowest-index other twin."""
    al = ALPHABET_319
    fm = model(MONO, 13.0, al)
    text = "Ao Αο Ао A"  # Latin, Greek, Cyrillic
    line = W.draw_line(MONO, 13.0, al, text)
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    assert s.text[: len(text)] == "Ao Ao Ao A"
    twins = {min(grp, key=al.index): sorted(grp, key=al.index)[1] for grp in TIE_GROUPS}
    run = MM.runner_text(fm, s.runner)
    assert set(s.text[: len(text)]) == set(twins)
    for k in range(len(text)):
        assert run[k] == twins[s.text[k]] and s.margin[k] == 0, k


def test_glyphs_of_one_advance(dec):
    """Sans 13 px, "bdpqo il": b, d, p and q share one inc64, so their edges from one state cover the same midpoints and
    end in the same state; only their terms tell them apart, and the runner of each is another of the four."""
    al = "bdpqo il"
    fm = model(SANS, 13.0, al)
    inc = W.inc64(fm.incs)
    assert len({int(inc[al.index(c)]) for c in "bdpq"}) == 1 and len(set(inc.tolist())) >= 3
    line = W.draw_line(SANS, 13.0, al, "bdpq lid dip")
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    assert s.text[:12] == "bdpq lid dip" and set(MM.runner_text(fm, s.runner)[:4]) <= set("bdpqo")


def test_an_edge_that_covers_several_midpoints(dec):
    """Sans 13 px, "im", a line of ten "i": the runner of every "i" is an "m" three and a half times as wide, whose edge
    covers the midpoints of up to four characters at once and enters each one's key."""
    al = "im"
    fm = model(SANS, 13.0, al)
    line = W.draw_line(SANS, 13.0, al, "i" * 10)
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    inc = W.inc64(fm.incs)
    mids = s.pens.astype(np.int64) + (inc[s.idx] >> 1)
    covered = [int(((mids >= p) & (mids < p + inc[r])).sum()) for p, r in zip(s.runner_pen, s.runner)]
    assert s.text[:10] == "i" * 10 and MM.runner_text(fm, s.runner)[:10] == "m" * 10 and max(covered) >= 2
    # one edge is the runner of several characters: the same pen and through-cost in each one's key
    assert len({(int(p), int(m)) for p, m in zip(s.runner_pen, s.margin)}) < len(s.text)


def test_several_lines_per_workgroup(dec):
    """Seven non-blank lines on a grid of two workgroups, then on the decoder's own grid: each workgroup takes several
    lines in turn, and the forward keys in the scratch (a shorter line leaves states unreached that the line before
    reached), the ring and the runner keys of one line must not reach the next."""
    al = "burn clif"
    fm = model(SANS, 13.0, al)
    texts = ["burn clif", "ffill bull", "i" * 16, "rnrn club", "l l l l l", "curl brr", "fin ruf"]
    h = W.alphabet_height(SANS, 13.0, al)
    pages = np.full((2, 5 * h, 70), 255, dtype=np.uint8)
    for text, (p, slot) in zip(texts, [(0, 0), (0, 1), (0, 3), (0, 4), (1, 0), (1, 2), (1, 3)]):
        put(pages[p], W.draw_line(SANS, 13.0, al, text, width=70, height=h), slot * h)
    dec.set_font(fm.font, 13.0)
    assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 2) == 0
    try:
        want = check(dec, fm, pages, (0, 0, 70, h, h))
    finally:
        assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 0) == 0
    assert sum(len(pg) for pg in want) == 7 and len({s.text for pg in want for _, s in pg}) == 7
    assert len({len(s.text) for pg in want for _, s in pg}) > 1
    check(dec, fm, pages, (0, 0, 70, h, h))


def test_bottom_clip_and_x_start(dec):
    """x_start 3 and a last slot cut by the page's bottom edge to 8 of its 13 rows: the crop's own h clips every glyph, in
    the backward sweep and in the terms as in the programme."""
    al = "burn clif"
    fm = model(SANS, 13.0, al)
    h = W.alphabet_height(SANS, 13.0, al)
    page = np.full((h + 8, 64), 255, dtype=np.uint8)
    put(page, W.draw_line(SANS, 13.0, al, "burn club", width=60, height=h), 0, 3)
    put(page, W.draw_line(SANS, 13.0, al, "fill in", width=60, height=h), h, 3)
    dec.set_font(fm.font, 13.0)
    want = check(dec, fm, [page], (3, 0, 60, h, h))[0]
    assert [y for y, _ in want] == [0, h] and want[0][1].text[:9] == "burn club" and len(want[1][1].text) > 3


@pytest.mark.parametrize("width", [844, 848])
def test_strip_in_lds_and_in_global_memory(dec, width):
    """Mono 13 px, four glyphs, 64-row slots: at width 844 the strip fits in LDS beside the ring, the live list and the
    characters' keys and midpoints; at 848 it does not and is read from global memory, although it would still fit
    without the characters (the whole-line run without margins has it in LDS at both widths)."""
    al, lh = "AB >", 64
    fm = model(MONO, 13.0, al)
    fixed = WHOLE_MISC_BYTES + 8 * ring_length(fm)
    assert fixed + chars_bytes(fm, width) < LDS_STRIP_MAX  # the characters themselves are in LDS
    assert (strip_bytes(width, lh) + fixed + chars_bytes(fm, width) <= LDS_STRIP_MAX) == (width == 844)
    assert strip_bytes(848, lh) + fixed <= LDS_STRIP_MAX
    rng = np.random.default_rng(width)
    page = np.full((lh, 900), 255, dtype=np.uint8)
    put(page, W.draw_line(MONO, 13.0, al, "".join(rng.choice(list(al), 114)), width=900, height=16), 20)
    page[:, 790:] = np.minimum(page[:, 790:], 200)  # ink in the last columns of either width
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [page], (0, 0, width, lh, lh))[0]
    assert len(s.text) >= width // 8


@pytest.mark.parametrize("width,line_height", [(340, 13), (500, 128)])
def test_characters_in_the_scratch(dec, width, line_height):
    """A hand-built font of two glyphs that advance by 4/64 and 8/64 px: a line may hold 16 characters a pixel, and at
    these widths their keys and midpoints do not fit in LDS beside the ring and live in the workgroup's scratch, with the
    strip in LDS (340 x 13) and in global memory (500 x 128).  Batches are four states long."""
    al = "AB"
    fm = FastModel(MONO, 13.0, al)
    fm.font.s.glyphs[0].increment, fm.font.s.glyphs[1].increment = 4 / 64, 8 / 64
    fm.incs = fm.font.increments()
    assert W.inc64(fm.incs).tolist() == [4, 8] and W.char_bound(fm.incs, width) == 16 * width
    fixed = WHOLE_MISC_BYTES + 8 * ring_length(fm)
    assert fixed + chars_bytes(fm, width) > LDS_STRIP_MAX
    assert (strip_bytes(width, line_height) + fixed <= LDS_STRIP_MAX) == (line_height == 13)
    page = np.full((line_height, width), 255, dtype=np.uint8)
    put(page, W.draw_line(MONO, 13.0, al, "ABBA"), 0, 2)
    put(page, W.draw_line(MONO, 13.0, al, "BAB"), 0, width - 40)
    try:
        dec.set_font(fm.font, 13.0)
        (_, s), = check(dec, fm, [page], (0, 0, width, line_height, line_height))[0]
        assert len(s.text) > 5 * width and len(set(s.text)) == 2 and np.any(s.margin > 0)
    finally:
        dec.font = None
        fm.close()


def test_batch_capped_below_the_smallest_advance(dec):
    """Sans 32 px, "il m": the smallest inc64 is 569, above the 512 states a batch may hold, so batches are shorter than
    every step, in the backward sweep as in the programme."""
    al = "il m"
    fm = model(SANS, 32.0, al)
    inc = W.inc64(fm.incs)
    assert int(inc.min()) > WHOLE_BATCH_MAX and len(set(inc.tolist())) >= 3
    line = W.draw_line(SANS, 32.0, al, "ill mil")
    dec.set_font(fm.font, 32.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    assert s.text[:7] == "ill mil" and 64 * line.shape[1] > 4 * WHOLE_BATCH_MAX


def test_one_glyph_alphabet(dec):
    """No other glyph, no covering edge of another glyph: the runner is "\\0" (0xFFFF in the C API) and the margin -1."""
    fm = model(MONO, 13.0, "A")
    line = W.draw_line(MONO, 13.0, "A", "AAA")
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    assert np.all(s.runner == MM.NO_RUNNER) and np.all(s.margin == -1) and len(s.text) >= 3
    ms = np.zeros(len(s.text), dtype=np.dtype([("term", "<i4"), ("runner", "<u2"), ("pad", "<u2"), ("margin", "<i8")]))
    assert dec._lib.focr_decoder_get_margins(dec._h, ms.ctypes.data) == 0
    assert np.all(ms["runner"] == 0xFFFF) and np.all(ms["margin"] == -1) and np.all(ms["pad"] == 0)
    assert np.array_equal(ms["term"], s.term)


def _raw_run(dec, page, x, y, width, line_height, line_advance):
    """focr_decoder_run of one page with whatever state the library is in: (return code, its message)."""
    page = np.ascontiguousarray(page)
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], x, y, width, line_height,
                                   line_advance)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def test_refusals(dec):
    """Margins with the whole-line decode off are refused by focr_decoder_run with a message that names both;
    focr_decoder_get_margins fails after a plain run and after a whole-line run without margins; whole-line with scores
    is still refused, with margins as without; the decoder decodes afterwards."""
    al = "burn clif"
    fm = model(SANS, 13.0, al)
    line = W.draw_line(SANS, 13.0, al, "burn")
    geo = (0, 0, line.shape[1], line.shape[0], line.shape[0])
    lib, h = dec._lib, dec._h
    dec.set_font(fm.font, 13.0)
    dec.decode([line], *geo, whole_line=True, margins=True)
    assert lib.focr_decoder_get_margins(h, None) == 0
    dec.decode([line], *geo)  # the Python API switches both off
    assert lib.focr_decoder_get_margins(h, None) != 0 and b"focr_decoder_get_margins" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_whole_margins(h, 1) == 0
    try:
        rc, msg = _raw_run(dec, line, *geo)
        assert rc != 0 and "focr_decoder_run: margins on with the whole-line decode off" in msg, msg
        assert "focr_decoder_set_whole_margins" in msg and "focr_decoder_set_whole_line" in msg
        assert lib.focr_decoder_n_lines(h) == 0 and lib.focr_decoder_last_launches(h) == 0
        assert lib.focr_decoder_get_margins(h, None) != 0 and lib.focr_decoder_get_pens(h, None, None) != 0
        # whole-line with scores: refused as before, whatever the margins switch says
        assert lib.focr_decoder_set_whole_line(h, 1) == 0 and lib.focr_decoder_set_scores(h, 1) == 0
        for on in (1, 0):
            assert lib.focr_decoder_set_whole_margins(h, on) == 0
            rc, msg = _raw_run(dec, line, *geo)
            assert rc != 0 and "whole-line decode with scores on (a runner-up has no definition under the dynamic programme)" in msg, msg
    finally:
        assert lib.focr_decoder_set_scores(h, 0) == 0 and lib.focr_decoder_set_whole_line(h, 0) == 0
        assert lib.focr_decoder_set_whole_margins(h, 0) == 0
    with pytest.raises(ValueError, match="margins=True needs whole_line=True"):
        dec.decode([line], *geo, margins=True)
    with pytest.raises(ValueError, match="a runner-up has no definition"):
        dec.decode([line], *geo, whole_line=True, margins=True, scores=True)
    dec.decode([line], *geo, whole_line=True)
    assert lib.focr_decoder_get_pens(h, None, None) == 0 and lib.focr_decoder_get_margins(h, None) != 0
    with pytest.raises(DecoderError, match="was not a margins run"):
        dec._check(lib.focr_decoder_get_margins(h, None))
    check(dec, fm, [line], geo)


def test_off_path_and_memory(dec):
    """After margins were on, a whole-line run and a plain run (scores and verify included) return what a fresh decoder
    returns, in 3 launches; a decoder that ran margins gives every byte of device memory back; decode_device returns the
    margins of decode."""
    al = FOCR_DEFAULT_ALPHABET
    a = W.draw_line(SANS, 13.0, al, TEXT)
    h, w = a.shape
    pages = np.full((2, 3 * h, w), 255, dtype=np.uint8)
    put(pages[0], a, 0), put(pages[1], W.draw_line(SANS, 13.0, al, "Il1 O0o", width=w), 2 * h)
    geo = (0, 0, w, h, h)
    before = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as fresh:
        fresh.set_font(SANS, 13.0)
        whole = fresh.decode(pages, *geo, whole_line=True, verify="image")
        plain = fresh.decode(pages, *geo, verify="image", scores=True)
        held = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as d:
        d.set_font(SANS, 13.0)
        got = d.decode(pages, *geo, whole_line=True, margins=True)
        assert len(got) == 4 and N.hip().focr_debug_device_bytes() > before
        hip = C.CDLL("libamdhip64.so.7")
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(pages.nbytes)) == 0
        try:
            assert hip.hipMemcpy(ptr, C.c_void_p(pages.ctypes.data), C.c_size_t(pages.nbytes), 1) == 0  # hipMemcpyHostToDevice
            assert hip.hipDeviceSynchronize() == 0
            on_dev = d.decode_device(ptr.value, *pages.shape, *geo, whole_line=True, margins=True)
        finally:
            assert hip.hipFree(ptr) == 0
        assert len(on_dev) == 4 and on_dev[0] == got[0] and on_dev[2] == got[2]
        for a_pg, b_pg in zip(on_dev[3], got[3]):
            assert [m.runner for m in a_pg] == [m.runner for m in b_pg]
            assert all(np.array_equal(x.term, y.term) and np.array_equal(x.margin, y.margin) for x, y in zip(a_pg, b_pg))
        again = d.decode(pages, *geo, whole_line=True, verify="image")
        assert d._lib.focr_decoder_last_launches(d._h) == 3 and d._lib.focr_decoder_get_margins(d._h, None) != 0
        assert again[0] == whole[0] == got[0] and again[1].tobytes() == whole[1].tobytes() and again[4] == whole[4] == got[2]
        assert all(np.array_equal(x, y) for x, y in zip(again[2], whole[2]))
        assert all(np.array_equal(x, y) for pa, pb in zip(again[3], whole[3]) for x, y in zip(pa, pb))
        off = d.decode(pages, *geo, verify="image", scores=True)
        assert d._lib.focr_decoder_last_launches(d._h) == 3
        assert off[0] == plain[0] and off[1].tobytes() == plain[1].tobytes() and all(np.array_equal(x, y) for x, y in zip(off[2], plain[2]))
        for a_pg, b_pg in zip(off[3], plain[3]):
            assert len(a_pg) == len(b_pg)
            for x, y in zip(a_pg, b_pg):
                assert x.base == y.base and all(np.array_equal(x[f], y[f]) for f in (1, 2, 3))
        assert N.hip().focr_debug_device_bytes() > held  # the margins' own buffers are still the decoder's
    assert N.hip().focr_debug_device_bytes() == before


def test_cli(dec, tmp_path):
    """focr --whole-line --margins on two PGMs: the CSV rows are the Python API's pens and margins, stdout is byte-equal
    to the run without --margins, and so is the verify's MSE line."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    al = FOCR_DEFAULT_ALPHABET
    line = W.draw_line(SANS, 13.0, al, TEXT)
    h, w = line.shape
    pages = np.full((2, 2 * h, w), 255, dtype=np.uint8)
    put(pages[0], line, h), put(pages[1], W.draw_line(SANS, 13.0, al, "Il1 O0o", width=w), 0)
    paths = [str(tmp_path / ("page%d.pgm" % i)) for i in range(2)]
    for path, page in zip(paths, pages):
        save_pgm(path, page)
    csv, vdir = tmp_path / "margins.csv", tmp_path / "v"
    vdir.mkdir()
    cmd = [FOCR, "-f", SANS, "-t", "13", "-w", str(w), "--line-height", str(h), "--line-advance", str(h), "--whole-line", "--verify", str(vdir),
           "-i"] + paths
    base = subprocess.run(cmd, capture_output=True, timeout=300)
    r = subprocess.run(cmd[:1] + ["--margins", str(csv)] + cmd[1:], capture_output=True, timeout=300)
    assert base.returncode == 0 and r.returncode == 0, r.stderr
    assert r.stdout == base.stdout and r.stderr == base.stderr and r.stdout[: len(TEXT)] == TEXT.encode()
    dec.set_font(SANS, 13.0)
    lines, pens, _, margins = dec.decode(pages, 0, 0, w, h, h, whole_line=True, margins=True)
    rows = ["image_index,y,column,codepoint,pen,term,runner_codepoint,margin"]
    for i in range(2):
        for (y, text), pen, m in zip(lines[i], pens[i], margins[i]):
            rows += ["%d,%d,%d,%d,%d,%d,%d,%d" % (i, y, c, ord(text[c]), pen[c], m.term[c], ord(m.runner[c]), m.margin[c]) for c in range(len(text))]
    assert csv.read_text().splitlines() == rows and len(rows) > len(TEXT) + 8
    # a one-glyph alphabet: the last two fields are empty
    r = subprocess.run([FOCR, "-f", SANS, "-t", "13", "-a", "l", "-w", str(w), "--line-height", str(h), "--line-advance", str(h), "--whole-line",
                        "--margins", str(csv), "-i", paths[1]], capture_output=True, text=True, timeout=300)
    got = csv.read_text().splitlines()
    assert r.returncode == 0 and len(got) > 10 and all(ln.endswith(",,") and ln.count(",") == 7 for ln in got[1:])

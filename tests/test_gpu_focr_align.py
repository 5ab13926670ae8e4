"""focr_decoder_align_text (align_text_kernel, align_strip_kernel, LineDecoder.align_text / rank_text_aligned, focr --rank-drift): a
forced alignment of a caller's lines.  Device == tests/focr_align_model.py (the definition state by state, its terms one FreeType
raster per glyph and pen) at the shapes the kernel branches on: the band against the workgroup's 256 threads and the wave's 64
lanes, the step against the band, the line's length, dead states at start 0, the strip in LDS and in global memory, empty and
one-column crops, ties, a candidate font, y-phase fonts; then score_text on the device at the fitted pens; every refusal; the
last run's getters; device memory; the CLI; and the seeded pages of tests/focr_fuzz_cases.py under the readings of
tests/focr_text_fuzz.py.  Every comparison is ==.  Pages are small but for those whose strips must leave LDS."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_align_model as A
import focr_fuzz_cases as FC
import focr_score_text_model as S
import focr_text_fuzz as TF
from focr_fast_model import crop
from font_ocr_amd import LineDecoder, fit_pens, nominal_pens, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import raster_glyph
from test_gpu_focr_score_text import AL, FOCR, LH, MONO, SANS, SERIF, fonts_of, noisy, snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def launches(dec):
    return dec._lib.focr_decoder_last_align_text_launches(dec._h)


def want_line(font, page, x, y, width, lh, text_idx, start, drift, step, q=0, y_bits=0):
    """The model's Align of one line: alphabet indices text_idx in the DecodeFont `font` at slot (x, y) of a luma page."""
    ref = crop(np.asarray(page), x, y, width, lh)
    return A.align(A.raster_term(font, ref, text_idx, q, y_bits), A.nominal(font.increments(), text_idx, start), drift, step, A.base_of(ref))


def check(dec, pages, lines, x, width, lh, fonts=None, baselines=None, y_bits=0, start=0, drift=2, step=1, n_launches=1):
    """align_text equals the model line by line: base, cost, first, last, every pen and every term."""
    got = dec.align_text(pages, lines, x, width, lh, fonts=fonts, baselines=baselines, y_bits=y_bits, start=start, drift=drift, step=step)
    assert launches(dec) == (n_launches if any(lines) else 0)
    for p, page in enumerate(pages):
        assert len(got[p]) == len(lines[p])
        for q, (y, text) in enumerate(lines[p]):
            font = fonts_of(dec)[fonts[p][q] if fonts is not None else 0]
            want = want_line(font, page, x, y, width, lh, [font.alphabet.index(c) for c in text], start, drift, step,
                             0 if baselines is None else baselines[p][q], y_bits)
            g = got[p][q]
            assert (g.base, g.cost, g.first, g.last) == (want.base, want.cost, want.first, want.last), (p, q, g[:4], want[:4])
            assert g.pens.dtype == np.uint32 and np.array_equal(g.pens, want.pens), (p, q)
            assert g.terms.dtype == np.int32 and np.array_equal(g.terms, want.terms), (p, q)
    return got


# ---- against the model, where the kernel branches ---------------------------------------------------------------------------

# (W, N): bands of 1, 3, 63, 65, 255, 257 and 2049 states; N = 0, 1 and 64, and an N above 2W
BANDS = [(0, 0), (0, 3), (1, 1), (1, 64), (31, 1), (32, 64), (127, 0), (128, 1), (128, 7)]


@pytest.mark.parametrize("drift,step", BANDS)
@pytest.mark.parametrize("start", [0, 200])
def test_band_widths_and_steps(dec, drift, step, start):
    """One thread, three, a wave less a lane, a wave and a lane, the workgroup less a thread, the workgroup and a thread; at
    start 0 the negative half of the first characters' band is dead.  On noise, where every state costs something else."""
    dec.set_font(SANS, 13.0, AL)
    dec.set_font_candidates([])
    check(dec, [noisy(90, 24, 7)], [[(3, "Hi mob"), (5, "ahoi")]], 4, 80, LH, start=start, drift=drift, step=step)


def test_the_widest_band(dec):
    """W = 1024: 2049 states, nine passes of the workgroup per character; five characters, so that the model stays quick.  The two
    cost rows (32 784 bytes) still leave the strip its place in LDS; on a wider crop they do not (test_strip_...)."""
    dec.set_font(SANS, 13.0, AL)
    dec.set_font_candidates([])
    check(dec, [noisy(70, 20, 9)], [[(1, "Hi ab")]], 2, 60, LH, start=0, drift=1024, step=64)
    check(dec, [noisy(70, 20, 9)], [[(1, "Hi ab")]], 2, 60, LH, start=1100, drift=1024, step=3)


def test_wide_tiles(dec):
    """Sans 30 px over "il.W@m": tiles of 2, 7 and 8 dwords a row (every font above is 13 px, at most 4 dwords) under a band of five
    states, the last W cut by the crop's right edge and the tall glyphs by its bottom."""
    font = dec.set_font(SANS, 30.0, "il.W@m")
    dec.set_font_candidates([])
    assert {font.s.glyphs[i].stride // 4 for i in range(6)} == {2, 7, 8}
    check(dec, [noisy(130, 40, 17)], [[(2, "W@mil."), (9, "lmWW")]], 3, 96, 26, start=40, drift=2, step=1)


def test_line_lengths(dec):
    """Lines of 0, 1, 64, 65 and 300 characters: the walk back and the terms' second pass over one thread, a full wave, a wave and
    a thread, the workgroup and 44.  The longest runs far past the crop: its last glyphs lie wholly right of it and cost 0, so
    the ranks decide there and their offset stays what the last inked character left."""
    dec.set_font(MONO, 8.0, AL)
    dec.set_font_candidates([])
    rng = np.random.default_rng(5)
    texts = ["".join(rng.choice(list(AL), n)) for n in (0, 1, 64, 65, 300)]
    pages = [noisy(330, 30, 51)]
    lines = [[(0, texts[0]), (0, texts[1]), (3, texts[2]), (9, texts[3]), (14, texts[4])]]
    for start in (0, 70):
        got = check(dec, pages, lines, 3, 320, 12, start=start, drift=3, step=1)
    g = got[0][0]
    assert (g.cost, g.first, g.last, len(g.pens), len(g.terms)) == (0, 0, 0, 0, 0) and g.base > 0
    long = got[0][4]
    assert not long.terms[-150:].any() and long.terms[:60].any()
    assert len({int(p) - int(m) for p, m in zip(long.pens[-150:], nominal_pens(dec.font, texts[4], 70)[-150:])}) == 1


@pytest.mark.parametrize("width,drift,n_launches", [(4072, 2, 1), (4073, 2, 2), (3000, 2, 1), (3000, 1024, 2)])
def test_strip_in_lds_and_in_global_memory(dec, width, drift, n_launches):
    """A 4100 x 17 page under a band of five states: 16 rows of 4072 columns just fit LDS beside the waves' sums and the two cost
    rows, one column more does not, and the strips are then built in global memory by a launch of their own.  3000 columns fit
    beside five states and not beside 2049.  Glyphs at both ends of the crop and in the middle, by `start`."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    pages = [noisy(4100, 17, 101)]
    if drift == 1024:  # one short line: the model draws every state of the band on the wide crop
        check(dec, pages, [[(1, "Hm")]], 0, width, 16, start=64 * (width - 20), drift=drift, step=5, n_launches=n_launches)
        return
    for start in (0, 64 * (width - 9)):
        check(dec, pages, [[(0, "Hm"), (1, "abe")]], 0, width, 16, start=start, drift=drift, step=2, n_launches=n_launches)
    check(dec, pages, [[(1, "oh")]], 0, width, 16, start=64 * 1500 + 7, drift=drift, step=1, n_launches=n_launches)


def test_crops_and_ties(dec):
    """A crop one column wide; y past the page and x at the page's edge (empty crops: every term 0, so the ranks give e = 0
    throughout and the pens are the nominal ones); a line of spaces on ink (the same, with a base); a glyph wholly right of the crop."""
    dec.set_font(SANS, 13.0, AL)
    dec.set_font_candidates([])
    pages = [noisy(70, 30, 91)]
    check(dec, pages, [[(5, "Hi"), (6, "ab")]], 9, 1, LH, start=100, drift=40, step=2)
    for x, y in ((3, 30), (3, 1000), (70, 2), (5000, 2)):
        got = check(dec, pages, [[(y, "Hinein")]], x, 60, LH, start=5, drift=9, step=3)
        g = got[0][0]
        assert (g.base, g.cost, g.first, g.last) == (0, 0, 0, 0) and not g.terms.any() and list(g.pens) == list(nominal_pens(dec.font, "Hinein", 5))
    got = check(dec, pages, [[(2, "    ")]], 3, 60, LH, start=0, drift=70, step=64)
    g = got[0][0]
    assert g.base > 0 and (g.cost, g.first, g.last) == (0, 0, 0) and list(g.pens) == list(nominal_pens(dec.font, "    ", 0))
    got = check(dec, pages, [[(2, "Hi H")]], 3, 12, LH, start=64, drift=20, step=4)  # the second H starts right of the crop's 12 columns
    assert got[0][0].terms[-1] == 0 and got[0][0].terms[0] != 0


def test_candidate_fonts_and_baselines(dec):
    """A candidate font with increments of its own; q with rows moved (B = 0) and fractional with the y-phase fonts (B = 2), per
    line; a candidate at a whole q."""
    dec.set_font(MONO, 13.0, AL, y_bits=2)
    dec.set_font_candidates([(SANS, 13.0, False, 1.0), (SERIF, 12.0, False, 1.0)])
    pages = [noisy(120, 44, 81)]
    lines = [[(2, "Hinein"), (2, "Hinein"), (22, "ab Hm"), (22, "mohr")]]
    check(dec, pages, lines, 4, 100, LH, fonts=[[0, 1, 2, 1]], start=30, drift=5, step=2)
    check(dec, pages, lines, 4, 100, LH, fonts=[[0, 1, 0, 2]], baselines=[[-2, 3, 0, -1]], y_bits=0, start=0, drift=4, step=1)
    check(dec, pages, lines, 4, 100, LH, fonts=[[0, 1, 0, 2]], baselines=[[-5, 8, 7, -4]], y_bits=2, start=9, drift=4, step=4)


def raw(dec, batch, x, width, lh, recs, chars, qs=None, y_bits=0, start=0, drift=2, step=1, want_terms=True, pens=True, out=True):
    """focr_decoder_align_text as it is: recs are (page, y, first, n_chars, font).  Returns (rc, results, pens, terms)."""
    n, H, W = batch.shape
    larr = (N.TextLine * max(1, len(recs)))(*recs)
    carr = np.asarray(chars, dtype=np.uint16) if len(chars) else np.zeros(1, dtype=np.uint16)
    qarr = None if qs is None else np.asarray(qs, dtype=np.int8)
    n_out = max(1, sum(r[3] for r in recs if r[3] < 1 << 20))
    parr, tarr = np.full(n_out, 7, dtype=np.uint32), np.full(n_out, 7, dtype=np.int32)
    aarr = (N.TextAlignStruct * max(1, len(recs)))()
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = dec._lib.focr_decoder_align_text(dec._h, ptr(batch), 0, n, W, H, x, width, lh, larr, len(recs), ptr(carr), len(chars), ptr(qarr), y_bits,
                                          start, drift, step, ptr(parr) if pens else None, ptr(tarr) if want_terms else None, aarr if out else None)
    return rc, [(a.line_base, a.cost, a.first, a.last) for a in aarr][: len(recs)], parr, tarr


def test_reverse_page_order_and_shared_characters(dec):
    """Lines of different lengths that share their characters, in descending page order, one listed twice, an empty one, a page
    without a line, in one call; then without terms."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([(SANS, 13.0, False, 1.0)])
    batch = np.ascontiguousarray(np.stack([noisy(100, 40, s) for s in (111, 112, 113)]))
    chars = [AL.index(c) for c in "Hinein im ohr"]
    recs = [(2, 20, 0, len(chars), 0), (2, 3, 0, len(chars), 1), (0, 3, 3, 5, 0), (0, 3, 3, 5, 0), (2, 20, 7, 0, 1), (0, 9, 11, 2, 1)]
    rc, got, pens, terms = raw(dec, batch, 4, 90, LH, recs, chars, start=10, drift=6, step=2)
    assert rc == 0 and launches(dec) == 1
    at = 0
    for (page, y, first, n, font), g in zip(recs, got):
        want = want_line(fonts_of(dec)[font], batch[page], 4, y, 90, LH, chars[first: first + n], 10, 6, 2)
        assert g == (want.base, want.cost, want.first, want.last), (g, want[:4])
        assert np.array_equal(pens[at: at + n], want.pens) and np.array_equal(terms[at: at + n], want.terms)
        at += n
    assert got[2] == got[3] and at == len(terms)
    rc, again, pens2, terms2 = raw(dec, batch, 4, 90, LH, recs, chars, start=10, drift=6, step=2, want_terms=False)
    assert rc == 0 and again == got and np.array_equal(pens2, pens) and (terms2 == 7).all()


# ---- on the device alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("font,start,drift,step", [(SANS, 64, 128, 4), (SERIF, 64, 128, 32), (MONO, 0, 40, 8)])
def test_score_text_at_the_fitted_pens(dec, font, start, drift, step):
    """score_text(pens=align's pens) returns align's base, cost and terms; rank_text_aligned is align_text listed per font, with
    fit_pens of each."""
    dec.set_font(font, 13.0, AL)
    dec.set_font_candidates([(MONO, 12.0, False, 1.0)])
    page = S.draw_text(dec.font, "Hinein bin ihr", 150, LH, shift64=23)
    page = np.minimum(page, noisy(150, LH, 3) | 0x80)
    lines = [[(0, "Hinein bin ihr"), (0, "Hm")]]
    got = dec.align_text([page], lines, 0, 146, LH, fonts=[[0, 1]], start=start, drift=drift, step=step)
    back = dec.score_text([page], lines, 0, 146, LH, fonts=[[0, 1]], pens=[[a.pens for a in got[0]]])
    for a, s in zip(got[0], back[0]):
        assert (a.base, a.cost, 0) == (s.base, s.cost, s.shift) and np.array_equal(a.terms, s.terms) and a.cost == int(a.terms.sum())
    base, cost, first, last, fits = dec.rank_text_aligned(page, 0, "Hinein bin ihr", 0, 146, LH, start=start, drift=drift, step=step)
    both = dec.align_text([page], [[lines[0][0]] * 2], 0, 146, LH, fonts=[[0, 1]], start=start, drift=drift, step=step)[0]
    assert base == both[0].base and list(cost) == [a.cost for a in both] and list(first) == [a.first for a in both] and list(last) == [a.last for a in both]
    assert fits == [fit_pens(nominal_pens(f, "Hinein bin ihr", start), a.pens, a.terms, start) for f, a in zip(fonts_of(dec), both)]
    assert int(np.argmin(cost)) == 0
    with pytest.raises(TypeError):  # rank_text is what it was: a shift and a drift do not combine
        dec.rank_text(page, 0, "Hm", 0, 146, LH, shift=1, drift=2)


@pytest.mark.parametrize("drift", [0, 1, 17, 64])
def test_no_step_is_score_texts_shift_search(dec, drift):
    """N = 0 with start >= W: score_text(shift=W) over the nominal pens returns align's cost, terms and first."""
    dec.set_font(SANS, 13.0, AL)
    dec.set_font_candidates([(MONO, 13.0, False, 1.0)])
    page = noisy(150, 40, 17)
    lines = [[(0, "Hinein bin ihr"), (20, "mohr ab"), (21, "")]]
    got = dec.align_text([page], lines, 2, 140, LH, fonts=[[0, 1, 0]], start=64, drift=drift, step=0)
    noms = [[nominal_pens(fonts_of(dec)[k], t, 64) for k, (_, t) in zip([0, 1, 0], lines[0])]]
    rigid = dec.score_text([page], lines, 2, 140, LH, fonts=[[0, 1, 0]], pens=noms, shift=drift)
    for a, s in zip(got[0], rigid[0]):
        assert (a.base, a.cost, a.first, a.last) == (s.base, s.cost, s.shift, s.shift) and np.array_equal(a.terms, s.terms)


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(dec):
    """Every refusal of include/focr_decode.h, each with its own words and nothing launched or written; the decoder aligns afterwards."""
    lib, h = dec._lib, dec._h
    batch = np.ascontiguousarray(np.stack([noisy(80, 20, 31), noisy(80, 20, 32)]))
    with LineDecoder(0) as bare:  # no decode font
        rc = raw(bare, batch, 0, 80, LH, [], [])[0]
        assert rc != 0 and b"focr_decoder_align_text: no decode font (focr_decoder_set_font)" in bare._lib.focr_decoder_last_error(bare._h)
        assert launches(bare) == 0
    dec.set_font(MONO, 13.0, AL, y_bits=2)
    dec.set_font_candidates([(SANS, 13.0, False, 1.0)])
    chars = [AL.index(c) for c in "ahoi"]
    good = [(0, 2, 0, 4, 0), (1, 2, 0, 4, 1)]
    seen = set()

    def refused(*words, **kw):
        args = dict(x=1, width=70, lh=LH, recs=good, chars=chars)
        args.update(kw)
        assert raw(dec, batch, 1, 70, LH, good, chars)[0] == 0 and launches(dec) == 1
        rc, _, pens, terms = raw(dec, batch, **args)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and msg.startswith("focr_decoder_align_text: ") and all(w in msg for w in words), msg
        assert launches(dec) == 0 and lib.focr_decoder_last_align_text_ms(h) == 0.0 and (terms == 7).all() and (pens == 7).all() and msg not in seen
        seen.add(msg)

    refused("width 0", width=0)
    refused("line_height 0", lh=0)
    refused("drift radius", "1024", drift=1025)
    refused("step radius", "64", step=65)
    refused("y_bits", "3", y_bits=4)
    refused("line 1", "font 2", "1 candidates", recs=[good[0], (1, 2, 0, 4, 2)])
    refused("line 1", "page 2 of 2", recs=[good[0], (2, 2, 0, 4, 0)])
    refused("line 0", "n_chars", recs=[(0, 2, 1, 4, 0)])
    refused("character 2", "alphabet", chars=[0, 1, len(AL), 2])
    refused("line_q", "y_bits > 0", "focr_decoder_set_baseline_fonts", qs=[1, 0], y_bits=3)  # the y-phase fonts are of y_bits 2
    refused("line 1", "fractional-phase q", "one vertical phase", qs=[1, 2], y_bits=2)
    inc = int(nominal_pens(dec.font, "ah", 0)[1])  # Mono: every advance
    assert raw(dec, batch, 1, 70, LH, good[:1], chars, start=(1 << 24) - 4 * inc - 3, drift=2)[0] == 0  # the last start accepted
    refused("line 0", "2^24", "sum of its increments", recs=good[:1], start=(1 << 24) - 4 * inc - 2, drift=2)
    refused("null pens_out", pens=False)
    refused("null out", out=False)
    # the backpointers: 2049 states x 131 009 listed characters pass 256 MiB by 31 457 bytes; one line less does not (a call
    # of 131 008 characters is not made here: it would be accepted and run)
    many = [(0, 2, 0, 4, 0)] * 32752 + [(0, 2, 0, 1, 0)]
    refused("backpointers", "131009 characters x 2049 states", "256 MiB", "list fewer lines or ask for less drift", recs=many, drift=1024)
    # origins: built fonts have whole ones, so bend a copy of the candidate's struct
    cand = dec._candidates[0]
    keep = (cand.s.origin_x, cand.s.origin_y)
    for ox, oy, words, kw in ((0.5, keep[1], ("line 1", "alignment", "origin_x", "whole number"), {}),
                              (-1.0, keep[1], ("line 1", "alignment", "origin_x", "whole number"), {}),
                              (keep[0], 9.5, ("line 1", "line_q", "origin_y", "whole number"), dict(qs=[0, 0]))):
        cand.s.origin_x, cand.s.origin_y = ox, oy
        assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
        rc, _, pens, _ = raw(dec, batch, 1, 70, LH, good, chars, **kw)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and all(w in msg for w in words) and launches(dec) == 0 and (pens == 7).all(), msg
        assert raw(dec, batch, 1, 70, LH, good[:1], chars, **kw)[0] == 0  # font 0 alone is not touched by it
    cand.s.origin_x, cand.s.origin_y = keep
    assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
    larr, carr, out, pens = (N.TextLine * 2)(*good), np.asarray(chars, dtype=np.uint16), (N.TextAlignStruct * 2)(), np.zeros(8, dtype=np.uint32)
    f = lib.focr_decoder_align_text
    pp = pens.ctypes.data
    for words, call in (("null pages", lambda: f(h, None, 0, 2, 80, 20, 1, 70, LH, larr, 2, carr.ctypes.data, 4, None, 0, 0, 2, 1, pp, None, out)),
                        ("null lines", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, None, 2, carr.ctypes.data, 4, None, 0, 0, 2, 1, pp, None, out)),
                        ("null chars", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, larr, 2, None, 4, None, 0, 0, 2, 1, pp, None, out)),
                        ("page too large", lambda: f(h, batch.ctypes.data, 0, 2, 0xffff * 16 + 1, 20, 1, 70, LH, larr, 0, carr.ctypes.data, 4, None, 0, 0, 2, 1, pp, None, out))):
        assert raw(dec, batch, 1, 70, LH, good, chars)[0] == 0 and launches(dec) == 1
        assert call() != 0
        msg = lib.focr_decoder_last_error(h).decode()
        assert msg.startswith("focr_decoder_align_text: ") and words in msg and launches(dec) == 0 and msg not in seen
        seen.add(msg)
    # usable afterwards
    check(dec, list(batch), [[(2, "ahoi")], [(2, "ahoi")]], 1, 70, LH, fonts=[[0], [1]], start=3, drift=4, step=2)
    for kw, words in ((dict(drift=1025), "drift must be"), (dict(step=65), "step must be"), (dict(start=1 << 24), "start must be"), (dict(y_bits=4), "y_bits must be")):
        with pytest.raises(ValueError, match=words):
            dec.align_text(list(batch), [[(2, "ahoi")], []], 1, 70, LH, **kw)
    with pytest.raises(ValueError, match="not in the alphabet"):
        dec.align_text(list(batch), [[(2, "ahoy")], []], 1, 70, LH)


# ---- the last run, memory, the CLI ------------------------------------------------------------------------------------------------

def test_a_decode_before_the_call_answers_the_same_afterwards(dec):
    """A whole-line decode, then align_text of its own reading in the LDS and the global-strip form: the run's getters, timings
    and verify, and score_text's and verify_text's last timings, answer afterwards as they did before."""
    dec.set_font(SANS, 13.0, AL)
    dec.set_font_candidates([])
    pages = [S.draw_text(dec.font, "Hinein bin ihr", 150, LH), S.draw_text(dec.font, "mohr ahoi", 150, LH, shift64=9)]
    lines, pens, costs = dec.decode(pages, 0, 0, 146, LH, LH, whole_line=True)
    dec.score_text(pages, lines, 0, 146, LH, pens=pens)
    dec.verify_text(pages, lines, 0, pens=pens)
    lib, h = dec._lib, dec._h
    timings = lambda: (lib.focr_decoder_last_score_text_ms(h), lib.focr_decoder_last_score_text_launches(h),  # noqa: E731
                       lib.focr_decoder_last_verify_text_ms(h), lib.focr_decoder_last_verify_text_launches(h))
    before, tb = snapshot(dec), timings()
    got = dec.align_text(pages, lines, 0, 146, LH, start=0, drift=16, step=2)
    assert launches(dec) == 1 and lib.focr_decoder_last_align_text_ms(h) > 0
    for p in range(2):
        for a, c in zip(got[p], costs[p]):
            assert a.cost <= c  # the run's own pens are one path of the band
    dec.align_text([noisy(4100, 17, 5)], [[(0, "Hm")]], 0, 4100, 16, drift=2)
    assert launches(dec) == 2
    assert snapshot(dec) == before and timings() == tb


def test_memory_returns():
    """A decoder that only ever called align_text, with strips in LDS and in global memory, gives every device byte back."""
    before = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, AL)
        d.set_font_candidates([(SANS, 13.0, False, 1.0)])
        up = N.hip().focr_debug_device_bytes()
        d.align_text([noisy(257, 33, 41)], [[(0, "ahoi"), (12, "Hob in")]], 2, 250, LH, fonts=[[0, 1]], drift=9, step=2)
        small = N.hip().focr_debug_device_bytes()
        d.align_text([noisy(4100, 17, 42)], [[(0, "ahoi")]], 0, 4100, 16, drift=300, terms=False)
        assert launches(d) == 2
        peak = N.hip().focr_debug_device_bytes()
        assert before < up < small < peak
        assert d._lib.focr_decoder_n_lines(d._h) == 0  # no run was ever made
    assert N.hip().focr_debug_device_bytes() == before


def test_cli_rank_drift(dec, tmp_path):
    """focr --rank-text TEXT --rank-drift W [--rank-step N] prints rank_text_aligned's rows for a saved PGM, one per font."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(os.path.dirname(os.path.dirname(FOCR)), "csrc"), "cli"], check=True)
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([(MONO, 12.0, False, 1.0), (SANS, 13.0, False, 1.0)])
    text = "Hinein bin ihr"
    sans = fonts_of(dec)[2]
    page = np.full((2 * LH + 2, 150), 255, dtype=np.uint8)
    drawn = [int(np.rint(1.01 * m)) + 40 for m in nominal_pens(sans, text, 0)]  # Sans at 1.01 x its advances, 40/64 px right of -x
    for c, p in zip(text, drawn):
        g = np.zeros((LH, 148), dtype=np.uint8)
        raster_glyph(SANS, 13.0, c, np.float32(sans.origin[0] + np.float32(p) / np.float32(64)), sans.origin[1], g)
        page[LH: 2 * LH, 2:] = np.minimum(page[LH: 2 * LH, 2:], 255 - g)
    path = str(tmp_path / "page.pgm")
    save_pgm(path, page)
    cmd = [FOCR, "-f", MONO, "-t", "13", "-a", AL, "-x", "2", "-y", str(LH), "-w", "146", "--line-height", str(LH), "--line-advance", str(LH),
           "--font-candidate", "t=12", "--font-candidate", "f=%s" % SANS, "-i", path, str(tmp_path / "never-read.pgm"), "--rank-text", text]
    for drift, step in ((96, None), (96, 8), (0, 0)):
        base, cost, first, last, fits = dec.rank_text_aligned(page, LH, text, 2, 146, LH, drift=drift, **({} if step is None else dict(step=step)))
        r = subprocess.run(cmd + ["--rank-drift", str(drift)] + ([] if step is None else ["--rank-step", str(step)]), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        rows = ["font,first,last,cost,line_base,error,scale,x64"]
        for k in range(3):
            fit = ("", "") if fits[k][0] is None else ("%.6f" % fits[k][0], "%.2f" % fits[k][1])
            rows.append(f"{k},{first[k]},{last[k]},{cost[k]},{base},{base + int(cost[k])},{fit[0]},{fit[1]}")
        assert r.stdout.splitlines() == rows
    base, cost, first, last, fits = dec.rank_text_aligned(page, LH, text, 2, 146, LH, drift=96, step=8)
    assert int(np.argmin(cost)) == 2 and abs(fits[2][0] - 1.01) < 2e-3 and abs(fits[2][1] - 40) < 1.5  # Sans, its kerning and its x
    for extra, words in ((["--rank-drift", "8", "--rank-shift", "2"], "--rank-shift"), (["--rank-drift", "1025"], "1024"), (["--rank-step", "2"], "--rank-drift")):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and words in r.stderr and r.stdout == ""
    r = subprocess.run(cmd[:-2] + ["--rank-drift", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--rank-text" in r.stderr


# ---- the seeded pages and readings -----------------------------------------------------------------------------------------------

SEED = 0xA116


def seeded():
    """(case, page, W, N, start) over every page of every case of tests/focr_fuzz_cases.py, shuffled."""
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(FC.N_CASES):
        for page in range(len(FC.case(i).pages)):
            out.append((i, page, int(rng.integers(0, 7)), int(rng.choice([0, 1, 2, 64])), int(rng.choice([0, 3, 64, 500]))))
    rng.shuffle(out)
    return out


def test_seeded_pages_and_readings(dec):
    """The pages and fonts of tests/focr_fuzz_cases.py under the readings of tests/focr_text_fuzz.py (their lines, ys and shared
    characters; the placement is the alignment's own), each at a seeded (W, N) and start, shuffled over one handle."""
    n_lines = 0
    for i, page, drift, step, start in seeded():
        s = TF.setup("cases", i)
        r = TF.random_reading("cases", i, page)
        font = s.fonts[0]
        dec.set_font(font, s.case.size)
        dec.set_font_candidates([])
        x, _, width, lh, _ = s.geo
        batch = np.ascontiguousarray(np.asarray(s.pages[page])[None])
        recs = [(0, y, first, n, 0) for y, first, n, _, _ in r.recs]
        rc, got, pens, terms = raw(dec, batch, x, width, lh, recs, r.chars, start=start, drift=drift, step=step)
        assert rc == 0, dec._lib.focr_decoder_last_error(dec._h)
        at = 0
        for (_, y, first, n, _), g in zip(recs, got):
            want = want_line(font, s.pages[page], x, y, width, lh, r.chars[first: first + n], start, drift, step)
            assert g == (want.base, want.cost, want.first, want.last), (s.name, page, y, g, want[:4])
            assert np.array_equal(pens[at: at + n], want.pens) and np.array_equal(terms[at: at + n], want.terms), (s.name, page, y)
            at += n
            n_lines += 1
    assert n_lines > FC.N_CASES

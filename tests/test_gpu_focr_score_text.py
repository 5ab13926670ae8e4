"""focr_decoder_score_text (score_text_kernel, score_strip_kernel, LineDecoder.score_text / rank_text, focr --rank-text): the
decoder's cost of a caller's lines, each in any uploaded font.  First every mode of the decoder fed back its own outputs: the
cost the mode returned is the cost score_text gives its reading, and the run's getters and verify answer afterwards as before.
Then tests/focr_score_text_model.py, one FreeType raster per glyph, at the shapes where the kernel branches; every refusal;
rank_text against the CLI; device memory.  Every comparison is ==.  Pages are at most 330 px wide but for the two whose
strips must miss or just fit LDS."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_baseline_model as B
import focr_score_text_model as S
from font_ocr_amd import LineDecoder, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO, SANS, SERIF = (os.path.join(GOLD, f) for f in ("DejaVuSansMono.ttf", "DejaVuSans.ttf", "DejaVuSerif.ttf"))
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
AL = "abehinor HIm"
LH = 18
# fifteen candidates of the K = 15 case: (font, size, hinting, kerning)
FILL = [(MONO, 12.0, False, 1.0), (MONO, 14.0, False, 1.0), (MONO, 13.0, True, 1.0), (MONO, 13.0, False, 1.05), (SANS, 13.0, False, 1.0),
        (SERIF, 13.0, False, 1.0), (MONO, 12.5, False, 1.0), (MONO, 11.0, False, 1.0), (MONO, 11.5, False, 1.0), (MONO, 13.5, False, 1.0),
        (MONO, 12.0, True, 1.0), (MONO, 13.0, False, 0.95), (SANS, 12.0, False, 1.0), (SERIF, 12.0, True, 1.0), (SANS, 20.0, False, 1.0)]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def noisy(W, H, seed):
    """A page without structure: every clipped pixel and every misplaced glyph moves a term."""
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)


def launches(dec):
    return dec._lib.focr_decoder_last_score_text_launches(dec._h)


def fonts_of(dec):
    """The DecodeFonts 0 ..= K of the decoder: what the model reads its numbers from."""
    return [dec.font] + list(dec._candidates)


def check(dec, pages, lines, x, width, lh, fonts=None, pens=None, offsets=None, baselines=None, y_bits=0, shift=0, n_launches=1):
    """score_text equals the model line by line: base, cost, shift and every term."""
    got = dec.score_text(pages, lines, x, width, lh, fonts=fonts, pens=pens, offsets=offsets, baselines=baselines, y_bits=y_bits, shift=shift)
    assert launches(dec) == (n_launches if any(lines) else 0)
    for p, page in enumerate(pages):
        assert len(got[p]) == len(lines[p])
        for q, (y, text) in enumerate(lines[p]):
            want = S.score_text(fonts_of(dec)[fonts[p][q] if fonts is not None else 0], np.asarray(page), x, y, width, lh, text,
                                None if pens is None else pens[p][q], None if offsets is None else offsets[p][q],
                                0 if baselines is None else baselines[p][q], y_bits, shift)
            g = got[p][q]
            assert (g.base, g.cost, g.shift) == (want.base, want.cost, want.shift), (p, q, g[:3], want[:3])
            assert g.terms.dtype == np.int32 and np.array_equal(g.terms, want.terms), (p, q)
    return got


# ---- every mode fed back its own outputs ----------------------------------------------------------------------------------

def snapshot(dec):
    """What the last run's getters, timings and verify answer."""
    lib, h = dec._lib, dec._h
    nl, nc = lib.focr_decoder_n_lines(h), lib.focr_decoder_n_chars(h)
    lines = (N.DecodedLine * max(1, nl))()
    chars, offs, pens = np.zeros(max(1, nc), dtype=np.uint16), np.zeros(max(1, nc), dtype=np.int8), np.zeros(max(1, nc), dtype=np.uint32)
    cost, q, qcost = np.zeros(max(1, nl), dtype=np.int64), np.zeros(max(1, nl), dtype=np.int8), np.zeros(max(1, nl), dtype=np.int64)
    font, fcost, base = np.zeros(max(1, nl), dtype=np.uint8), np.zeros(max(1, nl), dtype=np.int64), np.zeros(max(1, nl), dtype=np.uint64)
    scores, margins = (N.CharScore * max(1, nc))(), np.zeros(max(1, nc) * 16, dtype=np.uint8)  # focr_char_margin_t: 16 bytes
    assert lib.focr_decoder_get(h, lines, chars.ctypes.data) == 0 and lib.focr_decoder_get_offsets(h, offs.ctypes.data) == 0
    rcs = (lib.focr_decoder_get_pens(h, pens.ctypes.data, cost.ctypes.data), lib.focr_decoder_get_scores(h, scores, base.ctypes.data),
           lib.focr_decoder_get_margins(h, margins.ctypes.data), lib.focr_decoder_get_baselines(h, q.ctypes.data, qcost.ctypes.data),
           lib.focr_decoder_get_fonts(h, font.ctypes.data, fcost.ctypes.data))
    try:
        sums, imgs = dec.verify()
        drawn = (sums.tobytes(), imgs.tobytes(), lib.focr_decoder_last_verify_launches(h))
    except DecoderError as e:  # after a font search
        drawn = str(e)
    return (nl, nc, bytes(lines), chars.tobytes(), offs.tobytes(), rcs, pens.tobytes(), cost.tobytes(), bytes(scores), base.tobytes(), margins.tobytes(),
            q.tobytes(), qcost.tobytes(), font.tobytes(), fcost.tobytes(), lib.focr_decoder_last_launches(h), lib.focr_decoder_last_ms(h), drawn)


def _pages(font, size, texts, offset=0.0, x=2, W=150, step=LH):
    """Two pages of lines in `font`, each line drawn `offset` px below its slot; ink left of every crop as well."""
    pages = []
    for pl in texts:
        page = np.full((2 * LH + 2, W), 255, dtype=np.uint8)
        for i, t in enumerate(pl):
            if t:
                B.draw_offset(page, font, size, AL, t, x, i * step, offset)
        page[::3, 0] = 90
        pages.append(page)
    return pages


TEXTS = [["Hinein bin ihr", "mohr ahoi ab"], ["", "bahn in rom"]]
MODES = ["scores", "search_scores", "whole", "margins", "slack", "baseline", "whole_baseline", "baseline_frac", "whole_baseline_frac", "fonts", "whole_fonts"]


@pytest.mark.parametrize("mode", MODES)
def test_a_run_fed_back_costs_what_it_returned(dec, mode):
    """One small batch per mode, the mode's own outputs fed back: the terms, the line_base and the costs are the run's, and the
    run's getters, timings and verify answer afterwards as they did before."""
    x, W = 2, 150
    width = W - 4
    frac = dict(y_frac=20, line_advance_frac=38) if mode.endswith("_frac") else {}
    font = MONO if mode in ("scores", "search_scores", "baseline", "baseline_frac", "fonts") else SANS
    y_bits = 2 if "baseline" in mode else 0
    dec.set_font(font, 13.0, AL, y_bits=y_bits)
    dec.set_font_candidates([(MONO, 12.0, False, 1.0), (SANS, 13.0, False, 1.0), (MONO, 13.0, False, 1.0)] if "fonts" in mode else [])
    pages = _pages(font, 13.0, TEXTS, offset=0.5 if "baseline" in mode else 0.0)
    if "fonts" in mode:  # the second page in another candidate's font
        pages[1] = _pages(MONO, 12.0 if mode == "fonts" else 13.0, TEXTS)[1]  # Mono 12 (candidate 1) or Mono 13 (candidate 3)
    geo = (pages, x, 0, width, LH, LH)
    kw = {}
    if mode == "scores":
        lines, scores = dec.decode(*geo, scores=True)
    elif mode == "search_scores":
        lines, scores, offsets = dec.decode(*geo, scores=True, pen_search=4)
        kw = dict(offsets=offsets)
    elif mode == "whole":
        lines, pens, costs = dec.decode(*geo, whole_line=True)
        kw = dict(pens=pens)
    elif mode == "margins":
        lines, pens, costs, margins = dec.decode(*geo, whole_line=True, margins=True)
        kw = dict(pens=pens)
    elif mode == "slack":
        lines, pens, costs, offs = dec.decode(*geo, whole_line=True, pen_slack=4)
        kw = dict(pens=pens)  # the render pens
    elif mode.startswith("baseline"):
        lines, qs, costs = dec.decode(*geo, baseline_search=3, **frac)
        kw = dict(baselines=qs, y_bits=2)
    elif mode.startswith("whole_baseline"):
        lines, pens, costs, qs = dec.decode(*geo, whole_line=True, whole_baseline=2, **frac)
        kw = dict(pens=pens, baselines=qs, y_bits=2)
    elif mode == "fonts":
        lines, fonts, costs = dec.decode(*geo, font_search=True)
        kw = dict(fonts=fonts)
    else:
        lines, pens, costs, fonts = dec.decode(*geo, whole_line=True, font_search=True)
        kw = dict(pens=pens, fonts=fonts)
    assert [len(pg) for pg in lines] == [2, 1]
    if "fonts" in mode:
        assert fonts == [[0, 0], [1 if mode == "fonts" else 3]]
    if "baseline" in mode:
        assert all(q != 0 for pg in qs for q in pg)  # the lines sit half a pixel low: a fractional phase or a moved row
    before = snapshot(dec)
    got = dec.score_text(pages, lines, x, width, LH, **kw)
    assert launches(dec) == 1
    for p in range(2):
        for q in range(len(lines[p])):
            g = got[p][q]
            assert g.shift == 0 and g.cost == int(g.terms.sum()) and len(g.terms) == len(lines[p][q][1])
            if "scores" in mode:
                sc = scores[p][q]
                assert g.base == sc.base and np.array_equal(g.terms, sc.score - sc.base)
            else:
                assert g.cost == costs[p][q], (p, q)
            if mode == "margins":
                assert np.array_equal(g.terms, margins[p][q].term)
    assert snapshot(dec) == before


# ---- against the model, where the kernel branches ---------------------------------------------------------------------------

def test_lane_stripes(dec):
    """Lines of 1, 64, 65 and 130 characters: one lane, a full batch, a batch and a character, three batches (the winner's terms
    come from three different waves).  The longest runs past the crop: its last glyphs lie wholly outside and cost 0."""
    dec.set_font(MONO, 8.0, AL)
    dec.set_font_candidates([])
    rng = np.random.default_rng(5)
    texts = ["".join(rng.choice(list(AL), n)) for n in (1, 64, 65, 130)]
    pages = [noisy(330, 30, 51)]
    lines = [[(0, texts[0]), (3, texts[1]), (9, texts[2]), (14, texts[3])]]
    for shift in (0, 1):
        got = check(dec, pages, lines, 3, 320, 12, shift=shift)
    assert not got[0][3].terms[-40:].any() and got[0][3].terms[:60].any()


@pytest.mark.parametrize("shift", [0, 1, 2, 64])
def test_shift_radius(dec, shift):
    """One candidate, three (fewer than waves), five, and 129; the pen loop's placement and the pen search's; on noise, where
    every shift costs something else."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([(SANS, 13.0, False, 1.0)])
    pages = [noisy(120, 40, 61), noisy(120, 40, 62)]
    lines = [[(1, "Hinein"), (20, "ab Hm")], [(7, "mohr in")]]
    got = check(dec, pages, lines, 5, 100, LH, fonts=[[0, 1], [1]], shift=shift)
    check(dec, pages, lines, 5, 100, LH, fonts=[[1, 0], [0]], offsets=[[[3, 0, -2, 0, 0, 5], [-4, 0, 0, 1, 0]], [[0, 0, 64, -64, 0, 0, 9]]], shift=shift)
    if shift == 64:
        assert {abs(g.shift) for pg in got for g in pg} - {0}  # some line is better off moved


def test_ties_negative_deltas_and_clipping(dec):
    """Spaces cost 0 at every shift: the rank decides and the shift is 0.  A line drawn a pixel left of its pen is found at
    j = -64, where its first glyph's delta is negative, and costs -line_base.  Glyphs clipped on each of the four sides of a
    crop that is narrower and lower than the text."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    f = dec.font
    blank = np.full((LH, 80), 255, dtype=np.uint8)
    got = check(dec, [blank], [[(0, "   "), (0, "")]], 0, 80, LH, shift=2)
    assert [(g.base, g.cost, g.shift) for g in got[0]] == [(0, 0, 0), (0, 0, 0)]
    assert float(f.origin[0]) == 0 and S.deltas(f, [AL.index("H")], j=-64) == [-64]
    page = S.draw_text(f, "Hinein", 80, LH, shift64=-64)  # the first glyph's delta is -64: its left column is off the crop
    got = check(dec, [page], [[(0, "Hinein")]], 0, 80, LH, shift=64)
    assert got[0][0].shift == -64 and got[0][0].cost == -got[0][0].base < 0
    got = check(dec, [page], [[(0, "Hinein")]], 0, 80, LH, pens=[[S.deltas(f, [AL.index(c) for c in "Hinein"])]], shift=64)
    assert got[0][0].shift == -64 and got[0][0].cost == -got[0][0].base
    noise = [noisy(90, 40, 71)]
    # a 30 x 6 crop inside the text: the top and bottom rows of every glyph, the left of the first and the right of the last are cut
    check(dec, noise, [[(12, "HImHIm")]], 20, 30, 6, offsets=[[[-40, 0, 0, 0, 0, 0]]], shift=2)
    check(dec, noise, [[(12, "HImHIm")]], 20, 30, 6, pens=[[[0, 480, 960, 1440, 1700, 1900]]], shift=1)


def test_vertical_candidates(dec):
    """q with rows moved up and down, whole (B = 0) and fractional (B = 2), per line; a candidate font at a whole q."""
    dec.set_font(MONO, 13.0, AL, y_bits=2)
    dec.set_font_candidates([(SANS, 13.0, False, 1.0)])
    pages = [noisy(120, 44, 81)]
    lines = [[(2, "Hinein"), (2, "Hinein"), (22, "ab Hm"), (22, "mohr")]]
    check(dec, pages, lines, 4, 100, LH, fonts=[[0, 1, 0, 1]], baselines=[[-2, 3, 0, -1]], y_bits=0, shift=1)
    check(dec, pages, lines, 4, 100, LH, fonts=[[0, 1, 0, 1]], baselines=[[-5, 8, 7, -4]], y_bits=2, shift=1)
    check(dec, pages, lines, 4, 100, LH, baselines=[[-9, 1, 2, 3]], y_bits=2, pens=[[[0, 500, 1000, 1499, 1998, 2497]] * 2 + [[5, 505, 1005, 1505, 2005], [0, 499, 998, 1497]]])
    # a q that moves every row out of the crop: every term 0
    got = check(dec, pages, [[(2, "Hinein")]], 4, 100, LH, baselines=[[-128]], y_bits=0)
    assert got[0][0].cost == 0 and got[0][0].base > 0


def test_crops_at_the_page_edges(dec):
    """A crop cut by the page's right and bottom edges; empty crops (y >= page_h, x_start >= page_w): base 0, terms 0."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    pages = [noisy(70, 30, 91)]
    got = check(dec, pages, [[(20, "Hinein bin"), (29, "ab"), (30, "Hm"), (1000, "Hm")]], 30, 100, LH, shift=1)
    assert [g.base > 0 for g in got[0]] == [True, True, False, False] and not got[0][2].terms.any()
    for x in (70, 71, 5000):
        got = check(dec, pages, [[(2, "Hinein")]], x, 100, LH, shift=2)
        assert (got[0][0].base, got[0][0].cost, got[0][0].shift) == (0, 0, 0)


@pytest.mark.parametrize("width,n_launches", [(4076, 1), (4077, 2), (4100, 2)])
def test_strip_in_lds_and_in_global_memory(dec, width, n_launches):
    """A 4100 x 17 page: 16 rows of 4076 columns just fit LDS beside the waves' sums, one column more does not, and the strips
    are then built in global memory by a launch of their own.  Glyphs at both ends and in the middle, by their pens."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    assert float(dec.font.origin[0]) == int(dec.font.origin[0])
    pages = [noisy(4100, 17, 101)]
    pens = [[[0, 64 * 2000 + 7, 64 * (width - 6), 64 * (width - 3) + 30, 64 * 4099]] * 2]
    check(dec, pages, [[(0, "HmHmH"), (1, "abeHI")]], 0, width, 16, pens=pens, shift=1, n_launches=n_launches)
    check(dec, pages, [[(1, "Hinein bin ihr")]], 0, width, 16, shift=0, n_launches=n_launches)


def test_sixteen_fonts_one_line(dec):
    """K = 15: the same line listed sixteen times, once per font (rank_text), against the model font by font."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates(FILL)
    fonts = fonts_of(dec)
    page = S.draw_text(fonts[6], "Hinein bin ihr", 150, LH, shift64=5)  # Serif 13, a little to the right
    base, cost, shift = dec.rank_text(page, 0, "Hinein bin ihr", 0, 146, LH, shift=8)
    assert launches(dec) == 1 and cost.dtype == np.int64 and len(cost) == len(shift) == 16
    want = [S.score_text(f, page, 0, 0, 146, LH, "Hinein bin ihr", radius=8) for f in fonts]
    assert base == want[0].base and list(cost) == [w.cost for w in want] and list(shift) == [w.shift for w in want]
    assert int(np.argmin(cost)) == 6 and shift[6] == 5


def raw(dec, batch, x, width, lh, recs, chars, pens=None, offsets=None, qs=None, y_bits=0, radius=0, on_device=0, pages_ptr=None):
    """focr_decoder_score_text as it is: recs are (page, y, first, n_chars, font).  Returns (rc, scores, terms)."""
    n, H, W = batch.shape
    larr = (N.TextLine * max(1, len(recs)))(*recs)
    carr = np.asarray(chars, dtype=np.uint16) if len(chars) else np.zeros(1, dtype=np.uint16)
    parr = None if pens is None else np.asarray(pens, dtype=np.uint32)
    oarr = None if offsets is None else np.asarray(offsets, dtype=np.int8)
    qarr = None if qs is None else np.asarray(qs, dtype=np.int8)
    terms = np.full(max(1, sum(r[3] for r in recs if r[3] < 1 << 20)), 7, dtype=np.int32)
    out = (N.TextScoreStruct * max(1, len(recs)))()
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = dec._lib.focr_decoder_score_text(dec._h, ptr(batch) if pages_ptr is None else pages_ptr, on_device, n, W, H, x, width, lh, larr, len(recs),
                                          ptr(carr), ptr(parr), ptr(oarr), len(chars), ptr(qarr), y_bits, radius, ptr(terms), out)
    return rc, [(s.line_base, s.cost, s.shift) for s in out][: len(recs)], terms


def test_any_page_order_shared_characters_and_device_pages(dec):
    """Lines in descending page order that share their characters, a line listed twice, a page without a line; and the same
    call with the pages in device memory."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([(SANS, 13.0, False, 1.0)])
    batch = np.ascontiguousarray(np.stack([noisy(100, 40, s) for s in (111, 112, 113)]))
    chars = [AL.index(c) for c in "Hinein im ohr"]
    recs = [(2, 20, 0, len(chars), 0), (2, 3, 0, len(chars), 1), (0, 3, 3, 5, 0), (0, 3, 3, 5, 0), (2, 20, 7, 0, 1)]
    rc, got, terms = raw(dec, batch, 4, 90, LH, recs, chars, radius=3)
    assert rc == 0 and launches(dec) == 1
    at = 0
    for (page, y, first, n, font), g in zip(recs, got):
        text = "".join(AL[c] for c in chars[first: first + n])
        want = S.score_text(fonts_of(dec)[font], batch[page], 4, y, 90, LH, text, radius=3)
        assert g == (want.base, want.cost, want.shift) and np.array_equal(terms[at: at + n], want.terms)
        at += n
    assert got[2] == got[3] and at == len(terms)
    hip = C.CDLL("libamdhip64.so.7")
    src = C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(batch.nbytes)) == 0
    try:
        assert hip.hipMemcpy(src, C.c_void_p(batch.ctypes.data), C.c_size_t(batch.nbytes), 1) == 0  # host to device
        assert hip.hipDeviceSynchronize() == 0
        rc, there, terms2 = raw(dec, batch, 4, 90, LH, recs, chars, radius=3, on_device=1, pages_ptr=src)
        assert rc == 0 and there == got and np.array_equal(terms2, terms)
    finally:
        hip.hipFree(src)
    # terms == NULL: the scores alone
    out = (N.TextScoreStruct * len(recs))()
    carr = np.asarray(chars, dtype=np.uint16)
    assert dec._lib.focr_decoder_score_text(dec._h, batch.ctypes.data, 0, 3, 100, 40, 4, 90, LH, (N.TextLine * len(recs))(*recs), len(recs), carr.ctypes.data,
                                            None, None, len(chars), None, 0, 3, None, out) == 0
    assert [(s.line_base, s.cost, s.shift) for s in out] == got


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals(dec):
    """Every refusal of include/focr_decode.h, each with its own words and nothing launched; the decoder scores afterwards."""
    lib, h = dec._lib, dec._h
    batch = np.ascontiguousarray(np.stack([noisy(80, 20, 31), noisy(80, 20, 32)]))
    with LineDecoder(0) as bare:  # no decode font
        rc, _, _ = raw(bare, batch, 0, 80, LH, [], [])
        assert rc != 0 and b"focr_decoder_score_text: no decode font (focr_decoder_set_font)" in bare._lib.focr_decoder_last_error(bare._h)
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
        rc, got, terms = raw(dec, batch, **args)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and msg.startswith("focr_decoder_score_text: ") and all(w in msg for w in words), msg
        assert launches(dec) == 0 and lib.focr_decoder_last_score_text_ms(h) == 0.0 and (terms == 7).all() and msg not in seen
        seen.add(msg)

    refused("pens and offsets", pens=[0, 500, 1000, 1500], offsets=[0, 0, 0, 0])
    refused("width 0", width=0)
    refused("line_height 0", lh=0)
    refused("shift radius", "64", radius=65)
    refused("y_bits", "3", y_bits=4)
    refused("line 1", "font 2", "1 candidates", recs=[good[0], (1, 2, 0, 4, 2)])
    refused("line 1", "page 2 of 2", recs=[good[0], (2, 2, 0, 4, 0)])
    refused("line 0", "n_chars", recs=[(0, 2, 1, 4, 0)])
    refused("character 2", "alphabet", chars=[0, 1, len(AL), 2])
    refused("pen 3", "2^24", pens=[0, 500, 1000, 1 << 24])
    refused("line_q", "y_bits > 0", "focr_decoder_set_baseline_fonts", qs=[1, 0], y_bits=3)  # the y-phase fonts are of y_bits 2
    refused("line 1", "fractional-phase q", "one vertical phase", qs=[1, 2], y_bits=2)
    assert raw(dec, batch, 1, 70, LH, good, chars, qs=[1, 4], y_bits=2)[0] == 0  # a whole q in a candidate font is fine
    # origins: built fonts have whole ones, so bend a copy of the candidate's struct
    cand = dec._candidates[0]
    keep = (cand.s.origin_x, cand.s.origin_y)
    for ox, oy, words, kw in ((0.5, keep[1], ("line 1", "pens", "origin_x", "whole number"), dict(pens=[0, 500, 1000, 1500])),
                              (-1.0, keep[1], ("line 1", "pens", "origin_x", "whole number"), dict(pens=[0, 500, 1000, 1500])),
                              (keep[0], 9.5, ("line 1", "line_q", "origin_y", "whole number"), dict(qs=[0, 0]))):
        cand.s.origin_x, cand.s.origin_y = ox, oy
        assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
        rc, _, terms = raw(dec, batch, 1, 70, LH, good, chars, **kw)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and all(w in msg for w in words) and launches(dec) == 0 and (terms == 7).all(), msg
        assert raw(dec, batch, 1, 70, LH, good[:1], chars, **kw)[0] == 0  # font 0 alone is not touched by it
    cand.s.origin_x, cand.s.origin_y = keep
    assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
    larr, carr, out = (N.TextLine * 2)(*good), np.asarray(chars, dtype=np.uint16), (N.TextScoreStruct * 2)()
    f = lib.focr_decoder_score_text
    for words, call in (("null pages", lambda: f(h, None, 0, 2, 80, 20, 1, 70, LH, larr, 2, carr.ctypes.data, None, None, 4, None, 0, 0, None, out)),
                        ("null lines", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, None, 2, carr.ctypes.data, None, None, 4, None, 0, 0, None, out)),
                        ("null chars", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, larr, 2, None, None, None, 4, None, 0, 0, None, out)),
                        ("null out", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, larr, 2, carr.ctypes.data, None, None, 4, None, 0, 0, None, None)),
                        ("page too large", lambda: f(h, batch.ctypes.data, 0, 2, 0xffff * 16 + 1, 20, 1, 70, LH, larr, 0, carr.ctypes.data, None, None, 4, None, 0, 0, None, out))):
        assert raw(dec, batch, 1, 70, LH, good, chars)[0] == 0 and launches(dec) == 1
        assert call() != 0
        msg = lib.focr_decoder_last_error(h).decode()
        assert msg.startswith("focr_decoder_score_text: ") and words in msg and launches(dec) == 0 and msg not in seen
        seen.add(msg)
    # no y-phase fonts at all
    dec.set_font(MONO, 13.0, AL)
    rc, _, _ = raw(dec, batch, 1, 70, LH, good[:1], chars, qs=[1], y_bits=1)
    assert rc != 0 and b"focr_decoder_set_baseline_fonts" in lib.focr_decoder_last_error(h) and launches(dec) == 0
    # usable afterwards; the launch count does not depend on the lines, the placement or the radius
    for kw in (dict(), dict(shift=64), dict(offsets=[[[0, 1, 2, 3]], [[0, 0, 0, 0]]]), dict(pens=[[[0, 500, 1000, 1500]], [[0, 500, 1000, 1500]]], shift=3),
               dict(baselines=[[2], [-2]])):
        check(dec, list(batch), [[(2, "ahoi")], [(2, "ahoi")]], 1, 70, LH, **kw)
    with pytest.raises(ValueError, match="not in the alphabet"):
        dec.score_text(list(batch), [[(2, "ahoy")], []], 1, 70, LH)


# ---- rank_text and the CLI -----------------------------------------------------------------------------------------------------

def test_cli_rank_text(dec, tmp_path):
    """focr --rank-text prints rank_text's rows for a saved PGM: one per font, error = line_base + cost; it decodes nothing."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([(MONO, 12.0, False, 1.0), (SANS, 13.0, False, 1.0)])
    page = np.full((2 * LH + 2, 150), 255, dtype=np.uint8)
    page[LH: 2 * LH, 2:] = S.draw_text(fonts_of(dec)[2], "Hinein bin ihr", 148, LH, shift64=40)
    path = str(tmp_path / "page.pgm")
    save_pgm(path, page)
    cmd = [FOCR, "-f", MONO, "-t", "13", "-a", AL, "-x", "2", "-y", str(LH), "-w", "146", "--line-height", str(LH), "--line-advance", str(LH),
           "--font-candidate", "t=12", "--font-candidate", "f=%s" % SANS, "-i", path, str(tmp_path / "never-read.pgm")]
    for n in (0, 64):
        base, cost, shift = dec.rank_text(page, LH, "Hinein bin ihr", 2, 146, LH, shift=n)
        r = subprocess.run(cmd + ["--rank-text", "Hinein bin ihr"] + (["--rank-shift", str(n)] if n else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert r.stdout.splitlines() == ["font,shift,cost,line_base,error"] + [f"{k},{shift[k]},{cost[k]},{base},{base + int(cost[k])}" for k in range(3)]
    assert int(np.argmin(cost)) == 2 and shift[2] == 40 and cost[2] == -base < 0  # Sans, 40/64 px to the right of -x


# ---- memory ----------------------------------------------------------------------------------------------------------------

def test_memory_returns():
    """A decoder that only ever called score_text, with strips in LDS and in global memory, gives every device byte back."""
    before = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, AL)
        d.set_font_candidates([(SANS, 13.0, False, 1.0)])
        up = N.hip().focr_debug_device_bytes()
        d.score_text([noisy(257, 33, 41)], [[(0, "ahoi"), (12, "Hob in")]], 2, 250, LH, fonts=[[0, 1]], shift=2)
        small = N.hip().focr_debug_device_bytes()
        d.score_text([noisy(4100, 17, 42)], [[(0, "ahoi")]], 0, 4100, 16, pens=[[[0, 500, 1000, 1500]]], terms=False)
        assert launches(d) == 2
        peak = N.hip().focr_debug_device_bytes()
        assert before < up < small < peak
        assert d._lib.focr_decoder_n_lines(d._h) == 0  # no run was ever made
    assert N.hip().focr_debug_device_bytes() == before

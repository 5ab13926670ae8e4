"""The focr decoder's font search (line_fonts_kernel, line_whole_fonts_kernel, focr_decoder_set_font_candidates /
_set_font_search / _get_fonts, LineDecoder.decode(font_search=True), focr --font-candidate) against tests/focr_fonts_model.py,
the definition of include/focr_decode.h restated on the fast model.  Every quantity is an exact integer or an f32 computed by
stated operations, so every comparison is ==.  Each test asserts from its geometry, or from the model's answer, that it
reaches the case it names."""
import csv
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import focr_baseline_model as B
import focr_fonts_model as FM
import focr_whole_model as W
from focr_fast_model import FastModel, line_cap
from font_ocr_amd import DecodeFont, LineDecoder, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO, SANS, SERIF = (os.path.join(GOLD, f) for f in ("DejaVuSansMono.ttf", "DejaVuSans.ttf", "DejaVuSerif.ttf"))
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536   # decode_line.h: a strip of up to this many bytes is staged in LDS
FONTS_RED_BYTES = 64    # decode_fonts.hip: the waves' (cost, k) pairs share that LDS with the strip
AL = "abehinor HIm"     # 12 glyphs; the last is the widest of the proportional fonts
AL6 = "aeno H"
LH = 18                 # rows of a line slot

pytestmark = pytest.mark.gpu

# (font, size, hinting, kerning): sixteen fonts that differ in size, hinting, kerning or face
SIXTEEN = [(MONO, 13.0, False, 1.0), (MONO, 12.0, False, 1.0), (MONO, 14.0, False, 1.0), (MONO, 13.0, True, 1.0), (MONO, 13.0, False, 1.05),
           (SANS, 13.0, False, 1.0), (SERIF, 13.0, False, 1.0), (MONO, 12.5, False, 1.0), (MONO, 11.0, False, 1.0), (MONO, 11.5, False, 1.0),
           (MONO, 13.5, False, 1.0), (MONO, 12.0, True, 1.0), (MONO, 13.0, False, 0.95), (SANS, 12.0, False, 1.0), (SERIF, 12.0, True, 1.0),
           (MONO, 10.5, False, 1.0)]


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


@functools.lru_cache(maxsize=None)
def model(font, size, hinting=False, kerning=1.0, alphabet=AL):
    return FastModel(font, size, alphabet, hinting, kerning)


def models_of(specs, alphabet=AL):
    return [model(f, t, h, k, alphabet) for f, t, h, k in specs]


def strip_bytes(width, line_height):
    return ((width + 7) // 4 + 2) * 4 * line_height


def page_of(slots, W=150, alphabet=AL, n_chars=14, seed=0, x=2):
    """A page of LH-row slots: slots[s] is the (font, size, hinting, kerning) its random text is set in, or None for a blank one."""
    rng = np.random.default_rng(seed)
    ink = [c for c in alphabet if not c.isspace()]
    page = np.full((LH * len(slots) + 2, W), 255, dtype=np.uint8)
    for s, spec in enumerate(slots):
        if spec is not None:
            f, t, h, k = spec
            B.draw_offset(page, f, t, alphabet, "".join(rng.choice(ink, n_chars)), x, LH * s, 0.0, h, k)
    return page


def upload(dec, models):
    dec.set_font(models[0].font, models[0].font.text_size)
    dec.set_font_candidates([m.font for m in models[1:]])


def check_pen(dec, models, pages, geo, want=None):
    """Upload, decode with the search on: line order, texts, k and costs equal to the model's.  Returns the model's
    [[(y, Fonts)] per page]."""
    upload(dec, models)
    want = want or [FM.search_image(models, p, *geo) for p in pages]
    lines, fonts, costs = dec.decode(pages, *geo, font_search=True)
    assert lines == [[(y, r.text) for y, r in pg] for pg in want]
    assert fonts == [[r.k for _, r in pg] for pg in want]
    assert costs == [[r.cost for _, r in pg] for pg in want]
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    return want


def check_whole(dec, models, pages, geo):
    """As check_pen under the whole-line form: texts, pens, costs and k equal to the model's."""
    upload(dec, models)
    want = [FM.search_image(models, p, *geo, whole=True) for p in pages]
    lines, pens, costs, fonts = dec.decode(pages, *geo, whole_line=True, font_search=True)
    assert lines == [[(y, r.text) for y, r in pg] for pg in want]
    assert fonts == [[r.k for _, r in pg] for pg in want]
    assert costs == [[r.cost for _, r in pg] for pg in want]
    assert all(np.array_equal(a, r.pens) for got, pg in zip(pens, want) for a, (_, r) in zip(got, pg))
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    return want


def winners(want):
    return [[r.k for _, r in pg] for pg in want]


# ---- the pen-loop form -------------------------------------------------------------------------------------------------

def pen_case(K):
    specs = SIXTEEN[:K + 1]
    drawn = [specs[0], None, specs[K], specs[K // 2 + 1 if K > 1 else 0], specs[min(3, K)]]
    return models_of(specs), [page_of(drawn, seed=K)], (2, 0, 146, LH, LH)


@pytest.mark.parametrize("K", [1, 3, 4, 15])
def test_pen_loop_parity(dec, K):
    """K = 1 (two waves idle), 3 (one candidate per wave), 4 (wave 0 takes two) and 15 (four each): lines of four of the
    fonts between a blank slot, each Mono line won by its own font."""
    models, pages, geo = pen_case(K)
    want = check_pen(dec, models, pages, geo)
    ks = winners(want)[0]
    assert [y for y, _ in want[0]] == [0, 2 * LH, 3 * LH, 4 * LH]
    assert ks == [0, K, K // 2 + 1 if K > 1 else 0, min(3, K)] and all(r.cost == -r.base for _, r in want[0])


def tie_case(which):
    a, x, y, z, v = SIXTEEN[1], SIXTEEN[0], SIXTEEN[2], SIXTEEN[8], SIXTEEN[9]
    specs = {"decode font": [a, x, a], "two waves": [x, a, a, y], "one wave": [x, a, y, z, v, a]}[which]
    return models_of(specs), [page_of([a, x], seed=7)], (2, 0, 146, LH, LH)


@pytest.mark.parametrize("which,first", [("decode font", 0), ("two waves", 1), ("one wave", 1)])
def test_pen_loop_ties(dec, which, first):
    """An upload identical to the decode font: k = 0 wins.  Two identical uploads in different waves (k = 1 and 2), and two
    in the same wave (k = 1 and 5): the lower k wins."""
    models, pages, geo = tie_case(which)
    want = check_pen(dec, models, pages, geo)
    twin = max(k for k, m in enumerate(models) if m is models[first])
    assert twin > first and winners(want)[0][0] == first
    assert FM.pen_loop(models[twin], pages[0][:LH, 2:148])[1] == want[0][0][1].cost


def last_rows_case():
    specs = [SIXTEEN[0], SIXTEEN[1], (MONO, 14.0, False, 1.02)]
    return models_of(specs), [_m_line(specs[2])], (2, 0, 146, LH, LH)


def _m_line(spec):
    f, t, h, k = spec
    page = np.full((LH, 150), 255, dtype=np.uint8)
    B.draw_offset(page, f, t, AL, "mmHamnmobmeHmhim", 2, 0, 0.0, h, k)
    return page


def phases_of(m, idx):
    """The sub-pixel phase of every step of the model m's pen loop that chose the glyphs idx."""
    pos, out = np.float32(0), []
    for i in idx:
        out.append(int(np.float32(np.float32(m.ox + pos) * np.float32(64))) & 63)
        pos = np.float32(pos + m.incs[i])
    return out


def test_pen_loop_last_table_rows(dec):
    """The last candidate wins a line full of the alphabet's last and widest glyph, and one of its steps renders at phase 63:
    every glyph is scored there, so the last rows of the concatenated bitmap table are read, where the 16-byte reads stop."""
    models, pages, geo = last_rows_case()
    want = check_pen(dec, models, pages, geo)
    r = want[0][0][1]
    last = models[-1].font.s
    widths = [last.glyphs[i].box_w for i in range(last.n_glyphs)]
    assert r.k == len(models) - 1 and widths[-1] == max(widths) and r.text.rstrip(" ") == "mmHamnmobmeHmhim"
    assert 63 in phases_of(models[-1], r.idx)
    g = last.glyphs[last.n_glyphs - 1]
    assert g.offset + 64 * g.stride * g.box_h == last.bitmaps_len and g.stride // 4 < 4  # the table ends with it, in rows shorter than a read


AL_V = "abehinor HIv"   # Serif's v reaches left of the pen: origin_x 1


def origins_case():
    specs = [(MONO, 13.0, False, 1.0), (SERIF, 13.0, False, 1.0), (SANS, 13.0, False, 1.0), (SERIF, 12.0, True, 1.0)]
    return models_of(specs, AL_V), [page_of([specs[1], specs[0], specs[3], specs[2]], alphabet=AL_V, seed=11, n_chars=12)], (2, 0, 146, LH, LH)


def test_pen_loop_origins(dec):
    """Candidates with different origin_x: Serif's glyphs reach left of the pen, Mono's and Sans's do not."""
    models, pages, geo = origins_case()
    assert [float(m.ox) for m in models] == [0.0, 1.0, 0.0, 1.0]
    want = check_pen(dec, models, pages, geo)
    assert {1, 3} & set(winners(want)[0]) and winners(want)[0][1] == 0


def caps_case():
    specs = [(MONO, 27.0, False, 1.0), (MONO, 10.0, False, 1.0)]
    return models_of(specs), [page_of([specs[1], specs[0]], seed=12, n_chars=9)], (2, 0, 146, LH, LH)  # the tall font last


def test_pen_loop_caps(dec):
    """Very different smallest increments (16 px against 6 px), the decode font's the larger: the characters per line are the
    small candidate's, far more than the decode font's own bound."""
    models, pages, geo = caps_case()
    assert models[0].incs.min() > 16.0 and models[1].incs.min() < 6.1
    want = check_pen(dec, models, pages, geo)
    assert winners(want)[0][:2] == [1, 0]
    assert len(want[0][0][1].text) == line_cap(models[1].incs, 146) > 2 * line_cap(models[0].incs, 146)


def global_strip_case():
    specs = [(MONO, 13.0, False, 1.0), (MONO, 12.0, False, 1.0), (MONO, 13.0, True, 1.0)]
    page = np.full((17, 4002), 255, dtype=np.uint8)
    rng = np.random.default_rng(5)
    B.draw_offset(page, MONO, 12.0, AL6, "".join(rng.choice(list("aenoH"), 540)), 2, 0, 0.0)
    return models_of(specs, AL6), [page], (2, 0, 4000, 17, 17)


def test_pen_loop_strip_outside_lds(dec):
    """4000 columns by 17 rows with K = 2: the strip does not fit in LDS beside the waves' pairs and is read from global memory."""
    models, pages, geo = global_strip_case()
    assert strip_bytes(4000, 17) + FONTS_RED_BYTES > LDS_STRIP_MAX
    want = check_pen(dec, models, pages, geo)
    assert winners(want) == [[1]] and len(want[0][0][1].text) > 500


def pages_case():
    a, b, c = SIXTEEN[0], SIXTEEN[1], SIXTEEN[3]
    pages = [page_of([a, b, c, None, b], seed=21), np.full((LH * 5 + 2, 150), 255, dtype=np.uint8), page_of([c, None, a, a, b], seed=22)]
    return models_of([a, b, SIXTEEN[2], c]), pages, (2, 0, 146, LH, LH)


def test_pen_loop_pages_and_one_workgroup(dec):
    """Two pages with a blank one between them, lines of three fonts on each; then one workgroup takes all eight lines, and
    two take four each: the result is the one-line-per-workgroup run's."""
    models, pages, geo = pages_case()
    want = check_pen(dec, models, pages, geo)
    assert winners(want) == [[0, 1, 3, 1], [], [3, 0, 0, 1]]
    free = dec.decode(pages, *geo, font_search=True)
    try:
        for grid in (1, 2):
            assert dec._lib.focr_decoder_debug_set_fonts_grid(dec._h, grid) == 0
            assert dec.decode(pages, *geo, font_search=True) == free
    finally:
        assert dec._lib.focr_decoder_debug_set_fonts_grid(dec._h, 0) == 0


# ---- the whole-line form -----------------------------------------------------------------------------------------------

WHOLE5 = [(SANS, 13.0, False, 1.0), (SANS, 12.0, False, 1.0), (SANS, 13.0, True, 1.0), (SERIF, 13.0, False, 1.0), (MONO, 13.0, False, 1.0)]


def whole_case(K):
    specs = WHOLE5[:K + 1]
    drawn = [specs[0], specs[K], specs[1]] if K == 1 else [specs[0], specs[4], specs[1], specs[2], specs[3]]
    return models_of(specs, AL6), [page_of(drawn, W=84, alphabet=AL6, n_chars=8, seed=30 + K)], (2, 0, 80, LH, LH)


@pytest.mark.parametrize("K", [1, 4])
def test_whole_line_parity(dec, K):
    """K = 1 and K = 4 on proportional lines, each won by its own font: the best changes never (the first candidate wins, from
    half 0), once (the winner lies in half 1) and several times (half 0 again), and the last candidate wins as well."""
    models, pages, geo = whole_case(K)
    want = check_whole(dec, models, pages, geo)
    ks, trails = winners(want)[0], [len(r.trail) for _, r in want[0]]
    assert ks == ([0, 1, 1] if K == 1 else [0, 4, 1, 2, 3])
    assert {1, 2} <= set(trails) and (K == 1 or max(trails) >= 3)
    assert all(len(r.text) >= 8 for _, r in want[0])


def rings_case():
    specs = [(MONO, 8.0, False, 1.0), (MONO, 14.0, False, 1.0), (MONO, 11.0, False, 1.0)]
    return models_of(specs, AL6), [page_of([specs[1], specs[0], specs[2]], W=150, alphabet=AL6, n_chars=12, seed=41)], (2, 0, 146, LH, LH)


def test_whole_line_batches_and_rings(dec):
    """Candidates whose batches differ (min inc64 308, 539 and 424; the second is capped at 512) and whose largest inc64
    differ, so that the cost ring (2048 keys) is the second candidate's, not the decode font's (1024)."""
    models, pages, geo = rings_case()
    incs = [int(W.inc64(m.incs).min()) for m in models]
    assert incs[0] < 512 < incs[1] and len(set(incs)) == 3
    assert 2 * incs[0] <= 1024 < 512 + incs[1] <= 2048
    want = check_whole(dec, models, pages, geo)
    assert winners(want) == [[1, 0, 2]]


def test_whole_line_tie(dec):
    """An upload identical to the decode font, and a second copy behind another font: equal costs, and the first wins."""
    a, b = WHOLE5[0], WHOLE5[3]
    ms = models_of([a, b, a, a], AL6)
    page = page_of([a, b], W=84, alphabet=AL6, n_chars=8, seed=51)
    want = check_whole(dec, ms, [page], (2, 0, 80, LH, LH))
    assert winners(want) == [[0, 1]] and want[0][0][1].trail == [(0, want[0][0][1].cost)]
    ms = models_of([b, a, a], AL6)
    want = check_whole(dec, ms, [page], (2, 0, 80, LH, LH))
    assert winners(want) == [[1, 0]]


def whole_global_case():
    specs = [(MONO, 13.0, False, 1.0), (MONO, 40.0, False, 1.0), (MONO, 12.0, False, 1.0)]
    page = np.full((LH, 1760), 255, dtype=np.uint8)
    rng = np.random.default_rng(61)
    B.draw_offset(page, MONO, 12.0, AL6, "".join(rng.choice(list("aenoH"), 240)), 2, 0, 0.0)
    return models_of(specs, AL6), [page], (2, 0, 1750, LH, LH)


def test_whole_line_strip_outside_lds(dec):
    """A 40 px candidate makes the cost ring 4096 keys, and beside it the strip of 1750 columns by 18 rows does not fit in LDS."""
    models, pages, geo = whole_global_case()
    hi = int(W.inc64(models[1].incs).max())
    assert 2048 < 512 + hi <= 4096 and strip_bytes(1750, LH) + 1088 + 8 * 4096 > LDS_STRIP_MAX
    want = check_whole(dec, models, pages, geo)
    assert winners(want) == [[2]] and len(want[0][0][1].text) > 230


def test_whole_line_one_workgroup(dec):
    """One workgroup takes every line of two pages in turn: the scratch halves and the best so far start afresh per line."""
    models, pages, geo = whole_case(4)
    pages = pages + [pages[0][LH:].copy()]
    want = check_whole(dec, models, pages, geo)
    assert [len(pg) for pg in want] == [5, 4] and len({k for pg in winners(want) for k in pg}) == 5
    free = dec.decode(pages, *geo, whole_line=True, font_search=True)
    try:
        for grid in (1, 2):
            assert dec._lib.focr_decoder_debug_set_fonts_grid(dec._h, grid) == 0
            got = dec.decode(pages, *geo, whole_line=True, font_search=True)
            assert got[0] == free[0] and got[2:] == free[2:] and all(np.array_equal(a, b) for p, q in zip(got[1], free[1]) for a, b in zip(p, q))
    finally:
        assert dec._lib.focr_decoder_debug_set_fonts_grid(dec._h, 0) == 0


# ---- both forms --------------------------------------------------------------------------------------------------------

def _raw_run(dec, page, x, y, width, line_height, line_advance):
    page = np.ascontiguousarray(page)
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], x, y, width, line_height, line_advance)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def _get_fonts(d):
    n = d._lib.focr_decoder_n_lines(d._h)
    k, cost = np.full(max(n, 1), 99, dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int64)
    return d._lib.focr_decoder_get_fonts(d._h, k.ctypes.data, cost.ctypes.data), k[:n], cost[:n]


@pytest.mark.parametrize("whole", [False, True])
def test_search_off_is_the_run_of_before(dec, whole):
    """With candidates uploaded and the search off, before and after a run with it on, a run returns what a decoder that never
    heard of candidates returns, and focr_decoder_get_fonts fails; after a run with it on every other getter's refusal stands,
    and so does the verify's."""
    models, pages, geo = whole_case(1) if whole else pen_case(3)
    kw = dict(whole_line=True) if whole else {}
    with LineDecoder(0) as fresh:
        fresh.set_font(models[0].font, models[0].font.text_size)
        plain = fresh.decode(pages, *geo, verify="mse", **kw)
    upload(dec, models)
    lib, h = dec._lib, dec._h
    for again in (False, True):
        got = dec.decode(pages, *geo, verify="mse", **kw)
        assert got[0] == plain[0] and got[1].tobytes() == plain[1].tobytes() and lib.focr_decoder_last_launches(h) == 3
        if whole:
            assert got[4] == plain[4] and all(np.array_equal(a, b) for p, q in zip(got[3], plain[3]) for a, b in zip(p, q))
        rc, _, _ = _get_fonts(dec)
        assert rc != 0 and b"focr_decoder_set_font_search" in lib.focr_decoder_last_error(h)
        if again:
            break
        searched = dec.decode(pages, *geo, font_search=True, **kw)
        assert searched[0] != plain[0] and _get_fonts(dec)[0] == 0
        assert list(_get_fonts(dec)[1]) == [k for pg in searched[-1 if whole else 1] for k in pg]
        assert lib.focr_decoder_get_scores(h, None, None) != 0 and lib.focr_decoder_get_margins(h, None) != 0
        assert lib.focr_decoder_get_baselines(h, None, None) != 0 and (lib.focr_decoder_get_pens(h, None, None) == 0) == whole
        sums = np.zeros(len(pages), dtype=np.uint64)
        assert lib.focr_decoder_verify(h, None, 0, sums.ctypes.data) != 0
        msg = lib.focr_decoder_last_error(h)
        assert b"focr_decoder_verify" in msg and b"focr_decoder_set_font_search" in msg and b"later step" in msg
        with pytest.raises(DecoderError, match="searched fonts"):
            dec.verify()


def test_refusals(dec):
    """Every refusal of include/focr_decode.h, before anything is launched; the decoder decodes afterwards."""
    models, pages, geo = pen_case(1)
    page = pages[0]
    lib, h = dec._lib, dec._h
    want = check_pen(dec, models, pages, geo)

    def refused(*words):
        rc, msg = _raw_run(dec, page, *geo)
        assert rc != 0 and msg.startswith("focr_decoder_run: ") and all(w in msg for w in words), msg
        assert lib.focr_decoder_last_launches(h) == 0 and lib.focr_decoder_n_lines(h) == 0 and _get_fonts(dec)[0] != 0
        return msg

    assert lib.focr_decoder_set_font_search(h, 1) == 0
    for on, off, name in ((lambda: lib.focr_decoder_set_scores(h, 1), lambda: lib.focr_decoder_set_scores(h, 0), "focr_decoder_set_scores"),
                          (lambda: lib.focr_decoder_set_pen_search(h, 4), lambda: lib.focr_decoder_set_pen_search(h, 0), "focr_decoder_set_pen_search"),
                          (lambda: lib.focr_decoder_set_baseline_search(h, 0, 2), lambda: lib.focr_decoder_set_baseline_search(h, 0, 0), "focr_decoder_set_baseline_search")):
        assert on() == 0
        assert refused("focr_decoder_set_font_search", name).endswith(" yet")
        assert off() == 0
    assert lib.focr_decoder_set_whole_line(h, 1) == 0
    for on, off, name in ((lambda: lib.focr_decoder_set_whole_margins(h, 1), lambda: lib.focr_decoder_set_whole_margins(h, 0), "focr_decoder_set_whole_margins"),
                          (lambda: lib.focr_decoder_set_whole_slack(h, 4), lambda: lib.focr_decoder_set_whole_slack(h, 0), "focr_decoder_set_whole_slack"),
                          (lambda: lib.focr_decoder_set_whole_baseline(h, 0, 2), lambda: lib.focr_decoder_set_whole_baseline(h, 0, 0), "focr_decoder_set_whole_baseline")):
        assert on() == 0
        assert refused("focr_decoder_set_font_search", name).endswith(" yet")
        assert off() == 0
    # a candidate that fails a whole-line check of its own: an origin_x that is not a whole number, an advance too wide for the ring
    bent = DecodeFont(MONO, 12.0, AL)
    bent.s.origin_x = 0.5
    wide = DecodeFont(MONO, 120.0, AL)
    assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 2)(models[1].font.s, bent.s), 2) == 0
    refused("font candidate 2", "origin_x")
    assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(wide.s), 1) == 0
    refused("font candidate 1", "cost ring")
    assert lib.focr_decoder_set_whole_line(h, 0) == 0
    assert _raw_run(dec, page, *geo)[0] == 0 and _get_fonts(dec)[0] == 0  # the pen loop takes that candidate
    # no candidates: dropped by hand, by set_font and by a failed upload
    assert lib.focr_decoder_set_font_candidates(h, None, 0) == 0
    refused("focr_decoder_set_font_search", "focr_decoder_set_font_candidates")
    upload(dec, models)
    dec.set_font(models[0].font, 13.0)
    refused("focr_decoder_set_font_candidates")
    upload(dec, models)
    for other, n, words in ((DecodeFont(MONO, 12.0, AL[1:] + "a"), 1, b"code point"), (DecodeFont(MONO, 12.0, AL[:-1]), 1, b"glyph count"), (bent, 16, b"at most 15")):
        arr = (N.DecodeFontStruct * 16)(*([other.s] * 16))
        assert lib.focr_decoder_set_font_candidates(h, arr, n) != 0
        assert b"focr_decoder_set_font_candidates" in lib.focr_decoder_last_error(h) and words in lib.focr_decoder_last_error(h)
        refused("focr_decoder_set_font_candidates")  # a failed upload leaves none
        if other is not bent:
            other.close()
    stuck = DecodeFont(MONO, 12.0, AL)
    stuck.s.glyphs[2].increment = 0.0
    assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(stuck.s), 1) != 0 and b"advance" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_font_search(h, 0) == 0
    dec._font_search = False
    for f in (bent, wide, stuck):
        f.close()
    dec.set_font_candidates([])
    with pytest.raises(ValueError, match="needs candidates"):
        dec.decode(pages, *geo, font_search=True)
    assert check_pen(dec, models, pages, geo, want) is want


def test_cli(dec, tmp_path):
    """focr --font-candidate t=12 --font-candidate h=1 --fonts out.csv on one small page: stdout and the CSV are the model's."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    specs = [(MONO, 13.0, False, 1.0), (MONO, 12.0, False, 1.0), (MONO, 13.0, True, 1.0)]
    models = models_of(specs)
    page = page_of([specs[2], specs[0], None, specs[1]], seed=71)
    path, out = str(tmp_path / "page.pgm"), tmp_path / "fonts.csv"
    save_pgm(path, page)
    want = FM.search_image(models, page, 2, 0, 146, LH, LH)
    assert [r.k for _, r in want] == [2, 0, 1]
    cmd = [FOCR, "-f", MONO, "-t", "13", "-a", AL, "-x", "2", "-y", "0", "-w", "146", "--line-height", str(LH), "--line-advance", str(LH)]
    r = subprocess.run(cmd + ["--font-candidate", "t=12", "--font-candidate", "h=1", "--fonts", str(out), "-i", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join(w.text + "\n" for _, w in want)
    with open(out, newline="") as f:
        assert list(csv.reader(f)) == [["image_index", "y", "font", "cost"]] + [["0", str(y), str(w.k), str(w.cost)] for y, w in want]
    r = subprocess.run(cmd + ["-i", path], capture_output=True, text=True, timeout=300)  # without candidates: today's text
    assert r.returncode == 0 and r.stdout == "".join(models[0].decode_line(page[y: y + LH, 2:148]) + "\n" for y, _ in want)


def test_memory_returns():
    """A decoder that uploaded candidates and searched in both forms gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    models, pages, geo = whole_case(1)
    with LineDecoder(0) as d:
        d.set_font(models[0].font, 13.0)
        d.decode(pages, *geo)
        off = N.hip().focr_debug_device_bytes()
        d.set_font_candidates([m.font for m in models[1:]])
        up = N.hip().focr_debug_device_bytes()
        d.decode(pages, *geo, font_search=True)
        d.decode(pages, *geo, whole_line=True, font_search=True)
        searched = N.hip().focr_debug_device_bytes()
        assert before < off < up < searched
        d.set_font_candidates([])
        assert N.hip().focr_debug_device_bytes() < searched
    assert N.hip().focr_debug_device_bytes() == before

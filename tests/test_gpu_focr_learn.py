"""focr_decoder_learn_text (learn_text_kernel, learn_strip_kernel, LineDecoder.learn_text, DecodeFont.learned, focr --learn): the
page's inverted luma summed under every (glyph, phase) cell of a reading the caller trusts.  Device == tests/focr_learn_model.py
(the definition one character at a time, in numpy) by == on sums, counts and used, at the shapes where the kernel branches: the
three placements, font 0 and a candidate, a use mask, a box at and over each crop edge, clipped and empty crops, thousands of
adds to one cell, glyph boxes against the wave's 64 lanes and the workgroup's 256, the strip in LDS and in global memory, the
64-character batches of the walk; then the learned font on the device, every refusal, the last run's getters, device memory, the
CLI, and the seeded readings of tests/focr_text_fuzz.py.  Pages are small but for the two whose strips must just fit or miss LDS."""
import os
import subprocess

import numpy as np
import pytest

import focr_fuzz_cases as FC
import focr_learn_model as L
import focr_score_text_model as S
import focr_text_fuzz as TF
from focr_fast_model import ALPHABET_319, FastModel, crop
from font_ocr_amd import DecodeFont, LearnedGlyphs, LineDecoder, save_pgm
from font_ocr_amd import _native as N
from test_gpu_focr_score_text import AL, FOCR, LH, MONO, SANS, fonts_of, noisy, snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def launches(dec):
    return dec._lib.focr_decoder_last_learn_text_launches(dec._h)


def raw(dec, batch, x, width, lh, recs, chars, pens=None, offsets=None, use=None, font=0, sums=True, counts=True, n_sums=None):
    """One focr_decoder_learn_text call as the library takes it: (rc, sums, counts, used), the outputs filled with 7 beforehand."""
    n, h, w = batch.shape
    larr = (N.TextLine * max(1, len(recs)))(*recs)
    carr = np.asarray(chars if len(chars) else [0], dtype=np.uint16)
    ptr = lambda a, t: None if a is None else np.asarray(a, dtype=t)  # noqa: E731
    parr, oarr, uarr = ptr(pens, np.uint32), ptr(offsets, np.int8), ptr(use, np.uint8)
    f = fonts_of(dec)[font] if font < len(fonts_of(dec)) else dec.font
    sarr = np.full(max(1, f.s.bitmaps_len if n_sums is None else n_sums), 7, dtype=np.uint32)
    karr = np.full(max(1, 64 * f.s.n_glyphs), 7, dtype=np.uint32)
    darr = np.full(max(1, sum(r[3] for r in recs)), 7, dtype=np.uint8)
    at = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = dec._lib.focr_decoder_learn_text(dec._h, batch.ctypes.data, 0, n, w, h, x, width, lh, larr, len(recs), carr.ctypes.data, at(parr), at(oarr), at(uarr),
                                          len(chars), font, sarr.ctypes.data if sums else None, karr.ctypes.data if counts else None, darr.ctypes.data)
    return rc, sarr, karr, darr


def same(got, want, where=None):
    """A LearnedGlyphs of the device against the model's Learned, by ==."""
    assert got.sums.dtype == np.uint64 and got.counts.dtype == np.uint64
    assert np.array_equal(got.counts, want.counts), where
    assert np.array_equal(got.sums, want.sums), where
    assert len(got.used) == len(want.used)
    for g, w in zip(got.used, want.used):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert a.dtype == np.uint8 and np.array_equal(a, b), where


def check(dec, pages, lines, x, width, lh, fonts=None, pens=None, offsets=None, use=None, font=0, n_launches=1):
    got = dec.learn_text(pages, lines, x, width, lh, fonts=fonts, pens=pens, offsets=offsets, use=use, font=font)
    assert launches(dec) == (n_launches if any(lines) else 0)
    want = L.learn_text(fonts_of(dec)[font], [np.asarray(p) for p in pages], lines, x, width, lh, fonts=fonts, pens=pens, offsets=offsets, use=use, k=font)
    same(got, want, (font, x, width, lh))
    return got


def pens_of(font, text, start, gap=0):
    """Whole-line pens: the font's own advances from `start`, every character a further `gap` / 64 px on."""
    inc = font.increments()
    out, s = [], start
    for c in text:
        out.append(s)
        s += int(np.rint(inc[font.alphabet.index(c)] * 64)) + gap
    return out


# ---- placements and fonts ---------------------------------------------------------------------------------------------------

PAGES = [noisy(120, 40, 61), noisy(120, 40, 62)]
LINES = [[(2, "Hinein bin ihr"), (20, "mohr ahoi ab")], [(1, "bahn in rom"), (19, "Hi mob")]]


@pytest.mark.parametrize("placement", ["none", "offsets", "pens"])
@pytest.mark.parametrize("font", [0, 1])
def test_placements_and_fonts(dec, placement, font):
    """The pen loop's walk, the pen search's offsets and a whole-line run's pens, in the decode font and in a candidate of another
    box size; the lines of the other font are in the list and contribute nothing."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([(SANS, 11.0, False, 1.0)])
    fs = fonts_of(dec)
    assert {(g.box_w, g.box_h) for g in fs[0].s.glyphs[:len(AL)]} != {(g.box_w, g.box_h) for g in fs[1].s.glyphs[:len(AL)]}
    fonts = [[0, 1], [1, 0]]
    rng = np.random.default_rng(63)
    kw = {}
    if placement == "offsets":
        kw["offsets"] = [[[int(v) for v in rng.integers(-9, 10, len(t))] for _, t in pg] for pg in LINES]
    if placement == "pens":
        kw["pens"] = [[pens_of(fs[fonts[p][q]], t, 5 + 17 * q, gap=3) for q, (_, t) in enumerate(pg)] for p, pg in enumerate(LINES)]
    got = check(dec, PAGES, LINES, 3, 110, LH, fonts=fonts, font=font, **kw)
    assert got.counts.sum() > 10 and got.sums.sum() > 0
    for p in range(2):
        for q in range(2):
            assert got.used[p][q].any() == (fonts[p][q] == font)
    both = check(dec, PAGES, LINES, 3, 110, LH, fonts=[[font, font], [font, font]], font=font, **kw)
    assert both.counts.sum() > got.counts.sum()


def test_reverse_page_order_repeats_shared_characters_and_a_mask(dec):
    """Lines in reverse page order, one listed three times, two that share their characters (one a prefix of the other), and a
    use mask that drops every second entry of chars: the dropped characters still move the pen."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    batch = np.ascontiguousarray(np.stack(PAGES))
    chars = [AL.index(c) for c in "Hinein bin ihrmohr"]
    recs = [(1, 19, 0, 14, 0), (0, 2, 0, 14, 0), (1, 19, 0, 14, 0), (0, 20, 3, 6, 0), (1, 19, 0, 14, 0), (0, 2, 14, 4, 0), (1, 1, 0, 0, 0)]
    for use in (None, [i % 2 for i in range(len(chars))]):
        rc, sums, counts, used = raw(dec, batch, 3, 110, LH, recs, chars, use=use)
        assert rc == 0 and launches(dec) == 1
        acc, flags = L.empty(dec.font), []
        for page, y, first, n, _ in recs:
            flags.append(L.learn_crop(dec.font, acc, crop(PAGES[page], 3, y, 110, LH), chars[first: first + n], use=None if use is None else use[first: first + n]))
        assert np.array_equal(counts, acc.counts) and np.array_equal(sums, acc.sums) and np.array_equal(used, np.concatenate(flags))
        assert counts.sum() == used.sum() > (20 if use is None else 8)
    assert not used[0:14:2].any() and used[1:14:2].any()  # the first listed line: its even characters are masked out


# ---- box edges ----------------------------------------------------------------------------------------------------------------

def test_a_box_at_and_over_each_crop_edge(dec):
    """One character whose box touches the left, the right and the bottom edge of the crop is counted; one pixel over it is not.
    Left by an offset that makes the delta negative, right by `width`, bottom by `line_height`, top by a glyph whose off_y is 0
    (a box over the top edge cannot be listed: off_y is never negative and there is no line_q).  Then crops the page clips."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    f = dec.font
    page = noisy(60, 30, 64)
    top = [i for i in range(len(AL)) if f.phase(i, 0)[2] == 0 and f.phase(i, 0)[0].any()]
    assert top  # the tallest glyph starts at row 0 of the line
    i = top[0]
    text = AL[i]
    box = lambda **kw: L.boxes(f, [i], S.deltas(f, [i], **kw))[0]  # noqa: E731
    # left: the offset whose box starts at column 0 and, with a negative delta, the one at column -1
    at = {box(offsets=[o])[1]: o for o in range(127, -129, -1)}
    assert 0 in at and -1 in at and S.deltas(f, [i], offsets=[at[-1]])[0] < 0
    for x0, counted in ((0, 1), (-1, 0)):
        got = check(dec, [page], [[(2, text)]], 5, 50, LH, offsets=[[[at[x0]]]])
        assert got.counts.sum() == counted and got.used[0][0][0] == counted
    # right and bottom: the crop ends with the box, and one pixel before
    p, x0, y0, bw, bh = box()
    assert y0 == 0 and x0 >= 0
    for width, lh, counted in ((x0 + bw, LH, 1), (x0 + bw - 1, LH, 0), (50, bh, 1), (50, bh - 1, 0)):
        got = check(dec, [page], [[(2, text)]], 5, width, lh)
        assert got.counts.sum() == counted, (width, lh)
        assert got.counts[i * 64 + p] == counted
    # the page clips the crop: its last rows and columns still hold the box, or do not; an empty crop and a y past the page give zeros
    for x, y, counted in ((60 - x0 - bw, 30 - bh, 1), (60 - x0 - bw + 1, 30 - bh, 0), (60 - x0 - bw, 30 - bh + 1, 0)):
        got = check(dec, [page], [[(y, text)]], x, 50, LH)
        assert got.counts.sum() == counted and bool(got.sums.any()) == bool(counted), (x, y)
    for x, y in ((60, 2), (61, 2), (5, 30), (5, 4000)):  # a blank glyph's box has no pixels, and an empty crop does not hold it either
        got = check(dec, [page], [[(y, " " + text + " ")]], x, 50, LH)
        assert not got.counts.any() and not got.sums.any() and not got.used[0][0].any(), (x, y)
    assert check(dec, [page], [[(2, " ")]], 5, 50, LH).counts[AL.index(" ") * 64:][:64].sum() == 1  # ... which a crop with pixels does


# ---- many samples in one cell ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 5000])
def test_many_samples_in_one_cell(dec, n):
    """One one-character line listed n times: one cell takes every add, from n workgroups.  The kernel has no chunk or split per
    cell (its adds go straight to memory), so the two sizes stand for "some" and "more than any wave count of the device"."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    page = noisy(40, 20, 65)
    i = AL.index("H")
    rc, sums, counts, used = raw(dec, page[None].copy(), 1, 30, LH, [(0, 0, 0, 1, 0)] * n, [i])
    assert rc == 0 and launches(dec) == 1
    one = L.empty(dec.font)
    assert L.learn_crop(dec.font, one, crop(page, 1, 0, 30, LH), [i])[0] == 1
    assert np.array_equal(counts, one.counts * n) and np.array_equal(sums, one.sums * n) and used.all() and len(used) == n
    assert counts.max() == n and sums.max() > 200 * n


# ---- sizes ----------------------------------------------------------------------------------------------------------------------

def test_one_glyph_and_319_glyphs(dec):
    dec.set_font(MONO, 13.0, "H")
    dec.set_font_candidates([])
    check(dec, [noisy(70, 20, 66)], [[(1, "HHHH")]], 2, 60, LH)
    dec.set_font(MONO, 10.0, ALPHABET_319)
    rng = np.random.default_rng(67)
    text = "".join(ALPHABET_319[j] for j in rng.permutation(319)[:40])
    got = check(dec, [noisy(300, 20, 68)], [[(1, text), (2, ALPHABET_319[318] + ALPHABET_319[0])]], 2, 290, LH)
    assert got.counts.sum() > 30


def test_boxes_wider_than_a_wave_and_than_the_workgroup(dec):
    """A 13 px glyph's cell has more entries than a wave has lanes, a 40 px glyph's more than the workgroup has threads."""
    dec.set_font(SANS, 13.0, AL)
    dec.set_font_candidates([(SANS, 40.0, False, 1.0)])
    small, big = (max(g.stride * g.box_h for g in f.s.glyphs[:len(AL)]) for f in fonts_of(dec))
    assert 64 < small <= 256 < big
    page = noisy(200, 64, 69)
    check(dec, [page], [[(1, "Hmbo")]], 2, 190, LH)
    got = check(dec, [page], [[(1, "Hmbo")]], 2, 190, 60, fonts=[[1]], font=1)
    assert got.counts.sum() == 4


@pytest.mark.parametrize("width,n_launches", [(4084, 1), (4085, 2)])
def test_strip_in_lds_and_in_global_memory(dec, width, n_launches):
    """A 4100 x 17 page: 16 rows of 4084 columns fill LDS_STRIP_MAX to the byte, one column more does not fit and the strips are
    built in global memory by a launch of their own.  Glyphs at both ends of the crop and in the middle, by their pens."""
    dec.set_font(MONO, 8.0, AL)
    dec.set_font_candidates([])
    page = noisy(4100, 17, 70)
    pens = [[[0, 300, 64 * 2000, 64 * (width - 12), 64 * (width - 3)], [64 * 100]]]
    got = check(dec, [page], [[(0, "Hobim"), (1, "a")]], 0, width, 16, pens=pens, n_launches=n_launches)
    assert list(got.used[0][0]) == [1, 1, 1, 1, 0] and got.used[0][1][0] == 1


def test_line_lengths(dec):
    """Lines of 0, 1, 64, 65 and 257 characters: the walk goes in 64-character batches, and a wave takes every fourth character."""
    dec.set_font(MONO, 8.0, AL)
    dec.set_font_candidates([])
    rng = np.random.default_rng(71)
    texts = ["".join(rng.choice(list(AL), n)) for n in (0, 1, 64, 65, 257)]
    page = noisy(1300, 30, 72)
    lines = [[(0, texts[0]), (0, texts[1]), (3, texts[2]), (9, texts[3]), (14, texts[4])]]
    got = check(dec, [page], lines, 3, 1290, 12)
    assert [int(u.sum()) for u in got.used[0]] == [0, 1, 64, 65, 257]
    check(dec, [page], lines, 3, 1290, 12, offsets=[[[int(v) for v in rng.integers(-5, 6, len(t))] for t in texts]])


# ---- the learned font on the device ------------------------------------------------------------------------------------------------

def test_the_learned_font_on_the_device(dec):
    """Hinted 8 px pages read with the unhinted font: DecodeFont.learned of the device's sums is the model's font byte for byte;
    uploaded as candidate 1, score_text's terms of the used characters sum to no more than the base font's (per pixel the rounded
    mean is the integer minimiser); and a decode under set_font(learned) is the fast model's over the same tables."""
    hinted = DecodeFont(MONO, 8.0, AL, hinting=True)
    texts = ["Hinein bin ihr Hirn", "mohr ahoi ab in rom", "bahn in rom heim an", "oben Ihm ein Hai ab"]
    W = 130
    pages = [np.vstack([S.draw_text(hinted, t, W, 12) for t in texts[:2]]), np.vstack([S.draw_text(hinted, t, W, 12) for t in texts[2:]])]
    lines = [[(0, texts[0]), (12, texts[1])], [(0, texts[2]), (12, texts[3])]]
    dec.set_font(MONO, 8.0, AL)
    dec.set_font_candidates([])
    base = dec.font
    got = check(dec, pages, lines, 0, W, 12)
    for grow in (0, 1):
        learned = base.learned(got, min_count=1, grow=grow)
        cells, inked = L.learned_phases(base, got, 1, grow)
        assert (learned.n_learned, learned.n_inked) == (len(cells), inked) and 0 < len(cells) < inked
        want = L.Tables(base, cells)
        for i in range(len(AL)):
            for p in range(64):
                a, b = learned.phase(i, p), want.phase(i, p)
                assert a[1:] == b[1:] and np.array_equal(a[0], b[0]), (grow, i, p)
        assert learned.y_bits == 0 and np.array_equal(learned.increments(), base.increments()) and learned.origin == base.origin
        dec.set_font_candidates([learned])
        scores = dec.score_text(pages, lines + [], 0, W, 12, fonts=[[0, 0], [0, 0]]), dec.score_text(pages, lines, 0, W, 12, fonts=[[1, 1], [1, 1]])
        total = [sum(int(s.terms[u.astype(bool)].astype(np.int64).sum()) for ps, us in zip(sc, got.used) for s, u in zip(ps, us)) for sc in scores]
        assert total[1] <= total[0] < 0, total
        if grow:
            learned.close()
    learned = base.learned(got)
    fm = FastModel(MONO, 8.0, AL)
    fm.font.close()
    fm.font = learned
    want = [fm.decode_image(p, 0, 0, W, 12, 12) for p in pages]
    dec.set_font(learned)
    assert dec.decode(pages, 0, 0, W, 12, 12) == want
    assert [t for pg in want for _, t in pg] != []
    hinted.close()


def test_adding_calls_up(dec):
    """LearnedGlyphs add: two calls of a page each are one call of both."""
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([])
    a = dec.learn_text(PAGES[:1], LINES[:1], 3, 110, LH)
    b = dec.learn_text(PAGES[1:], LINES[1:], 3, 110, LH)
    both = dec.learn_text(PAGES, LINES, 3, 110, LH)
    total = a + b
    assert isinstance(total, LearnedGlyphs)
    same(total, L.Learned(both.sums, both.counts, both.used))
    with pytest.raises(ValueError, match="not this font's"):
        dec.font.learned(LearnedGlyphs(both.sums[:-4], both.counts, both.used))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(dec):
    """Every refusal of include/focr_decode.h, each with its own words and nothing launched or written; the decoder learns afterwards."""
    lib, h = dec._lib, dec._h
    batch = np.ascontiguousarray(np.stack([noisy(80, 20, 31), noisy(80, 20, 32)]))
    with LineDecoder(0) as bare:  # no decode font
        bare.font = DecodeFont(MONO, 13.0, AL)  # only so that raw() can size the outputs
        rc = raw(bare, batch, 0, 80, LH, [], [])[0]
        assert rc != 0 and b"focr_decoder_learn_text: no decode font (focr_decoder_set_font)" in bare._lib.focr_decoder_last_error(bare._h)
        assert launches(bare) == 0
        bare.font = None
    dec.set_font(MONO, 13.0, AL)
    dec.set_font_candidates([(SANS, 13.0, False, 1.0)])
    chars = [AL.index(c) for c in "ahoi"]
    good = [(0, 2, 0, 4, 0), (1, 2, 0, 4, 1)]
    seen = set()

    def refused(*words, **kw):
        args = dict(x=1, width=70, lh=LH, recs=good, chars=chars)
        args.update(kw)
        assert raw(dec, batch, 1, 70, LH, good, chars)[0] == 0 and launches(dec) == 1 and lib.focr_decoder_last_learn_text_ms(h) > 0
        rc, sums, counts, used = raw(dec, batch, **args)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and msg.startswith("focr_decoder_learn_text: ") and all(w in msg for w in words), msg
        assert launches(dec) == 0 and lib.focr_decoder_last_learn_text_ms(h) == 0.0 and msg not in seen
        assert (sums == 7).all() and (counts == 7).all() and (used == 7).all()
        seen.add(msg)

    refused("width 0", width=0)
    refused("line_height 0", lh=0)
    refused("pens and offsets together", pens=[0, 1, 2, 3], offsets=[0, 0, 0, 0])
    refused("line 1", "font 2", "1 candidates", recs=[good[0], (1, 2, 0, 4, 2)])
    refused("line 1", "page 2 of 2", recs=[good[0], (2, 2, 0, 4, 0)])
    refused("line 0", "n_chars", recs=[(0, 2, 1, 4, 0)])
    refused("character 2", "alphabet", chars=[0, 1, len(AL), 2])
    refused("pen 3", "2^24", pens=[0, 1, 2, 1 << 24])
    refused("null sums", sums=False)
    refused("null counts", counts=False)
    refused("font 2 to learn", "1 candidates", font=2)
    # 2^24 listed characters: 65 536 lines that share 256 characters; one line less is accepted (and not run here)
    wide = [0] * 256
    refused("2^24 or more listed characters", "list fewer lines", recs=[(0, 2, 0, 256, 0)] * 65536, chars=wide)
    # origins: built fonts have whole ones, so bend a copy of the candidate's struct
    cand = dec._candidates[0]
    keep = cand.s.origin_x
    for ox in (0.5, -1.0):
        cand.s.origin_x = ox
        assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
        rc = raw(dec, batch, 1, 70, LH, good, chars, pens=[0, 9, 18, 27])[0]
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and all(w in msg for w in ("line 1", "pens", "origin_x", "whole number")) and launches(dec) == 0, msg
    cand.s.origin_x = keep
    assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
    larr, carr = (N.TextLine * 2)(*good), np.asarray(chars, dtype=np.uint16)
    sarr, karr = np.zeros(dec.font.s.bitmaps_len, dtype=np.uint32), np.zeros(64 * len(AL), dtype=np.uint32)
    f, sp, kp = lib.focr_decoder_learn_text, sarr.ctypes.data, karr.ctypes.data
    for words, call in (("null pages", lambda: f(h, None, 0, 2, 80, 20, 1, 70, LH, larr, 2, carr.ctypes.data, None, None, None, 4, 0, sp, kp, None)),
                        ("null lines", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, None, 2, carr.ctypes.data, None, None, None, 4, 0, sp, kp, None)),
                        ("null chars", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, larr, 2, None, None, None, None, 4, 0, sp, kp, None)),
                        ("page too large", lambda: f(h, batch.ctypes.data, 0, 2, 0xffff * 16 + 1, 20, 1, 70, LH, larr, 0, carr.ctypes.data, None, None, None, 4, 0, sp, kp, None))):
        assert raw(dec, batch, 1, 70, LH, good, chars)[0] == 0 and launches(dec) == 1
        assert call() != 0
        msg = lib.focr_decoder_last_error(h).decode()
        assert msg.startswith("focr_decoder_learn_text: ") and words in msg and launches(dec) == 0 and msg not in seen
        seen.add(msg)
    # no lines: nothing launched, zeros written
    rc, sums, counts, _ = raw(dec, batch, 1, 70, LH, [], chars)
    assert rc == 0 and launches(dec) == 0 and not sums.any() and not counts.any()
    # usable afterwards
    check(dec, list(batch), [[(2, "ahoi")], [(2, "ahoi")]], 1, 70, LH, fonts=[[0], [1]], font=1)
    for kw, words in ((dict(font=2), "font must be"), (dict(pens=[[[0] * 4], []], offsets=[[[0] * 4], []]), "not both"), (dict(use=[[[1] * 3], []]), "use flags"),
                      (dict(use=[[]]), "one entry per line")):
        with pytest.raises(ValueError, match=words):
            dec.learn_text(list(batch), [[(2, "ahoi")], []], 1, 70, LH, **kw)
    with pytest.raises(ValueError, match="not in the alphabet"):
        dec.learn_text(list(batch), [[(2, "ahoy")], []], 1, 70, LH)


# ---- the last run, memory -----------------------------------------------------------------------------------------------------------

def test_a_decode_before_the_call_answers_the_same_afterwards(dec):
    """A decode, then learn_text of its own reading in the LDS and the global-strip form: the run's getters, timings and verify,
    and the other text calls' last timings, answer afterwards as they did before."""
    dec.set_font(SANS, 13.0, AL)
    dec.set_font_candidates([])
    pages = [S.draw_text(dec.font, "Hinein bin ihr", 150, LH), S.draw_text(dec.font, "mohr ahoi", 150, LH, shift64=9)]
    lines, pens, costs = dec.decode(pages, 0, 0, 146, LH, LH, whole_line=True)
    dec.score_text(pages, lines, 0, 146, LH, pens=pens)
    dec.verify_text(pages, lines, 0, pens=pens)
    dec.align_text(pages, lines, 0, 146, LH)
    lib, h = dec._lib, dec._h
    timings = lambda: (lib.focr_decoder_last_score_text_ms(h), lib.focr_decoder_last_score_text_launches(h),  # noqa: E731
                       lib.focr_decoder_last_verify_text_ms(h), lib.focr_decoder_last_verify_text_launches(h),
                       lib.focr_decoder_last_align_text_ms(h), lib.focr_decoder_last_align_text_launches(h))
    before, tb = snapshot(dec), timings()
    got = check(dec, pages, lines, 0, 146, LH, pens=pens)
    assert got.counts.sum() > 15 and lib.focr_decoder_last_learn_text_ms(h) > 0
    dec.learn_text([noisy(4100, 17, 5)], [[(0, "Hm")]], 0, 4100, 16)
    assert launches(dec) == 2
    assert snapshot(dec) == before and timings() == tb


def test_memory_returns():
    """A decoder that only ever called learn_text, with strips in LDS and in global memory, gives every device byte back."""
    before = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, AL)
        d.set_font_candidates([(SANS, 13.0, False, 1.0)])
        up = N.hip().focr_debug_device_bytes()
        d.learn_text([noisy(257, 33, 41)], [[(0, "ahoi"), (12, "Hob in")]], 2, 250, LH, fonts=[[0, 1]], use=[[[1, 0, 1, 1], [1] * 6]], font=1)
        small = N.hip().focr_debug_device_bytes()
        d.learn_text([noisy(4100, 17, 42)], [[(0, "ahoi")]], 0, 4100, 16)
        assert launches(d) == 2
        peak = N.hip().focr_debug_device_bytes()
        assert before < up < small < peak
        assert d._lib.focr_decoder_n_lines(d._h) == 0  # no run was ever made
    assert N.hip().focr_debug_device_bytes() == before


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------

def test_cli_learn(dec, tmp_path):
    """focr --learn FILE on two small hinted pages with the true reading of the first: stdout is the Python path's (a plain decode
    for the slots, learn_text of the paired lines, DecodeFont.learned, set_font, decode), stderr has the summary, and every usage
    error is raised."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(os.path.dirname(os.path.dirname(FOCR)), "csrc"), "cli"], check=True)
    hinted = DecodeFont(MONO, 8.0, AL, hinting=True)
    texts = [["Hinein bin ihr Hirn", "mohr ahoi ab in rom", "bahn in rom heim an"], ["oben Ihm ein Hai ab", "Horn in der Bahn an", "ahoi bin am Rhein"]]
    texts = [[t.replace("d", "b").replace("R", "H").replace("B", "H") for t in pg] for pg in texts]
    W = 130
    blank = np.full((12, W), 255, dtype=np.uint8)
    pages = [np.vstack([S.draw_text(hinted, pg[0], W, 12), blank, S.draw_text(hinted, pg[1], W, 12), S.draw_text(hinted, pg[2], W, 12)]) for pg in texts]
    hinted.close()
    paths = [str(tmp_path / f"page{i}.pgm") for i in range(2)]
    for path, page in zip(paths, pages):
        save_pgm(path, page)
    reading = str(tmp_path / "reading.txt")
    with open(reading, "w") as f:
        f.write(texts[0][0] + "\n\n" + texts[0][2] + "\n" + texts[1][0] + "\n")  # the second slot skipped, and it stops early
    cmd = [FOCR, "-f", MONO, "-t", "8", "-a", AL, "-w", str(W), "--line-height", "12", "--line-advance", "12", "-i"] + paths + ["--learn", reading]
    for extra, kw in (([], {}), (["--learn-min-count", "2"], dict(min_count=2)), (["--learn-grow", "1"], dict(grow=1))):
        dec.set_font(MONO, 8.0, AL)
        dec.set_font_candidates([])
        slots = dec.decode(pages, 0, 0, W, 12, 12)
        assert [[y for y, _ in pg] for pg in slots] == [[0, 24, 36], [0, 24, 36]]
        trusted = [[(0, texts[0][0]), (36, texts[0][2])], [(0, texts[1][0])]]
        glyphs = dec.learn_text(pages, trusted, 0, W, 12)
        learned = dec.font.learned(glyphs, **kw)
        dec.set_font(learned)
        want = dec.decode(pages, 0, 0, W, 12, 12)
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines() == [t for pg in want for _, t in pg]
        n_used = int(sum(u.sum() for pg in glyphs.used for u in pg))
        n_all = sum(len(t) for pg in trusted for _, t in pg)
        assert r.stderr == f"learn: {n_used} characters used, {n_all - n_used} skipped, {learned.n_learned} of {learned.n_inked} cells with ink learned\n"
        assert n_used > 40 and 0 < learned.n_learned < learned.n_inked
    for extra, words in ((["--pen-search", "2"], "--pen-search"), (["--whole-line"], "--whole-line"), (["--baseline-search", "1"], "--baseline-search"),
                         (["--whole-line", "--whole-baseline", "1"], "--whole-"), (["--font-candidate", "t=9"], "--font-candidate"),
                         (["--test", str(tmp_path / "t")], "--test"), (["--rank-text", "ab"], "--rank-text"), (["--learn-min-count", "0"], "at least 1")):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--learn" in r.stderr and words in r.stderr and r.stdout == "", (extra, r.stderr)
    for extra, words in ((["--learn-min-count", "2"], "--learn-min-count"), (["--learn-grow", "1"], "--learn-grow")):
        r = subprocess.run(cmd[:-2] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and words in r.stderr and "--learn <FILE>" in r.stderr and r.stdout == ""
    with open(reading, "w") as f:
        f.write(texts[0][0] + "\nahoy\n")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "line 2" in r.stderr and "'y' is not in the alphabet" in r.stderr and r.stdout == ""
    r = subprocess.run(cmd[:-1] + [str(tmp_path / "missing.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "cannot read" in r.stderr


# ---- the seeded readings -----------------------------------------------------------------------------------------------------------

def test_seeded_readings(dec):
    """The random readings of tests/focr_text_fuzz.py (their lines, ys, shared characters, fonts and placements) fed to learn_text,
    every font of the case learned in turn."""
    n_used = 0
    for family in TF.DRAWN:
        for i in TF.IDS[family][::3]:
            s = TF.setup(family, i)
            dec.set_font(s.fonts[0], s.case.size)
            dec.set_font_candidates(s.fonts[1:])
            x, _, width, lh, _ = s.geo
            for page in range(len(s.pages)):
                r = TF.random_reading(family, i, page)
                batch = np.ascontiguousarray(np.asarray(s.pages[page])[None])
                recs = [(0, y, first, n, k) for y, first, n, k, _ in r.recs]
                along = dict(pens=r.along) if r.placement == "pens" else dict(offsets=r.along) if r.placement == "offsets" else {}
                for k, font in enumerate(s.fonts):
                    rc, sums, counts, used = raw(dec, batch, x, width, lh, recs, r.chars, font=k, **along)
                    assert rc == 0, dec._lib.focr_decoder_last_error(dec._h)
                    acc, flags = L.empty(font), []
                    for _, y, first, n, kk in recs:
                        if kk != k:
                            flags.append(np.zeros(n, dtype=np.uint8))
                            continue
                        at = None if r.along is None else r.along[first: first + n]
                        flags.append(L.learn_crop(font, acc, crop(s.pages[page], x, y, width, lh), r.chars[first: first + n],
                                                  at if r.placement == "pens" else None, at if r.placement == "offsets" else None))
                    where = (family, s.name, page, k)
                    assert np.array_equal(counts, acc.counts) and np.array_equal(sums, acc.sums), where
                    assert np.array_equal(used[: sum(len(f) for f in flags)], np.concatenate(flags) if flags else np.zeros(0, dtype=np.uint8)), where
                    n_used += int(acc.counts.sum())
    assert n_used > FC.N_CASES

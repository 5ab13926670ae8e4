"""focr_decoder_refine_text (refine_text_kernel, refine_strip_kernel, LineDecoder.refine_text, placed_pens): a caller's reading repaired
against the composed line error.  Device == tests/focr_refine_model.py (the definition step by step over the phase tables the
decoder itself was given) at the shapes the kernel branches on: the alphabet and the candidates against the workgroup's 256 lanes,
the radius, the sweeps, the line's length against the waves, pens that lie on one another, pens at 0, crops cut on every side,
empty and one-column crops, a candidate font, the strip in LDS and in global memory, tiles of up to 11 dwords a row (24 to 44 px),
the table's last tile, a hinted font; then score_text on the device at the output
pens, the page the feature is for, every refusal, the last run's getters and device memory.  Every comparison is ==."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_refine_model as R
import focr_slack_model as K
import focr_score_text_model as S
from focr_fast_model import ALPHABET_319, ASCII95, FastModel, crop
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineDecoder, placed_pens, save_pgm
from font_ocr_amd import _native as N
from test_gpu_focr_score_text import AL, FOCR, LH, MONO, SANS, SERIF, noisy, snapshot

pytestmark = pytest.mark.gpu

_fms = {}


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def fm_of(font, size, al, hinting=False):
    key = (font, size, al, hinting)
    if key not in _fms:
        _fms[key] = FastModel(font, size, al, hinting)
    return _fms[key]


def setup(dec, font, size, al, cands=()):
    """The decoder on the very tables the model reads: font 0 and the candidates, as FastModels."""
    fms = [fm_of(font, size, al)] + [fm_of(f, s, al) for f, s in cands]
    dec.set_font(fms[0].font)
    dec.set_font_candidates([f.font for f in fms[1:]])
    return fms


def launches(dec):
    return dec._lib.focr_decoder_last_refine_text_launches(dec._h)


def check(dec, fms, pages, lines, x, width, lh, pens, fonts=None, radius=4, sweeps=4, glyphs=True, n_launches=1):
    """refine_text equals the model line by line: base, both costs, the sweeps, the changed characters, the text and every pen."""
    got = dec.refine_text(pages, lines, x, width, lh, pens, fonts=fonts, radius=radius, sweeps=sweeps, glyphs=glyphs)
    assert launches(dec) == (n_launches if any(len(pg) for pg in lines) else 0)
    for p, page in enumerate(pages):
        assert len(got[p]) == len(lines[p])
        for q, (y, text) in enumerate(lines[p]):
            fm = fms[fonts[p][q] if fonts is not None else 0]
            want = R.refine_crop(fm, crop(np.asarray(page), x, y, width, lh), [fm.alphabet.index(c) for c in text], pens[p][q], radius, sweeps, glyphs)
            g = got[p][q]
            assert g[:6] == (want.base, want.cost_in, want.cost, want.sweeps, want.changed, R.text_of(fm, want.idx)), (p, q, g[:6], want[:5])
            assert g.pens.dtype == np.uint32 and np.array_equal(g.pens, want.pens), (p, q)
            assert g.base + g.cost >= 0 and g.cost <= g.cost_in
    return got


def spaced(n, step, start=0):
    return [start + step * g for g in range(n)]


# ---- against the model, where the kernel branches ---------------------------------------------------------------------------

@pytest.mark.parametrize("al", ["m", "im", ASCII95[:65], ALPHABET_319], ids=["1", "2", "65", "319"])
def test_alphabets(dec, al):
    """One glyph (a step can only move it), two, a wave and a glyph, and 319 with their tie groups (equal glyphs: the lower index),
    on noise, where every candidate costs something else; the pens 4 px apart, so that neighbours lie on one another."""
    fms = setup(dec, SANS, 13.0, al)
    text = "".join(al[(7 * g) % len(al)] for g in range(6))
    check(dec, fms, [noisy(60, 24, 3)], [[(2, text), (4, text[:2])]], 3, 50, LH, [[spaced(6, 256, 5), [70, 70]]], radius=1, sweeps=2)


@pytest.mark.parametrize("n_glyphs,radius", [(4, 31), (4, 32), (256, 0), (65, 4), (12, 10)], ids=["252", "260", "256", "585", "252b"])
def test_candidate_counts(dec, n_glyphs, radius):
    """A * (2N + 1) candidates over 256 lanes: four short of them, exactly them, four more, and more than two passes."""
    al = {4: "rnmi", 12: AL, 65: ASCII95[:65], 256: ALPHABET_319[:256]}[n_glyphs]
    fms = setup(dec, SANS, 13.0, al)
    text = "".join(al[(5 * g + 1) % len(al)] for g in range(4))
    check(dec, fms, [noisy(50, 22, 11)], [[(1, text)]], 2, 44, LH, [[spaced(4, 300, 40)]], radius=radius, sweeps=2)


@pytest.mark.parametrize("radius", [0, 64])
@pytest.mark.parametrize("glyphs", [True, False], ids=["glyphs", "pens"])
def test_radius_and_own_glyph_only(dec, radius, glyphs):
    """No offset at all and a whole pixel either way; with glyphs=False a character keeps its glyph (radius 0 then changes nothing)."""
    fms = setup(dec, SERIF, 13.0, AL)
    got = check(dec, fms, [noisy(70, 24, 21)], [[(3, "Hi mob"), (3, "ahoi")]], 4, 60, LH, [[spaced(6, 330, 70), spaced(4, 200)]], radius=radius, sweeps=2,
                glyphs=glyphs)
    if not glyphs:
        assert [g.text for g in got[0]] == ["Hi mob", "ahoi"]
        assert radius or all(g.changed == 0 and g.cost == g.cost_in and g.sweeps == 1 for g in got[0])


def test_sweeps(dec):
    """sweeps = 0 only evaluates; one sweep; a drawn line read one character wrong converges before its cap; on noise two sweeps are
    cut short (a third still changes something)."""
    fms = setup(dec, SANS, 13.0, AL)
    pens = K.font_pens(fms[0], "Hinein bin")
    drawn = K.draw_at(SANS, 13.0, AL, "Hinein bin", pens, 80, LH)
    noise = noisy(80, LH, 5)
    lines, ps = [[(0, "Hinoin bin")]], [[[int(s) for s in pens]]]
    got = check(dec, fms, [drawn], lines, 0, 80, LH, ps, sweeps=0)[0][0]
    assert (got.sweeps, got.changed, got.text) == (0, 0, "Hinoin bin") and got.cost == got.cost_in > -got.base
    got = check(dec, fms, [drawn], lines, 0, 80, LH, ps, sweeps=1)[0][0]
    assert got.sweeps == 1 and got.text == "Hinein bin" and got.cost == -got.base
    got = check(dec, fms, [drawn], lines, 0, 80, LH, ps, sweeps=8)[0][0]
    assert got.sweeps == 2 and got.changed == 1 and got.text == "Hinein bin" and got.cost == -got.base
    two = check(dec, fms, [noise], lines, 0, 80, LH, ps, sweeps=2)[0][0]
    three = check(dec, fms, [noise], lines, 0, 80, LH, ps, sweeps=3)[0][0]
    assert two.sweeps == 2 and three.sweeps == 3 and three.cost < two.cost


def test_line_lengths(dec):
    """Lines of 0, 1, 63, 64, 65 and 257 characters, 1.5 px apart: the copy, the neighbour scan and the count of changed characters
    over no thread, one, a wave less one, a wave, a wave and one, the workgroup and one.  The longest runs past the crop: its last
    glyphs lie wholly right of it, every D there is 0 and they stay."""
    fms = setup(dec, MONO, 8.0, AL)
    rng = np.random.default_rng(5)
    ns = (0, 1, 63, 64, 65, 257)
    texts = ["".join(rng.choice(list(AL), n)) for n in ns]
    lines = [[(y, t) for y, t in zip((0, 0, 2, 5, 9, 14), texts)]]
    got = check(dec, fms, [noisy(330, 30, 51)], lines, 3, 320, 12, [[spaced(n, 96, 7) for n in ns]], radius=1, sweeps=1)
    g = got[0][0]
    assert (g.cost_in, g.cost, g.sweeps, g.changed, g.text, len(g.pens)) == (0, 0, 1, 0, "", 0) and g.base > 0
    long = got[0][5]
    assert long.text[-30:] == texts[5][-30:] and list(long.pens[-30:]) == spaced(257, 96, 7)[-30:] and long.changed > 100


def test_every_glyph_on_every_other_and_pens_at_zero(dec):
    """All pens equal: every character reaches every step's window.  Pens at 0: the candidates j < 0 are dropped."""
    fms = setup(dec, SANS, 13.0, AL)
    text = "".join(AL[(5 * g) % len(AL)] for g in range(70))
    check(dec, fms, [noisy(60, 24, 8)], [[(2, text)]], 2, 50, LH, [[[640] * 70]], radius=2, sweeps=2)
    got = check(dec, fms, [noisy(60, 24, 9)], [[(2, "Hmi")]], 2, 50, LH, [[[0, 0, 3]]], radius=4, sweeps=3)
    assert all(0 <= int(s) <= 15 for s in got[0][0].pens)
    drawn = K.draw_at(SANS, 13.0, AL, "m", [0], 30, LH)
    got = check(dec, fms, [drawn], [[(0, "m")]], 0, 30, LH, [[[3]]], radius=4, sweeps=2)
    assert got[0][0].pens.tolist() == [0] and got[0][0].cost == -got[0][0].base


def test_crops(dec):
    """Glyphs cut by the crop's right and bottom edge; by its left and top edge (a font whose boxes start 3 columns left of the pen and
    4 rows above the crop's top: the tables are the caller's); a glyph wholly right of the crop; empty crops (x at the page's width,
    y past the page); one column; one row."""
    fms = setup(dec, SANS, 13.0, AL)
    pages = [noisy(70, 30, 91)]
    check(dec, fms, pages, [[(20, "Hi H"), (5, "mohr")]], 3, 12, LH, [[[0, 560, 900, 64 * 30], spaced(4, 200)]], radius=3, sweeps=2)
    for x, y in ((70, 2), (5000, 2), (3, 30), (3, 1000)):
        got = check(dec, fms, pages, [[(y, "Hinein")]], x, 60, LH, [[spaced(6, 300)]])
        assert got[0][0][:6] == (0, 0, 0, 1, 0, "Hinein")
    check(dec, fms, pages, [[(5, "Hi"), (6, "ab")]], 9, 1, LH, [[[0, 5], [130, 140]]], radius=8, sweeps=2)
    check(dec, fms, pages, [[(7, "Hi mob")]], 2, 60, 1, [[spaced(6, 280)]], radius=2, sweeps=2)
    bent = FastModel(SANS, 13.0, AL)
    for i in range(len(AL)):
        for p in range(64):
            bent.font.s.glyphs[i].off_x[p] -= 3
            bent.font.s.glyphs[i].off_y[p] -= 4
    dec.set_font(bent.font)
    _, fx, fy = bent.font.phase(AL.index("H"), 0)
    assert int(bent.font.origin[0]) + fx < 0 and fy < 0  # the H at pen 0 starts left of the crop and above it
    check(dec, [bent], pages, [[(2, "Hmob")]], 5, 40, 9, [[[0, 100, 400, 800]]], radius=4, sweeps=2)
    dec.set_font(fms[0].font)
    bent.close()


def test_candidate_font_beside_the_decode_font(dec):
    """Lines in font 0 and in two candidates with boxes and increments of their own, in one call, on two pages of one size."""
    fms = setup(dec, MONO, 13.0, AL, [(SANS, 13.0), (SERIF, 11.0)])
    pages = [noisy(120, 44, 81), noisy(120, 44, 82)]
    lines = [[(2, "Hinein"), (2, "Hinein"), (22, "ab Hm")], [(22, "mohr")]]
    pens = [[spaced(6, 400, 3), spaced(6, 300, 3), spaced(5, 250)], [spaced(4, 350, 64)]]
    check(dec, fms, pages, lines, 4, 100, LH, pens, fonts=[[0, 1, 2], [1]], radius=3, sweeps=2)


@pytest.mark.parametrize("width,n_launches", [(3000, 1), (4100, 2)])
def test_strip_in_lds_and_in_global_memory(dec, width, n_launches):
    """A 4100 x 17 page: 16 rows of 3000 columns fit LDS beside the window, 4100 do not fit it at all, and the strips are then built
    in global memory by a launch of their own.  Glyphs at both ends of the crop and in the middle, by their pens."""
    fms = setup(dec, MONO, 13.0, AL)
    pens = [[[0, 300, 64 * 1500 + 7, 64 * 1500 + 300, 64 * (width - 9)], [64 * (width - 20), 64 * (width - 20) + 200]]]
    check(dec, fms, [noisy(4100, 17, 101)], [[(0, "Hmabe"), (1, "oh")]], 0, width, 16, pens, radius=2, sweeps=1, n_launches=n_launches)


def ndws(fm):
    """The dwords per tile row (DevGlyph.ndw, stride / 4) of every glyph of a FastModel, as the upload lays its tiles out."""
    out = []
    for i in range(len(fm.alphabet)):
        g = fm.font.s.glyphs[i]
        assert g.stride % 4 == 0 and g.stride >= fm.font.phase(i, 0)[0].shape[1] > g.stride - 4
        out.append(g.stride // 4)
    return out


WIDE = {24.0: {1, 2, 6}, 30.0: {2, 7, 8}, 36.0: {2, 8, 9}, 44.0: {2, 10, 11}}


@pytest.mark.parametrize("size", sorted(WIDE), ids=["24", "30", "36", "44"])
def test_wide_tiles(dec, size):
    """Tiles of more than four dwords a row: refine_term's second and third trip through a row and their partial tails (ndw 6 ..= 11;
    every font setup above stays within 4).  Sans over "il.W@m" on noise, the pens so close that the wide glyphs lie on one another;
    the crop cuts a W at its right edge and every tall glyph at its bottom; then the same with boxes that start 5 columns left of
    the pen (a W at pen 0 is cut at the crop's left edge), and once with glyphs=False."""
    al = "il.W@m"
    fms = setup(dec, SANS, size, al)
    assert set(ndws(fms[0])) == WIDE[size]
    g = fms[0].font.s.glyphs
    assert max(g[i].stride * g[i].box_h for i in range(len(al))) * 2 * 255 * 255 < 1 << 31  # the upload's box-area rule: set_font took it
    px = int(size)
    lh, w = px - 4, 3 * px
    pages = [noisy(w + 9, px + 12, int(size))]
    pens = [0, 16 * px, 40 * px, 64 * px, 64 * (w - px // 2), 64 * (w - px // 2) + 90]
    lines, ps = [[(3, "W@mi.W"), (9, "ml@W")]], [[pens, pens[1:5]]]
    check(dec, fms, pages, lines, 4, w, lh, ps, radius=2, sweeps=2)
    check(dec, fms, pages, lines, 4, w, lh, ps, radius=2, sweeps=2, glyphs=False)
    bent = FastModel(SANS, size, al)
    for i in range(len(al)):
        for p in range(64):
            bent.font.s.glyphs[i].off_x[p] -= 5
    dec.set_font(bent.font)
    assert int(bent.font.origin[0]) + bent.font.phase(al.index("W"), 0)[1] < 0
    check(dec, [bent], pages, lines, 4, w, lh, ps, radius=2, sweeps=2)
    dec.set_font(fms[0].font)
    bent.close()


@pytest.mark.parametrize("size,al,ndw", [(13.0, "Wi", 1), (8.0, "iH", 2), (13.0, "im", 3), (17.0, "iW", 5), (20.0, "iW", 6)], ids=["1", "2", "3", "5", "6"])
def test_last_glyph_of_the_table(dec, size, al, ndw):
    """The table's last tile (the last glyph's phase 63) is read dword by dword where four dwords would pass the table's end: the
    last glyph drawn at a pen of phase 63 and read as the other one, so the step's winner is that tile; narrow and wide rows."""
    fms = setup(dec, SANS, size, al)
    assert ndws(fms[0])[-1] == ndw and int(fms[0].font.origin[0]) == 0
    last, other = al[1], al[0]
    text, pens = other + last + other, [64, 64 * 30 + 63, 64 * 60]
    page = K.draw_at(SANS, size, al, text, pens, 100, 30)
    got = check(dec, fms, [page], [[(0, other * 3)]], 0, 100, 30, [[pens]], radius=1, sweeps=2)[0][0]
    assert got.text == text and got.pens.tolist() == pens and got.cost == -got.base
    check(dec, fms, [noisy(100, 30, ndw)], [[(0, other * 3), (2, last * 2)]], 0, 100, 30, [[pens, pens[1:]]], radius=1, sweeps=2)


def test_the_neighbour_scan_allows_for_every_sweep(dec):
    """The line of tests/test_focr_refine_fuzz_host.py on which the scan for the others that reach a step's window must allow a
    pen radius * sweeps of movement: two `m` that come 8 px closer to each other in eight sweeps of radius 64.  With a slack of
    one radius the right one ends at 1107 (the host test pins both results); no seeded line tells the two apart."""
    from test_focr_refine_fuzz_host import ramp_line
    fm, page, idx, pens = ramp_line()
    dec.set_font(fm.font)
    dec.set_font_candidates([])
    got = check(dec, [fm], [page], [[(0, "mm")]], 0, page.shape[1], page.shape[0], [[pens]], radius=64, sweeps=8, glyphs=False)[0][0]
    assert got.pens.tolist() == [596, 1279] and got.sweeps == 8 and idx == [0, 0]
    setup(dec, SANS, 13.0, AL)
    fm.close()


def test_a_hinted_font_beside_a_candidate(dec):
    """Mono 8 px hinted (learn_text's pinned setup: its phases differ from the unhinted font's in their boxes) with the unhinted
    font as a candidate beside it, lines in both."""
    fms = [fm_of(MONO, 8.0, AL, True), fm_of(MONO, 8.0, AL)]
    assert fms[0].font.hinting and not fms[1].font.hinting
    dec.set_font(fms[0].font)
    dec.set_font_candidates([fms[1].font])
    pages = [noisy(70, 26, 61)]
    lines, pens = [[(2, "Hinein"), (2, "Hinein"), (11, "mohr ab")]], [[spaced(6, 290, 3), spaced(6, 290, 3), spaced(7, 250)]]
    check(dec, fms, pages, lines, 3, 60, 12, pens, fonts=[[0, 1, 0]], radius=3, sweeps=3)


# ---- on the device alone ------------------------------------------------------------------------------------------------------

def test_score_text_at_the_output_pens(dec):
    """Mono at its own advances: no two footprints meet, and score_text of the output at the output pens costs what refine_text says,
    before and after; the misread characters are repaired and the line costs -line_base."""
    fms = setup(dec, MONO, 13.0, AL)
    text, read = "Hinein bin ihr", "Hinoin bim ihr"
    pens = [int(s) for s in placed_pens(dec.font, text)]  # the pen loop's own f32 walk
    assert pens == [d - 64 * int(dec.font.origin[0]) for d in S.deltas(dec.font, [AL.index(c) for c in text])]
    page = K.draw_at(MONO, 13.0, AL, text, pens, 150, LH)
    got = dec.refine_text([page], [[(0, read)]], 0, 146, LH, [[pens]])[0][0]
    assert got.text == text and got.changed == 2 and got.cost == -got.base and got.pens.tolist() == pens
    before = dec.score_text([page], [[(0, read)]], 0, 146, LH, pens=[[pens]])[0][0]
    after = dec.score_text([page], [[(0, got.text)]], 0, 146, LH, pens=[[got.pens]])[0][0]
    assert (before.base, before.cost, after.cost) == (got.base, got.cost_in, got.cost)
    drawn = dec.verify_text([page], [[(0, got.text)]], 0, pens=[[got.pens]], images=False)
    assert drawn is not None  # verify_text takes the outputs as they are


def test_the_sans_floored_page_is_read_whole(dec):
    """The page the call is for (tests/test_focr_refine_model.py has the table): DejaVu Sans 13 px, every pen floored to a pixel, the
    pen-slack reading `born clip ...` at N = 8: radius 4 and four sweeps read `burn clip ffH vvill rnrn c`."""
    from test_focr_slack_model import PAGES, snapped
    fms = setup(dec, SANS, 13.0, FOCR_DEFAULT_ALPHABET)
    line = snapped(SANS, *PAGES["floor"])
    s = K.slack_line(fms[0], line, 8)
    assert s.text == "born clip ffH vvill rnrn c"
    got = dec.refine_text([line], [[(0, s.text)]], 0, line.shape[1], line.shape[0], [[s.pens]])[0][0]
    assert (got.text, got.cost_in, got.cost, got.base) == ("burn clip ffH vvill rnrn c", -14445951, -15758225, 15779062)
    assert got.cost_in == s.cost and got.sweeps == 4


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def raw(dec, batch, x, width, lh, recs, chars, pens, radius=2, sweeps=1, glyphs=1, with_pens=True, chars_out=True, pens_out=True, out=True):
    """focr_decoder_refine_text as it is: recs are (page, y, first, n_chars, font).  Returns (rc, results, chars_out, pens_out)."""
    n, H, W = batch.shape
    larr = (N.TextLine * max(1, len(recs)))(*recs)
    carr = np.asarray(chars, dtype=np.uint16) if len(chars) else np.zeros(1, dtype=np.uint16)
    parr = np.asarray(pens, dtype=np.uint32) if len(pens) else np.zeros(1, dtype=np.uint32)
    n_out = max(1, sum(r[3] for r in recs if r[3] < 1 << 20))
    co, po = np.full(n_out, 7, dtype=np.uint16), np.full(n_out, 7, dtype=np.uint32)
    rarr = (N.TextRefineStruct * max(1, len(recs)))()
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = dec._lib.focr_decoder_refine_text(dec._h, ptr(batch), 0, n, W, H, x, width, lh, larr, len(recs), ptr(carr), ptr(parr) if with_pens else None, len(chars),
                                           radius, sweeps, glyphs, ptr(co) if chars_out else None, ptr(po) if pens_out else None, rarr if out else None)
    return rc, [(a.line_base, a.cost_in, a.cost, a.sweeps_run, a.changed) for a in rarr][: len(recs)], co, po


def test_refusals(dec):
    """Every refusal of include/focr_decode.h, each with its own words and nothing launched or written; the decoder refines afterwards."""
    lib, h = dec._lib, dec._h
    batch = np.ascontiguousarray(np.stack([noisy(80, 20, 31), noisy(80, 20, 32)]))
    with LineDecoder(0) as bare:  # no decode font
        rc = raw(bare, batch, 0, 80, LH, [], [], [])[0]
        assert rc != 0 and b"focr_decoder_refine_text: no decode font (focr_decoder_set_font)" in bare._lib.focr_decoder_last_error(bare._h)
        assert launches(bare) == 0
    fms = setup(dec, MONO, 13.0, AL, [(SANS, 13.0)])
    chars, pens = [AL.index(c) for c in "ahoi"], [0, 300, 300, 900]
    good = [(0, 2, 0, 4, 0), (1, 2, 0, 4, 1)]
    seen = set()

    def refused(*words, **kw):
        args = dict(x=1, width=70, lh=LH, recs=good, chars=chars, pens=pens)
        args.update(kw)
        assert raw(dec, batch, 1, 70, LH, good, chars, pens)[0] == 0 and launches(dec) == 1
        rc, _, co, po = raw(dec, batch, **args)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and msg.startswith("focr_decoder_refine_text: ") and all(w in msg for w in words), msg
        assert launches(dec) == 0 and lib.focr_decoder_last_refine_text_ms(h) == 0.0 and (co == 7).all() and (po == 7).all() and msg not in seen
        seen.add(msg)

    refused("width 0", width=0)
    refused("line_height 0", lh=0)
    refused("radius", "64", radius=65)
    refused("8 sweeps", sweeps=9)
    refused("line 1", "font 2", "1 candidates", recs=[good[0], (1, 2, 0, 4, 2)])
    refused("line 1", "page 2 of 2", recs=[good[0], (2, 2, 0, 4, 0)])
    refused("line 0", "n_chars", recs=[(0, 2, 1, 4, 0)])
    refused("character 2", "alphabet", chars=[0, 1, len(AL), 2])
    refused("pen 3", "2^24", pens=[0, 1, 2, 1 << 24])
    refused("line 0", "character 3", "do not decrease", pens=[0, 300, 300, 299])
    refused("line 1", "character 1", "do not decrease", recs=[(0, 2, 0, 2, 0), (1, 2, 2, 2, 1)], pens=[0, 300, 300, 299])
    refused("null pens", with_pens=False)
    refused("null chars_out", chars_out=False)
    refused("null pens_out", pens_out=False)
    refused("null out", out=False)
    cand = dec._candidates[0]  # origins: built fonts have whole ones, so bend a copy of the candidate's struct
    keep = cand.s.origin_x
    for ox in (0.5, -1.0):
        cand.s.origin_x = ox
        assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
        rc, _, co, _ = raw(dec, batch, 1, 70, LH, good, chars, pens)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and all(w in msg for w in ("line 1", "origin_x", "whole number")) and launches(dec) == 0 and (co == 7).all(), msg
        assert raw(dec, batch, 1, 70, LH, good[:1], chars, pens)[0] == 0  # font 0 alone is not touched by it
    cand.s.origin_x = keep
    assert lib.focr_decoder_set_font_candidates(h, (N.DecodeFontStruct * 1)(cand.s), 1) == 0
    larr, carr, parr = (N.TextLine * 2)(*good), np.asarray(chars, dtype=np.uint16), np.asarray(pens, dtype=np.uint32)
    out, co, po = (N.TextRefineStruct * 2)(), np.zeros(8, dtype=np.uint16), np.zeros(8, dtype=np.uint32)
    f = lib.focr_decoder_refine_text
    tail = (parr.ctypes.data, 4, 2, 1, 1, co.ctypes.data, po.ctypes.data, out)
    for words, call in (("null pages", lambda: f(h, None, 0, 2, 80, 20, 1, 70, LH, larr, 2, carr.ctypes.data, *tail)),
                        ("null lines", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, None, 2, carr.ctypes.data, *tail)),
                        ("null chars", lambda: f(h, batch.ctypes.data, 0, 2, 80, 20, 1, 70, LH, larr, 2, None, *tail)),
                        ("page too large", lambda: f(h, batch.ctypes.data, 0, 2, 0xffff * 16 + 1, 20, 1, 70, LH, larr, 0, carr.ctypes.data, *tail))):
        assert raw(dec, batch, 1, 70, LH, good, chars, pens)[0] == 0 and launches(dec) == 1
        assert call() != 0
        msg = lib.focr_decoder_last_error(h).decode()
        assert msg.startswith("focr_decoder_refine_text: ") and words in msg and launches(dec) == 0 and msg not in seen
        seen.add(msg)
    # usable afterwards
    check(dec, fms, list(batch), [[(2, "ahoi")], [(2, "ahoi")]], 1, 70, LH, [[pens], [pens]], fonts=[[0], [1]], radius=2, sweeps=1)
    for kw, words in ((dict(radius=65), "radius must be"), (dict(sweeps=9), "sweeps must be")):
        with pytest.raises(ValueError, match=words):
            dec.refine_text(list(batch), [[(2, "ahoi")], []], 1, 70, LH, [[pens], []], **kw)
    with pytest.raises(ValueError, match="needs pens"):
        dec.refine_text(list(batch), [[(2, "ahoi")], []], 1, 70, LH, None)
    with pytest.raises(ValueError, match="not in the alphabet"):
        dec.refine_text(list(batch), [[(2, "ahoy")], []], 1, 70, LH, [[pens], []])


# ---- the last run, memory -------------------------------------------------------------------------------------------------------

def test_a_decode_before_the_call_answers_the_same_afterwards(dec):
    """A whole-line decode, then refine_text of its own reading in the LDS and the global-strip form: the run's getters, timings and
    verify, and the other text calls' last timings, answer afterwards as they did before.  A plain reading goes in by placed_pens."""
    setup(dec, SANS, 13.0, AL)
    pages = [S.draw_text(dec.font, "Hinein bin ihr", 150, LH), S.draw_text(dec.font, "mohr ahoi", 150, LH, shift64=9)]
    plain = dec.decode(pages, 0, 0, 146, LH, LH)
    placed = [[placed_pens(dec.font, t) for _, t in pg] for pg in plain]
    scored = dec.score_text(pages, plain, 0, 146, LH)
    assert [[s.cost for s in pg] for pg in dec.score_text(pages, plain, 0, 146, LH, pens=placed)] == [[s.cost for s in pg] for pg in scored]
    lines, pens, costs = dec.decode(pages, 0, 0, 146, LH, LH, whole_line=True)
    dec.score_text(pages, lines, 0, 146, LH, pens=pens)
    dec.verify_text(pages, lines, 0, pens=pens)
    dec.align_text(pages, lines, 0, 146, LH, drift=2)
    lib, h = dec._lib, dec._h
    timings = lambda: (lib.focr_decoder_last_score_text_ms(h), lib.focr_decoder_last_score_text_launches(h),  # noqa: E731
                       lib.focr_decoder_last_verify_text_ms(h), lib.focr_decoder_last_verify_text_launches(h),
                       lib.focr_decoder_last_align_text_ms(h), lib.focr_decoder_last_align_text_launches(h))
    before, tb = snapshot(dec), timings()
    got = dec.refine_text(pages, lines, 0, 146, LH, pens)
    assert launches(dec) == 1 and lib.focr_decoder_last_refine_text_ms(h) > 0 and dec.last_refine_text_ms > 0
    for p in range(2):
        for r, (_, t) in zip(got[p], lines[p]):
            assert r.cost <= r.cost_in and len(r.text) == len(t)
    dec.refine_text([noisy(4100, 17, 5)], [[(0, "Hm")]], 0, 4100, 16, [[[0, 700]]])
    assert launches(dec) == 2
    assert snapshot(dec) == before and timings() == tb


def test_memory_returns():
    """A decoder that only ever called refine_text, with strips in LDS and in global memory, gives every device byte back."""
    before = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, AL)
        d.set_font_candidates([(SANS, 13.0, False, 1.0)])
        up = N.hip().focr_debug_device_bytes()
        d.refine_text([noisy(257, 33, 41)], [[(0, "ahoi"), (12, "Hob in")]], 2, 250, LH, [[spaced(4, 300), spaced(6, 200)]], fonts=[[0, 1]])
        small = N.hip().focr_debug_device_bytes()
        d.refine_text([noisy(4100, 17, 42)], [[(0, "ahoi")]], 0, 4100, 16, [[[0, 500, 1000, 1500]]], sweeps=1)
        assert launches(d) == 2
        peak = N.hip().focr_debug_device_bytes()
        assert before < up < small < peak
        assert d._lib.focr_decoder_n_lines(d._h) == 0  # no run was ever made
    assert N.hip().focr_debug_device_bytes() == before


def test_cli_refine(dec, tmp_path):
    """focr --refine S [--refine-radius N] after a pen-slack run, a plain run and a pen search: stdout carries refine_text's text of the
    run's own reading at the run's own pens, stderr says what changed; without --refine stdout is the run's; the usage errors."""
    from test_focr_slack_model import PAGES, snapped
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(os.path.dirname(os.path.dirname(FOCR)), "csrc"), "cli"], check=True)
    line = snapped(SANS, *PAGES["floor"])
    h, w = line.shape
    path = str(tmp_path / "page.pgm")
    save_pgm(path, line)
    cmd = [FOCR, "-f", SANS, "-t", "13", "-w", str(w), "--line-height", str(h), "--line-advance", str(h), "-i", path]
    dec.set_font(SANS, 13.0, FOCR_DEFAULT_ALPHABET)
    dec.set_font_candidates([])
    for flags, kw in ((["--whole-line", "--pen-slack", "8"], dict(whole_line=True, pen_slack=8)), ([], {}), (["--pen-search", "4"], dict(pen_search=4))):
        run = dec.decode([line], 0, 0, w, h, h, **kw)
        lines = run[0] if kw else run
        if "whole_line" in kw:
            pens = run[1]
        else:
            pens = [[placed_pens(dec.font, t, run[1][0][q] if kw else None) for q, (_, t) in enumerate(lines[0])]]
        radius = 4 if kw.get("pen_slack") else 3  # 4 is the default
        want = dec.refine_text([line], lines, 0, w, h, pens, radius=radius, sweeps=4)[0]
        if kw.get("pen_slack"):
            plain = subprocess.run(cmd + flags, capture_output=True, text=True, timeout=300)
            assert plain.returncode == 0 and plain.stdout == "born clip ffH vvill rnrn c\n" == lines[0][0][1] + "\n" and plain.stderr == ""
        r = subprocess.run(cmd + flags + ["--refine", "4"] + ([] if radius == 4 else ["--refine-radius", "3"]), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "".join(g.text + "\n" for g in want)
        n_lines = sum(g.changed != 0 for g in want)
        assert r.stderr == "refine: %d characters in %d of %d lines changed\n" % (sum(g.changed for g in want), n_lines, len(want))
        if kw.get("pen_slack"):
            assert r.stdout == "burn clip ffH vvill rnrn c\n"  # the table's first row
    for extra, words in ((["--refine", "2", "--baseline-search", "1"], "--baseline-search"), (["--refine", "2", "--whole-line", "--whole-baseline", "1"], "--whole-baseline"),
                         (["--refine", "2", "--font-candidate", "t=12"], "--font-candidate"), (["--refine", "9"], "8 sweeps"),
                         (["--refine", "1", "--refine-radius", "65"], "64"), (["--refine-radius", "2"], "--refine <S>")):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and words in r.stderr and "--refine" in r.stderr and r.stdout == "", (extra, r.stderr)

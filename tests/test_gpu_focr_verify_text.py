"""focr_decoder_verify_text (verify_layout_text_kernel, verify_compose_text_kernel, focr_decoder_set_verify_font_candidates,
LineDecoder.verify_text, focr --verify-fonts): a caller's lines drawn over their pages, each in any uploaded font.  Against the
existing verify where both can draw (byte for byte), and against tests/focr_verify_text_model.py, which rasterises every line
with FreeType in the line's own font.  Every image and sum comparison is ==.  Pages are at most 520 by 40 px."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import focr_verify_text_model as M
from font_ocr_amd import DecodeFont, LineDecoder, VerifyFont, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO, SANS, SERIF = (os.path.join(GOLD, f) for f in ("DejaVuSansMono.ttf", "DejaVuSans.ttf", "DejaVuSerif.ttf"))
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
AL = "abehinor HIm"
AL_V = "abehinor HIv"  # Serif's v reaches left of the pen
LH = 18
MONO13, SANS20, SERIF13 = (MONO, 13.0, False, 1.0), (SANS, 20.0, False, 1.0), (SERIF, 13.0, False, 1.0)
# fourteen fonts between the decode font and the last candidate of the K = 15 case
FILL = [(MONO, 12.0, False, 1.0), (MONO, 14.0, False, 1.0), (MONO, 13.0, True, 1.0), (MONO, 13.0, False, 1.05), (SANS, 13.0, False, 1.0),
        (SERIF, 13.0, False, 1.0), (MONO, 12.5, False, 1.0), (MONO, 11.0, False, 1.0), (MONO, 11.5, False, 1.0), (MONO, 13.5, False, 1.0),
        (MONO, 12.0, True, 1.0), (MONO, 13.0, False, 0.95), (SANS, 12.0, False, 1.0), (SERIF, 12.0, True, 1.0)]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def setup(dec, specs, alphabet=AL):
    """The decode font specs[0] and the candidates specs[1:], through the Python API (which forgets its verify tables)."""
    f, t, h, k = specs[0]
    dec.set_font(f, t, alphabet, h, k)
    dec.set_font_candidates([(f, t, h, k) for f, t, h, k in specs[1:]])
    return [M.Font(*s) for s in specs]


def noisy(W, H, seed):
    """A page without a white pixel: every pixel has red, so that every blue pixel and every missing one moves the sum."""
    return np.random.default_rng(seed).integers(0, 255, (H, W)).astype(np.uint8)


def launches(dec):
    return dec._lib.focr_decoder_last_verify_text_launches(dec._h)


def check(dec, pages, lines, fonts_of, x, alphabet=AL, fonts=None, pens=None, offsets=None):
    """verify_text equals the model, page by page: images and sums; two launches."""
    sums, imgs = dec.verify_text(pages, lines, x, fonts=fonts, pens=pens, offsets=offsets)
    assert launches(dec) == 2 and sums.dtype == np.uint64
    for p, page in enumerate(pages):
        ml = [M.Line(y, t, fonts[p][q] if fonts is not None else 0, None if pens is None else pens[p][q], None if offsets is None else offsets[p][q])
              for q, (y, t) in enumerate(lines[p])]
        want, sq = M.verify_text(np.asarray(page), ml, fonts_of, alphabet, x)
        assert np.array_equal(imgs[p], want), (p, np.argwhere(imgs[p] != want)[:4])
        assert int(sums[p]) == sq
    return sums, imgs


def raw(dec, pages, x, recs, chars, pens=None, offsets=None, rgb=True, n_chars=None):
    """focr_decoder_verify_text as it is: recs are (page, y, first, n_chars, font).  Returns (rc, sums, images)."""
    batch = np.ascontiguousarray(np.stack(pages))
    n, H, W = batch.shape
    larr = (N.TextLine * max(1, len(recs)))(*recs)
    carr = np.asarray(chars, dtype=np.uint16) if len(chars) else np.zeros(1, dtype=np.uint16)
    parr = None if pens is None else np.asarray(pens, dtype=np.uint32)
    oarr = None if offsets is None else np.asarray(offsets, dtype=np.int8)
    sums = np.full(n, 7, dtype=np.uint64)
    out = np.zeros((n, H, W, 3), dtype=np.uint8) if rgb else None
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = dec._lib.focr_decoder_verify_text(dec._h, ptr(batch), 0, n, W, H, x, larr, len(recs), ptr(carr), ptr(parr), ptr(oarr),
                                           len(chars) if n_chars is None else n_chars, ptr(out), 0, sums.ctypes.data)
    return rc, sums, out


# ---- equivalence with focr_decoder_verify ----------------------------------------------------------------------------------

def snapshot(dec):
    """What the last run's getters, timing and verify answer."""
    lib, h = dec._lib, dec._h
    nl, nc = lib.focr_decoder_n_lines(h), lib.focr_decoder_n_chars(h)
    lines = (N.DecodedLine * max(1, nl))()
    chars, offs, pens = np.zeros(max(1, nc), dtype=np.uint16), np.zeros(max(1, nc), dtype=np.int8), np.zeros(max(1, nc), dtype=np.uint32)
    assert lib.focr_decoder_get(h, lines, chars.ctypes.data) == 0 and lib.focr_decoder_get_offsets(h, offs.ctypes.data) == 0
    have_pens = lib.focr_decoder_get_pens(h, pens.ctypes.data, None) == 0
    sums, imgs = dec.verify()
    return (nl, nc, bytes(lines), chars.tobytes(), offs.tobytes(), have_pens, pens.tobytes(), lib.focr_decoder_last_launches(h), lib.focr_decoder_last_ms(h),
            lib.focr_decoder_last_verify_launches(h), sums.tobytes(), imgs.tobytes())


@pytest.mark.parametrize("mode", ["plain", "pen_search", "whole_line", "pen_slack"])
def test_equals_the_existing_verify(dec, mode):
    """After a plain run, a pen-search run, a whole-line run and a pen-slack run: focr_decoder_get's lines, passed unchanged
    (font 0), and the run's offsets or pens give focr_decoder_verify's images and sums byte for byte; afterwards the last
    run's getters, timing and verify answer as before."""
    fonts_of = setup(dec, [MONO13])
    x, W, H = 2, 150, 2 * LH + 2
    texts = [[M.Line(0, "Hinein bin ich", 0), M.Line(LH, "mohr ahoi ab", 0)], [M.Line(LH, "bahn in rom", 0)]]
    pages = []
    for pl in texts:
        page = M.draw_lines(np.full((H, W), 255, dtype=np.uint8), pl, fonts_of, x)
        page[::3, 0] = 90  # ink left of every crop, so that the sums are not zero
        pages.append(page)
    kw = {"plain": {}, "pen_search": dict(pen_search=4), "whole_line": dict(whole_line=True), "pen_slack": dict(whole_line=True, pen_slack=4)}[mode]
    res = dec.decode(pages, x, 0, W - 4, LH, LH, **kw)
    got = res if mode == "plain" else res[0]
    assert [len(pg) for pg in got] == [2, 1]
    lib, h = dec._lib, dec._h
    before = snapshot(dec)
    nl, nc = before[0], before[1]
    lines = (N.DecodedLine * nl)()
    chars, offs, pens = np.zeros(nc, dtype=np.uint16), np.zeros(nc, dtype=np.int8), np.zeros(nc, dtype=np.uint32)
    assert lib.focr_decoder_get(h, lines, chars.ctypes.data) == 0 and all(l.pad == 0 for l in lines)
    assert lib.focr_decoder_get_offsets(h, offs.ctypes.data) == 0
    if "whole_line" in kw:
        assert lib.focr_decoder_get_pens(h, pens.ctypes.data, None) == 0
    batch = np.ascontiguousarray(np.stack(pages))
    sums, out = np.zeros(2, dtype=np.uint64), np.zeros((2, H, W, 3), dtype=np.uint8)
    rc = lib.focr_decoder_verify_text(h, batch.ctypes.data, 0, 2, W, H, x, lines, nl, chars.ctypes.data,
                                      pens.ctypes.data if "whole_line" in kw else None, offs.ctypes.data if mode == "pen_search" else None, nc,
                                      out.ctypes.data, 0, sums.ctypes.data)
    assert rc == 0, lib.focr_decoder_last_error(h)
    assert launches(dec) == 2
    assert sums.tobytes() == before[-2] and out.tobytes() == before[-1] and sums.min() > 0
    assert snapshot(dec) == before


# ---- mixed fonts against the model -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 15])
@pytest.mark.parametrize("whole", [False, True])
def test_font_search_result_round_trips(dec, K, whole):
    """A font-search run's result in both forms, the pen loop's and the whole-line decode's with its pens, drawn by verify_text
    and by the model: a Sans 20 px line won by the decode font and a Mono 13 px line won by the last candidate, so the canvases
    differ in height.  Under the pen loop the page is reproduced (the sum is 0: its pens are render()'s); the whole-line
    decode's pens are whole 1/64 px, so there a residue stays, below what the decode font alone leaves."""
    specs = [SANS20] + FILL[:K - 1] + [MONO13]
    fonts_of = setup(dec, specs)
    drawn = [M.Line(0, "Hob in Hm", 0), M.Line(LH, "moheb in Hinein", K)]
    pages = [M.draw_lines(np.full((2 * LH + 2, 150), 255, dtype=np.uint8), drawn, fonts_of, 2)]
    if whole:
        lines, pens, _, fonts = dec.decode(pages, 2, 0, 146, LH, LH, whole_line=True, font_search=True)
    else:
        (lines, fonts, _), pens = dec.decode(pages, 2, 0, 146, LH, LH, font_search=True), None
    assert fonts == [[0, K]] and [t.rstrip() for _, t in lines[0]] == [l.text for l in drawn]
    with pytest.raises(DecoderError, match="searched fonts"):
        dec.verify()
    sums, _ = check(dec, pages, lines, fonts_of, 2, fonts=fonts, pens=pens)
    one, _ = check(dec, pages, lines, fonts_of, 2, pens=pens)  # every line in the decode font, as the existing verify would draw it
    assert (int(sums[0]) > 0 if whole else int(sums[0]) == 0) and int(sums[0]) < int(one[0])
    with pytest.raises(DecoderError, match="searched fonts"):  # the last run is still the font search
        dec.verify()


# ---- tile edges ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(255, 16), (256, 17), (257, 33), (513, 33)])
def test_tile_edges(dec, W, H):
    """Pages one column short of a tile, exactly one, one more, and two tiles and a column; one tile row, one more row, two
    and a row.  A 70-character line (two batches of layout_line) at y = 9 straddles the tile row at 16 and the tile columns at
    256 and 512 where the page has them; a Sans 20 px line starts on the last row of the first tile row."""
    fonts_of = setup(dec, [MONO13, SANS20])
    rng = np.random.default_rng(W * 100 + H)
    long_line = "".join(rng.choice(list("abehinorHIm"), 70))
    lines = [[(9, long_line), (15, "Hob in Hm im ohr"), (0, "mm")]]
    check(dec, [noisy(W, H, W + H)], lines, fonts_of, 3, fonts=[[0, 1, 1]])


# ---- layout and compose edges ----------------------------------------------------------------------------------------------

def test_layout_and_compose_edges(dec):
    """Three pages of 520 x 40 with lines only on the last: 64 and 65 characters (one and two batches), an empty line, two
    lines at the same y, a later line with a smaller y over an earlier one (list order decides), lines clipped at the right
    and bottom edges, y = page_h - 1 and y = page_h (nothing), and a Serif v, which reaches left of the pen."""
    fonts_of = setup(dec, [MONO13, SANS20, SERIF13], AL_V)
    W, H = 520, 40
    rng = np.random.default_rng(11)
    t64, t65 = ("".join(rng.choice(list("abehinorHIv"), n)) for n in (64, 65))
    lines = [[], [], [(0, t64), (13, t65), (20, ""), (22, "Hob in Hv"), (22, "vier bav"), (18, "Ihr vorn"), (26, t65 + t65), (H - 5, "bahn vor ohr"),
                      (H - 1, "Ihr"), (H, "Ihr"), (4, "vvv ahoi vvv")]]
    fonts = [[], [], [0, 0, 1, 1, 2, 1, 0, 1, 2, 0, 2]]
    pages = [noisy(W, H, s) for s in (1, 2, 3)]
    df = DecodeFont(*SERIF13[:2], AL_V)
    assert float(df.origin[0]) == 1.0  # Serif's v has ink left of its pen
    df.close()
    sums, imgs = check(dec, pages, lines, fonts_of, 3, AL_V, fonts=fonts)
    assert not imgs[0][..., 2].any() and not imgs[1][..., 2].any() and imgs[2][..., 2].any()
    assert imgs[2][:, W - 2:, 2].any() and imgs[2][H - 1, :, 2].any()  # ink reaches the right edge (but for a gap between glyphs) and the bottom one
    # list order decides: the same lines with the overlapping pair swapped give another image
    swapped = [[], [], lines[2][:4] + [lines[2][5], lines[2][4]] + lines[2][6:]]
    fswapped = [[], [], fonts[2][:4] + [fonts[2][5], fonts[2][4]] + fonts[2][6:]]
    _, other = check(dec, pages, swapped, fonts_of, 3, AL_V, fonts=fswapped)
    assert not np.array_equal(other[2], imgs[2])
    # pens and offsets in a candidate font
    df, _ = M.tables(fonts_of[1], AL_V)
    text = "Hob in Hv"
    idx = [AL_V.index(c) for c in text]
    pens64 = np.concatenate([[0], np.cumsum(np.rint(df.increments() * 64).astype(np.int64)[idx][:-1])]) + np.arange(len(idx)) * 7
    check(dec, pages[:1], [[(3, text), (20, text)]], fonts_of, 5, AL_V, fonts=[[1, 1]], pens=[[pens64, pens64[::-1].copy()]])
    check(dec, pages[:1], [[(3, text), (20, text)]], fonts_of, 5, AL_V, fonts=[[1, 2]], offsets=[[[0, 5, -3, 0, 9, -9, 0, 64, -64], [-20, 0, 0, 0, 0, 0, 0, 0, 0]]])


def test_no_lines_null_rgb_and_device_buffers(dec):
    """n_lines = 0 still draws the pages and sums them; rgb NULL gives the sums alone; pages and rgb in device memory give what
    host memory gives; two lines may share their characters."""
    fonts_of = setup(dec, [MONO13, SANS20])
    pages = [noisy(257, 17, 21), noisy(257, 17, 22)]
    rc, sums, out = raw(dec, pages, 0, [], [])
    assert rc == 0 and launches(dec) == 2
    red = np.stack(pages)
    red = np.where(red != 255, red, 0)
    assert np.array_equal(out[..., 0], red) and not out[..., 1:].any()
    assert list(sums) == [int((red[p].astype(np.int64) ** 2).sum()) for p in range(2)]
    dec.verify_text(pages, [[(0, "a")], []], 0, fonts=[[1], []])  # builds and uploads both verify tables
    dec._ensure_verify_font()
    chars = [AL.index(c) for c in "Hinein im ohr"]
    recs = [(0, 1, 0, len(chars), 0), (1, 2, 0, len(chars), 1), (1, 0, 3, 5, 0)]  # two lines share their characters, a third some of them
    rc, want_sums, want = raw(dec, pages, 4, recs, chars)
    assert rc == 0
    for p in range(2):
        ml = [M.Line(y, "".join(AL[c] for c in chars[first: first + n]), font) for page, y, first, n, font in recs if page == p]
        img, sq = M.verify_text(pages[p], ml, fonts_of, AL, 4)
        assert np.array_equal(want[p], img) and int(want_sums[p]) == sq
    rc, sums, none = raw(dec, pages, 4, recs, chars, rgb=False)
    assert rc == 0 and none is None and sums.tobytes() == want_sums.tobytes() and launches(dec) == 2
    hip = C.CDLL("libamdhip64.so.7")
    batch = np.ascontiguousarray(np.stack(pages))
    src, dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(batch.nbytes)) == 0
    try:
        assert hip.hipMalloc(C.byref(dst), C.c_size_t(batch.nbytes * 3)) == 0
        try:
            assert hip.hipMemcpy(src, C.c_void_p(batch.ctypes.data), C.c_size_t(batch.nbytes), 1) == 0  # host to device
            assert hip.hipDeviceSynchronize() == 0
            larr = (N.TextLine * len(recs))(*recs)
            carr = np.asarray(chars, dtype=np.uint16)
            sums = np.zeros(2, dtype=np.uint64)
            assert dec._lib.focr_decoder_verify_text(dec._h, src, 1, 2, 257, 17, 4, larr, len(recs), carr.ctypes.data, None, None, len(chars), dst, 1,
                                                     sums.ctypes.data) == 0
            got = np.empty_like(want)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), dst, C.c_size_t(got.nbytes), 2) == 0  # device to host
            assert np.array_equal(got, want) and sums.tobytes() == want_sums.tobytes()
        finally:
            hip.hipFree(dst)
    finally:
        hip.hipFree(src)


# ---- the staging verify_text shares with score_text ------------------------------------------------------------------------

def test_shared_staging_keeps_nothing_between_calls(dec):
    """verify_text and score_text stage their reading in one set of device arrays.  One handle draws with pens, costs the same
    lines with neither pens nor offsets, draws with offsets, costs a longer list (eight lines that share characters) and draws
    the first again: every answer (sums, image bytes, TextScores with their terms) is what a fresh decoder gives to that
    call alone, so no call reads an earlier call's pens or offsets, or arrays of an earlier call's size."""
    setup(dec, [MONO13, SANS20])
    pages = [noisy(80, 20, 31), noisy(80, 20, 32)]
    batch = np.ascontiguousarray(np.stack(pages))
    lines, fonts = [[(2, "ahoi")], [(2, "ahoi")]], [[0], [1]]
    pens, offs = [[[0, 500, 1000, 1500]]] * 2, [[[3, -5, 0, 64]], [[-64, 0, 7, 1]]]
    chars = [AL.index(c) for c in "Hinein im ohr ab"]
    recs = [(0, 0, 0, 16, 0), (0, 2, 0, 16, 1), (0, 4, 3, 9, 0), (1, 1, 3, 9, 1), (1, 1, 8, 8, 0), (1, 3, 15, 1, 1), (1, 5, 16, 0, 0), (1, 6, 0, 6, 1)]

    def drawn(got):
        return got[0].tobytes(), [img.tobytes() for img in got[1]]

    def costs(got):
        return [(s.base, s.cost, s.shift, s.terms.tobytes()) for s in got]

    calls = [lambda d: drawn(d.verify_text(pages, lines, 1, fonts=fonts, pens=pens)),
             lambda d: costs(sum(d.score_text(pages, lines, 1, 70, LH, fonts=fonts, shift=2), [])),
             lambda d: drawn(d.verify_text(pages, lines, 1, fonts=fonts, offsets=offs)),
             lambda d: costs(d._score_text(batch, recs, chars, None, None, None, 1, 70, LH, 0, 2, True))]
    calls.append(calls[0])
    want = []
    for call in calls[:4]:
        with LineDecoder(0) as fresh:
            fresh.set_font(dec.font, None)
            fresh.set_font_candidates(dec._candidates)
            want.append(call(fresh))
    want.append(want[0])
    assert len({repr(w) for w in want}) == 4  # pens, offsets and the longer list each change the answer
    assert [call(dec) for call in calls] == want


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals(dec):
    """Every refusal of include/focr_decode.h, each with its own words and nothing launched; the decoder draws afterwards."""
    lib, h = dec._lib, dec._h
    with LineDecoder(0) as bare:  # no decode font
        rc, _, _ = raw(bare, [noisy(40, 16, 1)], 0, [], [])
        assert rc != 0 and b"focr_decoder_verify_text: no decode font (focr_decoder_set_font)" in bare._lib.focr_decoder_last_error(bare._h)
        assert launches(bare) == 0
    fonts_of = setup(dec, [MONO13, SANS20])
    pages = [noisy(80, 20, 31), noisy(80, 20, 32)]
    chars = [AL.index(c) for c in "ahoi"]
    good = [(0, 2, 0, 4, 0), (1, 2, 0, 4, 1)]
    seen = set()

    def refused(*words, again=False, **kw):
        args = dict(recs=good, chars=chars)
        args.update(kw)
        rc, sums, _ = raw(dec, pages, 1, **args)
        msg = lib.focr_decoder_last_error(h).decode()
        assert rc != 0 and msg.startswith("focr_decoder_verify_text: ") and all(w in msg for w in words), msg
        assert launches(dec) == 0 and list(sums) == [7, 7] and (again or msg not in seen)
        seen.add(msg)

    # no verify tables yet: the message names the setter to call
    refused("font 0", "focr_decoder_set_verify_font)")
    dec._ensure_verify_font()
    refused("candidate font", "focr_decoder_set_verify_font_candidates")
    dec._ensure_verify_candidates()
    assert raw(dec, pages, 1, good, chars)[0] == 0 and launches(dec) == 2
    refused("line 1", "font 2", recs=[good[0], (1, 2, 0, 4, 2)])
    refused("line 1", "page 2 of 2", recs=[good[0], (2, 2, 0, 4, 0)])
    refused("line 1", "page order", recs=[good[1], good[0]])
    refused("line 0", "n_chars", recs=[(0, 2, 1, 4, 0)])
    refused("line 0", "n_chars", again=True, recs=[(0, 2, 2 ** 63, 2 ** 32 - 1, 0)])
    refused("character 2", "alphabet", chars=[0, 1, len(AL), 2])
    refused("pen 3", "2^24", pens=[0, 500, 1000, 1 << 24])
    refused("pens and offsets", pens=[0, 500, 1000, 1500], offsets=[0, 0, 0, 0])
    batch = np.ascontiguousarray(np.stack(pages))
    larr, carr, sums = (N.TextLine * 2)(*good), np.asarray(chars, dtype=np.uint16), np.full(2, 7, dtype=np.uint64)
    for words, call in (("null pages", lambda: lib.focr_decoder_verify_text(h, None, 0, 2, 80, 20, 1, larr, 2, carr.ctypes.data, None, None, 4, None, 0, sums.ctypes.data)),
                        ("null lines", lambda: lib.focr_decoder_verify_text(h, batch.ctypes.data, 0, 2, 80, 20, 1, None, 2, carr.ctypes.data, None, None, 4, None, 0, sums.ctypes.data)),
                        ("null chars", lambda: lib.focr_decoder_verify_text(h, batch.ctypes.data, 0, 2, 80, 20, 1, larr, 2, None, None, None, 4, None, 0, sums.ctypes.data)),
                        ("null sq_sums", lambda: lib.focr_decoder_verify_text(h, batch.ctypes.data, 0, 2, 80, 20, 1, larr, 2, carr.ctypes.data, None, None, 4, None, 0, None)),
                        ("page too large", lambda: lib.focr_decoder_verify_text(h, batch.ctypes.data, 0, 2, 0xffff * 16 + 1, 20, 1, larr, 0, carr.ctypes.data, None, None, 4, None, 0, sums.ctypes.data))):
        assert raw(dec, pages, 1, good, chars)[0] == 0 and launches(dec) == 2
        assert call() != 0
        msg = lib.focr_decoder_last_error(h).decode()
        assert msg.startswith("focr_decoder_verify_text: ") and words in msg and launches(dec) == 0 and list(sums) == [7, 7] and msg not in seen
        seen.add(msg)
    # the candidates' tables: refused unless there is one per candidate and each matches; a failed upload drops them
    vf0, vf1, other = VerifyFont(*MONO13[:2], AL), VerifyFont(*SANS20[:2], AL), VerifyFont(SANS, 19.0, AL)
    bent = VerifyFont(*SANS20[:2], AL)
    bent.s.glyphs[3].rect_w[5] = 10000
    for arr, n, words in (((N.VerifyFontStruct * 2)(vf1.s, vf1.s), 2, b"one table per uploaded candidate"), ((N.VerifyFontStruct * 1)(other.s), 1, b"does not match the candidate"),
                          ((N.VerifyFontStruct * 1)(vf0.s), 1, b"does not match the candidate"), ((N.VerifyFontStruct * 1)(bent.s), 1, b"phase rectangle leaves the candidate's box"),
                          (None, 0, b"bad arguments")):
        assert lib.focr_decoder_set_verify_font_candidates(h, (N.VerifyFontStruct * 1)(vf1.s), 1) == 0
        assert raw(dec, pages, 1, good, chars)[0] == 0
        assert lib.focr_decoder_set_verify_font_candidates(h, arr, n) != 0
        msg = lib.focr_decoder_last_error(h)
        assert msg.startswith(b"focr_decoder_set_verify_font_candidates: ") and words in msg, msg
        rc, _, _ = raw(dec, pages, 1, good, chars)
        assert rc != 0 and b"focr_decoder_set_verify_font_candidates" in lib.focr_decoder_last_error(h) and launches(dec) == 0
        assert raw(dec, pages, 1, good[:1], chars)[0] == 0  # the decode font's table stands
    # ... and so do focr_decoder_set_font_candidates and focr_decoder_set_font
    cand = DecodeFont(*SANS20[:2], AL)
    carr1 = (N.DecodeFontStruct * 1)(cand.s)
    assert lib.focr_decoder_set_verify_font_candidates(h, (N.VerifyFontStruct * 1)(vf1.s), 1) == 0 and raw(dec, pages, 1, good, chars)[0] == 0
    assert lib.focr_decoder_set_font_candidates(h, carr1, 1) == 0
    rc, _, _ = raw(dec, pages, 1, good, chars)
    assert rc != 0 and b"focr_decoder_set_verify_font_candidates" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_verify_font_candidates(h, (N.VerifyFontStruct * 1)(vf1.s), 1) == 0 and raw(dec, pages, 1, good, chars)[0] == 0
    assert lib.focr_decoder_set_font(h, C.byref(dec.font.s)) == 0
    assert lib.focr_decoder_set_verify_font_candidates(h, (N.VerifyFontStruct * 1)(vf1.s), 1) != 0  # no candidates to match
    assert lib.focr_decoder_set_font_candidates(h, carr1, 1) == 0
    rc, _, _ = raw(dec, pages, 1, good[1:], chars)
    assert rc != 0 and b"focr_decoder_set_verify_font_candidates" in lib.focr_decoder_last_error(h)
    for f in (vf0, vf1, other, bent, cand):
        f.close()
    # usable afterwards, through the Python API from scratch
    fonts_of = setup(dec, [MONO13, SANS20])
    check(dec, pages, [[(2, "ahoi")], [(2, "ahoi")]], fonts_of, 1, fonts=[[0], [1]])
    with pytest.raises(ValueError, match="not in the alphabet"):
        dec.verify_text(pages, [[(2, "ahoy")], []], 1)


# ---- memory ----------------------------------------------------------------------------------------------------------------

def test_memory_returns():
    """A decoder that uploaded candidates and their verify tables and drew text gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    pages = [noisy(257, 33, 41)]
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, AL)
        d.set_font_candidates([SANS20])
        up = N.hip().focr_debug_device_bytes()
        d.verify_text(pages, [[(0, "ahoi"), (12, "Hob in")]], 2, fonts=[[0, 1]])
        drawn = N.hip().focr_debug_device_bytes()
        d.verify_text(pages, [[(0, "ahoi")]], 2, pens=[[[0, 500, 1000, 1500]]], images=False)
        peak = N.hip().focr_debug_device_bytes()
        assert before < up < drawn <= peak
        d.set_font_candidates([])
        assert N.hip().focr_debug_device_bytes() < peak  # the candidates' verify tables went with them
    assert N.hip().focr_debug_device_bytes() == before


# ---- CLI -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("whole", [False, True])
def test_cli(dec, tmp_path, whole):
    """focr --font-candidate ... --verify-fonts DIR writes the PNGs that LineDecoder.verify_text draws of the same run, and
    prints f32(sum) / f32(W * H) per page on stderr; stdout is the run's without it."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    specs = [MONO13, (MONO, 12.0, False, 1.0), SANS20]
    fonts_of = setup(dec, specs)
    pages, paths = [], []
    for p, drawn in enumerate(([M.Line(0, "Hinein ahoi", 2), M.Line(LH, "moheb in rom", 1)], [M.Line(LH, "bahn mehr Hi", 0)])):
        page = M.draw_lines(np.full((2 * LH + 2, 150), 255, dtype=np.uint8), drawn, fonts_of, 2)
        page[::4, 149] = 60  # ink right of every crop: the MSEs are not zero
        pages.append(page)
        paths.append(str(tmp_path / f"page{p}.pgm"))
        save_pgm(paths[-1], page)
    vdir = tmp_path / "out"
    vdir.mkdir()
    kw = dict(whole_line=True) if whole else {}
    res = dec.decode(pages, 2, 0, 146, LH, LH, font_search=True, **kw)
    lines, fonts, pens = (res[0], res[3], res[1]) if whole else (res[0], res[1], None)
    assert fonts == [[2, 1], [0]]
    sums, imgs = dec.verify_text(pages, lines, 2, fonts=fonts, pens=pens)
    cmd = [FOCR, "-f", MONO, "-t", "13", "-a", AL, "-x", "2", "-y", "0", "-w", "146", "--line-height", str(LH), "--line-advance", str(LH),
           "--font-candidate", "t=12", "--font-candidate", "f=%s,t=20" % SANS] + (["--whole-line"] if whole else [])
    r = subprocess.run(cmd + ["--verify-fonts", str(vdir), "-i"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run(cmd + ["-i"] + paths, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and plain.stderr == "" and r.stdout == plain.stdout == "".join(t + "\n" for pg in lines for _, t in pg)
    for p, path in enumerate(paths):
        got = np.asarray(Image.open(str(vdir / f"page{p}.png")).convert("RGB"))
        assert np.array_equal(got, imgs[p]), path
    mse = sums.astype(np.float32) / np.float32(150 * (2 * LH + 2))
    assert r.stderr.splitlines() == [f"{path} {float(m):.6f}" for path, m in zip(paths, mse)] and sums.min() > 0

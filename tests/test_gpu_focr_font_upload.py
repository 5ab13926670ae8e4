"""The five font uploaders of the focr decoder (focr_decoder_set_font, _set_baseline_fonts, _set_font_candidates,
_set_verify_font, _set_verify_font_candidates; csrc/hip/decode_font.h holds what they share), through the C ABI.

First the refusals, each with the full text of focr_decoder_last_error: the strings below are literals copied from the source
as it stood before the uploaders shared one packer, and that part of this file passed unmodified on that source.  Then the
decoder's state after a refusal, and one round trip: after the five uploads every mode that reads the tables gives exactly what
its model in tests/ gives.  The tables are those of a 4-glyph alphabet at 8 and 9 px, bent in place and put back."""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest

import focr_baseline_model as B
import focr_fonts_model as FM
import focr_score_text_model as S
import focr_verify_text_model as M
from focr_fast_model import FastModel
from font_ocr_amd import DecodeFont, LineDecoder
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import VerifyFont

pytestmark = pytest.mark.gpu

MONO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "DejaVuSansMono.ttf")
AL = "anH "  # the last glyph has no ink
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def fonts():
    """The decode font with its two y-phases, two candidates, and the verify tables of all three."""
    f = {"font": DecodeFont(MONO, 8.0, AL, y_bits=1), "cands": [DecodeFont(MONO, 9.0, AL), DecodeFont(MONO, 8.0, AL, hinting=True)],
         "vfont": VerifyFont(MONO, 8.0, AL), "vcands": [VerifyFont(MONO, 9.0, AL), VerifyFont(MONO, 8.0, AL, hinting=True)]}
    yield f
    for x in [f["font"], f["vfont"]] + f["cands"] + f["vcands"]:
        x.close()


@pytest.fixture()
def dec():
    with LineDecoder(0) as d:
        yield d


@contextlib.contextmanager
def bent(*bends):
    """Every (struct, field, value), (struct, field, index, value) or (array, index, value) set, and put back on the way out."""
    undo = []
    try:
        for obj, field, *at, value in bends:
            if at:
                obj, field = getattr(obj, field), at[0]
            old = obj[field] if isinstance(field, int) else getattr(obj, field)
            if isinstance(old, C._Pointer):  # a pointer field reads as a view of the struct's own bytes: keep a copy
                old = type(old).from_buffer_copy(old)
            undo.append((obj, field, old))
            if isinstance(field, int):
                obj[field] = value
            else:
                setattr(obj, field, value)
        yield
    finally:
        for obj, field, old in reversed(undo):
            if isinstance(field, int):
                obj[field] = old
            else:
                setattr(obj, field, old)


def refused(dec, rc, text):
    assert rc != 0
    assert dec._lib.focr_decoder_last_error(dec._h).decode() == text


def array_of(kind, structs):
    arr = (kind * max(1, len(structs)))()
    for i, s in enumerate(structs):
        arr[i] = s  # by value: the tables stay their owner's
    return arr


def glyph_faults(g, bitmaps_len):
    """(bends of one decode glyph, is it the increment's fault): the tables every decode-font uploader refuses."""
    phase = g.stride * g.box_h
    assert phase > 0 and g.stride % 4 == 0 and bitmaps_len >= 64 * phase
    return [([(g, "increment", 0.0)], True), ([(g, "increment", -1.0)], True), ([(g, "increment", NAN)], True),
            ([(g, "stride", g.stride + 1)], False), ([(g, "box_w", g.stride + 4)], False), ([(g, "offset", g.offset + 2)], False),
            ([(g, "offset", bitmaps_len - 63 * phase)], False),  # its last phase ends one phase past the table
            ([(g, "stride", 8), (g, "box_w", 8), (g, "box_h", 2065)], False)]  # 8 * 2065 * 2 * 255^2 >= 2^31


# ---- the refusals, word for word -----------------------------------------------------------------------------------------

def test_refusal_text_set_font(dec, fonts):
    who = "focr_decoder_set_font: "
    lib, h, s = dec._lib, dec._h, fonts["font"].s
    set_font = lambda: lib.focr_decoder_set_font(h, C.byref(s))  # noqa: E731
    refused(dec, lib.focr_decoder_set_font(h, None), who + "bad arguments")
    with bent((s, "n_glyphs", 0)):
        refused(dec, set_font(), who + "bad arguments")
    with bent((s, "n_glyphs", 65536)):
        refused(dec, set_font(), who + "more than 65535 glyphs")
    with bent((s, "bitmaps_len", s.bitmaps_len - 1)):
        refused(dec, set_font(), who + "bad bitmap table")
    with bent((s, "bitmaps_len", s.bitmaps_len - 2), (s.glyphs[0], "increment", 0.0)):  # the table's length comes before the glyphs
        refused(dec, set_font(), who + "bad bitmap table")
    for bends, advance in glyph_faults(s.glyphs[1], s.bitmaps_len):
        with bent(*bends):
            refused(dec, set_font(), who + ("a glyph does not advance the pen" if advance else "inconsistent glyph table"))
    g = s.glyphs[2]
    with bent((g, "increment", 0.0), (g, "stride", g.stride + 2)):  # of one glyph's two faults, the increment's
        refused(dec, set_font(), who + "a glyph does not advance the pen")
    with bent((s.glyphs[1], "offset", 2), (g, "increment", 0.0)):  # of two glyphs' faults, the first glyph's
        refused(dec, set_font(), who + "inconsistent glyph table")
    assert set_font() == 0


def test_refusal_text_set_baseline_fonts(dec, fonts):
    who = "focr_decoder_set_baseline_fonts: "
    lib, h, font = dec._lib, dec._h, fonts["font"]
    y0, y1 = font.fonts[0], font.fonts[1]
    upload = lambda bits=1: lib.focr_decoder_set_baseline_fonts(h, font.fonts, bits)  # noqa: E731
    refused(dec, upload(), who + "no font (focr_decoder_set_font)")
    assert lib.focr_decoder_set_font(h, C.byref(font.s)) == 0
    refused(dec, lib.focr_decoder_set_baseline_fonts(h, None, 1), who + "bad arguments")
    refused(dec, upload(4), who + "y_bits is at most 3")
    count = who + "a font does not match the decode font (glyph count)"
    for bends in ([(y1, "n_glyphs", 3)], [(y1, "glyphs", None)], [(y1, "bitmaps_len", y1.bitmaps_len - 1)], [(y0, "n_glyphs", 5), (y0, "kerning", 2.0)]):
        with bent(*bends):
            refused(dec, upload(), count)
    head = who + "a font does not match the decode font (origin, size, kerning or hinting)"
    assert y0.origin_x == 0.0
    other_zero = -math.copysign(0.0, y0.origin_x)  # equal as a number, not as bits
    for bends in ([(y1, "origin_x", other_zero)], [(y1, "origin_y", y1.origin_y + 1)], [(y1, "text_size", 9.0)], [(y1, "kerning", 1.5)], [(y1, "hinting", 1)],
                  [(y0, "hinting", 1), (y0.glyphs[0], "codepoint", 7)]):
        with bent(*bends):
            refused(dec, upload(), head)
    match = who + "a font does not match the decode font (code points or increments)"
    g = y1.glyphs[1]
    for bends in ([(g, "codepoint", g.codepoint + 1)], [(g, "increment", float(np.nextafter(np.float32(g.increment), np.float32(9))))],
                  [(g, "codepoint", 7), (g, "stride", g.stride + 1)], [(g, "increment", 0.0), (y1.glyphs[2], "offset", 2)]):
        with bent(*bends):
            refused(dec, upload(), match)
    for bends, advance in glyph_faults(g, y1.bitmaps_len):
        with bent(*bends):
            refused(dec, upload(), match if advance else who + "inconsistent glyph table")
    g0 = y0.glyphs[1]
    with bent((g0, "offset", g0.offset + 2)):  # fonts[0]'s table is checked as a table before it is compared
        refused(dec, upload(), who + "inconsistent glyph table")
    for bends in ([(g0, "off_x", 0, g0.off_x[0] + 1)], [(g0, "off_y", 63, g0.off_y[63] - 1)], [(g0, "box_w", g0.box_w - 1)]):
        with bent(*bends):
            refused(dec, upload(), who + "fonts[0] is not the decode font (glyph table)")
    with bent((y1, "bitmaps_len", 4 * 0xffffffff + 4)):  # lengths only: refused before a byte of it is read
        refused(dec, upload(), who + "bitmap tables too large")
    with bent((y0.bitmaps, 5, y0.bitmaps[5] ^ 1)):
        refused(dec, upload(), who + "fonts[0] is not the decode font (bitmaps)")
    assert upload() == 0


def test_refusal_text_set_font_candidates(dec, fonts):
    who = "focr_decoder_set_font_candidates: "
    lib, h, a, b = dec._lib, dec._h, fonts["cands"][0].s, fonts["cands"][1].s
    upload = lambda n=2: lib.focr_decoder_set_font_candidates(h, array_of(N.DecodeFontStruct, [a, b] + [b] * (n - 2)), n)  # noqa: E731
    refused(dec, upload(), who + "no font (focr_decoder_set_font)")
    assert lib.focr_decoder_set_font(h, C.byref(fonts["font"].s)) == 0
    refused(dec, upload(16), who + "at most 15 candidates (FOCR_FONT_CANDIDATES_MAX - 1)")
    with bent((a, "n_glyphs", 3), (a, "bitmaps_len", a.bitmaps_len - 1)):
        refused(dec, upload(), who + "candidate 1: the glyph count differs from the decode font's")
    with bent((b, "glyphs", None)):
        refused(dec, upload(), who + "candidate 2: the glyph count differs from the decode font's")
    with bent((b, "bitmaps_len", b.bitmaps_len - 1), (b.glyphs[0], "codepoint", 7)):
        refused(dec, upload(), who + "candidate 2: bad bitmap table")
    g = b.glyphs[1]
    with bent((g, "codepoint", g.codepoint + 1), (b.glyphs[0], "increment", 0.0)):  # glyph 0's fault comes first
        refused(dec, upload(), who + "candidate 2: a glyph does not advance the pen")
    with bent((g, "codepoint", g.codepoint + 1), (g, "increment", 0.0), (g, "stride", g.stride + 1)):
        refused(dec, upload(), who + "candidate 2: a code point differs from the decode font's")
    with bent((g, "increment", 0.0), (g, "stride", g.stride + 1)):
        refused(dec, upload(), who + "candidate 2: a glyph does not advance the pen")
    for k, s in ((1, a), (2, b)):
        for bends, advance in glyph_faults(s.glyphs[2], s.bitmaps_len):
            with bent(*bends):
                refused(dec, upload(), who + f"candidate {k}: " + ("a glyph does not advance the pen" if advance else "inconsistent glyph table"))
    with bent((a, "bitmaps_len", 4 * 0xffffffff + 4)):  # lengths only; no candidate is named
        refused(dec, upload(), who + "bitmap tables too large")
    with bent((a, "bitmaps_len", 4 * 0xffffffff + 4), (b.glyphs[0], "increment", 0.0)):  # candidate 1's length before candidate 2's glyphs
        refused(dec, upload(), who + "bitmap tables too large")
    assert upload() == 0 and lib.focr_decoder_set_font_candidates(h, None, 0) == 0


def verify_faults(v, d, whose):
    """(bends of verify glyph v over decode glyph d, the refusal behind the prefix)."""
    glyph = f"the table does not match the {whose} (code points or increments)"
    rect = f"a phase rectangle leaves the {whose}'s box"
    assert v.rect_x[5] + v.rect_w[5] <= d.box_w and v.rect_y[9] + v.rect_h[9] <= d.box_h
    return [([(v, "codepoint", v.codepoint + 1)], glyph), ([(v, "increment", float(np.nextafter(np.float32(v.increment), np.float32(0))))], glyph),
            ([(v, "box", 0, NAN)], "bad glyph box"), ([(v, "box", 1, -INF)], "bad glyph box"), ([(v, "box", 2, float(2 ** 20 + 1))], "bad glyph box"),
            ([(v, "box", 3, -float(2 ** 20 + 1))], "bad glyph box"),
            ([(v, "rect_x", 5, d.box_w - v.rect_w[5] + 1)], rect), ([(v, "rect_h", 9, d.box_h - v.rect_y[9] + 1)], rect),
            ([(v, "codepoint", 7), (v, "box", 0, NAN)], glyph), ([(v, "box", 3, INF), (v, "rect_w", 0, 999)], "bad glyph box")]


def head_faults(s):
    return [[(s, "n_glyphs", 3)], [(s, "text_size", s.text_size + 0.5)], [(s, "kerning", 1.25)], [(s, "hinting", 0 if s.hinting else 1)],
            [(s, "origin_y", s.origin_y + 1)], [(s, "origin_y", NAN), (s.glyphs[0], "codepoint", 7)]]


def test_refusal_text_set_verify_font(dec, fonts):
    who = "focr_decoder_set_verify_font: "
    lib, h, s = dec._lib, dec._h, fonts["vfont"].s
    upload = lambda: lib.focr_decoder_set_verify_font(h, C.byref(s))  # noqa: E731
    refused(dec, upload(), who + "no decode font (focr_decoder_set_font)")
    refused(dec, lib.focr_decoder_set_verify_font(h, None), who + "bad arguments")  # before the decode font is asked for
    assert lib.focr_decoder_set_font(h, C.byref(fonts["font"].s)) == 0
    for bends in ([(s, "glyphs", None)], [(s, "n_glyphs", 0)]):
        with bent(*bends):
            refused(dec, upload(), who + "bad arguments")
    for bends in head_faults(s):
        with bent(*bends):
            refused(dec, upload(), who + "the table does not match the decode font (glyph count, size, kerning, hinting or origin)")
    for bends, text in verify_faults(s.glyphs[2], fonts["font"].s.glyphs[2], "decode font"):
        with bent(*bends):
            refused(dec, upload(), who + text)
    assert upload() == 0


def test_refusal_text_set_verify_font_candidates(dec, fonts):
    who = "focr_decoder_set_verify_font_candidates: "
    lib, h, a, b = dec._lib, dec._h, fonts["vcands"][0].s, fonts["vcands"][1].s
    upload = lambda n=2: lib.focr_decoder_set_verify_font_candidates(h, array_of(N.VerifyFontStruct, [a, b][:n]), n)  # noqa: E731
    refused(dec, lib.focr_decoder_set_verify_font_candidates(h, None, 2), who + "bad arguments")
    refused(dec, upload(0), who + "bad arguments")
    refused(dec, upload(), who + "no decode font (focr_decoder_set_font)")
    assert lib.focr_decoder_set_font(h, C.byref(fonts["font"].s)) == 0
    refused(dec, upload(), who + "no font candidates (focr_decoder_set_font_candidates)")
    assert lib.focr_decoder_set_font_candidates(h, array_of(N.DecodeFontStruct, [c.s for c in fonts["cands"]]), 2) == 0
    refused(dec, upload(1), who + "one table per uploaded candidate: 2 of them")
    for k, s in ((1, a), (2, b)):
        for bends in head_faults(s) + [[(s, "glyphs", None)]]:
            with bent(*bends):
                refused(dec, upload(), who + f"candidate {k}: the table does not match the candidate (glyph count, size, kerning, hinting or origin)")
        for bends, text in verify_faults(s.glyphs[1], fonts["cands"][k - 1].s.glyphs[1], "candidate"):
            with bent(*bends):
                refused(dec, upload(), who + f"candidate {k}: " + text)
    with bent((a.glyphs[2], "box", 0, NAN), (b, "n_glyphs", 3)):  # candidate 1's glyphs before candidate 2's head
        refused(dec, upload(), who + "candidate 1: bad glyph box")
    assert upload() == 0
    with bent((b, "hinting", 2)):  # a truth value: candidate 2 is hinted
        assert upload() == 0


# ---- the decoder after a refusal ---------------------------------------------------------------------------------------------

LH = 12
GEO = (2, 0, 60, LH, 16)  # x, y, width, line_height, line_advance


def two_lines(spec=(MONO, 8.0, False), second=(MONO, 8.0, False)):
    page = np.full((40, 64), 255, dtype=np.uint8)
    for y, text, (f, t, h) in ((0, "Han naH", spec), (16, "nana H", second)):
        B.draw_offset(page, f, t, AL, text, 2, y, 0.0, h, 1.0)
    return page


def raw_run(dec, page, geo=GEO):
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], *geo)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def test_refused_baseline_fonts_leave_none(dec, fonts):
    """A baseline run with y_bits > 0 after a refused upload of the y-phase fonts is refused as one without any."""
    lib, h, font = dec._lib, dec._h, fonts["font"]
    dec.set_font(font, 8.0)  # uploads the y-phases as well
    page = two_lines()
    assert lib.focr_decoder_set_baseline_search(h, 1, 1) == 0
    assert raw_run(dec, page)[0] == 0
    with bent((font.fonts[1].glyphs[0], "stride", 6)):
        assert lib.focr_decoder_set_baseline_fonts(h, font.fonts, 1) != 0
    refused(dec, raw_run(dec, page)[0], "focr_decoder_run: a baseline search with y_bits > 0 (focr_decoder_set_baseline_search) needs the y-phase fonts of "
            "that y_bits (focr_decoder_set_baseline_fonts)")
    assert lib.focr_decoder_set_baseline_fonts(h, font.fonts, 1) == 0 and raw_run(dec, page)[0] == 0


def test_refused_set_font_keeps_the_font(dec, fonts):
    """set_font with a 2-glyph table whose second increment is 0 is refused, and the decode font is intact: its increments on
    the host, which a whole-line run plans from, its tables and its glyph count.  What set_font has always dropped on the way
    in stays dropped: the candidates."""
    lib, h, font = dec._lib, dec._h, fonts["font"]
    dec.set_font(font, 8.0)
    dec.set_font_candidates(fonts["cands"])
    pages = [two_lines()]
    before = dec.decode(pages, *GEO, whole_line=True)
    assert [len(pg) for pg in before[0]] == [2] and all(len(t) >= 6 for _, t in before[0][0])
    with bent((font.s, "n_glyphs", 2), (font.s.glyphs[1], "increment", 0.0)):
        refused(dec, lib.focr_decoder_set_font(h, C.byref(font.s)), "focr_decoder_set_font: a glyph does not advance the pen")
    dec._batch, dec._vfont, dec._candidates = None, None, []  # what LineDecoder.set_font forgets with the library
    after = dec.decode(pages, *GEO, whole_line=True)
    assert after[0] == before[0] and after[2] == before[2]
    assert all(np.array_equal(a, b) for a, b in zip(after[1][0], before[1][0]))
    assert lib.focr_decoder_set_font_search(h, 1) == 0
    rc, msg = raw_run(dec, pages[0])
    assert rc != 0 and msg == "focr_decoder_run: a font search (focr_decoder_set_font_search) with no candidates uploaded (focr_decoder_set_font_candidates)"
    assert lib.focr_decoder_set_font_search(h, 0) == 0


# ---- the round trip --------------------------------------------------------------------------------------------------------

def test_round_trip_against_the_models(dec, fonts):
    """All five uploads, then decode, the font search, verify, verify_text in every font and score_text in every font and at a
    fractional baseline: each exactly its model's."""
    specs = [(MONO, 8.0, False), (MONO, 9.0, False), (MONO, 8.0, True)]
    models = [FastModel(f, t, AL, h, 1.0) for f, t, h in specs]
    vfonts = [M.Font(f, t, h, 1.0) for f, t, h in specs]
    page = two_lines(second=specs[1])
    dec.set_font(fonts["font"], 8.0)
    dec.set_font_candidates(fonts["cands"])
    lines = dec.decode([page], *GEO)
    assert lines == [models[0].decode_image(page, *GEO)] and len(lines[0]) == 2
    sums, imgs = dec.verify()  # uploads the decode font's verify table
    img, sq = M.verify_text(page, [M.Line(y, t, 0) for y, t in lines[0]], vfonts, AL, 2)
    assert int(sums[0]) == sq and np.array_equal(imgs[0], img)
    want = FM.search_image(models, page, *GEO)
    got, ks, costs = dec.decode([page], *GEO, font_search=True)
    assert got == [[(y, r.text) for y, r in want]] and ks == [[r.k for _, r in want]] == [[0, 1]] and costs == [[r.cost for _, r in want]]
    texts = [(0, "Han n"), (16, "nanaH"), (24, "aH n")]
    for per_line in ([0, 1, 2], [2, 0, 1]):  # uploads the candidates' verify tables
        sums, imgs = dec.verify_text([page], [texts], 2, fonts=[per_line])
        img, sq = M.verify_text(page, [M.Line(y, t, k) for (y, t), k in zip(texts, per_line)], vfonts, AL, 2)
        assert int(sums[0]) == sq and np.array_equal(imgs[0], img)
    every = [dec.font] + fonts["cands"]
    for per_line, qs in (([0, 1, 2], [1, 0, -2]), ([0, 0, 0], [-1, 3, 0])):  # candidates have one vertical phase: whole rows only
        got = dec.score_text([page], [texts], 2, 60, LH, fonts=[per_line], baselines=[qs], y_bits=1)
        for (y, t), k, q, g in zip(texts, per_line, qs, got[0]):
            s = S.score_text(every[k], page, 2, y, 60, LH, t, q=q, y_bits=1)
            assert (g.base, g.cost, g.shift) == (s.base, s.cost, 0) and np.array_equal(g.terms, s.terms)
    for m in models:
        m.close()

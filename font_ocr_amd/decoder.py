"""The `focr` line decoder (src/main.rs of the reference): host side and the device decoder, over include/focr_decode.h.

    with LineDecoder(0) as dec:
        dec.set_font("DejaVuSansMono.ttf", 13.0)
        pages = dec.decode(luma_pages, x=45, y=39, width=608, line_height=12, line_advance=15)
        # [[(y, text), ...] per page]
        pages, mse, images = dec.decode(luma_pages, 45, 39, 608, 12, 15, verify="image")
        # focr --verify on the device: red = the page's ink, blue = the decoded text re-rendered; MSE per page
        pages, scores = dec.decode(luma_pages, 45, 39, 608, 12, 15, scores=True)
        # scores[page][line]: what the argmin knew about each character of pages[page][line] (LineScores)
        pages, offsets = dec.decode(luma_pages, 45, 39, 608, 12, 15, pen_search=8)
        # a search of 8/64 px around the pen at every step, carried forward; offsets[page][line]: each character's offset
        pages, pens, costs = dec.decode(luma_pages, 45, 39, 608, 12, 15, whole_line=True)
        # the whole line's squared error minimised over pens on the 1/64 px grid (for proportional fonts); pens[page][line]:
        # each character's pen in 1/64 px, costs[page][line]: the line's sum of footprint terms
        pages, pens, costs, margins = dec.decode(luma_pages, 45, 39, 608, 12, 15, whole_line=True, margins=True)
        # margins[page][line]: which characters of a whole line to doubt (LineMargins): each one's term, the glyph the
        # best other whole line reads over its middle, and how much worse that line is
        pages, pens, costs, offsets = dec.decode(luma_pages, 45, 39, 608, 12, 15, whole_line=True, pen_slack=8)
        # the whole-line decode for text off the 1/64 px grid: every step may move the pen by up to 8/64 px before its glyph
        # is rendered; pens[page][line]: each character's render pen, offsets[page][line]: the offset it took
        dec.set_font("DejaVuSansMono.ttf", 13.0, y_bits=2)
        pages, baselines, costs = dec.decode(luma_pages, 45, 39, 608, 12, 15, baseline_search=8)
        # every line decoded at the vertical offsets -8 ..= 8 quarter pixels and the one with the lowest summed footprint
        # term kept; baselines[page][line]: its q (the line sits q / 4 px below the crop's baseline), costs[page][line]: its sum
        pages, pens, costs, baselines = dec.decode(luma_pages, 45, 39, 608, 12, 15, whole_line=True, whole_baseline=2)
        # the whole-line decode under every vertical offset -2 ..= 2 quarter pixels, the candidate whose whole line costs
        # least kept: proportional text whose baseline is off the crop grid; baselines[page][line]: its q
        pages, baselines, costs = dec.decode(luma_pages, 45, 39, 608, 12, 15, baseline_search=1, y_frac=20, line_advance_frac=38)
        # a fractional line grid for the two baseline modes: the first line's top at 39 + 20/64 px and a leading of
        # 15 + 38/64 px; every line is cropped at the whole row of its own top and searched around its own sub-pixel part
        dec.set_font_candidates([("DejaVuSansMono.ttf", 12.0, False, 1.0), ("DejaVuSansMono-Bold.ttf", 13.0, False, 1.0)])
        pages, fonts, costs = dec.decode(luma_pages, 45, 39, 608, 12, 15, font_search=True)
        # every line decoded in the decode font (0) and in each candidate (1, 2) and the cheapest reading kept: pages that
        # mix fonts, or a font whose size, kerning or hinting is being looked for; fonts[page][line]: the winner's index,
        # costs[page][line]: its sum of footprint terms.  With whole_line=True: pages, pens, costs, fonts
        sums, images = dec.verify_text(luma_pages, pages, 45, fonts=fonts)
        # focr --verify of a reading the caller supplies, each line in its own font: a font search's result, or edited text
        scores = dec.score_text(luma_pages, pages, 45, 608, 12, fonts=fonts)
        # the decoder's own cost of such a reading: scores[page][line] is a TextScore(base, cost, shift, terms)
        base, cost, shift = dec.rank_text(luma_pages[0], 39, "the first line as a person reads it", 45, 608, 12, shift=8)
        # a known string under the decode font and every candidate: the argmin of cost is the font, no decoding
        aligned = dec.align_text(luma_pages, pages, 45, 608, 12, start=64, drift=128, step=4)
        # every character's pen fitted to the page: aligned[page][line] is a TextAlign(base, cost, first, last, pens, terms)
        base, cost, first, last, fit = dec.rank_text_aligned(luma_pages[0], 39, "the first line as a person reads it", 45, 608, 12, drift=128, step=4)
        # the same ranking with the pens fitted under each font; fit[k] = (scale, x64): the page's kerning relative to font k's
        # and where its text starts, in 1/64 px
        glyphs = dec.learn_text(luma_pages[:2], corrected_pages, 45, 608, 12)
        dec.set_font(dec.font.learned(glyphs))
        # glyph tables averaged from a reading somebody trusts (a LearnedGlyphs(sums, counts, used)): the rest of the pages are
        # then decoded with the page's own glyph shapes instead of this FreeType build's
        rects, texts = dec.test_images(luma_pages, 45, 39, 608, 12, 15)
        # focr --test on the device: the line boxes, and the alphabet at the top-left corner, over each page

There is no CPU path: the decoder needs a device, and says so when it has none.
"""
import collections
import ctypes as C

import numpy as np

from . import _native as N

FOCR_DEFAULT_ALPHABET = "> =ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"  # src/main.rs:13-14


class DecoderError(RuntimeError):
    pass


class LineScores(collections.namedtuple("LineScores", "base score runner runner_score")):
    """The scores of one decoded line (decode(..., scores=True)), aligned with its text.  base: the sum of r^2 over the
    line's crop (int), the part of a score every candidate shares.  Per character: score, the reference's score of the
    chosen glyph (int64); runner, the alphabet index of the glyph the argmin would have taken next (uint16; 0xFFFF for
    a one-glyph alphabet); runner_score, that glyph's score (int64; INT64_MAX without a runner).  Glyphs with
    identical bitmaps tie: runner_score == score."""

    __slots__ = ()


class LineMargins(collections.namedtuple("LineMargins", "term runner margin")):
    """The margins of one whole line (decode(..., whole_line=True, margins=True)), aligned with its text.  Per character:
    term, its footprint term (int32; the terms of a line sum to its cost); runner, the glyph that the best whole line
    reading another glyph over the character's midpoint reads there (a str, one character each; NO_RUNNER, "\\0", for a
    one-glyph alphabet); margin, that line's cost less the decoded line's (int64; >= 0, 0 between identical glyphs, -1
    without a runner).  include/focr_decode.h has the definition."""

    __slots__ = ()
    NO_RUNNER = "\0"


class TextScore(collections.namedtuple("TextScore", "base cost shift terms")):
    """The decoder's cost of one line the caller supplied (LineDecoder.score_text).  base: the sum of r^2 over the line's
    crop (int); cost: the sum of its characters' footprint terms at the winning rigid shift (int), what decode() returns as
    a line's cost; shift: that shift in 1/64 px (0 without a shift search); terms: each character's footprint term (an
    int32 array aligned with the text; None when not asked for).  base + cost is the squared error of the rendering
    against the crop where footprints do not overlap."""

    __slots__ = ()


class TextAlign(collections.namedtuple("TextAlign", "base cost first last pens terms")):
    """The forced alignment of one line the caller supplied (LineDecoder.align_text).  base: the sum of r^2 over the line's
    crop (int); cost: the sum of its characters' footprint terms at the fitted pens (int); first, last: the first and the
    last character's offset from its nominal pen in 1/64 px; pens: each character's fitted pen in 1/64 px (a uint32 array
    aligned with the text), which score_text(pens=) and verify_text(pens=) take as they are; terms: each character's footprint
    term there (an int32 array; None when not asked for)."""

    __slots__ = ()


class TextRefine(collections.namedtuple("TextRefine", "base cost_in cost sweeps changed text pens")):
    """One line the caller supplied, repaired against the composed line error (LineDecoder.refine_text).  base: the sum of r^2
    over the line's crop (int); cost_in, cost: the composed cost of the input and of the output (int; base + cost is the squared
    error of the line with all its glyphs drawn together, the max of their ink); sweeps: the sweeps made; changed: the
    characters whose glyph or pen differs from the input; text: the repaired text; pens: each character's pen in 1/64 px (a
    uint32 array aligned with the text), which score_text(pens=), verify_text(pens=) and learn_text(pens=) take as they are."""

    __slots__ = ()


class LearnedGlyphs(collections.namedtuple("LearnedGlyphs", "sums counts used")):
    """What a trusted reading showed of a font's glyphs (LineDecoder.learn_text).  sums: the page's inverted luma summed under
    every byte of the font's bitmaps (a uint64 array in the font's own `bitmaps` layout); counts: the samples of every cell, a
    uint64 array at [glyph * 64 + phase]; used[page][line]: a uint8 array aligned with the text, 1 where the character
    contributed (in use, its box wholly inside the crop, its line in the font that was learned).  a + b adds two: the sums and
    the counts, b's pages listed behind a's.  DecodeFont.learned() turns one into a font."""

    __slots__ = ()

    def __add__(self, other):
        if not isinstance(other, LearnedGlyphs):
            return NotImplemented
        if self.sums.shape != other.sums.shape or self.counts.shape != other.counts.shape:
            raise ValueError("LearnedGlyphs of different fonts do not add")
        return LearnedGlyphs(self.sums + other.sums, self.counts + other.counts, list(self.used) + list(other.used))


def nominal_pens(font, text, start=0):
    """The pens the whole-line programme gives `text` in the DecodeFont `font`: start + the running sum of
    inc64 = rint(increment * 64) in f32, in 1/64 px: what align_text measures its offsets from."""
    inc = font.increments()
    index = {c: i for i, c in reversed(list(enumerate(font.alphabet)))}
    inc64 = [int(np.rint(np.float32(inc[index[c]]) * np.float32(64))) for c in text]
    return np.array([int(start) + sum(inc64[:g]) for g in range(len(text))], dtype=np.int64)


def placed_pens(font, text, offsets=None):
    """The pens at which the pen loop (offsets None) or the pen search (its offsets, 1/64 px per character) places `text` in the
    DecodeFont `font`: the f32 walk of both (pos = pos + offset / 64, then pos + increment) and FreeType's delta
    trunc((origin_x + pos) * 64), less 64 * origin_x, in 1/64 px: what refine_text(pens=), score_text(pens=) and verify_text(pens=)
    take for a plain or pen_search reading.  origin_x must be a whole number >= 0, as for every pens placement."""
    ox = font.origin[0]
    if float(ox) != int(ox) or ox < 0:
        raise ValueError("placed_pens needs a font whose origin_x is a whole number >= 0")
    if offsets is not None and len(offsets) != len(text):
        raise ValueError(f"{len(offsets)} offsets for {len(text)} characters")
    inc = font.increments()
    index = {c: i for i, c in reversed(list(enumerate(font.alphabet)))}
    f32 = np.float32
    out, pos = [], f32(0)
    for g, c in enumerate(text):
        p = f32(pos + f32(int(offsets[g]) if offsets is not None else 0) * f32(0.015625))
        out.append(int(f32(f32(ox + p) * f32(64))) - 64 * int(ox))
        pos = f32(p + inc[index[c]])
    return np.array(out, dtype=np.int64)


def fit_pens(nominal, pens, terms, start=None):
    """The least-squares line of pen on nominal - start over the characters whose term is not 0 (a space never has one):
    (scale, x64), the page's kerning relative to the font's and the pen of a character at nominal `start` in 1/64 px, or
    (None, None) with fewer than two such characters or when they share one nominal pen.  start defaults to nominal[0].
    The sums are include/focr_decode.h's, in list order and in double arithmetic, so every implementation agrees to the bit."""
    nominal = [int(v) for v in nominal]
    if start is None:
        start = nominal[0] if nominal else 0
    k, su, sp, suu, sup = 0, 0.0, 0.0, 0.0, 0.0
    for m, p, t in zip(nominal, pens, terms):
        if int(t) == 0:
            continue
        u, q = float(m - int(start)), float(int(p))
        k += 1
        su += u
        sp += q
        suu += u * u
        sup += u * q
    d = k * suu - su * su
    if k < 2 or d == 0.0:
        return None, None
    scale = (k * sup - su * sp) / d
    return scale, (sp - scale * su) / k


# The modes of one decode()/decode_device() call, checked (LineDecoder._modes).
_Modes = collections.namedtuple("_Modes", "scores pen_search whole_line margins pen_slack baseline_search whole_baseline line_frac font_search")

# The results of one call as per-page lists, in the order of the public tuple; None where the modes write no such result.
_Run = collections.namedtuple("_Run", "text scores offsets pens costs margins slack_offsets whole_qs baselines baseline_costs fonts font_costs")


def _record(m, make):
    """A _Run with make() in the fields the modes m fill, and None in the others."""
    on = (True, m.scores, m.pen_search, m.whole_line, m.whole_line, m.margins, m.pen_slack, m.whole_baseline, m.baseline_search, m.baseline_search,
          m.font_search, m.font_search and not m.whole_line)
    return _Run(*(make() if o else None for o in on))


# The library's settings in the order _run issues them: the attribute that caches what the library was last given (its
# switch, its radius, or its (y_bits, radius) / (y_frac, advance_frac) pair), the setter, and the library's own default.
_SETTINGS = (("_baseline", "focr_decoder_set_baseline_search", (0, 0)), ("_whole_baseline", "focr_decoder_set_whole_baseline", (0, 0)),
             ("_line_frac", "focr_decoder_set_line_frac", (0, 0)), ("_pen_slack", "focr_decoder_set_whole_slack", 0),
             ("_margins", "focr_decoder_set_whole_margins", False), ("_whole", "focr_decoder_set_whole_line", False),
             ("_pen_search", "focr_decoder_set_pen_search", 0), ("_scores", "focr_decoder_set_scores", False),
             ("_font_search", "focr_decoder_set_font_search", False))


def _err():
    return C.create_string_buffer(512)


def _codepoints(text):
    cps = [ord(c) for c in text]
    return (C.c_uint32 * max(1, len(cps)))(*cps), len(cps)


def raster_glyph(font_path, text_size, char, tx, ty, canvas, hinting=False):
    """focr_raster_glyph: copy the glyph rendered at float translation (tx, ty) into `canvas` (uint8 h x w, in place)."""
    assert canvas.dtype == np.uint8 and canvas.flags.c_contiguous and canvas.ndim == 2
    e = _err()
    h, w = canvas.shape
    if N.decode_raster().focr_raster_glyph(font_path.encode(), float(text_size), int(hinting), ord(char), float(tx), float(ty),
                                           canvas.ctypes.data, w, h, e, len(e)) != 0:
        raise DecoderError(e.value.decode())
    return canvas


def glyph_metrics(font_path, text_size, char):
    """(advance in font units as f32, units_per_em, raster_bounds at the identity as (ox, oy, lx, ly))."""
    adv, upem, b, e = C.c_float(), C.c_uint32(), (C.c_int32 * 4)(), _err()
    if N.decode_raster().focr_glyph_metrics(font_path.encode(), float(text_size), ord(char), C.byref(adv), C.byref(upem), b, e,
                                            len(e)) != 0:
        raise DecoderError(e.value.decode())
    return np.float32(adv.value), int(upem.value), tuple(int(v) for v in b)


def render_text(font_path, text_size, text, kerning=1.0, hinting=False):
    """focr_render_text: render() of the reference (src/main.rs:40-85) -> uint8 coverage canvas (h x w, 255 = ink)."""
    cps, n = _codepoints(text)
    p, w, h, e = C.c_void_p(), C.c_size_t(), C.c_size_t(), _err()
    lib = N.decode_raster()
    if lib.focr_render_text(font_path.encode(), float(text_size), int(hinting), float(kerning), cps, n, C.byref(p), C.byref(w),
                            C.byref(h), e, len(e)) != 0:
        raise DecoderError(e.value.decode())
    try:
        out = np.ctypeslib.as_array((C.c_uint8 * max(1, w.value * h.value)).from_address(p.value)).copy()
    finally:
        C.CDLL(None).free(p)
    return out[: w.value * h.value].reshape(h.value, w.value)


def _page_list(luma_pages):
    """One (H, W) page, an (N, H, W) batch or a sequence of pages, as a list of pages."""
    if isinstance(luma_pages, np.ndarray) and luma_pages.ndim in (2, 3):
        return [luma_pages] if luma_pages.ndim == 2 else list(luma_pages)
    return list(luma_pages)


def _size_groups(pages):
    """The pages grouped by size, in the order each size first appears: ((h, w), idx, batch) with the pages idx stacked into one
    contiguous batch."""
    by_size = {}
    for i, p in enumerate(pages):
        by_size.setdefault(np.asarray(p).shape, []).append(i)
    for shape, idx in by_size.items():
        yield shape, idx, np.ascontiguousarray(np.stack([np.asarray(pages[i], dtype=np.uint8) for i in idx]))


def _ptr(a, empty=False):
    """The address of an array for the library; None for no array and, unless `empty`, for an array without elements."""
    return C.c_void_p(a.ctypes.data) if a is not None and (empty or a.size) else None


def _check_verify(verify):
    if verify not in (None, "mse", "image"):
        raise ValueError(f"verify must be None, 'mse' or 'image', not {verify!r}")


class DecodeFont:
    """The 64-phase table of an alphabet (focr_decode_font_build), and with y_bits > 0 its 1 << y_bits y-phase tables
    (focr_decode_font_build_y; phase 0 is the plain table).  Owns the native structs; free with close()."""

    def __init__(self, font_path, text_size, alphabet=FOCR_DEFAULT_ALPHABET, hinting=False, kerning=1.0, y_bits=0):
        if not 0 <= int(y_bits) <= 3:
            raise ValueError(f"y_bits must be 0 .. 3, not {y_bits!r}")
        self.font_path, self.text_size, self.alphabet = font_path, float(text_size), alphabet
        self.hinting, self.kerning, self.y_bits = bool(hinting), float(kerning), int(y_bits)
        self.fonts = (N.DecodeFontStruct * (1 << self.y_bits))()
        self.s = self.fonts[0]
        cps, n = _codepoints(alphabet)
        e = _err()
        lib = N.decode_raster()
        if self.y_bits:
            rc = lib.focr_decode_font_build_y(font_path.encode(), self.text_size, int(hinting), self.kerning, cps, n, self.y_bits,
                                              self.fonts, e, len(e))
        else:
            rc = lib.focr_decode_font_build(font_path.encode(), self.text_size, int(hinting), self.kerning, cps, n,
                                            C.byref(self.s), e, len(e))
        if rc != 0:
            self.s = self.fonts = None
            raise DecoderError(e.value.decode())

    @property
    def origin(self):
        return np.float32(self.s.origin_x), np.float32(self.s.origin_y)

    def increments(self):
        return np.array([self.s.glyphs[i].increment for i in range(self.s.n_glyphs)], dtype=np.float32)

    def phase(self, i, p, v=0):
        """(bitmap h x w, off_x, off_y) of glyph i's phase p in y-phase v."""
        f = self.fonts[v]
        g = f.glyphs[i]
        n = g.stride * g.box_h
        raw = np.ctypeslib.as_array(f.bitmaps, shape=(f.bitmaps_len,))
        bm = raw[g.offset + p * n: g.offset + (p + 1) * n].reshape(g.box_h, g.stride)[:, : g.box_w]
        return bm.copy(), int(g.off_x[p]), int(g.off_y[p])

    def learned(self, glyphs, min_count=1, grow=0):
        """This font with the cells a trusted reading showed replaced by their means (focr_decode_font_learn): glyphs is the
        LearnedGlyphs of LineDecoder.learn_text for this font, calls added up.  A cell (glyph, phase) is learned when it has at
        least min_count samples and its phase has ink here; inside the bounding rectangle of that ink, grown by `grow` pixels a
        side and clipped to the box, each byte becomes the mean rounded half up; everything else, every increment, box, offset
        and the origin are this font's.  With grow=1 supports of neighbours overlap and a page's cost drops below -line_base
        (the objective counts an overlap once per glyph), hence the default 0.  Returns a DecodeFont (y_bits 0) that set_font()
        and set_font_candidates() take as they are; n_learned and n_inked on it count the learned cells and the cells with ink."""
        if int(min_count) < 1 or int(grow) < 0:
            raise ValueError("learned: min_count must be at least 1 and grow at least 0")
        sums = np.ascontiguousarray(glyphs.sums, dtype=np.uint64)
        counts = np.ascontiguousarray(glyphs.counts, dtype=np.uint64)
        if sums.shape != (self.s.bitmaps_len,) or counts.shape != (self.s.n_glyphs * 64,):
            raise ValueError("learned: the sums and counts are not this font's")
        new = DecodeFont.__new__(DecodeFont)
        new.font_path, new.text_size, new.alphabet = self.font_path, self.text_size, self.alphabet
        new.hinting, new.kerning, new.y_bits = self.hinting, self.kerning, 0
        new.fonts = (N.DecodeFontStruct * 1)()
        new.s = new.fonts[0]
        n_learned, n_inked = C.c_size_t(), C.c_size_t()
        e = _err()
        if N.decode_raster().focr_decode_font_learn(C.byref(self.s), _ptr(sums, True), _ptr(counts, True), int(min_count), int(grow), C.byref(new.s),
                                                    C.byref(n_learned), C.byref(n_inked), e, len(e)) != 0:
            new.s = new.fonts = None
            raise DecoderError(e.value.decode())
        new.n_learned, new.n_inked = int(n_learned.value), int(n_inked.value)
        return new

    def close(self):
        if self.s is not None:
            for f in self.fonts:
                N.decode_raster().focr_decode_font_free(C.byref(f))
            self.s = self.fonts = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VerifyFont:
    """The verify table of an alphabet (focr_verify_font_build): each glyph's f32 raster box and each phase's true
    bitmap rectangle inside the decode font's box.  Owns the native struct; free with close()."""

    def __init__(self, font_path, text_size, alphabet=FOCR_DEFAULT_ALPHABET, hinting=False, kerning=1.0):
        self.font_path, self.text_size, self.alphabet = font_path, float(text_size), alphabet
        self.hinting, self.kerning = bool(hinting), float(kerning)
        self.s = N.VerifyFontStruct()
        cps, n = _codepoints(alphabet)
        e = _err()
        if N.decode_raster().focr_verify_font_build(font_path.encode(), self.text_size, int(hinting), self.kerning, cps, n,
                                                    C.byref(self.s), e, len(e)) != 0:
            raise DecoderError(e.value.decode())

    def box(self, i):
        """raster_bounds of glyph i at the identity before round_out: (ox, oy, lx, ly) as f32."""
        return np.array(self.s.glyphs[i].box[:], dtype=np.float32)

    def rect(self, i, p):
        """(x, y, w, h) of glyph i's phase p bitmap inside the decode font's box."""
        g = self.s.glyphs[i]
        return int(g.rect_x[p]), int(g.rect_y[p]), int(g.rect_w[p]), int(g.rect_h[p])

    def close(self):
        if self.s is not None:
            N.decode_raster().focr_verify_font_free(C.byref(self.s))
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LineDecoder:
    """focr's decode_image on one device: set_font(), then decode() batches of luma pages."""

    def __init__(self, device=0):
        self._lib = N.decode_hip()
        h = C.c_void_p()
        if self._lib.focr_decoder_create(int(device), C.byref(h)) != 0:
            raise DecoderError(self._lib.focr_decoder_last_error(None).decode())
        self._h = h
        self.font = None
        self.last_ms = 0.0
        self.last_verify_ms = 0.0
        self.last_test_ms = 0.0
        self._vfont = None
        self._batch = None  # (n_pages, page_h, page_w) of the last run
        self._candidates = []  # the DecodeFonts of set_font_candidates
        self._vcands = None  # ... and their VerifyFonts, once verify_text() has built them
        self.last_verify_text_ms = 0.0
        self.last_score_text_ms = 0.0
        self.last_align_text_ms = 0.0
        self.last_learn_text_ms = 0.0
        self.last_refine_text_ms = 0.0
        for attr, _, default in _SETTINGS:
            setattr(self, attr, default)

    def _check(self, rc):
        if rc != 0:
            raise DecoderError(self._lib.focr_decoder_last_error(self._h).decode())

    def set_font(self, font_path, text_size=None, alphabet=FOCR_DEFAULT_ALPHABET, hinting=False, kerning=1.0, y_bits=0):
        """Build (or take, when font_path is a DecodeFont) and upload the decode font.  y_bits > 0 also builds and uploads
        its 1 << y_bits y-phase tables, for decode(baseline_search=N) and decode(whole_line=True, whole_baseline=N) in steps
        of 2^-y_bits px; a DecodeFont (a learned one too: DecodeFont.learned) brings its own, and needs no text_size."""
        if text_size is None and not isinstance(font_path, DecodeFont):
            raise TypeError("set_font() needs a text_size to build a font from a path")
        font = font_path if isinstance(font_path, DecodeFont) else DecodeFont(font_path, text_size, alphabet, hinting, kerning, y_bits)
        self._vfont, self._batch = None, None  # the library drops its verify table, its y-phase fonts and its last run here too
        self._candidates, self._vcands = [], None  # ... and the candidates of the font search, with their verify tables
        self._check(self._lib.focr_decoder_set_font(self._h, C.byref(font.s)))
        self.font = font
        if font.y_bits:
            self._check(self._lib.focr_decoder_set_baseline_fonts(self._h, font.fonts, font.y_bits))
        return font

    def set_font_candidates(self, fonts):
        """Upload the candidates 1 ..= K of decode(font_search=True), K <= 15: a list of DecodeFonts over the decode font's
        alphabet, or of (font_path, text_size, hinting, kerning) tuples, which are built with it.  An empty list drops them, and
        so does set_font().  Returns the DecodeFonts."""
        if self.font is None:
            raise DecoderError("set_font() first")
        fonts = list(fonts)
        if len(fonts) > 15:
            raise ValueError(f"at most 15 font candidates, not {len(fonts)}")
        built = [f if isinstance(f, DecodeFont) else DecodeFont(f[0], f[1], self.font.alphabet, f[2], f[3]) for f in fonts]
        for f in built:
            if f.alphabet != self.font.alphabet:
                raise ValueError("a font candidate must have the decode font's alphabet")
        arr = (N.DecodeFontStruct * max(1, len(built)))()
        for i, f in enumerate(built):
            arr[i] = f.s  # the struct by value: its tables stay the DecodeFont's
        self._candidates, self._vcands = [], None  # the library drops the candidates' verify tables here too
        self._check(self._lib.focr_decoder_set_font_candidates(self._h, arr, len(built)))
        self._candidates = built
        return built

    def verify(self, images=True, rgb_device=None):
        """focr --verify of the last decode on the device: (sums, images).  sums[p] is page p's exact sum of
        (R - B)^2 (uint64); images is an (N, H, W, 3) uint8 array (red = the page's ink, blue = the decoded text
        re-rendered), or None when images is false or when they go to rgb_device, a device address of the HIP runtime
        this library uses with room for N * H * W * 3 bytes.  The verify table is built on first use."""
        if self._batch is None:
            raise DecoderError("verify: no decode since the font was set")
        if self._font_search:
            raise DecoderError("verify: the last decode searched fonts (drawing every line in its own font is a later step)")
        self._ensure_verify_font()
        n, h, w = self._batch
        sums = np.zeros(max(1, n), dtype=np.uint64)
        out = np.empty((n, h, w, 3), dtype=np.uint8) if images and rgb_device is None else None
        if rgb_device is not None:
            rgb, on_device = C.c_void_p(int(rgb_device)), 1
        else:
            rgb, on_device = (C.c_void_p(out.ctypes.data) if out is not None and out.size else None), 0
        self._check(self._lib.focr_decoder_verify(self._h, rgb, on_device, sums.ctypes.data))
        self.last_verify_ms = float(self._lib.focr_decoder_last_verify_ms(self._h))
        return sums[:n], out

    def _ensure_verify_font(self):
        if self._vfont is None:
            f = self.font
            vf = VerifyFont(f.font_path, f.text_size, f.alphabet, f.hinting, f.kerning)
            self._check(self._lib.focr_decoder_set_verify_font(self._h, C.byref(vf.s)))
            self._vfont = vf

    def _ensure_verify_candidates(self):
        if self._vcands is None:
            built = [VerifyFont(f.font_path, f.text_size, f.alphabet, f.hinting, f.kerning) for f in self._candidates]
            arr = (N.VerifyFontStruct * max(1, len(built)))()
            for i, vf in enumerate(built):
                arr[i] = vf.s  # the struct by value: its tables stay the VerifyFont's
            self._check(self._lib.focr_decoder_set_verify_font_candidates(self._h, arr, len(built)))
            self._vcands = built

    def verify_text(self, luma_pages, lines, x, fonts=None, pens=None, offsets=None, images=True):
        """focr --verify of a reading the caller supplies (focr_decoder_verify_text): (sums, images), as verify() returns them,
        for luma_pages (as for decode(); pages are grouped by size) under lines, [[(y, text), ...] per page]: every line rendered
        at (x, y) as render() renders a string, in list order (a later line's ink replaces an earlier line's blue).
        fonts, [[k, ...] per page], draws line by line in the decode font (0) or in candidate k of set_font_candidates();
        None is the decode font throughout.  pens (per page and line a sequence of 1/64 px, one per character) places every
        character at its pen, as the verify does after decode(whole_line=True); offsets (likewise) moves the pen by
        offsets / 64 px before each character and advances from there, as after decode(pen_search=N); giving both raises.
        The inputs have the shapes decode() returns, so a font search's picture is
            res = dec.decode(pages, x, y, w, lh, la, font_search=True); dec.verify_text(pages, res[0], x, fonts=res[1])
        and an edited reading is drawn by editing res[0].  A character outside the alphabet raises ValueError.  sums is a
        uint64 array in page order; images a per-page list of (H, W, 3) uint8 arrays, or None when images is false.  The verify
        tables are built on first use.  The last decode and its verify() are left as they were."""
        if self.font is None:
            raise DecoderError("set_font() first")
        if pens is not None and offsets is not None:
            raise ValueError("verify_text takes pens or offsets, not both")
        pages, lines, used, groups = self._pack_text("verify_text", luma_pages, lines, fonts, pens, offsets)
        if fonts is None and any(lines):
            used = {0}
        if 0 in used:
            self._ensure_verify_font()
        if used - {0}:
            self._ensure_verify_candidates()
        sums = np.zeros(len(pages), dtype=np.uint64)
        out = [None] * len(pages) if images else None
        for idx, batch, recs, chars, along, _, _ in groups:
            got, rgb = self._verify_text(batch, recs, chars, along if pens is not None else None, along if offsets is not None else None, x, images)
            for j, i in enumerate(idx):
                sums[i] = got[j]
                if images:
                    out[i] = rgb[j]
        return sums, out

    def _verify_text(self, batch, recs, chars, pens, offsets, x, images):
        """One focr_decoder_verify_text call over an (N, H, W) uint8 batch, its arguments as _score_text's: (sums, images or None)."""
        n, h, w = batch.shape
        larr = (N.TextLine * max(1, len(recs)))(*recs)
        carr = np.array(chars, dtype=np.uint16) if chars else np.zeros(1, dtype=np.uint16)
        parr = np.array(pens, dtype=np.uint32) if pens else None
        oarr = np.array(offsets, dtype=np.int8) if offsets else None
        got = np.zeros(n, dtype=np.uint64)
        rgb = np.empty((n, h, w, 3), dtype=np.uint8) if images else None
        self._check(self._lib.focr_decoder_verify_text(self._h, _ptr(batch), 0, n, w, h, int(x), larr, len(recs), _ptr(carr), _ptr(parr), _ptr(oarr),
                                                       len(chars), _ptr(rgb), 0, got.ctypes.data))
        self.last_verify_text_ms = float(self._lib.focr_decoder_last_verify_text_ms(self._h))
        return got, rgb

    def score_text(self, luma_pages, lines, x, width, line_height, fonts=None, pens=None, offsets=None, baselines=None, y_bits=0, shift=0,
                   terms=True):
        """The decoder's cost of a reading the caller supplies (focr_decoder_score_text): per [page][line] a
        TextScore(base, cost, shift, terms).  luma_pages and lines, [[(y, text), ...] per page], are decode()'s and
        verify_text()'s; every line is cropped as decode() crops it (x, width, line_height at its y) and its text scored in
        the decode font (0) or candidate fonts[page][line] of set_font_candidates(): base is the crop's sum of r^2, terms
        each character's footprint term (an int32 array; None when terms is false) and cost their sum, the number every
        mode of decode() minimises and returns.  Without pens and offsets the characters are placed as the pen loop places
        them; offsets (per page and line one per character, 1/64 px) as after decode(pen_search=N); pens (likewise) as after
        decode(whole_line=True); giving both raises.  baselines[page][line] is each line's q in steps of 2^-y_bits px, as
        decode(baseline_search=N) returns it.  shift=N scores every line at the rigid shifts -N ..= N in 1/64 px and keeps the
        lowest (cost, rank of the shift); TextScore.shift is the winner.  A character outside the alphabet raises ValueError.
        The last decode, its results and its verify() are left as they were."""
        if self.font is None:
            raise DecoderError("set_font() first")
        if pens is not None and offsets is not None:
            raise ValueError("score_text takes pens or offsets, not both")
        if not 0 <= int(shift) <= 64:
            raise ValueError(f"shift must be 0 .. 64 (1/64 px), not {shift!r}")
        if not 0 <= int(y_bits) <= 3:
            raise ValueError(f"y_bits must be 0 .. 3, not {y_bits!r}")
        if int(width) <= 0 or int(line_height) <= 0:
            raise ValueError("score_text: width and line_height must be positive")
        _, lines, _, groups = self._pack_text("score_text", luma_pages, lines, fonts, pens, offsets, baselines)
        out = [[None] * len(pg) for pg in lines]
        for _, batch, recs, chars, along, qs, where in groups:
            got = self._score_text(batch, recs, chars, along if pens is not None else None, along if offsets is not None else None,
                                   qs if baselines is not None else None, x, width, line_height, y_bits, shift, terms)
            for (i, q), score in zip(where, got):
                out[i][q] = score
        return out

    def _score_text(self, batch, recs, chars, pens, offsets, qs, x, width, line_height, y_bits, shift, terms):
        """One focr_decoder_score_text call over an (N, H, W) uint8 batch: recs are (page, y, first, n_chars, font) into chars
        (alphabet indices), pens / offsets lie beside chars and qs beside recs (None: not given).  A TextScore per record."""
        n, h, w = batch.shape
        larr = (N.TextLine * max(1, len(recs)))(*recs)
        carr = np.array(chars, dtype=np.uint16) if chars else np.zeros(1, dtype=np.uint16)
        parr = np.array(pens, dtype=np.uint32) if pens else None
        oarr = np.array(offsets, dtype=np.int8) if offsets else None
        qarr = np.array(qs, dtype=np.int8) if qs else None
        n_terms = sum(r[3] for r in recs)
        tarr = np.zeros(max(1, n_terms), dtype=np.int32) if terms else None
        sarr = (N.TextScoreStruct * max(1, len(recs)))()
        self._check(self._lib.focr_decoder_score_text(self._h, _ptr(batch), 0, n, w, h, int(x), int(width), int(line_height), larr, len(recs), _ptr(carr),
                                                      _ptr(parr), _ptr(oarr), len(chars), _ptr(qarr), int(y_bits), int(shift), _ptr(tarr), sarr))
        self.last_score_text_ms = float(self._lib.focr_decoder_last_score_text_ms(self._h))
        out, at = [], 0
        for r, s in zip(recs, sarr):
            out.append(TextScore(int(s.line_base), int(s.cost), int(s.shift), tarr[at: at + r[3]].copy() if terms else None))
            at += r[3]
        return out

    def _pack_text(self, who, luma_pages, lines, fonts, pens, offsets, baselines=None):
        """The reading of verify_text / score_text (`who`, for the messages), checked: (pages, lines, used, groups).  pages and lines
        as lists, used the set of fonts named, groups a generator of one (idx, batch, recs, chars, along, qs, where) per page size:
        the pages idx as one uint8 batch, recs (page in batch, y, first, n_chars, font) into chars (alphabet indices), along the
        pens or offsets beside chars, qs the baselines beside recs, where each record's (page, line)."""
        pages = _page_list(luma_pages)
        lines = [list(pg) for pg in lines]
        if len(lines) != len(pages):
            raise ValueError(f"lines must hold one list per page: {len(lines)} for {len(pages)} pages")
        for name, per in (("fonts", fonts), ("pens", pens), ("offsets", offsets), ("baselines", baselines)):
            if per is not None and (len(per) != len(pages) or any(len(a) != len(b) for a, b in zip(per, lines))):
                raise ValueError(f"{name} must hold one entry per line of lines")
        used = {int(k) for pg in fonts for k in pg} if fonts is not None else set()
        if any(k < 0 or k > len(self._candidates) for k in used):
            raise ValueError(f"fonts must be 0 .. {len(self._candidates)} (the decode font and the candidates of set_font_candidates)")
        index = {c: i for i, c in reversed(list(enumerate(self.font.alphabet)))}  # the first of equal characters
        per = pens if pens is not None else offsets

        def groups():
            for _, idx, batch in _size_groups(pages):
                recs, chars, along, qs, where = [], [], [], [], []
                for j, i in enumerate(idx):
                    for q, (ly, text) in enumerate(lines[i]):
                        try:
                            cs = [index[c] for c in text]
                        except KeyError as e:
                            raise ValueError(f"{who}: {e.args[0]!r} (page {i}, line {q}) is not in the alphabet") from None
                        recs.append((j, int(ly), len(chars), len(cs), int(fonts[i][q]) if fonts is not None else 0))
                        where.append((i, q))
                        chars.extend(cs)
                        if baselines is not None:
                            qs.append(int(baselines[i][q]))
                        if per is not None:
                            if len(per[i][q]) != len(cs):
                                raise ValueError(f"{who}: page {i}, line {q}: {len(per[i][q])} pens or offsets for {len(cs)} characters")
                            along.extend(int(v) for v in per[i][q])
                yield idx, batch, recs, chars, along, qs, where

        return pages, lines, used, groups()

    def align_text(self, luma_pages, lines, x, width, line_height, fonts=None, baselines=None, y_bits=0, start=0, drift=64, step=2, terms=True):
        """A forced alignment of a reading the caller supplies (focr_decoder_align_text): per [page][line] a
        TextAlign(base, cost, first, last, pens, terms).  luma_pages, lines, fonts, baselines and y_bits are score_text()'s.
        Every character g of a line starts from its nominal pen (nominal_pens(font, text, start): `start` in 1/64 px plus the
        font's own advances) and may sit e_g / 64 px from it, -drift <= e_g <= drift, with consecutive characters' offsets at
        most step / 64 px apart; the call returns the pens with the lowest summed footprint term (ties: the pen search's rank,
        0, -1, +1, ...).  step=0 is a rigid search of radius drift.  fit_pens() turns a result into the page's kerning and x.
        A character outside the alphabet raises ValueError.  The last decode, its results and its verify() are left as they were."""
        if self.font is None:
            raise DecoderError("set_font() first")
        if not 0 <= int(drift) <= 1024:
            raise ValueError(f"drift must be 0 .. 1024 (1/64 px), not {drift!r}")
        if not 0 <= int(step) <= 64:
            raise ValueError(f"step must be 0 .. 64 (1/64 px), not {step!r}")
        if not 0 <= int(start) < 1 << 24:
            raise ValueError(f"start must be 0 .. 2^24 - 1 (1/64 px), not {start!r}")
        if not 0 <= int(y_bits) <= 3:
            raise ValueError(f"y_bits must be 0 .. 3, not {y_bits!r}")
        if int(width) <= 0 or int(line_height) <= 0:
            raise ValueError("align_text: width and line_height must be positive")
        _, lines, _, groups = self._pack_text("align_text", luma_pages, lines, fonts, None, None, baselines)
        out = [[None] * len(pg) for pg in lines]
        for _, batch, recs, chars, _, qs, where in groups:
            got = self._align_text(batch, recs, chars, qs if baselines is not None else None, x, width, line_height, y_bits, start, drift, step, terms)
            for (i, q), a in zip(where, got):
                out[i][q] = a
        return out

    def _align_text(self, batch, recs, chars, qs, x, width, line_height, y_bits, start, drift, step, terms):
        """One focr_decoder_align_text call over an (N, H, W) uint8 batch, its arguments as _score_text's.  A TextAlign per record."""
        n, h, w = batch.shape
        larr = (N.TextLine * max(1, len(recs)))(*recs)
        carr = np.array(chars, dtype=np.uint16) if chars else np.zeros(1, dtype=np.uint16)
        qarr = np.array(qs, dtype=np.int8) if qs else None
        n_out = sum(r[3] for r in recs)
        parr = np.zeros(max(1, n_out), dtype=np.uint32)
        tarr = np.zeros(max(1, n_out), dtype=np.int32) if terms else None
        aarr = (N.TextAlignStruct * max(1, len(recs)))()
        self._check(self._lib.focr_decoder_align_text(self._h, _ptr(batch), 0, n, w, h, int(x), int(width), int(line_height), larr, len(recs), _ptr(carr),
                                                      len(chars), _ptr(qarr), int(y_bits), int(start), int(drift), int(step), _ptr(parr), _ptr(tarr), aarr))
        self.last_align_text_ms = float(self._lib.focr_decoder_last_align_text_ms(self._h))
        out, at = [], 0
        for r, a in zip(recs, aarr):
            out.append(TextAlign(int(a.line_base), int(a.cost), int(a.first), int(a.last), parr[at: at + r[3]].copy(),
                                 tarr[at: at + r[3]].copy() if terms else None))
            at += r[3]
        return out

    def refine_text(self, luma_pages, lines, x, width, line_height, pens, fonts=None, radius=4, sweeps=4, glyphs=True):
        """A reading the caller supplies, repaired against the composed line error (focr_decoder_refine_text): per [page][line] a
        TextRefine(base, cost_in, cost, sweeps, changed, text, pens).  luma_pages, lines and fonts are score_text()'s; pens (per
        page and line one per character, 1/64 px, not decreasing within a line) are required: a whole-line run's, align_text's,
        or placed_pens() of a plain or pen_search reading.  The line is drawn with all its glyphs together (the max of their
        ink); a sweep visits the characters in order, and each takes the (glyph, pen offset j, -radius <= j <= radius) that lowers
        the composed cost the most, if any does (glyphs=False: its own glyph only); at most `sweeps` sweeps, 0 only evaluates.
        No other pen moves when a glyph with another advance is chosen.  A character outside the alphabet raises ValueError.  The
        last decode, its results and its verify() are left as they were."""
        if self.font is None:
            raise DecoderError("set_font() first")
        if pens is None:
            raise ValueError("refine_text needs pens (placed_pens() gives a plain or pen_search reading's)")
        if not 0 <= int(radius) <= 64:
            raise ValueError(f"radius must be 0 .. 64 (1/64 px), not {radius!r}")
        if not 0 <= int(sweeps) <= 8:
            raise ValueError(f"sweeps must be 0 .. 8, not {sweeps!r}")
        if int(width) <= 0 or int(line_height) <= 0:
            raise ValueError("refine_text: width and line_height must be positive")
        _, lines, _, groups = self._pack_text("refine_text", luma_pages, lines, fonts, pens, None)
        out = [[None] * len(pg) for pg in lines]
        for _, batch, recs, chars, along, _, where in groups:
            got = self._refine_text(batch, recs, chars, along, x, width, line_height, radius, sweeps, glyphs)
            for (i, q), r in zip(where, got):
                out[i][q] = r
        return out

    def _refine_text(self, batch, recs, chars, pens, x, width, line_height, radius, sweeps, glyphs):
        """One focr_decoder_refine_text call over an (N, H, W) uint8 batch, its arguments as _score_text's.  A TextRefine per record."""
        n, h, w = batch.shape
        larr = (N.TextLine * max(1, len(recs)))(*recs)
        carr = np.array(chars, dtype=np.uint16) if chars else np.zeros(1, dtype=np.uint16)
        parr = np.array(pens, dtype=np.uint32) if pens else np.zeros(1, dtype=np.uint32)
        n_out = sum(r[3] for r in recs)
        cout = np.zeros(max(1, n_out), dtype=np.uint16)
        pout = np.zeros(max(1, n_out), dtype=np.uint32)
        rarr = (N.TextRefineStruct * max(1, len(recs)))()
        self._check(self._lib.focr_decoder_refine_text(self._h, _ptr(batch), 0, n, w, h, int(x), int(width), int(line_height), larr, len(recs), _ptr(carr),
                                                       _ptr(parr), len(chars), int(radius), int(sweeps), int(bool(glyphs)), _ptr(cout), _ptr(pout), rarr))
        self.last_refine_text_ms = float(self._lib.focr_decoder_last_refine_text_ms(self._h))
        out, at = [], 0
        for r, a in zip(recs, rarr):
            text = "".join(self.font.alphabet[i] for i in cout[at: at + r[3]])
            out.append(TextRefine(int(a.line_base), int(a.cost_in), int(a.cost), int(a.sweeps_run), int(a.changed), text, pout[at: at + r[3]].copy()))
            at += r[3]
        return out

    def learn_text(self, luma_pages, lines, x, width, line_height, fonts=None, pens=None, offsets=None, use=None, font=0):
        """What a reading the caller TRUSTS shows of font `font`'s glyphs (focr_decoder_learn_text): a LearnedGlyphs(sums, counts,
        used).  luma_pages, lines, fonts, pens and offsets are score_text()'s, placed as there at shift 0; font is 0 for the decode
        font or k for a candidate of set_font_candidates(), and only the lines in that font contribute.  Every character in use
        whose glyph box lies wholly inside its line's crop adds the page's inverted luma under the box to its cell (glyph, phase)
        and 1 to the cell's count; use[page][line] holds one truth value per character (None: all), and a character left out
        still moves the pen.  Page sizes and batches are added up in uint64; add further calls with +.  DecodeFont.learned()
        makes the font.  The reading must be right: tables learned from the decoder's own reading reproduce its errors.
        A character outside the alphabet raises ValueError.  The last decode, its results and its verify() are left as they were."""
        if self.font is None:
            raise DecoderError("set_font() first")
        if pens is not None and offsets is not None:
            raise ValueError("learn_text takes pens or offsets, not both")
        if not 0 <= int(font) <= len(self._candidates):
            raise ValueError(f"font must be 0 .. {len(self._candidates)} (the decode font and the candidates of set_font_candidates)")
        if int(width) <= 0 or int(line_height) <= 0:
            raise ValueError("learn_text: width and line_height must be positive")
        _, lines, _, groups = self._pack_text("learn_text", luma_pages, lines, fonts, pens, offsets)
        if use is not None and (len(use) != len(lines) or any(len(a) != len(b) for a, b in zip(use, lines))):
            raise ValueError("use must hold one entry per line of lines")
        target = self._candidates[int(font) - 1] if int(font) else self.font
        sums = np.zeros(target.s.bitmaps_len, dtype=np.uint64)
        counts = np.zeros(target.s.n_glyphs * 64, dtype=np.uint64)
        used = [[None] * len(pg) for pg in lines]
        for _, batch, recs, chars, along, _, where in groups:
            mask = None
            if use is not None:
                mask = []
                for (i, q), r in zip(where, recs):
                    if len(use[i][q]) != r[3]:
                        raise ValueError(f"learn_text: page {i}, line {q}: {len(use[i][q])} use flags for {r[3]} characters")
                    mask.extend(1 if v else 0 for v in use[i][q])
            s, c, u = self._learn_text(batch, recs, chars, along if pens is not None else None, along if offsets is not None else None, mask, x, width,
                                       line_height, int(font), len(sums), len(counts))
            sums += s
            counts += c
            at = 0
            for (i, q), r in zip(where, recs):
                used[i][q] = u[at: at + r[3]].copy()
                at += r[3]
        return LearnedGlyphs(sums, counts, used)

    def _learn_text(self, batch, recs, chars, pens, offsets, use, x, width, line_height, font, n_sums, n_counts):
        """One focr_decoder_learn_text call over an (N, H, W) uint8 batch, its reading as _score_text's and use beside chars
        (None: all).  (sums uint32, counts uint32, used uint8 per listed character)."""
        n, h, w = batch.shape
        larr = (N.TextLine * max(1, len(recs)))(*recs)
        carr = np.array(chars, dtype=np.uint16) if chars else np.zeros(1, dtype=np.uint16)
        parr = np.array(pens, dtype=np.uint32) if pens else None
        oarr = np.array(offsets, dtype=np.int8) if offsets else None
        uarr = np.array(use, dtype=np.uint8) if use else None
        sarr = np.zeros(max(1, n_sums), dtype=np.uint32)
        karr = np.zeros(max(1, n_counts), dtype=np.uint32)
        darr = np.zeros(max(1, sum(r[3] for r in recs)), dtype=np.uint8)
        self._check(self._lib.focr_decoder_learn_text(self._h, _ptr(batch), 0, n, w, h, int(x), int(width), int(line_height), larr, len(recs), _ptr(carr),
                                                      _ptr(parr), _ptr(oarr), _ptr(uarr), len(chars), int(font), _ptr(sarr), _ptr(karr), _ptr(darr)))
        self.last_learn_text_ms = float(self._lib.focr_decoder_last_learn_text_ms(self._h))
        return sarr[:n_sums], karr[:n_counts], darr

    def rank_text(self, page, y, text, x, width, line_height, shift=0):
        """Which uploaded font renders a known string closest to the page: text scored at line slot (x, y) of one luma page
        under the decode font and every candidate of set_font_candidates() in one call, the same line listed K + 1 times.
        Returns (base, cost[K + 1], shift[K + 1]): the crop's sum of r^2, and per font its cost (int64) and its winning rigid
        shift in 1/64 px (shift=N searches -N ..= N).  The argmin over (cost, k) is the font; base + cost[k] is its squared
        error (footprints that overlap counted once each).  Nothing is decoded.  rank_text_aligned() fits the pens instead."""
        page = np.asarray(page)
        if page.ndim != 2:
            raise ValueError("rank_text takes one luma page (H, W)")
        k1 = len(self._candidates) + 1
        got = self.score_text([page], [[(y, text)] * k1], x, width, line_height, fonts=[list(range(k1))], shift=shift, terms=False)[0]
        return got[0].base, np.array([s.cost for s in got], dtype=np.int64), np.array([s.shift for s in got], dtype=np.int32)

    def rank_text_aligned(self, page, y, text, x, width, line_height, drift=64, step=2, start=0):
        """rank_text() with the pens fitted under every font (align_text(start=start, drift=drift, step=step), the same line
        listed K + 1 times), for a page whose kerning or x is not the font's, where a rigid shift loses the page's own font.
        Returns (base, cost[K + 1], first[K + 1], last[K + 1], fit[K + 1]): the crop's sum of r^2 and per font its cost (int64),
        its first and last character's offset in 1/64 px (int32) and fit_pens()'s (scale, x64), (None, None) without a fit.  It is
        a method of its own, so that rank_text() stays exactly what it was: a rigid shift and a drift do not combine."""
        page = np.asarray(page)
        if page.ndim != 2:
            raise ValueError("rank_text_aligned takes one luma page (H, W)")
        k1 = len(self._candidates) + 1
        got = self.align_text([page], [[(y, text)] * k1], x, width, line_height, fonts=[list(range(k1))], start=start, drift=drift, step=step)[0]
        fonts = [self.font] + list(self._candidates)
        fits = [fit_pens(nominal_pens(f, text, start), a.pens, a.terms, start) for f, a in zip(fonts, got)]
        return (got[0].base, np.array([a.cost for a in got], dtype=np.int64), np.array([a.first for a in got], dtype=np.int32),
                np.array([a.last for a in got], dtype=np.int32), fits)

    def test_images(self, luma_pages, x, y, width, line_height, line_advance, rgba=None, rect=True, text=True):
        """focr --test on the device: (rect_images, text_images), each a per-page list of (H, W, 4) uint8 RGBA images,
        or None where that image was not asked for.  rect draws the box of every non-blank line slot, text the whole
        alphabet rendered at the top-left corner, both blended in red over the page: over rgba (per page (H, W, 4)
        uint8, in the layout of luma_pages) when given, else over the grey page.  luma_pages as for decode(); pages are
        grouped by size.  The text image needs set_font(); its verify table is built on first use.  The last decode
        and its verify are left as they were."""
        if text and self.font is None:
            raise DecoderError("set_font() first")
        geo = (int(x), int(y), int(width), int(line_height), int(line_advance))
        pages = _page_list(luma_pages)
        if rgba is not None:
            if isinstance(rgba, np.ndarray) and rgba.ndim == 3:
                rgba = [rgba]
            rgba = list(rgba)
            if len(rgba) != len(pages) or any(np.asarray(c).shape != np.asarray(p).shape + (4,) for c, p in zip(rgba, pages)):
                raise ValueError("rgba must hold one (H, W, 4) image per page, of its page's size")
        if text:
            self._ensure_verify_font()
        rects = [None] * len(pages) if rect else None
        texts = [None] * len(pages) if text else None
        for (h, w), idx, batch in _size_groups(pages):
            base = None if rgba is None else np.ascontiguousarray(np.stack([np.asarray(rgba[i], dtype=np.uint8) for i in idx]))
            r_out = np.empty((len(idx), h, w, 4), dtype=np.uint8) if rect else None
            t_out = np.empty((len(idx), h, w, 4), dtype=np.uint8) if text else None
            self._check(self._lib.focr_decoder_test_images(self._h, _ptr(batch, True), _ptr(base, True), 0, len(idx), w, h, *geo, _ptr(r_out, True),
                                                           _ptr(t_out, True), 0))
            self.last_test_ms = float(self._lib.focr_decoder_last_test_ms(self._h))
            for j, i in enumerate(idx):
                if rect:
                    rects[i] = r_out[j]
                if text:
                    texts[i] = t_out[j]
        return rects, texts

    def test_images_device(self, pages_ptr, n_pages, page_h, page_w, x, y, width, line_height, line_advance, rgba_ptr=None,
                           rect_ptr=None, text_ptr=None):
        """As test_images(), all in device memory of the decoder's device (addresses of the HIP runtime this library
        uses): n_pages luma pages at pages_ptr, their RGBA base at rgba_ptr (or None for grey), and the images written
        to rect_ptr / text_ptr (n_pages * page_h * page_w * 4 bytes each, 4-byte aligned; None: not drawn)."""
        if text_ptr is not None:
            if self.font is None:
                raise DecoderError("set_font() first")
            self._ensure_verify_font()
        p = lambda a: C.c_void_p(int(a)) if a is not None else None  # noqa: E731
        self._check(self._lib.focr_decoder_test_images(self._h, p(pages_ptr), p(rgba_ptr), 1, int(n_pages), int(page_w),
                                                       int(page_h), int(x), int(y), int(width), int(line_height),
                                                       int(line_advance), p(rect_ptr), p(text_ptr), 1))
        self.last_test_ms = float(self._lib.focr_decoder_last_test_ms(self._h))

    def debug_blend(self, bg, fg):
        """The device's blend (image's Blend for Rgba<u8>, as test_images draws with) of fg onto bg: (N, 4) uint8 each."""
        bg = np.ascontiguousarray(bg, dtype=np.uint8).reshape(-1, 4)
        fg = np.ascontiguousarray(fg, dtype=np.uint8).reshape(-1, 4)
        if bg.shape != fg.shape:
            raise ValueError("bg and fg must have the same shape")
        out = np.empty_like(bg)
        self._check(self._lib.focr_decoder_debug_blend(self._h, bg.ctypes.data, fg.ctypes.data, len(bg), out.ctypes.data))
        return out

    def _verified(self, verify, h, w):
        """(mse per page as f32, images or None) of the last run, for decode(verify=...)."""
        sums, imgs = self.verify(images=verify == "image")
        mse = sums.astype(np.float32) / np.float32((h * w) & 0xFFFFFFFF)  # red_blue_mse: (sum as f32) / (w * h as u32)
        return mse, imgs

    def _run(self, ptr, on_device, n, h, w, x, y, width, line_height, line_advance, m):
        """One batch under the modes m: the _Run of its per-page lists."""
        self._batch = None
        y_bits = self.font.y_bits
        values = ((y_bits if m.baseline_search else 0, m.baseline_search), (y_bits if m.whole_baseline else 0, m.whole_baseline), m.line_frac,
                  m.pen_slack, m.margins, m.whole_line, m.pen_search, m.scores, m.font_search)
        for (attr, setter, _), value in zip(_SETTINGS, values):
            if value != getattr(self, attr):
                self._check(getattr(self._lib, setter)(self._h, *(value if isinstance(value, tuple) else (int(value),))))
                setattr(self, attr, value)
        self._check(self._lib.focr_decoder_run(self._h, ptr, int(on_device), n, w, h, x, y, width, line_height, line_advance))
        self._batch = (n, h, w)
        self.last_ms = float(self._lib.focr_decoder_last_ms(self._h))
        nl, nc = self._lib.focr_decoder_n_lines(self._h), self._lib.focr_decoder_n_chars(self._h)
        lines = (N.DecodedLine * max(1, nl))()
        chars = np.zeros(max(1, nc), dtype=np.uint16)
        self._check(self._lib.focr_decoder_get(self._h, lines, chars.ctypes.data))
        if m.scores:
            cs = np.zeros(max(1, nc), dtype=np.dtype([("score", "<i8"), ("runner_score", "<i8"), ("runner", "<u2"), ("pad", "<u2", 3)]))
            base = np.zeros(max(1, nl), dtype=np.uint64)
            self._check(self._lib.focr_decoder_get_scores(self._h, cs.ctypes.data_as(C.POINTER(N.CharScore)), base.ctypes.data))
        if m.pen_search or m.pen_slack:
            js = np.zeros(max(1, nc), dtype=np.int8)
            self._check(self._lib.focr_decoder_get_offsets(self._h, js.ctypes.data))
        if m.whole_line:
            ps = np.zeros(max(1, nc), dtype=np.uint32)
            lc = np.zeros(max(1, nl), dtype=np.int64)
            self._check(self._lib.focr_decoder_get_pens(self._h, ps.ctypes.data, lc.ctypes.data))
        if m.margins:
            ms = np.zeros(max(1, nc), dtype=np.dtype([("term", "<i4"), ("runner", "<u2"), ("pad", "<u2"), ("margin", "<i8")]))
            self._check(self._lib.focr_decoder_get_margins(self._h, ms.ctypes.data))
        if m.baseline_search or m.whole_baseline:
            bq = np.zeros(max(1, nl), dtype=np.int8)
            bc = np.zeros(max(1, nl), dtype=np.int64)
            self._check(self._lib.focr_decoder_get_baselines(self._h, bq.ctypes.data, bc.ctypes.data))
        if m.font_search:
            fk = np.zeros(max(1, nl), dtype=np.uint8)
            fc = np.zeros(max(1, nl), dtype=np.int64)
            self._check(self._lib.focr_decoder_get_fonts(self._h, fk.ctypes.data, fc.ctypes.data))
        alpha = self.font.alphabet
        r = _record(m, lambda: [[] for _ in range(n)])
        text, sc, offs, pens, costs, mar, slack_offs, whole_qs, bqs, bcosts, fonts, fcosts = r  # locals, like the modes: the loop runs once per line
        scores, pen_search, whole_line, margins, pen_slack, baseline_search, whole_baseline, _, font_search = m
        for k in range(nl):
            ln = lines[k]
            page, at = ln.page, slice(ln.first, ln.first + ln.n_chars)
            text[page].append((int(ln.y), "".join(alpha[c] for c in chars[at])))
            if scores:
                c = cs[at]
                sc[page].append(LineScores(int(base[k]), c["score"].copy(), c["runner"].copy(), c["runner_score"].copy()))
            if pen_search:
                offs[page].append(js[at].copy())
            if whole_line:
                pens[page].append(ps[at].copy())
                costs[page].append(int(lc[k]))
            if margins:
                c = ms[at]
                runner = "".join(LineMargins.NO_RUNNER if i == 0xFFFF else alpha[i] for i in c["runner"])
                mar[page].append(LineMargins(c["term"].copy(), runner, c["margin"].copy()))
            if pen_slack:
                slack_offs[page].append(js[at].copy())
            if whole_baseline:
                whole_qs[page].append(int(bq[k]))
            if baseline_search:
                bqs[page].append(int(bq[k]))
                bcosts[page].append(int(bc[k]))
            if font_search:
                fonts[page].append(int(fk[k]))
                if fcosts is not None:
                    fcosts[page].append(int(fc[k]))
        return r

    @staticmethod
    def _assemble(verified, r):
        """The public result of decode() and decode_device(): (lines[, mse, images][, scores][, offsets][, pens, costs][, margins]
        [, slack offsets][, whole-baseline qs][, baselines, costs][, fonts[, costs]]), or the bare lines when nothing else was asked for.
        verified: () or (mse, images)."""
        res = (r.text,) + verified + tuple(v for v in r[1:] if v is not None)
        return res if len(res) > 1 else r.text

    @staticmethod
    def _check_pen_search(pen_search):
        if not 0 <= int(pen_search) <= 64:
            raise ValueError(f"pen_search must be 0 .. 64 (1/64 px), not {pen_search!r}")
        return int(pen_search)

    @staticmethod
    def _check_whole_line(whole_line, scores, pen_search):
        if whole_line and scores:
            raise ValueError("whole_line=True does not go with scores=True (a runner-up has no definition under the dynamic programme)")
        if whole_line and pen_search:
            raise ValueError("whole_line=True does not go with pen_search (the dynamic programme does not search offsets)")
        return bool(whole_line)

    @staticmethod
    def _check_margins(margins, whole_line):
        if margins and not whole_line:
            raise ValueError("margins=True needs whole_line=True (the margins are the whole-line decode's)")
        return bool(margins)

    @staticmethod
    def _check_pen_slack(pen_slack, whole_line, margins):
        if not 0 <= int(pen_slack) <= 64:
            raise ValueError(f"pen_slack must be 0 .. 64 (1/64 px), not {pen_slack!r}")
        if int(pen_slack) and not whole_line:
            raise ValueError("pen_slack needs whole_line=True (the slack is the whole-line decode's; pen_search is the pen loop's)")
        if int(pen_slack) and margins:
            raise ValueError("pen_slack does not go with margins=True (margins under a pen slack have no definition yet)")
        return int(pen_slack)

    @staticmethod
    def _check_baseline_search(baseline_search, scores, pen_search, whole_line, margins, pen_slack):
        n = int(baseline_search)
        if not 0 <= n <= 32:
            raise ValueError(f"baseline_search must be 0 .. 32 (steps of 2^-y_bits px), not {baseline_search!r}")
        for on, what in ((scores, "scores=True"), (pen_search, "pen_search"), (whole_line, "whole_line=True"), (margins, "margins=True"),
                         (pen_slack, "pen_slack")):
            if n and on:
                raise ValueError(f"baseline_search does not go with {what} (the baseline search runs the plain pen loop per candidate)")
        return n

    @staticmethod
    def _check_whole_baseline(whole_baseline, whole_line, margins, pen_slack):
        n = int(whole_baseline)
        if not 0 <= n <= 32:
            raise ValueError(f"whole_baseline must be 0 .. 32 (steps of 2^-y_bits px), not {whole_baseline!r}")
        if n and not whole_line:
            raise ValueError("whole_baseline needs whole_line=True (the pen loop's search is baseline_search)")
        for on, what in ((margins, "margins=True"), (pen_slack, "pen_slack")):
            if n and on:
                raise ValueError(f"whole_baseline does not go with {what} (neither has a definition across candidates yet)")
        return n

    @staticmethod
    def _check_line_frac(y_frac, line_advance_frac, baseline_search, whole_baseline):
        fr = (int(y_frac), int(line_advance_frac))
        for v, name in zip(fr, ("y_frac", "line_advance_frac")):
            if not 0 <= v <= 63:
                raise ValueError(f"{name} must be 0 .. 63 (1/64 px), not {v!r}")
        if fr != (0, 0) and not baseline_search and not whole_baseline:
            raise ValueError("y_frac and line_advance_frac need baseline_search or whole_baseline (no other mode renders at a sub-pixel row yet)")
        return fr

    def _check_font_search(self, font_search, verify, scores, pen_search, margins, pen_slack, baseline_search, whole_baseline):
        for on, what in ((scores, "scores=True"), (pen_search, "pen_search"), (margins, "margins=True"), (pen_slack, "pen_slack"),
                         (baseline_search, "baseline_search"), (whole_baseline, "whole_baseline"), (verify, "verify")):
            if font_search and on:
                raise ValueError(f"font_search=True does not go with {what} yet (the candidates run the plain pen loop or the plain whole-line decode)")
        if font_search and not getattr(self, "_candidates", None):
            raise ValueError("font_search=True needs candidates (set_font_candidates)")
        return bool(font_search)

    def _modes(self, verify, scores, pen_search, whole_line, margins, pen_slack, baseline_search, whole_baseline, y_frac, line_advance_frac,
               font_search=False):
        """The checks of decode() and decode_device() in their order, and the modes as one record."""
        if self.font is None:
            raise DecoderError("set_font() first")
        _check_verify(verify)
        pen_search = self._check_pen_search(pen_search)
        whole_line = self._check_whole_line(whole_line, scores, pen_search)
        margins = self._check_margins(margins, whole_line)
        pen_slack = self._check_pen_slack(pen_slack, whole_line, margins)
        baseline_search = self._check_baseline_search(baseline_search, scores, pen_search, whole_line, margins, pen_slack)
        whole_baseline = self._check_whole_baseline(whole_baseline, whole_line, margins, pen_slack)
        line_frac = self._check_line_frac(y_frac, line_advance_frac, baseline_search, whole_baseline)
        font_search = self._check_font_search(font_search, verify, scores, pen_search, margins, pen_slack, baseline_search, whole_baseline)
        return _Modes(bool(scores), pen_search, whole_line, margins, pen_slack, baseline_search, whole_baseline, line_frac, font_search)

    def decode(self, luma_pages, x, y, width, line_height, line_advance, verify=None, scores=False, pen_search=0, pen_slack=0,
               baseline_search=0, whole_baseline=0, y_frac=0, line_advance_frac=0, font_search=False, margins=False, whole_line=False):
        """luma_pages: one (H, W) uint8 page, an (N, H, W) batch, or a list of pages (grouped by size into batches).
        Returns [[(y, text), ...] per page] in page order.  With verify="mse" or "image", returns (lines, mse, images):
        mse is focr --verify's red/blue MSE per page (f32, page order), images the (H, W, 3) verify image per page for
        "image" and None for "mse"; each size group is verified on the device right after its own decode.  With
        scores=True the result has one more element at its end: scores[page][line], the LineScores of lines[page][line].
        With pen_search=N > 0 (an extension, in 1/64 px up to 64; include/focr_decode.h) every step searches the pen
        offsets -N ..= N as well as the glyphs and carries the chosen offset forward; the result gains one last element,
        after the scores: offsets[page][line], an int8 array aligned with the line's text.  The verify then renders every
        character where it was decoded, and a LineScores' runner is the best candidate of another glyph.
        With whole_line=True (an extension for proportional fonts; include/focr_decode.h) every line is the text that
        minimises the whole line's squared error over pens on the 1/64 px grid, not the pen loop's greedy choice; the
        result gains two last elements: pens[page][line], a uint32 array of each character's pen in 1/64 px, and
        costs[page][line], the line's sum of footprint terms (int).  The verify then renders every character at its pen.
        It goes with neither scores nor pen_search.  With margins=True as well the result gains one more element after
        costs: margins[page][line], the LineMargins of lines[page][line]: which characters of the line to doubt.
        margins=True without whole_line raises ValueError.  With pen_slack=N > 0 as well (in 1/64 px up to 64, and at
        most half the font's smallest advance) every step of the whole-line decode may move the pen by an offset of -N ..= N
        before its glyph is rendered, for pages whose glyphs do not sit on this FreeType's 1/64 px pens; pens then holds
        each character's render pen and the result gains one last element after costs: offsets[page][line], an int8 array
        of the offset each character took.  It needs whole_line=True and does not go with margins.
        With baseline_search=N > 0 (an extension, up to 32; include/focr_decode.h) every line is decoded at the vertical
        offsets q in -N ..= N, in steps of 2^-y_bits px of the font's y_bits (set_font(..., y_bits=B)), and the candidate
        with the lowest summed footprint term is the line (on a tie the offset nearest 0).  The result gains two last
        elements: baselines[page][line], the chosen q (int), and costs[page][line], its sum of footprint terms (int).  The
        verify then draws each line moved by the nearest whole row of its offset.  It goes with none of scores, pen_search,
        whole_line, margins and pen_slack (ValueError).
        With whole_line=True and whole_baseline=N > 0 (up to 32) every line is decoded by the whole-line programme at the
        vertical offsets q in -N ..= N, in steps of 2^-y_bits px of the font's y_bits, and the candidate whose whole line
        costs least is the line (on a tie the offset nearest 0): proportional text whose baseline is off the crop grid.
        The result gains one last element after costs: baselines[page][line], the chosen q (int); pens and costs are that
        candidate's.  The verify renders every character at its pen on a canvas moved by the nearest whole row of the
        offset.  It needs whole_line=True and goes with neither margins nor pen_slack (ValueError).
        With y_frac and line_advance_frac (each 0 .. 63, in 1/64 px; include/focr_decode.h) beside baseline_search or
        whole_baseline, the lines lie on a fractional grid: line i's top is at y + y_frac / 64 + i * (line_advance +
        line_advance_frac / 64) px, its crop starts at the whole row of that (the y of the result's line), and its candidates
        are searched around its own sub-pixel part; the returned q is the absolute one, so y + q * 2^-y_bits px stays the
        line's top.  For pages whose leading is not a whole number of pixels.  Without either search: ValueError.
        With font_search=True (an extension; include/focr_decode.h) every line is decoded once in the decode font (candidate 0)
        and once in every font of set_font_candidates() (1 ..= K), by the plain pen loop, or by the whole-line decode with
        whole_line=True, and the candidate with the lowest summed footprint term is the line (on a tie the first).  The result
        gains two last elements: fonts[page][line], the winner's index (int), and costs[page][line], its sum of footprint
        terms (int); with whole_line=True it gains fonts alone, after costs, which are then the winner's.  It goes with none of
        scores, pen_search, margins, pen_slack, baseline_search, whole_baseline and verify, and needs candidates (ValueError)."""
        m = self._modes(verify, scores, pen_search, whole_line, margins, pen_slack, baseline_search, whole_baseline, y_frac, line_advance_frac, font_search)
        geo = (int(x), int(y), int(width), int(line_height), int(line_advance))
        pages = _page_list(luma_pages)
        out = _record(m, lambda: [None] * len(pages))
        mse = np.zeros(len(pages), dtype=np.float32)
        images = [None] * len(pages) if verify == "image" else None
        for (h, w), idx, batch in _size_groups(pages):
            r = self._run(C.c_void_p(batch.ctypes.data), False, len(idx), h, w, *geo, m)
            for all_pages, these in zip(out, r):
                for j, i in enumerate(idx if these is not None else ()):
                    all_pages[i] = these[j]
            if verify:
                mse[idx], imgs = self._verified(verify, h, w)
                for j, i in enumerate(idx if images is not None else ()):
                    images[i] = imgs[j]
        return self._assemble((mse, images) if verify else (), out)

    def decode_device(self, ptr, n_pages, page_h, page_w, x, y, width, line_height, line_advance, verify=None, scores=False,
                      pen_search=0, pen_slack=0, baseline_search=0, whole_baseline=0, y_frac=0, line_advance_frac=0, font_search=False,
                      margins=False, whole_line=False):
        """As decode(), for n_pages equal-size pages already in device memory at `ptr` (an address of the HIP runtime
        this library uses, on the decoder's device, written before the call and still valid for the verify)."""
        m = self._modes(verify, scores, pen_search, whole_line, margins, pen_slack, baseline_search, whole_baseline, y_frac, line_advance_frac, font_search)
        r = self._run(C.c_void_p(int(ptr)), True, int(n_pages), int(page_h), int(page_w), int(x), int(y), int(width), int(line_height),
                      int(line_advance), m)
        if not verify:
            return self._assemble((), r)
        mse, imgs = self._verified(verify, int(page_h), int(page_w))
        return self._assemble((mse, list(imgs) if imgs is not None else None), r)

    def close(self):
        if self._h is not None:
            self._lib.focr_decoder_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

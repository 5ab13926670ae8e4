"""What a caller feeds back to focr_decoder_score_text and focr_decoder_verify_text after every decode mode's seeded cases,
and what the two references say of it (tests/test_focr_text_fuzz_host.py on the CPU, tests/test_gpu_focr_text_fuzz.py on the
device).  No device here.

The families are the seeded cases the decoder's kernels have met before: "cases" (tests/focr_fuzz_cases.py, seven modes),
"fonts" (tests/focr_fonts_fuzz.py, two forms), "whole_baseline" (tests/focr_whole_baseline_fuzz.py) and "frac_base" /
"frac_whole" (focr_line_frac_cases.fuzz_case, the two baseline modes on a fractional line grid).  setup(family, i, mode) names
what a run needs (pages, geometry, the DecodeFonts 0 ..= K, y_bits); model_run(s) is the models' answer in the shapes
LineDecoder.decode returns, so that the same functions serve a device run's outputs; feed(s, got) is what DESIGN.md 4b-0's
table says a caller feeds back (pen_search: offsets; the whole kinds: pens, the render pens under a slack; the baseline kinds:
q with y_bits, on the fractional grid y = yc_i and the absolute q; the fonts kinds: fonts); reference_scores is
focr_score_text_model.score_text line by line in the DecodeFont of the line's k, reference_pictures is
focr_verify_text_model.verify_text page by page, and identity() holds a run's own numbers to a score of its outputs.

random_reading(family, i, page) is a reading of one page that no run produced, a function of SEED, the family, the case index
and the page alone: one to three lines as raw records (y, first, n_chars, font, q) into one character array, so that a line
can be listed twice and two lines can share characters (the records go to LineDecoder._score_text as they are; verify_text
takes the same lines as texts).  The text is random, 1 .. 2 x as many characters as fit the crop; a y is a slot's, a random
row, or the page's last row (a crop of one row); the placement is none, offsets of -8 ..= 8, or pens below 2^24 that are not
monotonic and of which some lie past 64 x the crop's width; a fonts case draws k of 0 ..= K per line (and, having no y-phase
fonts, whole rows q at y_bits 0 in every second case: the only q a candidate takes); a baseline case draws q over all of
int8 at its own y_bits; shift is a radius on every third case (the case's pen-search radius in "cases", the baseline radius
or a draw of 1 .. 8 elsewhere).  SEED was chosen so that the readings reach what tests/test_focr_text_fuzz_host.py asserts
they reach (a negative delta, a pen past the crop, a repeated line, shared characters, a winner at a shift other than 0).

Why none of the ranges drawn can read out of bounds (decode_score.hip, decode_pen.h, decode_text.hip and decode.h, as read):
  - a line's y: score_crop clamps it to page_h and gives min(line_height, page_h - y) rows, none where the crop has no
    column; score_stage reads rows below that and columns below g.w = min(width, page_w - x) only, and writes sdw * h dwords
    of a strip of stride * line_height bytes;
  - q: footprint_term_wide takes y0 = o.y + (q >> B) and walks the tile rows max(0, -y0) .. min(box_h, h - y0), so the strip
    row y0 + r lies in 0 .. h - 1 for every q of int8; v = q & (2^B - 1) is below the 2^B y-phase tables the host has
    checked to be uploaded (a fractional v on a candidate is refused on the host);
  - pens, offsets and the shift: a delta is an int of at most 2^22 + 2^24 + 64 in magnitude from pens, and from the f32
    pen about 64 x (2 x the crop's width + 1); term_dword drops a dword whose column `base` is not in -3 .. w - 1 and masks
    the edges, and for those bases reads the strip dwords (base + PAD) >> 2 and the next, at most (w + 3) / 4 + 1, inside
    the row's sdw = (w + 7) / 4 + 2; a negative delta gives phase delta & 63 and the floor delta >> 6, both in range;
  - the tile: rows below box_h of the phase's own tile, four dwords at a time while that stays below the font's end_dw,
    dword by dword past it;
  - verify_text: layout_line clips every glyph rectangle to its canvas and to the page (X0 >= x_start, X1 <= page_w,
    Y0 >= y, Y1 <= page_h) and points src at the clipped corner inside the phase rectangle; a pen below 0 widens the canvas to
    the left and the delta stays >= 0; mark_glyphs clips to the tile.  A y at or past page_h draws nothing.
So every draw is clipped, as include/focr_decode.h promises ("clipped to the crop on all four sides"), and none was narrowed.

The two FIXED geometries without a crop ("x-at-page-width": g.w == 0; "y-past-page": no slot): batch_geometry refuses
neither for score_text (it is called with one slot of its own), and the header says "an empty crop has line_base 0 and every
term 0": the runs return no line, and their random readings score (0, 0, 0) with zero terms (the model's empty canvas).
"""
import collections

import numpy as np

import focr_fonts_fuzz as FZ
import focr_fuzz_cases as FC
import focr_line_frac_cases as K
import focr_line_frac_model as LF
import focr_score_text_model as SM
import focr_verify_text_model as VT
import focr_whole_baseline_fuzz as WF
import focr_whole_baseline_model as WB
from focr_fast_model import crop

SEED = 0x7E87
FAMILIES = ("cases", "fonts", "whole_baseline", "frac_base", "frac_whole")
MODES = {"cases": FC.MODES, "fonts": FZ.FORMS, "whole_baseline": ("whole_baseline",), "frac_base": ("baseline_frac",),
         "frac_whole": ("whole_baseline_frac",)}
IDS = {"cases": tuple(range(FC.N_CASES)), "fonts": tuple(range(FZ.N_CASES)), "whole_baseline": tuple(range(WF.N_CASES)),
       "frac_base": K.FUZZ_IDS, "frac_whole": K.FUZZ_IDS}
DRAWN = ("cases", "fonts")  # the families whose runs verify_text can draw: the baseline kinds have no verify_text form

# case: the family's own record; fonts: the DecodeFonts 0 ..= K; geo: (x, y, width, line_height, line_advance); run: decode()'s switches
Setup = collections.namedtuple("Setup", "family index mode name case pages geo fonts alphabet y_bits run")


def setup(family, i, mode=None):
    """What a run of (family, case i, mode) needs; mode None is the family's first."""
    mode = MODES[family][0] if mode is None else mode
    assert mode in MODES[family], (family, mode)
    if family == "cases":
        c = FC.case(i)
        return Setup(family, i, mode, c.name, c, c.pages, c.geo, [FC.model(c).font], c.alphabet, 0, None)
    if family == "fonts":
        c = FZ.case(i)
        return Setup(family, i, mode, c.name, c, c.pages, c.geo, [m.font for m in FZ.models(c)], c.alphabet, 0, None)
    if family == "whole_baseline":
        c = WF.case(i)
        return Setup(family, i, mode, "wb-%d" % i, c, [c.page], c.geo, [K.fuzz_model(c).font], c.alphabet, c.y_bits,
                     dict(whole_line=True, whole_baseline=c.n))
    c = K.fuzz_case(family == "frac_whole", i)
    run = dict(whole_line=True, whole_baseline=c.n) if c.whole else dict(baseline_search=c.n)
    return Setup(family, i, mode, c.name, c, c.pages, c.geo, [K.fuzz_model(c).font], c.alphabet, c.y_bits,
                 dict(run, y_frac=c.frac[0], line_advance_frac=c.frac[1]))


def named(s, res):
    """decode()'s tuple of a baseline kind, named as the other families' runs are."""
    names = ("lines", "pens", "costs", "baselines") if "whole_line" in s.run else ("lines", "baselines", "costs")
    assert len(res) == len(names), (s.name, s.mode)
    return dict(zip(names, res))


def model_run(s):
    """The models' answer of a setup in the shapes LineDecoder.decode returns, named: lines and, where the mode has them,
    scores (records with base and score), offsets, pens, costs, margins (records with term), fonts, baselines."""
    if s.family == "cases":
        want = FC.want(s.case, s.mode)
        got = {"lines": [[(y, r if s.mode == "plain" else r.text) for y, r in pg] for pg in want]}
        per = lambda f: [[f(r) for _, r in pg] for pg in want]  # noqa: E731
        if s.mode in ("scores", "search_scores"):
            got["scores"] = per(lambda r: r)
        if s.mode in ("search", "search_scores", "slack"):
            got["offsets"] = per(lambda r: np.asarray(r.offsets, dtype=np.int8))
        if s.mode in FC.WHOLE_MODES:
            got["pens"], got["costs"] = per(lambda r: np.asarray(r.pens, dtype=np.uint32)), per(lambda r: int(r.cost))
        if s.mode == "margins":
            got["margins"] = per(lambda r: r)
        return got
    if s.family == "fonts":
        want = FZ.want(s.case, s.mode)
        got = {"lines": [[(y, r.text) for y, r in pg] for pg in want], "fonts": [[r.k for _, r in pg] for pg in want],
               "costs": [[int(r.cost) for _, r in pg] for pg in want]}
        if s.mode == "whole":
            got["pens"] = [[np.asarray(r.pens, dtype=np.uint32) for _, r in pg] for pg in want]
        return got
    if s.family == "whole_baseline":
        want = [WB.search_image(K.fuzz_model(s.case), p, *s.geo, s.case.n) for p in s.pages]
    else:
        want = K.fuzz_expected(s.case)
    got = {"lines": [[(y, r.text) for y, r in pg] for pg in want], "baselines": [[int(r.q) for _, r in pg] for pg in want],
           "costs": [[int(r.cost) for _, r in pg] for pg in want]}
    if s.family != "frac_base":
        got["pens"] = [[np.asarray(r.pens, dtype=np.uint32) for _, r in pg] for pg in want]
    return got


def feed(s, got):
    """What the row of DESIGN.md 4b-0's table feeds back beside the lines: score_text's keywords."""
    kw = {}
    if "pens" in got:  # the whole kinds; under a slack the render pens, and not the offsets beside them
        kw["pens"] = got["pens"]
    elif "offsets" in got:
        kw["offsets"] = got["offsets"]
    if "fonts" in got:
        kw["fonts"] = got["fonts"]
    if "baselines" in got:
        kw["baselines"], kw["y_bits"] = got["baselines"], s.y_bits
    return kw


def reference_scores(s, lines, fonts=None, pens=None, offsets=None, baselines=None, y_bits=0, shift=0):
    """focr_score_text_model.score_text of every line, [page][line], in the DecodeFont of the line's k."""
    x, _, width, lh, _ = s.geo
    return [[SM.score_text(s.fonts[fonts[p][n] if fonts is not None else 0], page, x, y, width, lh, text, None if pens is None else pens[p][n],
                           None if offsets is None else offsets[p][n], 0 if baselines is None else baselines[p][n], y_bits, shift)
             for n, (y, text) in enumerate(lines[p])] for p, page in enumerate(s.pages)]


def identity(s, got, scores):
    """The row's `must equal` column: a score of a run's outputs against the run's own numbers, by ==."""
    for p, pg in enumerate(got["lines"]):
        assert len(scores[p]) == len(pg), (s.name, s.mode, p)
        for n, (y, text) in enumerate(pg):
            at, g = (s.family, s.name, s.mode, p, y), scores[p][n]
            assert g.shift == 0 and len(g.terms) == len(text) and g.cost == int(np.asarray(g.terms, dtype=np.int64).sum()), at
            if "scores" in got:
                sc = got["scores"][p][n]
                assert g.base == sc.base, at + ("base", g.base, sc.base)
                assert np.array_equal(g.terms, np.asarray(sc.score, dtype=np.int64) - sc.base), at + ("terms",)
            if "costs" in got:
                assert g.cost == got["costs"][p][n], at + ("cost", g.cost, got["costs"][p][n])
            if "margins" in got:
                assert np.array_equal(g.terms, got["margins"][p][n].term), at + ("margins",)


def vt_fonts(s):
    return [VT.Font(f.font_path, f.text_size, f.hinting, f.kerning) for f in s.fonts]


def reference_pictures(s, lines, fonts=None, pens=None, offsets=None, pages=None):
    """focr_verify_text_model.verify_text of every page (or of the pages listed): [(image, sum)]."""
    fs = vt_fonts(s)
    return [VT.verify_text(s.pages[p], [VT.Line(y, text, fonts[p][n] if fonts is not None else 0, None if pens is None else pens[p][n],
                                               None if offsets is None else offsets[p][n]) for n, (y, text) in enumerate(lines[p])],
                           fs, s.alphabet, s.geo[0]) if pages is None or p in pages else None for p in range(len(s.pages))]


def picture_feed(kw):
    """verify_text's keywords of score_text's."""
    return {k: v for k, v in kw.items() if k in ("fonts", "pens", "offsets")}


def strip_bytes(s, page):
    """The strip of a line of this page, as focr_decoder_score_text sizes it; with 128 bytes of sums it must fit 65536."""
    return K.strip_bytes(page.shape[1], s.geo[0], s.geo[2], s.geo[3])


# ---- readings no run produced -----------------------------------------------------------------------------------------------

# recs: [(y, first, n_chars, font, q)] into chars; along: the pens or offsets beside chars (None: the pen loop's placement)
Reading = collections.namedtuple("Reading", "page recs chars placement along with_q y_bits shift")


def slot_rows(s, page):
    x, y, width, lh, la = s.geo
    H = page.shape[0]
    if s.family.startswith("frac"):
        return [sl.yc for sl in LF.slots(H, y, s.case.frac[0], lh, la, s.case.frac[1])]
    return list(range(y, H, la)) if lh else []


def random_reading(family, i, page):
    """A reading of page `page` of case i that no run produced (the module docstring says what is drawn)."""
    s = setup(family, i)
    n = IDS[family].index(i)
    rng = np.random.default_rng([SEED, FAMILIES.index(family), n, page])
    luma = s.pages[page]
    H, Wp = luma.shape
    x, _, width, lh, _ = s.geo
    w = min(width, Wp - min(x, Wp))
    incs = s.fonts[0].increments()
    fit = max(1, int(np.ceil(max(w, 1) / float(np.mean(incs)))))
    n_chars = int(rng.integers(fit, 2 * fit + 1))
    chars = [int(c) for c in rng.integers(0, len(s.alphabet), n_chars)]
    rows = slot_rows(s, luma)

    def row():
        u = rng.random()
        if u < 0.4 and rows:
            return int(rows[int(rng.integers(0, len(rows)))])
        return H - 1 if u < 0.6 else int(rng.integers(0, H + 2))  # H and H + 1: an empty crop

    K_ = len(s.fonts) - 1
    baseline = "baseline" in s.mode
    with_q = baseline or (family == "fonts" and n % 2 == 1)
    y_bits = s.y_bits if baseline else 0

    def font_q():
        k = int(rng.integers(0, K_ + 1))
        if not with_q:
            return k, 0
        return k, int(rng.integers(-128, 128)) if rng.random() < 0.5 else int(rng.integers(-3 << y_bits, (3 << y_bits) + 1))

    recs = [(row(), 0, int(rng.integers(max(1, n_chars // 2), n_chars + 1))) + font_q()]
    for _ in range(int(rng.integers(0, 3))):
        u = rng.random()
        if u < 0.4:
            recs.append(recs[int(rng.integers(0, len(recs)))])  # a line listed twice
        else:  # a range of its own choosing, which shares characters with every line it overlaps
            first = int(rng.integers(0, n_chars))
            recs.append((row(), first, int(rng.integers(1, n_chars - first + 1))) + font_q())
    placement = ("none", "offsets", "pens")[int(rng.integers(0, 3))]
    along = None
    if placement == "offsets":
        along = [int(v) for v in rng.integers(-8, 9, n_chars)]
    elif placement == "pens":
        along = []
        for _ in range(n_chars):
            u = rng.random()
            lo, hi = (0, 64 * max(w, 1)) if u < 0.7 else (64 * w, 64 * w + 1024) if u < 0.85 else (64 * w, 1 << 24)
            along.append(int(rng.integers(lo, hi)))
    shift = 0
    if n % 3 == 0:
        shift = s.case.radius if family == "cases" else s.case.n if baseline else int(rng.integers(1, 9))
    return Reading(page, recs, chars, placement, along, with_q, y_bits, shift)


def reading_lines(s, r):
    """A reading as score_text and verify_text take it from Python, one page: (lines, keywords)."""
    text = lambda first, n: "".join(s.alphabet[c] for c in r.chars[first: first + n])  # noqa: E731
    lines = [(y, text(first, n)) for y, first, n, _, _ in r.recs]
    kw = {}
    if len(s.fonts) > 1:
        kw["fonts"] = [[k for _, _, _, k, _ in r.recs]]
    if r.placement != "none":
        kw[r.placement] = [[r.along[first: first + n] for _, first, n, _, _ in r.recs]]
    return [lines], kw


def reading_scores(s, r):
    """focr_score_text_model.score_text of every record of a reading, with its shift."""
    x, _, width, lh, _ = s.geo
    out = []
    for y, first, n, k, q in r.recs:
        at = None if r.along is None else r.along[first: first + n]
        out.append(SM.score_crop(s.fonts[k], crop(s.pages[r.page], x, y, width, lh), r.chars[first: first + n], at if r.placement == "pens" else None,
                                 at if r.placement == "offsets" else None, q, r.y_bits, r.shift))
    return out


def reading_deltas(s, r, scores):
    """FreeType's deltas of every record at its winning shift."""
    out = []
    for (y, first, n, k, q), sc in zip(r.recs, scores):
        at = None if r.along is None else r.along[first: first + n]
        out.append(SM.deltas(s.fonts[k], r.chars[first: first + n], at if r.placement == "pens" else None, at if r.placement == "offsets" else None, sc.shift))
    return out


def reading_picture(s, r):
    """focr_verify_text_model.verify_text of a reading's page (a reading without q)."""
    lines, kw = reading_lines(s, r)
    fonts, pens, offsets = kw.get("fonts"), kw.get("pens"), kw.get("offsets")
    return VT.verify_text(s.pages[r.page], [VT.Line(y, text, fonts[0][n] if fonts else 0, None if pens is None else pens[0][n],
                                                    None if offsets is None else offsets[0][n]) for n, (y, text) in enumerate(lines[0])],
                          vt_fonts(s), s.alphabet, s.geo[0])

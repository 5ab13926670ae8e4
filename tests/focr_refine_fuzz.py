"""What a caller feeds to focr_decoder_refine_text after every decode mode's seeded cases, and what its model says of it
(tests/test_focr_refine_fuzz_host.py on the CPU, tests/test_gpu_focr_refine_fuzz.py on the device).  No device here.

The families are focr_text_fuzz.DRAWN: "cases" (tests/focr_fuzz_cases.py, seven modes) and "fonts" (tests/focr_fonts_fuzz.py, two
forms); refine_text has no line_q, so the baseline families stay out.  pens_of(s, got) is the rule of LineDecoder.refine_text's
docstring: a whole kind's pens (under a slack the render pens), placed_pens of a plain reading or of a pen search's offsets, in the
line's own font.  draw(family, i, mode) is the call's (radius, sweeps, glyphs), a function of SEED, the family, the case index and
the mode alone; cut(...) says whether the lines go in cut to their first CUT characters (a radius above 7 with more than two sweeps:
the model's time).  reading(family, i, page) is focr_text_fuzz.random_reading with its pens made acceptable: records, characters,
ys and fonts as they are (lines listed twice, shared characters, a crop of one row, empty crops, k of 0 ..= K), one pen array beside
the characters that does not decrease, so that every record's slice is sorted even where records share characters: placed_pens in
the decode font (the offsets applied, then a running maximum), or the drawn pens sorted once, pens past 64 x the crop's width kept.

refine_line() is focr_refine_model.refine_crop with every step noted (what won it and what tied); reference() and
reading_reference() run it line by line in the FastModel of the line's k.  compose_within() composes only the characters that the
kernel's neighbour scan admits (decode_refine.hip step (1), refine_plan.h): the host test holds it to the plain model.

SEED was chosen so that the cases and readings reach what tests/test_focr_refine_fuzz_host.py asserts they reach.
"""
import collections

import numpy as np

import focr_fonts_fuzz as FZ
import focr_fuzz_cases as FC
import focr_refine_model as R
import focr_text_fuzz as TF
from focr_fast_model import crop
from focr_search_model import rank
from font_ocr_amd import placed_pens

SEED = 0x4EF1
FAMILIES = TF.DRAWN
MODES = {f: TF.MODES[f] for f in FAMILIES}
IDS = {f: TF.IDS[f] for f in FAMILIES}
RADII = (0, 1, 2, 4, 7, 33, 64)
SWEEPS = (0, 1, 2, 3, 8)
CUT = 6
STRIP_PAD = 4  # refine_plan.h's REFINE_STRIP_PAD
GROUP = 6      # cases per group, as tests/test_gpu_focr_text_fuzz.py has them
GROUPS = [(f, list(IDS[f][a: a + GROUP])) for f in FAMILIES for a in range(0, len(IDS[f]), GROUP)]
GROUP_IDS = ["%s%s-%s" % (f, g[0], g[-1]) for f, g in GROUPS]
# the lines every mode's run returns, over all cases (the models'; tests/test_focr_refine_fuzz_host.py holds them to it), and the
# records of all the readings: what the device module must have compared
LINES = {"cases": 212, "fonts": 156}
RECORDS = 313

# What one line's steps reached.  glyph / pen: steps won by another glyph / at another pen; late: a step of a later sweep that changed a
# character every earlier sweep left alone; tie_rank / tie_glyph: a winning step where another candidate had the winner's D at
# another pen (the rank decided) / at the winner's pen (the glyph index decided); tie_inc: a step where the lowest key belonged to
# another candidate than the incumbent, at the incumbent's D (the incumbent stays); neg_pen: a step with a candidate pen below 0.
NOTES = ("glyph", "pen", "late", "tie_rank", "tie_glyph", "tie_inc", "neg_pen")


def models(s):
    """The FastModels of the setup's fonts 0 ..= K."""
    return [FC.model(s.case)] if s.family == "cases" else FZ.models(s.case)


def _key(mode):
    if isinstance(mode, int):  # a reading's page
        return 64 + mode
    return (FC.MODES + FZ.FORMS).index(mode)


def draw(family, i, mode):
    """(radius, sweeps, glyphs) of the call that refines (family, case i, mode); mode is a page number for the case's reading."""
    rng = np.random.default_rng([SEED, FAMILIES.index(family), IDS[family].index(i), _key(mode)])
    u = rng.random()
    radius = RADII[5 + int(rng.integers(0, 2))] if u < 0.12 else RADII[int(rng.integers(0, 5))]
    sweeps = SWEEPS[int(rng.integers(0, len(SWEEPS)))]
    return radius, sweeps, bool(rng.random() >= 0.25)


def cut(family, i, mode):
    """The characters a line of the call keeps (its first CUT), or None: all."""
    radius, sweeps, _ = draw(family, i, mode)
    return CUT if radius > 7 and sweeps > 2 else None


def pens_of(s, got):
    """[[pens per line] per page] a caller feeds back for a run's output `got` (focr_text_fuzz.model_run's shapes)."""
    out = []
    for p, pg in enumerate(got["lines"]):
        out.append([])
        for n, (_, text) in enumerate(pg):
            if "pens" in got:  # the whole kinds; under a slack the render pens
                pens = np.asarray(got["pens"][p][n], dtype=np.int64)
            else:
                font = s.fonts[got["fonts"][p][n] if "fonts" in got else 0]
                pens = placed_pens(font, text, got["offsets"][p][n] if "offsets" in got else None)
            # a pen search at origin_x 0 whose first offset is negative places its first character left of 0: refine_text's pens are
            # unsigned, and all a caller can feed is 0 (below_zero() counts these; the host test pins how many there are)
            at = (s.family, s.name, s.mode, p, n)
            assert len(pens) == len(text), at + ("one pen per character",)
            assert np.all(np.diff(pens) >= 0), at + ("a run's pens decrease", pens.tolist())  # on the pens as the run gave them
            assert len(pens) == 0 or pens[-1] < R.PEN_END, at + ("a pen at 2^24 or beyond",)
            out[-1].append([int(v) for v in np.maximum(pens, 0)])
    return out


def below_zero(s, got):
    """The characters of a run's output that placed_pens puts left of pen 0 (pens_of feeds them at 0)."""
    if "pens" in got:
        return 0
    return sum(int((placed_pens(s.fonts[got["fonts"][p][n] if "fonts" in got else 0], text, got["offsets"][p][n] if "offsets" in got else None) < 0).sum())
               for p, pg in enumerate(got["lines"]) for n, (_, text) in enumerate(pg))


def fed(s, got):
    """(lines, pens, fonts or None, radius, sweeps, glyphs): refine_text's arguments after a run, the lines cut where cut() says."""
    radius, sweeps, glyphs = draw(s.family, s.index, s.mode)
    n = cut(s.family, s.index, s.mode)
    pens = [[ps[:n] for ps in pg] for pg in pens_of(s, got)]
    lines = [[(y, text[:n]) for y, text in pg] for pg in got["lines"]]
    return lines, pens, got.get("fonts"), radius, sweeps, glyphs


# ---- the model, every step noted ----------------------------------------------------------------------------------------------

def refine_line(fm, ref, idx, pens, radius, sweeps, glyphs, canvas=None):
    """(focr_refine_model.Refine, Counter over NOTES) of one line; canvas as refine_crop's."""
    h, w = ref.shape if ref.size else (0, 0)
    compose = canvas or (lambda idx_, pens_, skip=None: R.compose(fm.font, idx_, pens_, h, w, skip))
    steps = []

    def noted_canvas(idx_, pens_, skip=None):
        if skip is not None:
            steps.append((skip, idx_[skip], pens_[skip], []))
        return compose(idx_, pens_, skip)

    def noted_terms(fm_, r, o, pen):
        t = R.stack_terms(fm_, r, o, pen)
        steps[-1][3].append((pen, t))
        return t

    got = R.refine_crop(fm, ref, idx, pens, radius, sweeps, glyphs, terms=noted_terms, canvas=noted_canvas)
    notes, n, touched = collections.Counter(), len(idx), set()
    for k, (g, a0, s0, ts) in enumerate(steps):
        inc = int(ts[0][1][a0])
        keys = sorted((int(t[a]), rank(pen - s0), a) for pen, t in ts[1:] for a in (range(len(t)) if glyphs else [a0]))
        best = keys[0]
        if len(ts) - 1 < 2 * radius + 1:
            notes["neg_pen"] += 1
        if best[0] < inc:
            notes["glyph"] += best[2] != a0
            notes["pen"] += best[1] != 0
            notes["late"] += k >= n and g not in touched
            touched.add(g)
            notes["tie_rank"] += any(d == best[0] and r != best[1] for d, r, _ in keys[1:])
            notes["tie_glyph"] += any(d == best[0] and r == best[1] for d, r, _ in keys[1:])
        elif best[1:] != (0, a0):
            assert best[0] == inc
            notes["tie_inc"] += 1
    return got, notes


def reference(s, lines, pens, fonts, radius, sweeps, glyphs):
    """[[(Refine, notes) per line] per page] of a call after a run."""
    x, _, width, lh, _ = s.geo
    ms = models(s)
    out = []
    for p, page in enumerate(s.pages):
        out.append([])
        for n, (y, text) in enumerate(lines[p]):
            fm = ms[fonts[p][n] if fonts is not None else 0]
            out[-1].append(refine_line(fm, crop(page, x, y, width, lh), [s.alphabet.index(c) for c in text], pens[p][n], radius, sweeps, glyphs))
    return out


_runs = {}


def model_fed(family, i, mode):
    """(setup, the models' run, fed(), reference()) of (family, case i, mode), computed once."""
    key = (family, i, mode)
    if key not in _runs:
        s = TF.setup(family, i, mode)
        got = TF.model_run(s)
        args = fed(s, got)
        _runs[key] = (s, got, args, reference(s, *args))
    return _runs[key]


# ---- readings no run produced ---------------------------------------------------------------------------------------------------

Reading = collections.namedtuple("Reading", "page recs chars pens placement")  # recs: (y, first, n_chars, font) into chars and pens


def reading(family, i, page):
    """focr_text_fuzz.random_reading of page `page` of case i with pens refine_text accepts."""
    s = TF.setup(family, i)
    r = TF.random_reading(family, i, page)
    text = "".join(s.alphabet[c] for c in r.chars)
    if r.placement == "pens":
        pens = sorted(int(v) for v in r.along)
    else:
        pens = np.maximum.accumulate(placed_pens(s.fonts[0], text, r.along if r.placement == "offsets" else None))
        pens = [int(v) for v in np.maximum(pens, 0)]
    assert all(a <= b for a, b in zip(pens, pens[1:])) and (not pens or 0 <= pens[0] and pens[-1] < R.PEN_END)
    return Reading(page, [rec[:4] for rec in r.recs], list(r.chars), pens, r.placement)


_readings = {}


def reading_reference(family, i, page):
    """(setup, Reading, (radius, sweeps, glyphs), [(Refine, notes) per record]) of a case's reading, computed once."""
    key = (family, i, page)
    if key not in _readings:
        s = TF.setup(family, i)
        r = reading(family, i, page)
        x, _, width, lh, _ = s.geo
        ms = models(s)
        par = draw(family, i, page)
        n = cut(family, i, page)
        if n is not None:  # the records cut as a run's lines are
            r = r._replace(recs=[(y, first, min(m, n), k) for y, first, m, k in r.recs])
        _readings[key] = (s, r, par, [refine_line(ms[k], crop(s.pages[page], x, y, width, lh), r.chars[first: first + m], r.pens[first: first + m], *par)
                                      for y, first, m, k in r.recs])
    return _readings[key]


# ---- the kernel's neighbour bound -------------------------------------------------------------------------------------------------

def extent(font):
    """refine_plan.h's refine_extent of a DecodeFont: (x_lo, x_hi) over every glyph and phase, off_x and off_x + stride."""
    g = font.s.glyphs
    xs = [(int(g[i].off_x[p]), int(g[i].off_x[p]) + int(g[i].stride)) for i in range(font.s.n_glyphs) for p in range(64)]
    return min(a for a, _ in xs), max(b for _, b in xs)


def step_window(font, ext, pen, radius, w):
    """The columns (cx0, cx1) of the window of a step at `pen`, as refine_text_kernel lays it out in whole strip dwords; None where no
    candidate reaches the crop's w columns."""
    od = 64 * int(font.origin[0])
    wx0, wx1 = max(0, ((od + pen - radius) >> 6) + ext[0]), min(w, ((od + pen + radius) >> 6) + ext[1])
    if wx0 >= wx1:
        return None
    q0 = (wx0 + STRIP_PAD - 3) >> 2  # refine_row_dwords
    dw = ((wx1 - 1 + STRIP_PAD) >> 2) + 1 - q0 + 1
    return 4 * q0 - STRIP_PAD, 4 * q0 - STRIP_PAD + 4 * dw


def compose_within(font, ext, idx, pens, pens_in, slack, window, skip, h, w):
    """The canvas of the characters the kernel's scan admits to the step of character `skip`: outwards from it over the input pens
    pens_in, with the font-wide extent, up to the first character whose box at pens_in -+ slack cannot reach the window's columns."""
    od = 64 * int(font.origin[0])
    lo, hi = skip, skip + 1
    while lo > 0 and ((od + pens_in[lo - 1] + slack) >> 6) + ext[1] > window[0]:
        lo -= 1
    while hi < len(idx) and ((od + pens_in[hi] - slack) >> 6) + ext[0] < window[1]:
        hi += 1
    v = np.zeros((h, w), dtype=np.int64)
    for g in range(lo, hi):
        box = None if g == skip else R.clipped(font, idx[g], pens[g], h, w)
        if box is not None:
            ya, yb, xa, xb, c = box
            np.maximum(v[ya:yb, xa:xb], c, out=v[ya:yb, xa:xb])
    return v


def refine_within(fm, ref, idx, pens, radius, sweeps, glyphs, slack):
    """refine_line on the canvas of compose_within at `slack`: the kernel's pruning rule in place of the definition's every character."""
    h, w = ref.shape if ref.size else (0, 0)
    ext, pens_in = extent(fm.font), [int(v) for v in pens]

    def canvas(idx_, pens_, skip=None):
        if skip is None:
            return R.compose(fm.font, idx_, pens_, h, w)
        window = step_window(fm.font, ext, pens_[skip], radius, w)
        if window is None:  # the kernel skips the step: every D is 0 on any canvas
            return np.zeros((h, w), dtype=np.int64)
        return compose_within(fm.font, ext, idx_, pens_, pens_in, slack, window, skip, h, w)

    return refine_line(fm, ref, idx, pens, radius, sweeps, glyphs, canvas=canvas)

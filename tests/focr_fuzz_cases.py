"""Seeded cases for every mode of the focr line decoder off its default font setup, and what the models say of them
(tests/test_focr_fuzz_cases_host.py on the CPU, tests/test_gpu_focr_fuzz.py on the device).

build(i) is a function of the case index and SEED alone (np.random.default_rng([SEED, i])).  A random case draws a font
(Sans, Serif, Mono in turn), a size, a kerning, hinting (on in every second triple of cases, so each font meets both),
an alphabet of 2 .. 12 characters of ASCII95, a run geometry (x, y, width, line_height, line_advance, a page that may clip
the width and whose bottom edge cuts the last slot), one to three pages that may have two sizes and a blank one in the
middle, a pen-search radius and a pen slack.  The ink is lines of random alphabet characters, each glyph one FreeType
raster at the case's hinting on the decoder's own line canvas: the pen starts at a random sub-pixel position, every
advance is scaled by 0.97 .. 1.03, the baseline is moved by up to 0.4 px, and 2 % of the band's pixels are salted.
Behind the random cases comes FIXED, geometries a draw rarely hits.  Nothing here comes from the device path.

want(case, mode) is the models' answer, cached: FastModel.decode_image, focr_scores_model.image_scores,
focr_search_model.search_image, and focr_whole_model.whole_image's page walk over whole_line, margins_line and slack_line.
"""
import collections
import os

import numpy as np

import focr_margins_model as MM
import focr_scores_model as SC
import focr_search_model as S
import focr_slack_model as K
import focr_whole_model as W
from focr_fast_model import ASCII95, FastModel, crop
from font_ocr_amd.decoder import raster_glyph

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FONTS = tuple(os.path.join(GOLD, f) for f in ("DejaVuSans.ttf", "DejaVuSerif.ttf", "DejaVuSansMono.ttf"))
SANS, SERIF, MONO = FONTS
SIZES = (6.0, 7.15, 9.0, 11.5, 13.0, 17.3, 24.0)
KERNINGS = (0.6, 0.85, 1.0, 1.07, 1.3)
DEFAULT_SEED = 0xF0C2
SEED = int(os.environ.get("FOCR_FUZZ_SEED", str(DEFAULT_SEED)), 0)
N_RANDOM = 36
MODES = ("plain", "scores", "search", "search_scores", "whole", "margins", "slack")
WHOLE_MODES = ("whole", "margins", "slack")
WHOLE_BATCH_MAX = 512   # decode_whole.hip: states per batch at most
WHOLE_RING_MAX = 4096   # decode_whole.hip: keys of the cost ring at most

# name -> what the draw is replaced by.  x_at_width and y_past_page move the run's start after the pages are drawn.
FIXED = (
    ("x-at-page-width", dict(x_at_width=True, pages=2)),          # every crop empty (g.w == 0): every line skipped, three launches
    ("y-past-page", dict(y_past_page=True, pages=2)),             # no slot: total == 0, nothing launched
    ("one-column", dict(width=1)),
    ("line-height-1", dict(line_height=1, line_advance=3)),
    ("advance-1-height-12", dict(font=SANS, size=9.0, width=16, line_height=12, line_advance=1, slots=14, pages=1)),  # every slot overlaps the next eleven
    ("min-inc64-above-512", dict(font=MONO, size=24.0, kerning=1.3, alphabet="AB >x", width=48, line_height=28)),     # 1202: batches of 512, mostly empty
    ("min-inc64-below-64", dict(font=SERIF, size=6.0, kerning=0.6, alphabet="'il.aJ")),                               # 63
)
N_CASES = N_RANDOM + len(FIXED)

Case = collections.namedtuple("Case", "index name font size kerning hinting alphabet geo pages radius slack")


def _alphabet(rng):
    """2 .. 12 distinct characters of ASCII95, in drawn order; in one draw of three the first comes from "jJTYAVvy", the
    glyphs that reach left of the pen in Sans or Serif (origin_x = 1)."""
    n = int(rng.integers(2, 13))
    al = [ASCII95[k] for k in rng.permutation(len(ASCII95))[:n]]
    if rng.random() < 1 / 3:
        c = "jJTYAVvy"[int(rng.integers(0, 8))]
        if c not in al:
            al[0] = c
    return "".join(al)


def _ink_line(rng, page, fm, case_font, size, hinting, x, ly):
    """Darken `page` from (x, ly) with a line of random alphabet characters: each glyph one raster_glyph on the decoder's
    line canvas at a pen that starts inside the first pixel and advances by increment * (0.97 .. 1.03), the baseline
    moved by up to 0.4 px; then 2 % of the band's pixels take a random luma."""
    H, Wp = page.shape
    h, w = min(int(np.ceil(size)) + 4, H - ly), Wp - min(x, Wp)
    if h <= 0 or w <= 0:
        return
    ox, oy = fm.font.origin
    ty = F32(oy + F32(rng.uniform(-0.4, 0.4)))
    pen = F32(rng.uniform(0.0, 1.0))
    band = page[ly: ly + h, x: x + w]
    while pen < F32(w):
        i = int(rng.integers(0, len(fm.alphabet)))
        g = np.zeros((h, w), dtype=np.uint8)
        raster_glyph(case_font, size, fm.alphabet[i], F32(ox + pen), ty, g, hinting)
        np.minimum(band, 255 - g, out=band)
        pen = F32(pen + F32(fm.incs[i] * F32(rng.uniform(0.97, 1.03))))
    salt = rng.random(band.shape) < 0.02
    band[salt] = rng.integers(0, 255, int(salt.sum()), dtype=np.uint8)


_fast = {}


def fast(font, size, alphabet, hinting, kerning):
    """The FastModel of a font setup, built once."""
    key = (font, float(size), alphabet, bool(hinting), float(kerning))
    if key not in _fast:
        _fast[key] = FastModel(font, size, alphabet, hinting, kerning)
    return _fast[key]


def model(case):
    return fast(case.font, case.size, case.alphabet, case.hinting, case.kerning)


def build(i):
    """Case i: random below N_RANDOM, FIXED[i - N_RANDOM] on a random base above."""
    rng = np.random.default_rng([SEED, i])
    name, fix = ("random", {}) if i < N_RANDOM else FIXED[i - N_RANDOM]
    font = fix.get("font", FONTS[i % 3])
    hinting = bool((i // 3) % 2)
    size = float(SIZES[int(rng.integers(0, len(SIZES)))])
    kerning = float(KERNINGS[int(rng.integers(0, len(KERNINGS)))])
    alphabet = _alphabet(rng)
    size, kerning, alphabet = fix.get("size", size), fix.get("kerning", kerning), fix.get("alphabet", alphabet)
    fm = fast(font, size, alphabet, hinting, kerning)
    x, y, width = int(rng.integers(0, 6)), int(rng.integers(0, 5)), int(rng.integers(12, 49))
    line_height = max(1, int(round(size * rng.uniform(0.6, 1.6))))
    line_advance = max(1, line_height + int(rng.integers(-3, 4)))
    clip = int(rng.integers(1, 5)) if rng.random() < 0.4 else 0  # the page ends this many columns inside x + width
    slots = int(rng.integers(2, 5))
    n_pages = int(rng.integers(1, 4))
    two_sizes = n_pages > 1 and rng.random() < 0.5
    blank_middle = n_pages == 3 and rng.random() < 0.5
    width, line_height = fix.get("width", width), fix.get("line_height", line_height)
    line_advance, slots, n_pages = fix.get("line_advance", line_advance), fix.get("slots", slots), fix.get("pages", n_pages)
    if fix:
        two_sizes, blank_middle, clip = False, False, 0
    # slots - 1 whole advances and a last slot that the bottom edge cuts (where line_height > 1 leaves something to cut)
    cut = int(rng.integers(1, max(2, min(line_height - 1, line_advance) + 1)))
    Wp, Hp = max(1, x + width - clip), y + (slots - 1) * line_advance + cut
    pages = []
    for p in range(n_pages):
        shape = (Hp + int(rng.integers(0, line_advance + 1)), Wp + int(rng.integers(1, 4))) if two_sizes and p == 1 else (Hp, Wp)
        page = np.full(shape, 255, dtype=np.uint8)
        n = -(-(shape[0] - y) // line_advance)
        inked = rng.random(n) < 0.3
        inked[int(rng.integers(0, n))] = True
        for s in np.flatnonzero(inked) if not (blank_middle and p == 1) else ():
            _ink_line(rng, page, fm, font, size, hinting, x, y + int(s) * line_advance)
        pages.append(page)
    radius = int(rng.integers(1, min(64, S.max_radius(fm.incs)) + 1))
    slack = int(rng.integers(1, min(16, K.max_slack(fm.incs)) + 1))
    if fix.get("x_at_width"):
        x = Wp
    if fix.get("y_past_page"):
        y = Hp + int(rng.integers(0, 3))
    return Case(i, "%d-%s" % (i, name), font, size, kerning, hinting, alphabet, (x, y, width, line_height, line_advance), pages, radius, slack)


_cases = {}


def case(i):
    if i not in _cases:
        _cases[i] = build(i)
    return _cases[i]


def crops(c, page):
    """[(y, crop)] of every slot of a page with a non-empty crop, as the reference's loop visits them."""
    x, y, width, line_height, line_advance = c.geo
    out, i = [], 0
    while True:
        ly = y + i * line_advance
        i += 1
        line = crop(page, x, ly, width, line_height)
        if line.shape[0] == 0:
            return out
        out.append((ly, np.ascontiguousarray(line)))


def plan(c):
    """What decode_whole.hip's whole_plan derives for the case: the width of its widest crop, min and max inc64, the batch
    length without and with the slack, and the keys the slack's ring must hold."""
    inc = W.inc64(model(c).incs)
    lo, hi = int(inc.min()), int(inc.max())
    w = max(min(c.geo[2], p.shape[1] - min(c.geo[0], p.shape[1])) for p in c.pages)
    return dict(w=w, lo=lo, hi=hi, batch=min(lo, WHOLE_BATCH_MAX), slack_batch=min(lo - c.slack, WHOLE_BATCH_MAX),
                ring=min(lo - c.slack, WHOLE_BATCH_MAX) + 2 * c.slack + hi)


_want = {}


def want(c, mode):
    """The models' answer of a case in a mode: [[(y, result)] per page], result a text ("plain"), a Scored, a Searched
    (both search modes), a Whole, a Margins or a Slack."""
    mode = "search" if mode == "search_scores" else mode
    key = (c.index, mode)
    if key not in _want:
        fm = model(c)
        if mode == "plain":
            out = [fm.decode_image(p, *c.geo) for p in c.pages]
        elif mode == "scores":
            out = [SC.image_scores(fm, p, *c.geo) for p in c.pages]
        elif mode == "search":
            out = [S.search_image(fm, p, *c.geo, c.radius) for p in c.pages]
        else:
            line = {"whole": lambda ref: W.whole_line(fm, ref), "margins": lambda ref: MM.margins_line(fm, ref),
                    "slack": lambda ref: K.slack_line(fm, ref, c.slack)}[mode]
            out = [[(y, line(ref)) for y, ref in crops(c, p) if not np.all(ref == 255)] for p in c.pages]
        _want[key] = out
    return _want[key]


# ---- a case on a LineDecoder (the device tests') ---------------------------------------------------------------------------

SWITCHES = {"plain": {}, "scores": dict(scores=True), "search": dict(pen_search=True), "search_scores": dict(pen_search=True, scores=True),
            "whole": dict(whole_line=True), "margins": dict(whole_line=True, margins=True), "slack": dict(whole_line=True, pen_slack=True)}


def run(dec, c, mode, verify=None):
    """decode() of a case in a mode, its result named: lines, (mse, images,) scores, offsets, pens, costs, margins."""
    kw = dict(SWITCHES[mode])
    if "pen_search" in kw:
        kw["pen_search"] = c.radius
    if "pen_slack" in kw:
        kw["pen_slack"] = c.slack
    fm = model(c)
    if dec.font is not fm.font:
        dec.set_font(fm.font, c.size)
    grid = 1 + (c.index // 2) % 2 if c.index % 2 and mode in WHOLE_MODES else 0  # several lines through one workgroup
    assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, grid) == 0, (c.name, mode)
    try:
        res = dec.decode(c.pages, *c.geo, verify=verify, **kw)
    finally:
        assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 0) == 0, (c.name, mode)
    res = res if isinstance(res, tuple) else (res,)
    names = ["lines"] + (["mse", "images"] if verify else []) + [n for n, on in (
        ("scores", "scores" in kw), ("offsets", "pen_search" in kw), ("pens", "whole_line" in kw), ("costs", "whole_line" in kw),
        ("margins", "margins" in kw), ("offsets", "pen_slack" in kw)) if on]
    assert len(res) == len(names), (c.name, mode)
    return dict(zip(names, res))


def last_batch(c):
    """The pages of the size group that decode() runs last, and whether that run has any line slot."""
    shapes = list(dict.fromkeys(p.shape for p in c.pages))
    idx = [i for i, p in enumerate(c.pages) if p.shape == shapes[-1]]
    return idx, c.geo[3] > 0 and c.geo[1] < shapes[-1][0]

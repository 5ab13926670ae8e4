"""Seeded cases for the focr decoder's font search in both forms, and what tests/focr_fonts_model.py says of them
(tests/test_focr_fonts_fuzz_host.py on the CPU, tests/test_gpu_focr_fonts_fuzz.py on the device).

build(i) is a function of the case index and SEED alone (np.random.default_rng([SEED, i])).  A random case draws its decode
font, alphabet and run geometry as tests/focr_fuzz_cases.py's build does (Sans, Serif, Mono in turn, hinting on in every
second triple, its SIZES and KERNINGS, an alphabet of 2 .. 12 characters, x of 0 .. 5, y of 0 .. 4, a width of 12 .. 48, a
page that may clip the width and whose bottom edge cuts the last slot, line_advance = line_height +- 3, one to three pages
that may have two sizes and a blank one in the middle), then K of KS and K candidates (face, size, hinting, kerning) over
the same alphabet: any face, the case's size times one of FACTORS or any of SIZES, the case's hinting flipped in every
second draw, any of KERNINGS.  A candidate that focr_decoder_set_font_candidates or a whole-line run would refuse is drawn
again from the same generator, so no case is left out anywhere.  Every inked slot is set in the font of a drawn index of
0 ..= K with focr_fuzz_cases._ink_line's perturbations (a sub-pixel pen start, advances scaled by 0.97 .. 1.03, the baseline
moved by up to 0.4 px, 2 % of the pixels salted).  Behind the random cases comes FIXED: ties, the last of fifteen, caps and
whole-line batches that a draw rarely hits, each on a clipped, cut and overlapping geometry.  Nothing here comes from the
device path.

want(case, form) is focr_fonts_model.search_image of every page, cached; form is "pen" or "whole".
"""
import collections

import numpy as np

import focr_fonts_model as FM
import focr_whole_model as W
from focr_fuzz_cases import FONTS, KERNINGS, MONO, SANS, SERIF, SIZES, WHOLE_BATCH_MAX, WHOLE_RING_MAX, _alphabet, _ink_line, crops, fast, last_batch

SEED = 0xF0F7
N_RANDOM = 24
KS = (1, 2, 3, 4, 5, 8, 15)  # n_fonts & 3 of 2, 3, 0, 1, 2, 1, 0: every writer wave; one and four candidates per wave
FACTORS = (0.8, 0.9, 1.0, 1.1, 1.25)
FORMS = ("pen", "whole")
DECODE = "the decode font"  # in a FIXED candidate list: the case's own (font, size, hinting, kerning)

# name -> what the draw is replaced by.  cands: the candidates 1 ..= K; ink: the indices the inked slots are set in.
# Every one keeps a clip of four columns (a second page size is up to three wider), line_advance three rows below line_height (slots overlap), a cut last slot and denser ink.
_CLIPPED = dict(clip=4, overlap=3, width=36, slots=4, pages=2)
FIXED = (
    ("tie-with-the-decode-font", dict(_CLIPPED, font=SERIF, size=11.5, kerning=1.07, alphabet="aenT vH",
                                      cands=[(SANS, 11.5, False, 1.0), DECODE, (SERIF, 13.0, True, 0.85)], ink=(0,))),
    ("tie-in-two-waves", dict(_CLIPPED, font=SANS, size=13.0, kerning=1.0, alphabet="omn Hi",
                              cands=[(SERIF, 11.5, False, 1.07), (SERIF, 11.5, False, 1.07), (MONO, 13.0, False, 1.0)], ink=(1,))),
    ("tie-in-one-wave", dict(_CLIPPED, font=MONO, size=11.5, kerning=0.85, alphabet="xo+ ANj",
                             cands=[(SANS, 9.0, True, 1.0), (MONO, 13.0, False, 1.0), (SERIF, 11.5, False, 1.0), (SANS, 13.0, False, 1.3),
                                    (SANS, 9.0, True, 1.0), (MONO, 9.0, False, 1.0)], ink=(1,))),
    ("last-of-fifteen", dict(_CLIPPED, font=SANS, size=9.0, kerning=1.0, alphabet="ab Eg",
                             cands=[(MONO, 9.0, False, 1.0), (SERIF, 9.0, False, 1.0), (SANS, 11.5, False, 1.0), (SANS, 7.15, False, 1.0),
                                    (MONO, 11.5, False, 1.0), (SERIF, 7.15, False, 1.0), (SANS, 9.0, False, 1.3), (SANS, 9.0, False, 0.6),
                                    (MONO, 7.15, True, 1.0), (SERIF, 11.5, True, 1.0), (MONO, 6.0, False, 1.0), (SANS, 6.0, False, 1.0),
                                    (SERIF, 6.0, False, 1.0), (MONO, 9.0, False, 1.3), (SERIF, 13.0, True, 1.07)], ink=(15,))),
    ("cap-is-the-candidate's", dict(_CLIPPED, font=MONO, size=24.0, kerning=1.0, alphabet="ilne A", width=48, line_height=14, pages=1,
                                    cands=[(SANS, 6.0, False, 0.85), (SERIF, 9.0, True, 1.0)], ink=(1, 2))),
    ("whole-batches-and-rings", dict(_CLIPPED, font=MONO, size=7.15, kerning=1.0, alphabet="Ho ea", width=40, line_height=20, pages=3,
                                     cands=[(MONO, 17.3, False, 1.0), (MONO, 11.5, False, 1.0), (MONO, 24.0, True, 1.07)], ink=(0, 1, 2, 3))),
)
N_CASES = N_RANDOM + len(FIXED)

# cands: [(font, size, hinting, kerning)] of the candidates 1 ..= K; ink: [[(slot, k)] per page], the font each inked slot is set in
Case = collections.namedtuple("Case", "index name font size kerning hinting alphabet cands geo pages ink")


def font_plan(fm, w):
    """What decode_whole.hip's whole_font_plan derives for one font on a crop of w columns: min and max inc64, the characters
    per line at most, the batch and the keys its ring must hold; None where it (or the upload) refuses the font."""
    ox, incs = float(fm.ox), np.asarray(fm.incs, dtype=np.float32)
    if not (ox >= 0 and ox == int(ox)) or not (incs > 0).all():
        return None
    inc = W.inc64(incs)
    lo, hi = int(inc.min()), int(inc.max())
    g = fm.font.s.glyphs
    T = max(g[k].stride * g[k].box_h * 2 * 255 * 255 for k in range(len(fm.alphabet)))
    cap = max(-(-64 * w // lo), 1) if lo >= 1 else 0
    batch = min(lo, WHOLE_BATCH_MAX)
    ring = 64
    while ring < batch + hi:
        ring *= 2
    if lo < 1 or 64 * w + hi >= 1 << 24 or cap * T >= 1 << 47 or ring > WHOLE_RING_MAX:
        return None
    return dict(lo=lo, hi=hi, cap=cap, T=T, batch=batch, ring=ring)


def _candidate(rng, size, hinting):
    face = FONTS[int(rng.integers(0, len(FONTS)))]
    if rng.random() < 0.5:
        t = float(np.float32(size * FACTORS[int(rng.integers(0, len(FACTORS)))]))
    else:
        t = float(SIZES[int(rng.integers(0, len(SIZES)))])
    return face, t, bool(hinting ^ (rng.random() < 0.5)), float(KERNINGS[int(rng.integers(0, len(KERNINGS)))])


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
    x, y, width = int(rng.integers(0, 6)), int(rng.integers(0, 5)), int(rng.integers(12, 49))
    line_height = max(1, int(round(size * rng.uniform(0.6, 1.6))))
    line_advance = max(1, line_height + int(rng.integers(-3, 4)))
    clip = int(rng.integers(1, 5)) if rng.random() < 0.4 else 0  # the page ends this many columns inside x + width
    slots = int(rng.integers(2, 5))
    n_pages = int(rng.integers(1, 4))
    two_sizes = n_pages > 1 and rng.random() < 0.5
    blank_middle = n_pages == 3 and rng.random() < 0.5
    width, line_height, clip = fix.get("width", width), fix.get("line_height", line_height), fix.get("clip", clip)
    slots, n_pages = fix.get("slots", slots), fix.get("pages", n_pages)
    blank_middle = blank_middle and not fix
    if "overlap" in fix:
        line_advance = max(1, line_height - fix["overlap"])
    # slots - 1 whole advances and a last slot that the bottom edge cuts (where line_height > 1 leaves something to cut)
    cut = int(rng.integers(1, max(2, min(line_height - 1, line_advance) + 1)))
    Wp, Hp = max(1, x + width - clip), y + (slots - 1) * line_advance + cut
    shapes = [(Hp + int(rng.integers(0, line_advance + 1)), Wp + int(rng.integers(1, 4))) if two_sizes and p == 1 else (Hp, Wp) for p in range(n_pages)]
    w = max(min(width, s[1] - min(x, s[1])) for s in shapes)  # the widest crop: what every font's plan must fit
    specs = [(font, size, hinting, kerning)]
    if fix:
        specs += [specs[0] if c is DECODE else c for c in fix["cands"]]
    else:
        for _ in range(KS[int(rng.integers(0, len(KS)))]):
            c = _candidate(rng, size, hinting)
            while font_plan(fast(c[0], c[1], alphabet, c[2], c[3]), w) is None:  # a refusable draw: the next one of the same generator
                c = _candidate(rng, size, hinting)
            specs.append(c)
    models = [fast(f, t, alphabet, h, k) for f, t, h, k in specs]
    assert all(font_plan(m, w) is not None for m in models), name
    pool = fix.get("ink", range(len(specs)))
    pages, ink = [], []
    for p, shape in enumerate(shapes):
        page = np.full(shape, 255, dtype=np.uint8)
        n = -(-(shape[0] - y) // line_advance)
        inked = rng.random(n) < (0.6 if fix else 0.3)
        inked[int(rng.integers(0, n))] = True
        ink.append([])
        for s in np.flatnonzero(inked) if not (blank_middle and p == 1) else ():
            k = int(pool[int(rng.integers(0, len(pool)))])
            f, t, h, _ = specs[k]
            _ink_line(rng, page, models[k], f, t, h, x, y + int(s) * line_advance)
            ink[-1].append((int(s), k))
        pages.append(page)
    return Case(i, "%d-%s" % (i, name), font, size, kerning, hinting, alphabet, specs[1:], (x, y, width, line_height, line_advance), pages, ink)


_cases = {}


def case(i):
    if i not in _cases:
        _cases[i] = build(i)
    return _cases[i]


def models(c):
    """The FastModels of a case: [0] the decode font's, [1:] the candidates'."""
    return [fast(f, t, c.alphabet, h, k) for f, t, h, k in [(c.font, c.size, c.hinting, c.kerning)] + list(c.cands)]


def crop_width(c):
    """g.w of the case's widest size group."""
    return max(min(c.geo[2], p.shape[1] - min(c.geo[0], p.shape[1])) for p in c.pages)


_want = {}


def want(c, form):
    """The model's answer of a case in a form: [[(y, focr_fonts_model.Fonts)] per page]."""
    key = (c.index, form)
    if key not in _want:
        ms = models(c)
        _want[key] = [FM.search_image(ms, p, *c.geo, whole=form == "whole") for p in c.pages]
    return _want[key]


# ---- a case on a LineDecoder (the device tests') ---------------------------------------------------------------------------

def get_fonts(d):
    n = d._lib.focr_decoder_n_lines(d._h)
    k, cost = np.full(max(n, 1), 99, dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int64)
    return d._lib.focr_decoder_get_fonts(d._h, k.ctypes.data, cost.ctypes.data), [int(v) for v in k[:n]], [int(v) for v in cost[:n]]


def searched(d, c, form):
    """set_font, set_font_candidates and a searched decode() of a case in a form, its result named; every second odd case
    runs several lines through one workgroup, or through two."""
    who = (c.name, form)
    ms = models(c)
    d.set_font(ms[0].font, c.size)
    d.set_font_candidates([m.font for m in ms[1:]])
    grid = 1 + (c.index // 4) % 2 if c.index % 4 == 1 else 0
    assert d._lib.focr_decoder_debug_set_fonts_grid(d._h, grid) == 0, who
    try:
        res = d.decode(c.pages, *c.geo, font_search=True, whole_line=form == "whole")
    finally:
        assert d._lib.focr_decoder_debug_set_fonts_grid(d._h, 0) == 0, who
    names = ("lines", "pens", "costs", "fonts") if form == "whole" else ("lines", "fonts", "costs")
    assert len(res) == len(names), who
    got = dict(zip(names, res))
    launches = d._lib.focr_decoder_last_launches(d._h)
    idx, has_slots = last_batch(c)
    assert launches == (3 if has_slots else 0), who + (launches,)
    rc, ks, costs = get_fonts(d)  # of the size group that ran last
    assert rc == 0 and ks == [k for i in idx for k in got["fonts"][i]] and costs == [v for i in idx for v in got["costs"][i]], who + ("focr_decoder_get_fonts",)
    return got

"""tests/focr_align_model.py, the definition of focr_decoder_align_text (include/focr_decode.h) the GPU tests compare with, pinned
without a device: against an enumeration of every offset path, against focr_score_text_model (one FreeType raster per glyph) at
its own pens, against the rigid shift search at N = 0, monotone in both radii, and on the pages the call is for: a line set at
another kerning, moved by a fraction of a pixel, or snapped to the pixel grid.  fit_pens at its edges.  Every comparison is ==."""
import numpy as np
import pytest

import focr_align_model as A
import focr_score_text_model as S
import focr_slack_model as SL
from focr_fast_model import FastModel
from focr_fuzz_cases import FONTS
from font_ocr_amd import fit_pens, nominal_pens

SANS, SERIF, MONO = FONTS
AL = "abcdefghilmnoprstuv HI01+/"
TEXT = "burn clip ffH vvill rnrn cl"
SIZE, ROWS, START = 13.0, 18, 64

_models = {}


def model(font):
    if font not in _models:
        _models[font] = FastModel(font, SIZE, AL)
    return _models[font]


def drawn_pens(nom, scale=1.0, x=0, floor=False):
    """Where the page's characters are drawn: the font's pens from START stretched by `scale`, moved by x / 64 px, and with
    `floor` snapped down to whole pixels."""
    pens = [START + int(np.rint(scale * (m - START))) + x for m in nom]
    return [64 * (p // 64) for p in pens] if floor else pens


_pages = {}


def page(font, text, scale=1.0, x=0, floor=False):
    """(the cropped line, the pens it was drawn at, the nominal pens, the alphabet indices): 18 rows, cropped 12 columns past the
    last pen; built once."""
    key = (font, text, scale, x, floor)
    if key not in _pages:
        fm = model(font)
        idx = [AL.index(c) for c in text]
        nom = A.nominal(fm.incs, idx, START)
        drawn = drawn_pens(nom, scale, x, floor)
        ref = SL.draw_at(font, SIZE, AL, text, drawn, drawn[-1] // 64 + 12, ROWS)
        ref.setflags(write=False)
        _pages[key] = (ref, drawn, nom, idx)
    return _pages[key]


def same(a, b):
    return (a.base, a.cost, a.first, a.last) == (b.base, b.cost, b.first, b.last) and np.array_equal(a.pens, b.pens) and np.array_equal(a.terms, b.terms)


@pytest.mark.parametrize("font", FONTS)
@pytest.mark.parametrize("drift,step", [(2, 0), (2, 1), (3, 2), (1, 1)])
def test_the_programme_is_the_best_of_every_offset_path(font, drift, step):
    """n <= 3: every path through the band enumerated, with the definition's tie rules.  On a page moved by 2/64 px, and from
    start = 1 where the band's negative half is dead for the first character."""
    fm = model(font)
    ref = page(font, "fH i", x=2)[0]
    for text, start in (("fH ", START), ("H", START), (" i", START), ("fH", 1), ("", 5)):
        idx = [AL.index(c) for c in text]
        term = A.fast_term(fm, ref, idx)
        nom = A.nominal(fm.incs, idx, start)
        assert same(A.align(term, nom, drift, step, A.base_of(ref)), A.brute(term, nom, drift, step, A.base_of(ref))), (text, start)


CASES = [(font, scale, x, floor, cfg) for font in FONTS for scale, x, floor in ((1.01, 0, False), (0.99, 37, False), (1.0, 0, True), (1.0, 0, False))
         for cfg in ((0, 0), (5, 1), (128, 4), (128, 8), (128, 32))]


@pytest.mark.parametrize("font,scale,x,floor,cfg", CASES)
def test_cost_and_terms_are_score_texts_at_the_fitted_pens(font, scale, x, floor, cfg):
    """The fitted pens fed to focr_score_text_model, which draws every glyph with FreeType: the same base, cost and terms."""
    ref, _, _, idx = page(font, TEXT, scale, x, floor)
    a = A.align_crop(model(font), ref, idx, START, *cfg)
    s = S.score_crop(model(font).font, ref, idx, pens=a.pens)
    assert (a.base, a.cost) == (s.base, s.cost) and np.array_equal(a.terms, s.terms)
    assert a.first == int(a.pens[0]) - START and a.last == int(a.pens[-1]) - A.nominal(model(font).incs, idx, START)[-1]


@pytest.mark.parametrize("font", FONTS)
@pytest.mark.parametrize("drift", [0, 1, 17, 64])
def test_no_step_is_the_rigid_shift_search(font, drift):
    """N = 0 with start >= W and W <= 64: score_text's shift search over the nominal pens, in cost and in shift."""
    ref, _, nom, idx = page(font, TEXT, 1.0, 37, False)
    a = A.align_crop(model(font), ref, idx, START, drift, 0)
    s = S.score_crop(model(font).font, ref, idx, pens=nom, radius=drift)
    assert (a.cost, a.first, a.last) == (s.cost, s.shift, s.shift) and np.array_equal(a.terms, s.terms)
    if drift >= 37:
        # the page's own pens; where footprints overlap (Sans's and Serif's "ff", "rn") each glyph counts the overlap: below -base
        assert a.first == 37 and (a.cost == -a.base if font == MONO else a.cost < -a.base)


@pytest.mark.parametrize("font", FONTS)
def test_cost_does_not_rise_with_either_radius(font):
    ref, _, _, idx = page(font, TEXT, 1.01, 0, False)
    fm = model(font)
    term = A.fast_term(fm, ref, idx)
    nom = A.nominal(fm.incs, idx, START)
    cost = {(w, n): A.align(term, nom, w, n).cost for w in (0, 3, 40, 128) for n in (0, 1, 4, 64)}
    for (w, n), c in cost.items():
        assert all(c >= c2 for (w2, n2), c2 in cost.items() if w2 >= w and n2 >= n), (w, n)


# (font, scale, x, floored, (W, N)) -> base, the rigid search's (cost, shift) at radius 64, cost, first, last, the largest deviation of
# an inked character from its drawn pen, fit_pens: the model's own numbers
STORY = [
    (SANS, 1.01, 0, False, (128, 4), 16924910, (-12153318, 46), -16922345, 1, 97, 2, (1.0100000482399762, 63.69839919179305)),
    (SANS, 1.01, 0, False, (128, 8), 16924910, (-12153318, 46), -16927170, 0, 98, 1, (1.0100003255443362, 64.10612673399869)),
    (SANS, 0.99, 37, False, (128, 4), 16926831, (-11852144, -9), -16928331, 36, -60, 2, (0.9899999517600238, 101.30160080820696)),
    (SANS, 0.99, 37, False, (128, 8), 16926831, (-11852144, -9), -16933035, 37, -61, 0, (0.98999408718465, 100.96679762939576)),
    (SANS, 1.0, 0, True, (128, 32), 16479494, (-14217157, -36), -16451359, 0, -47, 7, (0.998141937237221, 38.27152920956657)),
    (MONO, 1.01, 0, False, (128, 8), 17963017, (-10784592, 58), -17961825, 0, 128, 2, (1.0099419982327669, 64.15339116719207)),
    (MONO, 0.99, 37, False, (128, 8), 18505538, (-10658739, -23), -18505538, 37, -93, 0, (0.9900199600798403, 101.0)),
    (MONO, 1.0, 0, True, (128, 32), 18082887, (-15798221, -33), -17818557, -10, -34, 14, (1.0006296555154675, 29.047318611987233)),
    (SERIF, 1.0, 0, True, (128, 32), 16757342, (-14774314, -24), -16665946, 0, -28, 14, (1.0001570951278624, 34.46379447455018)),
    # Mono's advance of 501/64 px times 1 % passes a step of 4: the alignment cannot follow, and says so in its cost
    (MONO, 1.01, 0, False, (128, 4), 17963017, (-10784592, 58), -17542935, 12, 116, 14, (1.0079840319361277, 76.0)),
    # Serif on its own pens: once a step is allowed the cost goes slightly below -base (overlapping footprints count once per glyph)
    (SERIF, 1.0, 0, False, (128, 4), 17779685, (-17801998, 0), -17802705, 0, 0, 1, (1.0000099087127334, 63.90352233990879)),
]


@pytest.mark.parametrize("font,scale,x,floor,cfg,base,rigid,cost,first,last,dev,fit", STORY)
def test_the_pages_it_is_for(font, scale, x, floor, cfg, base, rigid, cost, first, last, dev, fit):
    """A known line on a page whose kerning is 1 % off, which is moved by 37/64 px, or whose pens are snapped to whole pixels:
    the rigid shift search loses a quarter of the line; the alignment costs what the page's own pens cost to within its step, puts
    every inked character within `dev` / 64 px of where it was drawn, and its least-squares fit reads the kerning and x off."""
    ref, drawn, nom, idx = page(font, TEXT, scale, x, floor)
    fm = model(font)
    r = S.score_crop(fm.font, ref, idx, pens=nom, radius=64)
    a = A.align_crop(fm, ref, idx, START, *cfg)
    assert (a.base, (r.cost, r.shift), a.cost, a.first, a.last) == (base, rigid, cost, first, last)
    assert max(abs(int(p) - d) for p, d, t in zip(a.pens, drawn, a.terms) if t) == dev
    assert list(nominal_pens(fm.font, TEXT, START)) == nom
    assert fit_pens(nom, a.pens, a.terms, START) == fit
    if not floor and cfg[1] >= 8:  # the step follows the stretch: the kerning to 1e-4 and x to half a 1/64 px
        assert abs(fit[0] - scale) < 1e-4 and abs(fit[1] - START - x) < 0.5


def test_fit_pens_edges():
    assert fit_pens([], [], []) == (None, None)
    assert fit_pens([64, 500, 900], [70, 505, 912], [0, 0, 0]) == (None, None)      # no inked character
    assert fit_pens([64, 500, 900], [70, 505, 912], [0, -5, 0]) == (None, None)     # one
    assert fit_pens([64, 64, 64], [70, 71, 72], [-1, -1, 3], 64) == (None, None)    # equal nominals: no slope
    assert fit_pens([64, 164], [70, 171], [-1, 2], 64) == (1.01, 70.0)              # two: the line through them
    assert fit_pens([64, 100, 164], [70, 9999, 171], [-1, 0, 2]) == (1.01, 70.0)    # a space is left out; start defaults to nominal[0]
    assert fit_pens([64, 192], [70, 134], [-1, 2], 0) == (0.5, 38.0)                # x64 is the pen at nominal == start
    assert fit_pens(np.array([0, 10, 20], dtype=np.uint32), np.array([3, 13, 23], dtype=np.uint32), np.array([-7, 1, -2], dtype=np.int32), 0) == (1.0, 3.0)

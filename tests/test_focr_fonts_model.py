"""tests/focr_fonts_model.py on the two experiments the font search was proposed on (include/focr_decode.h, "font candidates"):
what the cost separates and what it does not.  The numbers are the model's own on the committed fonts.  No GPU needed."""
import os

import numpy as np
import pytest

import focr_baseline_model as B
import focr_fonts_model as FM
from focr_fast_model import FastModel

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MONO, SANS, SERIF = (os.path.join(GOLD, f) for f in ("DejaVuSansMono.ttf", "DejaVuSans.ttf", "DejaVuSerif.ttf"))
ALPHABET = "abcdefghilmnoprstuv HI01+/"
# (font, size, hinting, kerning)
PEN = [(MONO, 13.0, False, 1.0), (MONO, 12.0, False, 1.0), (MONO, 14.0, False, 1.0), (MONO, 13.0, True, 1.0), (MONO, 13.0, False, 1.05),
       (SANS, 13.0, False, 1.0), (SERIF, 13.0, False, 1.0), (MONO, 12.5, False, 1.0)]
WHOLE = [(SANS, 13.0, False, 1.0), (SANS, 12.0, False, 1.0), (SANS, 13.0, True, 1.0), (SERIF, 13.0, False, 1.0), (MONO, 13.0, False, 1.0),
         (SERIF, 12.0, False, 1.0)]
PEN_TEXT, WHOLE_TEXT = "burn clip HI01 vill+/no", "burn clip HI01 vill"


def _models(cands):
    return [FastModel(f, t, ALPHABET, h, k) for f, t, h, k in cands]


def _line(cand, text, page_w, rows, cols):
    """`text` in the candidate's font on a 20-row page, cropped to rows x cols."""
    f, t, h, k = cand
    page = np.full((20, page_w), 255, dtype=np.uint8)
    B.draw_offset(page, f, t, ALPHABET, text, 0, 0, 0.0, h, k)
    return page[:rows, :cols]


@pytest.fixture(scope="module")
def pen_models():
    ms = _models(PEN)
    yield ms
    for m in ms:
        m.close()


@pytest.fixture(scope="module")
def whole_models():
    ms = _models(WHOLE)
    yield ms
    for m in ms:
        m.close()


@pytest.mark.parametrize("j,cost,runner_up", [(0, -18071583, -16737995), (1, -14387884, -6254552), (2, -20339293, -6202003), (3, -17932493, -16598905),
                                              (4, -18096953, -6578967), (7, -16391906, -6320519)])
def test_pen_loop_mono_lines_are_won_by_their_own_font(pen_models, j, cost, runner_up):
    """A line drawn in any Mono candidate is won by that candidate, with cost == -line_base exactly (the true text's
    rendering cancels the page), and is read whole; size, kerning and hinting each separate by a wide margin, hinting least."""
    ref = _line(PEN[j], PEN_TEXT, 200, 18, 190)
    r = FM.search_line(pen_models, ref)
    assert (r.k, r.cost) == (j, cost) and r.cost == -r.base and r.text.startswith(PEN_TEXT)
    assert r.trail[-1] == (j, cost) and [k for k, _ in r.trail] == sorted(k for k, _ in r.trail)
    costs = sorted(FM.pen_loop(m, ref)[1] for m in pen_models)
    assert costs[:2] == [cost, runner_up]
    if j == 0:  # the hinted candidate comes second, every other font far behind
        assert FM.pen_loop(pen_models[3], ref)[1] == -16737995 and costs[2] == -7095592


def test_pen_loop_loses_a_proportional_line(pen_models):
    """The Sans 13 line under the pen loop: the greedy loop loses it under every candidate, its own font included, and the
    cheapest wrong reading picks candidate 4.  The pen-loop form is a monospace tool; the Serif line is won but misread."""
    sans = FM.search_line(pen_models, _line(PEN[5], PEN_TEXT, 200, 18, 190))
    assert (sans.k, sans.cost, sans.base) == (4, -7673832, 16211193) and sans.text.startswith("bucfrho rc1 nh+/+i")
    assert FM.pen_loop(pen_models[5], _line(PEN[5], PEN_TEXT, 200, 18, 190))[1] == -6609579
    serif = FM.search_line(pen_models, _line(PEN[6], PEN_TEXT, 200, 18, 190))
    assert (serif.k, serif.cost) == (6, -11682231) and serif.cost > -serif.base and not serif.text.startswith(PEN_TEXT)


@pytest.mark.parametrize("j,cost,trail", [(0, -13068658, [0]), (1, -10658169, [0, 1]), (2, -13021325, [0, 2]), (3, -13171571, [0, 3]),
                                          (4, -12042304, [0, 1, 4]), (5, -10963377, [0, 1, 5])])
def test_whole_line_lines_are_won_by_their_own_font(whole_models, j, cost, trail):
    """All six lines, proportional ones included, are won by their own font under the whole-line form and read whole (the
    Mono line as far as the 120 columns reach)."""
    r = FM.whole_search_line(whole_models, _line(WHOLE[j], WHOLE_TEXT, 130, 18, 120))
    assert (r.k, r.cost) == (j, cost) and [k for k, _ in r.trail] == trail and len(r.pens) == len(r.text)
    assert r.text.rstrip(" ") == (WHOLE_TEXT if j != 4 else "burn clip HI01 v")
    if j == 0:
        assert r.trail == [(0, -13068658)] and r.base == 13094656


def test_search_image_walks_a_page(pen_models):
    """Two lines of different fonts and a blank slot between them: line order, y and winners."""
    page = np.full((60, 200), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 12.0, ALPHABET, PEN_TEXT, 0, 0, 0.0)
    B.draw_offset(page, MONO, 13.0, ALPHABET, PEN_TEXT, 0, 40, 0.0, True)
    got = FM.search_image(pen_models[:4], page, 0, 0, 190, 18, 20)
    assert [(y, r.k) for y, r in got] == [(0, 1), (40, 3)] and all(r.text.startswith(PEN_TEXT) for _, r in got)
    assert FM.search_image(pen_models[:1], page, 0, 0, 190, 18, 20)[0][1].k == 0

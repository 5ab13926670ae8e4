"""The refine model (tests/focr_refine_model.py: focr_decoder_refine_text's definition in numpy over the phase tables) against a brute
force with one FreeType raster per candidate, against focr_score_text_model where footprints are disjoint, on the invariants of the
definition, and on the pages it is for: the misread lines of tests/test_focr_slack_model.py, whose figures the strings and numbers
below record.  No GPU needed."""
import os

import numpy as np
import pytest

import focr_refine_model as R
import focr_score_text_model as ST
import focr_slack_model as K
import focr_whole_model as W
from focr_fast_model import FastModel
from font_ocr_amd import FOCR_DEFAULT_ALPHABET
from test_focr_slack_model import PAGES, model, snapped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
SERIF = os.path.join(GOLD, "DejaVuSerif.ttf")


def check(fm, ref, got, radius, sweeps, glyphs=True):
    """The invariants of the definition on a result."""
    assert got.base + got.cost >= 0 and got.cost <= got.cost_in and got.sweeps <= sweeps
    assert got.cost == R.composed_cost(fm.font, ref, got.idx, got.pens)
    assert (got.cost < got.cost_in) == (got.changed > 0)  # every change lowers the cost strictly
    if 0 < got.sweeps < sweeps and np.all(np.diff(got.pens.astype(np.int64)) >= 0):  # it stopped before its cap: a fixed point
        again = R.refine_crop(fm, ref, got.idx, got.pens, radius, sweeps, glyphs)
        assert again.changed == 0 and again.sweeps == 1 and again.cost_in == again.cost == got.cost


# (font, alphabet, the text drawn, its pens in 1/64 px, the reading that goes in, its pens): tight pens, so that boxes overlap
BRUTE = [
    (SANS, "rnmi", "rni", [0, 330, 700], "nmr", [10, 340, 690]),
    (SERIF, "fil", "fil", [0, 250, 440], "lif", [0, 250, 445]),
    (MONO, "ab.c", "ab.", [64, 300, 560], "caa", [60, 300, 562]),
    (SERIF, "vwilIA", "vilA", [0, 300, 500, 640], "wlIv", [2, 301, 499, 640]),
]


@pytest.mark.parametrize("font,al,text,pens,read,read_pens", BRUTE, ids=["sans", "serif", "mono", "serif6"])
@pytest.mark.parametrize("glyphs", [True, False], ids=["glyphs", "pens"])
def test_model_is_the_brute_force(font, al, text, pens, read, read_pens, glyphs):
    """Every D from one FreeType raster of the candidate on the crop, every canvas composed anew from rasters: the same result,
    field for field, on lines whose glyphs lie on one another."""
    fm = model(font, 13.0, al)
    line = K.draw_at(font, 13.0, al, text, pens, 22)
    idx = [al.index(c) for c in read]
    got, want = R.refine_crop(fm, line, idx, read_pens, 2, 2, glyphs), R.brute(fm, line, idx, read_pens, 2, 2, glyphs)
    assert got[:6] == want[:6] and np.array_equal(got.pens, want.pens)
    assert got.cost_in > -got.base  # the reading that went in is not the page
    boxes = [R.clipped(fm.font, i, s, *line.shape) for i, s in zip(idx, read_pens)]
    ink = sum((np.pad(b[4], ((b[0], line.shape[0] - b[1]), (b[2], line.shape[1] - b[3]))) > 0).astype(int) for b in boxes if b)
    assert ink.max() >= 2  # two glyphs put ink on one pixel: the case the separable sum gets wrong
    check(fm, line, got, 2, 2, glyphs)


@pytest.mark.parametrize("font", [SANS, SERIF, MONO], ids=["sans", "serif", "mono"])
def test_own_page_costs_minus_base(font):
    """A line drawn with the max of ink at its own pens: cost_in == -line_base, nothing changes, one sweep is made."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(font, 13.0, al)
    text = "ffH vvill"
    pens = K.font_pens(fm, text)
    line = K.draw_at(font, 13.0, al, text, pens, 70)
    got = R.refine_crop(fm, line, [al.index(c) for c in text], pens, 4, 4)
    assert got.cost_in == got.cost == -got.base and got.changed == 0 and got.sweeps == 1 and R.text_of(fm, got.idx) == text
    check(fm, line, got, 4, 4)


def test_disjoint_footprints_cost_what_score_text_costs():
    """Mono 13 px at the font's own pens: no pixel carries two glyphs' ink, and cost_in is focr_score_text_model's cost, on the
    line's own page and on another one."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(MONO, 13.0, al)
    text = "burn clip"
    idx = [al.index(c) for c in text]
    pens = K.font_pens(fm, text)
    own, other = K.draw_at(MONO, 13.0, al, text, pens, 80), K.draw_at(MONO, 13.0, al, "born cIIp", pens, 80)
    v = np.zeros(own.shape, dtype=int)
    for box in (R.clipped(fm.font, i, s, *own.shape) for i, s in zip(idx, pens)):
        if box is not None:  # the space has no bitmap
            ya, yb, xa, xb, c = box
            v[ya:yb, xa:xb] += c > 0
    assert v.max() == 1
    for page in (own, other):
        assert R.refine_crop(fm, page, idx, pens, 0, 0).cost_in == ST.score_crop(fm.font, page, idx, pens=pens).cost


def test_edges():
    """No characters, an empty crop, sweeps 0, pens at 0 (j < 0 is dropped) and a glyph wholly right of the crop."""
    al = "rnmi"
    fm = model(SANS, 13.0, al)
    line = K.draw_at(SANS, 13.0, al, "rn", [0, 330], 20)
    assert R.refine_crop(fm, line, [], [], 4, 4)[:5] == (R.refine_crop(fm, line, [0], [0], 0, 0).base, 0, 0, 1, 0)
    got = R.refine_crop(fm, line[:, :0], [0, 1], [0, 330], 4, 4)
    assert got[:5] == (0, 0, 0, 1, 0)
    got = R.refine_crop(fm, line, [1, 0], [0, 330], 4, 0)
    assert got.sweeps == 0 and got.changed == 0 and got.cost == got.cost_in
    got = R.refine_crop(fm, line, [1, 0], [0, 330], 4, 4)
    assert R.text_of(fm, got.idx) == "rn" and got.pens.tolist() == [0, 330] and got.cost == -got.base
    got = R.refine_crop(fm, line, [0, 1, 2], [0, 330, 64 * 40], 4, 4)
    assert got.idx == [0, 1, 2] and got.changed == 0 and got.cost == -got.base  # the m lies right of the crop: every D is 0


# the reading and pens of focr_slack_model.slack_line at slack N on the pages of tests/test_focr_slack_model.py, refined with radius 4
# and at most 4 sweeps: (font, page, N, reading in, reading out, composed cost in, out, line_base)
ROWS = [
    (SANS, "floor", 8, "born clip ffH vvill rnrn c", "burn clip ffH vvill rnrn c", -14445951, -15758225, 15779062),
    (SANS, "round", 8, "burn cIIp ffH vviIl rnrn c", "burn clip ffH vvill rnrn c", -14768503, -15647614, 15668767),
    (SERIF, "floor", 8, "barn clfp ffH vvill rnrn ", "burn clip ffH vvill rnrn ", -14607313, -15508657, 15575415),
    (SERIF, "floor", 32, "burn clip ffH vvill rnrnA", "burn clip ffH vvill rnrnA", -15444998, -15575415, 15575415),
    (SERIF, "round", 32, "burn clip ffH vvilI rnrn ", "burn clip ffH vvilI rnrn ", -15429086, -15512053, 15542806),
]


@pytest.mark.parametrize("font,page,n,read,want,cost_in,cost,base", ROWS, ids=[f"{os.path.basename(r[0])[6:-4]}-{r[1]}-{r[2]}" for r in ROWS])
def test_pinned_pages(font, page, n, read, want, cost_in, cost, base):
    """Three of the four misread lines are read whole; Serif floored at N = 32 is reproduced with squared error 0 (its `A` hangs over
    the right edge); Serif rounded at N = 32 keeps `vvilI`: the limit of a repair that moves one character at a time."""
    fm = model(font, 13.0, FOCR_DEFAULT_ALPHABET)
    line = snapped(font, *PAGES[page])
    s = K.slack_line(fm, line, n)
    assert s.text == read
    got = R.refine_crop(fm, line, s.idx, s.pens, 4, 4)
    assert (R.text_of(fm, got.idx), got.cost_in, got.cost, got.base) == (want, cost_in, cost, base)
    if (font, page) == (SANS, "floor"):
        assert got.cost_in == s.cost  # no two glyphs of this reading share a pixel of ink: the programme's own cost
    else:
        assert got.cost_in > s.cost  # the overlap, counted once here and once per glyph there (Sans rounded: by 621, under `cIIp`)
    check(fm, line, got, 4, 4)

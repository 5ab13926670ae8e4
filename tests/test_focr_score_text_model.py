"""tests/focr_score_text_model.py (focr_decoder_score_text restated with one FreeType raster per glyph) against every other
model of the decoder on that model's own output, a small case each: the cost a mode returns is the cost score_text gives the
mode's reading.  Then the case the entry point was proposed on: a known string ranks fonts, proportional ones included, where
the pen-loop font search cannot, and a rigid shift search recovers the page's x to 1/64 px.  The numbers are the model's own
on the committed fonts.  No GPU needed."""
import os

import numpy as np
import pytest

import focr_baseline_model as B
import focr_fonts_model as FM
import focr_line_frac_model as LF
import focr_margins_model as MM
import focr_score_text_model as S
import focr_scores_model as SC
import focr_search_model as SE
import focr_slack_model as SL
import focr_whole_baseline_model as WB
import focr_whole_model as WM
from focr_fast_model import FastModel
from font_ocr_amd.decoder import DecodeFont

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MONO, SANS, SERIF = (os.path.join(GOLD, f) for f in ("DejaVuSansMono.ttf", "DejaVuSans.ttf", "DejaVuSerif.ttf"))
ALPHABET = "abcdefghilmnoprstuv HI01+/"
TEXT = "burn clip HI01 vill"
# the six candidates of the ranking: (font, size)
CANDS = [(SANS, 13.0), (SANS, 12.0), (SERIF, 13.0), (MONO, 13.0), (SERIF, 12.0), (SANS, 13.5)]


def _idx(text):
    return [ALPHABET.index(c) for c in text]


@pytest.fixture(scope="module")
def mono():
    fm = FastModel(MONO, 13.0, ALPHABET)
    yield fm
    fm.close()


@pytest.fixture(scope="module")
def sans():
    fm = FastModel(SANS, 13.0, ALPHABET)
    yield fm
    fm.close()


@pytest.fixture(scope="module")
def mono_y2():
    return B.BaselineModel(MONO, 13.0, ALPHABET, y_bits=2)


@pytest.fixture(scope="module")
def sans_y2():
    return B.BaselineModel(SANS, 13.0, ALPHABET, y_bits=2)


def _mono_line(offset=0.0, cols=60):
    page = np.full((20, 70), 255, dtype=np.uint8)
    B.draw_offset(page, MONO, 13.0, ALPHABET, "HI01 no+", 0, 0, offset)
    return page[:18, :cols]


def _sans_line(offset=0.0, cols=40):
    page = np.full((20, 60), 255, dtype=np.uint8)
    B.draw_offset(page, SANS, 13.0, ALPHABET, "Hill 01", 0, 0, offset)
    return page[:18, :cols]


def test_scores_model(mono):
    ref = _mono_line()
    s = SC.line_scores(mono, ref)
    got = S.score_crop(mono.font, ref, _idx(s.text))
    assert s.text.startswith("HI01 no+") and got.base == s.base and np.array_equal(got.terms, s.score - s.base) and got.shift == 0
    assert got.cost == int((s.score - s.base).sum())


def test_search_model(mono):
    ref = np.asarray(S.draw_text(mono.font, "HI01 no+", 70, 18, shift64=3)[:, :60])
    s = SE.search_line(mono, ref, 4)
    assert s.offsets[0] == 3 and s.text.startswith("HI01 no+")  # the search finds the page's shift at its first step
    got = S.score_crop(mono.font, ref, _idx(s.text), offsets=s.offsets)
    assert got.base == s.base and np.array_equal(got.terms, s.score - s.base)
    # the same reading without its offsets costs more, and a rigid shift search finds the 3/64 px again
    plain = S.score_crop(mono.font, ref, _idx(s.text))
    moved = S.score_crop(mono.font, ref, _idx(s.text), radius=4)
    assert plain.cost > got.cost and moved.shift == 3 and moved.cost == got.cost


def test_whole_and_margins_models(sans):
    ref = _sans_line()
    w = WM.whole_line(sans, ref)
    got = S.score_crop(sans.font, ref, w.idx, pens=w.pens)
    assert w.text.startswith("Hill 01") and (got.base, got.cost) == (w.base, w.cost)
    m = MM.margins_line(sans, ref)
    assert np.array_equal(m.idx, w.idx) and np.array_equal(got.terms, m.term) and got.cost == m.cost


def test_slack_model(sans):
    ref = np.asarray(SL.draw_at(SANS, 13.0, ALPHABET, "Hill", [2, 531, 744, 968], 40, 18))  # pens off the font's own advances
    s = SL.slack_line(sans, ref, 3)
    assert s.offsets.any()
    got = S.score_crop(sans.font, ref, s.idx, pens=s.pens)  # the render pens
    assert (got.base, got.cost) == (s.base, s.cost)


def test_baseline_model(mono_y2):
    ref = _mono_line(0.5)
    b = mono_y2.search_line(ref, 3)
    assert b.q == 2 and b.text.startswith("HI01 no+")
    got = S.score_crop(mono_y2.font, ref, _idx(b.text), q=b.q, y_bits=2)
    assert got.cost == b.cost
    for q in (-5, -4, 1, 4, 7):  # d < 0 and d > 0, whole and fractional
        text, cost = mono_y2.decode_line_q(ref, q)
        assert S.score_crop(mono_y2.font, ref, _idx(text), q=q, y_bits=2).cost == cost, q


def test_whole_baseline_model(sans_y2):
    ref = _sans_line(-0.25)
    w = WB.search_line(sans_y2, ref, 2)
    assert w.q == -1
    got = S.score_crop(sans_y2.font, ref, w.idx, pens=w.pens, q=w.q, y_bits=2)
    assert got.cost == w.cost


def test_line_frac_model(mono_y2, sans_y2):
    c = LF.centre(40, 2)  # a line 40/64 px below its crop's top: the candidates lie around q = 3
    assert c == 3
    ref = _mono_line(0.625)
    b = LF.search_line(mono_y2, ref, c, 1)
    assert b.q in (2, 3, 4) and S.score_crop(mono_y2.font, ref, _idx(b.text), q=b.q, y_bits=2).cost == b.cost  # the absolute q
    ref = _sans_line(0.625)
    w = LF.whole_search_line(sans_y2, ref, c, 1)
    assert S.score_crop(sans_y2.font, ref, w.idx, pens=w.pens, q=w.q, y_bits=2).cost == w.cost


def test_fonts_model():
    models = [FastModel(f, t, ALPHABET) for f, t in ((MONO, 13.0), (MONO, 12.0), (SANS, 13.0))]
    try:
        page = np.full((20, 70), 255, dtype=np.uint8)
        B.draw_offset(page, MONO, 12.0, ALPHABET, "HI01 no+", 0, 0, 0.0)
        r = FM.search_line(models, page[:18, :60])
        assert r.k == 1
        got = S.score_crop(models[r.k].font, page[:18, :60], r.idx)
        assert (got.base, got.cost) == (r.base, r.cost)
        ref = _sans_line()
        r = FM.whole_search_line(models, ref)
        assert r.k == 2
        got = S.score_crop(models[r.k].font, ref, r.idx, pens=r.pens)
        assert (got.base, got.cost) == (r.base, r.cost)
    finally:
        for m in models:
            m.close()


# ---- the ranking a known string gives ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cands():
    fonts = [DecodeFont(f, t, ALPHABET) for f, t in CANDS]
    yield fonts
    for f in fonts:
        f.close()


RANKING = {  # source font -> the cost of TEXT under each of the six candidates, on the first 120 columns of its 130-column line
    0: [-13094656, 1156055, 3537383, 1588347, -3121531, 5102336],
    2: [3455352, 3345579, -13176687, 4237249, 1117573, 6105256],
    3: [2633124, 1096525, 5364057, -12049879, 1979131, 4188676],
}


@pytest.mark.parametrize("src", sorted(RANKING))
def test_a_known_string_ranks_the_fonts(cands, src):
    """TEXT drawn in Sans 13, Serif 13 and Mono 13 and scored under six candidates: the page's own font costs -line_base
    exactly (its rendering cancels the page), and no other candidate comes near it, proportional fonts included."""
    ref = S.draw_text(cands[src], TEXT, 130, 18)[:, :120]
    got = [S.score_crop(f, ref, _idx(TEXT)) for f in cands]
    assert [g.cost for g in got] == RANKING[src]
    assert got[src].cost == -got[src].base and int(np.argmin([g.cost for g in got])) == src
    assert sorted(g.cost for g in got)[1] - got[src].cost > 9_000_000  # the runner-up is far behind
    assert len({g.base for g in got}) == 1


@pytest.mark.parametrize("src,at_zero,base64,cost21,base21", [(0, 164886, 13094656, -13086136, 13086136), (2, -742979, 12609287, -13721814, 13715924),
                                                              (3, -717879, 11895277, -11740513, 11740513)])
def test_a_rigid_shift_search_recovers_x(cands, src, at_zero, base64, cost21, base21):
    """The page moved one pixel to the right loses its own font at shift 0 and finds it again at j = 64; a page moved 21/64 px
    is found at j = 21.  (Serif's glyphs overlap at that phase: its cost counts the overlap once per glyph and passes -base.)"""
    idx = _idx(TEXT)
    ref = S.draw_text(cands[src], TEXT, 130, 18, shift64=64)[:, :120]
    assert S.score_crop(cands[src], ref, idx).cost == at_zero
    got = S.score_crop(cands[src], ref, idx, radius=64)
    assert (got.shift, got.cost, got.base) == (64, -base64, base64)
    ref = S.draw_text(cands[src], TEXT, 130, 18, shift64=21)[:, :120]
    got = S.score_crop(cands[src], ref, idx, radius=24)
    assert (got.shift, got.cost, got.base) == (21, cost21, base21)


def test_placements_and_edges(cands):
    """deltas: the three placements, the shift joining the first offset, a negative delta; an empty crop and an empty line."""
    f = cands[3]  # Mono 13
    idx = _idx("HI0")
    inc, ox = f.increments(), f.origin[0]
    assert float(ox) == int(ox)
    plain = S.deltas(f, idx)
    assert plain[0] == 64 * int(ox) and plain[1] == int(np.float32(np.float32(ox + inc[idx[0]]) * np.float32(64)))
    assert S.deltas(f, idx, j=-64 * int(ox) - 64)[0] == -64  # what FreeType would receive
    assert S.deltas(f, idx, offsets=[2, -1, 0], j=5)[0] == plain[0] + 7
    assert S.deltas(f, idx, pens=[0, 500, 1001], j=-3) == [64 * int(ox) - 3, 64 * int(ox) + 497, 64 * int(ox) + 998]
    blank = np.full((18, 40), 255, dtype=np.uint8)
    got = S.score_crop(f, blank, idx)
    assert (got.base, got.cost) == (0, int(got.terms.sum())) and got.cost > 0  # the sum of c^2 on a white crop
    spaces = S.score_crop(f, blank, _idx("   "), radius=2)  # every shift costs 0: the rank decides
    assert (spaces.cost, spaces.shift) == (0, 0) and not spaces.terms.any()
    none = S.score_crop(f, blank[:0], idx, radius=1)  # an empty crop
    assert (none.base, none.cost, none.shift) == (0, 0, 0) and not none.terms.any()
    empty = S.score_crop(f, blank, [])
    assert (empty.base, empty.cost, empty.shift, len(empty.terms)) == (0, 0, 0, 0)

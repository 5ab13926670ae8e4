"""The whole-line model with pen slack (tests/focr_slack_model.py) against the plain whole-line model, against FreeType
and against the pages it is for.  The model is the definition of include/focr_decode.h on FastModel.scores: at N = 0 it
must be tests/focr_whole_model.py field for field, every term it uses must equal one FreeType raster of the candidate at
its render pen, the invariants of the definition must hold on every result, and on pages whose glyphs were snapped to
the pixel grid or set with another advance it must read what the strings below record.  No GPU needed."""
import os

import numpy as np
import pytest

import focr_search_model as S
import focr_slack_model as K
import focr_whole_model as W
from focr_fast_model import FastModel
from font_ocr_amd import FOCR_DEFAULT_ALPHABET
from font_ocr_amd.decoder import raster_glyph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
SERIF = os.path.join(GOLD, "DejaVuSerif.ttf")
F32 = np.float32
TEXT = "burn clip ffH vvill rnrn cl"
CROP = 150  # columns: the line is cut after "rnrn c"
PAGES = {"floor": ("floor", 1.0), "round": ("round", 1.0), "x1.01": ("exact", 1.01), "x0.99": ("exact", 0.99)}
# what the model reads at 13 px, unhinted, kerning 1, the default alphabet, at N = 0, 8 and 32
READS = {
    (SANS, "floor"): ("bum cIIp ffH vvill rnrn o", "born clip ffH vvill rnrn c", "burn clip ffH vvill rnrn c"),
    (SANS, "round"): ("burn clip ffH vvill rnrn c", "burn cIIp ffH vviIl rnrn c", "burn clip ffH vvill rnrn c"),
    (SANS, "x1.01"): ("burri clip ffH vvIII rnrn e", "burn clip ffH vvill rnrn c", "burn clip ffH vvill rnrn c"),
    (SANS, "x0.99"): ("born clio ffHivvill rnrn d", "burn clip ffH vvill rnrn c", "burn clip ffH vvill rnrn c"),
    (SERIF, "floor"): ("barn cl/p ffH vvill rnrm", "barn clfp ffH vvill rnrn ", "burn clip ffH vvill rnrnA"),
    (SERIF, "round"): ("burn clip ffH vvill rnrn ", "burn clip ffH vvifl rnrn ", "burn clip ffH vvilI rnrn "),
    (SERIF, "x1.01"): ("burn cfip ffH vvfll rnrn", "burn clip ffH vvill rnrn", "burn clip ffH vvill rnrn"),
    (SERIF, "x0.99"): ("buro clip flH vvill rnrnA", "burn clip ffH vvill rnrnA", "burn clip ffH vvill rnrnA"),
}
WHOLE = "burn clip ffH vvill rnrn"  # the drawn text the crop holds whole; what follows hangs over the right edge

_models = {}


def model(font, size, alphabet):
    key = (font, size, alphabet)
    if key not in _models:
        _models[key] = FastModel(font, size, alphabet)
    return _models[key]


def snapped(font, snap, advance, text=TEXT, alphabet=FOCR_DEFAULT_ALPHABET, width=CROP):
    page = np.full((W.alphabet_height(font, 13.0, alphabet), width), 255, dtype=np.uint8)
    return S.draw_snapped(page, font, 13.0, alphabet, text, 0, 0, snap, advance)


@pytest.mark.parametrize("font,text", [(SANS, TEXT), (SERIF, TEXT), (SANS, "i" * 40), (MONO, TEXT)], ids=["sans", "serif", "sans-i40", "mono"])
def test_no_slack_is_the_whole_line_model(font, text):
    """N = 0 on the lines of test_focr_whole_model.py: text, indices, pens, cost and base are whole_line's, every offset
    is 0, and the states that render are the reachable ones."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(font, 13.0, al)
    page = W.draw_line(font, 13.0, al, text)
    want, got = W.whole_line(fm, page), K.slack_line(fm, page, 0)
    assert got.text == want.text and got.cost == want.cost and got.base == want.base
    assert np.array_equal(got.idx, want.idx) and got.idx.dtype == want.idx.dtype
    assert np.array_equal(got.pens, want.pens) and got.pens.dtype == want.pens.dtype
    assert got.offsets.dtype == np.int8 and not got.offsets.any()
    K.check_invariants(fm, got)
    assert K.char_bound(fm.incs, page.shape[1], 0) == W.char_bound(fm.incs, page.shape[1])


def test_every_term_is_one_freetype_raster():
    """Sans 13 px, four glyphs, "rni" with every pen floored, N = 8: each term(i, p) the programme asks for equals the
    full-canvas SSD of one raster_glyph canvas at origin + p / 64, the render pen, less the canvas's sum of r^2; every
    pen that renders is asked for all four glyphs; the cost is the sum of the terms along the text."""
    font, size, al = SANS, 13.0, "rnmi"
    page = snapped(font, "floor", 1.0, "rni", al, 21)
    h, w = page.shape
    fm = model(font, size, al)
    ox, oy = fm.font.origin
    seen = {}

    def pinned(fm_, r, total, p):
        got = W.term_from_scores(fm_, r, total, p)
        for i, ch in enumerate(al):
            canvas = np.zeros((h, w), dtype=np.uint8)
            raster_glyph(font, size, ch, F32(ox + F32(p) / F32(64)), oy, canvas)
            assert got[i] == int(((r - canvas.astype(np.int64)) ** 2).sum()) - total, (p, ch)
            seen[(p, i)] = int(got[i])
        return got

    got = K.slack_line(fm, page, 8, term=pinned)
    assert len({p for p, _ in seen}) == got.states and got.states * 4 == len(seen)
    assert got.text[:3] == "rni" and got.offsets.any()
    assert got.cost == sum(seen[(int(p), int(i))] for p, i in zip(got.pens, got.idx))
    K.check_invariants(fm, got)
    assert got.pens[-1] < 64 * w <= got.pens[-1] + W.inc64(fm.incs)[got.idx[-1]]


@pytest.mark.parametrize("font", [SANS, SERIF], ids=["sans", "serif"])
@pytest.mark.parametrize("page", list(PAGES))
def test_pages_off_the_grid(font, page):
    """The strings the model returns for the issue's pages at N = 0, 8 and 32.  Required: Sans reads the drawn text whole
    at N = 32 on every page, and both fonts read the two advance pages whole at N = 8.  N = 0 is whole_line's string."""
    fm = model(font, 13.0, FOCR_DEFAULT_ALPHABET)
    line = snapped(font, *PAGES[page])
    got = [K.slack_line(fm, line, n) for n in (0, 8, 32)]
    for s, n in zip(got, (0, 8, 32)):
        K.check_invariants(fm, s)
        assert np.abs(s.offsets.astype(int)).max() <= n and len(s.text) <= K.char_bound(fm.incs, CROP, n)
    assert tuple(s.text for s in got) == READS[(font, page)]
    assert got[0].text == W.whole_line(fm, line).text
    if font == SANS:
        assert got[2].text.startswith(WHOLE)
    if page in ("x1.01", "x0.99"):
        assert got[1].text.startswith(WHOLE) and got[2].text.startswith(WHOLE)
    assert got[0].cost >= got[1].cost >= got[2].cost  # a wider window only adds paths
    assert got[0].states <= got[1].states <= got[2].states <= 64 * CROP


@pytest.mark.parametrize("font,read", [(SANS, "burn clip ffH vvill rnrn c"), (SERIF, "burn clip ffH vvill rnrn ")], ids=["sans", "serif"])
def test_exact_pens_read_the_same_with_slack(font, read):
    """The line drawn at the font's own f32 pens: the slack changes nothing of the text."""
    fm = model(font, 13.0, FOCR_DEFAULT_ALPHABET)
    line = snapped(font, "exact", 1.0)
    assert [K.slack_line(fm, line, n).text for n in (0, 8, 32)] == [read] * 3 and read.startswith(WHOLE)


@pytest.mark.parametrize("n", [8, 32])
def test_blank_gap_takes_no_offset(n):
    """"burn", a blank gap of 40 px and "clip", every character drawn at its state (the running sum of inc64): the line
    needs no offset anywhere, a space scores the same at every pen, so inside the gap ties decide; they go to rank, and
    every space of the gap sits at offset 0, as every letter does."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(SANS, 13.0, al)
    sp = int(W.inc64(fm.incs)[al.index(" ")])
    n_sp = -(-40 * 64 // sp)
    text = "burn" + " " * n_sp + "clip"
    line = K.draw_at(SANS, 13.0, al, text, K.font_pens(fm, text), 110)
    assert n_sp * sp >= 40 * 64 and np.all(line[:, 30: 30 + 40] == 255)
    s = K.slack_line(fm, line, n)
    K.check_invariants(fm, s)
    assert s.text[: len(text)] == text and not s.offsets[: len(text)].any()
    assert np.array_equal(s.pens[: len(text)], K.font_pens(fm, text))


def test_duplicate_glyph_decodes_to_the_lower_index():
    """"rnir": the fourth glyph is the first again, so both tie at every pen and the programme remembers index 0."""
    al = "rnir"
    fm = model(SANS, 13.0, al)
    line = snapped(SANS, "floor", 1.0, "rnirr", al, 30)
    s = K.slack_line(fm, line, 8)
    K.check_invariants(fm, s)
    assert s.text[:5] == "rnirr" and 3 not in s.idx.tolist() and s.idx.tolist()[:5] == [0, 1, 2, 0, 0]


def by_definition(fm, ref, n):
    """include/focr_decode.h's slack programme read literally, state by state: cost[t] and glyph[t] are the lowest
    (G[t - inc64[i]].cost + term(i, t - inc64[i]), i) over the glyphs i, G[p] the lowest (cost[p - j], rank(j)).  Every state
    G[p] looks at lies below p + N < t, so ascending t sees only final costs.  Returns (text, pens, offsets, cost)."""
    r = 255 - ref.astype(np.int64)
    total = int((r * r).sum())
    inc = [int(v) for v in W.inc64(fm.incs)]
    n_live = 64 * ref.shape[1]
    cost, glyph, G, terms = {0: 0}, {}, {}, {}

    def window(p):
        if p not in G:
            reach = [(cost[p - j], S.rank(j), j) for j in range(-n, n + 1) if 0 <= p - j < n_live and p - j in cost]
            G[p] = min(reach) if reach else None
            if reach:
                terms[p] = W.term_from_scores(fm, r, total, p)
        return G[p]

    for t in range(1, n_live + max(inc)):
        cand = [(window(t - v)[0] + int(terms[t - v][i]), i) for i, v in enumerate(inc) if 0 <= t - v < n_live and window(t - v)]
        if cand:
            cost[t], glyph[t] = min(cand)
    end = min((cost[t], t) for t in cost if t >= n_live)[1]
    text, pens, offs, t = [], [], [], end
    while t > 0:
        i = glyph[t]
        p = t - inc[i]
        text.append(fm.alphabet[i]), pens.append(p), offs.append(G[p][2])
        t = p - G[p][2]
    return "".join(text[::-1]), pens[::-1], offs[::-1], cost[end]


@pytest.mark.parametrize("n", [0, 1, 8])
def test_ties_between_glyphs_of_different_advances_go_to_the_lower_index(n):
    """Sans 11.5 px hinted, "v=,-b", crops one row high (the line-height-1 case of tests/focr_fuzz_cases.py, where the
    device and this model first differed): "," and "-" miss the row, so both cost nothing at every pen, and a state that
    ",-" and "-," both reach is a tie between glyphs pushed from different render pens.  The definition remembers the
    lower index; a push loop with a strict compare would keep the glyph of the lower pen, the wider one.  The model must
    be the definition read literally, on an inked row and on a blank one."""
    al = ",-v=b"
    fm = FastModel(SANS, 11.5, al, True, 1.0)
    inc = W.inc64(fm.incs)
    assert inc[0] < inc[1]  # the lower index is the narrower glyph: pushed from the higher pen, so visited later
    row = np.full((1, 32), 255, dtype=np.uint8)
    raster = np.zeros((14, 32), dtype=np.uint8)
    raster_glyph(SANS, 11.5, "b", F32(fm.font.origin[0] + F32(20.3)), fm.font.origin[1], raster, True)
    inked = 255 - raster[3:4]
    assert (inked != 255).any()
    for ref in (row, inked):
        s = K.slack_line(fm, ref, n)
        K.check_invariants(fm, s)
        assert (s.text, s.pens.tolist(), s.offsets.tolist(), s.cost) == by_definition(fm, ref, n)
        if n == 0:
            w = W.whole_line(fm, ref)
            assert (s.text, s.pens.tolist(), s.cost) == (w.text, w.pens.tolist(), w.cost)
    fm.close()


def test_helpers():
    incs = np.array([3.611328, 7.8], dtype=F32)  # inc64 231 and 499
    assert K.max_slack(incs) == 64 and K.max_slack(np.array([1.0], dtype=F32)) == 32 and K.max_slack(np.array([0.02], dtype=F32)) == 0
    assert K.char_bound(incs, 145, 0) == 41 and K.char_bound(incs, 145, 8) == -(-64 * 145 // 223) == 42
    assert K.batch(incs, 8) == 223 and K.batch(np.array([19.27], dtype=F32), 8) == 512

"""The margins model (tests/focr_margins_model.py) against the whole-line model it extends and against the pages it is
for.  The model is the definition of include/focr_decode.h with a forward and a backward table; here its text, pens and
cost must be focr_whole_model.whole_line's, B[0] must be the line's cost, every margin must be what the unmodified
whole-line model pays when the chosen glyph is forbidden over the character's midpoint (the cut identity), the smallest
margins must fall where a reader would look (l / i / I), and in a monospace font the runner and margin must be the plain
decoder's.  No GPU needed."""
import os

import numpy as np
import pytest

import focr_margins_model as MM
import focr_scores_model as SM
import focr_whole_model as W
from focr_fast_model import FastModel
from font_ocr_amd import FOCR_DEFAULT_ALPHABET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
TEXT = "burn clip ffH vvill rnrn cl"


@pytest.fixture(scope="module")
def small():
    fm = FastModel(SANS, 13.0, "burn clif")
    yield fm
    fm.close()


@pytest.fixture(scope="module")
def sans():
    fm = FastModel(SANS, 13.0, FOCR_DEFAULT_ALPHABET)
    yield fm
    fm.close()


def check_whole(fm, line, got):
    """The margins model's line is the whole-line model's; B[0] is its cost; the terms sum to it; margins are >= 0."""
    want = W.whole_line(fm, line)
    assert got.text == want.text and np.array_equal(got.idx, want.idx) and np.array_equal(got.pens, want.pens)
    assert got.cost == want.cost == got.b0 == int(got.term.astype(np.int64).sum()) and got.base == want.base
    assert got.term.dtype == np.int32 and got.runner.dtype == np.uint16 and got.margin.dtype == np.int64
    assert np.all(got.margin >= 0) and not np.any(got.runner == got.idx)
    return want


@pytest.mark.parametrize("text", ["burn clif", "ffill bull"])
def test_cut_identity(small, text):
    """Two short Sans 13 px lines over "burn clif", 70 px wide: for every character, the whole-line model re-run with the
    chosen glyph prohibitively dear at every state that covers the character's midpoint costs exactly cost + margin, and
    reads another glyph over that midpoint, the runner or a glyph after it that ties with it."""
    line = W.draw_line(SANS, 13.0, small.alphabet, text, width=70)
    got = MM.margins_line(small, line)
    check_whole(small, line, got)
    assert got.text[: len(text)] == text
    inc = W.inc64(small.incs)
    for k, (i_k, s_k) in enumerate(zip(got.idx, got.pens)):
        m_k = int(s_k) + (int(inc[i_k]) >> 1)
        cut = W.whole_line(small, line, term=MM.forbid(small, int(i_k), m_k))
        assert cut.cost == got.cost + int(got.margin[k]) < MM.DEAR // 2, (k, got.text[k])
        over, = [int(i) for i, s in zip(cut.idx, cut.pens) if int(s) <= m_k < int(s) + int(inc[i])]
        assert over != i_k
        assert got.runner[k] <= over  # the cut's covering edge has the lowest through-cost; the runner is the lowest such glyph


def test_confusable_letters(sans):
    """Sans 13 px, the default alphabet, "Il1 O0o": the smallest margin is the I's, whose runner is l; O's runner is Q."""
    line = W.draw_line(SANS, 13.0, sans.alphabet, "Il1 O0o")
    got = MM.margins_line(sans, line)
    check_whole(sans, line, got)
    assert got.text[:7] == "Il1 O0o"
    run = MM.runner_text(sans, got.runner)
    print("Il1 O0o:", list(zip(got.text, run, got.margin.tolist())))
    k = int(np.argmin(got.margin[:7]))
    assert {got.text[k], run[k]} == {"I", "l"} and int(got.margin[k]) == 45763
    assert run[4] == "Q" and int(got.margin[4]) == 104161


def test_readme_line(sans):
    """Sans 13 px, the README's line: the l / i / I characters carry the smallest margins, 8 659 to 63 720, and every other
    inked character has a margin above 100 000."""
    line = W.draw_line(SANS, 13.0, sans.alphabet, TEXT)
    got = MM.margins_line(sans, line)
    check_whole(sans, line, got)
    assert got.text[:-1] == TEXT
    run = MM.runner_text(sans, got.runner)
    print(TEXT, list(zip(got.text, run, got.margin.tolist())))
    thin = [int(m) for c, m in zip(TEXT, got.margin) if c in "liI"]
    rest = [int(m) for c, m in zip(TEXT, got.margin) if c not in "liI "]
    assert len(thin) == 6 and min(thin) == 8659 and max(thin) == 63720 and min(rest) > 100000


def same_rendering(fm, got):
    """The characters of a whole-line result that the plain decoder renders at the same 26.6 delta: its f32 pen, the sum
    of the f32 increments, truncates to the character's state s."""
    pos, out = np.float32(0), []
    for i, s in zip(got.idx, got.pens):
        out.append(int(np.float32(np.float32(fm.ox + pos) * np.float32(64))) == 64 * int(fm.ox) + int(s))
        pos = np.float32(pos + fm.incs[i])
    return np.array(out)


@pytest.mark.parametrize("size,text", [(13.0, TEXT), (13.0, "Il1 O0o"), (32.0, "Il1 O0o")])
def test_monospace_margins_are_the_plain_decoders(size, text):
    """Mono: every glyph has one advance, so every covering edge of a character starts at its own pen, the suffix cost B
    is shared, and runner and margin are the plain decoder's runner and runner_score - score -- where the two render the
    character at the same delta.  The definition puts the pens on multiples of inc64 = rint(64 * increment); the plain
    decoder's pen is the f32 sum of the increments.  At 13 px the increment is 7.82666 px = 500.906 / 64 and inc64 is 501,
    so from the second character on the plain decoder renders at another sub-pixel phase (500 / 64 against 501 / 64) and
    its scores are those of another rendering: the equality holds for the first character only, and is asserted there.
    At 32 px the increment is 1233 / 64 px exactly, the pens agree all along the line, and so does every character."""
    al = FOCR_DEFAULT_ALPHABET
    fm = FastModel(MONO, size, al)
    line = W.draw_line(MONO, size, al, text)
    got, plain = MM.margins_line(fm, line), SM.line_scores(fm, line)
    check_whole(fm, line, got)
    same = same_rendering(fm, got)
    fm.close()
    assert got.text == plain.text and same[0] and (same.all() if size == 32.0 else not same[1:].any())
    assert np.array_equal(got.runner[same], plain.runner[same])
    assert np.array_equal(got.margin[same], (plain.runner_score - plain.score)[same])
    assert np.array_equal(got.term.astype(np.int64)[same], (plain.score - plain.base)[same])


def test_one_glyph_alphabet_has_no_runner():
    fm = FastModel(MONO, 13.0, "A")
    got = MM.margins_line(fm, W.draw_line(MONO, 13.0, "A", "AAA"))
    fm.close()
    assert got.text[:3] == "AAA" and np.all(got.runner == MM.NO_RUNNER) and np.all(got.margin == -1)
    assert MM.runner_text(fm, got.runner) == "\0" * len(got.text)

"""tests/focr_verify_text_model.py, the CPU model of focr_decoder_verify_text, against the models it restates, and the pinned
numbers of one mixed-font page (README.md quotes them).  No GPU."""
import os

import numpy as np

import focr_line_model as L
import focr_search_model as S
import focr_verify_text_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO, SANS = os.path.join(GOLD, "DejaVuSansMono.ttf"), os.path.join(GOLD, "DejaVuSans.ttf")
AL = "abehinor HIm"
FONTS = [M.Font(MONO, 13.0), M.Font(MONO, 12.0), M.Font(SANS, 13.0)]
MIXED = [M.Line(2, "Hinein inea", 0), M.Line(20, "moheb in H", 1), M.Line(38, "neben im Io", 2)]


def mixed_page():
    return M.draw_lines(np.full((58, 120), 255, dtype=np.uint8), MIXED, FONTS, 3)


def test_single_font_grid_equals_line_model():
    """Lines of one font on a regular grid, the last clipped at the page's bottom, one blank slot and noise on the page: the
    image is focr_line_model.verify_image's, byte for byte, and the sum gives its MSE."""
    rng = np.random.default_rng(3)
    page, texts = L.synth_page(rng, MONO, 13.0, AL, 150, 70, 4, 3, 15, 5, blank_every=3, noise=20)
    lines = [(3 + 15 * i, t) for i, t in enumerate(texts) if t is not None]
    assert len(lines) == 4 and lines[-1][0] + 15 > 70
    want, want_mse = L.verify_image(page, lines, MONO, 13.0, 4)
    got, sq = M.verify_text(page, [M.Line(y, t, 0) for y, t in lines], FONTS, AL, 4)
    assert np.array_equal(got, want) and M.mse(sq, 150, 70) == want_mse and sq > 0


def test_pens_and_offsets_equal_search_model():
    """Zero offsets and the f32 running sum are the same pens; a whole-line run's pens go through s / 64: both equal
    focr_search_model.verify_image, the model of the existing verify."""
    page = mixed_page()
    line = MIXED[2]
    df, vf = M.tables(FONTS[2], AL)
    idx = [AL.index(c) for c in line.text]
    plain = M.verify_text(page, [line], FONTS, AL, 3)
    zero = M.verify_text(page, [line._replace(offsets=[0] * len(idx))], FONTS, AL, 3)
    assert np.array_equal(plain[0], zero[0]) and plain[1] == zero[1]
    offs = [0, 3, -2, 0, 1, 0, 0, -4, 0, 2, 0]
    pens64 = np.concatenate([[0], np.cumsum(np.rint(df.increments() * 64).astype(np.int64)[idx][:-1])])
    for kw, at in ((dict(offsets=offs), M.offset_pens(df, idx, offs)), (dict(pens=pens64), [np.float32(int(s)) / np.float32(64) for s in pens64])):
        got = M.verify_text(page, [line._replace(**kw)], FONTS, AL, 3)
        want = S.verify_image(page, [(line.y, line.text, at)], df, vf, 3)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        assert got[1] != plain[1]


def test_list_order_decides():
    """Two overlapping lines: the later one's ink replaces the earlier one's blue, whichever has the smaller y."""
    page = np.full((40, 120), 255, dtype=np.uint8)
    a, b = M.Line(6, "Hinein", 0), M.Line(2, "mohebm", 2)
    ab, ba = M.verify_text(page, [a, b], FONTS, AL, 3)[0], M.verify_text(page, [b, a], FONTS, AL, 3)[0]
    assert not np.array_equal(ab, ba)
    only_a, only_b = M.verify_text(page, [a], FONTS, AL, 3)[0], M.verify_text(page, [b], FONTS, AL, 3)[0]
    ink_a, ink_b = only_a[..., 2] != 0, only_b[..., 2] != 0
    assert (ink_a & ink_b).any()  # they do overlap
    assert np.array_equal(ab[..., 2][ink_b], only_b[..., 2][ink_b]) and np.array_equal(ba[..., 2][ink_a], only_a[..., 2][ink_a])


def test_mixed_page_pinned():
    """Mono 13 px, Mono 12 px and Sans 13 px lines on one page: drawn each in its own font the verify reproduces the page
    (sum 0); drawn all in the decode font, as the existing verify would, the MSE is 2900.7754."""
    page = mixed_page()
    own = M.verify_text(page, MIXED, FONTS, AL, 3)
    one = M.verify_text(page, [l._replace(font=0) for l in MIXED], FONTS, AL, 3)
    assert own[1] == 0 and M.mse(own[1], 120, 58) == np.float32(0)
    assert one[1] == 20189395 and M.mse(one[1], 120, 58) == np.float32(2900.7754)
    ref, ref_mse = L.verify_image(page, [(l.y, l.text) for l in MIXED], MONO, 13.0, 3)
    assert np.array_equal(ref, one[0]) and ref_mse == M.mse(one[1], 120, 58)

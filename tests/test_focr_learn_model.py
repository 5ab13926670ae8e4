"""What learning glyph tables from a trusted reading does, and what it does not, pinned on the CPU with tests/focr_learn_model.py
(the definition in numpy; nothing here touches a device).

The setup is the one the feature was proposed with: DejaVu Sans Mono, the 65-glyph base64 alphabet with a space, 58-character lines of
random glyphs, pages drawn by FreeType in another rendering than the decode font's (hinted, or unhinted through a gamma of 0.6), the
decode font unhinted, pen-loop placements, bitmaps learned inside the bounding rectangle of the phase's own ink (grow 0), twelve test
lines nobody trained on.  The proposal trained on 600 lines; that takes the model some 40 s, so the suite trains on 200 (median 3
samples per seen cell, where 600 give 10) and pins what 200 give.  How the 8 px hinted case's errors fall with the training size,
measured with this file's generator: 60 lines 45 -> 58 (half the cells are seen, and a learned cell outbids an unlearned one),
200 lines 42 -> 5, 600 lines 46 -> 0.  The costs of the learned tables end close to -line_base, and below it where neighbouring
boxes overlap (the objective counts an overlap once per glyph).
"""
import numpy as np
import pytest

import focr_learn_model as L
import focr_score_text_model as S
from font_ocr_amd import DecodeFont

from test_focr_learn_host import MONO

ALPHA = " ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
N_CHARS, N_TRAIN, N_TEST = 58, 200, 12


def through_gamma(page, g):
    """The page with every pixel's coverage c in 0 .. 1 replaced by c ** g."""
    c = (255 - page.astype(np.float64)) / 255
    return (255 - np.rint(255 * c ** g)).astype(np.uint8)


class Case:
    """Training and test lines of one (size, rendering): (alphabet indices, luma line) each, and the tables learned from the
    training lines' true text."""

    def __init__(self, size, hinting, gamma, seed, line_height, n_train=N_TRAIN):
        self.base = DecodeFont(MONO, size, ALPHA)
        drawn = DecodeFont(MONO, size, ALPHA, hinting=hinting)
        rng = np.random.default_rng(seed)
        width = int(np.ceil(N_CHARS * float(self.base.increments()[0]))) + 2

        def lines(n):
            out = []
            for _ in range(n):
                idx = [int(v) for v in rng.integers(0, len(ALPHA), N_CHARS)]
                page = S.draw_text(drawn, "".join(ALPHA[i] for i in idx), width, line_height)
                out.append((idx, through_gamma(page, gamma) if gamma else page))
            return out

        self.train, self.test = lines(n_train), lines(N_TEST)
        drawn.close()
        self.acc = self.learn([idx for idx, _ in self.train])
        self.cells, self.inked = L.learned_phases(self.base, self.acc)

    def learn(self, reading):
        """The sums of the training pages under `reading`, one list of alphabet indices per training line."""
        acc = L.empty(self.base)
        acc.used.extend(L.learn_crop(self.base, acc, page, idx) for (_, page), idx in zip(self.train, reading))
        return acc

    def decode(self, tables, data):
        """The pen loop's reading of every line of data under `tables`, cut to the line's length."""
        return [L.decode_line(tables, page, len(ALPHA), self.base.increments(), self.base.origin[0])[:N_CHARS] for _, page in data]

    def wrong(self, tables, data=None):
        data = self.test if data is None else data
        return sum(a != b for (idx, _), got in zip(data, self.decode(tables, data)) for a, b in zip(got, idx))

    def cost(self, tables, data=None):
        data = self.test if data is None else data
        return sum(int(L.table_terms(tables, page, idx, S.deltas(self.base, idx)).sum()) for idx, page in data)

    def line_base(self):
        return sum(int(((255 - page.astype(np.int64)) ** 2).sum()) for _, page in self.test)


@pytest.fixture(scope="module")
def hinted8():
    return Case(8.0, True, 0, 1, 12)


# (size, hinting, gamma, seed, line height): cells learned of cells with ink, wrong before and after, test cost before and after, line_base
TABLE = {"8 px hinted": ((8.0, True, 0, 1, 12), (3158, 4096, 42, 5, -254091452, -294836811, 295968815)),
         "13 px hinted": ((13.0, True, 0, 2, 16), (3137, 4096, 0, 0, -651944519, -720118819, 721352147)),
         "13 px unhinted through gamma 0.6": ((13.0, False, 0.6, 3, 16), (3137, 4096, 0, 0, -896948318, -928294416, 929248052))}


@pytest.mark.parametrize("name", list(TABLE))
def test_the_three_cases(name, hinted8):
    """The proposal's table at 200 training lines: the characters the pen loop gets wrong on the twelve test lines, and their cost
    at the true text, under the base tables and under the learned ones.  Every trained character is used: each box lies in its crop."""
    args, want = TABLE[name]
    c = hinted8 if name == "8 px hinted" else Case(*args)
    assert all(u.all() for u in c.acc.used) and int(c.acc.counts.sum()) == N_TRAIN * N_CHARS
    assert int(np.median(c.acc.counts[c.acc.counts > 0])) == 3
    base, learned = L.Tables(c.base), L.Tables(c.base, c.cells)
    got = (len(c.cells), c.inked, c.wrong(base), c.wrong(learned), c.cost(base), c.cost(learned), c.line_base())
    assert got == want, got
    assert got[5] < got[4] and abs(got[5] + got[6]) < abs(got[4] + got[6]) // 20  # the learned tables explain all but a twentieth of what the base left


def test_self_training_does_not_help(hinted8):
    """Tables learned from the decoder's own reading of the training pages reproduce that reading's errors: no fewer wrong
    characters on the test lines after than before.  It is a tool for a reading one trusts."""
    c = hinted8
    base = L.Tables(c.base)
    reading = c.decode(base, c.train)
    n_wrong = sum(a != b for (idx, _), got in zip(c.train, reading) for a, b in zip(got, idx))
    cells, _ = L.learned_phases(c.base, c.learn(reading))
    got = (n_wrong, c.wrong(base), c.wrong(L.Tables(c.base, cells)))
    assert got == (782, 42, 48), got
    assert got[2] >= got[1]


@pytest.mark.parametrize("hinting,gamma", [(True, 0), (False, 0.6)])
@pytest.mark.parametrize("grow", [0, 1, 3])
def test_least_squares(hinting, gamma, grow):
    """For min_count 1 and any grow the summed terms of the characters that were used are no higher under the learned tables than
    under the base: per pixel of a support the rounded mean is the integer minimiser of the samples' summed squared error, and
    outside the supports nothing changes.  On hinted and on gamma pages, cell by cell as well."""
    c = Case(8.0, hinting, gamma, 5, 12, n_train=20)
    cells, _ = L.learned_phases(c.base, c.acc, 1, grow)
    base, learned = L.Tables(c.base), L.Tables(c.base, cells)
    per_cell = {}
    for (idx, page), used in zip(c.train, c.acc.used):
        ds = S.deltas(c.base, idx)
        tb, tl = L.table_terms(base, page, idx, ds), L.table_terms(learned, page, idx, ds)
        for i, d, a, b, u in zip(idx, ds, tb, tl, used):
            if u:
                s = per_cell.setdefault((i, d & 63), [0, 0])
                s[0] += int(a)
                s[1] += int(b)
    assert len(per_cell) > 500 and all(b <= a for a, b in per_cell.values())
    assert sum(b for _, b in per_cell.values()) < sum(a for a, _ in per_cell.values())
    assert set(cells) == {k for k in per_cell if ALPHA[k[0]] != " "}


def test_identity():
    """Pages drawn in the decode font itself, at a kerning where no neighbour's ink enters a support (checked on the boxes: the
    columns of consecutive characters' ink do not meet), give back the base font: every learned cell is byte-equal to the base's."""
    font = DecodeFont(MONO, 13.0, ALPHA, kerning=1.5)
    rng = np.random.default_rng(7)
    acc = L.empty(font)
    for _ in range(12):
        idx = [int(v) for v in rng.integers(0, len(ALPHA), 30)]
        page = S.draw_text(font, "".join(ALPHA[i] for i in idx), 380, 16)
        spans = []
        for i, (p, x0, _, _, _) in zip(idx, L.boxes(font, idx, S.deltas(font, idx))):
            s = L.support(font.phase(i, p)[0], 0)
            if s is not None:
                spans.append((x0 + s[2], x0 + s[3]))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert L.learn_crop(font, acc, page, idx).all()
    cells, inked = L.learned_phases(font, acc)
    assert 250 < len(cells) < inked == 64 * 64
    for (i, p), bm in cells.items():
        assert np.array_equal(bm, font.phase(i, p)[0]), (i, p)
    font.close()

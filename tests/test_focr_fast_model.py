"""The fast model of the focr decoder (tests/focr_fast_model.py) against the brute-force model (tests/focr_line_model.py),
line for line, on every configuration tests/test_gpu_focr_shapes.py decodes: both fonts; sizes 7.5 to the largest the
builder accepts; kerning 0.6 to 1.07, hinted and not; the default, ASCII95 and 319-glyph alphabets; noise, thin crops,
glyphs left of column 0 and crops past the page.  Also the builder's size bound and the tie groups the GPU tie test
relies on.  No GPU needed."""
import os
import zlib

import numpy as np
import pytest

import focr_line_model as M
from focr_fast_model import ALPHABET_319, ASCII95, LARGEST_SIZE, TIE_GROUPS, FastModel, narrowest_glyph_line, permuted_319
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
ALPHABETS = {"default": FOCR_DEFAULT_ALPHABET, "ascii95": ASCII95, "319": ALPHABET_319}


def _ink(alphabet):
    return "".join(c for c in alphabet if not c.isspace())


def _agree(font, size, alphabet, kerning, hinting, pages, geos):
    fm = FastModel(font, size, alphabet, hinting, kerning)
    try:
        n = 0
        for page in pages:
            for geo in geos:
                want = M.decode_image(page, font, size, alphabet, *geo, kerning, hinting)
                assert fm.decode_image(page, *geo) == want, (geo, want)
                n += len(want)
        assert n > 0
    finally:
        fm.close()


def _small_pages(font, size, alphabet, kerning, hinting, n_lines=2, W=110):
    """A clean page and a noisy one (near-ties), narrow, with the text running past the right edge."""
    adv, lh = int(size * 1.2) + 2, int(size) + 2
    rng = np.random.default_rng(zlib.crc32(repr((os.path.basename(font), size, kerning, hinting, len(alphabet))).encode()))
    H = (n_lines - 1) * adv + lh + 4
    a, _ = M.synth_page(rng, font, size, _ink(alphabet), W, H, 3, 2, adv, n_lines, kerning, hinting)
    b, _ = M.synth_page(rng, font, size, _ink(alphabet), W, H, 3, 2, adv, n_lines, kerning, hinting, noise=20)
    return [a, b], adv, lh


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("kerning", [0.6, 0.85, 1.0, 1.07])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
def test_kerning_and_hinting_at_13px(font, kerning, hinting):
    pages, adv, lh = _small_pages(font, 13.0, FOCR_DEFAULT_ALPHABET, kerning, hinting)
    _agree(font, 13.0, FOCR_DEFAULT_ALPHABET, kerning, hinting, pages, [(1, 2, 200, lh, adv)])


@pytest.mark.parametrize("font,size,alphabet,kerning,hinting", [
    ("mono", 7.5, "ascii95", 1.0, False), ("sans", 7.5, "default", 0.85, True),
    ("mono", 24.0, "ascii95", 1.07, False),  # the 2480-px page of the GPU tests
    ("sans", 24.0, "default", 1.0, False),   # the LDS / global boundary of the GPU tests
    ("mono", 24.0, "default", 1.0, True), ("sans", 24.0, "ascii95", 0.6, True),
    ("mono", 60.0, "default", 1.0, False), ("sans", 60.0, "ascii95", 1.07, True),
])
def test_sizes(font, size, alphabet, kerning, hinting):
    font, al = {"mono": MONO, "sans": SANS}[font], ALPHABETS[alphabet]
    pages, adv, lh = _small_pages(font, size, al, kerning, hinting, n_lines=1 if size > 30 else 2, W=int(size * 6))
    _agree(font, size, al, kerning, hinting, pages, [(1, 2, 10 * int(size), lh, adv)])


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
def test_largest_accepted_size(font):
    """Short lines, a fully inked block (every score at its most negative) and a thin crop through the glyph boxes."""
    size = LARGEST_SIZE[(os.path.basename(font), "default")]
    rng = np.random.default_rng(2)
    page, _ = M.synth_page(rng, font, size, _ink(FOCR_DEFAULT_ALPHABET), 520, 240, 2, 2, 230, 1)
    page[10:200, 330:470] = 0
    page = np.minimum(page, 255 - rng.integers(0, 40, page.shape)).astype(np.uint8)
    _agree(font, size, FOCR_DEFAULT_ALPHABET, 1.0, False, [page], [(1, 2, 600, int(size) + 30, 400), (0, 60, 600, 9, 400)])


def _tie_page(font, alphabet_text, W, seed):
    """Lines that are mostly A, o and spaces, so that every tie group decides something."""
    rng = np.random.default_rng(seed)
    page = np.full((34, W), 255, dtype=np.uint8)
    for ly in (2, 18):
        text = "".join(rng.choice(list("AAoo  " + alphabet_text), 30))
        c = M.render_text(font, 13.0, text)
        hh, ww = min(c.shape[0], 34 - ly), min(c.shape[1], W - 1)
        page[ly: ly + hh, 1: 1 + ww] = np.minimum(page[ly: ly + hh, 1: 1 + ww], 255 - c[:hh, :ww])
    return page


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("order", ["plain", "permuted"])
def test_319_glyph_alphabet(font, order):
    al = ALPHABET_319 if order == "plain" else permuted_319()
    page = _tie_page(font, "xyzéŁž", 110, 5 + (font == SANS))
    _agree(font, 13.0, al, 1.0, False, [page], [(0, 0, 200, 15, 16)])


def test_cap_line_of_the_narrowest_glyph():
    """The GPU cap test's line: Sans 13 px over the 319-glyph alphabet, U+0027 drawn at its own pen positions."""
    page, ch, cap = narrowest_glyph_line(SANS, 13.0, ALPHABET_319, 300)
    assert ch == "'" and cap == 84
    _agree(SANS, 13.0, ALPHABET_319, 1.0, False, [page], [(0, 0, 300, 16, 16)])


def test_edge_geometry():
    """Thin crops, crops that start left of the text or past the page, and Sans J, T, Y, j reaching left of the pen."""
    font, size = SANS, 13.0
    W, H = 120, 64
    rng = np.random.default_rng(9)
    page = np.full((H, W), 255, dtype=np.uint8)
    for i, first in enumerate("JTYj"):
        c = M.render_text(font, size, first + "".join(rng.choice(list(_ink(FOCR_DEFAULT_ALPHABET)), 14)))
        ly = 1 + 15 * i
        hh, ww = min(c.shape[0], H - ly), min(c.shape[1], W)
        page[ly: ly + hh, :ww] = np.minimum(page[ly: ly + hh, :ww], 255 - c[:hh, :ww])
    assert all(M.glyph_metrics(font, size, ch)[2][0] < 0 for ch in "JTYj")
    geos = [(0, 1, 200, 15, 15),   # line starts at column 0: J, T, Y, j reach left of the canvas
            (0, 0, 50, 3, 4),      # thin crops every 4 rows
            (7, 5, 40, 1, 6),      # one-row crops
            (100, 50, 300, 30, 9),  # past the right and the bottom of the page
            (119, 0, 10, 15, 15)]  # a one-column crop
    _agree(font, size, FOCR_DEFAULT_ALPHABET, 1.0, False, [page], geos)


@pytest.mark.parametrize("key", sorted(LARGEST_SIZE), ids=lambda k: f"{k[0][:-4]}-{k[1]}")
def test_builder_refuses_the_first_size_above_the_bound(key):
    font, alphabet = os.path.join(GOLD, key[0]), ALPHABETS[key[1]]
    size = LARGEST_SIZE[key]
    f = DecodeFont(font, size, alphabet)
    area = max(f.s.glyphs[i].stride * f.s.glyphs[i].box_h for i in range(f.s.n_glyphs))
    assert area * 2 * 255 * 255 < 2 ** 31
    f.close()
    with pytest.raises(DecoderError, match="glyph box too large"):
        DecodeFont(font, size + 1, alphabet)


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
def test_tie_groups_are_identical(font, hinting):
    """Every glyph of a tie group has the first one's increment and, in all 64 phases, its bitmap and offsets: else the
    GPU tie test would decide nothing."""
    perm = permuted_319()
    for al in (ALPHABET_319, perm):
        f = DecodeFont(font, 13.0, al, hinting)
        inc = f.increments()
        for grp in TIE_GROUPS:
            i0 = al.index(grp[0])
            for ch in grp[1:]:
                i = al.index(ch)
                assert inc[i] == inc[i0], (grp, ch)
                for p in range(64):
                    a, b = f.phase(i0, p), f.phase(i, p)
                    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (grp, ch, p)
        f.close()
    # the permuted alphabet puts each group on one lane, in 64-glyph stripes, in another order than the plain one
    assert sorted(perm) == sorted(ALPHABET_319) and len(set(ALPHABET_319)) == 319
    for grp in TIE_GROUPS:
        idx = sorted(perm.index(ch) for ch in grp)
        assert len({i % 64 for i in idx}) == 1 and len({i // 64 for i in idx}) == len(grp), grp
        assert min(grp, key=perm.index) != grp[0]
        assert len({ALPHABET_319.index(ch) % 64 for ch in grp}) == len(grp)  # plain: one lane each

"""Seeded cases for the focr decoder's whole-line decode under baseline candidates (tests/test_gpu_focr_whole_baseline.py),
in the style of tests/focr_fuzz_cases.py but small enough for the composed CPU model: N_CASES cases, each a function of
its index and SEED alone.  A case draws a font (Sans, Serif, Mono in turn), a size of 6 .. 16 px, a kerning of 0.8 .. 1.2,
hinting (on in every second triple of cases, so each font meets both), an alphabet of 2 .. 6 characters, B of 1 or 2 and a
radius of 1 .. 3, an x and a y that are not 0, a width of 40 .. 56 columns that the page clips in every second case, and
one page of two or three slots whose bottom edge cuts the last.  The ink is lines of random alphabet characters, each
glyph one FreeType raster on the decoder's own line canvas at the decoder's own pens, the baseline moved by a multiple of
2^-B px within the radius, and 1 % of the band's pixels salted.  Nothing here comes from the device path."""
import collections
import os

import numpy as np

from focr_fast_model import ASCII95
from font_ocr_amd.decoder import DecodeFont, raster_glyph

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FONTS = tuple(os.path.join(GOLD, f) for f in ("DejaVuSans.ttf", "DejaVuSerif.ttf", "DejaVuSansMono.ttf"))
SIZES = (6.0, 7.15, 9.0, 11.5, 13.0, 16.0)
KERNINGS = (0.8, 0.93, 1.0, 1.07, 1.2)
SEED = 0xB45E
N_CASES = 12

Case = collections.namedtuple("Case", "index font size kerning hinting alphabet y_bits n geo page")


def build(i):
    rng = np.random.default_rng([SEED, i])
    font, hinting = FONTS[i % 3], bool((i // 3) % 2)
    size = float(SIZES[int(rng.integers(0, len(SIZES)))])
    kerning = float(KERNINGS[int(rng.integers(0, len(KERNINGS)))])
    alphabet = "".join(ASCII95[k] for k in rng.permutation(len(ASCII95))[: int(rng.integers(2, 7))])
    y_bits, n = int(rng.integers(1, 3)), int(rng.integers(1, 4))
    x, y, width = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(40, 57))
    line_height = int(np.ceil(size)) + int(rng.integers(2, 6))
    line_advance = line_height + int(rng.integers(-2, 3))
    slots = int(rng.integers(2, 4))
    clip = int(rng.integers(1, 5)) if i % 2 else 0  # the page ends this many columns inside x + width
    cut = int(rng.integers(2, line_height))
    page = np.full((y + (slots - 1) * line_advance + cut, x + width - clip), 255, dtype=np.uint8)
    f = DecodeFont(font, size, alphabet, hinting, kerning)
    inc, (ox, oy) = f.increments(), f.origin
    f.close()
    H, Wp = page.shape
    for s in range(slots):
        if s and rng.random() < 0.3:
            continue  # a blank slot
        ly = y + s * line_advance
        h, w = min(line_height + 3, H - ly), Wp - x
        ty = F32(oy + F32(int(rng.integers(-n, n + 1))) / F32(1 << y_bits))
        band, pen = page[ly: ly + h, x:], F32(0)
        while pen < F32(w):
            k = int(rng.integers(0, len(alphabet)))
            g = np.zeros((h, w), dtype=np.uint8)
            raster_glyph(font, size, alphabet[k], F32(ox + pen), ty, g, hinting)
            np.minimum(band, 255 - g, out=band)
            pen = F32(pen + inc[k])
        salt = rng.random(band.shape) < 0.01
        band[salt] = rng.integers(0, 255, int(salt.sum()), dtype=np.uint8)
    return Case(i, font, size, kerning, hinting, alphabet, y_bits, n, (x, y, width, line_height, line_advance), page)


_cases = {}


def case(i):
    if i not in _cases:
        _cases[i] = build(i)
    return _cases[i]

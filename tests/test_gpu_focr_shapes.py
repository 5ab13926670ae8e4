"""The focr decoder and verify kernels (csrc/hip/decode.hip, decode_images.hip) at the shapes they branch on, against the fast model
(tests/focr_fast_model.py, proven equal to the brute-force model by tests/test_focr_fast_model.py) and the model's
draw_verify (tests/focr_line_model.py): lists exactly, images byte for byte, MSE as f32.  Each test asserts from the
geometry that it reaches the branch it names."""
import os

import numpy as np
import pytest

import focr_line_model as M
from focr_fast_model import ALPHABET_319, ASCII95, LARGEST_SIZE, TIE_GROUPS, FastModel, line_cap, narrowest_glyph_line, permuted_319
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder, VerifyFont
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
LDS_STRIP_MAX = 65536     # decode.hip: a strip up to this many bytes is staged in LDS, a larger one is read from global
COMPACT_THREADS = 1024    # decode.hip: line_compact_kernel's slots per iteration
VERIFY_TILE = (16, 256)   # decode.h: the compose kernels' tile, rows x columns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def _ink(alphabet):
    return "".join(c for c in alphabet if not c.isspace())


def strip_bytes(page_w, x, width, line_height):
    """focr_decoder_run's strip: crop width w clamped to the page, stride = ((w + 7) / 4 + 2) * 4 bytes per row."""
    w = min(width, page_w - min(x, page_w))
    return ((w + 7) // 4 + 2) * 4 * line_height


def n_slots(page_h, y, line_advance):
    return max(0, -(-(page_h - y) // line_advance))


def _draw(page, font, size, text, x, y, kerning=1.0, hinting=False):
    c = M.render_text(font, size, text, kerning, hinting)
    H, W = page.shape
    hh, ww = min(c.shape[0], H - y), min(c.shape[1], W - x)
    if hh > 0 and ww > 0:
        page[y: y + hh, x: x + ww] = np.minimum(page[y: y + hh, x: x + ww], 255 - c[:hh, :ww])


def _text(rng, alphabet, n):
    return "".join(rng.choice(list(alphabet), n))


def _check(dec, fm, pages, geo, font, size, kerning=1.0, hinting=False):
    """Decode and verify on the device: lists must equal the fast model's, images and MSE the model's draw_verify."""
    want = [fm.decode_image(p, *geo) for p in pages]
    got, mse, images = dec.decode(pages, *geo, verify="image")
    assert got == want
    for i, (p, lines) in enumerate(zip(pages, got)):
        img, m = M.verify_image(p, lines, font, size, geo[0], kerning, hinting)
        assert np.array_equal(images[i], img), i
        assert mse[i].tobytes() == np.float32(m).tobytes(), (i, mse[i], m)
    return got, images


def _raw_lines(dec):
    """The library's work-list order: [(page, y, n_chars)] as focr_decoder_get returns it."""
    n = dec._lib.focr_decoder_n_lines(dec._h)
    lines = (N.DecodedLine * max(1, n))()
    chars = np.zeros(max(1, dec._lib.focr_decoder_n_chars(dec._h)), dtype=np.uint16)
    assert dec._lib.focr_decoder_get(dec._h, lines, chars.ctypes.data) == 0
    return [(int(lines[k].page), int(lines[k].y), int(lines[k].n_chars)) for k in range(n)]


def test_lds_global_boundary(dec):
    """line_decode_kernel<true> with a strip of exactly 65536 bytes (w 1012) and <false> one dword per row past it
    (w 1013), on the same lines: two rows of Sans 24 px text per 64-row slot."""
    font, size, lh = SANS, 24.0, 64
    W, H = 1013, 3 * lh
    assert strip_bytes(W, 0, 1012, lh) == LDS_STRIP_MAX
    assert strip_bytes(W, 0, 1013, lh) == 65792 > LDS_STRIP_MAX
    rng = np.random.default_rng(31)
    pages = []
    for _ in range(2):
        page = np.full((H, W), 255, dtype=np.uint8)
        for s in range(3):
            for dy in (3, 33):
                _draw(page, font, size, _text(rng, FOCR_DEFAULT_ALPHABET, 85), 0, s * lh + dy)
        pages.append(page)
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    lds = _check(dec, fm, pages, (0, 0, 1012, lh, lh), font, size)[0]
    glob = _check(dec, fm, pages, (0, 0, 1013, lh, lh), font, size)[0]
    assert all(len(t) > 60 for pg in glob for _, t in pg)
    assert [[y for y, _ in pg] for pg in lds] == [[y for y, _ in pg] for pg in glob] == [[0, 64, 128]] * 2
    fm.close()


def test_wide_page_global_strip(dec):
    """A 300-dpi A4 width (2480 px) at a tall line height: the global-memory strip and 10 verify tiles per row."""
    font, size, kern, lh, adv = MONO, 24.0, 1.07, 40, 44
    W, H = 2480, 4 * adv + 10
    assert strip_bytes(W, 0, W, lh) > LDS_STRIP_MAX
    rng = np.random.default_rng(32)
    page = np.full((H, W), 255, dtype=np.uint8)
    for i in range(4):
        _draw(page, font, size, _text(rng, ASCII95, 170), 0, 3 + i * adv, kern)
    fm = FastModel(font, size, ASCII95, False, kern)
    dec.set_font(fm.font, size)
    got, _ = _check(dec, fm, [page], (0, 3, W, lh, adv), font, size, kern)
    assert len(got[0]) == 4 and all(len(t) > 150 for _, t in got[0])
    fm.close()


def _largest_size_page(font, size):
    """As tests/test_focr_fast_model.py's test_largest_accepted_size: one line of big glyphs, a fully inked block, noise."""
    rng = np.random.default_rng(2)
    page, _ = M.synth_page(rng, font, size, _ink(FOCR_DEFAULT_ALPHABET), 520, 240, 2, 2, 230, 1)
    page[10:200, 330:470] = 0
    return np.minimum(page, 255 - rng.integers(0, 40, page.shape)).astype(np.uint8)


def test_largest_accepted_size(dec):
    """Sans at the largest size the builder accepts: glyph boxes next to the int32 score bound, scores at their most
    negative over a fully inked block; a tall crop (global strip) and a thin crop that cuts the glyph boxes (LDS)."""
    font, size = SANS, LARGEST_SIZE[("DejaVuSans.ttf", "default")]
    with pytest.raises(DecoderError, match="glyph box too large"):
        DecodeFont(font, size + 1)
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    area = max(fm.font.s.glyphs[i].stride * fm.font.s.glyphs[i].box_h for i in range(fm.font.s.n_glyphs))
    assert 2 ** 30 < area * 2 * 255 * 255 < 2 ** 31
    page = _largest_size_page(font, size)
    dec.set_font(fm.font, size)
    tall, thin = (1, 2, 600, int(size) + 30, 400), (0, 60, 600, 9, 400)
    assert strip_bytes(520, 1, 600, tall[3]) > LDS_STRIP_MAX >= strip_bytes(520, 0, 600, thin[3])
    assert max(fm.font.s.glyphs[i].box_h for i in range(fm.font.s.n_glyphs)) > thin[3]
    for geo in (tall, thin):
        got, _ = _check(dec, fm, [page], geo, font, size)
        assert got[0]
    fm.close()


def _bench_pages(n_pages, seed, W=608, H=720, x=45, y=39, n_lines=40, advance=15, size=13.0):
    """tools/bench_focr.py's synthetic pages: DejaVu Sans Mono 13 px, 40 lines of up to 68 characters."""
    rng = np.random.default_rng(seed)
    ink = _ink(FOCR_DEFAULT_ALPHABET)
    pages = np.full((n_pages, H, W), 255, dtype=np.uint8)
    for p in range(n_pages):
        for i in range(n_lines):
            words = ["".join(rng.choice(list(ink), int(rng.integers(2, 10)))) for _ in range(12)]
            _draw(pages[p], MONO, size, " ".join(words)[:68], x, y + i * advance)
    return pages


def test_production_shape(dec):
    """The benchmark's geometry for 32 pages: 32 * 46 = 1472 slots, so line_compact_kernel loops past 1024."""
    font, size, geo = MONO, 13.0, (45, 39, 608, 12, 15)
    pages = _bench_pages(32, 1)
    assert len(pages) * n_slots(720, 39, 15) == 1472 > COMPACT_THREADS
    assert strip_bytes(608, 45, 608, 12) <= LDS_STRIP_MAX
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    got, _ = _check(dec, fm, list(pages), geo, font, size)
    assert all(len(pg) == 40 for pg in got)
    assert [(p, y) for p, y, _ in _raw_lines(dec)] == [(p, y) for p, pg in enumerate(got) for y, _ in pg]
    fm.close()


@pytest.mark.parametrize("n_pages,slots", [(33, 31), (16, 64), (25, 41), (7, 439)], ids=["1023", "1024", "1025", "3073"])
def test_compaction_boundaries(dec, n_pages, slots):
    """Mostly blank batches of n_pages * n_slots = 1023, 1024, 1025 and 3073 slots, with ink exactly on slots 1022, 1023,
    1024 and the last, and on a sparse random set: the work list must hold every inked slot, in (page, line) order."""
    font, size, adv, W = MONO, 13.0, 4, 24
    total = n_pages * slots
    rng = np.random.default_rng(total)
    inked = {s for s in (1022, 1023, 1024, total - 1) if s < total} | {int(s) for s in rng.choice(total, 25, replace=False)}
    pages = np.full((n_pages, slots * adv, W), 255, dtype=np.uint8)
    for s in inked:
        p, i = divmod(s, slots)
        c = int(rng.integers(0, W - 4))
        pages[p, i * adv + 1: i * adv + 3, c: c + 1 + s % 4] = int(rng.integers(0, 120))
    assert n_slots(slots * adv, 0, adv) == slots
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    got, _ = _check(dec, fm, list(pages), (0, 0, W, adv, adv), font, size)
    assert [(p, y) for p, y, _ in _raw_lines(dec)] == [(s // slots, s % slots * adv) for s in sorted(inked)]
    assert sum(len(pg) for pg in got) == len(inked)
    fm.close()


def _tie_page(font, W, seed):
    """As tests/test_focr_fast_model.py's _tie_page: lines that are mostly A, o and spaces."""
    rng = np.random.default_rng(seed)
    page = np.full((34, W), 255, dtype=np.uint8)
    for ly in (2, 18):
        text = "".join(rng.choice(list("AAoo  " + "xyzéŁž"), 30))
        _draw(page, font, 13.0, text, 1, ly)
    return page


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("order", ["plain", "permuted"])
def test_319_glyph_alphabet_ties(dec, font, order):
    """319 glyphs: five stripes of the per-lane argmin.  Plain, each tie group is spread over lanes; permuted, a group
    sits on one lane at i, i + 64, i + 128.  Either way the first listed member must win every tie."""
    al = ALPHABET_319 if order == "plain" else permuted_319()
    assert len(al) == 319 > 4 * 64
    page = _tie_page(font, 110, 5 + (font == SANS))
    fm = FastModel(font, 13.0, al)
    dec.set_font(fm.font, 13.0)
    got, _ = _check(dec, fm, [page], (0, 0, 200, 15, 16), font, 13.0)
    text = "".join(t for _, t in got[0])
    for grp in TIE_GROUPS:
        first = min(grp, key=al.index)
        lanes = {al.index(ch) % 64 for ch in grp}
        assert len(lanes) == (1 if order == "permuted" else len(grp))
        assert first in text and not any(ch in text for ch in grp if ch != first), (grp, first)
    fm.close()


def test_cap_reached_exactly(dec):
    """A Sans 13 px line of U+0027, the narrowest of the 319 glyphs, drawn at the decoder's own pen positions: the pen
    takes exactly the host's cap of steps (more than 64, so verify's layout takes two passes)."""
    font, size, W = SANS, 13.0, 300
    page, ch, cap = narrowest_glyph_line(font, size, ALPHABET_319, W)
    assert ch == "'" and cap > 64
    fm = FastModel(font, size, ALPHABET_319)
    assert cap == line_cap(fm.incs, W)
    dec.set_font(fm.font, size)
    got, _ = _check(dec, fm, [page], (0, 0, W, 16, 16), font, size)
    (y, text), = got[0]
    assert len(text) == cap and text[:-1] == ch * (cap - 1)
    fm.close()


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("kerning", [0.6, 0.85])
@pytest.mark.parametrize("hinting", [False, True], ids=["unhinted", "hinted"])
def test_overlapping_glyphs(dec, font, kerning, hinting):
    """Kerning below 1: neighbouring glyph boxes overlap, in the decoder's scores and in verify's last-rectangle-wins."""
    size = 13.0
    adv, lh = int(size * 1.2) + 2, int(size) + 2
    rng = np.random.default_rng(int(kerning * 100) + 2 * hinting + (font == SANS))
    a, _ = M.synth_page(rng, font, size, _ink(FOCR_DEFAULT_ALPHABET), 150, 4 * adv, 3, 2, adv, 4, kerning, hinting)
    b, _ = M.synth_page(rng, font, size, _ink(FOCR_DEFAULT_ALPHABET), 150, 4 * adv, 3, 2, adv, 4, kerning, hinting, noise=20)
    vf = VerifyFont(font, size, FOCR_DEFAULT_ALPHABET, hinting, kerning)
    ink = [i for i, ch in enumerate(FOCR_DEFAULT_ALPHABET) if not ch.isspace()]
    reach = sum(vf.box(i)[2] > vf.s.glyphs[i].increment for i in ink)  # the ink reaches past the next pen position
    assert reach > len(ink) // 2, reach
    vf.close()
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET, hinting, kerning)
    dec.set_font(fm.font, size)
    got, _ = _check(dec, fm, [a, b], (1, 2, 200, lh, adv), font, size, kerning, hinting)
    assert all(pg for pg in got)
    fm.close()


@pytest.mark.parametrize("W", [256, 257, 513, 2480])
def test_verify_tile_boundaries(dec, W):
    """Page widths around verify_compose_kernel's 256-column tiles; lines that cross columns 256 and 512 and rows at
    multiples of 16."""
    font, size, y0, lh, adv = SANS, 13.0, 3, 15, 13
    H = 70
    x = {256: 200, 257: 200, 513: 240, 2480: 0}[W]
    rng = np.random.default_rng(W)
    page = np.full((H, W), 255, dtype=np.uint8)
    for i in range(n_slots(H, y0, adv)):
        _draw(page, font, size, _text(rng, _ink(FOCR_DEFAULT_ALPHABET), 2 + (W - x) // 6), x, y0 + i * adv)
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    got, images = _check(dec, fm, [page], (x, y0, W, lh, adv), font, size)
    blue = images[0][..., 2] != 0
    th, tw = VERIFY_TILE
    for c in range(tw, W, tw):  # blue on both sides of every tile column boundary
        assert blue[:, c - 4: c].any() and blue[:, c: c + 4].any(), c
    if W > tw:
        assert blue[:, W - 3:].any()
    for r in range(th, H, th):  # and of every tile row boundary
        assert blue[r - 4: r, x:].any() and blue[r: r + 4, x:].any(), r
    fm.close()

"""Host side of focr --test: the model of its images (tests/focr_testimg_model.py) on cases worked out by hand, and
focr_image_load_rgba8 (image::open(..).into_rgba8()) on generated PNM and PNG files of every colour type, bit depth,
tRNS form and interlace, against the luma loader.  No GPU needed."""
import os
import struct
import zlib

import numpy as np
import pytest

import focr_testimg_model as T
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, load_image, load_image_rgba
from font_ocr_amd.decoder import render_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
F32 = np.float32


def _blend_scalar(bg, fg):
    """The crate's blend for one pixel, written out with np.float32 scalars in the crate's order."""
    m = F32(255.0)
    if fg[3] == 0:
        return tuple(bg)
    if fg[3] == 255:
        return tuple(fg)
    b = [F32(v) / m for v in bg]
    f = [F32(v) / m for v in fg]
    a = F32(F32(b[3] + f[3]) - F32(b[3] * f[3]))
    if a == F32(0):
        return tuple(bg)
    out = [int(F32(m * F32(F32(F32(f[c] * f[3]) + F32(F32(b[c] * b[3]) * F32(F32(1.0) - f[3]))) / a))) for c in range(3)]
    return tuple(out + [int(F32(m * a))])


def test_blend_model_matches_scalar_arithmetic():
    rng = np.random.default_rng(7)
    bg = rng.integers(0, 256, (3000, 4), dtype=np.uint8)
    fg = rng.integers(0, 256, (3000, 4), dtype=np.uint8)
    fg[:1000, 3] = 128
    fg[1000:1100, 3] = 0
    fg[1100:1200, 3] = 255
    bg[:200, 3] = 0
    got = T.blend(bg, fg)
    for i in range(len(bg)):
        assert tuple(int(v) for v in got[i]) == _blend_scalar([int(v) for v in bg[i]], [int(v) for v in fg[i]]), (bg[i], fg[i])


def test_blend_model_known_values():
    # red at half alpha over opaque white and over a transparent pixel; the output alpha is what the f32 arithmetic gives
    assert tuple(T.blend((255, 255, 255, 255), T.RED)) == _blend_scalar((255, 255, 255, 255), T.RED)
    over_clear = T.blend((10, 20, 30, 0), T.RED)
    assert tuple(over_clear[:3]) == (255, 0, 0) and over_clear[3] in (127, 128)
    # repeated blends converge: once a blend leaves the pixel as it was, every later one does too
    p = np.array([0, 200, 90, 40], np.uint8)
    seq = [p]
    for _ in range(40):
        seq.append(T.blend(seq[-1], T.RED))
    fixed = next(i for i in range(40) if np.array_equal(seq[i], seq[i + 1]))
    assert all(np.array_equal(seq[fixed], s) for s in seq[fixed:])
    assert np.array_equal(T.blend_times(p[None], T.RED, np.array([25])), seq[25][None])


def test_rect_counts_by_hand():
    luma = np.full((12, 10), 255, np.uint8)
    luma[1, 3] = 0      # slot 0 (y 0 .. 3) has ink
    luma[9, 3] = 0      # slot 2 (y 8 .. 11); slot 1 (y 4 .. 7) is blank
    k = T.rect_counts(luma, 2, 0, 4, 3, 4)
    want = np.zeros((12, 10), np.int64)
    for y0 in (0, 8):
        y1 = y0 + 3
        want[y0, 2:7] += 1
        if y1 < 12:
            want[y1, 2:7] += 1
        want[y0: min(y1, 11) + 1, 2] += 1
        want[y0: min(y1, 11) + 1, 6] += 1
    assert np.array_equal(k, want)
    assert k[0, 2] == 2 and k[3, 6] == 2 and k[5, 2] == 0


def test_rect_counts_overlap_clip_and_empty():
    luma = np.zeros((6, 5), np.uint8)
    # line_height 2, line_advance 1: every row meets three boxes; rows 1.. are on two horizontal edges; clipped right
    k = T.rect_counts(luma, 1, 0, 10, 2, 1)
    assert k.shape == (6, 5) and k[:, 0].sum() == 0
    assert k[0, 2] == 1 and k[2, 2] == 2 and k[2, 1] == 2 + 3  # two edges, three left sides through row 2
    assert np.array_equal(T.rect_counts(luma, 5, 0, 3, 2, 1), np.zeros((6, 5)))  # x past the page: every crop empty
    assert np.array_equal(T.rect_counts(luma, 0, 6, 3, 2, 1), np.zeros((6, 5)))  # y past the page: no slot
    one = T.rect_counts(luma, 0, 0, 4, 1, 1)  # line_height = line_advance = 1: every pixel on an edge
    assert one.min() >= 1
    with pytest.raises(ValueError):
        T.rect_counts(luma, 0, 0, 3, 2, 0)


@pytest.mark.parametrize("size,alphabet", [(13.0, FOCR_DEFAULT_ALPHABET), (24.0, "Ag/|")])
def test_text_model_matches_pixel_loop(size, alphabet):
    canvas = render_text(MONO, size, alphabet)
    rng = np.random.default_rng(3)
    for H, W in ((canvas.shape[0] + 3, 40), (5, canvas.shape[1] + 7)):
        base = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        assert np.array_equal(T.draw_test_text(canvas, base), T.draw_test_text_loop(canvas, base))


# ---- focr_image_load_rgba8 ----------------------------------------------------------------------------------------

ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def _pack_row(samples, depth):
    flat = samples.reshape(-1).astype(np.int64)
    if depth == 16:
        return b"".join(struct.pack(">H", int(v)) for v in flat)
    if depth == 8:
        return bytes(int(v) for v in flat)
    out, acc, bits = bytearray(), 0, 0
    for v in flat:
        acc, bits = (acc << depth) | int(v), bits + depth
        if bits == 8:
            out.append(acc)
            acc, bits = 0, 0
    if bits:
        out.append(acc << (8 - bits))
    return bytes(out)


def _png(samples, depth, ctype, interlace=0, plte=None, trns=None):
    H, W = samples.shape[:2]

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    raw = bytearray()
    for x0, y0, dx, dy in (ADAM7 if interlace else ((0, 0, 1, 1),)):
        sub = samples[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            for row in sub:
                raw += b"\x00" + _pack_row(row, depth)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace))
    if plte is not None:
        out += chunk(b"PLTE", bytes(int(v) for v in np.asarray(plte).reshape(-1)))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    return out + chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b"")


def _to8(v, depth, palette=False):
    v = v.astype(np.int64)
    if depth == 16:
        return (v + 128) // 257
    if depth == 8 or palette:
        return v
    return v * 255 // ((1 << depth) - 1)


def _expected(samples, depth, ctype, plte=None, trns=None):
    H, W = samples.shape[:2]
    out = np.zeros((H, W, 4), np.int64)
    out[..., 3] = 255
    s8 = _to8(samples, depth, ctype == 3)
    if ctype in (0, 4):
        out[..., :3] = s8[..., :1]
        if ctype == 4:
            out[..., 3] = s8[..., 1]
    elif ctype in (2, 6):
        out[..., :3] = s8[..., :3]
        if ctype == 6:
            out[..., 3] = s8[..., 3]
    else:
        idx = samples[..., 0]
        out[..., :3] = np.asarray(plte)[idx]
        alpha = np.full(256, 255)
        if trns is not None:
            alpha[: len(trns)] = list(trns)
        out[..., 3] = alpha[idx]
    if trns is not None and ctype in (0, 2):
        n = CHANNELS[ctype]
        key = [(trns[2 * k] << 8 | trns[2 * k + 1]) if depth == 16 else trns[2 * k + 1] for k in range(n)]
        out[np.all(samples[..., :n] == np.array(key), axis=-1), 3] = 0
    return out.astype(np.uint8)


def _luma_of(rgba):
    r, g, b = (rgba[..., c].astype(np.int64) for c in range(3))
    return ((2126 * r + 7152 * g + 722 * b) // 10000).astype(np.uint8)


def _cases():
    for ctype, depths in ((0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))):
        for depth in depths:
            for interlace in (0, 1):
                for trns in ((False, True) if ctype in (0, 2, 3) else (False,)):
                    yield ctype, depth, interlace, trns


@pytest.mark.parametrize("ctype,depth,interlace,trns", list(_cases()))
def test_rgba_loader_png(tmp_path, ctype, depth, interlace, trns):
    rng = np.random.default_rng(ctype * 1000 + depth * 10 + interlace)
    H, W = 11, 13  # odd sizes: partial bytes at low depths, Adam7 passes of unequal sizes
    n = CHANNELS[ctype]
    hi = (1 << depth) if ctype != 3 else min(1 << depth, 6)
    samples = rng.integers(0, hi, (H, W, n))
    plte = rng.integers(0, 256, (6, 3)) if ctype == 3 else None
    t = None
    if trns:
        if ctype == 3:
            t = [0, 77, 255]  # entries 3 .. 5 are past the list: alpha 255
        else:
            key = samples[2, 3]  # a key that occurs in the image
            t = b"".join(struct.pack(">H", int(v)) for v in key)
            t = list(t)
    path = tmp_path / "p.png"
    path.write_bytes(_png(samples, depth, ctype, interlace, plte, t))
    got = load_image_rgba(path)
    want = _expected(samples, depth, ctype, plte, t)
    assert got.shape == (H, W, 4) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    if trns and ctype != 3:
        assert got[2, 3, 3] == 0
    assert np.array_equal(_luma_of(got), load_image(path))  # the luma loader is into_luma8 of the same decode


def _pnm(kind, samples, maxval):
    H, W = samples.shape[:2]
    head = f"P{kind}\n# c\n{W} {H}\n".encode() + (b"" if kind in (1, 4) else f"{maxval}\n".encode())
    if kind in (1, 2, 3):
        return head + " ".join(str(int(v)) for v in samples.reshape(-1)).encode() + b"\n"
    if kind == 4:
        return head + b"".join(_pack_row(row, 1) for row in samples)
    return head + b"".join(_pack_row(row, 16 if maxval > 255 else 8) for row in samples)


@pytest.mark.parametrize("kind,maxval", [(1, 1), (4, 1), (2, 255), (2, 1000), (3, 255), (3, 40000), (5, 255), (5, 100), (5, 65535),
                                         (6, 255), (6, 300)])
def test_rgba_loader_pnm(tmp_path, kind, maxval):
    rng = np.random.default_rng(kind * 7 + maxval)
    n = 3 if kind in (3, 6) else 1
    samples = rng.integers(0, maxval + 1, (7, 9, n))
    path = tmp_path / "p.pnm"
    path.write_bytes(_pnm(kind, samples, maxval))
    got = load_image_rgba(path)
    if kind in (1, 4):
        v = np.where(samples == 1, 0, 255)
    elif maxval > 255:
        v = (samples.astype(np.int64) * 65535 // maxval + 128) // 257
    else:
        v = samples
    want = np.zeros((7, 9, 4), np.uint8)
    want[..., :3] = v if n == 3 else np.repeat(v, 3, axis=-1)
    want[..., 3] = 255
    assert np.array_equal(got, want)
    assert np.array_equal(_luma_of(got), load_image(path))


def test_rgba_loader_errors(tmp_path):
    with pytest.raises(OSError, match="cannot read"):
        load_image_rgba(tmp_path / "missing.png")
    (tmp_path / "x.bmp").write_bytes(b"BM" + bytes(60))
    with pytest.raises(OSError, match="unsupported"):
        load_image_rgba(tmp_path / "x.bmp")

"""The focr decoder's whole-line decode with pen slack (line_whole_slack_kernel, focr_decoder_set_whole_slack,
LineDecoder.decode(whole_line=True, pen_slack=N), focr --whole-line --pen-slack) against tests/focr_slack_model.py, the
definition of include/focr_decode.h restated on the fast model and pinned to FreeType by tests/test_focr_slack_model.py.
Every quantity is an exact integer, so characters, pens, offsets and costs are compared with ==.  Each test asserts from
its geometry, or from the model's answer, that it reaches the case it names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_search_model as S
import focr_slack_model as K
import focr_whole_model as W
from focr_fast_model import FastModel, crop
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder, VerifyFont, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536           # decode_line.h: strip, cost ring, live list and G share this much LDS, else the strip is read from global
WHOLE_SLACK_MISC_BYTES = 5184   # decode_whole.hip: the end keys, the counts, the live list and G
WHOLE_BATCH_MAX = 512           # decode_whole.hip: render pens per batch at most
WHOLE_RING_MAX = 4096           # decode_whole.hip: keys of the cost ring at most
TEXT = "burn clip ffH vvill rnrn cl"
SMALL = "burn clif"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


_models, _lines = {}, {}


def model(font, size, alphabet):
    key = (font, size, alphabet)
    if key not in _models:
        _models[key] = FastModel(font, size, alphabet)
    return _models[key]


def want_line(fm, line, n):
    """The model's Slack of one crop, computed once per (model, crop, N)."""
    key = (id(fm), n, line.shape, line.tobytes())
    if key not in _lines:
        _lines[key] = K.slack_line(fm, line, n)
        K.check_invariants(fm, _lines[key])
    return _lines[key]


def want_pages(fm, pages, n, x, y, width, line_height, line_advance):
    """[[(y, Slack)] per page], over the crops FastModel.decode_image walks."""
    out = []
    for page in pages:
        out.append([])
        i = 0
        while True:
            ly = y + i * line_advance
            i += 1
            line = crop(page, x, ly, width, line_height)
            if line.shape[0] == 0:
                break
            if not np.all(line == 255):
                out[-1].append((ly, want_line(fm, np.ascontiguousarray(line), n)))
    return out


def ring_length(fm, n):
    inc = W.inc64(fm.incs)
    need, r = K.batch(fm.incs, n) + 2 * n + int(inc.max()), 64
    while r < need:
        r *= 2
    return r


def strip_bytes(w, line_height):
    return ((w + 7) // 4 + 2) * 4 * line_height


def same(got, want):
    """A decode(whole_line=True, pen_slack=N) result against the model's pages."""
    lines, pens, costs, offsets = got
    assert lines == [[(y, s.text) for y, s in pg] for pg in want]
    assert [len(pg) for pg in pens] == [len(pg) for pg in costs] == [len(pg) for pg in offsets] == [len(pg) for pg in lines]
    for p, (pen_pg, cost_pg, off_pg, want_pg) in enumerate(zip(pens, costs, offsets, want)):
        for pen, cost, off, (y, s) in zip(pen_pg, cost_pg, off_pg, want_pg):
            assert pen.dtype == np.uint32 and np.array_equal(pen, s.pens), (p, y)
            assert off.dtype == np.int8 and np.array_equal(off, s.offsets), (p, y)
            assert cost == s.cost, (p, y)


def check(dec, fm, pages, geo, n):
    """Decode whole lines with slack n: line order, texts, pens, offsets and costs equal to the model's, in 3 launches.
    Returns the model's pages."""
    want = want_pages(fm, pages, n, *geo)
    same(dec.decode(pages, *geo, whole_line=True, pen_slack=n), want)
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    return want


def snapped(font, size, alphabet, text, width, snap, advance=1.0):
    page = np.full((W.alphabet_height(font, size, alphabet), width), 255, dtype=np.uint8)
    return S.draw_snapped(page, font, size, alphabet, text, 0, 0, snap, advance)


def put(page, line, y, x=0):
    h, w = min(line.shape[0], page.shape[0] - y), min(line.shape[1], page.shape[1] - x)
    page[y: y + h, x: x + w] = np.minimum(page[y: y + h, x: x + w], line[:h, :w])


def crossings(fm, s, n):
    """The characters of a model result whose arrival state p - j and render pen p fall in different batches: (those
    with j > 0, those with j < 0)."""
    B = K.batch(fm.incs, n)
    p, j = s.pens.astype(np.int64), s.offsets.astype(np.int64)
    other = (p - j) // B != p // B
    return int((other & (j > 0)).sum()), int((other & (j < 0)).sum())


@pytest.mark.parametrize("n", [8, 32])
@pytest.mark.parametrize("snap,advance", [("floor", 1.0), ("exact", 1.01)], ids=["floor", "x1.01"])
def test_proportional_pages_off_the_grid(dec, snap, advance, n):
    """Sans 13 px, the default alphabet, a 150-column crop of the table's line: B = 231 - N, dozens of batches and many
    ring lengths a line.  The advance page reads whole at both radii and the floored one at N = 32; without slack the
    whole-line run loses both."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(SANS, 13.0, al)
    line = snapped(SANS, 13.0, al, TEXT, 150, snap, advance)
    h, w = line.shape
    assert K.batch(fm.incs, n) == 231 - n < WHOLE_BATCH_MAX and 64 * w > 4 * ring_length(fm, n)
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, w, h, h), n)[0]
    assert s.offsets.any() and (s.text.startswith(TEXT[:-3]) or (snap, n) == ("floor", 8))
    plain = dec.decode([line], 0, 0, w, h, h, whole_line=True)
    assert not plain[0][0][0][1].startswith(TEXT[:-3])


def test_monospace_batches_of_512(dec):
    """Mono 32 px, four glyphs, a short line with every pen rounded to whole pixels: min inc64 - N is above 512, so
    B = 512 and most batches are empty."""
    al, n = "AB >", 8
    fm = model(MONO, 32.0, al)
    assert K.batch(fm.incs, n) == WHOLE_BATCH_MAX < int(W.inc64(fm.incs).min()) - n
    line = snapped(MONO, 32.0, al, "AB>A", 100, "round")
    dec.set_font(fm.font, 32.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]), n)[0]
    assert s.text[:4] == "AB>A" and s.offsets.any()


def test_characters_across_batch_edges(dec):
    """Sans 13 px with rounded pens at N = 32: the model's solution has a character whose arrival state lies in the batch
    before its render pen's (j > 0: the window reads the last states of the batch before, which the lagged clear must
    have kept) and one whose arrival state lies in the batch after (j < 0: the window reads ahead of the batch)."""
    al, n = FOCR_DEFAULT_ALPHABET, 32
    fm = model(SANS, 13.0, al)
    line = snapped(SANS, 13.0, al, TEXT, 150, "round")
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, 150, line.shape[0], line.shape[0]), n)[0]
    up, down = crossings(fm, s, n)
    assert up >= 1 and down >= 1


def test_first_character_takes_a_positive_offset(dec):
    """Text drawn 24/64 px right of x: state 0 is the only one reachable at first, so the first character's render pen is
    its offset, 24, and no character can reach left of it."""
    al, n = SMALL, 32
    fm = model(SANS, 13.0, al)
    line = K.draw_at(SANS, 13.0, al, SMALL, K.font_pens(fm, SMALL, 24), 70)
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, 70, line.shape[0], line.shape[0]), n)[0]
    assert s.text[: len(SMALL)] == SMALL and s.offsets[0] == s.pens[0] == 24 and s.offsets.min() >= 0


@pytest.mark.parametrize("size,n,width", [(13.0, 64, 70), (6.0, 53, 40)], ids=["sans13-64", "sans6-53"])
def test_largest_radius(dec, size, n, width):
    """N = min(64, min inc64 / 2): 64 at 13 px, and 53 at 6 px, where B = 54 is barely above N; one more is refused."""
    al = SMALL
    fm = model(SANS, size, al)
    assert n == K.max_slack(fm.incs) == min(64, int(W.inc64(fm.incs).min()) // 2)
    line = snapped(SANS, size, al, SMALL, width, "floor")
    dec.set_font(fm.font, size)
    (_, s), = check(dec, fm, [line], (0, 0, width, line.shape[0], line.shape[0]), n)[0]
    assert np.abs(s.offsets.astype(int)).max() > 32
    if n < 64:
        with pytest.raises(DecoderError, match="more than half the smallest inc64 .*could crawl"):
            dec.decode([line], 0, 0, width, line.shape[0], line.shape[0], whole_line=True, pen_slack=n + 1)
        check(dec, fm, [line], (0, 0, width, line.shape[0], line.shape[0]), n)


def _plain_whole(d, pages, geo):
    lines, pens, costs = d.decode(pages, *geo, whole_line=True)
    return lines, [[p.tobytes() for p in pg] for pg in pens], costs


def test_no_slack_through_the_setter_is_the_whole_line_run(dec):
    """focr_decoder_set_whole_slack(0) and a whole-line run: byte-equal to a decoder that never heard of the slack, in the
    same 3 launches, with all-zero offsets; and the Python API with pen_slack=0 returns the whole-line run's three."""
    al = FOCR_DEFAULT_ALPHABET
    line = snapped(SANS, 13.0, al, TEXT, 150, "floor")
    h, w = line.shape
    pages = np.full((2, 3 * h, w), 255, dtype=np.uint8)
    put(pages[0], line, 0), put(pages[1], W.draw_line(SANS, 13.0, al, "i" * 30, width=w), 2 * h)
    geo = (0, 0, w, h, h)
    with LineDecoder(0) as fresh:
        fresh.set_font(SANS, 13.0)
        want = _plain_whole(fresh, pages, geo)
        launches = fresh._lib.focr_decoder_last_launches(fresh._h)
    dec.set_font(SANS, 13.0)
    dec.decode(pages, *geo, whole_line=True, pen_slack=8)
    assert dec._lib.focr_decoder_set_whole_slack(dec._h, 0) == 0
    dec._pen_slack = 0
    assert _plain_whole(dec, pages, geo) == want
    assert dec._lib.focr_decoder_last_launches(dec._h) == launches == 3
    offs = np.ones(dec._lib.focr_decoder_n_chars(dec._h), dtype=np.int8)
    assert dec._lib.focr_decoder_get_offsets(dec._h, offs.ctypes.data) == 0 and not offs.any()
    got = dec.decode(pages, *geo, whole_line=True, pen_slack=0)
    assert len(got) == 3 and (got[0], [[p.tobytes() for p in pg] for pg in got[1]], got[2]) == want


def test_three_lines_through_one_workgroup(dec):
    """Three different lines on a grid of one workgroup: the ring, G, the backpointer scratch and the offset scratch of
    one line must not leak into the next; the results equal the model's and a run's on the decoder's own grid."""
    al, n = SMALL, 8
    fm = model(SANS, 13.0, al)
    h = W.alphabet_height(SANS, 13.0, al)
    pages = np.full((2, 3 * h, 70), 255, dtype=np.uint8)
    put(pages[0], snapped(SANS, 13.0, al, "burn clif", 70, "floor"), 0)
    put(pages[0], snapped(SANS, 13.0, al, "ffill bull", 70, "exact", 1.01), 2 * h)
    put(pages[1], snapped(SANS, 13.0, al, "i" * 16, 70, "round"), h)
    dec.set_font(fm.font, 13.0)
    geo = (0, 0, 70, h, h)
    assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 1) == 0
    try:
        want = check(dec, fm, pages, geo, n)
        one = dec.decode(pages, *geo, whole_line=True, pen_slack=n)
    finally:
        assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 0) == 0
    assert sum(len(pg) for pg in want) == 3 and len({s.text for pg in want for _, s in pg}) == 3
    assert all(s.offsets.any() for pg in want for _, s in pg)
    same(one, want)
    check(dec, fm, pages, geo, n)  # and on the decoder's own grid


@pytest.mark.parametrize("width", [660, 700])
def test_strip_in_lds_and_in_global_memory(dec, width):
    """Mono 32 px, four glyphs, 64-row slots, N = 4: at width 660 strip, ring, live list and G fit the LDS budget; at 700
    they do not, and the strip is read from global memory."""
    al, lh, n = "AB >", 64, 4
    fm = model(MONO, 32.0, al)
    lds = strip_bytes(width, lh) + WHOLE_SLACK_MISC_BYTES + 8 * ring_length(fm, n)
    assert (lds <= LDS_STRIP_MAX) == (width == 660) and 8 * ring_length(fm, n) + WHOLE_SLACK_MISC_BYTES < LDS_STRIP_MAX
    rng = np.random.default_rng(width)
    page = np.full((lh, 700), 255, dtype=np.uint8)
    put(page, W.draw_line(MONO, 32.0, al, "".join(rng.choice(list(al), 40)), width=700, height=40), 10)
    page[:, 650:] = np.minimum(page[:, 650:], 200)  # ink in the columns the widths differ by
    dec.set_font(fm.font, 32.0)
    (_, s), = check(dec, fm, [page], (0, 0, width, lh, lh), n)[0]
    assert len(s.text) >= width // 20 and s.offsets.any()


def test_character_bound_is_filled(dec):
    """Sans 13 px, "il ", 63 columns: nineteen "i" drawn 223/64 px apart, the smallest gain a step can have at N = 8, fill
    ceil(64 * 63 / (231 - 8)) = 19 places, one more than the plain whole-line bound: the line cap is sized from the new
    bound."""
    al, n, w = "il ", 8, 63
    fm = model(SANS, 13.0, al)
    gain = int(W.inc64(fm.incs).min()) - n
    bound = K.char_bound(fm.incs, w, n)
    assert (gain, bound) == (223, 19) and bound == W.char_bound(fm.incs, w) + 1
    line = K.draw_at(SANS, 13.0, al, "i" * bound, np.arange(bound) * gain, w)
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, w, line.shape[0], line.shape[0]), n)[0]
    assert s.text == "i" * bound and s.offsets.tolist() == [0] + [-n] * (bound - 1)


def test_verify_draws_every_character_at_its_render_pen(dec):
    """After a slack run on the floored Sans line the verify image and sums are draw_verify with every character at
    pos = p / 64 of its returned render pen, and the page's error is below the plain whole-line run's.  The alphabet is
    the one of the whole-line verify test, whose origin_x is 0."""
    al, n = "burn clipfHvmd", 32
    fm = model(SANS, 13.0, al)
    assert float(fm.ox) == 0
    line = snapped(SANS, 13.0, al, TEXT, 150, "floor")
    h, w = line.shape
    page = np.full((h + 9, w + 12), 255, dtype=np.uint8)
    put(page, line, 4, 5)
    geo = (5, 4, w, h, h)
    dec.set_font(fm.font, 13.0)
    want = want_pages(fm, [page], n, *geo)
    got = dec.decode([page], *geo, verify="image", whole_line=True, pen_slack=n)
    assert len(got) == 6
    lines, mse, images = got[:3]
    same((lines,) + got[3:], want)
    assert want[0][0][1].offsets.any()
    vf = VerifyFont(SANS, 13.0, al)
    img, sq = W.verify_image(page, [(y, s.text, s.pens) for y, s in want[0]], fm.font, vf, geo[0])
    vf.close()
    assert np.array_equal(images[0], img)
    sums, _ = dec.verify(images=False)
    assert int(sums[0]) == sq and mse[0].tobytes() == (np.float32(sq) / np.float32(page.size)).tobytes()
    assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
    _, plain_mse, _, _, _ = dec.decode([page], *geo, verify="mse", whole_line=True)
    assert mse[0] < plain_mse[0]


def test_cli(dec, tmp_path):
    """focr --whole-line --pen-slack 8 --verify on two PGMs: stdout is the Python API's text and the MSEs on stderr its
    verify's."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    al = FOCR_DEFAULT_ALPHABET
    a, b = snapped(SANS, 13.0, al, TEXT, 150, "exact", 1.01), snapped(SANS, 13.0, al, TEXT, 150, "exact", 0.99)
    h, w = a.shape
    pages = np.full((2, 2 * h, w), 255, dtype=np.uint8)
    put(pages[0], a, h), put(pages[1], b, 0)
    paths, vdir = [str(tmp_path / ("page%d.pgm" % i)) for i in range(2)], tmp_path / "v"
    for path, page in zip(paths, pages):
        save_pgm(path, page)
    vdir.mkdir()
    cmd = [FOCR, "-f", SANS, "-t", "13", "-w", str(w), "--line-height", str(h), "--line-advance", str(h), "--whole-line", "-i"] + paths
    r = subprocess.run(cmd + ["--pen-slack", "8", "--verify", str(vdir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    dec.set_font(SANS, 13.0)
    lines, mse, _, _, _, offsets = dec.decode(pages, 0, 0, w, h, h, verify="mse", whole_line=True, pen_slack=8)
    assert r.stdout == "".join(t + "\n" for pg in lines for _, t in pg) and r.stdout.count(TEXT[:-3]) == 2
    assert r.stderr.splitlines() == ["%s %.6f" % (p, m) for p, m in zip(paths, mse)] and sorted(os.listdir(vdir)) == ["page0.png", "page1.png"]
    assert all(o.any() for pg in offsets for o in pg)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count(TEXT[:-3]) == 0


def test_switching_back(dec):
    """The switch turned off again gives the earlier whole-line result, offsets of zero included, and on again the
    slack's."""
    al, n = SMALL, 8
    fm = model(SANS, 13.0, al)
    line = snapped(SANS, 13.0, al, "burn clif", 70, "floor")
    geo = (0, 0, 70, line.shape[0], line.shape[0])
    dec.set_font(fm.font, 13.0)
    before = _plain_whole(dec, [line], geo)
    want = check(dec, fm, [line], geo, n)
    assert _plain_whole(dec, [line], geo) == before
    offs = np.ones(dec._lib.focr_decoder_n_chars(dec._h), dtype=np.int8)
    assert dec._lib.focr_decoder_get_offsets(dec._h, offs.ctypes.data) == 0 and not offs.any()
    assert before[0] != [[(y, s.text) for y, s in pg] for pg in want] or before[2] != [[s.cost for _, s in pg] for pg in want]
    check(dec, fm, [line], geo, n)
    plain = dec.decode([line], *geo)  # and the plain decoder after both
    with LineDecoder(0) as fresh:
        fresh.set_font(SANS, 13.0, al)
        assert fresh.decode([line], *geo) == plain


def _raw_run(dec, page, x, y, width, line_height, line_advance):
    """focr_decoder_run of one page with whatever state the library is in: (return code, its message)."""
    page = np.ascontiguousarray(page)
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], x, y, width, line_height,
                                   line_advance)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def test_refusals(dec):
    """Every refusal of include/focr_decode.h, each with its own message; the decoder decodes afterwards."""
    al = SMALL
    fm = model(SANS, 13.0, al)
    line = snapped(SANS, 13.0, al, "burn clif", 70, "floor")
    geo = (0, 0, 70, line.shape[0], line.shape[0])
    lib, h = dec._lib, dec._h
    dec.set_font(fm.font, 13.0)
    dec.decode([line], *geo)  # every switch off
    # the setter's own bound
    assert lib.focr_decoder_set_whole_slack(h, 65) != 0 and b"focr_decoder_set_whole_slack" in lib.focr_decoder_last_error(h)
    # slack on with the whole-line decode off, and beside margins: states of the library the Python API never makes
    assert lib.focr_decoder_set_whole_slack(h, 8) == 0
    rc, msg = _raw_run(dec, line, *geo)
    assert rc != 0 and "whole-line decode off" in msg and "focr_decoder_set_whole_slack" in msg and "focr_decoder_set_whole_line" in msg
    assert lib.focr_decoder_set_whole_line(h, 1) == 0 and lib.focr_decoder_set_whole_margins(h, 1) == 0
    rc, msg = _raw_run(dec, line, *geo)
    assert rc != 0 and "margins on" in msg and "focr_decoder_set_whole_slack" in msg and "focr_decoder_set_whole_margins" in msg
    assert lib.focr_decoder_get_pens(h, None, None) != 0  # the failed run left no result
    assert lib.focr_decoder_set_whole_margins(h, 0) == 0 and lib.focr_decoder_set_whole_line(h, 0) == 0
    assert lib.focr_decoder_set_whole_slack(h, 0) == 0
    with pytest.raises(ValueError):
        dec.decode([line], *geo, pen_slack=8)
    with pytest.raises(ValueError):
        dec.decode([line], *geo, whole_line=True, margins=True, pen_slack=8)
    with pytest.raises(ValueError, match="does not go with pen_search"):
        dec.decode([line], *geo, whole_line=True, pen_search=8)
    # 2 * N > min inc64: 107 at 6 px
    fm6 = model(SANS, 6.0, al)
    dec.set_font(fm6.font, 6.0)
    with pytest.raises(DecoderError, match="more than half the smallest inc64 .*could crawl"):
        dec.decode([snapped(SANS, 6.0, al, "burn", 40, "floor")], 0, 0, 40, 6, 6, whole_line=True, pen_slack=K.max_slack(fm6.incs) + 1)

    def hand_built(size=13.0, alphabet="AB", **change):
        df = DecodeFont(MONO, size, alphabet)
        if "increment" in change:
            df.s.glyphs[0].increment = change["increment"]
        dec.set_font(df, size)
        return df

    # a ring above WHOLE_RING_MAX only with the slack: inc64 3590 and 501, so 501 + 3590 fits and 493 + 16 + 3590 does not
    df = hand_built(increment=3590 / 64)
    mono_line = W.draw_line(MONO, 13.0, "AB", "ABBA")
    mgeo = (0, 0, mono_line.shape[1], mono_line.shape[0], mono_line.shape[0])
    assert 501 + 3590 <= WHOLE_RING_MAX < 501 - 8 + 16 + 3590
    dec.decode([mono_line], *mgeo, whole_line=True)
    with pytest.raises(DecoderError, match="with pen slack: the widest advance and the slack are too large .*cost ring does not fit in LDS"):
        dec.decode([mono_line], *mgeo, whole_line=True, pen_slack=8)
    df.close()
    # the cost bound with the new character bound: inc64 2 and N = 1 make 64 * w characters possible where 32 * w were
    df = hand_built(size=60.0, increment=2.0 / 64)
    T = max(df.s.glyphs[i].stride * df.s.glyphs[i].box_h * 2 * 255 * 255 for i in range(2))
    w = -(-(1 << 47) // (64 * T))  # the first width with 64 * w * T >= 2^47
    assert 64 * w * T >= 1 << 47 > 32 * w * T and 64 * w + int(W.inc64(np.array([df.s.glyphs[1].increment])).max()) < 1 << 24
    wide = np.full((1, w), 255, dtype=np.uint8)
    wide[0, 5] = 0
    with pytest.raises(DecoderError, match=r"reaches 2\^47 .a packed cost could overflow"):
        dec.decode([wide], 0, 0, w, 1, 1, whole_line=True, pen_slack=1)
    df.close()
    dec.set_font(fm.font, 13.0)
    check(dec, fm, [line], geo, 8)


def test_memory_returns():
    """A decoder that ran whole lines with slack, with a verify, gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    line = W.draw_line(MONO, 13.0, "AB >", "AB > BA")
    geo = (0, 0, line.shape[1], line.shape[0], line.shape[0])
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, "AB >")
        d.decode([line], *geo, whole_line=True)
        off = N.hip().focr_debug_device_bytes()
        d.decode([line], *geo, whole_line=True, pen_slack=8, verify="mse")
        assert before < off < N.hip().focr_debug_device_bytes()  # the offset scratch and the offsets are the slack's own
    assert N.hip().focr_debug_device_bytes() == before

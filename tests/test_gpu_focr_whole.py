"""The focr decoder's whole-line decode (line_whole_kernel, focr_decoder_set_whole_line / focr_decoder_get_pens,
LineDecoder.decode(whole_line=True), focr --whole-line) against tests/focr_whole_model.py, the definition of
include/focr_decode.h restated on the fast model and pinned to FreeType by tests/test_focr_whole_model.py.  Every
quantity is an exact integer, so characters, pens and costs are compared with ==.  Each test asserts from its geometry,
or from the model's answer, that it reaches the case it names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_whole_model as W
from focr_fast_model import ALPHABET_319, TIE_GROUPS, FastModel
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder, VerifyFont, save_pgm
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536      # decode_line.h: strip, cost ring and live list share this much LDS, else the strip is read from global
WHOLE_MISC_BYTES = 1088    # decode_whole.hip: the end keys, the counts and the live list
WHOLE_BATCH_MAX = 512      # decode_whole.hip: states per batch at most
TEXT = "burn clip ffH vvill rnrn cl"  # the line the greedy loop decodes as "bunY dm+Tl vvillmmY d>" in Sans 13

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


def want_line(fm, line):
    """The model's Whole of one crop, computed once per (model, crop)."""
    key = (id(fm), line.shape, line.tobytes())
    if key not in _lines:
        _lines[key] = W.whole_line(fm, line)
    return _lines[key]


def want_pages(fm, pages, x, y, width, line_height, line_advance):
    """[[(y, Whole)] per page], over the crops FastModel.decode_image walks."""
    from focr_fast_model import crop
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
                out[-1].append((ly, want_line(fm, np.ascontiguousarray(line))))
    return out


def ring_length(fm):
    inc = W.inc64(fm.incs)
    need, n = min(int(inc.min()), WHOLE_BATCH_MAX) + int(inc.max()), 64
    while n < need:
        n *= 2
    return n


def strip_bytes(w, line_height):
    return ((w + 7) // 4 + 2) * 4 * line_height


def check(dec, fm, pages, geo):
    """Decode whole lines: line order, texts, pens and costs equal to the model's.  Returns the model's pages."""
    want = want_pages(fm, pages, *geo)
    lines, pens, costs = dec.decode(pages, *geo, whole_line=True)
    assert lines == [[(y, s.text) for y, s in pg] for pg in want]
    assert [len(pg) for pg in pens] == [len(pg) for pg in costs] == [len(pg) for pg in lines]
    for p, (pen_pg, cost_pg, want_pg) in enumerate(zip(pens, costs, want)):
        for got, cost, (y, s) in zip(pen_pg, cost_pg, want_pg):
            assert got.dtype == np.uint32 and np.array_equal(got, s.pens), (p, y)
            assert cost == s.cost, (p, y)
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    return want


def put(page, line, y, x=0):
    h, w = min(line.shape[0], page.shape[0] - y), min(line.shape[1], page.shape[1] - x)
    page[y: y + h, x: x + w] = np.minimum(page[y: y + h, x: x + w], line[:h, :w])


def test_proportional_line_in_a_batch(dec):
    """Sans 13 px, the default alphabet: the table's line and forty "i" in a 3-page batch of four slots a page, with blank
    slots between the inked ones and a blank page.  The greedy run of the same pages loses both lines.  The lines are
    dozens of ring lengths long, so every ring slot is reused many times."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(SANS, 13.0, al)
    a, b = W.draw_line(SANS, 13.0, al, TEXT), W.draw_line(SANS, 13.0, al, "i" * 40, width=157)
    h, w = a.shape
    assert (h, w) == (13, 157) and 64 * w > 4 * ring_length(fm)
    pages = np.full((3, 4 * h, w), 255, dtype=np.uint8)
    put(pages[0], a, 0), put(pages[0], b, 2 * h), put(pages[2], a, 3 * h)
    dec.set_font(fm.font, 13.0)
    want = check(dec, fm, pages, (0, 0, w, h, h))
    assert [[y for y, _ in pg] for pg in want] == [[0, 2 * h], [], [3 * h]]
    assert want[0][0][1].text[:-1] == TEXT and want[0][1][1].text[:40] == "i" * 40
    plain = dec.decode(pages, 0, 0, w, h, h)
    assert plain[0][0] == (0, "bunY dm+Tl vvillmmY d>") and plain[2][0][1] == plain[0][0][1]


def test_monospace_line(dec):
    """Mono 13 px: every glyph advances by 501/64 px, so one state in 501 is reachable and most batches are empty.  The
    programme returns what the plain run returns."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(MONO, 13.0, al)
    assert set(W.inc64(fm.incs).tolist()) == {501}
    line = W.draw_line(MONO, 13.0, al, TEXT)
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    assert s.text[: len(TEXT)] == TEXT and np.all(s.pens % 501 == 0)
    assert dec.decode([line], 0, 0, line.shape[1], line.shape[0], line.shape[0]) == [[(0, s.text)]]


def test_ties_between_identical_glyphs(dec):
    """ALPHABET_319 in Mono 13 px with every tie group on the page: identical glyphs tie in cost at every state, and the
    lowest index is the one remembered."""
    al = ALPHABET_319
    fm = model(MONO, 13.0, al)
    text = "Ao \u0391\u03bf \u0410\u043e A"  # Latin, Greek, Cyrillic
    line = W.draw_line(MONO, 13.0, al, text)
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    assert s.text[: len(text)] == "Ao Ao Ao A"
    for grp in TIE_GROUPS:
        first = min(grp, key=al.index)
        assert first in s.text and not set(grp) - {first} & set(s.text), grp


def test_ties_between_glyphs_of_one_advance(dec):
    """Sans 13 px, "bdpqo il": b, d, p and q share one inc64, so from any state they land on the same state and the
    lowest (cost, index) of the four is the one pushed."""
    al = "bdpqo il"
    fm = model(SANS, 13.0, al)
    inc = W.inc64(fm.incs)
    assert len({int(inc[al.index(c)]) for c in "bdpq"}) == 1 and len(set(inc.tolist())) >= 3
    line = W.draw_line(SANS, 13.0, al, "bdpq lid dip")
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [line], (0, 0, line.shape[1], line.shape[0], line.shape[0]))[0]
    assert s.text[:12] == "bdpq lid dip"


def test_several_lines_per_workgroup(dec):
    """Seven non-blank lines on a grid of two workgroups: each takes three or four lines in turn, and the cost ring and
    the backpointer scratch of one line must not leak into the next."""
    al = "burn clif"
    fm = model(SANS, 13.0, al)
    texts = ["burn clif", "ffill bull", "i" * 16, "rnrn club", "l l l l l", "curl brr", "fin ruf"]
    h = W.alphabet_height(SANS, 13.0, al)
    pages = np.full((2, 5 * h, 70), 255, dtype=np.uint8)
    for k, (text, (p, slot)) in enumerate(zip(texts, [(0, 0), (0, 1), (0, 3), (0, 4), (1, 0), (1, 2), (1, 3)])):
        put(pages[p], W.draw_line(SANS, 13.0, al, text, width=70, height=h), slot * h)
    dec.set_font(fm.font, 13.0)
    assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 2) == 0
    try:
        want = check(dec, fm, pages, (0, 0, 70, h, h))
    finally:
        assert dec._lib.focr_decoder_debug_set_whole_grid(dec._h, 0) == 0
    assert sum(len(pg) for pg in want) == 7 and len({s.text for pg in want for _, s in pg}) == 7
    check(dec, fm, pages, (0, 0, 70, h, h))  # and on the decoder's own grid


def test_bottom_clip_and_x_start(dec):
    """x_start 3 and a last slot cut by the page's bottom edge to 8 of its 13 rows: the crop's own h clips every glyph."""
    al = "burn clif"
    fm = model(SANS, 13.0, al)
    h = W.alphabet_height(SANS, 13.0, al)
    page = np.full((h + 8, 64), 255, dtype=np.uint8)
    put(page, W.draw_line(SANS, 13.0, al, "burn club", width=60, height=h), 0, 3)
    put(page, W.draw_line(SANS, 13.0, al, "fill in", width=60, height=h), h, 3)
    dec.set_font(fm.font, 13.0)
    want = check(dec, fm, [page], (3, 0, 60, h, h))[0]
    assert [y for y, _ in want] == [0, h] and want[0][1].text[:9] == "burn club" and len(want[1][1].text) > 3


@pytest.mark.parametrize("width", [800, 900])
def test_strip_in_lds_and_in_global_memory(dec, width):
    """Mono 13 px, four glyphs, 64-row slots: at width 800 strip, ring and live list fit the LDS budget; at 900 they do
    not, and the strip is read from global memory."""
    al, lh = "AB >", 64
    fm = model(MONO, 13.0, al)
    lds = strip_bytes(width, lh) + WHOLE_MISC_BYTES + 8 * ring_length(fm)
    assert (lds <= LDS_STRIP_MAX) == (width == 800) and 8 * ring_length(fm) + WHOLE_MISC_BYTES < LDS_STRIP_MAX
    rng = np.random.default_rng(width)
    page = np.full((lh, 900), 255, dtype=np.uint8)
    put(page, W.draw_line(MONO, 13.0, al, "".join(rng.choice(list(al), 114)), width=900, height=16), 20)
    page[:, 790:] = np.minimum(page[:, 790:], 200)  # ink in the columns the widths differ by
    dec.set_font(fm.font, 13.0)
    (_, s), = check(dec, fm, [page], (0, 0, width, lh, lh))[0]
    assert len(s.text) >= width // 8


def test_verify_draws_every_character_at_its_pen(dec):
    """After a whole-line run on the Sans line the verify image and sums are draw_verify with every character at
    pos = s / 64 of its returned pen, and the page's error is below the plain run's, whose text is another.  draw_verify
    puts render() of the text at the crop's corner, which is where the decoder read the ink only when the text's own
    bounds start where the alphabet's do (with the default alphabet Sans has origin_x = 1 and this text's bounds start at
    0, so every verify of it, right or wrong, is a pixel off the page's ink): the alphabet here is the line's own letters
    and the wide glyphs the greedy loop confuses them with, none of which reaches left of the pen."""
    al = "burn clipfHvmd"
    fm = model(SANS, 13.0, al)
    assert float(fm.ox) == 0 and fm.decode_line(W.draw_line(SANS, 13.0, al, TEXT)) != TEXT
    line = W.draw_line(SANS, 13.0, al, TEXT)
    h, w = line.shape
    page = np.full((h + 9, w + 12), 255, dtype=np.uint8)
    put(page, line, 4, 5)
    geo = (5, 4, w, h, h)
    dec.set_font(fm.font, 13.0)
    want = want_pages(fm, [page], *geo)[0]
    lines, mse, images, pens, costs = dec.decode([page], *geo, verify="image", whole_line=True)
    assert lines[0] == [(y, s.text) for y, s in want] and all(np.array_equal(p, s.pens) for p, (_, s) in zip(pens[0], want))
    assert want[0][1].text[:-1] == TEXT
    vf = VerifyFont(SANS, 13.0, al)
    img, sq = W.verify_image(page, [(y, s.text, s.pens) for y, s in want], fm.font, vf, geo[0])
    assert np.array_equal(images[0], img)
    sums, _ = dec.verify(images=False)
    assert int(sums[0]) == sq and mse[0].tobytes() == (np.float32(sq) / np.float32(page.size)).tobytes()
    assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
    plain, plain_mse, _ = dec.decode([page], *geo, verify="mse")
    assert plain != lines and mse[0] < plain_mse[0]
    vf.close()


def _raw_run(dec, page, x, y, width, line_height, line_advance):
    """focr_decoder_run of one page with whatever state the library is in: (return code, its message)."""
    page = np.ascontiguousarray(page)
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], x, y, width, line_height,
                                   line_advance)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def test_refusals(dec):
    """Every refusal of include/focr_decode.h, at focr_decoder_run and with its message; the decoder decodes afterwards."""
    al = FOCR_DEFAULT_ALPHABET
    fm = model(MONO, 13.0, al)
    line = W.draw_line(MONO, 13.0, al, "refuse")
    geo = (0, 0, line.shape[1], line.shape[0], line.shape[0])
    lib, h = dec._lib, dec._h

    def hand_built(size=13.0, alphabet="AB", **change):
        df = DecodeFont(MONO, size, alphabet)
        if "origin_x" in change:
            df.s.origin_x = change["origin_x"]
        if "increment" in change:
            df.s.glyphs[0].increment = change["increment"]
        dec.set_font(df, size)
        return df

    # scores on, and a pen search radius: states of the library that the Python API never combines with the mode
    dec.set_font(fm.font, 13.0)
    dec.decode([line], *geo, whole_line=True)
    for setter, value, word in ((lib.focr_decoder_set_scores, 1, "scores on"), (lib.focr_decoder_set_pen_search, 8, "pen search radius")):
        assert setter(h, value) == 0
        rc, msg = _raw_run(dec, line, *geo)
        assert setter(h, 0) == 0
        assert rc != 0 and "focr_decoder_run: whole-line decode" in msg and word in msg, msg
        assert lib.focr_decoder_get_pens(h, None, None) != 0  # the failed run left no result
    with pytest.raises(ValueError):
        dec.decode([line], *geo, whole_line=True, scores=True)
    with pytest.raises(ValueError):
        dec.decode([line], *geo, whole_line=True, pen_search=8)
    # a fractional and a negative origin
    for ox in (0.5, -1.0):
        df = hand_built(origin_x=ox)
        with pytest.raises(DecoderError, match="origin_x to be a whole number >= 0"):
            dec.decode([line], *geo, whole_line=True)
        df.close()
    # an increment that rounds to no sixty-fourth
    df = hand_built(increment=0.005)
    with pytest.raises(DecoderError, match="inc64 below 1"):
        dec.decode([line], *geo, whole_line=True)
    df.close()
    # an advance of 70 px: min(min inc64, 512) + 4480 keys need a ring of 8192
    df = hand_built(increment=70.0)
    with pytest.raises(DecoderError, match="widest advance is too large .*cost ring does not fit in LDS"):
        dec.decode([line], *geo, whole_line=True)
    df.close()
    # pens past 2^24 sixty-fourths on a one-row page
    wide = np.full((1, 262144), 255, dtype=np.uint8)
    wide[0, 5] = 0
    dec.set_font(fm.font, 13.0)
    with pytest.raises(DecoderError, match=r"below 2\^24 .pens must stay exact in f32"):
        dec.decode([wide[:, : 262144 - 7]], 0, 0, 262144, 1, 1, whole_line=True)  # 64 * w + 501 >= 2^24
    # the cost bound: one glyph advancing by 1/64 px makes 64 * w characters possible; Mono 60 px bounds a term by T
    df = hand_built(size=60.0, increment=1.0 / 64)
    T = max(df.s.glyphs[i].stride * df.s.glyphs[i].box_h * 2 * 255 * 255 for i in range(2))
    w = -(-(1 << 47) // (64 * T))  # the first width with 64 * w * T >= 2^47
    assert 64 * w * T >= 1 << 47 > 64 * (w - 1) * T and 64 * w + int(W.inc64(np.array([df.s.glyphs[1].increment])).max()) < 1 << 24
    with pytest.raises(DecoderError, match=r"reaches 2\^47 .a packed cost could overflow"):
        dec.decode([wide[:, :w]], 0, 0, w, 1, 1, whole_line=True)
    df.close()
    dec.set_font(fm.font, 13.0)
    check(dec, fm, [line], geo)


def test_off_path_is_the_plain_decoder(dec):
    """With the mode off after it was on, a run returns what a decoder that never heard of it returns, scores and verify
    included, in 3 launches; focr_decoder_get_pens fails after a plain run and works after a whole-line one."""
    al = FOCR_DEFAULT_ALPHABET
    a = W.draw_line(SANS, 13.0, al, TEXT)
    h, w = a.shape
    pages = np.full((2, 3 * h, w), 255, dtype=np.uint8)
    put(pages[0], a, 0), put(pages[1], W.draw_line(SANS, 13.0, al, "Plain 0 decode", width=w), 2 * h)
    geo = (0, 0, w, h, h)
    with LineDecoder(0) as fresh:
        fresh.set_font(SANS, 13.0)
        lines, mse, images, scores = fresh.decode(pages, *geo, verify="image", scores=True)
        assert fresh._lib.focr_decoder_get_pens(fresh._h, None, None) != 0
        assert b"focr_decoder_get_pens" in fresh._lib.focr_decoder_last_error(fresh._h)
    dec.set_font(SANS, 13.0)
    whole, pens, _ = dec.decode(pages, *geo, whole_line=True)
    assert whole != lines and dec._lib.focr_decoder_get_pens(dec._h, None, None) == 0
    got = dec.decode(pages, *geo, verify="image", scores=True)
    assert len(got) == 4 and got[0] == lines and got[1].tobytes() == mse.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(got[2], images))
    for a_pg, b_pg in zip(got[3], scores):
        assert len(a_pg) == len(b_pg)
        for x, y in zip(a_pg, b_pg):
            assert x.base == y.base and all(np.array_equal(x[f], y[f]) for f in (1, 2, 3))
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    assert dec._lib.focr_decoder_get_pens(dec._h, None, None) != 0
    lines8, offs = dec.decode(pages, *geo, pen_search=8)
    with LineDecoder(0) as fresh:
        fresh.set_font(SANS, 13.0)
        assert fresh.decode(pages, *geo, pen_search=8)[0] == lines8


def test_cli(dec, tmp_path):
    """focr --whole-line --verify on a PGM: stdout is the Python API's text and the MSE on stderr its verify's."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    al = FOCR_DEFAULT_ALPHABET
    line = W.draw_line(SANS, 13.0, al, TEXT)
    h, w = line.shape
    page = np.full((2 * h, w), 255, dtype=np.uint8)
    put(page, line, h)
    path, vdir = str(tmp_path / "page.pgm"), tmp_path / "v"
    save_pgm(path, page)
    vdir.mkdir()
    cmd = [FOCR, "-f", SANS, "-t", "13", "-w", str(w), "--line-height", str(h), "--line-advance", str(h), "-i", path]
    r = subprocess.run(cmd + ["--whole-line", "--verify", str(vdir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    dec.set_font(SANS, 13.0)
    lines, mse, _, _, _ = dec.decode([page], 0, 0, w, h, h, verify="mse", whole_line=True)
    assert r.stdout == "".join(t + "\n" for _, t in lines[0]) and r.stdout[: len(TEXT)] == TEXT
    assert r.stderr.splitlines() == ["%s %.6f" % (path, mse[0])] and os.listdir(vdir) == ["page.png"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "bunY dm+Tl vvillmmY d>\n"


def test_memory_returns():
    """A decoder that ran whole lines, with a verify, gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    line = W.draw_line(MONO, 13.0, "AB >", "AB > BA")
    geo = (0, 0, line.shape[1], line.shape[0], line.shape[0])
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0, "AB >")
        d.decode([line], *geo)
        off = N.hip().focr_debug_device_bytes()
        d.decode([line], *geo, whole_line=True, verify="mse")
        assert before < off < N.hip().focr_debug_device_bytes()
    assert N.hip().focr_debug_device_bytes() == before

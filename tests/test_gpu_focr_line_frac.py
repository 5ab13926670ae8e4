"""The focr decoder's fractional line grid (focr_decoder_set_line_frac; line_prepass_frac_kernel,
line_whole_baseline_frac_kernel, verify_compose_moved_frac_kernel, and the two kernels that take the grid as an argument and
serve the whole-pixel grid at (0, 0) as well: line_baseline_kernel, verify_layout_kernel;
LineDecoder.decode(y_frac=, line_advance_frac=); focr --y-frac --line-advance-frac) against tests/focr_line_frac_model.py,
the definition of include/focr_decode.h restated in plain integers on the two baseline models.  Every quantity is an exact
integer, so every comparison is ==.  The cases are tests/focr_line_frac_cases.py's; tests/test_focr_line_frac_model.py proves
on the CPU that each reaches the case its name promises.  The edge cases run at (0, 0) too (the *_at_zero_fraction tests),
against the two whole-pixel models: there the grid-taking kernels must give what the whole-pixel kernels they replaced gave.

Teeth of test_fuzz_cases, as measured on an MI355X with one-line mutations of the DEVICE code only (decode.h; neither touches
an index, a bound, a size or a stride), each built once and run once against test_fuzz_cases: frac_centre with `+ 31` for
`+ 32` fails base-2, base-5 and whole-3, the cases with an inked slot whose centre only the half rounds up, and slot_rows_frac
with slot 0's f for every slot fails eight cases of both forms; in each the first assertion to fail is the texts' ==."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import focr_line_frac_cases as K
import focr_line_frac_model as LF
from font_ocr_amd import LineDecoder, VerifyFont, save_pgm
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def _decode(dec, c, pages=None, verify=None):
    kw = dict(y_frac=c.frac[0], line_advance_frac=c.frac[1], verify=verify)
    if c.whole:
        return dec.decode(c.pages if pages is None else pages, *c.geo, whole_line=True, whole_baseline=c.n, **kw)
    return dec.decode(c.pages if pages is None else pages, *c.geo, baseline_search=c.n, **kw)


def _check(dec, c, verify=True):
    """Decode a case on its grid: line order, y, text, q, cost (and pens) equal to the model's, and with verify the image,
    the MSE, and from a verify without images of each page size the exact sums.  Returns the model's [[(yc_i, result)] per
    page]."""
    fuzz = isinstance(c, K.Fuzz)  # a seeded case brings its hinting and kerning
    m = K.fuzz_model(c) if fuzz else K.model(c.font, c.size, c.alphabet, c.y_bits)
    dec.set_font(m.font, c.size)
    want = K.fuzz_expected(c) if fuzz else K.expected(c)
    got = _decode(dec, c, verify="image" if verify else None)
    lines, rest = got[0], got[3:] if verify else got[1:]
    assert lines == [[(y, r.text) for y, r in pg] for pg in want]
    if c.whole:
        pens, costs, qs = rest
        assert [[list(p) for p in pg] for pg in pens] == [[[int(s) for s in r.pens] for _, r in pg] for pg in want]
    else:
        qs, costs = rest
    assert qs == [[r.q for _, r in pg] for pg in want]
    assert costs == [[r.cost for _, r in pg] for pg in want]
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    if verify:
        vf = VerifyFont(c.font, c.size, c.alphabet, c.hinting, c.kerning) if fuzz else VerifyFont(c.font, c.size, c.alphabet)
        sqs = []
        for page, found, mse, img in zip(c.pages, want, got[1], got[2]):
            wimg, sq = LF.verify_image(page, found, m.font, vf, c.geo[0], c.y_bits, whole=c.whole)
            sqs.append(sq)
            assert np.array_equal(img, wimg)
            assert mse.tobytes() == (np.float32(sq) / np.float32(page.size)).tobytes()
        assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
        # the exact integer sums (the MSE above is their f32 rounding), by the verify that draws no image: decode() keeps
        # only the last size group's run, so every group is decoded on its own
        for shape in {p.shape for p in c.pages}:
            idx = [i for i, p in enumerate(c.pages) if p.shape == shape]
            _decode(dec, c, pages=[c.pages[i] for i in idx])
            sums, none = dec.verify(images=False)
            assert none is None and len(sums) == len(idx)
            assert [int(s) for s in sums] == [sqs[i] for i in idx]
            assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2
        vf.close()
    return want


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("y_bits", [0, 2, 3])
@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_standard_grid(dec, whole, y_bits, n):
    """Both modes at B = 0, 2, 3 and N = 1, 4 on the standard grid: a centre of 2^B in slot 0, crop rows off the whole-pixel
    grid, a blank slot between inked ones, and (the baseline search's pages) a last slot cut by the page."""
    want = _check(dec, K.std_case(whole, y_bits, n))
    assert want[0][0][0] == 3 and want[0][1][0] in (19, 35) and want[0][0][1].q >= (1 << y_bits) - n


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_dropped_candidates(dec, whole):
    want = _check(dec, K.dropped_case(whole))[0]
    assert [r.q for _, r in want] == [0, -2, 0]


def test_line_advance_one(dec):
    """line_advance 1 with a fraction under a line_height of 12: about a dozen slots share every tile row of the moved compose."""
    want = _check(dec, K.advance_one_case())[0]
    assert len(want) > 20


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_canvas_moved_off_the_page(dec, whole):
    """The first canvas moved above row 0, the last one past the page's last row: the verify clips both."""
    want = _check(dec, K.moved_off_page_case(whole))[0]
    assert want[0][1].q == -3 and want[-1][1].q == 3


def test_canvas_at_the_far_lower_reach(dec):
    """q = 2^B + 32 = 33 at B = 0: the canvas lies 33 rows below its slot, and over the sweep of y its last row is once the
    first row of a compose tile, which only the full lower reach of slot_range_frac finds."""
    for y in range(16):
        (_, b), = _check(dec, K.far_below_case(y))[0]
        assert b.q == 33


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_strip_too_large_for_lds(dec, whole):
    c = K.wide_case(whole)
    assert K.strip_bytes(c.pages[0].shape[1], c.geo[0], c.geo[2], c.geo[3]) > 65536
    _check(dec, c)


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_two_page_sizes_through_decode(dec, whole):
    c = K.two_sizes_case(whole)
    want = _check(dec, c)
    slots = [len(LF.slots(p.shape[0], c.geo[1], c.frac[0], c.geo[3], c.geo[4], c.frac[1])) for p in c.pages]
    assert len({p.shape for p in c.pages}) == 2 and len(set(slots)) == 2  # two grids in one call
    assert [y for y, _ in want[0]] == [y for y, _ in want[2]] and all(len(pg) >= 2 for pg in want)


def _same_under_debug_grids(dec, c, whole):
    free = _decode(dec, c)
    setter = dec._lib.focr_decoder_debug_set_whole_grid if whole else dec._lib.focr_decoder_debug_set_baseline_grid
    try:
        for grid in (1, 2):
            assert setter(dec._h, grid) == 0
            assert repr(_decode(dec, c)) == repr(free)
    finally:
        assert setter(dec._h, 0) == 0


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_one_workgroup_takes_several_lines(dec, whole):
    """With the debug grid at 1 and 2 one workgroup takes every line, or every other one: the centre is worked out again for
    each, so the result is the free run's, which is the model's."""
    c = K.std_case(whole, 2, 1)
    c = c._replace(pages=K.std_pages(whole, 31, 2))
    want = _check(dec, c, verify=False)
    assert len({r.q for pg in want for _, r in pg}) >= (2 if whole else 4)  # several centres
    _same_under_debug_grids(dec, c, whole)


# ---- the same edges at the fraction (0, 0): the baseline search's kernel and the verify's layout kernel are the same ones on
# both grids, and at (0, 0) the fractional grid is the whole-pixel one, so K.off(case) is held to the two whole-pixel models
# (focr_baseline_model, focr_whole_baseline_model; K.expected).  The pages are the cases' own: their lines were drawn for the
# fractional grid and sit off these slots, so the searches move them (tests/test_focr_line_frac_model.py proves each q) ----


def _moved(want):
    return any(r.q != 0 for pg in want for _, r in pg)


def test_line_advance_one_at_zero_fraction(dec):
    want = _check(dec, K.off(K.advance_one_case()))[0]
    assert len(want) > 20 and _moved([want])


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_canvas_moved_off_the_page_at_zero_fraction(dec, whole):
    """The last line, drawn for a leading of 15 + 38/64 px, lies four rows below its whole-pixel slot."""
    want = _check(dec, K.off(K.moved_off_page_case(whole)))[0]
    assert want[0][1].q == -3 and want[-1][1].q == 4


def test_canvas_at_the_far_lower_reach_at_zero_fraction(dec):
    """The centre is 0, so the largest q is 32 = FOCR_BASELINE_MAX: the same sweep with the canvas 32 rows below its slot."""
    for y in range(16):
        (_, b), = _check(dec, K.off(K.far_below_case(y)))[0]
        assert b.q == 32


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_strip_too_large_for_lds_at_zero_fraction(dec, whole):
    c = K.off(K.wide_case(whole))
    assert K.strip_bytes(c.pages[0].shape[1], c.geo[0], c.geo[2], c.geo[3]) > 65536
    assert _moved(_check(dec, c))


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_one_workgroup_takes_several_lines_at_zero_fraction(dec, whole):
    """Every centre is 0, and the lines drift off their slots until the radius of one step saturates either way."""
    c = K.std_case(whole, 2, 1)
    c = K.off(c._replace(pages=K.std_pages(whole, 31, 2)))
    want = _check(dec, c, verify=False)
    assert _moved(want) and {r.q for pg in want for _, r in pg} <= {-1, 0, 1}
    _same_under_debug_grids(dec, c, whole)


@pytest.mark.parametrize("whole", [False, True], ids=["base", "whole"])
def test_off_after_on_is_a_fresh_decoder(dec, whole):
    """(0, 0) after a fractional run returns exactly what a decoder that never had a grid returns: lines, q, costs, verify
    images and MSE, in three launches; and the device's q on the whole-pixel grid differs from the fractional one's.  The
    baseline search and the verify's layout launch the same kernel in both runs: (0, 0) after (60, 38) differs in its
    arguments alone."""
    c = K.std_case(whole, 2, 1)
    m = K.model(c.font, c.size, c.alphabet, c.y_bits)
    off = c._replace(frac=(0, 0))
    with LineDecoder(0) as fresh:
        fresh.set_font(m.font, c.size)
        want = _decode(fresh, off, verify="image")
        assert fresh._lib.focr_decoder_last_launches(fresh._h) == 3
    dec.set_font(m.font, c.size)
    on = _decode(dec, c, verify="image")
    got = _decode(dec, off, verify="image")
    assert dec._lib.focr_decoder_last_launches(dec._h) == 3
    assert repr(got[0]) == repr(want[0]) and repr(got[3:]) == repr(want[3:]) and got[1].tobytes() == want[1].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))
    assert repr(on[0]) != repr(got[0])


@pytest.mark.parametrize("whole,i", [(w, i) for w in (False, True) for i in K.FUZZ_IDS], ids=[f"{w}-{i}" for w in ("base", "whole") for i in K.FUZZ_IDS])
def test_fuzz_cases(dec, whole, i):
    """The first dozen seeded cases of tests/focr_fuzz_cases.py at B = 2, N = 4 and the dozen of
    tests/focr_whole_baseline_fuzz.py at their own B and N (Sans, Serif and Mono, hinting on and off, kernings off 1, clipped
    widths, cut last slots, pages of two sizes), each on its seeded fraction of focr_line_frac_cases.fuzz_frac, and the
    low-origin case that drops candidates: crop rows, texts, the absolute q, costs and pens equal to the model's, and for
    every third case the verify image, the per-page sums and the MSE as well.  tests/test_focr_line_frac_model.py proves
    what the fractions reach."""
    c = K.fuzz_case(whole, i)
    assert c.frac != (0, 0) and all(0 <= f <= 63 for f in c.frac)
    want = _check(dec, c, verify=i == "low" or i % 3 == 0)
    assert sum(len(pg) for pg in want) > 0


def _raw_run(dec, page, x, y, width, line_height, line_advance):
    page = np.ascontiguousarray(page)
    rc = dec._lib.focr_decoder_run(dec._h, C.c_void_p(page.ctypes.data), 0, 1, page.shape[1], page.shape[0], x, y, width, line_height, line_advance)
    return rc, dec._lib.focr_decoder_last_error(dec._h).decode()


def test_refusals(dec):
    """The setter's bounds, and every refusal of focr_decoder_run, before anything is launched and with a message that names
    the setters; what the mode in force refuses is still refused; the decoder decodes afterwards."""
    c = K.std_case(False, 2, 1)
    m = K.model(c.font, c.size, c.alphabet, 2)
    page, geo = c.pages[0], c.geo
    lib, h = dec._lib, dec._h
    want = _check(dec, c, verify=False)
    for bad in ((64, 0), (0, 64), (1 << 31, 0)):
        assert lib.focr_decoder_set_line_frac(h, *bad) != 0 and b"focr_decoder_set_line_frac" in lib.focr_decoder_last_error(h)
        assert b"at most 63" in lib.focr_decoder_last_error(h)
    assert lib.focr_decoder_set_line_frac(h, 63, 63) == 0  # the bounds themselves are taken

    def refused(*words):
        rc, msg = _raw_run(dec, page, *geo)
        assert rc != 0 and all(w in msg for w in words), msg
        assert lib.focr_decoder_last_launches(h) == 0 and lib.focr_decoder_n_lines(h) == 0

    grid_words = ("focr_decoder_set_line_frac", "focr_decoder_set_baseline_search", "focr_decoder_set_whole_baseline", "radius >= 1")
    # the grid with neither search: the plain loop, scores, a pen search, the whole-line decode, margins, a pen slack
    assert lib.focr_decoder_set_baseline_search(h, 2, 0) == 0
    refused(*grid_words)
    for on, off in ((lambda: lib.focr_decoder_set_scores(h, 1), lambda: lib.focr_decoder_set_scores(h, 0)),
                    (lambda: lib.focr_decoder_set_pen_search(h, 4), lambda: lib.focr_decoder_set_pen_search(h, 0)),
                    (lambda: lib.focr_decoder_set_whole_line(h, 1), lambda: lib.focr_decoder_set_whole_line(h, 0))):
        assert on() == 0
        refused(*grid_words)
        assert off() == 0
    assert lib.focr_decoder_set_whole_line(h, 1) == 0
    for on, off in ((lambda: lib.focr_decoder_set_whole_margins(h, 1), lambda: lib.focr_decoder_set_whole_margins(h, 0)),
                    (lambda: lib.focr_decoder_set_whole_slack(h, 4), lambda: lib.focr_decoder_set_whole_slack(h, 0))):
        assert on() == 0
        refused(*grid_words)
        assert off() == 0
    assert lib.focr_decoder_set_whole_line(h, 0) == 0
    # what the mode in force refuses anyway is still refused, with its own message
    assert lib.focr_decoder_set_baseline_search(h, 2, 1) == 0 and lib.focr_decoder_set_scores(h, 1) == 0
    refused("focr_decoder_set_baseline_search", "focr_decoder_set_scores")
    assert lib.focr_decoder_set_scores(h, 0) == 0 and lib.focr_decoder_set_baseline_search(h, 2, 0) == 0
    assert lib.focr_decoder_set_whole_baseline(h, 2, 1) == 0
    refused("focr_decoder_set_whole_baseline", "focr_decoder_set_whole_line")
    assert lib.focr_decoder_set_whole_baseline(h, 0, 0) == 0 and lib.focr_decoder_set_baseline_search(h, 2, 1) == 0
    # line_advance 0 stays refused, whatever advance_frac
    rc, msg = _raw_run(dec, page, geo[0], geo[1], geo[2], geo[3], 0)
    assert rc != 0 and "line_advance 0" in msg
    # an empty first crop is no refusal: no slots, no lines
    assert _raw_run(dec, page, geo[0], page.shape[0], geo[2], geo[3], 15)[0] == 0 and lib.focr_decoder_n_lines(h) == 0
    assert lib.focr_decoder_set_line_frac(h, *c.frac) == 0
    dec._baseline, dec._line_frac = (2, 1), tuple(c.frac)
    with pytest.raises(ValueError, match="y_frac and line_advance_frac need baseline_search or whole_baseline"):
        dec.decode(c.pages, *geo, y_frac=1)
    assert _decode(dec, c)[0] == [[(y, r.text) for y, r in pg] for pg in want]
    assert m.y_bits == 2


def test_cli(dec, tmp_path):
    """focr --baseline-search 1 --y-bits 2 --y-frac 60 --line-advance-frac 38 --baselines --verify on two PGMs of different
    sizes: stdout is the model's text, and the CSV and the verify PNGs are the model's files byte for byte."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    c = K.two_sizes_case(False)
    c = c._replace(pages=c.pages[:2])
    m = K.model(c.font, c.size, c.alphabet, 2)
    want = K.expected(c)
    paths = []
    for i, pg in enumerate(c.pages):
        paths.append(str(tmp_path / f"page{i}.pgm"))
        save_pgm(paths[-1], pg)
    out, vdir, wdir = tmp_path / "baselines.csv", tmp_path / "v", tmp_path / "w"
    vdir.mkdir()
    wdir.mkdir()
    x, y, width, lh, la = c.geo
    cmd = [FOCR, "-f", c.font, "-t", str(c.size), "-a", c.alphabet, "-x", str(x), "-y", str(y), "-w", str(width), "--line-height", str(lh),
           "--line-advance", str(la), "--baseline-search", "1", "--y-bits", "2", "--y-frac", str(c.frac[0]), "--line-advance-frac", str(c.frac[1])]
    r = subprocess.run(cmd + ["--baselines", str(out), "--verify", str(vdir), "-i"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join(b.text + "\n" for pg in want for _, b in pg) and len(r.stdout) > 100
    rows = ["image_index,y,q,offset_px,cost"] + ["%d,%d,%d,%g,%d" % (i, yc, b.q, b.q / 4, b.cost) for i, pg in enumerate(want) for yc, b in pg]
    assert open(out).read() == "".join(row + "\n" for row in rows)
    vf = VerifyFont(c.font, c.size, c.alphabet)
    mses = []
    for i, (page, found) in enumerate(zip(c.pages, want)):
        img, sq = LF.verify_image(page, found, m.font, vf, x, 2)
        img = np.ascontiguousarray(img)
        assert N.host().focr_image_save_png(str(wdir / f"page{i}.png").encode(), img.ctypes.data, page.shape[1], page.shape[0], 3) == 0
        assert open(vdir / f"page{i}.png", "rb").read() == open(wdir / f"page{i}.png", "rb").read()
        mses.append("%s %.6f" % (paths[i], np.float32(sq) / np.float32(page.size)))
    assert sorted(r.stderr.splitlines()) == sorted(mses)
    vf.close()


def test_memory_returns():
    """A decoder that ran both modes on the fractional grid, with a verify, gives every byte of device memory back."""
    before = N.hip().focr_debug_device_bytes()
    for whole in (False, True):
        c = K.std_case(whole, 2, 1)
        with LineDecoder(0) as d:
            d.set_font(c.font, c.size, c.alphabet, y_bits=2)
            _decode(d, c, verify="mse")
            assert N.hip().focr_debug_device_bytes() > before
        assert N.hip().focr_debug_device_bytes() == before

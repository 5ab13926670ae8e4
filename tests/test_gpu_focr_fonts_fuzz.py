"""The focr decoder's font search in both forms (line_fonts_kernel, line_whole_fonts_kernel and the host plans behind them)
against tests/focr_fonts_model.py on the seeded cases of tests/focr_fonts_fuzz.py: decode fonts and candidates of mixed
faces, sizes, hinting and kerning, K of 1 .. 15, run geometries of every kind (clipped widths, cut last slots, overlapping
slots, two page sizes), and one decoder handle for the whole module, so that every run meets the buffers another form,
another K and another geometry left; between the searched runs the same handle, candidates still uploaded, runs the plain
pen loop and the plain whole-line decode.  tests/test_focr_fonts_fuzz_host.py proves on the CPU that no case is refused and
what the cases reach.  Every quantity is an exact integer and is compared with ==; every message names its case, form,
page and y.

Teeth, as measured on an MI355X with one-line mutations of the DEVICE code only, each of which changes a comparison or which
value is selected (none an index, a bound, a size or a stride), each built once and run once against this module; the first
assertion to fail is named:
  line_fonts_kernel's merge, `r < best_font` -> `r > best_font`: the fonts ==, first on a random case whose candidate 2 costs
    what the decode font costs (2 for 0); three of the five groups fail, the FIXED ties among them;
  line_fonts_kernel's per-wave `cost < best_cost` -> `<=`: the fonts == on tie-in-one-wave alone (5 for 1);
  font_loop with candidate 0's origin_x for every k: the costs ==, in all five groups;
  line_whole_fonts_kernel's `cost < best_cost` -> `<=`: the fonts == (2 for 0), in three groups;
  line_whole_fonts_kernel's WholeParams with desc[0].origin_d for every candidate: the costs ==, in all five groups.
"""
import numpy as np
import pytest

import focr_fonts_fuzz as FZ
import focr_whole_model as W
from focr_fonts_fuzz import get_fonts, searched
from font_ocr_amd import LineDecoder
from font_ocr_amd import _native as N

pytestmark = pytest.mark.gpu

GROUP = 6
GROUPS = [list(range(a, min(a + GROUP, FZ.N_CASES))) for a in range(0, FZ.N_CASES, GROUP)]
_module = {}


@pytest.fixture(scope="module")
def dec():
    _module["bytes"] = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as d:
        yield d


def same(got, c, form):
    """A searched device result against the model's answer of (case, form)."""
    want = FZ.want(c, form)
    for name, pages in got.items():
        assert len(pages) == len(want), (c.name, form, name)
    for p, want_pg in enumerate(want):
        at = (c.name, form, p)
        assert [y for y, _ in got["lines"][p]] == [y for y, _ in want_pg], at
        for name in got:
            assert len(got[name][p]) == len(want_pg), at + (name,)
        for n, (y, r) in enumerate(want_pg):
            at = (c.name, form, p, y)
            assert got["fonts"][p][n] == r.k, at + ("font", got["fonts"][p][n], r.k, r.trail)
            assert got["costs"][p][n] == r.cost, at + ("cost", got["costs"][p][n], r.cost)
            assert got["lines"][p][n][1] == r.text, at + ("text",)
            if form == "whole":
                pens = got["pens"][p][n]
                assert pens.dtype == np.uint32 and np.array_equal(pens, r.pens), at + ("pens",)


_off = {}


def want_off(c, form):
    """The decode font's own answer, the search off: FastModel.decode_image, or focr_whole_model.whole_image."""
    key = (c.index, form)
    if key not in _off:
        fm = FZ.models(c)[0]
        _off[key] = [W.whole_image(fm, p, *c.geo) if form == "whole" else fm.decode_image(p, *c.geo) for p in c.pages]
    return _off[key]


def same_off(d, c):
    """The candidates still uploaded and the search off: the plain pen loop and the plain whole-line decode of the decode font."""
    lines = d.decode(c.pages, *c.geo)
    for p, want_pg in enumerate(want_off(c, "pen")):
        assert lines[p] == want_pg, (c.name, "plain", p, [y for y, _ in want_pg])
    lines, pens, costs = d.decode(c.pages, *c.geo, whole_line=True)
    for p, want_pg in enumerate(want_off(c, "whole")):
        assert [y for y, _ in lines[p]] == [y for y, _ in want_pg], (c.name, "whole", p)
        for n, (y, r) in enumerate(want_pg):
            at = (c.name, "whole", p, y)
            assert lines[p][n][1] == r.text and costs[p][n] == r.cost and np.array_equal(pens[p][n], r.pens), at
    assert get_fonts(d)[0] != 0, (c.name, "focr_decoder_get_fonts after a run without the search")


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=["cases%d-%d" % (g[0], g[-1]) for g in GROUPS])
def test_both_forms_equal_the_model(dec, group):
    """The group's (case, form) pairs in a seeded shuffled order on the module's one handle; behind every searched run the
    same handle decodes the case with the search off."""
    cases = [FZ.case(i) for i in GROUPS[group]]
    pairs = [(c, form) for c in cases for form in FZ.FORMS]
    order = np.random.default_rng([FZ.SEED, 1 << 20, group]).permutation(len(pairs))
    for c, form in (pairs[k] for k in order):
        same(searched(dec, c, form), c, form)
        same_off(dec, c)


def test_the_used_handle_is_as_good_as_new(dec):
    """Last in the module: a searched run of case 0 in both forms on the handle equals a fresh decoder's, and closing the
    handle gives every byte of device memory back."""
    c = FZ.case(0)
    with LineDecoder(0) as fresh:
        for form in FZ.FORMS:
            got, want = searched(dec, c, form), searched(fresh, c, form)
            assert repr(got) == repr(want), (c.name, form)
            same(got, c, form)
    dec.close()
    assert N.hip().focr_debug_device_bytes() == _module["bytes"], "device bytes after the module"

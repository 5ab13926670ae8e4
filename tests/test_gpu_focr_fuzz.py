"""Every mode of the focr line decoder (line_decode_kernel, line_search_kernel, line_whole_kernel,
line_whole_margins_kernel, line_whole_slack_kernel and the verify compose behind them) against its model on the seeded
cases of tests/focr_fuzz_cases.py: fonts, sizes, kernings and hinting off the default setup, run geometries of every
kind, and one decoder handle for the whole module, so that every run meets the buffers another mode, another font and
another geometry left.  tests/test_focr_fuzz_cases_host.py proves on the CPU that no case is refused and what the cases
reach.  Every quantity is an exact integer and is compared with ==; every message names its case and mode.
FOCR_FUZZ_SEED replaces the seed (the host test proves the committed one only)."""
import numpy as np
import pytest

import focr_fuzz_cases as FC
import focr_line_model as M
import focr_margins_model as MM
import focr_search_model as S
import focr_slack_model as K
import focr_whole_model as W
from focr_fuzz_cases import last_batch, run
from font_ocr_amd import LineDecoder, LineMargins, LineScores, VerifyFont
from font_ocr_amd import _native as N

pytestmark = pytest.mark.gpu

GROUP = 6
GROUPS = [list(range(a, min(a + GROUP, FC.N_CASES))) for a in range(0, FC.N_CASES, GROUP)]
_module = {}


@pytest.fixture(scope="module")
def dec():
    _module["bytes"] = N.hip().focr_debug_device_bytes()
    with LineDecoder(0) as d:
        yield d


_vfonts = {}


def verify_font(c):
    if c.index not in _vfonts:
        _vfonts[c.index] = VerifyFont(c.font, c.size, c.alphabet, c.hinting, c.kerning)
    return _vfonts[c.index]


def same(got, c, mode):
    """A device result against the models' answer of (case, mode)."""
    fm, want = FC.model(c), FC.want(c, mode)
    who = (c.name, mode)
    text = (lambda r: r) if mode == "plain" else (lambda r: r.text)
    assert got["lines"] == [[(y, text(r)) for y, r in pg] for pg in want], who
    for name in ("scores", "offsets", "pens", "costs", "margins"):
        assert name not in got or [len(pg) for pg in got[name]] == [len(pg) for pg in want], who + (name,)
    for p, want_pg in enumerate(want):
        for k, (y, r) in enumerate(want_pg):
            at = who + (p, y)
            if "scores" in got:
                sc = got["scores"][p][k]
                assert isinstance(sc, LineScores) and sc.base == r.base, at
                for name, dtype in (("score", np.int64), ("runner", np.uint16), ("runner_score", np.int64)):
                    g = getattr(sc, name)
                    assert g.dtype == dtype and np.array_equal(g, getattr(r, name)), at + (name,)
            if "offsets" in got:
                off = got["offsets"][p][k]
                assert off.dtype == np.int8 and np.array_equal(off, r.offsets), at
            if "pens" in got:
                pens = got["pens"][p][k]
                assert pens.dtype == np.uint32 and np.array_equal(pens, r.pens), at
                assert got["costs"][p][k] == r.cost, at
            if "margins" in got:
                m = got["margins"][p][k]
                assert isinstance(m, LineMargins) and m.term.dtype == np.int32 and m.margin.dtype == np.int64, at
                assert np.array_equal(m.term, r.term) and m.runner == MM.runner_text(fm, r.runner) and np.array_equal(m.margin, r.margin), at
                assert int(m.term.astype(np.int64).sum()) == got["costs"][p][k], at
            if mode == "slack":
                idx = np.array([c.alphabet.index(ch) for ch in got["lines"][p][k][1]], dtype=np.uint16)
                K.check_invariants(fm, K.Slack(got["lines"][p][k][1], idx, got["pens"][p][k], got["offsets"][p][k], got["costs"][p][k], r.base, None))


def same_verify(dec, got, c, mode):
    """The verify image, sums and MSE of a run against draw_verify of the models' answer: the plain pens for the pen
    loop, the searched pens for the search, the returned pens for the whole-line modes."""
    who = (c.name, mode, "verify")
    want, x = FC.want(c, mode), c.geo[0]
    sq = []
    for p, (page, want_pg) in enumerate(zip(c.pages, want)):
        if mode in ("plain", "scores"):
            img, _ = M.verify_image(page, [(y, r if mode == "plain" else r.text) for y, r in want_pg], c.font, c.size, x, c.kerning, c.hinting)
        elif mode in ("search", "search_scores"):
            img, _ = S.verify_image(page, [(y, r.text, r.pens) for y, r in want_pg], FC.model(c).font, verify_font(c), x)
        else:
            img, _ = W.verify_image(page, [(y, r.text, r.pens) for y, r in want_pg], FC.model(c).font, verify_font(c), x)
        assert got["images"][p].shape == img.shape and np.array_equal(got["images"][p], img), who + (p,)
        d = img[..., 0].astype(np.int64) - img[..., 2].astype(np.int64)
        sq.append(int((d * d).sum()))
        assert got["mse"][p].tobytes() == (np.float32(sq[-1]) / np.float32(page.size)).tobytes(), who + (p,)
    idx, _ = last_batch(c)
    sums, _ = dec.verify(images=False)  # of the size group that ran last
    assert [int(s) for s in sums] == [sq[i] for i in idx], who
    assert dec._lib.focr_decoder_last_verify_launches(dec._h) == 2, who


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=["cases%d-%d" % (g[0], g[-1]) for g in GROUPS])
def test_every_mode_equals_its_model(dec, group):
    """The group's (case, mode) pairs in a seeded shuffled order on the module's one handle, every third case with the
    verify image as well, every second case's whole-line modes on a grid of one or two workgroups."""
    cases = [FC.case(i) for i in GROUPS[group]]
    pairs = [(c, mode, None) for c in cases for mode in FC.MODES] + [(c, mode, "image") for c in cases if c.index % 3 == 0 for mode in FC.MODES]
    order = np.random.default_rng([FC.SEED, 1 << 20, group]).permutation(len(pairs))
    whole = {}
    for c, mode, verify in (pairs[k] for k in order):
        got = run(dec, c, mode, verify)
        launches = dec._lib.focr_decoder_last_launches(dec._h)
        assert launches == (3 if last_batch(c)[1] else 0), (c.name, mode, launches)
        same(got, c, mode)
        if verify:
            same_verify(dec, got, c, mode)
        if mode in ("whole", "margins"):
            whole[(c.index, mode)] = got
    for c in cases:  # the margins run's texts, pens and costs are the whole-line run's
        a, b = whole[(c.index, "whole")], whole[(c.index, "margins")]
        assert a["lines"] == b["lines"] and a["costs"] == b["costs"], (c.name, "margins and whole")
        assert all(np.array_equal(u, v) for pa, pb in zip(a["pens"], b["pens"]) for u, v in zip(pa, pb)), (c.name, "margins and whole")


def test_the_used_handle_is_as_good_as_new(dec):
    """Last in the module: a plain run of case 0 on the handle equals a fresh decoder's, and closing the handle gives every
    byte of device memory back."""
    c = FC.case(0)
    got = run(dec, c, "plain", "image")
    with LineDecoder(0) as fresh:
        want = run(fresh, c, "plain", "image")
    assert got["lines"] == want["lines"] and got["mse"].tobytes() == want["mse"].tobytes(), (c.name, "plain")
    assert all(np.array_equal(a, b) for a, b in zip(got["images"], want["images"])), (c.name, "plain")
    same(got, c, "plain")
    dec.close()
    assert N.hip().focr_debug_device_bytes() == _module["bytes"], "device bytes after the module"

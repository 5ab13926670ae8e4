"""focr_decoder_refine_text (refine_text_kernel and the host plumbing of decode_refine.hip, refine_plan.h, LineDecoder.refine_text)
on the seeded cases of every decode mode that has pens to feed (tests/focr_refine_fuzz.py: the seven modes of
tests/focr_fuzz_cases.py and both forms of tests/focr_fonts_fuzz.py): Serif, sizes of 6 to 24 px, kernings off 1, hinting, crops the
page clips and cuts, two page sizes in one call, K up to 15 candidates.  Every mode runs on the DEVICE, and the device's own reading
goes back in at the pens LineDecoder.refine_text's docstring names, at a drawn (radius, sweeps, glyphs): the result equals
tests/focr_refine_model.py line by line (base, cost_in, cost, sweeps, changed, text, every pen), one launch, and the run's getters and
verify answer afterwards as before.  Device against device: cost <= cost_in, base + cost >= 0; sweeps = 0 only evaluates; cost_in is
score_text's cost wherever the model says no two glyphs share an inked pixel; a converged line fed back with its output stays as it
is; and on every third case score_text, verify_text and learn_text take the output as it is and equal their own models.  Then every
case's random readings (no run produced them: repeated lines, shared characters, empty and one-row crops, pens past the crop, any k)
through _refine_text with the raw records.  One decoder handle for the module and a seeded shuffled order, so every call meets the
buffers another font, K and geometry left.  tests/test_focr_refine_fuzz_host.py proves on the CPU what the cases reach and that the
kernel's neighbour bound is the definition.  Every comparison is == on integers or bytes.
Measured on an MI355X: the module alone 9.0 s of wall time, 7.2 s of it the CPU references; its slowest group 1.34 s.

Teeth, as measured on an MI355X with one-line mutations of the DEVICE code only (decode_refine.hip), each of which changes a
comparison or which value is selected or shortens a loop (none an index, a bound, a size or a stride), each built once and run once
against this module and tests/test_gpu_focr_refine.py; the first assertion of this module to fail is named, and whether the tests
that tests/test_gpu_focr_refine.py had before this module came (the "old" ones) fail too:
  `D < D_inc` -> `D <= D_inc` (a candidate that ties the incumbent replaces it): same_refine()'s fields == (cases 4-random, the
    random reading of page 0, radius 0), in all 13 groups and the used-handle test; old: 4 of 26 fail (test_sweeps,
    test_line_lengths, all pens equal and pens at 0, radius 0 with glyphs=False);
  `slack = radius * sweeps` -> `radius`: NOTHING here fails, and nothing old: no seeded line tells the two apart
    (tests/test_focr_refine_fuzz_host.py asserts that of the model, line by line).  The directed line for it is
    tests/test_gpu_focr_refine.py::test_the_neighbour_scan_allows_for_every_sweep (the host test's ramp page): that one fails,
    check()'s fields == (cost -333931 for -294544: the right `m` ends at pen 1107 for 1279), and it alone;
  refine_gather not skipping `k == skip` (the character's own ink in the canvas of the others): same_refine()'s fields == (cases
    4-random, whole, radius 7, 3 sweeps), in all 13 groups and the used-handle test; old: 22 of 26 fail;
  `max_bytes(c, ov)` -> `c` in refine_dword (the candidate's ink instead of the max with the others'): same_refine()'s fields ==
    (cases 4-random, whole), in all 13 groups and the used-handle test; old: 22 of 26 fail;
  refine_term's row loop ending after its first trip (`q < min(ndw, 4)`): this module PASSES (its widest tile has 5 dwords, case 4,
    and its fifth dword decides no step), and every old test passes; test_wide_tiles fails at all four sizes (check()'s fields ==,
    24 px: cost -5734225 for -5784957) and test_last_glyph_of_the_table at ndw 5 and 6 (the last column of the W is not repaired).
"""
import time

import numpy as np
import pytest

import focr_learn_model as L
import focr_refine_fuzz as RF
import focr_refine_model as R
import focr_text_fuzz as TF
from focr_fast_model import crop
from font_ocr_amd import LineDecoder
from font_ocr_amd import _native as N
from test_gpu_focr_text_fuzz import device_run, last_pages, same_scores, state

pytestmark = pytest.mark.gpu

_module = {"model_s": 0.0, "lines": {}, "records": 0, "groups": set(), "disjoint": 0, "converged": 0, "fed_again": 0, "left_out": 0}


@pytest.fixture(scope="module")
def dec():
    """One handle for the module.  Reports the module's wall time and the CPU references' share of it at the end."""
    _module["bytes"] = N.hip().focr_debug_device_bytes()
    _module["start"] = time.time()
    with LineDecoder(0) as d:
        yield d
    print(f"\ntest_gpu_focr_refine_fuzz: {time.time() - _module['start']:.1f} s of wall time, {_module['model_s']:.1f} s of it the CPU references and building the cases")


def model(f, *args, **kw):
    """A call of a CPU reference, its time counted."""
    t = time.time()
    try:
        return f(*args, **kw)
    finally:
        _module["model_s"] += time.time() - t


def launches(d):
    return d._lib.focr_decoder_last_refine_text_launches(d._h)


def same_refine(g, want, fm, who):
    """A TextRefine against focr_refine_model's Refine: every field and every pen."""
    assert tuple(g[:6]) == (want.base, want.cost_in, want.cost, want.sweeps, want.changed, R.text_of(fm, want.idx)), who + (tuple(g[:6]), tuple(want[:5]))
    assert g.pens.dtype == np.uint32 and np.array_equal(g.pens, want.pens), who + ("pens", g.pens.tolist(), want.pens.tolist())
    assert g.cost <= g.cost_in and g.base + g.cost >= 0, who


def disjoint(fm, ref, idx, pens):
    """The model's word that no two clipped glyph bitmaps of the line share an inked pixel."""
    h, w = ref.shape if ref.size else (0, 0)
    ink = np.zeros((h, w), dtype=np.int64)
    for i, s in zip(idx, pens):
        box = R.clipped(fm.font, i, s, h, w)
        if box is not None:
            ya, yb, xa, xb, c = box
            ink[ya:yb, xa:xb] += c > 0
    return ink.size == 0 or int(ink.max()) <= 1


def fed_back(d, s, count=True):
    """One (case, mode) pair: the run on the device, refine_text of its own output against the model, the properties, and the run's
    state afterwards.  Returns the run and refine_text's answer."""
    who = (s.family, s.name, s.mode)
    x, _, width, lh, _ = s.geo
    ran = device_run(d, s)
    before = state(d)
    lines, pens, fonts, radius, sweeps, glyphs = RF.fed(s, ran)
    who += (radius, sweeps, glyphs)
    ms = RF.models(s)
    listed = 1 if any(lines[i] for i in last_pages(s)) else 0
    got = d.refine_text(s.pages, lines, x, width, lh, pens, fonts=fonts, radius=radius, sweeps=sweeps, glyphs=glyphs)
    assert launches(d) == listed, who + ("launches", launches(d))
    want = model(RF.reference, s, lines, pens, fonts, radius, sweeps, glyphs)
    scored = d.score_text(s.pages, lines, x, width, lh, fonts=fonts, pens=pens, terms=False)
    again = [[], [], []]  # the converged lines whose output pens do not decrease: (page, line), the line, its pens
    n = 0
    for p, pg in enumerate(lines):
        assert len(got[p]) == len(pg), who + (p,)
        for q, (y, text) in enumerate(pg):
            g, (w, _), at = got[p][q], want[p][q], who + (p, y)
            fm = ms[fonts[p][q] if fonts is not None else 0]
            same_refine(g, w, fm, at)
            n += 1
            if sweeps == 0:
                assert (g.text, g.pens.tolist(), g.changed, g.sweeps) == (text, list(pens[p][q]), 0, 0) and g.cost == g.cost_in, at
            idx = [s.alphabet.index(c) for c in text]
            if model(disjoint, fm, crop(s.pages[p], x, y, width, lh), idx, pens[p][q]):
                assert (scored[p][q].base, scored[p][q].cost) == (g.base, g.cost_in), at + ("score_text", scored[p][q].cost, g.cost_in)
                _module["disjoint"] += count
            if 0 < g.sweeps < sweeps:
                _module["converged"] += count
                if np.all(np.diff(g.pens.astype(np.int64)) >= 0):
                    again[0].append((p, q)), again[1].append((y, g.text)), again[2].append(g.pens)
                else:
                    _module["left_out"] += count
    if again[0]:  # a fixed point: fed back with its output, nothing changes in one sweep
        pages = sorted({p for p, _ in again[0]})
        pick = lambda v: [[v[k] for k, (p, _) in enumerate(again[0]) if p == pp] for pp in pages]  # noqa: E731
        kf = None if fonts is None else [[fonts[p][q] for p, q in again[0] if p == pp] for pp in pages]
        second = d.refine_text([s.pages[p] for p in pages], pick(again[1]), x, width, lh, pick(again[2]), fonts=kf, radius=radius, sweeps=sweeps, glyphs=glyphs)
        first = pick([got[p][q] for p, q in again[0]])
        for a, b in zip((g for pg in second for g in pg), (g for pg in first for g in pg)):
            assert (a.changed, a.sweeps, a.cost, a.cost_in, a.text, a.pens.tolist()) == (0, 1, b.cost, b.cost, b.text, b.pens.tolist()), who + ("fed back",)
            _module["fed_again"] += count
    if s.index % 3 == 0:  # the other text calls take the output as it is
        out_lines = [[(y, g.text) for (y, _), g in zip(pg, got[p])] for p, pg in enumerate(lines)]
        out_pens = [[[int(v) for v in g.pens] for g in pg] for pg in got]
        scores = d.score_text(s.pages, out_lines, x, width, lh, fonts=fonts, pens=out_pens)
        ref = model(TF.reference_scores, s, out_lines, fonts=fonts, pens=out_pens)
        for p in range(len(s.pages)):
            same_scores(scores[p], ref[p], who + (p, "score_text of the output"))
        sums, imgs = d.verify_text(s.pages, out_lines, x, fonts=fonts, pens=out_pens)
        for p, (img, sq) in enumerate(model(TF.reference_pictures, s, out_lines, fonts=fonts, pens=out_pens)):
            assert int(sums[p]) == sq and imgs[p].shape == img.shape and imgs[p].tobytes() == img.tobytes(), who + (p, "verify_text of the output")
        k = max((k for pg in fonts for k in pg), default=0) if fonts is not None else 0
        learned = d.learn_text(s.pages, out_lines, x, width, lh, fonts=fonts, pens=out_pens, font=k)
        acc = model(L.learn_text, s.fonts[k], s.pages, out_lines, x, width, lh, fonts=fonts, pens=out_pens, k=k)
        assert np.array_equal(learned.sums, acc.sums) and np.array_equal(learned.counts, acc.counts), who + ("learn_text of the output", k)
        assert all(np.array_equal(a, b) for pa, pb in zip(learned.used, acc.used) for a, b in zip(pa, pb)), who + ("learn_text's used", k)
    assert state(d) == before, who + ("the run's state",)
    if count:
        key = (s.family, s.mode)
        _module["lines"][key] = _module["lines"].get(key, 0) + n
    return ran, got


def readings(d, s):
    """The case's random readings through _refine_text with the raw records, on the fonts the case's last run uploaded."""
    x, _, width, lh, _ = s.geo
    for p, page in enumerate(s.pages):
        _, r, par, want = model(RF.reading_reference, s.family, s.index, p)
        who = (s.family, s.name, "reading", p, r.placement) + par
        got = d._refine_text(np.ascontiguousarray(page[None]), [(0,) + rec for rec in r.recs], r.chars, r.pens, x, width, lh, *par)
        assert launches(d) == 1 and len(got) == len(r.recs), who
        ms = RF.models(s)
        for n, (rec, g, (w, _)) in enumerate(zip(r.recs, got, want)):
            same_refine(g, w, ms[rec[3]], who + (n,))
            _module["records"] += 1


@pytest.mark.parametrize("group", range(len(RF.GROUPS)), ids=RF.GROUP_IDS)
def test_every_mode_refined(dec, group):
    """The group's (case, mode) pairs in a seeded shuffled order on the module's one handle; behind a case's first pair, while its
    fonts are uploaded, its random readings."""
    family, ids = RF.GROUPS[group]
    pairs = [(i, mode) for i in ids for mode in RF.MODES[family]]
    order = np.random.default_rng([RF.SEED, 1 << 20, group]).permutation(len(pairs))
    read = set()
    for i, mode in (pairs[k] for k in order):
        s = model(TF.setup, family, i, mode)
        fed_back(dec, s)
        if i not in read:
            read.add(i)
            readings(dec, s)
    _module["groups"].add(group)


def compared_every_line():
    """Every mode's lines and every reading's record were compared (focr_refine_fuzz.LINES and RECORDS, which the host test holds to
    the models' runs), some lines were disjoint and some converged, and the one omission there is (a converged line whose output pens
    decrease is not fed back) stayed below half of the converged lines."""
    assert _module["lines"] == {(f, m): RF.LINES[f] for f in RF.FAMILIES for m in RF.MODES[f]}, _module["lines"]
    assert _module["records"] == RF.RECORDS
    assert _module["disjoint"] > 100 and _module["converged"] > 100, _module
    assert _module["fed_again"] + _module["left_out"] == _module["converged"] and 2 * _module["left_out"] < _module["converged"], _module


def test_the_used_handle_is_as_good_as_new(dec):
    """Last in the module: no line was left out (where every group ran in this session); case 0 of each family on the used handle
    equals a fresh decoder's; closing the handle gives every byte of device memory back."""
    if len(_module["groups"]) == len(RF.GROUPS):
        compared_every_line()
    else:
        print(f"\ntest_gpu_focr_refine_fuzz: {len(_module['groups'])} of {len(RF.GROUPS)} groups ran in this process: the count of compared lines was NOT checked")
    for family, mode in (("cases", "slack"), ("fonts", "whole")):
        s = TF.setup(family, 0, mode)
        with LineDecoder(0) as fresh:
            a, b = fed_back(dec, s, count=False), fed_back(fresh, s, count=False)
            assert repr(a) == repr(b), (family, mode)
    dec.close()
    assert N.hip().focr_debug_device_bytes() == _module["bytes"], "device bytes after the module"

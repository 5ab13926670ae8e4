"""focr_decoder_score_text and focr_decoder_verify_text (score_text_kernel, verify_layout_text_kernel, verify_compose_text_kernel
and the host plumbing of decode_score.hip and decode_text.hip) on the seeded cases of every decode mode
(tests/focr_text_fuzz.py): Serif, sizes of 6 to 24 px, kernings off 1, hinting, crops the page clips and cuts, two page sizes
in one call, K up to 15 candidates, fractional line grids.  Every mode's DEVICE outputs are fed back: score_text of them is
the run's own numbers (device against device, every row of DESIGN.md 4b-0's table) and tests/focr_score_text_model.py's,
line by line; verify_text of them is dec.verify() of that run byte for byte (after a font search, which verify() refuses,
and on every third case besides: tests/focr_verify_text_model.py's); and the run's getters and verify answer afterwards as
before.  Then every case's random readings (no run produced them: negative deltas, pens past the crop, repeated lines, shared
characters, any q, a shift radius) against the two references.  One decoder handle for the module and a seeded shuffled
order, so every call meets the buffers another font, mode and geometry left.  tests/test_focr_text_fuzz_host.py proves on
the CPU that the references agree with each other and what the cases reach.  That the runs equal their models is
tests/test_gpu_focr_fuzz.py's, test_gpu_focr_fonts_fuzz.py's, test_gpu_focr_whole_baseline.py's and
test_gpu_focr_line_frac.py's to say.  Every comparison is == on integers or bytes.
Measured on an MI355X: the module alone 5.7 s of wall time, 2.8 s of it the CPU references; its slowest group 0.85 s
(0.59 s inside the whole suite, where the slowest group of tests/test_gpu_focr_fuzz.py took 1.45 s).

Teeth, as measured on an MI355X with one-line mutations of the DEVICE code only, each of which changes a comparison or which
value is selected (none an index, a bound, a size or a stride), each built once and run once against this module; the first
assertion to fail is named:
  score_text_kernel with desc[0].origin_d for every candidate font: identity()'s cost == (the whole-line font search's own
    cost against the score of its pens; fonts 1-random, page 2, y 10), in all five fonts groups, in one of them first on a
    random reading with pens against focr_score_text_model;
  score_text_kernel's y-phase v from q >> B instead of q & (2^B - 1): identity()'s cost ==, in all eight groups of the three
    baseline families (first whole_baseline wb-0, y 4), and in no other;
  verify_layout_text_kernel with base 0 for every candidate (the tables of candidate 1): the sums == of
    focr_verify_text_model (fonts 0-random, form whole, page 0), in all five fonts groups and in the used-handle test;
  score_line's rigid shift joined to character 1's offset instead of character 0's: same_scores() of a random reading with a
    shift radius (cases 3-random, offsets, radius 21: cost and shift), in 16 of the 22 tests, every family among them;
  score_text_kernel's merge of the waves, `r < best_rank` -> `r > best_rank`: same_scores()'s shift of a random reading whose
    shifts tie (cases 3-random, radius 21: 20 for 19; and blank crops, -2 for 0), in 16 of the 22 tests.
"""
import time

import numpy as np
import pytest

import focr_fonts_fuzz as FZ
import focr_fuzz_cases as FC
import focr_text_fuzz as T
from font_ocr_amd import LineDecoder
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecoderError

pytestmark = pytest.mark.gpu

GROUP = 6
GROUPS = [(f, list(T.IDS[f][a: a + GROUP])) for f in T.FAMILIES for a in range(0, len(T.IDS[f]), GROUP)]
_module = {"model_s": 0.0}


@pytest.fixture(scope="module")
def dec():
    """One handle for the module.  Reports the module's wall time and the CPU references' share of it at the end."""
    _module["bytes"] = N.hip().focr_debug_device_bytes()
    _module["start"] = time.time()
    with LineDecoder(0) as d:
        yield d
    print(f"\ntest_gpu_focr_text_fuzz: {time.time() - _module['start']:.1f} s of wall time, {_module['model_s']:.1f} s of it the CPU references and building the cases")


def model(f, *args, **kw):
    """A call of a CPU reference, its time counted."""
    t = time.time()
    try:
        return f(*args, **kw)
    finally:
        _module["model_s"] += time.time() - t


def device_run(d, s):
    """The mode on the device, as the family's own GPU test runs it; the result named."""
    if s.family == "cases":
        return FC.run(d, s.case, s.mode)
    if s.family == "fonts":
        return FZ.searched(d, s.case, s.mode)
    d.set_font(s.fonts[0], s.case.size)
    return T.named(s, d.decode(s.pages, *s.geo, **s.run))


def last_pages(s):
    """The pages of the size group that decode(), score_text and verify_text run last."""
    shapes = list(dict.fromkeys(p.shape for p in s.pages))
    return [i for i, p in enumerate(s.pages) if p.shape == shapes[-1]]


def state(d):
    """What the last run's getters and verify answer: get, get_offsets, get_pens, get_baselines, get_fonts (through the existing
    wrapper) and the verify's sums, or its refusal."""
    lib, h = d._lib, d._h
    nl, nc = lib.focr_decoder_n_lines(h), lib.focr_decoder_n_chars(h)
    lines = (N.DecodedLine * max(1, nl))()
    chars, offs, pens = np.zeros(max(1, nc), dtype=np.uint16), np.zeros(max(1, nc), dtype=np.int8), np.zeros(max(1, nc), dtype=np.uint32)
    cost, q, qcost = np.zeros(max(1, nl), dtype=np.int64), np.zeros(max(1, nl), dtype=np.int8), np.zeros(max(1, nl), dtype=np.int64)
    assert lib.focr_decoder_get(h, lines, chars.ctypes.data) == 0 and lib.focr_decoder_get_offsets(h, offs.ctypes.data) == 0
    rcs = (lib.focr_decoder_get_pens(h, pens.ctypes.data, cost.ctypes.data), lib.focr_decoder_get_baselines(h, q.ctypes.data, qcost.ctypes.data))
    try:
        sums, none = d.verify(images=False)
        drawn = (sums.tobytes(), none, lib.focr_decoder_last_verify_launches(h))
    except DecoderError as e:  # after a font search
        drawn = str(e)
    return (nl, nc, bytes(lines), chars.tobytes(), offs.tobytes(), rcs, pens.tobytes(), cost.tobytes(), q.tobytes(), qcost.tobytes(), FZ.get_fonts(d),
            lib.focr_decoder_last_launches(h), drawn)


def same_scores(got, want, who):
    """score_text's TextScores against focr_score_text_model's Scores, [line]: base, cost, shift and every term."""
    assert len(got) == len(want), who
    for n, (g, w) in enumerate(zip(got, want)):
        assert (g.base, g.cost, g.shift) == (w.base, w.cost, w.shift), who + (n, tuple(g[:3]), tuple(w[:3]))
        assert g.terms.dtype == np.int32 and np.array_equal(g.terms, w.terms), who + (n, "terms")


def fed_back(d, s):
    """One (case, mode) pair: the run, score_text and verify_text of its outputs, and the run's state after both."""
    who = (s.family, s.name, s.mode)
    x, _, width, lh, _ = s.geo
    got = device_run(d, s)
    for page in s.pages:  # narrow pages: every strip fits LDS beside the waves' 128 bytes of sums
        assert T.strip_bytes(s, page) + 128 <= 65536, who
    before = state(d)
    kw = T.feed(s, got)
    idx = last_pages(s)
    scores = d.score_text(s.pages, got["lines"], x, width, lh, **kw)
    launches = d._lib.focr_decoder_last_score_text_launches(d._h)
    assert launches == (1 if any(got["lines"][i] for i in idx) else 0), who + ("score_text launches", launches)
    T.identity(s, got, scores)  # device against device
    want = model(T.reference_scores, s, got["lines"], **kw)
    for p in range(len(s.pages)):
        same_scores(scores[p], want[p], who + (p,))
    if s.family in T.DRAWN:
        pkw = T.picture_feed(kw)
        sums, imgs = d.verify_text(s.pages, got["lines"], x, **pkw)
        assert d._lib.focr_decoder_last_verify_text_launches(d._h) == 2, who
        assert sums.dtype == np.uint64 and len(sums) == len(imgs) == len(s.pages), who
        if s.family == "fonts":
            with pytest.raises(DecoderError, match="searched fonts"):
                d.verify()
        else:
            vsums, vimgs = d.verify()  # of the size group that ran last
            assert d._lib.focr_decoder_last_verify_launches(d._h) == 2, who
            assert [int(sums[i]) for i in idx] == [int(v) for v in vsums], who + ("sums",)
            for j, i in enumerate(idx):
                assert imgs[i].shape == vimgs[j].shape and imgs[i].tobytes() == vimgs[j].tobytes(), who + (i, "image")
        if s.family == "fonts" or s.index % 3 == 0:
            for p, (img, sq) in enumerate(model(T.reference_pictures, s, got["lines"], **pkw)):
                assert int(sums[p]) == sq and imgs[p].shape == img.shape and imgs[p].tobytes() == img.tobytes(), who + (p, "verify_text model")
    assert state(d) == before, who + ("the run's state",)
    return got, scores


def readings(d, s):
    """The case's random readings against the references only, on the fonts the case's last run uploaded."""
    x, _, width, lh, _ = s.geo
    for p, page in enumerate(s.pages):
        r = T.random_reading(s.family, s.index, p)
        who = (s.family, s.name, "reading", p, r.placement, r.shift)
        recs = [(0, y, first, n, k) for y, first, n, k, _ in r.recs]
        qs = [q for _, _, _, _, q in r.recs] if r.with_q else None
        got = d._score_text(np.ascontiguousarray(page[None]), recs, r.chars, r.along if r.placement == "pens" else None,
                            r.along if r.placement == "offsets" else None, qs, x, width, lh, r.y_bits, r.shift, True)
        assert d._lib.focr_decoder_last_score_text_launches(d._h) == 1, who
        same_scores(got, model(T.reading_scores, s, r), who)
        if not r.with_q:
            lines, kw = T.reading_lines(s, r)
            sums, imgs = d.verify_text([page], lines, x, **kw)
            img, sq = model(T.reading_picture, s, r)
            assert d._lib.focr_decoder_last_verify_text_launches(d._h) == 2, who
            assert int(sums[0]) == sq and imgs[0].shape == img.shape and imgs[0].tobytes() == img.tobytes(), who + ("verify_text",)


@pytest.mark.parametrize("group", range(len(GROUPS)), ids=["%s%s-%s" % (f, g[0], g[-1]) for f, g in GROUPS])
def test_every_mode_fed_back(dec, group):
    """The group's (case, mode) pairs in a seeded shuffled order on the module's one handle; behind a case's first pair, while
    its fonts are uploaded, its random readings."""
    family, ids = GROUPS[group]
    pairs = [(i, mode) for i in ids for mode in T.MODES[family]]
    order = np.random.default_rng([T.SEED, 1 << 20, group]).permutation(len(pairs))
    read = set()
    for i, mode in (pairs[k] for k in order):
        s = model(T.setup, family, i, mode)
        fed_back(dec, s)
        if i not in read:
            read.add(i)
            readings(dec, s)


def test_the_used_handle_is_as_good_as_new(dec):
    """Last in the module: case 0 fed back on the used handle equals a fresh decoder's, scores and pictures, and closing the
    handle gives every byte of device memory back."""
    for family, mode in (("cases", "search_scores"), ("fonts", "whole")):
        s = T.setup(family, 0, mode)
        x = s.geo[0]
        with LineDecoder(0) as fresh:
            (got, scores), (want, want_scores) = fed_back(dec, s), fed_back(fresh, s)
            assert repr(got) == repr(want) and repr(scores) == repr(want_scores), (family, mode)
            pkw = T.picture_feed(T.feed(s, got))
            a, b = dec.verify_text(s.pages, got["lines"], x, **pkw), fresh.verify_text(s.pages, got["lines"], x, **pkw)
            assert a[0].tobytes() == b[0].tobytes() and all(u.tobytes() == v.tobytes() for u, v in zip(a[1], b[1])), (family, mode)
    dec.close()
    assert N.hip().focr_debug_device_bytes() == _module["bytes"], "device bytes after the module"

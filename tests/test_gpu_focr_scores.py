"""The focr decoder's scores (line_decode_kernel<.., true>, focr_decoder_get_scores, LineDecoder.decode(scores=True), focr
--scores) at the shapes the kernel branches on, against tests/focr_scores_model.py (pinned to the reference's
score_glyph by tests/test_focr_scores_host.py): score, runner, runner_score and base are exact integers and must be
equal, and the texts must equal FastModel.decode_image's.  Each test asserts from its geometry, or from the model's
answer, that it reaches the branch it names."""
import csv
import os
import subprocess

import numpy as np
import pytest

import focr_line_model as M
import focr_scores_model as S
from focr_fast_model import ALPHABET_319, ASCII95, LARGEST_SIZE, TIE_GROUPS, FastModel, line_cap, narrowest_glyph_line, permuted_319
from font_ocr_amd import FOCR_DEFAULT_ALPHABET, LineDecoder, LineScores, save_pgm
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONO = os.path.join(GOLD, "DejaVuSansMono.ttf")
SANS = os.path.join(GOLD, "DejaVuSans.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
LDS_STRIP_MAX = 65536     # decode.hip: a strip up to this many bytes is staged in LDS, a larger one is read from global
COMPACT_THREADS = 1024    # decode.hip: line_compact_kernel's slots per iteration
LANES = 64                # decode.hip: lane l scores glyphs l, l + 64, ...

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    with LineDecoder(0) as d:
        yield d


def strip_bytes(page_w, x, width, line_height):
    """focr_decoder_run's strip: crop width w clamped to the page, stride = ((w + 7) / 4 + 2) * 4 bytes per row."""
    w = min(width, page_w - min(x, page_w))
    return ((w + 7) // 4 + 2) * 4 * line_height


def _ink(alphabet):
    return "".join(c for c in alphabet if not c.isspace())


def _text(rng, alphabet, n):
    return "".join(rng.choice(list(alphabet), n))


def _equal(got, want, where):
    """A LineScores of the device against the model's Scored of the same line."""
    assert isinstance(got, LineScores) and isinstance(got.base, int), where
    assert got.base == want.base, where
    for name, dtype in (("score", np.int64), ("runner", np.uint16), ("runner_score", np.int64)):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == dtype and g.shape == w.shape and np.array_equal(g, w), (where, name)


def _check(dec, fm, pages, geo):
    """Decode with scores on: texts equal to the fast model's, scores equal to the scores model's.  Returns the model's
    [[(y, Scored)] per page]."""
    want = [S.image_scores(fm, p, *geo) for p in pages]
    lines, scores = dec.decode(pages, *geo, scores=True)
    assert lines == [fm.decode_image(p, *geo) for p in pages]
    assert lines == [[(y, sc.text) for y, sc in pg] for pg in want]
    assert [len(pg) for pg in scores] == [len(pg) for pg in lines]
    for p, (got_pg, want_pg) in enumerate(zip(scores, want)):
        for got, (y, sc) in zip(got_pg, want_pg):
            _equal(got, sc, (p, y))
    return want


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129])
def test_alphabet_sizes_around_the_stripe(dec, n):
    """Alphabets of 1, 2, 63, 64, 65, 128 and 129 glyphs on one 200x16 line of Mono 13 px: no runner at all, a runner on
    another lane, full stripes, and a last stripe that holds one glyph.  The second ASCII95 repeats the first, so from
    96 glyphs on a glyph and its copy 95 places later tie."""
    al = (ASCII95 + ALPHABET_319)[:n]
    page = np.full((16, 200), 255, dtype=np.uint8)
    S.draw(page, MONO, 13.0, "Il1 O0o ;:., rn m +/= 5S 8B", 0, 1)
    fm = FastModel(MONO, 13.0, al)
    dec.set_font(fm.font, 13.0)
    (_, sc), = _check(dec, fm, [page], (0, 0, 200, 16, 16))[0]
    best = np.array([al.index(c) for c in sc.text])
    if n == 1:
        assert np.all(sc.runner == S.NO_RUNNER) and np.all(sc.runner_score == S.INT64_MAX)
    else:
        assert np.all(sc.runner < n) and np.all(sc.runner != best)
        assert np.any(sc.runner % LANES != best % LANES)
    assert (n + LANES - 1) // LANES == {1: 1, 2: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 3}[n]
    if n >= 128:
        tied = best + 95 < n
        assert tied.any() and np.all(sc.runner[tied] == best[tied] + 95) and np.all(sc.runner_score[tied] == sc.score[tied])
    fm.close()


def _tie_page(font, W, seed):
    """As tests/test_gpu_focr_shapes.py's: lines that are mostly A, o and spaces."""
    rng = np.random.default_rng(seed)
    page = np.full((34, W), 255, dtype=np.uint8)
    for ly in (2, 18):
        S.draw(page, font, 13.0, "".join(rng.choice(list("AAoo  " + "xyzéŁž"), 30)), 1, ly)
    return page


@pytest.mark.parametrize("font", [MONO, SANS], ids=["mono", "sans"])
@pytest.mark.parametrize("order", ["plain", "permuted"])
def test_ties_and_one_lane(dec, font, order):
    """319 glyphs with tie groups of identical glyphs.  Permuted, a group sits on one lane (5, 69, 133 for the three A
    look-alikes): the lane's own top-2 holds both the best and the runner.  Wherever a group's first member wins, the
    runner is its next member by index, at the same score."""
    al = ALPHABET_319 if order == "plain" else permuted_319()
    if order == "permuted":
        assert [al.index(c) for c in "АAΑ"] == [5, 69, 133]
    page = _tie_page(font, 110, 5 + (font == SANS))
    fm = FastModel(font, 13.0, al)
    dec.set_font(fm.font, 13.0)
    want = _check(dec, fm, [page], (0, 0, 200, 15, 16))[0]
    best = np.concatenate([[al.index(c) for c in sc.text] for _, sc in want])
    runner = np.concatenate([sc.runner for _, sc in want])
    margin = np.concatenate([sc.runner_score - sc.score for _, sc in want])
    for grp in TIE_GROUPS:
        first, second = sorted(al.index(c) for c in grp)[:2]
        assert (first % LANES == second % LANES) == (order == "permuted")
        won = best == first
        assert won.any() and np.all(margin[won] == 0), grp
        # (the blanks also tie with every glyph that falls outside the crop, such as '_' below it: an earlier index may be the runner)
        assert np.all(runner[won] <= second) if grp.isspace() else np.all(runner[won] == second), grp
    assert np.any(margin > 0)
    fm.close()


def test_lds_and_global_strip(dec):
    """line_decode_kernel<true, true> with a strip of exactly 65536 bytes (w 1012) and <false, true> one dword per row
    past it (w 1013): the top-2 and the r^2 sum read LDS on one side and global memory on the other."""
    font, size, lh = SANS, 24.0, 64
    W, H = 1013, 3 * lh
    assert strip_bytes(W, 0, 1012, lh) == LDS_STRIP_MAX
    assert strip_bytes(W, 0, 1013, lh) == 65792 > LDS_STRIP_MAX
    page = _boundary_page()
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    lds = _check(dec, fm, [page], (0, 0, 1012, lh, lh))[0]
    glob = _check(dec, fm, [page], (0, 0, 1013, lh, lh))[0]
    assert [y for y, _ in lds] == [y for y, _ in glob] == [0, 64, 128]
    assert all(len(sc.text) > 60 for _, sc in glob)
    assert any(a.base != b.base for (_, a), (_, b) in zip(lds, glob))  # column 1012 carries ink
    fm.close()


def _boundary_page():
    font, size, lh, W = SANS, 24.0, 64, 1013
    rng = np.random.default_rng(31)
    page = np.full((3 * lh, W), 255, dtype=np.uint8)
    for s in range(3):
        for dy in (3, 33):
            S.draw(page, font, size, _text(rng, FOCR_DEFAULT_ALPHABET, 85), 0, s * lh + dy)
    page[:, 1012] = np.minimum(page[:, 1012], 200)
    return page


def test_clipped_crops(dec):
    """A last line slot cut by the page bottom (6 rows of 15) and an x that leaves 50 of 120 columns: base sums the crop
    only, and the glyph rows below the crop do not count."""
    font, size = MONO, 13.0
    W, H, geo = 150, 40, (100, 2, 120, 15, 16)
    x, y, width, lh, adv = geo
    ys = list(range(y, H, adv))
    assert ys == [2, 18, 34] and H - ys[-1] == 6 < lh and W - x == 50 < width
    rng = np.random.default_rng(4)
    page = np.full((H, W), 255, dtype=np.uint8)
    for ly in ys:
        S.draw(page, font, size, _text(rng, _ink(FOCR_DEFAULT_ALPHABET), 12), 60, ly)
    page = np.minimum(page, 255 - rng.integers(0, 30, page.shape)).astype(np.uint8)
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    want = _check(dec, fm, [page], geo)[0]
    assert [ly for ly, _ in want] == ys
    r = 255 - page.astype(np.int64)
    assert [sc.base for _, sc in want] == [int((r[ly: ly + lh, x:] ** 2).sum()) for ly in ys]
    assert want[-1][1].base < int((r[ys[-1]:, :] ** 2).sum())
    fm.close()


def test_base_past_32_bits(dec):
    """A 2480-px line of 40 rows, fully black: base = 2480 * 40 * 255^2 is about 6.4e9, past uint32, and every score is
    base plus a negative term."""
    font, size, lh, adv = MONO, 13.0, 40, 44
    W, H = 2480, 44
    page = np.full((H, W), 255, dtype=np.uint8)
    page[2: 2 + lh] = 0
    assert strip_bytes(W, 0, W, lh) > LDS_STRIP_MAX
    fm = FastModel(font, size, ASCII95)
    dec.set_font(fm.font, size)
    (ly, sc), = _check(dec, fm, [page], (0, 2, W, lh, adv))[0]
    assert ly == 2 and sc.base == W * lh * 255 * 255 > 2 ** 32
    assert np.all(sc.score <= sc.base) and np.any(sc.score < sc.base) and np.all(sc.score > 2 ** 32)
    fm.close()


def _largest_size_page(font, size):
    """As tests/test_gpu_focr_shapes.py's: one line of big glyphs, a fully inked block, noise."""
    rng = np.random.default_rng(2)
    page, _ = M.synth_page(rng, font, size, _ink(FOCR_DEFAULT_ALPHABET), 520, 240, 2, 2, 230, 1)
    page[10:200, 330:470] = 0
    return np.minimum(page, 255 - rng.integers(0, 40, page.shape)).astype(np.uint8)


def test_largest_accepted_size(dec):
    """Sans at the largest size the builder accepts, over a fully inked block: the footprint term is at its most
    negative, next to the int32 bound the builder keeps, and the host adds it to base in int64."""
    font, size = SANS, LARGEST_SIZE[("DejaVuSans.ttf", "default")]
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    area = max(fm.font.s.glyphs[i].stride * fm.font.s.glyphs[i].box_h for i in range(fm.font.s.n_glyphs))
    assert 2 ** 30 < area * 2 * 255 * 255 < 2 ** 31
    page = _largest_size_page(font, size)
    dec.set_font(fm.font, size)
    tall, thin = (1, 2, 600, int(size) + 30, 400), (0, 60, 600, 9, 400)
    assert strip_bytes(520, 1, 600, tall[3]) > LDS_STRIP_MAX >= strip_bytes(520, 0, 600, thin[3])
    terms = []
    for geo in (tall, thin):
        (_, sc), = _check(dec, fm, [page], geo)[0]
        terms.append(sc.score - sc.base)
    assert terms[0].min() < -(2 ** 28), terms[0].min()  # a quarter of the int32 range below zero on the inked block
    fm.close()


@pytest.mark.parametrize("n_pages,slots", [(33, 31), (25, 41)], ids=["1023", "1025"])
def test_compaction_keeps_scores_aligned(dec, n_pages, slots):
    """Mostly blank batches of 1023 and 1025 slots, ink on slots 1022, 1023, 1024, the last, and a sparse random set:
    the per-line base and the per-step arrays follow the work list, so every line gets its own."""
    font, size, adv, W = MONO, 13.0, 4, 24
    total = n_pages * slots
    assert total in (COMPACT_THREADS - 1, COMPACT_THREADS + 1)
    rng = np.random.default_rng(total)
    inked = {s for s in (1022, 1023, 1024, total - 1) if s < total} | {int(s) for s in rng.choice(total, 25, replace=False)}
    pages = np.full((n_pages, slots * adv, W), 255, dtype=np.uint8)
    for s in inked:
        p, i = divmod(s, slots)
        c = int(rng.integers(0, W - 4))
        pages[p, i * adv + 1: i * adv + 3, c: c + 1 + s % 4] = int(rng.integers(0, 120))
    fm = FastModel(font, size, FOCR_DEFAULT_ALPHABET)
    dec.set_font(fm.font, size)
    want = _check(dec, fm, list(pages), (0, 0, W, adv, adv))
    assert [(p, y) for p, pg in enumerate(want) for y, _ in pg] == [(s // slots, s % slots * adv) for s in sorted(inked)]
    assert len({sc.base for pg in want for _, sc in pg}) > len(inked) // 2  # the lines differ: a misplaced one would show
    fm.close()


def test_cap_reached(dec):
    """A Sans 13 px line of the narrowest of 319 glyphs: the line fills its cap slots of every per-step array, with a
    second line behind it whose slots start right after."""
    font, size, W = SANS, 13.0, 300
    line, ch, cap = narrowest_glyph_line(font, size, ALPHABET_319, W)
    page = np.full((32, W), 255, dtype=np.uint8)
    page[:16] = line
    S.draw(page, font, size, "second line", 0, 16)
    fm = FastModel(font, size, ALPHABET_319)
    assert cap == line_cap(fm.incs, W) > LANES
    dec.set_font(fm.font, size)
    want = _check(dec, fm, [page], (0, 0, W, 16, 16))[0]
    assert [y for y, _ in want] == [0, 16] and len(want[0][1].text) == cap and len(want[1][1].text) < cap
    fm.close()


def test_switch_on_and_off(dec):
    """The LDS / global boundary batch with scores on, then off: the same texts, three launches either way, the same
    verify images and errors, and no scores to fetch after the run with scores off."""
    font, size, lh = SANS, 24.0, 64
    page = _boundary_page()
    dec.set_font(font, size)
    lib, h = dec._lib, dec._h
    for width in (1012, 1013):
        geo = (0, 0, width, lh, lh)
        on, on_mse, on_img, scores = dec.decode([page], *geo, verify="image", scores=True)
        assert lib.focr_decoder_last_launches(h) == 3
        nl, nc = lib.focr_decoder_n_lines(h), lib.focr_decoder_n_chars(h)
        assert nl == 3 == len(scores[0]) and nc == sum(len(s.score) for s in scores[0])
        cs, base = (N.CharScore * nc)(), np.zeros(nl, dtype=np.uint64)
        assert lib.focr_decoder_get_scores(h, cs, None) == 0 and lib.focr_decoder_get_scores(h, None, base.ctypes.data) == 0
        assert [c.score for c in cs] == [int(v) for s in scores[0] for v in s.score] and [int(b) for b in base] == [s.base for s in scores[0]]
        off, off_mse, off_img = dec.decode([page], *geo, verify="image")
        assert lib.focr_decoder_last_launches(h) == 3
        assert off == on and off_mse.tobytes() == on_mse.tobytes() and off_img[0].tobytes() == on_img[0].tobytes()
        assert lib.focr_decoder_get_scores(h, cs, base.ctypes.data) != 0
        assert b"scores" in lib.focr_decoder_last_error(h)
        assert dec.decode([page], *geo) == on


def test_no_scores_without_a_run():
    with LineDecoder(0) as d:
        assert d._lib.focr_decoder_get_scores(d._h, None, None) != 0
        d._check(d._lib.focr_decoder_set_scores(d._h, 1))
        assert d._lib.focr_decoder_get_scores(d._h, None, None) != 0
        assert b"focr_decoder_get_scores" in d._lib.focr_decoder_last_error(d._h)


def test_memory_returns(dec):
    """A decoder that ran with scores on gives all its device memory back when it is destroyed."""
    before = N.hip().focr_debug_device_bytes()
    page = np.full((32, 120), 255, dtype=np.uint8)
    S.draw(page, MONO, 13.0, "memory", 0, 1)
    with LineDecoder(0) as d:
        d.set_font(MONO, 13.0)
        plain = N.hip().focr_debug_device_bytes()
        d.decode([page], 0, 0, 120, 16, 16)
        off = N.hip().focr_debug_device_bytes()
        _, scores = d.decode([page], 0, 0, 120, 16, 16, scores=True)
        on = N.hip().focr_debug_device_bytes()
        assert len(scores[0]) == 1 and before < plain < off < on
    assert N.hip().focr_debug_device_bytes() == before


def test_cli_scores_csv(dec, tmp_path):
    """focr --scores on two pages of different sizes: the CSV rows are the Python API's values in the order of stdout,
    and stdout is the run's without the flag."""
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    font, size, geo = MONO, 13.0, (1, 2, 140, 15, 16)
    rng = np.random.default_rng(9)
    pages = [np.full((H, 150), 255, dtype=np.uint8) for H in (52, 36)]
    for pg in pages:
        for ly in range(2, pg.shape[0] - 15, 16):
            S.draw(pg, font, size, _text(rng, _ink(FOCR_DEFAULT_ALPHABET), 14), 1, ly)
    paths = []
    for i, pg in enumerate(pages):
        paths.append(str(tmp_path / f"page{i}.pgm"))
        save_pgm(paths[-1], pg)
    out = tmp_path / "out.csv"
    cmd = [FOCR, "-f", font, "-t", str(size), "-x", "1", "-y", "2", "-w", "140", "--line-height", "15", "--line-advance", "16"]
    plain = subprocess.run(cmd + ["-i"] + paths, capture_output=True, text=True, timeout=300)
    r = subprocess.run(cmd + ["--scores", str(out), "-i"] + paths, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and r.returncode == 0, (plain.stderr, r.stderr)
    dec.set_font(font, size)
    lines, scores = dec.decode(pages, *geo, scores=True)
    assert r.stdout == plain.stdout == "".join(t + "\n" for pg in lines for _, t in pg) and len(r.stdout) > 60
    want = [["image_index", "y", "column", "codepoint", "score", "runner_codepoint", "runner_score", "margin"]]
    for i, (pg, sc_pg) in enumerate(zip(lines, scores)):
        for (y, text), sc in zip(pg, sc_pg):
            for c, ch in enumerate(text):
                want.append([str(v) for v in (i, y, c, ord(ch), sc.score[c], ord(FOCR_DEFAULT_ALPHABET[sc.runner[c]]), sc.runner_score[c],
                                              sc.runner_score[c] - sc.score[c])])
    with open(out, newline="") as f:
        assert list(csv.reader(f)) == want
    one = subprocess.run(cmd + ["-a", "A", "--scores", str(out), "-i", paths[1]], capture_output=True, text=True, timeout=300)
    assert one.returncode == 0 and set(one.stdout) == {"A", "\n"}, one.stderr
    with open(out, newline="") as f:
        rows = list(csv.reader(f))[1:]
    assert len(rows) == len(one.stdout.replace("\n", "")) and all(r[3] == "65" and r[5] == "" and r[7] == "" for r in rows)

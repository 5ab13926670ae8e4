"""focr_verify_images (ncc_images.hip: ncc_records_kernel, ncc_compose_kernel) against the numpy model of
tests/ncc_verify_model.py, bit for bit in the images and the sums.  The model is fed the device's own characters (Scanner.lines()),
and most cases place them with Scanner.debug_process_hits, so that boxes land on the tile seams (16 rows x 256 columns), on each
other and on the page's edges on purpose; the last cases go through a scan, the executor, the fleet and the `ncc` CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from font_ocr_amd import ASCII95, Bank, save_pgm, synth_page
from font_ocr_amd.bank import SYNTH_SEED_BASE, TEMPLATE_DTYPE, load_image_rgba
from font_ocr_amd.searcher import Fleet, FocrError, Pipeline, Scanner, verify_mse
from ncc_verify_model import triple_of, verify_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCC = os.path.join(ROOT, "font_ocr_amd", "bin", "ncc")
FONT = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")


def make_bank(sizes, seed, holes=0.3):
    """Random templates of the given (w, h) sizes; about `holes` of their bytes are 0 (a character's see-through pixels)."""
    rng = np.random.default_rng(seed)
    tm = np.zeros(len(sizes), TEMPLATE_DTYPE)
    parts, off = [], 0
    for i, (w, h) in enumerate(sizes):
        nd = rng.integers(1, 256, w * h, dtype=np.uint8)
        nd[rng.random(w * h) < holes] = 0
        nd[0] = 255  # never a constant template
        tm[i]["letter"], tm[i]["n_w"], tm[i]["n_h"], tm[i]["offset"] = 65 + i, w, h, off
        parts.append(nd)
        off += nd.size
    return Bank(tm, np.concatenate(parts), len(sizes), 0, 0, 13.0, 8.0)


def random_luma(n, r_h, r_w, seed):
    """Pages with every kind of pixel: paper (255), black (0) and greys."""
    rng = np.random.default_rng(seed)
    luma = rng.integers(0, 256, (n, r_h, r_w), dtype=np.uint8)
    luma[rng.random(luma.shape) < 0.5] = 255
    luma[rng.random(luma.shape) < 0.05] = 0
    return luma


def place(sc, hits, overlap=-1):
    """hits: (page, y, x, t) tuples -> the context's characters (all above the anchor; overlap -1: each one its own character)."""
    hits = sorted(set(hits))
    cols = [np.array([h[k] for h in hits], np.uint32) for k in range(4)]
    sc.debug_process_hits(*cols, np.full(len(hits), 0.99, np.float32), np.ones(len(hits), np.uint8))
    sc.process_hits(0.95, overlap)
    return len(hits)


def check(sc, bank, luma, reverse_differs=False):
    """verify_images() == the model over the device's own characters; returns (rgb, sums)."""
    triple = triple_of(sc.lines())
    want_rgb, want_sums = verify_model(255 - luma, bank, *triple)
    rgb, sums = sc.verify_images()
    assert rgb.shape == want_rgb.shape and rgb.dtype == np.uint8 and sums.dtype == np.uint64
    assert np.array_equal(sums, want_sums), (sums, want_sums)
    bad = np.argwhere(rgb != want_rgb)
    assert len(bad) == 0, (len(bad), bad[:5])
    assert sc.last_verify_images()["launches"] == 2  # whatever the data
    if reverse_differs:
        back, _ = verify_model(255 - luma, bank, *triple, reverse=True)
        assert not np.array_equal(back, want_rgb)  # the case can tell the orders apart
    return rgb, sums


@pytest.fixture(scope="module")
def bank8():
    return make_bank([(8, 8)] * 4 + [(9, 15)] * 2, 11)


@pytest.fixture(scope="module")
def sc8(bank8):
    s = Scanner(0)
    s.set_bank(bank8)
    yield s
    s.close()


@pytest.mark.parametrize("r_w,r_h", [(257, 17), (301, 40), (512, 32)])
def test_tile_seams(sc8, bank8, r_w, r_h):
    """One pixel past a tile, a width that is no multiple of 4, exact multiples: 8x8 boxes with corners at x in {1, 248 .. 257 - w,
    r_w - w} and y in {1, 9 .. 17, r_h - h}, so that they straddle every x = 256 and y = 16 / 32 seam and touch the last row and
    column; two 9x15 boxes besides, and one box that hangs over the page's corner (clipped, as the model clips it)."""
    luma = random_luma(2, r_h, r_w, r_w)
    sc8.set_pages(luma)
    xs = sorted({1, r_w - 8} | {x for x in range(248, 257 - 8 + 1)} | {x for x in (500, 504) if x + 8 <= r_w})
    ys = sorted({1, r_h - 8} | {y for y in range(9, 18) if y + 8 <= r_h})
    hits = [(p, y, x, (x + y + p) % 4) for p in range(2) for y in ys for x in xs]
    hits += [(0, 1, 250, 4), (1, max(r_h - 15, 0), r_w - 9, 5), (1, r_h - 2, r_w - 3, 1)]
    n = place(sc8, hits)
    assert sc8.total_chars() == n
    check(sc8, bank8, luma)


def test_order_inside_a_line_and_across_lines(sc8, bank8):
    """Two anchored lines one pixel apart, hits one pixel apart inside them (overlap -1: every one a character), templates with
    interior zeros: a later character's ink wins, its zeros do not, inside a line and from line to line."""
    luma = random_luma(1, 20, 64, 3)
    sc8.set_pages(luma)
    n = place(sc8, [(0, y, x, (3 * x + y) % 4) for y in (3, 4) for x in range(1, 41)])
    assert sc8.total_chars() == n == 80
    check(sc8, bank8, luma, reverse_differs=True)


def test_many_characters_in_one_tile(sc8, bank8):
    """Rows y = 1 .. 20, x = 1 .. 280, 8x8 templates, overlap -1: 5 600 characters, about 4 000 of them over the page's first tile,
    from 20 lines.  ncc_compose_kernel stages no records and has no per-pass count to exceed (its marks carry the batch-wide
    character index, ncc_images.hip's header): this is the case that a kernel with a fixed per-tile list would truncate."""
    luma = random_luma(1, 40, 300, 9)
    sc8.set_pages(luma)
    n = place(sc8, [(0, y, x, (x * 7 + y * 3) % 4) for y in range(1, 21) for x in range(1, 281)])
    assert sc8.total_chars() == n == 5600
    check(sc8, bank8, luma, reverse_differs=True)


def test_template_sizes():
    """3x2, 16x32, 32x40 (wide and tall: the classes the exact scan serves) and 9x15 in one bank, a character of each on one page."""
    bank = make_bank([(3, 2), (16, 32), (32, 40), (9, 15)], 21)
    luma = random_luma(1, 64, 128, 4)
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(luma)
        assert place(sc, [(0, 1, 1, 0), (0, 10, 5, 1), (0, 20, 40, 2), (0, 40, 100, 3), (0, 20, 60, 1)]) == 5
        check(sc, bank, luma)


def test_empty_pages_empty_batches_and_single_outputs(sc8, bank8):
    luma = random_luma(3, 20, 64, 6)
    sc8.set_pages(luma)
    place(sc8, [(0, 2, 3, 0), (2, 5, 30, 1), (2, 5, 40, 4)])  # nothing on page 1
    rgb, sums = check(sc8, bank8, luma)
    assert not rgb[1, :, :, 2].any() and rgb[1, :, :, 0].any()
    only_sums = sc8.verify_images(rgb=None)
    assert only_sums[0] is None and np.array_equal(only_sums[1], sums)
    only_rgb = sc8.verify_images(sq_sums=None)
    assert only_rgb[1] is None and np.array_equal(only_rgb[0], rgb)
    with pytest.raises(FocrError):
        sc8.verify_images(rgb=None, sq_sums=None)  # FOCR_ERR_INVALID
    # hits, but none reaches the anchor: process_hits runs and yields no character
    cols = [np.array(v, np.uint32) for v in ([0, 1], [2, 3], [4, 5], [0, 1])]
    sc8.debug_process_hits(*cols, np.array([0.9, 0.9], np.float32), np.ones(2, np.uint8))
    sc8.process_hits(0.95, 5)
    assert sc8.total_chars() == 0
    rgb, _ = check(sc8, bank8, luma)
    assert not rgb[..., 2].any()
    # no hits at all: process_hits launches nothing
    empty = np.zeros(0, np.uint32)
    sc8.debug_process_hits(empty, empty, empty, empty, np.zeros(0, np.float32), np.zeros(0, np.uint8))
    sc8.process_hits(0.95, 5)
    rgb, _ = check(sc8, bank8, luma)
    assert not rgb[..., 2].any()


def plant(bank, n, r_h, r_w, seed):
    """Pages with the bank's templates pasted verbatim on two text rows (similarity 1 at every corner) on clean paper."""
    rng = np.random.default_rng(seed)
    ink = np.zeros((n, r_h, r_w), np.uint8)
    for p in range(n):
        for y in (3 + p % 3, 26 + p % 2):
            x = 2 + p
            while x + 12 < r_w:
                t = int(rng.integers(0, len(bank)))
                nd = bank.needle(t)
                ink[p, y: y + nd.shape[0], x: x + nd.shape[1]] = nd
                x += nd.shape[1] + int(rng.integers(2, 6))
    return 255 - ink


@pytest.fixture(scope="module")
def bank12():
    return make_bank([(9, 15)] * 6 + [(8, 15)] * 6, 31, holes=0.2)


def test_state(bank12):
    luma = plant(bank12, 2, 48, 301, 1)
    with Scanner(0) as sc:
        sc.set_bank(bank12)
        sc.set_pages(luma)
        with pytest.raises(FocrError, match=r"\[3\]"):  # FOCR_ERR_STATE: before any scan
            sc.verify_images()
        sc.scan(0.8)
        with pytest.raises(FocrError, match=r"\[3\]"):  # a scan without process_hits
            sc.verify_images()
        sc.process_hits(0.95, 5)
        assert sc.total_chars() > 20
        a = sc.verify_images()
        b = sc.verify_images()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        sc.scan(0.8)
        with pytest.raises(FocrError, match=r"\[3\]"):  # the next scan: again until process_hits has run
            sc.verify_images()
        sc.process_hits(0.95, 5)
        c = sc.verify_images()
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


def test_through_a_scan_split_batches_and_ink_high_uploads(bank12):
    luma = plant(bank12, 4, 48, 301, 2)
    with Scanner(0) as sc:
        sc.set_bank(bank12)
        sc.set_pages(luma)
        sc.scan(0.8)
        sc.process_hits(0.95, 5)
        assert sc.total_chars() > 100
        rgb, sums = check(sc, bank12, luma)
        assert rgb[..., 2].any() and sums.max() < 255 ** 2 * 301 * 48
        sc.force_split(True)
        sc.scan(0.8)
        sc.process_hits(0.95, 5)
        split = check(sc, bank12, luma)
        sc.force_split(False)
        assert split[0].tobytes() == rgb.tobytes() and np.array_equal(split[1], sums)
        sc.set_pages(255 - luma, invert=False)  # the same pages as ink-high bytes
        sc.scan(0.8)
        sc.process_hits(0.95, 5)
        ink_high = sc.verify_images()
        assert ink_high[0].tobytes() == rgb.tobytes() and np.array_equal(ink_high[1], sums)


def test_executor_and_fleet(bank12):
    """Three batches in flight; each waited context draws its own batch's images before its release, while later batches are
    queued behind it on the device: the same bytes as the batch gives on a plain Scanner."""
    batches = [plant(bank12, 3, 48, 301, 10 + b) for b in range(3)]
    want = []
    with Scanner(0) as sc:
        sc.set_bank(bank12)
        for luma in batches:
            sc.set_pages(luma)
            sc.scan(0.8)
            sc.process_hits(0.95, 5)
            want.append(check(sc, bank12, luma))
    assert want[0][0].tobytes() != want[1][0].tobytes()
    for make in (lambda: Pipeline(0, 2), lambda: Fleet([0], lanes=2)):
        ex = make()
        try:
            ex.set_bank(bank12)
            tickets = [ex.submit(luma, threshold=0.8, anchor_threshold=0.95, overlap=5) for luma in batches]
            for t, (rgb, sums) in zip(tickets, want):
                view = ex.wait(t)
                got = view.verify_images()
                assert got[0].tobytes() == rgb.tobytes() and np.array_equal(got[1], sums)
                ex.release(t)
        finally:
            ex.close()


DEVICE_OUTPUT = r"""
import sys
import numpy as np
import torch  # first: the process then has one HIP runtime, torch's, and the library binds to it
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from font_ocr_amd.searcher import Scanner
from ncc_verify_model import triple_of, verify_model
from test_gpu_ncc_verify import make_bank, place, random_luma
bank = make_bank([(8, 8)] * 4 + [(9, 15)] * 2, 11)
luma = random_luma(2, 20, 70, 8)
with Scanner(0) as sc:
    sc.set_bank(bank)
    sc.set_pages(luma)
    place(sc, [(0, 2, 3, 0), (1, 5, 30, 1), (1, 5, 40, 4)])
    want_rgb, want_sums = verify_model(255 - luma, bank, *triple_of(sc.lines()))
    out = torch.zeros(want_rgb.shape, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    back, sums = sc.verify_images(out=out.data_ptr())
    assert back == out.data_ptr() and np.array_equal(sums, want_sums)
    assert np.array_equal(out.cpu().numpy(), want_rgb)
    host = np.zeros_like(want_rgb)
    assert sc.verify_images(out=host)[0] is host and np.array_equal(host, want_rgb)
print("device output ok")
"""


def test_device_output():
    """rgb_on_device into a torch tensor equals the host output and the model.  In a process of its own that imports torch before
    the library is loaded, as bench.py does: torch brings a HIP runtime of its own, and a process gets one."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_OUTPUT, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "device output ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(FONT), reason="DejaVu Sans Mono not installed")
def test_cli_verify(tmp_path):
    if not os.path.exists(NCC):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    alphabet = ASCII95[1:60]
    bank = Bank.rasterize(FONT, 13, 0, 0, alphabet=alphabet)
    pages = np.stack([synth_page(bank, SYNTH_SEED_BASE + 700 + p, 300, 100) for p in range(3)])
    paths = []
    for p in range(3):
        paths.append(str(tmp_path / f"page{p}.pgm"))
        save_pgm(paths[-1], pages[p])
    out_dir = tmp_path / "verify"
    out_dir.mkdir()
    cmd = [NCC, "-f", FONT, "-t", "13", "-a", alphabet, "-i"] + paths
    plain = subprocess.run(cmd, capture_output=True)
    drawn = subprocess.run(cmd + ["--verify", str(out_dir)], capture_output=True)
    assert plain.returncode == 0 and drawn.returncode == 0, drawn.stderr
    assert drawn.stdout == plain.stdout and len(plain.stdout) > 50
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(pages)
        sc.scan(0.8)
        sc.process_hits(0.95, 5)
        rgb, sums = check(sc, bank, pages)
    assert rgb[..., 2].any()
    for p in range(3):
        png = load_image_rgba(str(out_dir / f"page{p}.png"))
        assert np.array_equal(png[..., :3], rgb[p]) and (png[..., 3] == 255).all()
    mse = verify_mse(sums, 300, 100)
    assert drawn.stderr.decode().splitlines() == [f"{paths[p]} {float(mse[p]):.6f}" for p in range(3)]

"""PageFeed (csrc/cli/page_feed.h: `ncc`'s header probe, batch plan, slab ring, decoder threads and PNG queue) without a
device: csrc/cli/page_feed_check.cpp is built as a stand-alone program under the sanitizers and run directly."""
import os
import platform
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "font_ocr_amd", "csrc")
LIB = os.path.join(ROOT, "font_ocr_amd", "lib")

N_PAGES, BATCH_PAGES = 37, 4
SIZES = ((23, 17), (31, 9))  # (w, h), in runs of 5 and 3 pages: the size changes in mid-batch
RUNS = (5, 3)


def page_size(i):
    return SIZES[0] if i % sum(RUNS) < RUNS[0] else SIZES[1]


@pytest.fixture(scope="module")
def pages(tmp_path_factory):
    d = tmp_path_factory.mktemp("feed_pages")
    for i in range(N_PAGES):
        w, h = page_size(i)
        px = ((i * 7 + np.arange(h)[:, None] + np.arange(w)[None, :]) & 255).astype(np.uint8)
        (d / f"p{i:02d}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (w, h) + px.tobytes())
    # the plan, computed here on its own: consecutive pages of one size, at most BATCH_PAGES per batch
    batches = []
    for i in range(N_PAGES):
        if not batches or batches[-1][1] == BATCH_PAGES or batches[-1][2:] != list(page_size(i)):
            batches.append([i, 0, *page_size(i)])
        batches[-1][1] += 1
    assert len(batches) == 14 and [b[1] for b in batches[:4]] == [4, 1, 3, 4]
    return d, [",".join(map(str, b)) for b in batches]


def own_env(cxx):
    """The environment of the compiler and of the check program: no sanitizer options, and none of this compiler's sanitizer
    runtimes preloaded. The program carries its own runtime, and a second one in the process aborts it at start."""
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "TSAN_OPTIONS", "LSAN_OPTIONS")}
    if env.get("LD_PRELOAD"):
        runtimes = {os.path.realpath(subprocess.run([cxx, f"-print-file-name=lib{s}.so"], capture_output=True, text=True).stdout.strip())
                    for s in ("asan", "ubsan", "tsan", "lsan")}
        env["LD_PRELOAD"] = ":".join(p for p in re.split("[: ]", env["LD_PRELOAD"]) if p and os.path.realpath(p) not in runtimes)
    return env


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_page_feed_under_sanitizers(pages, tmp_path, sanitizer):
    page_dir, batches = pages
    cxx = os.environ.get("CXX", "g++")
    env = own_env(cxx)
    exe = str(tmp_path / "page_feed_check")
    # the runtimes are linked statically: the program then runs whatever else the loader brings in before it
    static = [f"-static-lib{s}" for s in {"address,undefined": ("asan", "ubsan"), "thread": ("tsan",)}[sanitizer]]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all", *static, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(CSRC, "cli", "page_feed_check.cpp"), "-L" + LIB, "-lfocr_host", "-lpthread", "-Wl,-rpath," + LIB], check=True, env=env)
    out = tmp_path / "png"
    out.mkdir()
    cmd = [exe, str(page_dir), str(out), str(N_PAGES)] + batches
    # without -R (no address-space randomisation for this one process) g++ 11's TSan runtime exits with "unexpected memory
    # mapping" where the kernel randomises mmap by 32 bits
    if shutil.which("setarch"):
        cmd = ["setarch", platform.machine(), "-R"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
    assert r.stdout == "page feed ok\n"
    assert sorted(os.listdir(out)) == [f"p{i:02d}.png" for i in range(N_PAGES)]

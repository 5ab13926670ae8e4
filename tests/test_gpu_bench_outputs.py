"""bench.py's plain run and --dump-outputs: the line holds the headline fields and none of the --full legs, --steps sets the timed
steps, and the dumped results of the last timed step are the path's real results (page 0 against the committed golden lists),
float arrays within 64 MB, and identical from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "parity", "c3_value", "c4_stream_value", "e2e_value_incl_h2d_pipelined")


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--settle-s", "0.2", "--dump-outputs", str(out_dir), *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(out_dir):
    got = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir)) if f.endswith(".npy")}
    assert set(got) == {"counts", "matches", "lines_per_page", "chars_per_line", "chars"}, sorted(got)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()), {k: a.dtype for k, a in got.items()}
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) <= 64_000_000
    return got


def test_plain_line_and_dumped_page0_against_golden(tmp_path):
    """One context (--in-flight 1 --depth 1): every step rescans synthetic pages 0..127, so page 0 of the dump is
    tests/golden/c2_page0.npz."""
    d = _bench(tmp_path, "--steps", "7", "--warmup", "2", "--in-flight", "1", "--depth", "1")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert not [k for k in FULL_ONLY if k in d], d.keys()
    got = _load(tmp_path)
    counts = got["counts"]
    assert counts.shape == (128, 380)
    g = np.load(os.path.join(ROOT, "tests", "golden", "c2_page0.npz"))
    assert np.array_equal(counts[0], g["counts"].astype(np.float64))
    n0 = int(g["counts"].sum())
    m = got["matches"]
    assert m.shape[1] == 3
    if m.shape[0] == int(counts.sum()):  # not sampled: page 0's lists lead
        want = np.stack([g["matches"]["x"], g["matches"]["y"], g["matches"]["similarity"]], axis=1).astype(np.float32)
        assert np.array_equal(m[:n0], want)
    assert got["lines_per_page"].shape == (128,) and got["lines_per_page"].sum() == len(got["chars_per_line"])
    assert got["chars"].shape[1] == 7 and got["chars_per_line"].sum() == len(got["chars"]) > 0


def test_dumped_outputs_identical_run_to_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    da = _bench(a, "--steps", "5", "--warmup", "3")
    _bench(b, "--steps", "5", "--warmup", "3")
    assert da["steps"] == 5 and not [k for k in FULL_ONLY if k in da]
    ga, gb = _load(a), _load(b)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k

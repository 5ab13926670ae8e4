"""The runner-ups of the ncc path on the CPU: the lane-level model of the kernel's chunked top-2 merge (ncc_runners_model.model)
against the brute-force definition on every hit list the GPU test feeds the device, the definition's winners against the
reference's process_hits, and the host-side surface: `ncc --scores` and the header."""
import os
import subprocess

import numpy as np
import pytest

import focr_walk_model as W
import ncc_runners_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCC = os.path.join(ROOT, "font_ocr_amd", "bin", "ncc")
FAMILIES = {**R.FAMILIES, **W.FAMILIES}


@pytest.fixture(scope="module")
def ncc_bin():
    if not os.path.exists(NCC):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return NCC


def _small(cases):  # (the lane model is a Python loop per trip)
    return [c for c in cases if len(c.sim) < 50_000]  # the brute force is a Python loop: the 100 000-hit rows are the GPU test's


@pytest.mark.parametrize("family", list(FAMILIES))
def test_lane_model_equals_the_definition(family):
    for case in _small(FAMILIES[family]()):
        want_lines, want = R.brute_force(case)
        got_lines, got = R.model(case)
        assert got_lines == want_lines, case
        assert R.same_records(got, want) is None, (case, R.same_records(got, want))
        if case.expect_lines is not None:
            assert sum(len(p) for p in want_lines) == case.expect_lines, case


@pytest.mark.parametrize("family", list(FAMILIES))
def test_definition_winners_are_the_references(family):
    for case in _small(FAMILIES[family]()):
        assert R.brute_force(case)[0] == W.reference_lines(case), case


def test_families_hold_what_they_are_for():
    """Both kinds of record occur, groups cross chunk edges, and the odd similarities come back as runners."""
    recs = {name: np.concatenate([R.brute_force(c)[1] for c in fam()]) for name, fam in R.FAMILIES.items()}
    none = {name: r["template_index"] == R.NO_RUNNER for name, r in recs.items()}
    assert none["small_groups"].any() and not none["small_groups"].all()
    assert not none["placed_groups"].any() and set(recs["placed_groups"]["members"]) == {63, 64, 65, 127, 128, 129, 200}
    assert none["lone_overlaps"].all() and (recs["lone_overlaps"]["members"] == 1).all() and len(recs["lone_overlaps"]) > 100
    assert none["capped_others"].any() and not (recs["capped_others"]["letter"] == R._GLYPHS[R.C]).any()  # C is only ever capped there
    sp = recs["special_runners"]
    got = set(sp["similarity"][~none["special_runners"]].view(np.uint32).tolist())
    assert set(R.SPECIALS.view(np.uint32).tolist()) <= got, "an odd similarity never came back as a runner"
    real = sp[(sp["template_index"] != R.NO_RUNNER) & (sp["similarity"].view(np.uint32) == 0xFFFFFFFF)]
    assert len(real) and (real["letter"] != R.NO_RUNNER).all()
    d = R.brute_force(R.demotions()[0])[1]
    assert [int(l) for l in d["letter"][:4]] == [int(R._GLYPHS[g]) for g in (R.A, R.C, R.C, R.C)]
    assert d["similarity"][:4].tolist() == [np.float32(v) for v in (0.97, 0.98, 0.93, 0.93)]
    assert none["runner_fuzz"].any() and not none["runner_fuzz"].all() and recs["runner_fuzz"]["members"].max() > 64


def test_cli_scores_surface(ncc_bin):
    r = subprocess.run([ncc_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--scores" in r.stdout
    base = [ncc_bin, "-f", "/nonexistent.ttf", "-t", "13", "-i", "/nonexistent.pgm"]
    r = subprocess.run(base + ["--raw", "--scores", "/nonexistent-dir/s.csv"], capture_output=True, text=True)
    assert r.returncode == 2 and "--scores" in r.stderr and "--raw" in r.stderr, r.stderr  # before the font is even opened
    r = subprocess.run(base + ["--scores"], capture_output=True, text=True)
    assert r.returncode == 2 and "--scores" in r.stderr, r.stderr
    r = subprocess.run(base + ["--scores="], capture_output=True, text=True)
    assert r.returncode == 2 and "--scores" in r.stderr, r.stderr
    r = subprocess.run(base + ["--scores", "/nonexistent-dir/s.csv"], capture_output=True, text=True)
    assert r.returncode == 101, r.stderr  # accepted: the run stops at the missing font


def test_header_declares_the_runner_abi():
    text = open(os.path.join(ROOT, "include", "focr_ncc.h")).read()
    for s in ("int focr_get_runners(focr_ctx_t *ctx, focr_runner_t *out);", "int focr_last_runners(focr_ctx_t *ctx, float *ms, uint32_t *launches);",
              "#define FOCR_NO_RUNNER 0xffffffffu", "} focr_runner_t;"):
        assert s in text, s
    from font_ocr_amd.searcher import NO_RUNNER, RUNNER_DTYPE

    assert RUNNER_DTYPE == R.RUNNER_DTYPE and RUNNER_DTYPE.itemsize == 20 and NO_RUNNER == R.NO_RUNNER

"""The device's prefilter, phase by phase, against its host model and plain numpy (cases: tests/prefilter_cases.py).

The fast path is correct only if the int8 prefilter never drops a pair the reference would emit.  tests/test_prefilter_host.py proves
that bound for the host model; the parity tests compare final match lists.  Here the two are joined: per case, after one MFMA scan
with exact sizes and once more after the second, identical scan (estimated sizes),

  A  the planes say "never" (-32768) exactly where numpy says so: x = 0, y = 0, the box leaves the page, V = 0 (V in int64 from the
     page), over the whole region the scan kernel reads (x < 16 * mtx, y <= n_rows) — integer logic, no tolerance;
  B  the threshold a plane value stands for, -plane * S, is <= L64 = kq*sqrt(V) - crk*sqrt(W) in float64 from the exact integers (W
     exact, not the f32 bound) — the property the proof needs of the DEVICE.  No tolerance; exempt is the clamp value -32767 (a
     threshold no sum reaches) and, in the one case that asks for a threshold below the clamp on purpose ("clamp-lo"), +32767 (a
     threshold below every sum: S >= K / 2, so 32767 * S >= 16383 * K > 127 * 128 * K >= |G|);
  C  the device's plane equals the model's, or differs by one where the model's (L - 2) / S lies within E / S of an integer,
     E = 2^-22 * (|kq|*sqrt(V) + crk*sqrt(W)): the device's square roots are the 1-ulp instruction (2^-23 of each term), the multiply /
     fma behind them re-rounds by at most 2^-24 more.  An unexplained difference fails; the number of explained ones is printed;
  D  the candidate list is, as a set and without duplicates, {(p, y, x, t): G + (device plane << shift) > 0, t live} with the model's
     G — int8 MFMAs into int32 are exact.  Classes on the legacy kernel (int32 tables, a finer threshold: floor(L) - 2) must hold
     every emitting pair and stay inside the plane model's set with the model planes lowered by one unit;
  E  the case is not vacuous (prefilter_cases.vacuity; also checked on the CPU in tests/test_prefilter_host.py, with the kernel paths
     each case is there for: prefilter_cases.EXPECT).

Teeth, as measured on an MI355X with one-line mutations of the DEVICE code only (the model shares the inline functions of
mfma_common.h, so a mutation of both sides moves model and device together: that is caught by the numpy form of the plane value,
-floor((L - 2) / S) from the model's own L, here and in tests/test_prefilter_host.py).  "x + n_w <= r_w" -> "<" in the register form
fails A; dropped_column_W_upper without its 2^-21 term fails C (PAIR / DROP cases and "saturated"); plane_value with 1.0f * inv_S
fails C in every case that has a plane; a dead / padding template id not masked in the flush fails the scan itself, before A-D are
reached (the verify's guard meets a key outside the bank: FOCR_ERR_STATE), in ten cases; the last, partly filled item's M-tiles not
masked fails D with duplicates (case "dead").  Of the older GPU tests the first to fail were, in this order: the time-budgeted fuzz,
one random-bank parity case, test_threshold_plane_values_device_equals_host, the fuzz, the bench-output comparison.
"""
import time

import numpy as np
import pytest

import prefilter_cases as PC
from font_ocr_amd.searcher import PREFILTER_AUTO, SCAN_DIRECT, SCAN_MFMA, FocrError, Scanner

pytestmark = pytest.mark.gpu

NEVER = PC.NEVER


@pytest.fixture(scope="module")
def case_models():
    """case id -> (case, bank, pages, one model per page).  The last case is kept: its variants (statistics form, scan CUs) follow it in
    the parameter list and need no second model run.  Reports the module's wall time and the model's share of it at the end."""
    state = {"id": None, "v": None, "model_s": 0.0, "start": time.time()}

    def get(case_id):
        if state["id"] != case_id:
            t0 = time.time()
            case, bank, pages = PC.build(case_id)
            state["v"] = (case, bank, pages, [PC.model(case, bank, pg) for pg in pages])
            state["id"] = case_id
            state["model_s"] += time.time() - t0
        return state["v"]

    yield get
    print(f"\ntest_gpu_prefilter_model: {time.time() - state['start']:.1f} s of wall time, {state['model_s']:.1f} s of it the host model and building the cases")


def _check_planes(case, pages, models, dev, what):
    """A, B, C for every class that has a plane; returns {class: device plane over the page's own windows (n_pages, r_h, r_w)}."""
    n_pages, r_h, r_w = pages.shape
    Lpitch, Lrows = (r_w + 63) // 64 * 64 + 64, (r_h + 7) // 8 * 8 + 8
    one = n_pages * Lrows * Lpitch
    out, explained, compared = {}, 0, 0
    for k, c in enumerate(models[0]["classes"]):
        slot = int(c["plane_slot"])
        if slot < 0:
            continue
        n_w, n_h, kw, shift = int(c["n_w"]), int(c["n_h"]), int(c["keep_w"]), int(c["shift"])
        S, kq, crk = float(1 << shift), float(c["kq"]), float(c["crk"])
        assert dev.size >= (slot + 1) * one, (what, k, dev.size, slot, one)
        cols, rows = min(16 * int(c["mtx"]), Lpitch), int(c["n_rows"]) + 1
        pl = dev[slot * one:(slot + 1) * one].reshape(n_pages, Lrows, Lpitch)[:, :rows, :cols]
        out[k] = np.full((n_pages, r_h, r_w), NEVER, np.int16)
        out[k][:, :min(rows, r_h), :min(cols, r_w)] = pl[:, :r_h, :r_w]
        yy, xx = np.mgrid[0:rows, 0:cols]
        for p in range(n_pages):
            V, W = PC.window_sums(pages[p], n_w, n_h, kw, rows, cols)
            never = (xx == 0) | (yy == 0) | (xx + n_w > r_w) | (yy + n_h > r_h) | (V == 0)
            got_never = pl[p] == NEVER
            bad = np.argwhere(got_never != never)
            assert not len(bad), f"{what} A: class {n_w}x{n_h} page {p}: 'never' differs at (y, x) {bad[:6].tolist()}, device {pl[p][tuple(bad[:6].T)].tolist()}"
            can = ~never
            q = pl[p].astype(np.float64)
            L64 = kq * np.sqrt(V.astype(np.float64)) - crk * np.sqrt(W.astype(np.float64))
            free = can & (pl[p] != -32767)
            if case.get("vacuous_ok"):  # a threshold beyond the clamp on purpose: +32767 stands for "below every sum" (module docstring)
                free &= pl[p] != 32767
            bad = np.argwhere(free & (-q * S > L64))
            assert not len(bad), (f"{what} B: class {n_w}x{n_h} page {p}: the plane's threshold lies above L64 at (y, x) {bad[:6].tolist()}: "
                                  f"{(-q * S)[tuple(bad[:6].T)].tolist()} > {L64[tuple(bad[:6].T)].tolist()}")
            # C: against the model, on the page's own windows (elsewhere both say never: A)
            h, w = min(rows, r_h), min(cols, r_w)
            mp, Lm = models[p]["plane"][k][:h, :w].astype(np.int64), models[p]["L"][k][:h, :w].astype(np.float64)
            dp, cw = pl[p][:h, :w].astype(np.int64), can[:h, :w]
            assert np.array_equal(mp == NEVER, ~cw), f"{what}: the model's own 'never' differs from numpy's, class {n_w}x{n_h} page {p}"
            # ... and the model's plane is -floor((L - 2) / S) of its own f32 L in plain numpy: with C, that pins the device's "- 2" and unit
            # even if the shared plane_value were wrong on both sides
            with np.errstate(over="ignore", invalid="ignore"):
                ref = -np.clip(np.floor((models[p]["L"][k][:h, :w] - np.float32(2.0)).astype(np.float32) * np.float32(1.0 / S)), -32767.0, 32767.0)
            assert np.array_equal(mp[cw], ref[cw].astype(np.int64)), f"{what}: the model's plane is not -floor((L - 2) / S), class {n_w}x{n_h} page {p}"
            t = (Lm - 2.0) / S
            E = 2.0 ** -22 * (abs(kq) * np.sqrt(V[:h, :w].astype(np.float64)) + crk * np.sqrt(W[:h, :w].astype(np.float64)))
            may = np.abs(t - np.rint(t)) <= E / S
            diff = cw & (dp != mp)
            bad = np.argwhere(diff & ~(may & (np.abs(dp - mp) <= 1)))
            assert not len(bad), (f"{what} C: class {n_w}x{n_h} page {p}: device plane != model at (y, x) {bad[:6].tolist()}: device {dp[tuple(bad[:6].T)].tolist()} "
                                  f"model {mp[tuple(bad[:6].T)].tolist()} (L - 2) / S {t[tuple(bad[:6].T)].tolist()} E / S {(E / S)[tuple(bad[:6].T)].tolist()}")
            explained += int(diff.sum())
            compared += int(cw.sum())
    print(f"{what}: {explained} of {compared} plane values differ from the model by one unit next to an integer (L - 2) / S")
    return out


def _keys(a, shape):
    n_pages, r_h, r_w, T = shape
    a = a.astype(np.int64)
    return ((a[:, 0] * r_h + a[:, 1]) * r_w + a[:, 2]) * T + a[:, 3]


def _describe(keys, shape, models):
    n_pages, r_h, r_w, T = shape
    out = []
    for key in keys[:6].tolist():
        t, x, y, p = key % T, key // T % r_w, key // T // r_w % r_h, key // T // r_w // r_h
        out.append(dict(page=p, y=y, x=x, t=t, m_tile=x // 16, n_tile=int(models[0]["templates"][t, 3]), G=int(models[p]["G"][t, y, x])))
    return out


def _check_candidates(case, bank, pages, models, planes_dev, cand, n_counter, what):
    """D."""
    n_pages, r_h, r_w = pages.shape
    shape = (n_pages, r_h, r_w, len(bank))
    assert len(cand) == n_counter, (what, len(cand), n_counter)
    assert (cand[:, 0] < n_pages).all() and (cand[:, 1] < r_h).all() and (cand[:, 2] < r_w).all() and (cand[:, 3] < len(bank)).all(), what
    got = _keys(cand, shape)
    uniq, counts = np.unique(got, return_counts=True)
    assert len(uniq) == len(got), f"{what} D: duplicates in the device's list: {_describe(uniq[counts > 1], shape, models)}"
    exact, lower, upper = [], [], []  # plane classes: the set itself; legacy classes: what it must hold and what must hold it
    legacy_t = np.zeros(len(bank), bool)
    for t in range(len(bank)):
        if not models[0]["templates"][t, 2]:
            continue
        k = int(models[0]["templates"][t, 0])
        shift = int(models[0]["classes"][k]["shift"])
        for p in range(n_pages):
            G = models[p]["G"][t].astype(np.int64)
            fits = G != np.iinfo(np.int32).min
            base = (p * r_h * r_w + np.arange(r_h * r_w, dtype=np.int64).reshape(r_h, r_w)) * len(bank) + t
            if k in planes_dev:
                exact.append(base[fits & (G + (planes_dev[k][p].astype(np.int64) << shift) > 0)])
            else:
                legacy_t[t] = True
                mp = models[p]["plane"][k].astype(np.int64)
                with np.errstate(invalid="ignore"):
                    lower.append(base[models[p]["sim"][t] > case["thr"]])
                upper.append(base[fits & (mp != NEVER) & (G + ((mp + 1) << shift) > 0)])
    cat = lambda parts: np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
    exact, lower, upper = cat(exact), cat(lower), cat(upper)
    got_plane, got_legacy = np.sort(got[~legacy_t[cand[:, 3]]]), np.sort(got[legacy_t[cand[:, 3]]])
    lost, extra = np.setdiff1d(exact, got_plane), np.setdiff1d(got_plane, exact)
    assert not len(lost) and not len(extra), (f"{what} D: {len(lost)} pairs of the model's set are missing from the device's list: {_describe(lost, shape, models)}; "
                                              f"{len(extra)} of the device's are not in the model's set: {_describe(extra, shape, models)}")
    lost, extra = np.setdiff1d(lower, got_legacy), np.setdiff1d(got_legacy, upper)
    assert not len(lost) and not len(extra), (f"{what} D (legacy kernel): {len(lost)} emitting pairs are missing: {_describe(lost, shape, models)}; {len(extra)} candidates lie "
                                              f"outside the plane model's set lowered by one unit: {_describe(extra, shape, models)}")
    print(f"{what}: {len(got_plane)} candidates equal the model's set; legacy kernel: {len(lower)} <= {len(got_legacy)} <= {len(upper)}")
    return set(got.tolist())


VARIANTS = [(cid, 0, 0) for cid in PC.CASES]
# the LDS-tiled statistics for classes that otherwise take the register form (plain, DROP, PAIR at kept widths 8 and 12; 4 and 16)
VARIANTS += [(cid, 1, 0) for cid in ("w8-ksteps", "w16-ksteps", "w12-four", "drop9", "drop13", "drop9-tall", "pair9-tall", "pair9", "pair13", "saturated", "bench")]
VARIANTS += [("pair9", 0, 32)]  # the scan kernel on 32 CUs: other workgroups, the same set
VARIANTS.sort(key=lambda v: list(PC.CASES).index(v[0]))


@pytest.mark.parametrize("case_id,form,cus", VARIANTS, ids=[f"{c}{'-lds' if f else ''}{'-cus32' if u else ''}" for c, f, u in VARIANTS])
def test_device_prefilter_equals_its_model(case_models, case_id, form, cus):
    case, bank, pages, models = case_models(case_id)
    v = PC.vacuity(case, bank, pages, models)
    print(case_id, v)
    assert v["missed"] == 0
    if not case.get("vacuous_ok"):  # E (thresholds beyond the clamp have no pair near the threshold: nothing or everything passes)
        assert v["emit"] > 0 and v["cand_no_emit"] > 0 and v["near"] > 0 and v["blank_tiles"] > 0 and v["live_tiles"] > 0, v
    sets = []
    with Scanner(0) as sc:
        sc.set_column_drop(case.get("drop", True))
        sc.set_prefilter(case.get("prefilter", PREFILTER_AUTO))
        sc.set_stats_form(form)
        sc.set_scan_cus(cus)
        sc.set_bank(bank)
        sc.set_pages(pages, invert=False)
        for which in ("exact sizes", "estimated sizes"):
            what = f"{case_id} form {form} cus {cus}, {which}"
            sc.scan(case["thr"], 1024, SCAN_MFMA)
            cand = sc.candidates()
            planes_dev = _check_planes(case, pages, models, sc.planes(), what)
            sets.append(_check_candidates(case, bank, pages, models, planes_dev, cand, sc.counters()["candidates"], what))
        assert sc.size_estimate_stats()["redone"] == 0  # the second scan did run on estimates
    assert sets[0] == sets[1]
    if case_id in PC.ODD_MTILES:  # the last item of a pass is not full: from the device's own planes, an M-tile is live if a window of it can emit
        live = _live_mtiles(models, planes_dev)
        print(f"{case_id}: live M-tiles per pass {live}")
        assert any(n % 4 for n in live), live


def _live_mtiles(models, planes_dev):
    per_pass = {}
    for k, pl in planes_dev.items():
        su = int(models[0]["classes"][k]["super"])
        per_pass[su] = per_pass.get(su, False) | (pl != NEVER)
    out = []
    for su in sorted(per_pass):
        some = per_pass[su]
        pad = np.zeros(some.shape[:2] + ((some.shape[2] + 15) // 16 * 16,), bool)
        pad[:, :, : some.shape[2]] = some
        out.append(int(pad.reshape(pad.shape[0], pad.shape[1], -1, 16).any(3).sum()))
    return out


def test_candidates_hook_refuses_where_the_list_is_gone(case_models):
    """focr_debug_candidates after anything but a whole-batch MFMA scan with the hits-first tail: FOCR_ERR_STATE, never stale keys."""
    case, bank, pages, _ = case_models("drop9")
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(pages, invert=False)
        with pytest.raises(FocrError, match="no scan results"):
            sc.candidates()
        sc.scan(case["thr"], 1024, SCAN_MFMA)
        want = sc.candidates()
        assert len(want) == sc.counters()["candidates"] > 0
        sc.scan(case["thr"], 1024, SCAN_DIRECT)
        with pytest.raises(FocrError, match="not an MFMA scan"):
            sc.candidates()
        sc.set_row_tail(False)
        sc.scan(case["thr"], 1024, SCAN_MFMA)
        with pytest.raises(FocrError, match="legacy tail"):
            sc.candidates()
        sc.set_row_tail(True)
        sc.force_split(True)
        sc.scan(case["thr"], 1024, SCAN_MFMA)
        with pytest.raises(FocrError, match="split batch"):
            sc.candidates()
        sc.force_split(False)
        sc.scan(case["thr"], 1024, SCAN_MFMA)
        got = sc.candidates()
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist()))
        sc.debug_process_hits([0], [1], [1], [0], [0.9], [1])
        with pytest.raises(FocrError, match="focr_debug_process_hits"):
            sc.candidates()

"""The cases of tests/exact_cases.py have the properties they are there for, by the oracle alone (no device), set by set and seed by seed: a
match in every searchable size class, an emitted window whose s_n * s_p needs more than 32 bits, windows skipped by each rule of the Rust
scan, a zero denominator, no full buffer — and the oracle of the Rust arithmetic is held against a second witness in plain Python."""
import numpy as np
import pytest

import exact_cases as EC
from oracle import oracle as O

IDS = sorted(EC.SETS)
LOW = min(EC.THRESHOLDS)


def _t32(thr):
    return float(np.float32(thr))


@pytest.mark.parametrize("set_id", IDS)
def test_set_has_its_templates_pages_and_matches(set_id):
    shapes, per, geom = EC.SETS[set_id]
    bank, luma, info = EC.build(set_id)
    assert luma.shape == geom and len(bank) == (sum(per) if isinstance(per, list) else per * len(shapes))
    assert not bank.needle(info["zero"]).any()
    c = bank.needle(info["const"])
    assert c.min() == c.max() != 0
    for t in info["first"]:
        assert bank.needle(t).size == 1 or bank.needle(t).min() != bank.needle(t).max()
    ink = [O.invert(pg) for pg in luma]
    for t, y, x in info["planted"]:
        nd = bank.needle(t)
        assert np.array_equal(ink[0][y:y + nd.shape[0], x:x + nd.shape[1]], nd)
    a, b = EC.bands(geom[2])
    assert not ink[1][:, a:b].any() and (ink[1][:, b + 1:geom[2] - 1] == 255).all() and ink[1][:, :a].any() and ink[1][:, -1].any()
    assert geom[2] - 1 - b >= max(w for w, h in shapes) + 1  # every width has uniform windows (and the narrowest, at least, windows of paper alone)
    # at least one emitted match per searchable size class, in both arithmetics (a template of one pixel has no variance: it never emits);
    # the planted templates are found as themselves
    for lists in (EC.oracle_c(set_id, LOW), EC.oracle_rust(set_id, LOW)):
        for k, shape in enumerate(shapes):
            members = [t for t in range(len(bank)) if (int(bank.templates[t]["n_w"]), int(bank.templates[t]["n_h"])) == shape]
            n = sum(len(lists[p][t]) for p in range(geom[0]) for t in members)
            assert (n > 0) == (EC.searchable(shape, geom) and shape != (1, 1)), (shape, n)
    for lists in (EC.oracle_c(set_id, 0.9), EC.oracle_rust(set_id, 0.9)):
        for t, y, x in info["planted"]:
            if bank.needle(t).size == 1:
                continue
            m = lists[0][t]
            hit = m[(m["x"] == x) & (m["y"] == y)]
            assert len(hit) == 1 and hit[0]["similarity"] > 0.9999, (t, y, x)
    # the zero and the constant template never emit in either arithmetic
    for thr in EC.THRESHOLDS:
        for lists in (EC.oracle_c(set_id, thr), EC.oracle_rust(set_id, thr)):
            assert all(len(lists[p][t]) == 0 for p in range(geom[0]) for t in (info["zero"], info["const"]))
    # the C lists reach the reference's cap at the low threshold (it is part of what they are); the Rust lists run past it
    if set_id in ("w16", "w8", "w12"):
        assert max(len(m) for pl in EC.oracle_c(set_id, LOW) for m in pl) == EC.CAP_C
        assert max(len(m) for pl in EC.oracle_rust(set_id, LOW) for m in pl) > EC.CAP_C
    assert max(len(m) for thr in EC.THRESHOLDS for pl in EC.oracle_rust(set_id, thr) for m in pl) < EC.CAP_RUST


@pytest.mark.parametrize("set_id", IDS)
def test_rust_oracle_equals_the_python_witness_and_shows_the_sets_properties(set_id):
    bank, luma, info = EC.build(set_id)
    seen = dict(sp0=0, neg=0, sn0=0, den0=0, u64=0)
    for p in range(len(luma)):
        ink, _, se = EC._page_tables(set_id, p)
        for t in EC.witness_templates(set_id):
            nd = bank.needle(t)
            shape = (nd.shape[1], nd.shape[0])
            if not EC.searchable(shape, EC.SETS[set_id][2]):
                continue
            cand, skipped = EC.rust_witness(ink, nd, se[shape])
            for k, v in skipped.items():
                seen[k] += v
            for thr in EC.THRESHOLDS:
                want = EC.oracle_rust(set_id, thr)[p][t]
                got = [c for c in cand if c[2] > _t32(thr)]
                assert [(c[0], c[1]) for c in got] == list(zip(want["x"].tolist(), want["y"].tolist())), (p, t, thr)
                assert np.array([c[2] for c in got], np.float64).astype(np.float32).tobytes() == want["similarity"].tobytes(), (p, t, thr)
                if thr == LOW:
                    seen["u64"] += sum(1 for c in got if c[3] >= 1 << 32)
    for prop in EC.PROPS[set_id]:
        assert seen[prop] > 0, (prop, seen)
    if "u64" in EC.PROPS[set_id]:
        assert info["heavy"]


@pytest.mark.parametrize("set_id", IDS)
def test_per_template_rust_oracle_equals_the_page_loop_up_to_16_px(set_id):
    """O.search_rust_u8 template by template == O.scan_page_rust (which stops at 16 px like the reference's dispatch)."""
    bank, luma, _ = EC.build(set_id)
    for thr in EC.THRESHOLDS:
        lists = EC.oracle_rust(set_id, thr)
        for p in range(len(luma)):
            counts, m = O.scan_page_rust(O.invert(luma[p]), bank, thr, cap=EC.CAP_RUST)
            for t in range(len(bank)):
                if bank.templates[t]["n_w"] <= 16:
                    assert m[t, : counts[t]].tobytes() == lists[p][t].tobytes(), (thr, p, t)
                else:
                    assert counts[t] == 0


def test_the_sets_launch_every_kernel_they_are_there_for():
    every = set().union(*(EC.launches(k) for k in IDS))
    assert {"scan_tall_kernel<1>", "scan_tall_kernel<7>", "scan_tall_kernel<8>"} <= every
    assert {f"scan_direct_kernel<{n},{m}>" for n in (1, 2, 3, 4) for m in (16, 32)} <= every
    assert EC.launches("tall1") == {"scan_tall_kernel<1>", "scan_direct_kernel<1,16>"}
    assert EC.launches("tall7") == {"scan_tall_kernel<7>"}
    assert EC.launches("h255") == {"scan_tall_kernel<8>", "scan_tall_kernel<1>"}
    assert EC.launches("tallest") == {"scan_tall_kernel<2>"}  # 70 rows never fit a page of 61
    # TALL_TC = 8 templates per pass of the tall kernel: one full pass, a tail of one, two full passes
    tall_counts = set()
    for k in ("tall1", "tall7", "h255"):
        shapes, per, _ = EC.SETS[k]
        tall_counts |= {n for (w, h), n in zip(shapes, per) if h > 32 or w > 16}
    assert {8, 9, 16} <= tall_counts


def test_h255_holds_the_largest_dot_product():
    bank, luma, info = EC.build("h255")
    (t,) = info["heavy"]
    ink, _, se = EC._page_tables("h255", 1)
    acc, sp, s2p = EC.window_ints(ink, bank.needle(t))
    b = EC.bands(40)[1]
    assert int(acc.max()) == 255 * (255 * 8159 + 254) == 530_603_745 < 530_604_000 < 1 << 31  # a saturated window under the changed template
    assert int(sp.max()) == 255 * 8160 and int(s2p.max()) == 255 * 255 * 8160 < 1 << 32        # s2_p fits the kernel's 32-bit accumulator
    assert np.array_equal(ink[5:260, b:b + 32], bank.needle(t))                                 # and the window that is the template
    assert int(EC.window_ints(ink, bank.needle(info["const"]))[0].max()) == 530_604_000          # all 255 under all 255: what the kernel must hold
    m = EC.oracle_rust("h255", 0.9)[1][t]
    assert len(m) == 1 and (int(m[0]["x"]), int(m[0]["y"])) == (b, 5)

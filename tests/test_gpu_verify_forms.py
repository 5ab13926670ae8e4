"""The forms of the row tail's exact verify that no other test names, each on the smallest bank that takes it (the host's plan:
csrc/hip/verify_plan.h; its edges without a device: test_verify_plan_host.py): the 16-byte rows staged whole in LDS, the chunk passes
with 16- and with 12-byte rows, the template rows read from global memory.  Per case: two noise pages of 96 x 64 with a dozen templates
planted — eight as they are, four blended with noise down to a similarity just below the threshold, which the prefilter passes and the
verify must reject — scanned at 0.3 with exact and then with estimated sizes; both scans took the form the case names
(focr_debug_tail_path) and equal the exact scan (SCAN_DIRECT) on the same context bit for bit: offsets, match lists (x, y, f32 bits,
order), counts."""
import numpy as np
import pytest

from font_ocr_amd.searcher import Scanner
from verify_cases import noise_bank, noise_pages, scan_all

pytestmark = pytest.mark.gpu

THR = 0.3
SHAPE = (2, 64, 96)
# id: (classes [(n_w, n_h, templates)], tail_path()["verify"], ["verify_chunks"])
CASES = {
    "lds16": ([(14, 10, 4), (16, 12, 4)], "lds16", 0),
    "chunks-16B-2": ([(16, 32, 272)], "chunks", 2),   # 237 + 35 templates
    "chunks-12B-1": ([(12, 32, 272)], "chunks", 1),
    "global": ([(16, 32, 3793)], "global", 0),        # one template more than 16 chunks hold
}


def _ncc(window, needle):
    a, b = window.astype(np.float64).ravel(), needle.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


def _near_miss(needle, rng, target):
    """The needle blended with noise so that its similarity to the needle lies in (target - 0.004, target]: bisection on the blend."""
    noise = rng.integers(0, 256, needle.shape).astype(np.float64)
    lo, hi = 0.0, 1.0  # the similarity grows with the needle's share
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        w = np.clip(np.rint(mid * needle + (1.0 - mid) * noise), 0, 255).astype(np.uint8)
        if _ncc(w, needle) > target:
            hi = mid
        else:
            lo = mid
    w = np.clip(np.rint(lo * needle + (1.0 - lo) * noise), 0, 255).astype(np.uint8)
    assert target - 0.004 < _ncc(w, needle) <= target, _ncc(w, needle)
    return w


@pytest.mark.parametrize("case_id", sorted(CASES))
def test_form_equals_the_exact_scan(case_id):
    classes, form, chunks = CASES[case_id]
    bank = noise_bank(classes, 500 + len(case_id))
    T = len(bank)
    rng = np.random.default_rng(600 + len(case_id))
    # every template at most 16 x 32: five columns, the first and the last searched row of the tallest, two pages.  Planted: the first and the
    # last template and both sides of the 16-byte chunks' boundary (237), the rest anywhere (a bank of eight: each once, four of them twice)
    if T > 12:
        ts = list(dict.fromkeys([0, T - 1, 236, 237] + rng.choice(T, 12, replace=False).tolist()))[:12]
    else:
        ts = (list(range(T)) * 2)[:12]
    places = [(p, y, 1 + 18 * i) for p in range(2) for y in (1, 32) for i in range(5)]
    plants = [(t, *places[k]) for k, t in enumerate(ts)]
    ink = noise_pages(bank, SHAPE, 700 + len(case_id), plants[:8])
    for (t, p, y, x), target in zip(plants[8:], (0.299, 0.297, 0.294, 0.29)):
        nd = bank.needle(t)
        ink[p, y:y + nd.shape[0], x:x + nd.shape[1]] = _near_miss(nd, rng, target)
    with Scanner(0) as sc:
        sc.set_bank(bank)
        sc.set_pages(ink, invert=False)
        m, cands = scan_all(sc, THR, ((0, form),), case_id, chunks)  # (the candidate set: as many as counters()["candidates"] said, scan by scan)
    hits = len(m)
    assert hits >= 8, hits                        # every template planted as it is
    assert len(cands) > hits, (len(cands), hits)  # ... and the verify rejected something: the comparison is not an empty one
    planted = {(p, y, x, t) for t, p, y, x in plants[:8]}
    assert planted <= cands, planted - cands

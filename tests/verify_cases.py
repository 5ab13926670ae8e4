"""What the tests of the exact verify's forms share (test_gpu_verify_w89.py, test_gpu_verify_forms.py): banks of noise templates, noise
pages with templates planted, and the comparison of every MFMA scan of a context with the exact scan on the same pages."""
import numpy as np

import prefilter_cases as PC
from font_ocr_amd.searcher import SCAN_DIRECT, SCAN_MFMA

CAP = 1024


def noise_bank(classes, seed):
    """[(n_w, n_h, templates)] -> a bank of noise templates, the classes interleaved."""
    rng = np.random.default_rng(seed)
    needles = []
    for n_w, n_h, count in classes:
        for _ in range(count):
            nd = rng.integers(0, 256, (n_h, n_w), dtype=np.uint8)
            nd[0, 0], nd[-1, -1] = 255, 0  # never constant
            needles.append(nd)
    return PC.bank_of([needles[i] for i in rng.permutation(len(needles))])


def noise_pages(bank, shape, seed, plants):
    """Half-empty noise with the bank's templates planted at (t, page, y, x)."""
    rng = np.random.default_rng(seed)
    ink = rng.integers(0, 256, shape, dtype=np.uint8)
    ink[rng.random(shape) < 0.5] = 0
    for t, p, y, x in plants:
        nd = bank.needle(t)
        ink[p, y:y + nd.shape[0], x:x + nd.shape[1]] = nd
    return ink


def result(sc):
    offsets, m = sc.matches()
    return offsets.tobytes(), m.tobytes(), sc.counts().tobytes()


def cand_set(sc):
    cand = sc.candidates()
    assert len(cand) == sc.counters()["candidates"]
    keys = set(map(tuple, cand.tolist()))
    assert len(keys) == len(cand), "duplicates in the candidate list"
    return keys


def scan_all(sc, thr, forms, what, chunks=0):
    """Every (set_verify_form argument, expected tail_path()["verify"]) of `forms` on one context (exact sizes, then estimated), then the exact
    scan: all results equal, bit for bit, and all candidate sets equal.  Returns (the direct scan's matches, the candidate set)."""
    results, cands = [], []
    for form, name in forms:
        sc.set_verify_form(form)
        for which in ("exact sizes", "estimated sizes"):
            sc.scan(thr, CAP, SCAN_MFMA)
            tp = sc.tail_path()
            assert tp["tail"] == "rows" and tp["verify"] == name and tp["verify_chunks"] == chunks, (what, form, which, tp)
            results.append(result(sc))
            cands.append(cand_set(sc))
    sc.set_verify_form(0)
    sc.scan(thr, CAP, SCAN_DIRECT)
    direct = result(sc)
    for i, r in enumerate(results):
        assert r == direct, f"{what}: scan {i} (verify form {forms[i // 2][0]}, {'estimated' if i % 2 else 'exact'} sizes) differs from the exact scan"
    assert all(c == cands[0] for c in cands), (what, [len(c) for c in cands])
    return sc.matches()[1], cands[0]

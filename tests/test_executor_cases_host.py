"""The batches of tests/executor_cases.py are what their names say: proved here on the oracle alone, without a device, so that the GPU
tests of the executor's host results (tests/test_gpu_host_results.py) stand on conditions, not on what the library happens to return.
A change to synth_pages or to a seed that breaks one of them fails here first."""
import numpy as np
import pytest

import executor_cases as EC
from font_ocr_amd.bank import HIT_DTYPE

KINDS = ("text", "blank", "no-lines", "one-blank-page", "small", "big", "sparse", "dense", "cap1", "odd-width", "dword-width")


@pytest.fixture(scope="module")
def built():
    return EC.all_expected()


def test_every_kind_is_there(built):
    _, cases, exp = built
    assert set(cases) == set(exp) == set(KINDS)


def test_every_condition_holds_on_the_oracle(built):
    _, cases, exp = built
    results = EC.conditions(cases, exp)
    assert len(results) >= 10 + len(KINDS)
    failed = [(name, detail) for name, ok, detail in results if not ok]
    assert not failed, failed


@pytest.mark.parametrize("name", KINDS)
def test_expected_records_are_well_formed(built, name):
    """The expectation has the layout of focr_host_results_t: CSR offsets that end at the totals, characters inside their page
    and carrying their template's size and letter, lines in one page row, ascending in x."""
    bk, cases, exp = built
    e, pages = exp[name], cases[name]["pages"]
    assert e.counts.shape == (pages.shape[0], len(bk)) and e.counts.dtype == np.uint32
    assert e.n_matches == sum(len(h) for h in e.hits) and e.counts.max(initial=0) <= cases[name]["cap"]
    assert e.chars.dtype == HIT_DTYPE and e.page_line_off.dtype == e.line_char_off.dtype == np.uint64
    assert len(e.page_line_off) == e.n_pages + 1 and len(e.line_char_off) == e.n_lines + 1
    assert e.page_line_off[0] == 0 and e.page_line_off[-1] == e.n_lines and e.line_char_off[0] == 0 and e.line_char_off[-1] == e.n_chars
    assert np.all(np.diff(e.page_line_off.astype(np.int64)) >= 0) and np.all(np.diff(e.line_char_off.astype(np.int64)) > 0)
    t = e.chars["template_index"].astype(np.int64)
    assert np.all(t < len(bk))
    for f, g in (("w", "n_w"), ("h", "n_h"), ("letter", "letter")):
        assert np.array_equal(e.chars[f], bk.templates[g][t])
    assert np.all(e.chars["x"].astype(np.int64) + e.chars["w"] <= pages.shape[2]) and np.all(e.chars["y"].astype(np.int64) + e.chars["h"] <= pages.shape[1])
    for k in range(e.n_lines):
        line = e.chars[int(e.line_char_off[k]): int(e.line_char_off[k + 1])]
        assert len(set(line["y"].tolist())) == 1 and np.all(np.diff(line["x"].astype(np.int64)) > 0)


def test_without_process_hits_only_counts_are_expected(built):
    bk, cases, exp = built
    e = EC.expected(cases["text"], bk, post=False)
    assert e.page_line_off is None and e.line_char_off is None and e.chars is None and e.n_lines == e.n_chars == 0
    assert np.array_equal(e.counts, exp["text"].counts) and e.n_matches > 0

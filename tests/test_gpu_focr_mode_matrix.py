"""The focr decoder under every combination of its eight settings, and after the call sequences of tests/focr_mode_matrix.py,
against tests/golden/focr_mode_matrix.json: the walk of the commit before the host side resolved its settings in one place
(tools/record_focr_modes.py; the file names the commit).  Return codes, launch counts, every getter's answer, the verify's
sums and every refusal's message, byte for byte, are that commit's: the refactor changed none of them."""
import json
import os

import pytest

import focr_mode_matrix as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focr_mode_matrix.json")


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_is_whole(table):
    """Host only: the table loads, holds every combination and every sequence, and every refusal is focr_decoder_run's."""
    records = table["records"]
    assert len(table["commit"]) == 40
    assert len(records) == M.N_COMBINATIONS + M.N_SEQUENCES == 256 + 13
    assert len({r["name"] for r in records}) == len(records)
    refused = [r for r in records if r.get("rc", 0) != 0]
    assert len(refused) > 200 and all(r["error"].startswith("focr_decoder_run: ") and r["launches"] == 0 and r["n_lines"] == 0 for r in refused)
    accepted = [r for r in records[: M.N_COMBINATIONS] if r["rc"] == 0]
    assert len(accepted) == 11 and all(r["launches"] == 3 and r["n_lines"] > 0 for r in accepted)


@pytest.mark.gpu
def test_every_record_is_the_recorded_one(table):
    want = table["records"]
    got = json.loads(json.dumps(M.walk()))  # as the table was written: tuples are lists
    assert len(got) == len(want) == M.N_COMBINATIONS + M.N_SEQUENCES
    for g, w in zip(got, want):
        assert g == w, w["name"]

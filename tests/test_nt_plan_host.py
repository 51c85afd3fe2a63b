"""The NT convolution planner's answers (which kernel, how many K splits, how many statistics row blocks, how much split-K scratch) against
tests/golden/nt_plan_table.npz, recorded by tests/make_nt_plan_golden.py over the same enumeration.  The Python engines size buffers and
label the roofline from these queries, and the launches take the same decisions: a change of any answer is a change of behaviour.  Host
only: the queries are pure host code."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import make_nt_plan_golden as mk


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "nt_plan_table.npz")))


@pytest.fixture(scope="module")
def got():
    return mk.compute()


def test_fixture_covers_every_path(gold):
    """a shrunken grid cannot hide a path: every label code, fused and unfused statistics, split and unsplit scratch sizes occur"""
    assert gold["auto_ws"].shape == (len(mk.auto_cases()),) and gold["hint_tile"].shape == (len(mk.hint_cases()),)
    labels = np.concatenate([gold[k].ravel() for k in ("auto_tile", "hint_tile", "hint_tile_ep")])
    missing = set(mk.CODES) - mk.codes_of(labels)
    assert not missing, sorted(missing)
    assert {16, 32, 64, 128, 131, 132, 135, 147, 151, 152} <= mk.codes_of(gold["auto_tile"])
    assert {148, 149, 150} <= mk.codes_of(gold["hint_tile"]) and -1 in mk.codes_of(gold["hint_tile"])
    for key in ("auto_ws", "auto_stat", "hint_stat"):
        assert (gold[key] == 0).any() and (gold[key] > 0).any(), key
    assert os.path.getsize(os.path.join(GOLDEN, "nt_plan_table.npz")) < 200 * 1000


@pytest.mark.parametrize("key", ["auto_ws", "auto_tile", "auto_stat", "hint_tile", "hint_tile_ep", "hint_stat"])
def test_planner_answers_are_the_recorded_ones(gold, got, key):
    want, have = gold[key], got[key]
    assert want.shape == have.shape and want.dtype == have.dtype
    diff = np.argwhere(want != have)
    if diff.size:
        idx = tuple(diff[0])
        case = (mk.auto_cases() if key.startswith("auto") else mk.hint_cases())[idx[0]]
        scratch = idx[1] if len(idx) > 1 else None
        pytest.fail(f"{key}: {len(diff)} of {want.size} answers differ; first: {mk.describe(case, scratch)} -> (expected {want[idx]}, got {have[idx]})")

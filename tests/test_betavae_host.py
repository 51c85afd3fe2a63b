"""Host side of the BetaVAE score (ead-gan_amd/score.py): beta_vae_plan against the plans BetVAE.py's load_data / evaluate() drew, recorded
in tests/golden/score_betavae_{dsprites,colored}.npz by tests/make_betavae_golden.py, and the argument errors that need no GPU."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import score_data as sd

KINDS = ("dsprites", "colored")


def eg():
    return importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_betavae_{kind}.npz"))


@pytest.mark.parametrize("kind", KINDS)
def test_beta_vae_plan_is_the_reference_plan(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.SMALL_SIZES))
    rng = np.random.RandomState(int(g["seed"]))
    plan = eg().score.beta_vae_plan(sd.SMALL_SIZES, N, colored, rng=rng)
    assert set(plan) == ({"group_idx", "labels", "group_gains"} if colored else {"group_idx", "labels"})
    assert plan["group_idx"].shape == (500, 100) and np.array_equal(plan["group_idx"], g["bv_group_idx"].astype(np.int64))
    assert np.array_equal(plan["labels"], g["bv_labels"].astype(np.int64))
    if colored:
        n = int(g["bv_groups"])
        assert plan["group_gains"].shape == (500, 100, 3) and np.array_equal(plan["group_gains"][:n], g["bv_group_gains"])
    else:
        # the permutation the script draws and never uses is consumed: the stream stands where the script's stands
        assert rng.uniform() == float(g["bv_plan_next"])


@pytest.mark.parametrize("kind", KINDS)
def test_beta_vae_plan_at_the_archive_sizes(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.FULL_SIZES))
    np.random.seed(int(g["full_seed"]))                                     # the global stream, as the scripts use it
    plan = eg().score.beta_vae_plan(sd.FULL_SIZES, N, colored)
    assert np.array_equal(plan["labels"], g["full_labels"].astype(np.int64))
    assert np.array_equal(plan["group_idx"][:4], g["full_group_idx_head"].astype(np.int64))
    assert sd.digest(plan["group_idx"]) == str(g["full_group_idx_sha256"])
    assert plan["group_idx"].min() >= 0 and plan["group_idx"].max() < N
    if colored:
        assert np.array_equal(plan["group_gains"][:2], g["full_group_gains_head"])
        assert sd.digest(plan["group_gains"]) == str(g["full_group_gains_sha256"])
    assert np.random.uniform() == float(g["full_plan_next"])


def test_colored_gains_are_not_the_factor_vae_plans():
    """FactorVAE's evaluate() draws the eval set's gains first; BetaVAE's has no eval set, so the same seed gives other group gains"""
    s = eg().score
    N = int(np.prod(sd.SMALL_SIZES))
    b = s.beta_vae_plan(sd.SMALL_SIZES, N, True, rng=np.random.RandomState(3), L=10, M=7)
    f = s.factor_vae_plan(sd.SMALL_SIZES, N, True, rng=np.random.RandomState(3), L=10, M=7)
    assert np.array_equal(b["group_idx"], f["group_idx"]) and np.array_equal(b["labels"], f["labels"])
    assert b["group_gains"].shape == f["group_gains"].shape == (7, 10, 3)
    assert not np.array_equal(b["group_gains"], f["group_gains"])
    k = f["eval_gains"].size                                               # both streams stand behind the permutation: the same draws
    assert np.array_equal(b["group_gains"].reshape(-1)[:k], f["eval_gains"].reshape(-1))


def test_value_errors():
    """raised before the first launch: host tensors reach them"""
    s = eg().score
    with pytest.raises(ValueError, match="metric must be 'mig', 'factor_vae' or 'beta_vae'"):
        s.run_score("dsprites", "sap", "none.npz", "none.pt", "none.pt")
    rows = torch.zeros(6 * 4, 5, dtype=torch.float64)
    with pytest.raises(ValueError, match="at least 3"):
        s.beta_vae(rows, [0, 1, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="at least 3"):
        s.beta_vae_fit(rows, [2, 2, 2, 2, 2, 2])
    odd = torch.zeros(6 * 3, 5, dtype=torch.float64)
    with pytest.raises(ValueError, match="odd"):
        s.beta_vae(odd, [0, 1, 2, 0, 1, 2])

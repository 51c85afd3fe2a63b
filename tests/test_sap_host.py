"""Host side of the SAP score (ead-gan_amd/score.py): sap_plan / sap_latents against what SAP.py's load_data / evaluate() drew, recorded in
tests/golden/score_sap_{dsprites,colored}.npz by tests/make_sap_golden.py, the fixture's own consistency, and the argument errors that
need no GPU."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import score_data as sd

KINDS = ("dsprites", "colored")
LATENTS_NAMES = ("color", "shape", "scale", "orientation", "posX", "posY")
SVC_C = 0.01


def eg():
    return importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_sap_{kind}.npz"))


def possible_values(sizes):
    _, lv = sd.latents_grid(sizes)
    return {name: np.unique(lv[:, j]) for j, name in enumerate(LATENTS_NAMES)}


@pytest.mark.parametrize("kind", KINDS)
def test_sap_plan_is_the_reference_plan(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.SMALL_SIZES))
    s = eg().score
    rng = np.random.RandomState(int(g["seed"]))
    plan = s.sap_plan(sd.SMALL_SIZES, N, colored, rng=rng)
    assert set(plan) == {"latent_ids", "idx", "gains"}
    assert plan["idx"].shape == (N // 10,) and plan["idx"].dtype == np.int64 and np.array_equal(plan["idx"], g["sap_idx"].astype(np.int64))
    assert plan["latent_ids"].shape == (N // 10, 6) and not plan["latent_ids"][:, 0].any()
    assert np.array_equal(plan["latent_ids"][:, 1:], g["sap_latent_ids"].astype(np.int64))      # load_data keeps them without the color column
    if colored:
        assert plan["gains"].shape == (N // 10, 3) and np.array_equal(plan["gains"], g["sap_gains"])
    else:
        assert plan["gains"] is None
    # the group loop and the permutation the script draws and never uses are consumed: the stream stands where the script's stands
    assert rng.uniform() == float(g["sap_plan_next"])
    latents = s.sap_latents(plan["latent_ids"], LATENTS_NAMES, possible_values(sd.SMALL_SIZES))
    assert latents.shape == (N // 10, 5) and latents.dtype == np.float64 and np.array_equal(latents, g["sap_latents"])
    assert set(np.unique(latents[:, 0])) == {0.0, 1.0, 2.0}                          # shape minus 1


@pytest.mark.parametrize("kind", KINDS)
def test_sap_plan_at_the_archive_sizes(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.FULL_SIZES))
    s = eg().score
    np.random.seed(int(g["full_seed"]))                                     # the global stream, as the scripts use it
    plan = s.sap_plan(sd.FULL_SIZES, N, colored)
    assert plan["idx"].size == int(g["full_n"]) == 73728
    assert np.array_equal(plan["idx"][:64], g["full_idx_head"].astype(np.int64))
    assert sd.digest(plan["idx"]) == str(g["full_idx_sha256"])
    assert sd.digest(plan["latent_ids"][:, 1:]) == str(g["full_latent_ids_sha256"])     # load_data keeps the ids without the color column
    assert plan["idx"].min() >= 0 and plan["idx"].max() < N
    if colored:
        assert np.array_equal(plan["gains"][:8], g["full_gains_head"])
        assert sd.digest(plan["gains"]) == str(g["full_gains_sha256"])
    assert np.random.uniform() == float(g["full_plan_next"])
    latents = s.sap_latents(plan["latent_ids"], LATENTS_NAMES, possible_values(sd.FULL_SIZES))
    assert np.array_equal(latents[:8], g["full_latents_head"]) and sd.digest(latents) == str(g["full_latents_sha256"])


def test_sap_plan_follows_the_beta_vae_plans_draws():
    """SAP.py's load_data is BetVAE.py's with the sample_latent draw behind it: the same stream position before it, colored gains after"""
    s = eg().score
    N = int(np.prod(sd.SMALL_SIZES))
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    s.beta_vae_plan(sd.SMALL_SIZES, N, False, rng=a, L=10, M=7)
    want_ids = np.stack([a.randint(size, size=N // 10) for size in sd.SMALL_SIZES], 1)
    want_gains = a.uniform(0.5, 1, [N // 10, 3, 1, 1]).reshape(-1, 3)
    plan = s.sap_plan(sd.SMALL_SIZES, N, True, rng=b, L=10, M=7)
    assert np.array_equal(plan["latent_ids"], want_ids) and np.array_equal(plan["gains"], want_gains)
    assert np.array_equal(plan["idx"], want_ids @ s.latents_bases(sd.SMALL_SIZES))
    assert a.uniform() == b.uniform()


def np_objective_gradient(wb, x, s, c):
    """float64 gradient [2] of (w^2 + b^2) / 2 + sum_i c_i max(0, 1 - s_i (w x_i + b))^2, written out here independently of the generator"""
    m = np.maximum(0.0, 1.0 - s * (wb[0] * x + wb[1]))
    return np.array([wb[0] - 2.0 * np.sum(c * s * m * x), wb[1] - 2.0 * np.sum(c * s * m)])


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_is_consistent(kind):
    g = gold(kind)
    matrix = g["sap_matrix"]
    assert matrix.shape == (5, 5) and np.isfinite(matrix).all()
    sm = np.sort(matrix, axis=0)
    assert float(g["sap_score"]) == np.mean(sm[-1, :] - sm[-2, :])
    codes = np.concatenate([g["sap_cat"].astype(np.float64)[:, None], g["sap_cols"].astype(np.float64)], 1)
    n = codes.shape[0]
    assert n == 38
    y = g["sap_latents"][:, 0].astype(np.int32)
    W = g["sap_opt"]
    assert W.shape == (5, 3, 2)
    for k in range(3):
        pos = y == k
        s, c = np.where(pos, 1.0, -1.0), np.where(pos, SVC_C * (n / (3 * pos.sum())), SVC_C)
        for p in range(5):
            assert np.abs(np_objective_gradient(W[p, k], codes[:, p], s, c)).max() <= 1e-10
    assert np.array_equal(matrix[:, 0], (g["sap_predict"] == y[None, :]).mean(axis=1))
    for i in range(5):
        for j in range(1, 5):
            cov = np.cov(codes[:, i], g["sap_latents"][:, j], ddof=1)
            assert matrix[i, j] == cov[0, 1] ** 2 / cov[0, 0] / cov[1, 1]
    assert g["sap_skip"].shape == g["sap_near"].shape == (5, n)
    assert g["sap_skip"].sum(axis=1).max() <= 1 and g["sap_near"].sum(axis=1).max() <= 0.05 * n
    assert g["sap_tight_gap"].max() <= 1e-5 and g["sap_opt_gmax"].max() <= 1e-10
    dec = codes.T[:, :, None] * W[:, None, :, 0] + W[:, None, :, 1]
    assert np.array_equal(np.argmax(dec, axis=2) != g["sap_predict"], g["sap_skip"])


def test_value_errors():
    """raised before the first launch: host tensors reach them"""
    s = eg().score
    with pytest.raises(ValueError, match="metric must be"):
        s.run_score("dsprites", "dci", "none.npz", "none.pt", "none.pt")
    with pytest.raises(ValueError, match="kind must be"):
        s.run_sap("mnist", "none.npz", "none.pt", "none.pt")
    x = torch.zeros(6, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="K >= 3"):
        s.svc1_fit(x, [0, 1, 0, 1, 0, 1], 2)
    with pytest.raises(ValueError, match="do not span"):
        s.sap_latents(np.zeros((4, 6), dtype=np.int32), LATENTS_NAMES, possible_values(sd.SMALL_SIZES))
    assert s.SAP_IS_CONTINUOUS == (False, True, True, True, True)
    assert set(eg().ops.SVC_STATUS) == {0, 1, 2, 4, 5}


@pytest.mark.parametrize("kind", KINDS)
def test_generator_regenerates_fixture(kind):
    from oracle import ref_harness as rh
    if not rh.available():
        pytest.skip("the reference tree is not on this host")
    import make_sap_golden as gen
    got = gen.make(kind)
    want = gold(kind)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(np.asarray(got[k]), want[k]), k

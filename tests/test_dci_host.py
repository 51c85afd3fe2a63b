"""Host side of the DCI (Lasso) score (ead-gan_amd/score.py): dci_plan against what DCI.py's load_data / evaluate() drew and dci_scores
against the script's result dict, both recorded in tests/golden/score_dci_{dsprites,colored}.npz by tests/make_dci_golden.py, the fixture's
own consistency, the declared entry points, and the argument errors that need no GPU."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import score_data as sd

KINDS = ("dsprites", "colored")
LATENTS_NAMES = ("color", "shape", "scale", "orientation", "posX", "posY")
ALPHA = 0.02
ENTRIES = ("eg_score_norm_gram_ws_bytes", "eg_score_norm_gram", "eg_score_lasso_gram_fit")
KEYS = ("DCI_Lasso_disent_metric_detail", "DCI_Lasso_disent_metric", "DCI_Lasso_complete_metric_detail", "DCI_Lasso_complete_metric",
        "DCI_Lasso_metric_detail")


def eg():
    return importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_dci_{kind}.npz"))


def possible_values(sizes):
    _, lv = sd.latents_grid(sizes)
    return {name: np.unique(lv[:, j]) for j, name in enumerate(LATENTS_NAMES)}


@pytest.mark.parametrize("kind", KINDS)
def test_dci_plan_is_the_reference_plan(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.SMALL_SIZES))
    s = eg().score
    rng = np.random.RandomState(int(g["seed"]))
    plan = s.dci_plan(sd.SMALL_SIZES, N, colored, rng=rng)
    assert set(plan) == {"latent_ids", "idx", "gains"}
    assert plan["idx"].shape == (N // 10,) and plan["idx"].dtype == np.int64 and np.array_equal(plan["idx"], g["dci_idx"].astype(np.int64))
    assert plan["latent_ids"].shape == (N // 10, 6) and not plan["latent_ids"][:, 0].any()
    assert np.array_equal(plan["latent_ids"][:, 1:], g["dci_latent_ids"].astype(np.int64))      # load_data keeps them without the color column
    if colored:
        assert plan["gains"].shape == (N // 10, 3) and np.array_equal(plan["gains"], g["dci_gains"])
    else:
        assert plan["gains"] is None
    assert rng.uniform() == float(g["dci_plan_next"])                        # the stream stands where the script's stands
    latents = s.sap_latents(plan["latent_ids"], LATENTS_NAMES, possible_values(sd.SMALL_SIZES))
    assert latents.shape == (N // 10, 5) and np.array_equal(latents, g["dci_latents"])


@pytest.mark.parametrize("kind", KINDS)
def test_dci_plan_at_the_archive_sizes(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.FULL_SIZES))
    s = eg().score
    np.random.seed(int(g["full_seed"]))                                     # the global stream, as the scripts use it
    plan = s.dci_plan(sd.FULL_SIZES, N, colored)
    assert plan["idx"].size == int(g["full_n"]) == 73728
    assert np.array_equal(plan["idx"][:64], g["full_idx_head"].astype(np.int64))
    assert sd.digest(plan["idx"]) == str(g["full_idx_sha256"])
    assert sd.digest(plan["latent_ids"][:, 1:]) == str(g["full_latent_ids_sha256"])
    assert plan["idx"].min() >= 0 and plan["idx"].max() < N
    if colored:
        assert np.array_equal(plan["gains"][:8], g["full_gains_head"])
        assert sd.digest(plan["gains"]) == str(g["full_gains_sha256"])
    assert np.random.uniform() == float(g["full_plan_next"])
    latents = s.sap_latents(plan["latent_ids"], LATENTS_NAMES, possible_values(sd.FULL_SIZES))
    assert np.array_equal(latents[:8], g["full_latents_head"]) and sd.digest(latents) == str(g["full_latents_sha256"])


@pytest.mark.parametrize("kind", KINDS)
def test_entropic_arithmetic_reproduces_the_recorded_dict(kind):
    g = gold(kind)
    res = eg().score.dci_scores(g["dci_R"])
    assert tuple(res) == KEYS
    assert isinstance(res["DCI_Lasso_disent_metric_detail"], list) and isinstance(res["DCI_Lasso_complete_metric_detail"], list)
    assert np.array_equal(np.array(res["DCI_Lasso_disent_metric_detail"]), g["dci_disent_detail"])
    assert res["DCI_Lasso_disent_metric"] == float(g["dci_disent"])
    assert np.array_equal(np.array(res["DCI_Lasso_complete_metric_detail"]), g["dci_complete_detail"])
    assert res["DCI_Lasso_complete_metric"] == float(g["dci_complete"])
    assert np.array_equal(res["DCI_Lasso_metric_detail"], g["dci_R"])


def script_arithmetic(R, TINY=1e-12):
    """DCI.py:311-321,376-386 written out here independently of the package: (disent_scores, disent_w_avg, complete_scores, complete_avg)"""
    def entropic(r):
        r = np.abs(r)
        ps = r / np.sum(r, axis=0)
        return [1 - (- p.dot(np.log(p + TINY) / np.log(p.shape[0] + TINY))) for p in ps.T]
    with np.errstate(all="ignore"):
        d = entropic(R.T)
        return d, np.sum(np.array(d) * (np.sum(R, 1) / np.sum(R))), entropic(R), np.mean(entropic(R))


def test_unused_code_gives_the_scripts_nan():
    """a code no factor uses is a zero row of R: the script divides 0 by 0 in that code's disentanglement and carries the NaN into the
    weighted average; completeness, which normalises over codes, stays finite"""
    R = np.array([[0.5, 0.0, 0.1], [0.0, 0.0, 0.0], [0.0, 0.7, 0.2], [0.2, 0.1, 0.0]])
    res = eg().score.dci_scores(R)
    d, dw, c, ca = script_arithmetic(R)
    assert np.isnan(d[1]) and np.isnan(dw) and np.isfinite(c).all() and np.isfinite(ca)
    assert np.array_equal(np.array(res["DCI_Lasso_disent_metric_detail"]), np.array(d), equal_nan=True)
    assert np.isnan(res["DCI_Lasso_disent_metric"])
    assert np.array_equal(np.array(res["DCI_Lasso_complete_metric_detail"]), np.array(c)) and res["DCI_Lasso_complete_metric"] == ca
    one = eg().score.dci_scores(np.eye(3))                                    # one code per factor: both scores are 1 up to TINY
    assert abs(one["DCI_Lasso_disent_metric"] - 1) < 1e-10 and abs(one["DCI_Lasso_complete_metric"] - 1) < 1e-10


def np_kkt(A, c, w, alpha):
    """the KKT residual of (G_yy - 2 c.w + w.A w) / 2 + alpha |w|_1, written out here independently of the generator"""
    g = c - A @ w
    r = np.zeros(w.size)
    for i in range(w.size):
        r[i] = abs(g[i] - alpha * np.sign(w[i])) if w[i] != 0 else max(abs(g[i]) - alpha, 0.0)
    return r.max()


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_is_consistent(kind):
    g = gold(kind)
    codes = np.concatenate([g["dci_cat"].astype(np.float64)[:, None], g["dci_cols"].astype(np.float64)], 1)
    latents = g["dci_latents"]
    assert codes.shape == latents.shape == (38, 5)
    assert (np.std(codes, 0) > 0).all() and (np.std(latents, 0) > 0).all()
    Z = np.concatenate([(codes - codes.mean(0)) / codes.std(0), (latents - latents.mean(0)) / latents.std(0)], 1)
    G = Z.T @ Z / 38
    assert np.abs(G - g["dci_G"]).max() <= 1e-14 and np.abs(np.diag(G) - 1).max() <= 1e-14
    W, ref_W = g["dci_opt"], g["dci_coef"]
    assert W.shape == ref_W.shape == (5, 5) and float(g["dci_alpha"]) == ALPHA
    for j in range(5):
        assert np_kkt(G[:5, :5], G[:5, 5 + j], W[j], ALPHA) <= 1e-14
        assert np_kkt(G[:5, :5], G[:5, 5 + j], ref_W[j], ALPHA) > 1e-8           # the default fit stops at its duality gap, short of the optimum
    assert g["dci_opt_kkt"].max() <= 1e-14 and np.abs(g["dci_intercept"]).max() <= 1e-12
    assert np.array_equal(g["dci_R"], np.abs(ref_W).T)
    # the reference's fit lies within its recorded default gap of the optimum, entry by entry and score by score
    gap = g["dci_default_gap"]
    assert gap.shape == (6,) and g["dci_sens"].shape == (5,) and (gap > 0).all() and (g["dci_sens"] > 0).all()
    assert np.abs(ref_W - W).max() == gap[0] and np.abs(g["dci_R"] - np.abs(W).T).max() == gap[1] <= gap[0]
    assert gap[0] <= 1e-3                                                     # sklearn's default tolerance leaves 1e-5 .. 1e-3
    opt = eg().score.dci_scores(np.abs(W).T)
    assert np.abs(np.array(opt["DCI_Lasso_disent_metric_detail"]) - g["dci_disent_detail"]).max() == gap[2]
    assert abs(opt["DCI_Lasso_disent_metric"] - float(g["dci_disent"])) == gap[3]
    assert np.abs(np.array(opt["DCI_Lasso_complete_metric_detail"]) - g["dci_complete_detail"]).max() == gap[4]
    assert abs(opt["DCI_Lasso_complete_metric"] - float(g["dci_complete"])) == gap[5]
    assert 100 * g["dci_opt_kkt"].max() <= eg().score.DCI_KKT_TOL <= 1e-10


def test_value_errors():
    """raised before the first launch: host tensors reach them"""
    s = eg().score
    with pytest.raises(ValueError, match="metric must be"):
        s.run_score("dsprites", "dci", "none.npz", "none.pt", "none.pt")
    with pytest.raises(ValueError, match="kind must be"):
        s.run_dci("mnist", "none.npz", "none.pt", "none.pt")
    x = torch.zeros(6, 5, dtype=torch.float64)
    for name in ("RandomForest", "LassoCV", "RandomForestIBGAN", "RandomForestCV", "RandomForestEnum4"):
        with pytest.raises(NotImplementedError, match=name):
            s.dci(x, np.zeros((6, 5)), regressor=name)
    with pytest.raises(RuntimeError, match="MI355X only"):
        s.lasso_fit(x, np.zeros((6, 5)))
    assert eg().ops.LASSO_STATUS == {0: "converged", 1: "max_sweeps reached", 2: "non-finite", 3: "non-positive diagonal"}
    assert s.DCI_ALPHA == ALPHA and s.DCI_TINY == 1e-12


def test_entry_points_declared_and_bound():
    lib = eg()._lib
    protos = lib.parse_header()
    src = open(os.path.join(ROOT, "ead-gan_amd", "ops.py")).read()
    for name in ENTRIES:
        assert name in protos, name
        assert re.search(rf"""["']{name}["']""", src), name
    assert len(protos["eg_score_norm_gram"][1]) == 11 and len(protos["eg_score_lasso_gram_fit"][1]) == 9
    assert lib.lib().query("eg_version") >= 105
    ops = eg().ops
    assert ops.score_norm_gram_ws_bytes(73728, 5, 5) >= 144 * (3 * 10 + 100) * 8      # 144 row slices of sums, extrema and cross products
    assert ops.score_norm_gram_ws_bytes(1, 5, 5) == 0 and ops.score_norm_gram_ws_bytes(10, 0, 5) == 0
    assert ops.score_norm_gram_ws_bytes(10, 16, 17) == 0 and ops.score_norm_gram_ws_bytes(10, 16, 16) > 0
    assert ops.score_norm_gram_ws_bytes(2 ** 31 - 1, 5, 5) == ops.score_norm_gram_ws_bytes(10 ** 9, 5, 5)       # 1024 slices at most


@pytest.mark.parametrize("kind", KINDS)
def test_generator_regenerates_fixture(kind):
    from oracle import ref_harness as rh
    if not rh.available():
        pytest.skip("the reference tree is not on this host")
    import make_dci_golden as gen
    got = gen.make(kind)
    want = gold(kind)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(np.asarray(got[k]), want[k]), k

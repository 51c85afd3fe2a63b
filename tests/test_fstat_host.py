"""Host side of the F-stat score (ead-gan_amd/score.py): fstat_plan against what F_score.py's load_data / evaluate() drew, recorded in
tests/golden/score_fstat_{dsprites,colored}.npz by tests/make_fstat_golden.py, the fixture's own consistency, the argument errors that
need no GPU, and the new entry points' declarations and bindings."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import score_data as sd

KINDS = ("dsprites", "colored")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("eg_score_softmax_ws_bytes", "eg_score_softmax_fit", "eg_score_softmax_proba", "eg_score_auc_ovr")


def eg():
    return importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_fstat_{kind}.npz"))


@pytest.mark.parametrize("kind", KINDS)
def test_fstat_plan_is_the_reference_plan(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.SMALL_SIZES))
    s = eg().score
    rng = np.random.RandomState(int(g["seed"]))
    plan = s.fstat_plan(sd.SMALL_SIZES, N, colored, rng=rng)
    assert set(plan) == {"latent_ids", "latent_id", "idx", "gains"}
    assert plan["idx"].shape == (N // 10,) and plan["idx"].dtype == np.int64 and np.array_equal(plan["idx"], g["fstat_idx"].astype(np.int64))
    assert plan["latent_id"].shape == (N // 10, 5) and np.array_equal(plan["latent_id"], g["fstat_latent_id"].astype(np.int64))
    assert np.array_equal(plan["latent_id"], plan["latent_ids"][:, 1:]) and not plan["latent_ids"][:, 0].any()
    if colored:
        assert plan["gains"].shape == (N // 10, 3) and np.array_equal(plan["gains"], g["fstat_gains"])
    else:
        assert plan["gains"] is None
    # the group loop and the permutation the script draws and never uses are consumed: the stream stands where the script's stands
    assert rng.uniform() == float(g["fstat_plan_next"])


@pytest.mark.parametrize("kind", KINDS)
def test_fstat_plan_at_the_archive_sizes(kind):
    g = gold(kind)
    colored = kind == "colored"
    N = int(np.prod(sd.FULL_SIZES))
    s = eg().score
    np.random.seed(int(g["full_seed"]))                                     # the global stream, as the scripts use it
    plan = s.fstat_plan(sd.FULL_SIZES, N, colored)
    assert plan["idx"].size == int(g["full_n"]) == 73728
    assert np.array_equal(plan["idx"][:64], g["full_idx_head"].astype(np.int64))
    assert sd.digest(plan["idx"]) == str(g["full_idx_sha256"])
    assert sd.digest(plan["latent_id"]) == str(g["full_latent_id_sha256"])
    assert [np.unique(plan["latent_id"][:, j]).size for j in range(5)] == [3, 6, 40, 32, 32]      # the class counts the solver must take
    if colored:
        assert np.array_equal(plan["gains"][:8], g["full_gains_head"])
        assert sd.digest(plan["gains"]) == str(g["full_gains_sha256"])
    assert np.random.uniform() == float(g["full_plan_next"])


def test_fstat_plan_makes_the_sap_plans_draws():
    """F_score.py's load_data is SAP.py's line for line: the same draws, the same stream position after them"""
    s = eg().score
    N = int(np.prod(sd.SMALL_SIZES))
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    want = s.sap_plan(sd.SMALL_SIZES, N, True, rng=a, L=10, M=7)
    plan = s.fstat_plan(sd.SMALL_SIZES, N, True, rng=b, L=10, M=7)
    for k in want:
        assert np.array_equal(plan[k], want[k]), k
    assert a.uniform() == b.uniform()


def np_gradient(W, X, y, K):
    """float64 gradient of sklearn's objective, written out here independently of the generator: multinomial for K >= 3, binomial for 2"""
    n, d = X.shape
    Xt = np.concatenate([X, np.ones((n, 1))], 1)
    if K == 2:
        r = (1.0 / (1.0 + np.exp(-(Xt @ W[0]))) - (y == 1))[:, None]
    else:
        z = Xt @ W.T
        p = np.exp(z - z.max(1, keepdims=True))
        r = p / p.sum(1, keepdims=True) - (y[:, None] == np.arange(K)[None, :])
    grad = r.T @ Xt
    grad[:, :d] += W[:, :d]
    return grad


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_is_consistent(kind):
    from sklearn.metrics import mutual_info_score, roc_auc_score
    g = gold(kind)
    codes = np.concatenate([g["fstat_cat"].astype(np.float64)[:, None], g["fstat_cols"].astype(np.float64)], 1)
    n = codes.shape[0]
    assert n == 38
    lat_id = g["fstat_latent_id"].astype(np.int64)
    assert [int(k) for k in g["fstat_K"]] == list(sd.SMALL_SIZES[1:]) and 2 in g["fstat_K"]       # the binomial form is exercised
    mi = g["fstat_mi"]
    disc = g["fstat_disc"].astype(np.int64)
    assert mi.shape == (5, 5) and np.array_equal(mi, np.array([[mutual_info_score(lat_id[:, j], disc[:, i]) for j in range(5)] for i in range(5)]))
    sq = np.square(mi)
    detail = 1.0 - (sq.sum(axis=1) - sq.max(axis=1)) / (sq.max(axis=1) * 4)
    assert np.array_equal(detail, g["fstat_modu_detail"]) and float(g["fstat_modu"]) == np.mean(detail)
    assert float(g["fstat_expl"]) == np.mean(g["fstat_expl_detail"]) and g["fstat_expl_detail"].shape == (5, 1)
    for j in range(5):
        K = int(g["fstat_K"][j])
        y = lat_id[:, j]
        assert np.array_equal(np.unique(y), np.arange(K))
        W = g[f"fstat_opt_{j}"]
        assert W.shape == ((1 if K == 2 else K), 6) and np.abs(np_gradient(W, codes, y, K)).max() <= 1e-10
        if K >= 3:
            assert abs(W[:, 5].sum()) <= 1e-12
        ind = (y[:, None] == np.arange(K)[None, :]).astype(np.int64)
        assert g[f"fstat_proba_{j}"].shape == (n, K)
        assert float(g["fstat_expl_detail"][j, 0]) == roc_auc_score(ind, g[f"fstat_proba_{j}"])
    assert g["fstat_tight_gap"].max() <= 1e-5 and g["fstat_opt_gmax"].max() <= 1e-10 and g["fstat_opt_floor"].max() <= 1e-12
    assert g["fstat_near_edge"].shape == (n, 5) and g["fstat_near_edge"].sum(axis=0).max() <= 0.05 * n and not g["fstat_near_edge"][:, 0].any()
    assert (g["fstat_default_gap"] >= 0).all() and (g["fstat_sens"] >= 0).all() and g["fstat_warned"].shape == (5,)
    assert 100 * max(g["fstat_opt_floor"].max(), 0.0) <= eg().score.SOFTMAX_GTOL <= 1e-7


def test_value_errors():
    """raised before the first launch: host tensors reach them"""
    s = eg().score
    for name in ("fstat", "f_score", "dci"):
        with pytest.raises(ValueError, match="metric must be"):
            s.run_score("dsprites", name, "none.npz", "none.pt", "none.pt")
    with pytest.raises(ValueError, match="kind must be"):
        s.run_fstat("mnist", "none.npz", "none.pt", "none.pt")
    proba = torch.zeros(6, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="Only one class present"):
        s.roc_auc_ovr(proba, [0, 1, 0, 1, 0, 1], 3)                          # a class that is absent
    with pytest.raises(ValueError, match="Only one class present"):
        s.roc_auc_ovr(proba[:, :1].contiguous(), [0] * 6, 1)                 # a class that covers every row
    with pytest.raises(ValueError, match="class ids"):
        s.roc_auc_ovr(proba, [0, 1, 2, 3, 0, 1], 3)
    with pytest.raises(ValueError, match="do not match"):
        s.roc_auc_ovr(proba, [0, 1, 2], 3)
    assert set(eg().ops.SOFTMAX_STATUS) == {0, 1, 2, 3, 4, 5, 6}
    assert {k: v for k, v in eg().ops.SOFTMAX_STATUS.items() if k <= 5} == {                 # the codes' meanings stay as they are
        0: "converged", 1: "max_iter reached", 2: "line search failed", 3: "Hessian not positive definite",
        4: "a label outside 0..K-1", 5: "non-finite gradient"}
    assert s.SOFTMAX_GTOL <= 1e-7


def test_entry_points_declared_and_bound():
    lib = eg()._lib
    protos = lib.parse_header()
    src = open(os.path.join(ROOT, "ead-gan_amd", "ops.py")).read()
    for name in ENTRIES:
        assert name in protos, name
        assert re.search(rf"""["']{name}["']""", src), name
    assert len(protos["eg_score_softmax_fit"][1]) == 12 and len(protos["eg_score_auc_ovr"][1]) == 9
    assert lib.lib().query("eg_version") >= 104
    ops = eg().ops
    assert ops.score_softmax_ws_bytes(73728, 5, 40) > 64 * 240 * 240 * 8      # the Hessian's partial slabs live in the workspace
    assert ops.score_softmax_ws_bytes(10, 5, 65) == 0 and ops.score_softmax_ws_bytes(10, 5, 1) == 0
    assert ops.score_softmax_ws_bytes(10, 85, 3) == 0 and ops.score_softmax_ws_bytes(10, 84, 3) > 0
    header = open(lib.HEADER).read()
    assert "BLOCKING ENTRY POINT" in header and "capturing" in header


@pytest.mark.parametrize("kind", KINDS)
def test_generator_regenerates_fixture(kind):
    from oracle import ref_harness as rh
    if not rh.available():
        pytest.skip("the reference tree is not on this host")
    import make_fstat_golden as gen
    got = gen.make(kind)
    want = gold(kind)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(np.asarray(got[k]), want[k]), k

"""The DCI (Lasso) score of dSprites / colored-dSprites encoders on the MI355X (ead-gan_amd/score.py, csrc/score_dci.hip) against the
reference's own score/DCI.py, recorded in tests/golden/score_dci_{dsprites,colored}.npz by tests/make_dci_golden.py.

The moments kernel is judged against numpy's (X - mean) / std and Z^T Z / n.  The solver is judged by an optimality certificate (numpy's
float64 KKT residual at the returned W) and by its distance from the float64 numpy optimum, bounded through the strong convexity of the
objective; the whole score against the reference's own numbers, within the distance its default fit keeps from the optimum."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import score_data as sd
import make_dci_golden as gen           # the numpy objective and solver the fixture's optimum came from; imports no reference code here
import make_sap_golden as sapgen        # the archive's metadata

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("dsprites", "colored")
REP_TOL = {"dsprites": 1e-5, "colored": 1e-4}          # test_representation_matches_reference's
EPS = np.finfo(np.float64).eps
ALPHA = 0.02
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_dci_{kind}.npz"))


def base_gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_{kind}.npz"))


def ref_codes(g):
    return np.concatenate([g["dci_cat"].astype(np.float64)[:, None], g["dci_cols"].astype(np.float64)], 1)


# ---- 1. moments and the correlation matrix ------------------------------------------------------------------------------------------------
def device_norm_gram(codes, fv):
    n, k = codes.shape
    nf = fv.shape[1]
    m = k + nf
    ws = torch.empty(max(eg.ops.score_norm_gram_ws_bytes(n, k, nf), 8), device=DEV, dtype=torch.uint8)
    mean, std = torch.empty(m, device=DEV, dtype=torch.float64), torch.empty(m, device=DEV, dtype=torch.float64)
    G = torch.empty(m, m, device=DEV, dtype=torch.float64)
    status = torch.full((2,), 77, device=DEV, dtype=torch.int32)
    eg.ops.score_norm_gram(torch.from_numpy(codes).to(DEV), torch.from_numpy(fv).to(DEV), n, k, nf, ws, mean, std, G, status)
    return mean.cpu().numpy(), std.cpu().numpy(), G.cpu().numpy(), status.cpu().numpy()


def moment_inputs(n, k, nf):
    """codes [n,k]: an integer-valued column, float32-valued columns correlated with the factors and each other, one of the form
    7 + 1e-3 noise (column 2); factors [n,nf] on the archive's value grids.  At n = 2 the two rows differ in every column."""
    rng = np.random.RandomState(n + 100 * k + nf)
    grids = (lambda: rng.randint(6, size=n) / 5.0 * 0.5 + 0.5, lambda: rng.randint(40, size=n) * (2 * np.pi / 40), lambda: rng.randint(32, size=n) / 31.0)
    fv = np.stack([grids[j % 3]() + 0.01 * (j // 3) * rng.normal(size=n) for j in range(nf)], 1)
    cols = [rng.randint(3, size=n).astype(np.float64), fv[:, 0] * 3.0 + rng.normal(size=n), rng.normal(size=n) * 1e-3 + 7.0]
    for i in range(3, k):
        cols.append(np.sin(fv[:, i % nf]) + 0.5 * cols[i - 2] + 0.1 * rng.normal(size=n))
    codes = np.stack(cols[:k], 1)
    if n == 2:
        codes[1], fv[1] = codes[0] + 1.0 + np.arange(k), fv[0] + 0.25 + np.arange(nf)
    return codes.astype(np.float32).astype(np.float64), fv


def np_moments(codes, fv):
    X = np.concatenate([codes, fv], 1)
    mean, std = np.mean(X, 0), np.std(X, 0)
    Z = (X - mean) / std
    return mean, std, Z.T @ Z / X.shape[0]


# (n, k, nf): the row counts 2 .. 73 728 at nine columns (one slice .. 144 slices, one to four tiles a slice), then the other
# thread layouts of the cross products (m^2 <= 64: four row groups; m = 10: two; m = 32: one, four entries a thread) and the 1024-slice cap
MOMENT_CASES = [(2, 5, 4), (63, 5, 4), (65, 5, 4), (1025, 5, 4), (73728, 5, 4), (1025, 3, 2), (1025, 5, 5), (1025, 16, 16), (600001, 5, 5)]


@pytest.mark.parametrize("n,k,nf", MOMENT_CASES)
def test_norm_gram_against_numpy(n, k, nf):
    """Both sides add n rounded terms per entry, each side's sum carrying at most n eps of the sum of the terms' magnitudes -- sum |z_a z_b| / n
    <= 1 for G, max|x| for a mean, the variance itself for std^2 -- and the handful of elementwise operations around the sums (subtract,
    divide, square root, product) another few eps each, 16 eps in all: the bound is 2 (n + 16) eps of that magnitude."""
    codes, fv = moment_inputs(n, k, nf)
    mean, std, G, status = device_norm_gram(codes, fv)
    wm, wsd, wG = np_moments(codes, fv)
    assert status.tolist() == [0, -1]
    unit = 2 * (n + 16) * EPS
    em = (np.abs(mean - wm) / np.abs(np.concatenate([codes, fv], 1)).max(0)).max()
    es = (np.abs(std - wsd) / wsd).max()
    eG = np.abs(G - wG).max()
    print(f"n {n} k {k} nf {nf}: largest differences in units of n eps: mean {em / (n * EPS):.3g} std {es / (n * EPS):.3g} G {eG / (n * EPS):.3g}"
          f" (absolute {em:.3g} {es:.3g} {eG:.3g})")
    assert em <= unit and es <= unit and eG <= unit, (em, es, eG, unit)
    assert np.array_equal(G, G.T)                                             # x y and y x are one product: symmetric bit for bit
    mean2, std2, G2, status2 = device_norm_gram(codes, fv)
    assert np.array_equal(mean2, mean) and np.array_equal(std2, std) and np.array_equal(G2, G)       # fixed summation order: the same bits


def test_norm_gram_status_word():
    codes, fv = moment_inputs(63, 5, 4)
    const = codes.copy()
    const[:, 3] = 0.1                                                         # 63 x 0.1 / 63 need not round to 0.1: the test is min == max
    mean, std, G, status = device_norm_gram(const, fv)
    assert status.tolist() == [eg.ops.NORM_GRAM_ZERO_VAR, 3] and std[3] == 0.0 and mean[3] == 0.1
    assert (np.delete(std, 3) > 0).all()
    with pytest.raises(ValueError, match="code column 3 has zero variance"):
        eg.score.lasso_fit(torch.from_numpy(const).to(DEV), fv)
    cf = fv.copy()
    cf[:, 1] = 2.5
    assert device_norm_gram(codes, cf)[3].tolist() == [eg.ops.NORM_GRAM_ZERO_VAR, 6]
    with pytest.raises(ValueError, match="factor column 1 has zero variance"):
        eg.score.lasso_fit(torch.from_numpy(codes).to(DEV), cf)
    bad = codes.copy()
    bad[17, 1] = np.nan
    assert device_norm_gram(bad, fv)[3].tolist() == [eg.ops.NORM_GRAM_NONFINITE, 1]
    with pytest.raises(ValueError, match="code column 1 has a moment that is not finite"):
        eg.score.lasso_fit(torch.from_numpy(bad).to(DEV), fv)
    with pytest.raises(RuntimeError, match="at least 2"):
        device_norm_gram(codes[:1], fv[:1])
    with pytest.raises(RuntimeError, match="k \\+ nf <= 32"):
        device_norm_gram(np.zeros((4, 30)), np.zeros((4, 3)))
    assert device_norm_gram(codes, fv)[3].tolist() == [0, -1]                 # the device works afterwards


# ---- 2. the solver on numpy-built Gram matrices ---------------------------------------------------------------------------------------------
def data_gram(n, k, nf, seed, sign=1.0, mix=0.5):
    rng = np.random.RandomState(seed)
    fv = rng.normal(size=(n, nf))
    codes = sign * fv[:, np.arange(k) % nf] + mix * rng.normal(size=(n, k))
    codes[:, 1:] += mix * codes[:, :-1]
    return gen.gram(codes, fv)


def set_k1():
    return np.array([[1.0, 0.6], [0.6, 1.0]]), 1, ALPHA


def set_alpha_large():
    G = data_gram(200, 5, 3, 1)
    return G, 5, float(np.abs(G[:5, 5:]).max())                              # alpha >= max|c|: W = 0


def set_edge():
    """one target whose first right-hand side exceeds alpha by 1e-12, the others inside the dead zone"""
    G = np.eye(4)
    G[:3, :3] = data_gram(200, 3, 1, 2)[:3, :3]
    G[:3, 3] = G[3, :3] = [ALPHA + 1e-12, 0.5 * ALPHA, -0.3 * ALPHA]
    return G, 3, ALPHA


def set_negative():
    return data_gram(1025, 5, 4, 3, sign=-1.0), 5, ALPHA


def set_production():
    return gen.gram(*gen.production_set()), 5, ALPHA


def set_collinear():
    """codes 0 and 1 correlate at 1 - 2e-6: their 2 x 2 block has the eigenvalues 2 - 2e-6 and 2e-6, condition number 1e6"""
    rho = 1.0 - 2e-6
    G = np.eye(5)
    G[0, 1] = G[1, 0] = rho
    G[0, 2] = G[2, 0] = G[1, 2] = G[2, 1] = 0.3
    G[:3, 3] = G[3, :3] = [0.8, 0.79, 0.1]
    G[:3, 4] = G[4, :3] = [-0.5, -0.52, 0.4]
    return G, 3, ALPHA


SETS = {"k1_nf1": set_k1, "alpha_large": set_alpha_large, "edge_1e-12": set_edge, "negative": set_negative, "production": set_production,
        "collinear": set_collinear, "dsprites": lambda: (gold("dsprites")["dci_G"], 5, ALPHA), "colored": lambda: (gold("colored")["dci_G"], 5, ALPHA)}
_cache = {}


def problem(name):
    """(G, k, alpha, numpy optimum W [nf,k], its KKT residuals [nf]); computed once"""
    if name not in _cache:
        G, k, alpha = SETS[name]()
        W, _, res = gen.lasso_gram_fit_all(G, k, alpha)
        _cache[name] = (G, k, alpha, W, res)
    return _cache[name]


def device_fit(G, k, alpha, max_sweeps=10000, tol=None):
    nf = G.shape[0] - k
    W = torch.full((nf, k), 7.0, device=DEV, dtype=torch.float64)
    info = torch.zeros(nf, 4, device=DEV, dtype=torch.float64)
    eg.ops.score_lasso_gram_fit(torch.from_numpy(np.ascontiguousarray(G)).to(DEV), k, nf, alpha, max_sweeps, eg.score.DCI_KKT_TOL if tol is None else tol, W, info)
    return W.cpu().numpy(), info.cpu().numpy()


def judge(name, G, k, alpha, Wd, W_opt, kkt_opt, compare_objective=False):
    """Certificate: numpy's KKT residual at the device's W is <= 10 tol (the slack: k eps rounding between the two evaluations of A w).
    Distance: subgradients s_a, s_b of the objective at a, b with |s|inf <= their KKT residuals satisfy (s_a - s_b).(a - b) >=
    lambda_min(A) |a - b|^2, so |a - b|_2 <= sqrt(k) (kkt_a + kkt_b) / lambda_min(A), with the bound formed here from numpy's residuals on
    this G.  Where A is nearly singular that bound says little about W, and the objectives are compared instead: f(a) - f(b) <=
    s_a.(a - b), so |f(a) - f(b)| <= max(kkt_a, kkt_b) |a - b|_1, plus the k^2 products' rounding in evaluating f."""
    tol = eg.score.DCI_KKT_TOL
    A = G[:k, :k]
    lam = np.linalg.eigvalsh(A).min()
    for j in range(G.shape[0] - k):
        c = G[:k, k + j]
        kd = gen.kkt_residual(A, c, Wd[j], alpha)
        assert kd <= 10 * tol, (name, j, kd)
        dist = np.linalg.norm(Wd[j] - W_opt[j])
        bound = np.sqrt(k) * (kd + kkt_opt[j]) / lam
        print(f"{name} target {j}: numpy KKT at the device's W {kd:.3g}, at the numpy optimum {kkt_opt[j]:.3g}; |W - optimum|_2 {dist:.3g}, bound {bound:.3g}"
              f" (lambda_min {lam:.3g})")
        if compare_objective:
            gyy = G[k + j, k + j]
            fd, fo = gen.objective(A, c, gyy, Wd[j], alpha), gen.objective(A, c, gyy, W_opt[j], alpha)
            fb = max(kd, kkt_opt[j]) * np.abs(Wd[j] - W_opt[j]).sum() + 4 * k * k * EPS * (1 + np.abs(W_opt[j]).sum()) ** 2
            print(f"{name} target {j}: objective {fd!r}, at the numpy optimum {fo!r}, bound on the difference {fb:.3g}")
            assert abs(fd - fo) <= fb, (name, j, fd, fo, fb)
        else:
            assert dist <= bound, (name, j, dist, bound)


@pytest.mark.parametrize("name", sorted(SETS))
def test_solver_on_gram_matrices(name):
    G, k, alpha, W_opt, kkt_opt = problem(name)
    nf = G.shape[0] - k
    Wd, info = device_fit(G, k, alpha)
    assert Wd.shape == (nf, k) and (info[:, 3] == 0).all(), info
    assert (info[:, 1] <= eg.score.DCI_KKT_TOL).all()
    print(name, "sweeps", info[:, 0], "device KKT", info[:, 1])
    judge(name, G, k, alpha, Wd, W_opt, kkt_opt, compare_objective=name == "collinear")
    for j in range(nf):                                                       # info's objective is the objective at W
        f = gen.objective(G[:k, :k], G[:k, k + j], G[k + j, k + j], Wd[j], alpha)
        assert abs(info[j, 2] - f) <= 4 * k * k * EPS * (1 + np.abs(Wd[j]).sum()) ** 2, (info[j, 2], f)
    W2, info2 = device_fit(G, k, alpha)
    assert np.array_equal(W2, Wd) and np.array_equal(info2, info)             # the same bits
    if name == "alpha_large":
        assert (Wd == 0).all() and (info[:, 0] <= 1).all() and (W_opt == 0).all()
    if name == "edge_1e-12":
        assert 0 < Wd[0, 0] < 2e-12 and (Wd[0, 1:] == 0).all()
    if name == "k1_nf1":
        assert Wd[0, 0] == (0.6 - ALPHA) / 1.0
    if name == "negative":
        assert (Wd.min(axis=1) < -0.1).all()
    if name == "production":
        assert info[:, 0].max() > 50                                          # condition number 47: not a one-sweep problem
    if name == "collinear":
        assert (np.count_nonzero(Wd[:, :2], axis=1) == 1).all()               # the penalty keeps one of the collinear pair


def test_solver_status_paths():
    """an error return or a status, not a fault; the device works afterwards"""
    G, k, alpha, W_opt, _ = problem("production")
    Wd, info = device_fit(G, k, alpha, max_sweeps=3)
    assert (info[:, 3] == 1).any() and (info[info[:, 3] == 1, 0] == 3).all() and np.isfinite(Wd).all()
    assert (info[info[:, 3] == 1, 1] > eg.score.DCI_KKT_TOL).all()
    codes, fv = gen.production_set()
    with pytest.raises(RuntimeError, match="max_sweeps reached"):
        eg.score.lasso_fit(torch.from_numpy(codes).to(DEV), fv, max_sweeps=3)
    bad = G.copy()
    bad[1, 2] = bad[2, 1] = np.nan
    Wd, info = device_fit(bad, k, alpha)
    assert (info[:, 3] == 2).all() and (Wd == 0).all()
    bad = G.copy()
    bad[3, 3] = 0.0
    Wd, info = device_fit(bad, k, alpha)
    assert (info[:, 3] == 3).all() and (Wd == 0).all()
    with pytest.raises(RuntimeError, match="k \\+ nf <= 32"):
        device_fit(np.eye(33), 20, alpha)
    with pytest.raises(RuntimeError, match="alpha must not be negative"):
        device_fit(G, k, -1.0)
    Wd, info = device_fit(G, k, alpha)
    assert (info[:, 3] == 0).all()


# ---- 3. the reference's run ---------------------------------------------------------------------------------------------------------------
def score_arrays(res):
    return [np.array(res["DCI_Lasso_disent_metric_detail"]), np.array(res["DCI_Lasso_disent_metric"]),
            np.array(res["DCI_Lasso_complete_metric_detail"]), np.array(res["DCI_Lasso_complete_metric"])]


def gold_scores(g):
    return [g["dci_disent_detail"], g["dci_disent"], g["dci_complete_detail"], g["dci_complete"]]


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_on_reference_codes(kind):
    g = gold(kind)
    codes, latents = ref_codes(g), g["dci_latents"]
    fit = eg.score.lasso_fit(torch.from_numpy(codes).to(DEV), latents)
    assert set(fit) == {"R", "W", "mean", "std", "G", "info"} and (fit["info"][:, 3] == 0).all()
    Wd, R = fit["W"].cpu().numpy(), fit["R"].cpu().numpy()
    assert R.shape == (5, 5) and np.array_equal(R, np.abs(Wd).T)
    X = np.concatenate([codes, latents], 1)
    assert np.abs(fit["mean"].cpu().numpy() - X.mean(0)).max() <= 2 * (38 + 16) * EPS * np.abs(X).max()
    G = g["dci_G"]                                                            # numpy's: the residuals below carry the device's moments too
    assert np.abs(fit["G"].cpu().numpy() - G).max() <= 2 * (38 + 16) * EPS
    W_opt, kkt_opt = g["dci_opt"], g["dci_opt_kkt"]
    judge(kind, G, 5, ALPHA, Wd, W_opt, kkt_opt)
    lam = np.linalg.eigvalsh(G[:5, :5]).min()
    bound = max(np.sqrt(5) * (gen.kkt_residual(G[:5, :5], G[:5, 5 + j], Wd[j], ALPHA) + kkt_opt[j]) / lam for j in range(5))
    assert np.abs(R - np.abs(W_opt).T).max() <= bound
    # the reference's own numbers: its default fit's recorded distance from the optimum, plus that bound
    gap = g["dci_default_gap"]
    print(kind, "max|R - reference R|", np.abs(R - g["dci_R"]).max(), "reference |default - optimum|", gap[1], "bound", bound)
    assert np.abs(R - g["dci_R"]).max() <= gap[1] + bound
    res = eg.score.dci(torch.from_numpy(codes).to(DEV), latents)
    assert np.array_equal(res["DCI_Lasso_metric_detail"], R)
    for name, got, want, gp in zip(gen.GAP_NAMES[2:], score_arrays(res), gold_scores(g), gap[2:]):
        print(kind, name, "largest difference from the reference", np.abs(got - want).max(), "reference |default - optimum|", gp)
        assert np.abs(got - want).max() <= gp + bound, name


# ---- 4. end to end through run_dci --------------------------------------------------------------------------------------------------------
def encoders(kind, g):
    mod = eg.colored if kind == "colored" else eg.dsprites
    P, E = mod.Encoder_pxy(), mod.Encoder()
    s_pxy, s_enc = (int(s) for s in g["weight_seeds"])
    psd = sd.make_weights(P.state_dict(), s_pxy, float(g["cat_scale"]))
    esd = sd.make_weights(E.state_dict(), s_enc, float(g["cat_scale"]))
    assert np.array_equal(sd.checksums(psd), g["pxy_checksums"]) and np.array_equal(sd.checksums(esd), g["enc_checksums"])
    return psd, esd


@pytest.mark.parametrize("kind", KINDS)
def test_run_dci_end_to_end(kind, tmp_path, capsys):
    g, b = gold(kind), base_gold(kind)
    psd, esd = encoders(kind, b)
    sizes = tuple(int(s) for s in b["sizes"])
    imgs, lv, lc, _ = sd.dataset(sizes)
    meta = sapgen.metadata(sizes)
    npz, pp, ep = (os.path.join(str(tmp_path), n) for n in (sd.NPZ_NAME, "pxy.pt", "enc.pt"))
    sd.write_npz(npz, imgs, lv, lc, meta)
    torch.save(psd, pp)
    torch.save(esd, ep)
    res = eg.score.run_dci(kind, npz, pp, ep, seed=int(g["seed"]))
    out = capsys.readouterr().out
    assert "disent_scores [" in out and "complete_avg " in out
    assert tuple(res) == ("DCI_Lasso_disent_metric_detail", "DCI_Lasso_disent_metric", "DCI_Lasso_complete_metric_detail",
                          "DCI_Lasso_complete_metric", "DCI_Lasso_metric_detail")
    R = res["DCI_Lasso_metric_detail"]
    assert R.shape == (5, 5) and np.isfinite(R).all()
    # the optimum on the reference's codes, within 4 x what representation noise of twice the tolerance moved it (the SAP fixtures' factor)
    sens, gap = g["dci_sens"], g["dci_default_gap"]
    opt_R = np.abs(g["dci_opt"]).T
    opt_scores = score_arrays(eg.score.dci_scores(opt_R))
    print(kind, "max|R - optimum on the reference's codes|", np.abs(R - opt_R).max(), "4 sens", 4 * sens[0])
    assert np.abs(R - opt_R).max() <= 4 * sens[0]
    assert np.abs(R - g["dci_R"]).max() <= gap[1] + 4 * sens[0]
    for name, got, opt, want, s, gp in zip(gen.GAP_NAMES[2:], score_arrays(res), opt_scores, gold_scores(g), sens[1:], gap[2:]):
        print(kind, name, got, "from the optimum", np.abs(got - opt).max(), "4 sens", 4 * s, "from the reference", np.abs(got - want).max())
        assert np.abs(got - opt).max() <= 4 * s, name
        assert np.abs(got - want).max() <= gp + 4 * s, name

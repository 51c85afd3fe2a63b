"""The SAP score of dSprites / colored-dSprites encoders on the MI355X (ead-gan_amd/score.py, csrc/score.hip) against the reference's own
score/SAP.py, recorded in tests/golden/score_sap_{dsprites,colored}.npz by tests/make_sap_golden.py.

The correlation kernel is judged against the np.cov formula.  The solver is judged three ways: by an optimality certificate (numpy's float64
gradient of every one-vs-rest objective at the returned W), against the float64 numpy optimum / a tight sklearn fit, and against the
reference's own predictions and accuracies."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import score_data as sd
import make_sap_golden as gen           # the numpy objective and solver the fixture's optimum came from; imports no reference code here

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("dsprites", "colored")
REP_TOL = {"dsprites": 1e-5, "colored": 1e-4}          # test_representation_matches_reference's
CERT = 1e-9                                             # |g|inf of every one-vs-rest objective
IS_CONTINUOUS = [False, True, True, True, True]
# The tests assert 100 x these figures.  They come from a float64 numpy emulation of the kernels' arithmetic in the kernels'
# own summation order (row t, t + 256, ... per thread, the 64-lane butterfly, (w0 + w1) + (w2 + w3); IEEE operations, no contraction),
# which is what the device computes; no MI355X was reachable when they were taken, so a device run has yet to confirm them.
CORR_REL = 6.91e-14                                     # largest relative difference of eg_score_sq_corr from the np.cov formula
OPT_GAP = {"n3_K3": 6.94e-18, "n64_K3_single": 5.56e-17, "n65_K3_constant": 1.12e-16, "n1025_K3_integers": 3.34e-16,
           "n5003_K3_separated": 4.45e-16, "n1025_K8": 3.34e-16, "production": 2.21e-12, "dsprites": 8.33e-17,
           "colored": 1.12e-16}                         # max|W - numpy optimum|
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_sap_{kind}.npz"))


def base_gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_{kind}.npz"))


def ref_codes(g):
    return np.concatenate([g["sap_cat"].astype(np.float64)[:, None], g["sap_cols"].astype(np.float64)], 1)


# ---- 1. squared correlations ----------------------------------------------------------------------------------------------------------
def np_sq_corr(codes, fv):
    R = np.zeros((codes.shape[1], fv.shape[1]))
    with np.errstate(all="ignore"):
        for i in range(codes.shape[1]):
            for j in range(fv.shape[1]):
                cov = np.cov(codes[:, i], fv[:, j], ddof=1)
                R[i, j] = cov[0, 1] ** 2 / cov[0, 0] / cov[1, 1]
    return R


def device_sq_corr(codes, fv):
    R = torch.empty(codes.shape[1], fv.shape[1], device=DEV, dtype=torch.float64)
    eg.ops.score_sq_corr(torch.from_numpy(codes).to(DEV), codes.shape[0], codes.shape[1], torch.from_numpy(fv).to(DEV), fv.shape[1], R)
    return R.cpu().numpy()


def corr_inputs(n):
    """codes [n,5]: an integer-valued column, three correlated float32-valued ones, a constant one; factors [n,4]: one of them constant"""
    rng = np.random.RandomState(n)
    fv = np.stack([rng.randint(6, size=n) / 5.0 * 0.5 + 0.5, rng.randint(40, size=n) * (2 * np.pi / 40), rng.randint(32, size=n) / 31.0,
                   np.full(n, 0.25)], 1)
    codes = np.stack([rng.randint(3, size=n).astype(np.float64), fv[:, 0] * 3.0 + rng.normal(size=n), rng.normal(size=n) * 1e-3 + 7.0,
                      np.sin(fv[:, 1]) + 0.1 * rng.normal(size=n), np.full(n, -1.5)], 1)
    return codes.astype(np.float32).astype(np.float64), fv


@pytest.mark.parametrize("n", (2, 63, 65, 1025, 73728))
def test_sq_corr_against_numpy(n):
    codes, fv = corr_inputs(n)
    want, got = np_sq_corr(codes, fv), device_sq_corr(codes, fv)
    nan = np.isnan(want)
    assert nan[4].all() and nan[:, 3].all()                                   # the constant column / factor: 0 / 0 on both sides
    if n > 2:
        assert not nan[:4, :3].any()
    assert np.array_equal(np.isnan(got), nan), (got, want)
    ok = ~nan
    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok]) if ok.any() else np.zeros(1)
    print("n", n, "largest relative difference from np.cov's formula", rel.max())
    assert rel.max() <= 100 * CORR_REL, rel.max()
    assert np.array_equal(device_sq_corr(codes, fv), got, equal_nan=True)      # fixed summation order: the same bits
    if n == 2:
        with pytest.raises(RuntimeError, match="at least 2"):
            device_sq_corr(codes[:1], fv[:1])


# ---- 2. the solver ----------------------------------------------------------------------------------------------------------------------
def labels(n, K, rng):
    return rng.permutation(np.arange(n) % K)


def separated(y, rng):
    return 4.0 * y + 0.4 * rng.normal(size=y.size)


def integers(y, rng):
    flip = rng.uniform(size=y.size) < 0.3
    return np.where(flip, rng.randint(3, size=y.size), y % 3).astype(np.float64)


def set_n3():
    return np.array([[-1.0], [0.3], [2.0]]), np.array([0, 1, 2]), 3            # every class a single sample


def set_single():
    rng = np.random.RandomState(64)
    y = np.r_[rng.permutation(np.arange(63) % 2), 2]                          # class 2 has one sample: weight C n / K
    return (1.5 * y + rng.normal(size=64))[:, None], y, 3


def set_constant():
    return np.full((65, 1), 0.75), labels(65, 3, np.random.RandomState(65)), 3


def set_integers():
    rng = np.random.RandomState(1025)
    y = labels(1025, 3, rng)
    return integers(y, rng)[:, None], y, 3


def set_separated():
    rng = np.random.RandomState(5003)
    y = labels(5003, 3, rng)
    return separated(y, rng)[:, None], y, 3


def set_K8():
    rng = np.random.RandomState(8)
    y = labels(1025, 8, rng)
    return (0.7 * y + rng.normal(size=1025))[:, None], y, 8


def set_production():
    """the reference's shape: n = 73 728 samples, the five code columns, three shapes"""
    rng = np.random.RandomState(73728)
    n = 73728
    y = rng.randint(3, size=n)
    X = np.stack([integers(y, rng), separated(y, rng), 0.5 * y + rng.normal(size=n), np.full(n, 0.75), 1e3 * (0.5 * y + rng.normal(size=n))], 1)
    return X, y, 3


SETS = {"n3_K3": set_n3, "n64_K3_single": set_single, "n65_K3_constant": set_constant, "n1025_K3_integers": set_integers,
        "n5003_K3_separated": set_separated, "n1025_K8": set_K8, "production": set_production}
_cache = {}


def problem(name):
    """(X, y, K, numpy optimum W [P,K,2], the smallest |g|inf the numpy solver reached [P,K]); computed once"""
    if name not in _cache:
        X, y, K = SETS[name]()
        W, its, gmax, best = gen.svc_fit_all(X, y, K, gtol=0.0, max_iter=12)   # past convergence: `best` is the float64 rounding floor
        _cache[name] = (X, y, K, W, best)
    return _cache[name]


def np_gradients(W, X, y, K):
    """|g|inf [P,K] of every one-vs-rest objective at W, by the fixture generator's float64 formula"""
    out = np.zeros(W.shape[:2])
    for k in range(K):
        s, c = gen.svc_problem(y, k, K)
        for p in range(W.shape[0]):
            out[p, k] = np.abs(gen.svc_objective(W[p, k], X[:, p], s, c)[1]).max()
    return out


def certificate(name, W, X, y, K, floor):
    """numpy's gradient at the device's W is <= CERT; where float64 rounding of the sums cannot reach that (the 1e3-scaled column at
    n = 73 728), <= 10 x the floor the numpy solver itself reaches on that problem"""
    g = np_gradients(W, X, y, K)
    bound = np.maximum(CERT, 10 * floor)
    print(name, "certificate: |g|inf per column", g.max(axis=1), "numpy solver's floor", floor.max(axis=1))
    assert (g <= bound).all(), (g, bound)


def check_fit(name, X, y, K, W_opt, floor, sklearn_gap=True):
    Xd = torch.from_numpy(X).to(DEV)
    W, predict, correct, info = eg.score.svc1_fit(Xd, y, K)
    Wh = W.cpu().numpy()
    n, P = X.shape
    assert Wh.shape == (P, K, 2) and info.shape == (P, K, 4) and (info[:, :, 3] == 0).all()
    print(name, "iterations", info[:, :, 0].min(), "..", info[:, :, 0].max(), "largest |g|inf", info[:, :, 1].max())
    certificate(name, Wh, X, y, K, floor)
    gap = np.abs(Wh - W_opt).max()
    print(name, "max|W - numpy optimum|", gap)
    bound = min(100 * OPT_GAP[name], 1e-8)
    assert gap <= bound, gap
    # predictions: the device's own argmax exactly, the optimum's wherever the top-two gap exceeds what `bound` can move
    dec_dev, dec_opt = gen.decisions(Wh, X), gen.decisions(W_opt, X)
    ph = predict.cpu().numpy()
    top = np.sort(dec_dev, axis=2)
    clear = (top[:, :, -1] - top[:, :, -2]) > 1e-12 * (1.0 + np.abs(X.T))     # the argmax does not hang on the last bits of w x + b
    assert np.array_equal(ph[clear], np.argmax(dec_dev, axis=2)[clear])
    top = np.sort(dec_opt, axis=2)
    safe = (top[:, :, -1] - top[:, :, -2]) > 2 * bound * (1.0 + np.abs(X.T))
    assert np.array_equal(ph[safe], np.argmax(dec_opt, axis=2)[safe])
    ch = correct.cpu().numpy()
    assert np.array_equal(ch, (ph == y[None, :]).sum(axis=1))
    assert (np.abs(ch - (np.argmax(dec_opt, axis=2) == y[None, :]).sum(axis=1)) <= (~safe).sum(axis=1)).all()
    W2, p2, c2, i2 = eg.score.svc1_fit(Xd, y, K)
    assert torch.equal(W2, W) and torch.equal(p2, predict) and torch.equal(c2, correct) and np.array_equal(i2, info)     # the same bits
    if sklearn_gap:
        from sklearn.svm import LinearSVC
        for p in range(P):
            t = LinearSVC(C=0.01, class_weight="balanced", dual=False, tol=1e-12, max_iter=100000).fit(X[:, p:p + 1], y)
            sk = np.abs(np.stack([t.coef_[:, 0], t.intercept_], 1) - Wh[p]).max()
            print(name, "column", p, "max|W - tight sklearn|", sk)
            assert sk <= 1e-5, sk
    return Wh, ph, ch, info


@pytest.mark.parametrize("name", sorted(SETS))
def test_solver_on_synthetic_sets(name):
    X, y, K, W_opt, floor = problem(name)
    Wh, ph, ch, info = check_fit(name, X, y, K, W_opt, floor)
    acc = ch / X.shape[0]
    print(name, "accuracy", acc)
    if name == "n5003_K3_separated":
        assert acc[0] > 0.9
    if name == "production":
        assert acc[1] > 0.9 and info[:, :, 0].max() > 1


def test_status_paths():
    """an error return, not a fault; the device works afterwards"""
    X, y, K, _, _ = problem("n64_K3_single")
    Xd = torch.from_numpy(X).to(DEV)
    W = torch.full((1, 3, 2), 7.0, device=DEV, dtype=torch.float64)
    info = torch.zeros(1, 3, 4, device=DEV, dtype=torch.float64)
    for yb in (np.where(np.arange(64) == 17, 3, y), np.where(np.arange(64) == 17, -1, y), np.where(y == 2, 1, y)):     # a label = K; < 0; class 2 empty
        yd = torch.from_numpy(yb.astype(np.int32)).to(DEV)
        W.fill_(7.0)
        eg.ops.score_svc1_fit(Xd, yd, 64, 1, 3, 0.01, 50, 1e-10, W, info)
        assert (info.cpu().numpy()[:, :, 3] == 4).all() and (W == 0).all()
        with pytest.raises(RuntimeError, match="label outside|without a sample"):
            eg.score.svc1_fit(Xd, yb, 3)
    bad = X.copy()
    bad[5, 0] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        eg.score.svc1_fit(torch.from_numpy(bad).to(DEV), y, 3)
    with pytest.raises(RuntimeError, match="max_iter"):
        eg.score.svc1_fit(Xd, y, 3, max_iter=0)
    with pytest.raises(RuntimeError, match="3..64"):
        eg.ops.score_svc1_fit(Xd, torch.zeros(64, device=DEV, dtype=torch.int32), 64, 1, 65, 0.01, 50, 1e-10, W, info)
    W2, _, _, info2 = eg.score.svc1_fit(Xd, y, 3)
    assert (info2[:, :, 3] == 0).all() and torch.isfinite(W2).all()


# ---- 3. the reference's run -------------------------------------------------------------------------------------------------------------
def corr_bound(codes_ref, tol):
    """How far a code column within ``tol`` of the reference's can move a squared correlation: with x~ the centred column, the unit vector
    x~ / |x~| moves by at most 2 |e| / |x~| <= 2 tol sqrt(n / (n - 1)) / std(x), rho by as much, rho^2 by twice that"""
    n = codes_ref.shape[0]
    return 4.0 * tol * np.sqrt(n / (n - 1.0)) / np.std(codes_ref, axis=0, ddof=1)


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_on_reference_codes(kind):
    g = gold(kind)
    codes, latents = ref_codes(g), g["sap_latents"]
    n = codes.shape[0]
    y = latents[:, 0].astype(np.int32)
    Wh, ph, ch, info = check_fit(kind, codes, y, 3, g["sap_opt"], g["sap_opt_gmax"], sklearn_gap=False)
    ref_W = np.stack([g["sap_coef"], g["sap_intercept"]], 2)
    print(kind, "max|W - reference default fit|", np.abs(Wh - ref_W).max(), "reference |default - optimum|", g["sap_default_gap"].max())
    loose = g["sap_near"] | g["sap_skip"]
    assert np.array_equal(ph[~loose], g["sap_predict"].astype(np.int32)[~loose])
    R, fits = eg.score.sap_matrix(torch.from_numpy(codes).to(DEV), latents, IS_CONTINUOUS)
    R = R.cpu().numpy()
    assert set(fits) == {0} and torch.equal(fits[0]["W"].cpu(), torch.from_numpy(Wh)) and np.array_equal(fits[0]["classes"], np.arange(3))
    ref = g["sap_matrix"]
    assert (np.abs(R[:, 0] - ref[:, 0]) <= loose.sum(axis=1) / n + 1e-15).all(), (R[:, 0], ref[:, 0])
    rel = np.abs(R[:, 1:] - ref[:, 1:]) / np.abs(ref[:, 1:])
    print(kind, "discrete column", R[:, 0], "reference", ref[:, 0], "continuous entries: largest relative difference", rel.max())
    assert rel.max() <= 100 * CORR_REL, rel.max()
    res = eg.score.sap(torch.from_numpy(codes).to(DEV), latents, IS_CONTINUOUS)
    assert set(res) == {"SAP_metric", "SAP_metric_detail"} and np.array_equal(res["SAP_metric_detail"], R)
    sm = np.sort(R, axis=0)
    assert res["SAP_metric"] == np.mean(sm[-1] - sm[-2])
    move = np.r_[loose.sum(axis=1).max() / n, (100 * CORR_REL * np.abs(ref[:, 1:])).max(axis=0)]
    print(kind, "SAP", res["SAP_metric"], "reference", float(g["sap_score"]))
    assert abs(res["SAP_metric"] - float(g["sap_score"])) <= np.mean(2 * move) + 1e-15


# ---- 4. end to end through run_sap ------------------------------------------------------------------------------------------------------
def sprites(g):
    n = int(np.prod(g["sizes"]))
    return np.unpackbits(g["sprites_bits"], axis=1)[:, :4096].reshape(n, 64, 64)


def encoders(kind, g):
    mod = eg.colored if kind == "colored" else eg.dsprites
    P, E = mod.Encoder_pxy(), mod.Encoder()
    s_pxy, s_enc = (int(s) for s in g["weight_seeds"])
    psd = sd.make_weights(P.state_dict(), s_pxy, float(g["cat_scale"]))
    esd = sd.make_weights(E.state_dict(), s_enc, float(g["cat_scale"]))
    assert np.array_equal(sd.checksums(psd), g["pxy_checksums"]) and np.array_equal(sd.checksums(esd), g["enc_checksums"])
    P.load_state_dict(psd)
    E.load_state_dict(esd)
    return P.to(DEV), E.to(DEV), psd, esd


@pytest.mark.parametrize("kind", KINDS)
def test_run_sap_end_to_end(kind, tmp_path, capsys):
    g, b = gold(kind), base_gold(kind)
    colored = kind == "colored"
    P, E, psd, esd = encoders(kind, b)
    sizes = tuple(int(s) for s in b["sizes"])
    imgs, lv, lc, _ = sd.dataset(sizes)
    meta = gen.metadata(sizes)
    npz, pp, ep = (os.path.join(str(tmp_path), n) for n in (sd.NPZ_NAME, "pxy.pt", "enc.pt"))
    sd.write_npz(npz, imgs, lv, lc, meta)
    torch.save(psd, pp)
    torch.save(esd, ep)
    res = eg.score.run_sap(kind, npz, pp, ep, seed=int(g["seed"]))
    assert "score " in capsys.readouterr().out
    assert set(res) == {"SAP_metric", "SAP_metric_detail"}
    R = res["SAP_metric_detail"]
    # the same pipeline step by step
    np.random.seed(int(g["seed"]))
    plan = eg.score.sap_plan(meta["latents_sizes"], imgs.shape[0], colored)
    latents = eg.score.sap_latents(plan["latent_ids"], meta["latents_names"], meta["latents_possible_values"])
    assert np.array_equal(latents, g["sap_latents"])
    codes = eg.score.Representation(P, E, kind).codes(torch.from_numpy(sprites(b)).to(DEV), plan["idx"], plan["gains"])
    R2, fits = eg.score.sap_matrix(codes, latents, IS_CONTINUOUS)
    assert np.array_equal(R2.cpu().numpy(), R)
    ch, ref = codes.cpu().numpy(), ref_codes(g)
    n = ref.shape[0]
    err = np.abs(ch[:, 1:] - ref[:, 1:]).max()
    print(kind, "SAP", res["SAP_metric"], "reference", float(g["sap_score"]), "code error", err, "near", g["sap_near"].sum(axis=1))
    assert err <= REP_TOL[kind], err
    assert np.array_equal(ch[:, 0], ref[:, 0])                                # the fixture holds no cat tie
    loose = g["sap_near"] | g["sap_skip"]
    moved = fits[0]["predict"].cpu().numpy() != g["sap_predict"].astype(np.int32)
    assert not (moved & ~loose).any(), np.argwhere(moved & ~loose)
    want = g["sap_matrix"]
    assert (np.abs(R[:, 0] - want[:, 0]) <= loose.sum(axis=1) / n + 1e-15).all(), (R[:, 0], want[:, 0])
    cb = corr_bound(ref, REP_TOL[kind])
    cb[0] = 0.0                                                               # the cat column is equal
    cont = cb[:, None] + 100 * CORR_REL * np.abs(want[:, 1:])
    diff = np.abs(R[:, 1:] - want[:, 1:])
    print(kind, "continuous entries: largest difference", diff.max(), "bound", cont.max())
    assert (diff <= cont).all(), (diff, cont)
    move = np.r_[loose.sum(axis=1).max() / n, cont.max(axis=0)]               # a sorted column moves by at most its largest entry change
    assert abs(res["SAP_metric"] - float(g["sap_score"])) <= np.mean(2 * move) + 1e-15
    sm = np.sort(R, axis=0)
    assert res["SAP_metric"] == np.mean(sm[-1] - sm[-2]) and np.isfinite(R).all()

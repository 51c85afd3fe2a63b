"""The F-stat score of dSprites / colored-dSprites encoders on the MI355X (ead-gan_amd/score.py, csrc/score_fstat.hip) against the reference's
own score/F_score.py, recorded in tests/golden/score_fstat_{dsprites,colored}.npz by tests/make_fstat_golden.py.

The AUC kernel's counts are compared for integer equality with numpy.  The solver is judged as tests/test_gpu_sap.py judges its solver: by
an optimality certificate (numpy's float64 gradient of the objective at the returned W), against the float64 numpy optimum and a tight
sklearn fit, and, on the reference's recorded codes, against the reference's own explicitness."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import score_data as sd
import make_fstat_golden as gen         # the numpy objective and solver the fixture's optimum came from; imports no reference code here
import make_sap_golden as gen_sap       # the archive's metadata keys

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("dsprites", "colored")
REP_TOL = {"dsprites": 1e-5, "colored": 1e-4}          # test_representation_matches_reference's
EPS = np.finfo(np.float64).eps
# max|W - numpy optimum| as check_fit / test_fixture_on_reference_codes printed it on the first device run (one MI355X, the numpy optimum
# of problem() / the fixture; DESIGN 6h lists the same figures); the tests assert 100 x these, capped at 1e-6
OPT_GAP = {"n3_K3": 1.51e-11, "n64_K2": 1.12e-16, "n65_K3_constant": 1.12e-15, "n1025_K8": 1.19e-14, "n1025_K40": 3.86e-12,
           "n1027_K13_d7": 3.66e-14, "n1025_K3_scaled": 7.51e-13, "production": 1.11e-12, "dsprites": 1.51e-12, "colored": 3.63e-12}
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_fstat_{kind}.npz"))


def base_gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_{kind}.npz"))


def ref_codes(g):
    return np.concatenate([g["fstat_cat"].astype(np.float64)[:, None], g["fstat_cols"].astype(np.float64)], 1)


# ---- 1. AUC counts ----------------------------------------------------------------------------------------------------------------------
def np_counts_pairs(scores, y, K):
    """every pair compared"""
    less, equal = np.zeros(K, dtype=np.uint64), np.zeros(K, dtype=np.uint64)
    for k in range(K):
        pos, neg = scores[y == k, k], scores[y != k, k]
        less[k] = (neg[None, :] < pos[:, None]).sum()
        equal[k] = (neg[None, :] == pos[:, None]).sum()
    return less, equal


def np_counts_ranks(scores, y, K):
    """an independent method: ranks of the positives among the sorted negatives"""
    less, equal = np.zeros(K, dtype=np.uint64), np.zeros(K, dtype=np.uint64)
    for k in range(K):
        pos, neg = scores[y == k, k], np.sort(scores[y != k, k])
        lo, hi = np.searchsorted(neg, pos, "left"), np.searchsorted(neg, pos, "right")
        less[k], equal[k] = lo.sum(), (hi - lo).sum()
    return less, equal


def spread_labels(n, K, rng):
    return rng.permutation(np.arange(n) % K)


def auc_case(name):
    """-> (scores [n,K], y [n], K, the exact AUC every class must have or None)"""
    kind, n, K = name.split("-")
    n, K = int(n), int(K)
    rng = np.random.RandomState(n * 131 + K)
    y = spread_labels(n, K, rng)
    onehot = (y[:, None] == np.arange(K)[None, :]).astype(np.float64)
    if kind == "random":
        s = rng.uniform(size=(n, K)) + 0.5 * onehot
        return s / s.sum(1, keepdims=True), y, K, None
    if kind == "single":                                          # class K-1 has a single positive
        y = np.where(y == K - 1, 0, y)
        y[n // 2] = K - 1
        return rng.uniform(size=(n, K)), y, K, None
    if kind == "equal":
        return np.full((n, K), 0.25), y, K, 0.5
    if kind == "separated":
        return onehot + 0.25 * rng.uniform(size=(n, K)), y, K, 1.0
    if kind == "inverted":
        return -onehot - 0.25 * rng.uniform(size=(n, K)), y, K, 0.0
    if kind == "quantised":                                       # 8 levels: heavy ties
        return np.floor(8 * np.clip(rng.uniform(size=(n, K)) + 0.2 * onehot, 0, 0.999)) / 8, y, K, None
    if kind == "production":                                      # the reference's shape, scores rounded to 3 decimals: ties at scale
        return np.round(rng.uniform(size=(n, K)) + 0.3 * onehot, 3), y, K, None
    raise KeyError(name)


AUC_CASES = ("random-2-2", "random-65-3", "random-1025-40", "random-1025-2", "single-65-3", "equal-65-3", "equal-1025-2",
             "separated-65-3", "separated-1025-40", "inverted-65-3", "inverted-1025-2", "quantised-65-3", "quantised-1025-40",
             "production-73728-40")


@pytest.mark.parametrize("name", AUC_CASES)
def test_auc_counts(name):
    from sklearn.metrics import roc_auc_score
    s, y, K, exact = auc_case(name)
    n = s.shape[0]
    sd_ = torch.from_numpy(s).to(DEV)
    auc, less, equal = eg.score.roc_auc_ovr(sd_, y, K)
    want_less, want_equal = (np_counts_ranks if n > 2000 else np_counts_pairs)(s, y, K)
    assert less.dtype == np.uint64 and np.array_equal(less, want_less) and np.array_equal(equal, want_equal), (less, want_less, equal, want_equal)
    npos = np.bincount(y, minlength=K).astype(np.float64)
    assert np.array_equal(auc, (2.0 * less.astype(np.float64) + equal.astype(np.float64)) / (2.0 * npos * (n - npos)))
    ref = np.array([roc_auc_score(y == k, s[:, k]) for k in range(K)])
    err = np.abs(auc - ref).max()
    print(name, "largest |AUC - roc_auc_score|", err, "ties", int(equal.sum()))
    assert err <= 4 * n * EPS, err                                # the trapezoid sums at most n + 1 terms of size <= 1
    if exact is not None:
        assert (auc == exact).all(), auc
    if name.startswith("quantised") or name.startswith("production"):
        assert equal.sum() > 0
    auc2, less2, equal2 = eg.score.roc_auc_ovr(sd_, y, K)
    assert np.array_equal(less2, less) and np.array_equal(equal2, equal) and np.array_equal(auc2, auc)


def test_auc_value_errors():
    s = torch.zeros(6, 3, device=DEV, dtype=torch.float64)
    with pytest.raises(ValueError, match="Only one class"):
        eg.score.roc_auc_ovr(s, [0, 1, 0, 1, 0, 1], 3)           # class 2 is absent
    with pytest.raises(ValueError, match="Only one class"):
        eg.score.roc_auc_ovr(s[:, :1], [0] * 6, 1)               # one class covers every row
    with pytest.raises(ValueError, match="class ids"):
        eg.score.roc_auc_ovr(s, [0, 1, 2, 3, 0, 1], 3)


# ---- 2. the solver ----------------------------------------------------------------------------------------------------------------------
def f32(X):
    return X.astype(np.float32).astype(np.float64)


def set_n3():
    return np.array([[-1.0, 0.5], [0.3, -0.2], [2.0, 1.0]]), np.array([0, 1, 2]), 3              # every class a single sample


def set_n64_K2():
    rng = np.random.RandomState(64)
    y = spread_labels(64, 2, rng)
    return f32(np.stack([1.2 * y + rng.normal(size=64), rng.normal(size=64), rng.randint(3, size=64).astype(np.float64)], 1)), y, 2


def set_constant():
    rng = np.random.RandomState(65)
    y = spread_labels(65, 3, rng)
    return f32(np.stack([0.8 * y + rng.normal(size=65), np.full(65, 0.75), rng.normal(size=65)], 1)), y, 3


def codes_like(y, K, rng):
    """five columns of the real kind: an integer class code, two continuous codes that follow the factor, two positions"""
    n = y.size
    a = 2 * np.pi * y / K
    return f32(np.stack([rng.randint(3, size=n).astype(np.float64), np.cos(a) + 0.6 * rng.normal(size=n), np.sin(a) + 0.6 * rng.normal(size=n),
                         rng.uniform(-0.5, 0.5, size=n), 0.3 * y / K + rng.uniform(-0.5, 0.5, size=n)], 1))


def set_K8():
    rng = np.random.RandomState(8)
    y = spread_labels(1025, 8, rng)
    return codes_like(y, 8, rng), y, 8


def set_K40():
    rng = np.random.RandomState(40)
    y = spread_labels(1025, 40, rng)
    return codes_like(y, 40, rng), y, 40                          # P = 240: the Hessian at its largest


def set_K13():
    rng = np.random.RandomState(13)
    y = spread_labels(1027, 13, rng)
    X = np.concatenate([codes_like(y, 13, rng), f32(rng.normal(size=(1027, 2)))], 1)
    return X, y, 13                                               # d = 7, P = 104: no multiple of any tile


def set_scaled():
    rng = np.random.RandomState(1000)
    y = spread_labels(1025, 3, rng)
    flip = rng.uniform(size=1025) < 0.3
    ints = np.where(flip, rng.randint(3, size=1025), y).astype(np.float64)
    return f32(np.stack([ints, 1e3 * (0.5 * y + rng.normal(size=1025))], 1)), y, 3


def set_production():
    """the reference's shape: n = 73 728 samples, the five code columns, the 40 orientations"""
    rng = np.random.RandomState(73728)
    y = rng.randint(40, size=73728)
    return codes_like(y, 40, rng), y, 40


SETS = {"n3_K3": set_n3, "n64_K2": set_n64_K2, "n65_K3_constant": set_constant, "n1025_K8": set_K8, "n1025_K40": set_K40,
        "n1027_K13_d7": set_K13, "n1025_K3_scaled": set_scaled, "production": set_production}
_cache = {}


def problem(name):
    """(X, y, K, numpy optimum W, the smallest |g|inf the numpy solver reached); computed once"""
    if name not in _cache:
        X, y, K = SETS[name]()
        W, its, gmax, best = gen.lr_newton(X, y, K, gtol=0.0, max_iter=60, patience=3)    # past convergence: `best` is float64's floor
        print(name, "numpy solver: iterations", its, "floor", best)
        _cache[name] = (X, y, K, W, best)
    return _cache[name]


def np_gradient(W, X, y, K):
    return float(np.abs(gen.lr_objective(W, X, y, K)[1]).max())


def check_fit(name, X, y, K, W_opt, floor, sklearn_gap=True):
    gtol = eg.score.SOFTMAX_GTOL
    assert gtol <= 1e-7
    Xd = torch.from_numpy(X).to(DEV)
    W, info = eg.score.softmax_fit(Xd, y, K)
    Wh = W.cpu().numpy()
    n, d = X.shape
    assert Wh.shape == ((1 if K == 2 else K), d + 1) and info.shape == (4,) and info[3] == 0
    assert 1 <= info[0] <= 50 and info[1] <= gtol and np.isfinite(info[2])
    g = np_gradient(Wh, X, y, K)
    print(name, "iterations", int(info[0]), "device |g|inf", info[1], "certificate: numpy |g|inf", g, "numpy solver's floor", floor)
    assert g <= max(gtol, 10 * floor), g
    if K >= 3:
        assert abs(Wh[:, d].sum()) <= 1e-9 * max(1.0, np.abs(Wh[:, d]).max())       # zero-sum intercepts
    gap = np.abs(Wh - W_opt).max()
    bound = min(100 * OPT_GAP[name], 1e-6)
    print(name, "max|W - numpy optimum|", gap, "bound", bound)
    assert gap <= bound, gap
    W2, info2 = eg.score.softmax_fit(Xd, y, K)
    assert torch.equal(W2, W) and np.array_equal(info2, info)                       # one summation order: the same bits
    if sklearn_gap:
        sk = np.abs(gen.tight_sklearn(X, y, K) - Wh).max()
        print(name, "max|W - tight sklearn|", sk)
        assert sk <= 1e-5, sk
    return Wh, info, bound


@pytest.mark.parametrize("name", sorted(SETS))
def test_solver_on_synthetic_sets(name):
    X, y, K, W_opt, floor = problem(name)
    Wh, info, _ = check_fit(name, X, y, K, W_opt, floor)
    proba = eg.score.softmax_proba(torch.from_numpy(X).to(DEV), torch.from_numpy(Wh).to(DEV), K).cpu().numpy()
    want = gen.lr_proba(Wh, X, K)
    assert proba.shape == (X.shape[0], K)
    assert np.abs(proba - want).max() <= 64 * EPS * (1.0 + np.abs(X).sum(axis=1).max() * np.abs(Wh).max()), np.abs(proba - want).max()
    assert np.abs(proba.sum(axis=1) - 1.0).max() <= 64 * EPS
    if name == "production":
        assert info[0] > 1


def test_status_paths():
    """an error return, not a fault; the device works afterwards"""
    X, y, K, _, _ = problem("n65_K3_constant")
    n, d = X.shape
    Xd = torch.from_numpy(X).to(DEV)
    ws = torch.empty(eg.ops.score_softmax_ws_bytes(n, d, K), device=DEV, dtype=torch.uint8)
    W = torch.full((K, d + 1), 7.0, device=DEV, dtype=torch.float64)
    info = torch.zeros(4, device=DEV, dtype=torch.float64)
    cases = ((np.where(np.arange(n) == 17, K, y), 4, "label outside"), (np.where(np.arange(n) == 17, -1, y), 4, "label outside"),
             (np.where(y == 2, 1, y), 6, "without a sample"))
    for yb, status, text in cases:
        W.fill_(7.0)
        eg.ops.score_softmax_fit(Xd, torch.from_numpy(yb.astype(np.int32)).to(DEV), n, d, K, 1.0, 50, 1e-8, ws, W, info)
        assert info.cpu().numpy()[3] == status and (W == 0).all()
        with pytest.raises(RuntimeError, match=text):
            eg.score.softmax_fit(Xd, yb, K)
    bad = X.copy()
    bad[5, 0] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        eg.score.softmax_fit(torch.from_numpy(bad).to(DEV), y, K)
    with pytest.raises(RuntimeError, match="max_iter"):
        eg.score.softmax_fit(Xd, y, K, max_iter=0)
    assert eg.ops.score_softmax_ws_bytes(n, d, 65) == 0 and eg.ops.score_softmax_ws_bytes(n, 256, 2) == 0
    yd = torch.zeros(n, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="2..64"):
        eg.ops.score_softmax_fit(Xd, yd, n, d, 65, 1.0, 50, 1e-8, ws, W, info)
    with pytest.raises(RuntimeError, match="2..64"):
        eg.ops.score_softmax_fit(Xd, yd, n, d, 1, 1.0, 50, 1e-8, ws, W, info)
    wide = torch.zeros(4, 256, device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="exceed 256"):        # K = 2, d = 256: P = 257 in the binomial form
        eg.ops.score_softmax_fit(wide, yd, 4, 256, 2, 1.0, 50, 1e-8, ws, W, info)
    with pytest.raises(RuntimeError, match="exceed 256"):        # K (d + 1) = 258
        eg.ops.score_softmax_fit(wide, yd, 4, 85, 3, 1.0, 50, 1e-8, ws, W, info)
    with pytest.raises(RuntimeError, match="exceed 256"):
        eg.ops.score_softmax_proba(wide, 4, 85, 3, W, info)
    W2, info2 = eg.score.softmax_fit(Xd, y, K)
    assert info2[3] == 0 and torch.isfinite(W2).all()


# ---- 3. the reference's run ---------------------------------------------------------------------------------------------------------------
def close(got, want, rel, ab):
    return np.all(np.abs(got - want) <= np.maximum(rel * np.abs(want), ab))


def auc_margin(W_opt, X, y, K, wb):
    """How far a W within ``wb`` of the optimum (and the device's exp, a few ulp) can move the macro AUC at the optimum: a logit moves by
    at most dz = wb (1 + sum_a |x_a|), a probability by at most 2 dz, so only the (positive, negative) pairs of distinct rows whose scores
    lie within 4 dz of each other can change sides, each by at most one pair's weight."""
    proba = gen.lr_proba(W_opt, X, K)
    dz = max(wb, 64 * EPS * max(1.0, np.abs(W_opt).max())) * (1.0 + np.abs(X).sum(axis=1).max())
    distinct = (X[:, None, :] != X[None, :, :]).any(axis=2)
    out = np.zeros(K)
    for k in range(K):
        pos, neg = np.flatnonzero(y == k), np.flatnonzero(y != k)
        closeby = np.abs(proba[pos, k][:, None] - proba[neg, k][None, :]) <= 4 * dz
        out[k] = (closeby & distinct[np.ix_(pos, neg)]).sum() / (pos.size * neg.size)
    return float(out.mean())


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_on_reference_codes(kind):
    g = gold(kind)
    codes, lat_id = ref_codes(g), g["fstat_latent_id"].astype(np.int64)
    n = codes.shape[0]
    cd = torch.from_numpy(codes).to(DEV)
    assert np.array_equal(eg.score.discretize(cd).cpu().numpy().T, g["fstat_disc"].astype(np.int32))
    modu, detail, mi = eg.score.fstat_modularity(cd, lat_id)
    assert mi.shape == (5, 5) and close(mi, g["fstat_mi"], 1e-12, 1e-15), np.abs(mi - g["fstat_mi"]).max()
    assert close(detail, g["fstat_modu_detail"], 1e-12, 1e-15) and close(modu, float(g["fstat_modu"]), 1e-12, 1e-15)
    expl, edetail, fits = eg.score.fstat_explicitness(cd, lat_id)
    assert edetail.shape == (5, 1) and expl == np.mean(edetail) and set(fits) == set(range(5))
    for j in range(5):
        K = int(g["fstat_K"][j])
        y = lat_id[:, j]
        W_opt = g[f"fstat_opt_{j}"]
        Wh = fits[j]["W"].cpu().numpy()
        assert np.array_equal(fits[j]["classes"], np.arange(K)) and fits[j]["info"][3] == 0
        gcert = np_gradient(Wh, codes, y, K)
        gap = np.abs(Wh - W_opt).max()
        bound = min(100 * OPT_GAP[kind], 1e-6)
        print(kind, "factor", j, "K", K, "iterations", int(fits[j]["info"][0]), "numpy |g|inf", gcert, "max|W - numpy optimum|", gap,
              "max|W - reference default fit|", np.abs(Wh - gen.sklearn_W(g[f"fstat_coef_{j}"], g[f"fstat_intercept_{j}"], K)).max())
        assert gcert <= max(eg.score.SOFTMAX_GTOL, 10 * float(g["fstat_opt_floor"][j])) and gap <= bound
        margin = 4 * n * EPS + auc_margin(W_opt, codes, y, K, bound)
        got, opt, ref = float(edetail[j, 0]), float(g["fstat_auc_opt"][j]), float(g["fstat_expl_detail"][j, 0])
        print(kind, "factor", j, "explicitness", got, "at the optimum", opt, "reference", ref, "margin", margin)
        assert abs(got - opt) <= margin
        assert abs(got - ref) <= float(g["fstat_default_gap"][j]) + margin
    res = eg.score.fstat(cd, lat_id)
    assert list(res) == ["FStat_modu_metric", "FStat_modu_metric_detail", "FStat_modu_mi", "FStat_expl_metric", "FStat_expl_metric_detail"]
    assert res["FStat_modu_metric_detail"].shape == (5,) and res["FStat_modu_mi"].shape == (5, 5)
    assert res["FStat_expl_metric_detail"].shape == (5, 1)
    assert res["FStat_modu_metric"] == modu and np.array_equal(res["FStat_modu_mi"], mi) and res["FStat_expl_metric"] == expl
    assert np.array_equal(res["FStat_expl_metric_detail"], edetail) and np.array_equal(res["FStat_modu_metric_detail"], detail)


# ---- 4. end to end through run_fstat ------------------------------------------------------------------------------------------------------
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
def test_run_fstat_end_to_end(kind, tmp_path, capsys):
    from sklearn.metrics import mutual_info_score
    g, b = gold(kind), base_gold(kind)
    colored = kind == "colored"
    P, E, psd, esd = encoders(kind, b)
    sizes = tuple(int(s) for s in b["sizes"])
    imgs, lv, lc, _ = sd.dataset(sizes)
    meta = gen_sap.metadata(sizes)
    npz, pp, ep = (os.path.join(str(tmp_path), n) for n in (sd.NPZ_NAME, "pxy.pt", "enc.pt"))
    sd.write_npz(npz, imgs, lv, lc, meta)
    torch.save(psd, pp)
    torch.save(esd, ep)
    res = eg.score.run_fstat(kind, npz, pp, ep, seed=int(g["seed"]))
    printed = capsys.readouterr().out
    assert "modu_score " in printed and "expl_score " in printed
    # the same pipeline step by step: bit for bit
    np.random.seed(int(g["seed"]))
    plan = eg.score.fstat_plan(meta["latents_sizes"], imgs.shape[0], colored)
    lat_id = plan["latent_id"]
    assert np.array_equal(lat_id, g["fstat_latent_id"].astype(np.int64))
    codes = eg.score.Representation(P, E, kind).codes(torch.from_numpy(sprites(b)).to(DEV), plan["idx"], plan["gains"])
    step = eg.score.fstat(codes, lat_id)
    assert list(step) == list(res)
    for k in res:
        assert np.array_equal(np.asarray(step[k]), np.asarray(res[k])), k
    ch, ref = codes.cpu().numpy(), ref_codes(g)
    n = ref.shape[0]
    err = np.abs(ch[:, 1:] - ref[:, 1:]).max()
    assert err <= REP_TOL[kind], err
    assert np.array_equal(ch[:, 0], ref[:, 0])                                # the fixture holds no cat tie
    # modularity: a bin differs from the reference's only where the fixture lists the sample as near a bin edge, and the matrix is
    # sklearn's on the device's own bins
    bins = eg.score.discretize(codes).cpu().numpy().T
    moved = bins != g["fstat_disc"].astype(np.int32)
    assert not (moved & ~g["fstat_near_edge"]).any(), np.argwhere(moved & ~g["fstat_near_edge"])
    want_mi = g["fstat_mi"] if not moved.any() else np.array([[mutual_info_score(lat_id[:, j], bins[:, i]) for j in range(5)] for i in range(5)])
    assert close(res["FStat_modu_mi"], want_mi, 1e-12, 1e-15), np.abs(res["FStat_modu_mi"] - want_mi).max()
    if not moved.any():
        assert close(res["FStat_modu_metric"], float(g["fstat_modu"]), 1e-12, 1e-15)
    # explicitness
    got, want = res["FStat_expl_metric_detail"][:, 0], g["fstat_expl_detail"][:, 0]
    bound = g["fstat_default_gap"] + 4 * g["fstat_sens"] + 4 * n * EPS
    print(kind, "code error", err, "bins moved", int(moved.sum()), "modularity", res["FStat_modu_metric"], "reference", float(g["fstat_modu"]),
          "explicitness", got, "reference", want, "bound", bound)
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    assert abs(res["FStat_expl_metric"] - float(g["fstat_expl"])) <= bound.mean() + 4 * EPS

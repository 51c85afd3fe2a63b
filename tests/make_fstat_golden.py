"""Generate tests/golden/score_fstat_{dsprites,colored}.npz from the reference's own score/F_score.py (needs the reference tree; host only).

    python tests/make_fstat_golden.py [dsprites] [colored]

The scripts' load_data, encoders, add_color_2_img and FStatMetric are loaded with oracle.ref_harness.load_defs and run unchanged on
torch-CPU against the synthetic archive, weights and seeds of tests/score_data.py (the sprites are read back from score_{kind}.npz;
N = 384, so the reference scores 38 samples), with make_sap_golden's metadata.  The ``LogisticRegression`` they see is a subclass that
records its fits.  Next to the reference's numbers the file holds, per factor, ``fstat_opt_<j>``: the float64 optimum of the objective
LogisticRegression minimises (multinomial; binomial for the two-class factor) from the Newton iteration below, the AUC at it, how far the
reference's default fit sits from it (``fstat_default_gap``), what a representation within tolerance may move (``fstat_sens``) and which
samples sit near a bin edge of the modularity half's histogram (``fstat_near_edge``).  Only numbers are written out.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import ref_harness as rh        # noqa: E402
import score_data as sd                     # noqa: E402
import make_score_golden as msg             # noqa: E402
import make_betavae_golden as mbg           # noqa: E402
import make_sap_golden as mgs               # noqa: E402

GOLD = msg.GOLD
NAMES = ("load_data", "Encoder", "Encoder_pxy", "transformation_2D", "load_encoder", "add_color_2_img", "FStatMetric")
NOISE = mbg.NOISE
NOISE_DRAWS = mbg.NOISE_DRAWS
NOISE_SEED = mbg.NOISE_SEED
TIE = mbg.TIE
NUM_BINS = 20
NF = 5
# np.random.seed of the recorded run.  The base fixture's seed is tried first; a seed of this fixture's own stands here when the base
# seed's 38 samples do not meet the assertions of make() (None: the base seed does).
FSTAT_SEED = {"dsprites": None, "colored": None}


def recording_classifier():
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import LogisticRegression

    class Recorded(LogisticRegression):
        log = []

        def fit(self, X, y, sample_weight=None):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                super().fit(X, y, sample_weight)
            Recorded.log.append(dict(X=np.array(X), y=np.array(y), coef=self.coef_.copy(), intercept=self.intercept_.copy(),
                                     n_iter=self.n_iter_.copy(), proba=self.predict_proba(X), max_iter=self.max_iter, C=self.C,
                                     classes=self.classes_.copy(),
                                     warned=[str(w.message) for w in caught if issubclass(w.category, ConvergenceWarning)]))
            return self

    return Recorded


def ref_globals(kind, classifier=None):
    from sklearn import metrics
    from sklearn.metrics import mutual_info_score, roc_auc_score
    from sklearn.preprocessing import MultiLabelBinarizer
    names = ("from_latent_vector_2_affine_para_pxy", "from_latent_vector_2_color_para_pxy", "get_matrix_pxy_align")
    u = rh.load_defs(f"{msg.DIRS[kind]}/utils_pxy.py", names)
    extra = {k: u[k] for k in names if k in u}
    extra.update(metrics=metrics, code_dim=7 if kind == "colored" else 4, n_classes=3, img_shape=(64, 64, 1), LogisticRegression=classifier,
                 mutual_info_score=mutual_info_score, roc_auc_score=roc_auc_score, MultiLabelBinarizer=MultiLabelBinarizer)
    g = rh.load_defs(f"{msg.DIRS[kind]}/F_score.py", NAMES, extra=extra)
    g["trans_2D"] = g["transformation_2D"]()
    return g


# ---- the objective the reference's classifier minimises, in float64 numpy ---------------------------------------------------------
def lr_objective(W, X, y, K, inv_C=1.0):
    """K >= 3: f = sum_i CE(softmax(W [x_i, 1]), y_i) + inv_C / 2 |coefficients|^2, W [K,d+1].  K = 2: sklearn's binomial form
    f = sum_i [log(1 + exp(z_i)) - y_i z_i] + inv_C / 2 |w|^2, W [1,d+1].  -> (f, gradient, probabilities [n,K] or p [n,1], [X, 1])"""
    n, d = X.shape
    Xt = np.concatenate([X, np.ones((n, 1))], 1)
    if K == 2:
        z = Xt @ W[0]
        e = np.exp(-np.abs(z))
        q = 1.0 / (1.0 + e)
        p = np.where(z >= 0, q, e * q)[:, None]
        f = float(np.sum(np.maximum(z, 0.0) + np.log1p(e) - np.where(y == 1, z, 0.0)) + 0.5 * inv_C * np.sum(W[:, :d] ** 2))
        r = p - (y == 1)[:, None]
    else:
        z = Xt @ W.T
        m = z.max(1, keepdims=True)
        e = np.exp(z - m)
        se = e.sum(1, keepdims=True)
        p = e / se
        f = float(np.sum(np.log(se[:, 0]) - (z[np.arange(n), y] - m[:, 0])) + 0.5 * inv_C * np.sum(W[:, :d] ** 2))
        r = p.copy()
        r[np.arange(n), y] -= 1.0
    grad = r.T @ Xt
    grad[:, :d] += inv_C * W[:, :d]
    return f, grad, p, Xt


def lr_hessian(p, Xt, K, inv_C=1.0):
    """sum_i (diag(p_i) - p_i p_i^T) (x) [x_i, 1][x_i, 1]^T + the penalty + (K >= 3) v v^T, v = 1/sqrt(K) on each intercept"""
    n, D = Xt.shape
    d = D - 1
    if K == 2:
        H = (Xt * (p[:, 0] * (1.0 - p[:, 0]))[:, None]).T @ Xt
        H[np.arange(d), np.arange(d)] += inv_C
        return H
    A = (p[:, :, None] * Xt[:, None, :]).reshape(n, K * D)
    H = -(A.T @ A)
    blocks = (p.T @ (Xt[:, :, None] * Xt[:, None, :]).reshape(n, D * D)).reshape(K, D, D)
    for k in range(K):
        H[k * D:(k + 1) * D, k * D:(k + 1) * D] += blocks[k]
    H += np.diag(np.tile(np.r_[np.full(d, inv_C), 0.0], K))
    v = np.tile(np.r_[np.zeros(d), 1.0 / np.sqrt(K)], K)
    return H + np.outer(v, v)


def lr_newton(X, y, K, inv_C=1.0, gtol=1e-13, max_iter=50, patience=None):
    """damped Newton from W = 0 (make_betavae_golden.newton's iteration, with the binomial form for K = 2)
    -> (W, iterations, final |g|inf, smallest |g|inf seen).  ``patience``: with gtol = 0, stop once that many iterations in a row have
    not lowered the smallest |g|inf: the iteration has reached float64's rounding floor on this set."""
    n, d = X.shape
    W = np.zeros((1 if K == 2 else K, d + 1))
    f, grad, p, Xt = lr_objective(W, X, y, K, inv_C)
    best, stale = np.inf, 0
    for it in range(max_iter + 1):
        gm = float(np.abs(grad).max())
        stale = 0 if gm < best else stale + 1
        best = min(best, gm)
        if gm <= gtol or it == max_iter or (patience is not None and stale >= patience):
            break
        s = -np.linalg.solve(lr_hessian(p, Xt, K, inv_C), grad.reshape(-1)).reshape(W.shape)
        gs = float(np.sum(grad * s))
        t = 1.0
        while True:
            fn, gn, pn, _ = lr_objective(W + t * s, X, y, K, inv_C)
            if fn <= f + 1e-4 * t * gs + n * np.finfo(float).eps * abs(f) or t < 1e-12:
                break
            t *= 0.5
        W, f, grad, p = W + t * s, fn, gn, pn
    return W, it, float(np.abs(grad).max()), best


def lr_proba(W, X, K):
    """predict_proba at W [n,K]: softmax of the logits, or [1 - p, p] for K = 2"""
    p = lr_objective(W, X, np.zeros(X.shape[0], dtype=np.int64), K)[2]
    return np.concatenate([1.0 - p, p], 1) if K == 2 else p


def indicator(y, K):
    return (np.asarray(y)[:, None] == np.arange(K)[None, :]).astype(np.int64)


def auc_macro(proba, y, K):
    """what F_score.py:333-336 computes: roc_auc_score of the MultiLabelBinarizer indicator against predict_proba, macro average"""
    from sklearn.metrics import roc_auc_score
    return float(roc_auc_score(indicator(y, K), proba))


def sklearn_W(coef, intercept, K):
    """sklearn's coef_ / intercept_ as one [K,d+1] matrix ([1,d+1] for K = 2)"""
    W = np.concatenate([coef, intercept[:, None]], 1)
    assert W.shape[0] == (1 if K == 2 else K)
    return W


def tight_sklearn(X, y, K):
    from sklearn.linear_model import LogisticRegression
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = LogisticRegression(solver="newton-cg", tol=1e-12, max_iter=10000).fit(X, y)
    return sklearn_W(clf.coef_, clf.intercept_, K)


def bin_edges(x, num_bins=NUM_BINS):
    return np.histogram(x, num_bins)[1][:-1]


def near_edge(codes, tol, num_bins=NUM_BINS):
    """samples whose bin a representation within ``tol`` may change: within 2 tol (the sample and the edge each move by tol) of an inner
    bin edge of their column's histogram.  The cat column holds exact integers on both sides and is never near."""
    out = np.zeros(codes.shape, dtype=bool)
    for j in range(1, codes.shape[1]):
        edges = bin_edges(codes[:, j], num_bins)[1:]
        out[:, j] = np.abs(codes[:, j][:, None] - edges[None, :]).min(axis=1) <= 2 * tol
    return out


def plan_indices(kind, sizes, seed):
    """F_score load_data's plan read back through an archive whose images are their own indices, then (colored) the gains evaluate() would
    draw, through the script's own add_color_2_img; last the stream's next uniform draw"""
    g = ref_globals(kind)
    cls, lv = sd.latents_grid(sizes)
    N = lv.shape[0]
    with msg.workdir(np.arange(N, dtype=np.int64), lv, cls, mgs.metadata(sizes), {}, {}, kind):
        np.random.seed(seed)
        _, md, _, _ = g["load_data"]()
        d = md["img_with_latent"]
        n = d["img"].shape[0]
        gains = g["add_color_2_img"](torch.zeros(n, 1, 1, 1))[1].reshape(n, 3) if kind == "colored" else None
        nxt = np.random.uniform()
    return d["img"].astype(np.int64), d["latent_id"], gains, nxt


def make(kind):
    torch.set_num_threads(8)
    colored = kind == "colored"
    base = np.load(os.path.join(GOLD, f"score_{kind}.npz"))
    sizes = tuple(int(s) for s in base["sizes"])
    assert sizes == sd.SMALL_SIZES
    N = int(np.prod(sizes))
    imgs = np.unpackbits(base["sprites_bits"], axis=1)[:, :4096].reshape(N, 64, 64)
    lc, lv = sd.latents_grid(sizes)
    assert np.array_equal(lv, base["latents_values"])
    meta = mgs.metadata(sizes)
    pxy, enc = msg.weights(kind)
    assert np.array_equal(sd.checksums(pxy), base["pxy_checksums"]) and np.array_equal(sd.checksums(enc), base["enc_checksums"])
    seed = int(base["seed"]) if FSTAT_SEED[kind] is None else FSTAT_SEED[kind]
    out = {"seed": np.array(seed), "base_seed": np.array(int(base["seed"]))}

    # ---- the plan, at the fixture sizes and at the archive's ----
    idx, lat_id, pgains, nxt = plan_indices(kind, sizes, seed)
    n = idx.size
    assert n == N // 10 == 38 and lat_id.shape == (n, NF)
    fi, fid, fgains, fnxt = plan_indices(kind, sd.FULL_SIZES, msg.FULL_SEED)
    out.update(fstat_idx=idx.astype(np.uint16), fstat_latent_id=lat_id.astype(np.int8), fstat_plan_next=np.array(nxt),
               full_seed=np.array(msg.FULL_SEED), full_n=np.array(fi.size), full_idx_head=fi[:64].astype(np.uint32),
               full_idx_sha256=np.array(sd.digest(fi)), full_latent_id_sha256=np.array(sd.digest(fid)), full_plan_next=np.array(fnxt))
    if colored:
        out.update(fstat_gains=pgains, full_gains_head=fgains[:8], full_gains_sha256=np.array(sd.digest(fgains)))

    # ---- module-level code of F_score.py ----
    Rec = recording_classifier()
    g = ref_globals(kind, Rec)
    colors = []
    outs = msg.recording(g, colors)
    with msg.workdir(imgs, lv, lc, meta, pxy, enc, kind):
        np.random.seed(seed)
        _, md, _, _ = g["load_data"]()
        metric = g["FStatMetric"](md)
        res = metric.evaluate()
    log = list(Rec.log)
    assert len(outs["enc"]) == 1 and len(outs["pxy"]) == 1 and len(log) == NF
    codes, probs = msg.rows(outs, 0)
    d = md["img_with_latent"]
    assert np.array_equal(d["img"], imgs[idx]) and np.array_equal(d["latent_id"], lat_id)
    if colored:
        assert len(colors) == 1 and np.array_equal(colors[0], pgains)
    assert set(res) == {"FStat_modu_metric", "FStat_modu_metric_detail", "FStat_modu_mi", "FStat_expl_metric", "FStat_expl_metric_detail"}
    mi, modu_detail, modu = res["FStat_modu_mi"], res["FStat_modu_metric_detail"], float(res["FStat_modu_metric"])
    expl_detail, expl = res["FStat_expl_metric_detail"], float(res["FStat_expl_metric"])
    assert mi.shape == (5, NF) and modu_detail.shape == (5,) and expl_detail.shape == (NF, 1)
    assert np.isfinite(mi).all() and np.isfinite(modu_detail).all() and np.isfinite(expl_detail).all()
    disc = metric.discretize(codes)
    assert np.array_equal(mi, metric.mutual_info(disc, lat_id))

    # ---- the modularity half: which samples a representation within tolerance may move to another bin ----
    ps = np.sort(probs.astype(np.float64), axis=1)
    tie = (ps[:, -1] - ps[:, -2]) <= TIE
    assert not tie.any(), np.flatnonzero(tie)          # a cat tie would move column 0 of every fit: take another seed
    near = near_edge(codes, NOISE[kind] / 2)
    assert near.sum(axis=0).max() <= 0.05 * n, near.sum(axis=0)

    # ---- the explicitness half: the optimum per factor, and the checks that make it a target ----
    cat, cols = msg.split(codes)
    out.update(fstat_cat=cat, fstat_cols=cols, fstat_probs=probs.astype(np.float32), fstat_disc=disc.astype(np.int8), fstat_mi=mi,
               fstat_modu_detail=modu_detail, fstat_modu=np.array(modu), fstat_expl_detail=expl_detail, fstat_expl=np.array(expl),
               fstat_near_edge=near)
    Ks, its, gmax, floor, tight_gap, default_w_gap, auc_opt, default_gap, sens, n_iter, warned = ([] for _ in range(11))
    rng = np.random.RandomState(NOISE_SEED)
    noisy_sets = []
    for _ in range(NOISE_DRAWS):
        noisy = codes.copy()
        noisy[:, 1:] += rng.uniform(-NOISE[kind], NOISE[kind], (n, 4))
        noisy_sets.append(noisy)
    rng2 = np.random.RandomState(NOISE_SEED + 1)
    for j, l in enumerate(log):
        classes, y = np.unique(lat_id[:, j], return_inverse=True)
        y = y.reshape(-1)
        K = classes.size
        assert K == sizes[j + 1] and np.array_equal(classes, np.arange(K)), (j, classes)       # every class is among the samples
        assert np.array_equal(l["X"], codes) and np.array_equal(l["y"], lat_id[:, j]) and np.array_equal(l["classes"], classes)
        assert l["C"] == 1.0 and l["max_iter"] == 100
        ref_auc = auc_macro(l["proba"], y, K)
        assert ref_auc == float(expl_detail[j, 0])
        W, nit, gm, _ = lr_newton(codes, y, K)
        assert gm <= 1e-10, gm
        _, _, _, fl = lr_newton(codes, y, K, gtol=0.0, max_iter=nit + 12)
        tg = float(np.abs(tight_sklearn(codes, y, K) - W).max())
        assert tg <= 1e-5, tg
        a_opt = auc_macro(lr_proba(W, codes, K), y, K)
        sj = 0.0
        for noisy in noisy_sets:
            Wn, _, gn, _ = lr_newton(noisy, y, K)
            assert gn <= 1e-10
            sj = max(sj, abs(auc_macro(lr_proba(Wn, noisy, K), y, K) - a_opt))
        dg = abs(ref_auc - a_opt)
        for _ in range(NOISE_DRAWS):                   # the reference alone stays within the bound the end-to-end test applies
            noisy = codes.copy()
            noisy[:, 1:] += rng2.uniform(-NOISE[kind] / 2, NOISE[kind] / 2, (n, 4))
            Wn, _, gn, _ = lr_newton(noisy, y, K)
            assert gn <= 1e-10 and abs(auc_macro(lr_proba(Wn, noisy, K), y, K) - ref_auc) <= dg + 4 * sj + 4 * n * np.finfo(float).eps
        out[f"fstat_coef_{j}"], out[f"fstat_intercept_{j}"], out[f"fstat_proba_{j}"], out[f"fstat_opt_{j}"] = l["coef"], l["intercept"], l["proba"], W
        Ks.append(K), its.append(nit), gmax.append(gm), floor.append(fl), tight_gap.append(tg), auc_opt.append(a_opt)
        default_w_gap.append(float(np.abs(sklearn_W(l["coef"], l["intercept"], K) - W).max()))
        default_gap.append(dg), sens.append(sj), n_iter.append(int(l["n_iter"].max())), warned.append(len(l["warned"]))
    out.update(fstat_K=np.array(Ks, dtype=np.int32), fstat_opt_iters=np.array(its, dtype=np.int32), fstat_opt_gmax=np.array(gmax),
               fstat_opt_floor=np.array(floor), fstat_tight_gap=np.array(tight_gap), fstat_default_w_gap=np.array(default_w_gap),
               fstat_auc_opt=np.array(auc_opt), fstat_default_gap=np.array(default_gap), fstat_sens=np.array(sens),
               fstat_n_iter=np.array(n_iter, dtype=np.int32), fstat_warned=np.array(warned, dtype=np.int32))
    return out


def main(kinds):
    for kind in kinds:
        out = make(kind)
        path = os.path.join(GOLD, f"score_fstat_{kind}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes; seed", int(out["seed"]), "modularity", float(out["fstat_modu"]), "explicitness",
              float(out["fstat_expl"]), out["fstat_expl_detail"][:, 0], "AUC at the optimum", out["fstat_auc_opt"], "default gap",
              out["fstat_default_gap"], "sens", out["fstat_sens"], "newton iters", out["fstat_opt_iters"], "gmax", out["fstat_opt_gmax"],
              "floor", out["fstat_opt_floor"], "tight gap", out["fstat_tight_gap"], "default W gap", out["fstat_default_w_gap"],
              "lbfgs n_iter", out["fstat_n_iter"], "warned", out["fstat_warned"], "near edge", out["fstat_near_edge"].sum(axis=0))


if __name__ == "__main__":
    main(sys.argv[1:] or ["dsprites", "colored"])

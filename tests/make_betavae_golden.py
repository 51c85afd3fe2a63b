"""Generate tests/golden/score_betavae_{dsprites,colored}.npz from the reference's own score/BetVAE.py (needs the reference tree; host only).

    python tests/make_betavae_golden.py [dsprites] [colored]

The scripts' load_data, encoders, add_color_2_img and BetaVAEMetric are loaded with oracle.ref_harness.load_defs and run unchanged on
torch-CPU on the first FV_GROUPS groups, against the synthetic archive, weights and seeds of tests/score_data.py (the sprites are read back
from score_{kind}.npz).  The ``LogisticRegression`` they see is a subclass that records its fit.  Next to the reference's numbers the file
holds ``bv_opt``, the float64 optimum of the same objective from the Newton iteration below, and the figures that say which groups a
representation within tolerance may move (``bv_margin``, ``bv_logit_sens``, ``bv_near``).  Only numbers are written out.
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

GOLD = msg.GOLD
GROUPS = msg.FV_GROUPS
NAMES = ("load_data", "Encoder", "Encoder_pxy", "transformation_2D", "load_encoder", "add_color_2_img", "BetaVAEMetric")
NOISE = {"dsprites": 2e-5, "colored": 2e-4}       # twice the representation tolerances of test_representation_matches_reference
NOISE_DRAWS = 10
NOISE_SEED = 21
TIE = 1e-6
MAX_SKIP = 1


def recording_classifier():
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import LogisticRegression

    class Recorded(LogisticRegression):
        log = {}

        def fit(self, X, y, sample_weight=None):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                super().fit(X, y, sample_weight)
            Recorded.log.update(features=np.array(X), labels=np.array(y), coef=self.coef_.copy(), intercept=self.intercept_.copy(),
                                n_iter=self.n_iter_.copy(), predict=self.predict(X), max_iter=self.max_iter, C=self.C,
                                warned=[str(w.message) for w in caught if issubclass(w.category, ConvergenceWarning)])
            return self

    return Recorded


def ref_globals(kind, classifier=None):
    from sklearn import metrics
    names = ("from_latent_vector_2_affine_para_pxy", "from_latent_vector_2_color_para_pxy", "get_matrix_pxy_align")
    u = rh.load_defs(f"{msg.DIRS[kind]}/utils_pxy.py", names)
    extra = {k: u[k] for k in names if k in u}
    extra.update(metrics=metrics, code_dim=7 if kind == "colored" else 4, n_classes=3, img_shape=(64, 64, 1), LogisticRegression=classifier)
    g = rh.load_defs(f"{msg.DIRS[kind]}/BetVAE.py", NAMES, extra=extra)
    g["trans_2D"] = g["transformation_2D"]()
    return g


# ---- the objective the reference's classifier minimises, in float64 numpy ---------------------------------------------------------
def objective(W, X, y, inv_C):
    """f = sum_i CE(softmax(W [x_i, 1]), y_i) + inv_C / 2 |coefficients|^2 and its gradient; W [K, d+1]"""
    n, d = X.shape
    Xt = np.concatenate([X, np.ones((n, 1))], 1)
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


def newton(X, y, K, inv_C=1.0, gtol=1e-13, max_iter=50):
    """damped Newton from W = 0 with v v^T (v = 1/sqrt(K) on each intercept) on the Hessian: the zero-sum-intercept optimum"""
    n, d = X.shape
    D = d + 1
    W = np.zeros((K, D))
    f, grad, p, Xt = objective(W, X, y, inv_C)
    for it in range(max_iter + 1):
        if np.abs(grad).max() <= gtol or it == max_iter:
            break
        H = np.zeros((K * D, K * D))
        for k in range(K):
            for l in range(K):
                w = p[:, k] * ((k == l) - p[:, l])
                H[k * D:(k + 1) * D, l * D:(l + 1) * D] = (Xt * w[:, None]).T @ Xt
        pen = np.tile(np.r_[np.full(d, inv_C), 0.0], K)
        H += np.diag(pen)
        v = np.tile(np.r_[np.zeros(d), 1.0 / np.sqrt(K)], K)
        H += np.outer(v, v)
        s = -np.linalg.solve(H, grad.reshape(-1)).reshape(K, D)
        gs = float(np.sum(grad * s))
        t = 1.0
        while True:
            fn, gn, pn, _ = objective(W + t * s, X, y, inv_C)
            if fn <= f + 1e-4 * t * gs + n * np.finfo(float).eps * abs(f) or t < 1e-12:
                break
            t *= 0.5
        W, f, grad, p = W + t * s, fn, gn, pn
    return W, it, float(np.abs(grad).max())


def plan_indices(kind, sizes, seed, groups_with_gains):
    """BetVAE load_data's plan read back through an archive whose images are their own indices, then (colored) the gains evaluate() would
    draw for the first ``groups_with_gains`` groups, through the script's own add_color_2_img; last the stream's next uniform draw"""
    g = ref_globals(kind)
    cls, lv = sd.latents_grid(sizes)
    N = lv.shape[0]
    with msg.workdir(np.arange(N, dtype=np.int64), lv, cls, {"latents_sizes": np.array(sizes, dtype=np.int64)}, {}, {}, kind):
        np.random.seed(seed)
        _, md, _, _ = g["load_data"]()
        gains = None
        if kind == "colored":
            L = md["groups"][0]["img"].shape[0]
            gains = np.stack([g["add_color_2_img"](torch.zeros(L, 1, 1, 1))[1].reshape(L, 3) for _ in range(groups_with_gains)])
        nxt = np.random.uniform()
    return np.stack([d["img"] for d in md["groups"]]), np.array([d["label"] for d in md["groups"]]), gains, nxt


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
    meta = {"latents_sizes": np.array(sizes, dtype=np.int64)}
    pxy, enc = msg.weights(kind)
    assert np.array_equal(sd.checksums(pxy), base["pxy_checksums"]) and np.array_equal(sd.checksums(enc), base["enc_checksums"])
    seed = int(base["seed"])
    out = {"seed": np.array(seed), "bv_groups": np.array(GROUPS)}

    # ---- the plan, at the fixture sizes and at the archive's ----
    gidx, labels, pgains, nxt = plan_indices(kind, sizes, seed, GROUPS)
    fg, fl, fgains, fnxt = plan_indices(kind, sd.FULL_SIZES, msg.FULL_SEED, 500)
    out.update(bv_group_idx=gidx.astype(np.uint16), bv_labels=labels.astype(np.int8), bv_plan_next=np.array(nxt),
               full_seed=np.array(msg.FULL_SEED), full_labels=fl.astype(np.int8), full_group_idx_head=fg[:4].astype(np.uint32),
               full_group_idx_sha256=np.array(sd.digest(fg)), full_plan_next=np.array(fnxt))
    if colored:
        out.update(full_group_gains_head=fgains[:2], full_group_gains_sha256=np.array(sd.digest(fgains)))

    # ---- module-level code of BetVAE.py on the first GROUPS groups ----
    Rec = recording_classifier()
    g = ref_globals(kind, Rec)
    colors = []
    outs = msg.recording(g, colors)
    with msg.workdir(imgs, lv, lc, meta, pxy, enc, kind):
        np.random.seed(seed)
        _, md, _, _ = g["load_data"]()
        md["groups"] = md["groups"][:GROUPS]
        res = g["BetaVAEMetric"](md).evaluate()
    log = Rec.log
    per_group = 2 if colored else 1                 # the colored script runs encoder_pxy twice per group
    assert len(outs["enc"]) == GROUPS and len(outs["pxy"]) == GROUPS * per_group
    grp, probs = [], []
    for i in range(GROUPS):
        cat, cont = outs["enc"][i]
        pc = outs["pxy"][i * per_group + per_group - 1]
        grp.append(np.concatenate((np.argmax(cat.numpy(), axis=1).reshape(-1, 1), cont.numpy()[:, 0:2], pc.numpy()[:, 1:3]), axis=1))
        probs.append(cat.numpy())
    grp, probs = np.stack(grp), np.stack(probs)
    feats = np.stack([np.mean(np.abs(x[0::2] - x[1::2]), axis=0) for x in grp])
    assert np.array_equal(feats, log["features"]) and np.array_equal(log["labels"], labels[:GROUPS])
    assert np.array_equal(np.stack([d["img"] for d in md["groups"]]), imgs[gidx[:GROUPS]])
    if colored:
        assert np.array_equal(np.stack(colors), pgains)
        out["bv_group_gains"] = pgains
    acc = res["betaVAE_metric"]
    assert acc == np.mean(log["predict"] == labels[:GROUPS])

    # ---- the optimum, and the checks that make it a target ----
    assert log["warned"] == [] and int(log["n_iter"].max()) < log["max_iter"] == 100 and log["C"] == 1.0, (log["warned"], log["n_iter"])
    classes, y = np.unique(labels[:GROUPS], return_inverse=True)
    K = classes.size
    assert np.array_equal(classes, np.arange(5))
    W, nit, gmax = newton(feats, y, K)
    assert gmax <= 1e-10, gmax
    tight = Rec(tol=1e-12, max_iter=10000)
    log_default = dict(log)
    tight.fit(feats, labels[:GROUPS])
    tight_gap = float(np.abs(np.concatenate([tight.coef_, tight.intercept_[:, None]], 1) - W).max())
    assert tight_gap <= 1e-5, tight_gap
    log = log_default
    default_gap = float(np.abs(np.concatenate([log["coef"], log["intercept"][:, None]], 1) - W).max())
    Xt = np.concatenate([feats, np.ones((GROUPS, 1))], 1)
    logits = Xt @ W.T
    pred_opt = classes[np.argmax(logits, axis=1)]
    skip = np.flatnonzero(pred_opt != log["predict"])
    assert skip.size <= MAX_SKIP, skip
    top = np.sort(logits, axis=1)
    margin = top[:, -1] - top[:, -2]
    rng = np.random.RandomState(NOISE_SEED)
    sens = 0.0
    for _ in range(NOISE_DRAWS):
        noisy = feats.copy()
        noisy[:, 1:] += rng.uniform(-NOISE[kind], NOISE[kind], (GROUPS, 4))
        Wn, _, gn = newton(noisy, y, K)
        assert gn <= 1e-10
        sens = max(sens, float(np.abs(np.concatenate([noisy, np.ones((GROUPS, 1))], 1) @ Wn.T - logits).max()))
    ps = np.sort(probs.astype(np.float64), axis=2)
    tie = ((ps[:, :, -1] - ps[:, :, -2]) <= TIE).any(axis=1)
    near = (margin < 4 * sens) | tie
    assert near.sum() <= 0.05 * GROUPS, (int(near.sum()), np.flatnonzero(near))
    gcat, gcols = msg.split(grp.reshape(-1, 5))
    out.update(bv_group_cat=gcat, bv_group_cols=gcols, bv_probs=probs.reshape(-1, probs.shape[-1]).astype(np.float32), bv_features=feats,
               bv_acc=np.array(acc), bv_predict=log["predict"].astype(np.int8), bv_coef=log["coef"], bv_intercept=log["intercept"],
               bv_n_iter=log["n_iter"].astype(np.int32), bv_opt=W, bv_opt_iters=np.array(nit), bv_opt_gmax=np.array(gmax),
               bv_tight_gap=np.array(tight_gap), bv_default_gap=np.array(default_gap), bv_margin=margin, bv_logit_sens=np.array(sens),
               bv_skip=skip.astype(np.int32), bv_tie=tie, bv_near=near)
    return out


def main(kinds):
    for kind in kinds:
        out = make(kind)
        path = os.path.join(GOLD, f"score_betavae_{kind}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes; acc", float(out["bv_acc"]), "n_iter", out["bv_n_iter"], "newton iters", int(out["bv_opt_iters"]),
              "gmax", float(out["bv_opt_gmax"]), "tight gap", float(out["bv_tight_gap"]), "default gap", float(out["bv_default_gap"]),
              "min margin", float(out["bv_margin"].min()), "sens", float(out["bv_logit_sens"]), "near", int(out["bv_near"].sum()),
              "skip", out["bv_skip"])


if __name__ == "__main__":
    main(sys.argv[1:] or ["dsprites", "colored"])

"""Generate tests/golden/score_dci_{dsprites,colored}.npz from the reference's own score/DCI.py (needs the reference tree; host only).

    python tests/make_dci_golden.py [dsprites] [colored]

The scripts' load_data, encoders, add_color_2_img and DCIMetric are loaded with oracle.ref_harness.load_defs (the scripts' own imports are
never executed: ``sklearn.ensemble.forest`` no longer exists) and run unchanged on torch-CPU against the synthetic archive, weights and
seeds of tests/score_data.py (the sprites are read back from score_{kind}.npz; N = 384, so the reference scores 38 samples).  Two things
are injected: the ``Lasso`` they see is a subclass that records its fits, and the archive's metadata also carries ``latents_names`` /
``latents_possible_values`` (make_sap_golden.metadata).  Next to the reference's numbers the file holds ``dci_opt``, the float64 optimum of
the objective Lasso minimises from the Gram-matrix coordinate descent below run to its rounding floor, how far the reference's default
fit (which stops at a duality gap of 1e-4 |y|^2) lies from it (``dci_default_gap``), and how far a representation within tolerance moves
the optimum (``dci_sens``).  Only numbers are written out.
"""
from __future__ import annotations

import importlib
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
import make_sap_golden as msp               # noqa: E402

GOLD = msg.GOLD
NAMES = ("load_data", "Encoder", "Encoder_pxy", "transformation_2D", "load_encoder", "add_color_2_img", "DCIMetric")
NOISE = mbg.NOISE
NOISE_DRAWS = mbg.NOISE_DRAWS
NOISE_SEED = mbg.NOISE_SEED
TIE = mbg.TIE
ALPHA = 0.02
K = 5                                       # code columns; the factor table has as many
# np.random.seed of the recorded run.  The base fixture's seed is tried first; a seed of this fixture's own stands here when the base
# seed's 38 samples do not meet the assertions of make() (None: the base seed does).
DCI_SEED = {"dsprites": None, "colored": None}
GAP_NAMES = ("W", "R", "disent_detail", "disent", "complete_detail", "complete")       # dci_default_gap; dci_sens holds the last five


def recording_regressor():
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.linear_model import Lasso

    class Recorded(Lasso):
        log = []

        def fit(self, X, y, *args, **kwargs):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                super().fit(X, y, *args, **kwargs)
            Recorded.log.append(dict(X=np.array(X), y=np.array(y), coef=self.coef_.copy(), intercept=float(self.intercept_),
                                     n_iter=int(self.n_iter_), alpha=self.alpha,
                                     warned=[str(w.message) for w in caught if issubclass(w.category, ConvergenceWarning)]))
            return self

    return Recorded


def ref_globals(kind, regressor=None):
    names = ("from_latent_vector_2_affine_para_pxy", "from_latent_vector_2_color_para_pxy", "get_matrix_pxy_align")
    u = rh.load_defs(f"{msg.DIRS[kind]}/utils_pxy.py", names)
    extra = {k: u[k] for k in names if k in u}
    extra.update(code_dim=7 if kind == "colored" else 4, n_classes=3, img_shape=(64, 64, 1), Lasso=regressor)
    g = rh.load_defs(f"{msg.DIRS[kind]}/DCI.py", NAMES, extra=extra)
    g["trans_2D"] = g["transformation_2D"]()
    return g


# ---- the objective the reference's regressor minimises, in float64 numpy on the Gram matrix ----------------------------------------
def normalize(X):
    """DCIMetric.normalize"""
    return (X - np.mean(X, 0)) / np.std(X, 0)


def gram(codes, latents):
    """G = Z^T Z / n of the normalised columns [codes | latents]"""
    Z = np.concatenate([normalize(np.asarray(codes, dtype=np.float64)), normalize(np.asarray(latents, dtype=np.float64))], 1)
    return Z.T @ Z / Z.shape[0]


def kkt_residual(A, c, w, alpha=ALPHA):
    """max_i ( w_i != 0 ? |g_i - alpha sign(w_i)| : max(|g_i| - alpha, 0) ), g = c - A w: zero exactly at the optimum of
    (G_yy - 2 c.w + w.A w) / 2 + alpha |w|_1"""
    g = c - A @ w
    return float(np.max(np.where(w != 0, np.abs(g - alpha * np.sign(w)), np.maximum(np.abs(g) - alpha, 0.0))))


def objective(A, c, gyy, w, alpha=ALPHA):
    return 0.5 * (gyy - 2.0 * float(c @ w) + float(w @ A @ w)) + alpha * float(np.abs(w).sum())


def lasso_cd(A, c, alpha=ALPHA, tol=0.0, max_sweeps=100000, patience=500):
    """cyclic coordinate descent with soft thresholding from w = 0 -> (w, sweeps, KKT residual).  The residual is tested before the first
    sweep and after each one; with tol = 0 the iteration runs to its rounding floor: it ends when a sweep leaves w as it was or when the
    residual has not improved for ``patience`` sweeps (it is not monotone: while weight moves between two nearly collinear codes it stays
    where it is for many sweeps), and the best point seen is returned."""
    k = c.size
    w = np.zeros(k)
    best = (np.inf, w.copy(), 0)
    for sweep in range(max_sweeps + 1):
        r = kkt_residual(A, c, w, alpha)
        if r < best[0]:
            best = (r, w.copy(), sweep)
        if r <= tol or sweep == max_sweeps or sweep - best[2] >= patience:
            break
        before = w.copy()
        for i in range(k):
            rho = c[i] - A[i] @ w + A[i, i] * w[i]
            w[i] = np.sign(rho) * max(abs(rho) - alpha, 0.0) / A[i, i]
        if np.array_equal(w, before):
            break
    return best[1], best[2], best[0]


def lasso_gram_fit_all(G, k, alpha=ALPHA, tol=0.0, max_sweeps=100000):
    """every target of G [(k+nf),(k+nf)] -> (W [nf,k], sweeps [nf], KKT residual [nf])"""
    nf = G.shape[0] - k
    W, sweeps, res = np.zeros((nf, k)), np.zeros(nf, dtype=np.int64), np.zeros(nf)
    for j in range(nf):
        W[j], sweeps[j], res[j] = lasso_cd(G[:k, :k], G[:k, k + j], alpha, tol, max_sweeps)
    return W, sweeps, res


def production_set(n=73728, seed=73728):
    """codes and factors of the reference's production shape: n = 73 728 samples, the five code columns (an integer-valued one, float32
    values correlated with the factors and with each other: the code block's condition number is 47), the five factor columns of the
    archive's value grids"""
    rng = np.random.RandomState(seed)
    shape = rng.randint(3, size=n).astype(np.float64)
    fv = np.stack([shape, rng.randint(6, size=n) / 5.0 * 0.5 + 0.5, rng.randint(40, size=n) * (2 * np.pi / 40), rng.randint(32, size=n) / 31.0,
                   rng.randint(32, size=n) / 31.0], 1)
    flip = rng.uniform(size=n) < 0.3
    cat = np.where(flip, rng.randint(3, size=n), shape)
    c1 = 2.0 * fv[:, 1] + 0.3 * rng.normal(size=n) + 0.2 * cat
    c2 = 0.3 * np.sin(fv[:, 2]) + 1.5 * c1 + 0.2 * rng.normal(size=n)
    c3 = fv[:, 3] - 0.5 + 0.05 * rng.normal(size=n) + 0.4 * (c2 - c2.mean())
    c4 = 0.5 - fv[:, 4] + 0.05 * rng.normal(size=n) + 0.9 * c3
    codes = np.stack([cat, c1, c2, c3, c4], 1).astype(np.float32).astype(np.float64)
    return codes, fv


def scores_of(R):
    """this package's host arithmetic on R [k,nf] -> (dict, the four scores as arrays in GAP_NAMES[2:] order)"""
    res = importlib.import_module("ead-gan_amd").score.dci_scores(R)
    return res, [np.array(res["DCI_Lasso_disent_metric_detail"]), np.array(res["DCI_Lasso_disent_metric"]),
                 np.array(res["DCI_Lasso_complete_metric_detail"]), np.array(res["DCI_Lasso_complete_metric"])]


def plan_indices(kind, sizes, seed):
    """DCI load_data's plan read back through an archive whose images are their own indices, then (colored) the gains evaluate() would draw,
    through the script's own add_color_2_img; last the stream's next uniform draw"""
    g = ref_globals(kind)
    cls, lv = sd.latents_grid(sizes)
    N = lv.shape[0]
    with msg.workdir(np.arange(N, dtype=np.int64), lv, cls, msp.metadata(sizes), {}, {}, kind):
        np.random.seed(seed)
        _, md, _, _ = g["load_data"]()
        d = md["img_with_latent"]
        n = d["img"].shape[0]
        gains = g["add_color_2_img"](torch.zeros(n, 1, 1, 1))[1].reshape(n, 3) if kind == "colored" else None
        nxt = np.random.uniform()
    return d["img"].astype(np.int64), d["latent"], d["latent_id"], gains, nxt


def production_floor():
    """the KKT floor of the numpy coordinate descent on the production-sized set"""
    codes, fv = production_set()
    _, sweeps, res = lasso_gram_fit_all(gram(codes, fv), K)
    return float(res.max()), int(sweeps.max())


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
    meta = msp.metadata(sizes)
    pxy, enc = msg.weights(kind)
    assert np.array_equal(sd.checksums(pxy), base["pxy_checksums"]) and np.array_equal(sd.checksums(enc), base["enc_checksums"])
    seed = int(base["seed"]) if DCI_SEED[kind] is None else DCI_SEED[kind]
    out = {"seed": np.array(seed), "base_seed": np.array(int(base["seed"]))}

    # ---- the plan, at the fixture sizes and at the archive's ----
    idx, latents, lat_id, pgains, nxt = plan_indices(kind, sizes, seed)
    n = idx.size
    assert n == N // 10 == 38
    fi, fl, fid, fgains, fnxt = plan_indices(kind, sd.FULL_SIZES, msg.FULL_SEED)
    out.update(dci_idx=idx.astype(np.uint16), dci_latent_ids=lat_id.astype(np.int8), dci_latents=latents, dci_plan_next=np.array(nxt),
               full_seed=np.array(msg.FULL_SEED), full_n=np.array(fi.size), full_idx_head=fi[:64].astype(np.uint32),
               full_idx_sha256=np.array(sd.digest(fi)), full_latent_ids_sha256=np.array(sd.digest(fid)), full_latents_head=fl[:8],
               full_latents_sha256=np.array(sd.digest(fl)), full_plan_next=np.array(fnxt))
    if colored:
        out.update(dci_gains=pgains, full_gains_head=fgains[:8], full_gains_sha256=np.array(sd.digest(fgains)))

    # ---- module-level code of DCI.py ----
    Rec = recording_regressor()
    g = ref_globals(kind, Rec)
    colors = []
    outs = msg.recording(g, colors)
    with msg.workdir(imgs, lv, lc, meta, pxy, enc, kind):
        np.random.seed(seed)
        _, md, _, _ = g["load_data"]()
        res = g["DCIMetric"](md).evaluate()
    log = list(Rec.log)
    assert len(outs["enc"]) == 1 and len(outs["pxy"]) == 1 and len(log) == 5
    codes, probs = msg.rows(outs, 0)
    d = md["img_with_latent"]
    assert np.array_equal(d["img"], imgs[idx]) and np.array_equal(d["latent"], latents) and np.array_equal(d["latent_id"], lat_id)
    if colored:
        assert len(colors) == 1 and np.array_equal(colors[0], pgains)
    assert (np.std(codes, 0) > 0).all() and (np.std(latents, 0) > 0).all(), (np.std(codes, 0), np.std(latents, 0))
    Z, Y = normalize(codes), normalize(latents)
    for j, l in enumerate(log):
        assert np.array_equal(l["X"], Z) and np.array_equal(l["y"], Y[:, j])
        assert l["alpha"] == ALPHA and l["warned"] == [] and abs(l["intercept"]) <= 1e-12, l
    ref_W = np.stack([l["coef"] for l in log])                                     # [nf, k]
    R = res["DCI_Lasso_metric_detail"]
    assert np.array_equal(R, np.abs(ref_W).T) and np.isfinite(R).all(), R
    ps = np.sort(probs.astype(np.float64), axis=1)
    tie = (ps[:, -1] - ps[:, -2]) <= TIE
    assert not tie.any(), np.flatnonzero(tie)      # a cat tie would move column 0 as a whole: take another seed
    mine, ref_scores = scores_of(R)
    assert sorted(mine) == sorted(res)
    for key in res:                                # the recorded dict from this package's host arithmetic, bit for bit
        assert np.array_equal(np.asarray(mine[key]), np.asarray(res[key]), equal_nan=True), key
    assert all(np.isfinite(s).all() for s in ref_scores), ref_scores

    # ---- the optimum, how far the default fit lies from it, and what a representation within tolerance moves ----
    G = gram(codes, latents)
    W, sweeps, kkt = lasso_gram_fit_all(G, K)
    assert kkt.max() <= 1e-14, kkt
    _, opt_scores = scores_of(np.abs(W).T)
    default_gap = np.array([np.abs(ref_W - W).max(), np.abs(R - np.abs(W).T).max()] +
                           [np.abs(a - b).max() for a, b in zip(ref_scores, opt_scores)])
    rng = np.random.RandomState(NOISE_SEED)
    sens = np.zeros(5)
    for _ in range(NOISE_DRAWS):
        noisy = codes.copy()
        noisy[:, 1:] += rng.uniform(-NOISE[kind], NOISE[kind], (n, 4))
        Wn, _, kn = lasso_gram_fit_all(gram(noisy, latents), K)
        assert kn.max() <= 1e-14
        _, ns = scores_of(np.abs(Wn).T)
        sens = np.maximum(sens, [np.abs(np.abs(Wn) - np.abs(W)).max()] + [np.abs(a - b).max() for a, b in zip(ns, opt_scores)])
    cat, cols = msg.split(codes)
    out.update(dci_cat=cat, dci_cols=cols, dci_probs=probs.astype(np.float32), dci_coef=ref_W,
               dci_intercept=np.array([l["intercept"] for l in log]), dci_n_iter=np.array([l["n_iter"] for l in log], dtype=np.int32),
               dci_alpha=np.array(ALPHA), dci_R=R, dci_disent_detail=ref_scores[0], dci_disent=ref_scores[1],
               dci_complete_detail=ref_scores[2], dci_complete=ref_scores[3], dci_G=G, dci_opt=W, dci_opt_sweeps=sweeps.astype(np.int32),
               dci_opt_kkt=kkt, dci_default_gap=default_gap, dci_sens=sens)
    return out


def main(kinds):
    floor, sweeps = production_floor()
    print("production-sized set: KKT floor", floor, "after at most", sweeps, "sweeps")
    for kind in kinds:
        out = make(kind)
        path = os.path.join(GOLD, f"score_dci_{kind}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes; seed", int(out["seed"]), "disent", float(out["dci_disent"]), "complete",
              float(out["dci_complete"]), "sklearn n_iter", out["dci_n_iter"], "optimum sweeps", out["dci_opt_sweeps"], "KKT floor",
              out["dci_opt_kkt"].max(), "default gap", dict(zip(GAP_NAMES, out["dci_default_gap"])), "sens",
              dict(zip(GAP_NAMES[1:], out["dci_sens"])))


if __name__ == "__main__":
    main(sys.argv[1:] or ["dsprites", "colored"])

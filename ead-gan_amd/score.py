"""Disentanglement scores of a trained dSprites / colored-dSprites encoder pair on the MI355X: MIG, FactorVAE, BetaVAE, SAP, F-stat and
DCI (dSprites/score/MIG.py, FactorVAE.py, BetVAE.py, SAP.py, F_score.py, DCI.py; colored_dSprites/score/ likewise).

The reference pushes every sampled image through Encoder_pxy -> inverse translation -> grid_sample(padding_mode='zeros') [-> divide by
the colour gains] -> Encoder (eval) on the CPU and scores the rows [argmax(cat), cont0, cont1, pxy1, pxy2] with numpy / sklearn.  Here the
sampling plan is host numpy (the reference's draws, in its order), the dataset sits in HBM as uint8, the encoder passes run in fixed-size
chunks on the existing engines, and the metric arithmetic runs in float64 kernels (csrc/score.hip, score_fstat.hip, score_dci.hip).
Only the plan goes up and only the metric's scalars / small matrices come down.  There is no CPU fallback.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import colored as cd
from . import dsprites as ds
from . import ops
from .engine import _require_cuda

NUM_CODES = 5           # [argmax(cat), cont0, cont1, pxy1, pxy2] for both workloads
KINDS = ("dsprites", "colored")


# ================================================================================================
# sampling plans (host numpy, bit for bit the reference's draws)
# ================================================================================================
def _rs(rng):
    return np.random if rng is None else rng


def mig_plan(N, colored=False, rng=None, num_points=1000, batch_size=16):
    """generate_batch_factor_code's draws (MIG.py:206-212): per batch of 16 ``randint(N, size=16)`` then, colored, the batch's RGB gains
    ``uniform(0.5, 1, [16,3,1,1])`` (add_color_2_img).  -> {"idx": int64 [num_points], "gains": float64 [num_points,3] or None}"""
    r = _rs(rng)
    idx, gains = [], []
    i = 0
    while i < num_points:
        k = min(num_points - i, batch_size)
        idx.append(r.randint(N, size=k))
        if colored:
            gains.append(r.uniform(0.5, 1, [k, 3, 1, 1]).reshape(k, 3))
        i += k
    return {"idx": np.concatenate(idx), "gains": np.concatenate(gains) if colored else None}


def latents_bases(latents_sizes):
    s = np.asarray(latents_sizes)
    return np.concatenate((s[::-1].cumprod()[::-1][1:], np.array([1, ])))


def _group_draws(r, latents_sizes, L, M):
    """The group loop load_data runs in FactorVAE.py:36-69 and BetVAE.py:27-69 (the same code): group i fixes latent i % 5 + 1 (one randint
    per latent for L samples, then the fixed latent redrawn once).  -> (group_idx int64 [M,L], labels int64 [M])"""
    sizes = np.asarray(latents_sizes)
    bases = latents_bases(sizes)
    group_idx = np.empty((M, L), dtype=np.int64)
    labels = np.empty(M, dtype=np.int64)
    for i in range(M):
        fixed = i % 5 + 1
        samples = np.zeros((L, sizes.size))
        for lat_i, lat_size in enumerate(sizes):
            samples[:, lat_i] = r.randint(lat_size, size=L)
        samples[:, fixed] = r.randint(sizes[fixed], size=1)
        group_idx[i] = np.dot(samples, bases).astype(int)
        labels[i] = fixed - 1
    return group_idx, labels


def _group_gains(r, L, M):
    """evaluate()'s add_color_2_img draw of each group, in group order -> float64 [M,L,3]"""
    return np.stack([r.uniform(0.5, 1, [L, 3, 1, 1]).reshape(L, 3) for _ in range(M)])


def factor_vae_plan(latents_sizes, N, colored=False, rng=None, L=100, M=500):
    """load_data's plan (FactorVAE.py:36-97): the group draws, then the eval set ``permutation(N)[:N/10]``; colored, evaluate() then draws
    the eval set's gains and each group's, in group order.
    -> {"group_idx" int64 [M,L], "labels" int64 [M], "eval_idx" int64 [N/10] (+ "eval_gains", "group_gains" float64)}"""
    r = _rs(rng)
    group_idx, labels = _group_draws(r, latents_sizes, L, M)
    eval_idx = r.permutation(range(N))[0:int(N / 10)]
    plan = {"group_idx": group_idx, "labels": labels, "eval_idx": eval_idx}
    if colored:
        plan["eval_gains"] = r.uniform(0.5, 1, [eval_idx.size, 3, 1, 1]).reshape(-1, 3)
        plan["group_gains"] = _group_gains(r, L, M)
    return plan


def beta_vae_plan(latents_sizes, N, colored=False, rng=None, L=100, M=500):
    """load_data's plan (BetVAE.py:27-82): FactorVAE's group draws, then the ``permutation(N)`` the script draws and never uses (consumed
    here so that the stream stands where the script's does); colored, evaluate() then draws each group's gains in group order -- no eval
    set comes before them, so they are not factor_vae_plan's.  -> {"group_idx" int64 [M,L], "labels" int64 [M] (+ "group_gains" [M,L,3])}"""
    r = _rs(rng)
    group_idx, labels = _group_draws(r, latents_sizes, L, M)
    r.permutation(range(N))
    plan = {"group_idx": group_idx, "labels": labels}
    if colored:
        plan["group_gains"] = _group_gains(r, L, M)
    return plan


def sap_plan(latents_sizes, N, colored=False, rng=None, L=100, M=500):
    """load_data's plan (SAP.py:61-85): FactorVAE's group draws and the ``permutation(N)``, both drawn and never used by the score (consumed
    here so that the stream stands where the script's does), then ``sample_latent(size=N // 10)``: one randint per latent; colored,
    evaluate() then draws the samples' gains once.  -> {"latent_ids" int [n,6], "idx" int64 [n], "gains" float64 [n,3] or None}"""
    r = _rs(rng)
    sizes = np.asarray(latents_sizes)
    _group_draws(r, sizes, L, M)
    r.permutation(range(N))
    n = int(N / 10)
    samples = np.zeros((n, sizes.size))
    for lat_i, lat_size in enumerate(sizes):
        samples[:, lat_i] = r.randint(lat_size, size=n)
    latent_ids = samples.astype(np.int32)
    idx = np.dot(latent_ids, latents_bases(sizes)).astype(int)
    gains = r.uniform(0.5, 1, [n, 3, 1, 1]).reshape(n, 3) if colored else None
    return {"latent_ids": latent_ids, "idx": idx, "gains": gains}


def fstat_plan(latents_sizes, N, colored=False, rng=None, L=100, M=500):
    """load_data's plan (F_score.py:37-112): the function is SAP.py's line for line, and evaluate() draws the samples' gains once
    (colored F_score.py:296), so the draws are ``sap_plan``'s.  The score's ground truth is the sampled latent ids without the color
    column (F_score.py:104,308).  -> sap_plan's dict + {"latent_id": int32 [n,5]}"""
    plan = sap_plan(latents_sizes, N, colored, rng, L, M)
    plan["latent_id"] = plan["latent_ids"][:, 1:]
    return plan


def dci_plan(latents_sizes, N, colored=False, rng=None, L=100, M=500):
    """load_data's plan (DCI.py:36-111): the function is SAP.py's line for line, and evaluate() draws the samples' gains once (colored
    DCI.py:351), so the draws are ``sap_plan``'s; the factor table is ``sap_latents`` of its ids.  -> sap_plan's dict"""
    return sap_plan(latents_sizes, N, colored, rng, L, M)


def sap_latents(latent_ids, latents_names, latents_possible_values):
    """The factor table of load_data (SAP.py:87-97): the archive's value of every sampled latent id, the color column dropped and the
    shape column minus 1 -> float64 [n,5] (shape 0..2, scale, orientation, posX, posY)"""
    ids = np.asarray(latent_ids)
    out = np.zeros((ids.shape[0], 6))
    for i in range(6):
        out[:, i] = np.asarray(latents_possible_values[latents_names[i]])[ids[:, i]]
    if not (np.all(out[:, 0] == 1) and np.min(out[:, 1]) == 1 and np.max(out[:, 1]) == 3):
        raise ValueError("the sampled latents do not span color 1 and shapes 1..3 (SAP.py:92-94 asserts it)")
    out = out[:, 1:]
    out[:, 0] -= 1.0
    return out


# ================================================================================================
# representation: chunked encoder passes -> float64 rows
# ================================================================================================
@contextlib.contextmanager
def _eval_mode(*mods):
    modes = [m.training for m in mods]
    try:
        for m in mods:
            m.eval()
        yield
    finally:
        for m, t in zip(mods, modes):
            m.train(t)


class Representation:
    """The reference's representation function (MIG.py:214-243, FactorVAE.py:246-266 / 283-303; colored variants with the gain division)
    over a uint8 sprite table in HBM, ``batch`` images per chunk on engines built once for that batch."""

    def __init__(self, encoder_pxy, encoder, kind, batch=4096):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        self.P, self.E, self.kind, self.B = encoder_pxy, encoder, kind, int(batch)
        self.C = 3 if kind == "colored" else 1
        if encoder.channels != self.C or encoder_pxy.channels != self.C:
            raise ValueError(f"{kind} scores need {self.C}-channel encoders")
        p = next(encoder.parameters())
        _require_cuda(p)
        dev = p.device
        self.nout = encoder_pxy.fc1.weight.shape[0]
        self.ncat, self.cdim = encoder.n_classes, encoder.code_dim
        B, C = self.B, self.C
        self.img = torch.zeros(B, C, 64, 64, device=dev)
        self.warped = torch.zeros(B, C, 64, 64, device=dev)
        self.align = torch.zeros(B, C, 64, 64, device=dev) if self.C == 3 else self.warped
        self.theta = torch.zeros(B, 2, 3, device=dev)
        self.device = dev

    def _chunk(self, data, idx, gains, nb, out):
        B, C = self.B, self.C
        ops.score_stage_u8(data, idx, gains, self.img, nb, C, 64 * 64)
        pcode = self.pe.forward(self.img)                                           # [B, 3|6] = p,x,y(,r,g,b)
        ops.theta_pxy_align_inv(pcode, self.nout, B, self.theta)                    # inverse(get_matrix_pxy_align(code))[:, 0:2]
        ops.warp_affine_zeros(self.img, self.theta, self.warped, B, C, 64, 64)      # trans_2D, padding_mode='zeros' (score/MIG.py:136)
        if C == 3:
            ops.color_scale(self.warped, pcode, self.nout, 3, 0.1, True, self.align, B, 3, 64 * 64)    # / (align_code[:,3:] * .1 + 1)
        outs = self.ee.forward([self.align], 0, training=False, patches=False)
        ops.score_rows(outs["cat_layer.0"], self.ncat, self.ncat, outs["cont_layer.0"], self.cdim, pcode, self.nout, nb, out)

    def codes(self, dataset_u8, idx, gains=None, out=None):
        """dataset_u8: device uint8 [N,64,64] (or [N,1,64,64]) {0,1} sprites; idx: [n] indices; gains: [n,3] RGB gains (colored).
        -> device float64 [n,5] rows (``out`` when given)."""
        _require_cuda(dataset_u8)
        if dataset_u8.dtype != torch.uint8 or dataset_u8[0].numel() != 64 * 64:
            raise ValueError("dataset_u8 must be uint8 [N,64,64]")
        data = dataset_u8.contiguous()
        N = data.shape[0]
        idx_h = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).reshape(-1)
        n = idx_h.size
        if n and (idx_h.min() < 0 or idx_h.max() >= N):
            raise IndexError(f"sample index out of range [0, {N})")
        if (gains is None) != (self.C == 1):
            raise ValueError("colored scores need per-sample gains; dSprites scores take none")
        dev = self.device
        idx_d = torch.from_numpy(idx_h.astype(np.int32)).to(dev)
        g_d = None
        if gains is not None:
            g_h = np.asarray(gains.cpu() if torch.is_tensor(gains) else gains).reshape(n, 3)
            g_d = torch.from_numpy(g_h.astype(np.float32)).to(dev)               # float32(gain): the reference's img.float()
        if out is None:
            out = torch.empty(n, NUM_CODES, device=dev, dtype=torch.float64)
        with _eval_mode(self.P, self.E):
            self.pe = self.P.fresh_engine(self.B)
            self.ee = self.E.fresh_engine(self.B)
            for off in range(0, n, self.B):
                nb = min(self.B, n - off)
                self._chunk(data, idx_d[off:], None if g_d is None else g_d[off:], nb, out[off:])
        return out


# ================================================================================================
# metrics
# ================================================================================================
def discretize(codes, num_bins=20):
    """make_discretizer(codes.T, num_bins) (MIG.py:270-275) -> device int32 [5, n] bins in 1..num_bins."""
    _require_cuda(codes)
    codes = codes.to(torch.float64).contiguous()
    n, k = codes.shape
    bins = torch.empty(k, n, device=codes.device, dtype=torch.int32)
    ops.score_digitize(codes, n, k, num_bins, bins)
    return bins


def _discrete_mi(codes, factor_values, num_bins=20):
    """discrete_mutual_info / discrete_entropy of device codes [n,k] (discretised here) against host factor values [n,nf], which become
    class ids with ``np.unique(return_inverse=True)``, the partition mutual_info_score builds.  -> (m [k,nf], H [nf]) host float64"""
    bins = discretize(codes, num_bins)
    k, n = bins.shape
    fv = np.asarray(factor_values)
    if fv.ndim != 2 or fv.shape[0] != n:
        raise ValueError(f"factor values {fv.shape} do not give {n} codes a row of factors each")
    ys, kmax = [], 1
    for j in range(fv.shape[1]):
        u, inv = np.unique(fv[:, j], return_inverse=True)
        ys.append(inv.reshape(-1).astype(np.int32))
        kmax = max(kmax, u.size)
    nf = len(ys)
    dev = codes.device
    ys_d = torch.from_numpy(np.stack(ys)).to(dev)
    ws = torch.empty(ops.score_mig_ws_ints(k, nf, kmax, num_bins), device=dev, dtype=torch.int32)
    mi = torch.empty(k * nf + nf, device=dev, dtype=torch.float64)
    ops.score_mig(bins, k, ys_d, nf, n, kmax, num_bins, ws, mi)
    mi = mi.cpu().numpy()
    return mi[:k * nf].reshape(k, nf), mi[k * nf:]


def mig(codes, factor_values, num_bins=20):
    """MIG of device codes [n,5] against host factor values [n,nf] (MIG.py:304-311).  -> (score, m [5,nf], H [nf])"""
    m, H = _discrete_mi(codes, factor_values, num_bins)
    sorted_m = np.sort(m, axis=0)[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.mean(np.divide(sorted_m[0, :] - sorted_m[1, :], H[:]))
    return float(score), m, H


def factor_vae_votes(eval_codes, group_codes, labels, num_labels):
    """Device part of FactorVAEMetric.evaluate (FactorVAE.py:269-312): eval_std = np.std(eval rows, axis=0), per group the argmin of
    np.std(group rows / eval_std, axis=0), votes[argmin, label] += 1.  group_codes [M*L,5] or [M,L,5].
    -> (eval_std float64 [5], predict int32 [M], votes int64 [5, num_labels]) on the device"""
    _require_cuda(eval_codes)
    ev = eval_codes.to(torch.float64).contiguous()
    labels = np.asarray(labels).reshape(-1)
    M = labels.size
    gc = group_codes.to(torch.float64).contiguous().reshape(M, -1, NUM_CODES)
    L = gc.shape[1]
    if labels.min() < 0 or labels.max() >= num_labels:
        raise ValueError("group labels must lie in [0, num_labels)")
    dev = ev.device
    eval_std = torch.empty(NUM_CODES, device=dev, dtype=torch.float64)
    ops.score_col_std(ev, ev.shape[0], NUM_CODES, eval_std)
    predict = torch.empty(M, device=dev, dtype=torch.int32)
    votes = torch.empty(NUM_CODES, num_labels, device=dev, dtype=torch.int64)
    ops.score_fvae_votes(gc, L, M, NUM_CODES, eval_std, torch.from_numpy(labels.astype(np.int32)).to(dev), num_labels, predict, votes)
    return eval_std, predict, votes


def factor_vae(eval_codes, group_codes, labels, num_labels):
    """-> the reference's dict: factorVAE_metric, factorVAE_metric_revised, factorVAE_metric_detail (FactorVAE.py:314-330)."""
    _, _, votes = factor_vae_votes(eval_codes, group_codes, labels, num_labels)
    train_data = votes.cpu().numpy().astype(np.float64)
    total_sample = np.sum(train_data)
    maxs = np.amax(train_data, axis=1)
    correct_sample = np.sum(maxs)
    correct_sample_revised = np.sum(np.flip(np.sort(maxs), axis=0)[0:train_data.shape[1]])
    return {"factorVAE_metric": float(correct_sample) / total_sample,
            "factorVAE_metric_revised": float(correct_sample_revised) / total_sample,
            "factorVAE_metric_detail": train_data}


def _class_ids(y, n, dev):
    """class ids y [n] (host or device) -> contiguous int32 [n] on ``dev``"""
    y_d = (y if torch.is_tensor(y) else torch.from_numpy(np.asarray(y).reshape(-1))).to(device=dev, dtype=torch.int32).contiguous()
    if y_d.numel() != n:
        raise ValueError(f"{y_d.numel()} labels for {n} rows")
    return y_d


def logreg_fit(X, y, K, C=1.0, max_iter=50, gtol=1e-10):
    """The optimum of sklearn's multinomial LogisticRegression(C) on device X [n,d] float64 and class ids y [n] in 0..K-1 (host or device):
    ``softmax_fit`` and its training predictions.  ``gtol`` bounds the gradient's inf-norm of the summed objective.  3 <= K <= 64,
    K (d + 1) <= 256; K = 2 is refused, because the prediction kernel reads K weight rows and the binomial fit has one.
    -> (W f64 [K,d+1] (coefficients | intercept), predict int32 [n], correct int64 [1]) on the device, info (host float64: iterations,
    final |g|inf, objective, status).  Raises RuntimeError when the solver did not reach gtol."""
    if K == 2:
        raise RuntimeError("logreg_fit: K = 2 classes: sklearn fits two classes in the binomial form, whose one weight row has no "
                           "argmax (softmax_fit fits it)")
    _require_cuda(X)
    X = X.to(torch.float64).contiguous()
    n, d = X.shape
    dev = X.device
    y_d = _class_ids(y, n, dev)
    W, info_h = softmax_fit(X, y_d, K, C, max_iter, gtol)
    predict = torch.empty(n, device=dev, dtype=torch.int32)
    correct = torch.empty(1, device=dev, dtype=torch.int64)
    ops.score_logreg_accuracy(X, y_d, n, d, K, W, predict, correct)
    return W, predict, correct, info_h


def beta_vae_fit(group_codes, labels, C=1.0, max_iter=50, gtol=1e-10):
    """Device part of BetaVAEMetric.evaluate (BetVAE.py:256-268): features[g] = np.mean(np.abs(x_g[0::2] - x_g[1::2]), axis=0) bit for
    bit, then ``logreg_fit`` on (features, labels) and its training predictions.  group_codes [M*L,5] or [M,L,5]; labels become class
    ids with np.unique(return_inverse=True).
    -> {"features" f64 [M,5], "W" f64 [K,6], "predict" int32 [M] class ids, "correct" int64 [1]} on the device, "classes", "info" (host)"""
    labels = np.asarray(labels).reshape(-1)
    M = labels.size
    classes, y = np.unique(labels, return_inverse=True)
    K = classes.size
    if K < 3:
        raise ValueError(f"the BetaVAE score fits a multinomial model: {K} distinct labels, at least 3 needed")
    if group_codes.numel() % (M * NUM_CODES):
        raise ValueError(f"{group_codes.numel()} code values do not make {M} groups of rows of {NUM_CODES}")
    L = group_codes.numel() // (M * NUM_CODES)
    if L % 2:
        raise ValueError(f"the BetaVAE score pairs each group's rows: L = {L} is odd")
    _require_cuda(group_codes)
    gc = group_codes.to(torch.float64).contiguous().reshape(M, L, NUM_CODES)
    feat = torch.empty(M, NUM_CODES, device=gc.device, dtype=torch.float64)
    ops.score_pair_absdiff_mean(gc, L, M, NUM_CODES, feat)
    W, predict, correct, info = logreg_fit(feat, y.reshape(-1), K, C, max_iter, gtol)
    return {"features": feat, "W": W, "predict": predict, "correct": correct, "classes": classes, "info": info}


def beta_vae(group_codes, labels, C=1.0):
    """-> the reference's dict {"betaVAE_metric": acc}: classifier.score(features, labels) of BetVAE.py:265-272."""
    fit = beta_vae_fit(group_codes, labels, C)
    return {"betaVAE_metric": int(fit["correct"].item()) / fit["predict"].numel()}


def svc1_fit(X, y, K, C=0.01, max_iter=50, gtol=1e-10):
    """The optimum of sklearn's LinearSVC(C, class_weight="balanced") (its defaults: L2 penalty, squared hinge, one-vs-rest, regularised
    intercept) for each one-feature column of device X [n,P] float64 (or [n]) against class ids y [n] in 0..K-1 (host or device), by
    eg_score_svc1_fit's float64 generalised Newton iteration, and the training predictions.  ``gtol`` bounds the gradient's inf-norm of
    every one-vs-rest problem.  -> (W f64 [P,K,2] (w, b), predict int32 [P,n], correct int64 [P]) on the device, info (host float64
    [P,K,4]: iterations, final |g|inf, objective, status).  Raises RuntimeError when a problem did not reach gtol."""
    if K < 3:
        raise ValueError(f"svc1_fit fits one-vs-rest problems of K >= 3 classes (liblinear fits K = 2 as a single problem), got K = {K}")
    _require_cuda(X)
    X = X.to(torch.float64)
    X = (X.reshape(-1, 1) if X.dim() == 1 else X).contiguous()
    n, P = X.shape
    dev = X.device
    y_d = _class_ids(y, n, dev)
    W = torch.empty(P, K, 2, device=dev, dtype=torch.float64)
    info = torch.empty(P, K, 4, device=dev, dtype=torch.float64)
    ops.score_svc1_fit(X, y_d, n, P, K, float(C), max_iter, gtol, W, info)
    predict = torch.empty(P, n, device=dev, dtype=torch.int32)
    correct = torch.empty(P, device=dev, dtype=torch.int64)
    ops.score_svc1_accuracy(X, y_d, n, P, K, W, predict, correct)
    info_h = info.cpu().numpy()                                                    # the one sync: offline evaluation
    if (info_h[:, :, 3] != 0).any():
        p, k = (int(v[0]) for v in np.nonzero(info_h[:, :, 3]))
        st = int(info_h[p, k, 3])
        raise RuntimeError(f"linear SVC fit of column {p}, class {k} did not reach |g|inf <= {gtol:g}: {int(info_h[p, k, 0])} iterations, "
                           f"|g|inf = {info_h[p, k, 1]:.3e} (status {st}: {ops.SVC_STATUS.get(st, '?')})")
    return W, predict, correct, info_h


def sap_matrix(codes, latents, is_continuous, C=0.01):
    """SAPMetric.evaluate's score matrix (SAP.py:286-306) of device codes [n,k] against factor values [n,nf] (host or device): a continuous
    factor's column holds the squared correlations of eg_score_sq_corr, a discrete one's the training accuracy of ``svc1_fit`` on each
    code column alone (the factor's values cast to int32 as the script casts them, class ids by np.unique).
    -> (device float64 [k,nf], {factor j: {"W", "predict", "correct" (device), "classes", "info" (host)}})"""
    _require_cuda(codes)
    codes = codes.to(torch.float64).contiguous()
    n, k = codes.shape
    dev = codes.device
    fv_h = np.asarray(latents.cpu() if torch.is_tensor(latents) else latents, dtype=np.float64)
    if fv_h.ndim != 2 or fv_h.shape[0] != n or fv_h.shape[1] != len(is_continuous):
        raise ValueError(f"factor values {fv_h.shape} do not match {n} codes and {len(is_continuous)} factors")
    nf = fv_h.shape[1]
    fv = torch.from_numpy(np.ascontiguousarray(fv_h)).to(dev)
    R = torch.empty(k, nf, device=dev, dtype=torch.float64)
    ops.score_sq_corr(codes, n, k, fv, nf, R)                                     # the discrete factors' columns are overwritten below
    fits = {}
    for j, cont in enumerate(is_continuous):
        if cont:
            continue
        classes, y = np.unique(fv_h[:, j].astype(np.int32), return_inverse=True)
        W, predict, correct, info = svc1_fit(codes, y.reshape(-1), classes.size, C)
        R[:, j] = correct.to(torch.float64) / n                                   # np.mean(pred == gt_values)
        fits[j] = {"W": W, "predict": predict, "correct": correct, "classes": classes, "info": info}
    return R, fits


def sap(codes, latents, is_continuous):
    """-> the reference's dict {"SAP_metric", "SAP_metric_detail"} (SAP.py:307-314): per factor the gap between the two best codes"""
    R, _ = sap_matrix(codes, latents, is_continuous)
    score_matrix = R.cpu().numpy()
    sorted_score_matrix = np.sort(score_matrix, axis=0)
    score = np.mean(sorted_score_matrix[-1, :] - sorted_score_matrix[-2, :])
    return {"SAP_metric": score, "SAP_metric_detail": score_matrix}


SAP_IS_CONTINUOUS = (False, True, True, True, True)          # shape, scale, orientation, posX, posY (SAP.py:103)


# default |g|inf of softmax_fit: 100 x the largest floor the float64 numpy solver reaches on the production-sized set (6.43e-13) and the
# fixtures (<= 6.7e-16)
SOFTMAX_GTOL = 6.5e-11


def softmax_fit(X, y, K, C=1.0, max_iter=50, gtol=SOFTMAX_GTOL):
    """The optimum of sklearn's LogisticRegression(C) on device X [n,d] float64 and class ids y [n] in 0..K-1 (host or device) by
    eg_score_softmax_fit's float64 Newton iteration: the multinomial objective for K >= 3, the binomial form sklearn fits for K = 2
    (one weight row).  2 <= K <= 64, K (d + 1) <= 256.  ``gtol`` bounds the gradient's inf-norm of the summed objective.  Blocks: the
    host reads the solver's decision record after every trial.
    -> (W f64 [K,d+1] ([1,d+1] for K = 2; coefficients | intercept) on the device, info (host float64: iterations, final |g|inf,
    objective, status)).  Raises RuntimeError when the solver did not reach gtol."""
    _require_cuda(X)
    X = X.to(torch.float64).contiguous()
    n, d = X.shape
    dev = X.device
    y_d = _class_ids(y, n, dev)
    ws = torch.empty(max(ops.score_softmax_ws_bytes(n, d, K), 8), device=dev, dtype=torch.uint8)
    W = torch.empty(1 if K == 2 else K, d + 1, device=dev, dtype=torch.float64)
    info = torch.empty(4, device=dev, dtype=torch.float64)
    ops.score_softmax_fit(X, y_d, n, d, K, 1.0 / C, max_iter, gtol, ws, W, info)
    info_h = info.cpu().numpy()
    if info_h[3] != 0:
        raise RuntimeError(f"logistic fit did not reach |g|inf <= {gtol:g}: {int(info_h[0])} iterations, |g|inf = {info_h[1]:.3e} "
                           f"(status {int(info_h[3])}: {ops.SOFTMAX_STATUS.get(int(info_h[3]), '?')})")
    return W, info_h


def softmax_proba(X, W, K):
    """predict_proba at W: device float64 [n,K] (softmax of the logits; [1 - p, p] for K = 2)"""
    _require_cuda(X)
    X = X.to(torch.float64).contiguous()
    n, d = X.shape
    if tuple(W.shape) != (1 if K == 2 else K, d + 1):
        raise ValueError(f"W {tuple(W.shape)} does not fit K = {K} classes of {d} columns")
    proba = torch.empty(n, K, device=X.device, dtype=torch.float64)
    ops.score_softmax_proba(X, n, d, K, W.to(torch.float64).contiguous(), proba)
    return proba


def roc_auc_ovr(proba, y, K):
    """roc_auc_score of every column of device proba [n,K] float64 against the indicator of class ids y [n] (host), from
    eg_score_auc_ovr's exact pair counts: AUC_k = (2 less + equal) / (2 n_pos n_neg), ties counting one half.  Raises ValueError where
    sklearn raises: a class without a row, or one that holds every row.
    -> (auc float64 [K], less uint64 [K], equal uint64 [K]) on the host"""
    y_h = np.asarray(y.cpu() if torch.is_tensor(y) else y).reshape(-1).astype(np.int64)
    n = y_h.size
    if proba.dim() != 2 or tuple(proba.shape) != (n, K):
        raise ValueError(f"scores {tuple(proba.shape)} do not match {n} labels of {K} classes")
    if n == 0 or y_h.min() < 0 or y_h.max() >= K:
        raise ValueError(f"class ids must lie in 0..{K - 1}")
    counts = np.bincount(y_h, minlength=K)
    if (counts == 0).any() or (counts == n).any():
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    _require_cuda(proba)
    dev = proba.device
    order = torch.from_numpy(np.argsort(y_h, kind="stable").astype(np.int32)).to(dev)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    counts_d = torch.empty(2, K, device=dev, dtype=torch.int64)               # uint64 counts: below 2^63 for any n a launch takes
    ops.score_auc_ovr(proba.to(torch.float64).contiguous(), order, offsets, n, K, int(counts.max()), counts_d[0], counts_d[1])
    less, equal = (c.astype(np.uint64) for c in counts_d.cpu().numpy())
    pairs = counts.astype(np.float64) * (n - counts).astype(np.float64)
    auc = (2.0 * less.astype(np.float64) + equal.astype(np.float64)) / (2.0 * pairs)
    return auc, less, equal


def fstat_modularity(codes, latent_ids, num_bins=20):
    """The modularity half of FStatMetric.evaluate (F_score.py:313-324): its discretize and mutual_info are MIG.py's make_discretizer
    and discrete_mutual_info (the same np.histogram / np.digitize / mutual_info_score calls), so the 5 x nf matrix comes from the MIG
    kernels; the script's arithmetic on it runs on the host.  -> (score, detail [5], mi [5,nf])"""
    modu_mi, _ = _discrete_mi(codes, latent_ids, num_bins)
    squared_modu_mi = np.square(modu_mi)
    max_squared_modu_mi = np.max(squared_modu_mi, axis=1)
    numerator = np.sum(squared_modu_mi, axis=1) - max_squared_modu_mi
    denominator = max_squared_modu_mi * (modu_mi.shape[1] - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        modu_score_detail = 1.0 - numerator / denominator
    return np.mean(modu_score_detail), modu_score_detail, modu_mi


def fstat_explicitness(codes, latent_ids, C=1.0):
    """The explicitness half (F_score.py:327-338): per factor the class ids by np.unique, ``softmax_fit`` on all code columns,
    ``softmax_proba``, and the mean of the per-class one-vs-rest AUCs (roc_auc_score's macro average over the indicator columns).
    -> (score, detail [nf,1], {factor j: {"W", "proba" (device), "auc", "less", "equal", "classes", "info" (host)}})"""
    _require_cuda(codes)
    codes = codes.to(torch.float64).contiguous()
    ids = np.asarray(latent_ids.cpu() if torch.is_tensor(latent_ids) else latent_ids)
    if ids.ndim != 2 or ids.shape[0] != codes.shape[0]:
        raise ValueError(f"latent ids {ids.shape} do not match {codes.shape[0]} codes")
    detail = np.zeros([ids.shape[1], 1])
    fits = {}
    for j in range(ids.shape[1]):
        classes, y = np.unique(ids[:, j], return_inverse=True)
        y = y.reshape(-1)
        if classes.size < 2:
            raise ValueError(f"factor {j} takes one value: LogisticRegression needs at least 2 classes")
        W, info = softmax_fit(codes, y, classes.size, C)
        proba = softmax_proba(codes, W, classes.size)
        auc, less, equal = roc_auc_ovr(proba, y, classes.size)
        detail[j] = np.mean(auc)
        fits[j] = {"W": W, "proba": proba, "auc": auc, "less": less, "equal": equal, "classes": classes, "info": info}
    return np.mean(detail), detail, fits


def fstat(codes, latent_ids):
    """-> the reference's dict (F_score.py:346-350): FStat_modu_metric, _detail [5], FStat_modu_mi [5,nf], FStat_expl_metric, _detail [nf,1]"""
    modu_score, modu_score_detail, modu_mi = fstat_modularity(codes, latent_ids)
    expl_score, expl_score_detail, _ = fstat_explicitness(codes, latent_ids)
    return {"FStat_modu_metric": modu_score,
            "FStat_modu_metric_detail": modu_score_detail,
            "FStat_modu_mi": modu_mi,
            "FStat_expl_metric": expl_score,
            "FStat_expl_metric_detail": expl_score_detail}


# default KKT residual of lasso_fit: 100 x the largest floor the float64 numpy coordinate descent of tests/make_dci_golden.py reaches on
# the production-sized set (1.29e-16) and the fixtures (<= 3.9e-17)
DCI_KKT_TOL = 1.3e-14
DCI_ALPHA = 0.02                                             # DCIMetric's Lasso(alpha) (DCI.py:251)
DCI_TINY = 1e-12                                             # DCIMetric.TINY (DCI.py:302)


def lasso_fit(codes, latents, alpha=DCI_ALPHA, max_sweeps=10000, tol=DCI_KKT_TOL):
    """The optimum of sklearn's Lasso(alpha) for every column of ``latents`` [n,nf] (host or device) on device codes [n,k] float64, both
    normalised as DCIMetric.normalize does (DCI.py:304-309,355-364): eg_score_norm_gram's moments and correlation matrix G, then
    eg_score_lasso_gram_fit's cyclic coordinate descent on G until the KKT residual is <= tol.  k + nf <= 32.  One host read: the
    solver's info with the moments' status word behind it.
    -> {"R" f64 [k,nf] = |W|^T, "W" f64 [nf,k], "mean" f64 [k+nf], "std" f64 [k+nf], "G" f64 [k+nf,k+nf]} on the device, "info" (host
    float64 [nf,4]: sweeps, final KKT residual, objective, status).  Raises ValueError for a column without variance (the reference's
    normalize yields NaN there and sklearn raises), RuntimeError when a target did not reach tol."""
    _require_cuda(codes)
    codes = codes.to(torch.float64).contiguous()
    n, k = codes.shape
    dev = codes.device
    fv = latents if torch.is_tensor(latents) else torch.from_numpy(np.ascontiguousarray(np.asarray(latents, dtype=np.float64)))
    fv = fv.to(device=dev, dtype=torch.float64).contiguous()
    if fv.dim() != 2 or fv.shape[0] != n:
        raise ValueError(f"factor values {tuple(fv.shape)} do not give {n} codes a row of factors each")
    nf = fv.shape[1]
    m = k + nf
    ws = torch.empty(max(ops.score_norm_gram_ws_bytes(n, k, nf), 8), device=dev, dtype=torch.uint8)
    mean = torch.empty(m, device=dev, dtype=torch.float64)
    std = torch.empty(m, device=dev, dtype=torch.float64)
    G = torch.empty(m, m, device=dev, dtype=torch.float64)
    rec = torch.zeros(nf * 4 + 1, device=dev, dtype=torch.float64)                 # info [nf,4] | the int32 status words
    info, status = rec[:nf * 4].view(nf, 4), rec[nf * 4:].view(torch.int32)
    W = torch.empty(nf, k, device=dev, dtype=torch.float64)
    ops.score_norm_gram(codes, fv, n, k, nf, ws, mean, std, G, status)
    ops.score_lasso_gram_fit(G, k, nf, alpha, max_sweeps, tol, W, info)
    rec_h = rec.cpu()                                                              # the one sync: offline evaluation
    info_h = rec_h[:nf * 4].view(nf, 4).numpy().copy()
    flags, col = (int(v) for v in rec_h[nf * 4:].view(torch.int32))
    if flags:
        which = f"code column {col}" if col < k else f"factor column {col - k}"
        if flags & ops.NORM_GRAM_NONFINITE:
            raise ValueError(f"{which} has a moment that is not finite")
        raise ValueError(f"{which} has zero variance: DCIMetric.normalize divides by its standard deviation")
    if (info_h[:, 3] != 0).any():
        j = int(np.nonzero(info_h[:, 3])[0][0])
        st = int(info_h[j, 3])
        raise RuntimeError(f"Lasso fit of factor {j} did not reach a KKT residual <= {tol:g}: {int(info_h[j, 0])} sweeps, residual "
                           f"{info_h[j, 1]:.3e} (status {st}: {ops.LASSO_STATUS.get(st, '?')})")
    return {"R": W.abs().t().contiguous(), "W": W, "mean": mean, "std": std, "G": G, "info": info_h}


def dci_scores(R, regressor="Lasso"):
    """DCIMetric.evaluate's arithmetic on the importance matrix R [k,nf] (DCI.py:311-321,376-399), operation for operation on the host
    -> the reference's dict; a code no factor uses (a zero row) gives the NaN the script's 0 / 0 gives"""
    R = np.asarray(R, dtype=np.float64)

    def entropic(r):
        """per column of r: 1 - the entropy of the column's shares, in units of log(rows)"""
        share = np.abs(r) / np.sum(np.abs(r), axis=0)
        return [1 - (-p.dot(np.log(p + DCI_TINY) / np.log(p.shape[0] + DCI_TINY))) for p in share.T]

    with np.errstate(divide="ignore", invalid="ignore"):
        disent = entropic(R.T)                                                     # per code, over the factors
        code_weight = np.sum(R, 1) / np.sum(R)
        complete = entropic(R)                                                     # per factor, over the codes
        res = {f"DCI_{regressor}_disent_metric_detail": disent,
               f"DCI_{regressor}_disent_metric": np.sum(np.array(disent) * code_weight),
               f"DCI_{regressor}_complete_metric_detail": complete,
               f"DCI_{regressor}_complete_metric": np.mean(complete),
               f"DCI_{regressor}_metric_detail": R}
    return res


def dci(codes, latents, regressor="Lasso"):
    """-> the reference's dict (DCI.py:391-399) for DCIMetric's default regressor, Lasso(alpha = 0.02): DCI_Lasso_disent_metric_detail
    (list [k]), DCI_Lasso_disent_metric, DCI_Lasso_complete_metric_detail (list [nf]), DCI_Lasso_complete_metric, DCI_Lasso_metric_detail
    (R [k,nf]).  The script's other regressors have no fixed target: LassoCV picks alpha from a grid by cross-validation folds, the
    random forests are random."""
    if regressor != "Lasso":
        raise NotImplementedError(f"dci: regressor {regressor!r} is not built: only 'Lasso', the script's default, is a fixed target "
                                  "(LassoCV selects a discrete alpha, the random forests are random)")
    return dci_scores(lasso_fit(codes, latents)["R"].cpu().numpy(), regressor)


# ================================================================================================
# drop-in for the scripts' module-level code
# ================================================================================================
def load_encoders(kind, encoder_pxy_path, encoder_path, device="cuda", dtype="f32"):
    """load_encoder() (MIG.py:146-158): the reference's checkpoints (its key layout) into this package's modules."""
    mod = cd if kind == "colored" else ds
    P, E = mod.Encoder_pxy(dtype=dtype), mod.Encoder(dtype=dtype)
    P.load_state_dict(torch.load(encoder_pxy_path, map_location="cpu", weights_only=True))
    E.load_state_dict(torch.load(encoder_path, map_location="cpu", weights_only=True))
    return P.to(device).eval(), E.to(device).eval()


def _open_run(kind, npz_path, encoder_pxy_path, encoder_path, seed, batch, device):
    """What every score script does before its plan: the archive, the encoders, then ``np.random.seed(seed)`` (else the global numpy
    stream as it stands).  -> (the open archive, its imgs, the Representation, kind == "colored")"""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    dataset_zip = np.load(npz_path, encoding="latin1", allow_pickle=True)
    imgs = dataset_zip["imgs"]
    P, E = load_encoders(kind, encoder_pxy_path, encoder_path, device)
    if seed is not None:
        np.random.seed(seed)
    return dataset_zip, imgs, Representation(P, E, kind, batch), kind == "colored"


def run_score(kind, metric, npz_path, encoder_pxy_path, encoder_path, seed=None, batch=4096, groups=None, device="cuda"):
    """What dSprites|colored_dSprites/score/{MIG,FactorVAE,BetVAE}.py do at module level, on the MI355X.  ``seed``: np.random.seed first (else
    the global numpy stream as it stands).  ``groups``: score only the first groups of the 500-group FactorVAE / BetaVAE plan (the plan is
    drawn in full).  Prints the score; returns it (MIG), the reference's three-key dict (FactorVAE) or its one-key dict (BetaVAE).
    score/SAP.py is ``run_sap``, score/F_score.py ``run_fstat`` and score/DCI.py ``run_dci``: this function's refusal of every other metric
    name is part of its contract."""
    if metric not in ("mig", "factor_vae", "beta_vae"):
        raise ValueError(f"metric must be 'mig', 'factor_vae' or 'beta_vae', got {metric!r}")
    dataset_zip, imgs, rep, colored = _open_run(kind, npz_path, encoder_pxy_path, encoder_path, seed, batch, device)
    N = imgs.shape[0]
    if metric == "mig":
        plan = mig_plan(N, colored)
        data = torch.from_numpy(np.ascontiguousarray(imgs)).to(device)
        codes = rep.codes(data, plan["idx"], plan["gains"])
        score, _, _ = mig(codes, dataset_zip["latents_values"][:, 1:6][plan["idx"]])
        print("MIG score", score)
        return score
    metadata = dataset_zip["metadata"][()]
    if metric == "beta_vae":
        plan = beta_vae_plan(metadata["latents_sizes"], N, colored)
        M = plan["labels"].size if groups is None else int(groups)
        data = torch.from_numpy(np.ascontiguousarray(imgs)).to(device)
        gc = rep.codes(data, plan["group_idx"][:M].reshape(-1), plan["group_gains"][:M].reshape(-1, 3) if colored else None)
        res = beta_vae(gc, plan["labels"][:M])
        print("acc", res["betaVAE_metric"])
        return res
    plan = factor_vae_plan(metadata["latents_sizes"], N, colored)
    M = plan["labels"].size if groups is None else int(groups)
    data = torch.from_numpy(np.ascontiguousarray(imgs)).to(device)
    ev = rep.codes(data, plan["eval_idx"], plan.get("eval_gains"))
    gi = plan["group_idx"][:M].reshape(-1)
    gg = plan["group_gains"][:M].reshape(-1, 3) if colored else None
    gc = rep.codes(data, gi, gg)
    labels = plan["labels"][:M]
    res = factor_vae(ev, gc, labels, len(set(labels.tolist())))
    print("score", res["factorVAE_metric"])
    return res


def run_sap(kind, npz_path, encoder_pxy_path, encoder_path, seed=None, batch=4096, device="cuda"):
    """What dSprites|colored_dSprites/score/SAP.py do at module level, on the MI355X (``run_score``'s arguments without the metric name).
    Prints ``score`` as the script does; returns the reference's dict {"SAP_metric", "SAP_metric_detail"}."""
    dataset_zip, imgs, rep, colored = _open_run(kind, npz_path, encoder_pxy_path, encoder_path, seed, batch, device)
    metadata = dataset_zip["metadata"][()]
    plan = sap_plan(metadata["latents_sizes"], imgs.shape[0], colored)
    latents = sap_latents(plan["latent_ids"], metadata["latents_names"], metadata["latents_possible_values"])
    data = torch.from_numpy(np.ascontiguousarray(imgs)).to(device)
    codes = rep.codes(data, plan["idx"], plan["gains"])                            # SAP.py:277 builds the same five columns
    res = sap(codes, latents, SAP_IS_CONTINUOUS)
    print("score", res["SAP_metric"])
    return res


def run_fstat(kind, npz_path, encoder_pxy_path, encoder_path, seed=None, batch=4096, device="cuda"):
    """What dSprites|colored_dSprites/score/F_score.py do at module level, on the MI355X (``run_sap``'s arguments).  Prints ``modu_score``
    and ``expl_score`` as the script does; returns the reference's five-key dict."""
    dataset_zip, imgs, rep, colored = _open_run(kind, npz_path, encoder_pxy_path, encoder_path, seed, batch, device)
    metadata = dataset_zip["metadata"][()]
    plan = fstat_plan(metadata["latents_sizes"], imgs.shape[0], colored)
    data = torch.from_numpy(np.ascontiguousarray(imgs)).to(device)
    codes = rep.codes(data, plan["idx"], plan["gains"])                            # F_score.py:304 builds the same five columns
    res = fstat(codes, plan["latent_id"])
    print("modu_score", res["FStat_modu_metric"])
    print("expl_score", res["FStat_expl_metric"])
    return res


def run_dci(kind, npz_path, encoder_pxy_path, encoder_path, seed=None, batch=4096, device="cuda"):
    """What dSprites|colored_dSprites/score/DCI.py do at module level, on the MI355X (``run_sap``'s arguments).  Prints ``disent_scores``
    and ``complete_avg`` as the script does; returns the reference's five-key dict."""
    dataset_zip, imgs, rep, colored = _open_run(kind, npz_path, encoder_pxy_path, encoder_path, seed, batch, device)
    metadata = dataset_zip["metadata"][()]
    plan = dci_plan(metadata["latents_sizes"], imgs.shape[0], colored)
    latents = sap_latents(plan["latent_ids"], metadata["latents_names"], metadata["latents_possible_values"])
    data = torch.from_numpy(np.ascontiguousarray(imgs)).to(device)
    codes = rep.codes(data, plan["idx"], plan["gains"])                            # DCI.py:350 builds the same five columns
    res = dci(codes, latents)
    print("disent_scores", res["DCI_Lasso_disent_metric_detail"])
    print("complete_avg", res["DCI_Lasso_complete_metric"])
    return res

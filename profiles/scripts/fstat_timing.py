"""production-shaped F-stat explicitness: device wall times, sklearn's time on this host, default-vs-optimum AUC"""
import importlib, os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
eg = importlib.import_module("ead-gan_amd")
from sklearn.linear_model import LogisticRegression
from sklearn.metrics import roc_auc_score

rng = np.random.RandomState(7)
n = 73728
sizes = (3, 6, 40, 32, 32)
ids = np.stack([rng.randint(s, size=n) for s in sizes], 1)
a = 2 * np.pi * ids[:, 2] / 40
flip = rng.uniform(size=n) < 0.2
codes = np.stack([np.where(flip, rng.randint(3, size=n), ids[:, 0]).astype(np.float64),
                  (0.5 + 0.1 * ids[:, 1]) * np.cos(a) + 0.3 * rng.normal(size=n), (0.5 + 0.1 * ids[:, 1]) * np.sin(a) + 0.3 * rng.normal(size=n),
                  ids[:, 3] / 31.0 - 0.5 + 0.05 * rng.normal(size=n), ids[:, 4] / 31.0 - 0.5 + 0.05 * rng.normal(size=n)], 1)
codes = codes.astype(np.float32).astype(np.float64)
cd = torch.from_numpy(codes).cuda()
eg.score.softmax_fit(cd[:2048], ids[:2048, 0], 3)                       # library load, first launches
torch.cuda.synchronize()
tot_fit = tot_auc = 0.0
for rep in range(2):
    for j, K in enumerate(sizes):
        y = ids[:, j]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        W, info = eg.score.softmax_fit(cd, y, K)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        proba = eg.score.softmax_proba(cd, W, K)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        auc, less, equal = eg.score.roc_auc_ovr(proba, y, K)
        torch.cuda.synchronize(); t3 = time.perf_counter()
        yd = torch.from_numpy(y.astype(np.int32)).cuda()
        order = torch.from_numpy(np.argsort(y, kind="stable").astype(np.int32)).cuda()
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(y, minlength=K))]).astype(np.int32)).cuda()
        cnt = torch.empty(2, K, device="cuda", dtype=torch.int64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); eg.ops.score_auc_ovr(proba, order, offs, n, K, int(np.bincount(y).max()), cnt[0], cnt[1]); e1.record(); torch.cuda.synchronize()
        print(f"rep {rep} factor {j} K {K}: fit {1e3 * (t1 - t0):.2f} ms ({int(info[0])} iterations, |g|inf {info[1]:.2e}), proba {1e3 * (t2 - t1):.2f} ms, "
              f"roc_auc_ovr {1e3 * (t3 - t2):.2f} ms, AUC kernel alone {e0.elapsed_time(e1):.3f} ms, mean AUC {auc.mean():.9f}", flush=True)
        if rep == 1:
            tot_fit += t1 - t0; tot_auc += e0.elapsed_time(e1) * 1e-3
print(f"five factors: fits {1e3 * tot_fit:.1f} ms, AUC kernels {1e3 * tot_auc:.2f} ms", flush=True)
tot = 0.0
for j, K in enumerate(sizes):
    y = ids[:, j]
    W, info = eg.score.softmax_fit(cd, y, K)
    a_opt = eg.score.roc_auc_ovr(eg.score.softmax_proba(cd, W, K), y, K)[0].mean()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = LogisticRegression(max_iter=100).fit(codes, y)
    dt = time.perf_counter() - t0
    tot += dt
    a_def = float(roc_auc_score((y[:, None] == np.arange(K)[None, :]).astype(np.int64), clf.predict_proba(codes)))
    Wd = np.concatenate([clf.coef_, clf.intercept_[:, None]], 1)
    print(f"factor {j} K {K}: sklearn default fit {dt:.2f} s, {int(clf.n_iter_.max())} lbfgs iterations; AUC default {a_def:.9f} at the optimum {a_opt:.9f} "
          f"|difference| {abs(a_def - a_opt):.3e}; max|W default - W device| {np.abs(Wd - W.cpu().numpy()).max():.3e}", flush=True)
print(f"sklearn default, five factors: {tot:.2f} s", flush=True)

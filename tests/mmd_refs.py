"""The kernel MMD over uint8 rows, restated in numpy on top of tests/knn_refs.py's int64 distances: what ops.dist_select_u8 must
return bit for bit, and what ops.kernel_sum_u8 and the functions of quality.py built on the two must return within the rounding of a
float64 sum.  The kernel's argument is formed as the device forms it, (double)d * inv_gamma in one rounding."""
import math

import numpy as np

import knn_refs


def _kept(nq, n, self0):
    """bool [nq, n]: the pairs (i, j) with j != self0 + i"""
    keep = np.ones((nq, n), bool)
    if self0 >= 0:
        for i in range(nq):
            if self0 + i < n:
                keep[i, self0 + i] = False
    return keep


def pairs(q, x, self0=-1):
    """int64, ascending: the multiset { d(q[i], x[j]) : j != self0 + i }"""
    d = knn_refs.distances(q, x)
    return np.sort(d[_kept(*d.shape, self0)], kind="stable")


def select(q, x, rank, self0=-1):
    """-> (the element of 0-based rank, or the largest one / 0 where the rank is beyond the pairs; 1 if it is beyond, else 0)"""
    p = pairs(q, x, self0)
    if rank >= len(p):
        return (int(p[-1]) if len(p) else 0), 1
    return int(p[rank]), 0


def median_rank(T):
    """0-based rank of the lower median among the P = T (T - 1) ordered pairs of T rows"""
    return (T * (T - 1) - 1) // 2


def median_distance(z):
    """the lower median of { d(z[i], z[j]) : i != j }"""
    return select(z, z, median_rank(len(z)), self0=0)[0]


def kernel_sums(q, x, inv_gamma, self0=-1):
    """float64 [nq, nb]: sum over j != self0 + i of exp(-(d(q[i], x[j]) * inv_gamma[b]))"""
    d = knn_refs.distances(q, x)
    keep = _kept(*d.shape, self0)
    ig = np.asarray(inv_gamma, np.float64)
    out = np.empty((d.shape[0], len(ig)), np.float64)
    with np.errstate(under="ignore"):
        for b in range(len(ig)):
            out[:, b] = np.where(keep, np.exp(-(d.astype(np.float64) * ig[b])), 0.0).sum(1)
    return out


def sums(real, fake, inv_gamma):
    """-> (S_xx, S_yy, S_xy), float64 [nb] each"""
    sxx = kernel_sums(real, real, inv_gamma, self0=0).sum(0)
    syy = kernel_sums(fake, fake, inv_gamma, self0=0).sum(0)
    sxy = kernel_sums(real, fake, inv_gamma).sum(0)
    return sxx, syy, sxy


def estimators(sxx, syy, sxy, N, M):
    """-> (mmd2, mmd2_biased), float64 [nb]"""
    sxx, syy, sxy = (np.asarray(v, np.float64) for v in (sxx, syy, sxy))
    unbiased = sxx / (N * (N - 1)) + syy / (M * (M - 1)) - 2.0 * sxy / (N * M)
    biased = (sxx + N) / (N * N) + (syy + M) / (M * M) - 2.0 * sxy / (N * M)
    return unbiased, biased


def mmd(real, fake, scales=(0.5, 1.0, 2.0), bandwidths=None):
    """quality.mmd's dictionary with numpy float64 values"""
    N, M = len(real), len(fake)
    med = None
    if bandwidths is None:
        med = median_distance(np.concatenate((np.asarray(real).reshape(N, -1), np.asarray(fake).reshape(M, -1))))
        bandwidths = [float(s) * float(med) for s in scales]
    gam = np.asarray(bandwidths, np.float64)
    u, b = estimators(*sums(real, fake, 1.0 / gam), N, M)
    return {"gamma_median": med, "bandwidths": [float(g) for g in gam], "mmd2": [float(v) for v in u], "mmd2_biased": [float(v) for v in b],
            "mean": float(np.mean(u))}


def witness(real, fake, queries, bandwidth):
    """float64 [nq]: (1/N) sum_i k(z, X_i) - (1/M) sum_j k(z, Y_j)"""
    ig = np.array([1.0 / np.float64(bandwidth)])
    return kernel_sums(queries, real, ig)[:, 0] / len(real) - kernel_sums(queries, fake, ig)[:, 0] / len(fake)


def tolerance(n):
    """relative bound of a device row sum of n non-negative terms against this file's: every term within a few ulp, at most n additions"""
    return (n + 8) * 2.0 ** -52


# ---- the same from the definitions, by loops over Python numbers: the check of the above on tiny sets -----------------------------------
def _d(a, b):
    return sum((int(u) - int(v)) ** 2 for u, v in zip(a, b))


def _rows(a):
    return [list(r) for r in np.asarray(a).reshape(len(a), -1)]


def pairs_brute(q, x, self0=-1):
    q, x = _rows(q), _rows(x)
    return sorted(_d(q[i], x[j]) for i in range(len(q)) for j in range(len(x)) if not (self0 >= 0 and j == self0 + i))


def kernel_sums_brute(q, x, inv_gamma, self0=-1):
    q, x = _rows(q), _rows(x)
    return [[math.fsum(math.exp(-(float(_d(q[i], x[j])) * float(g))) for j in range(len(x)) if not (self0 >= 0 and j == self0 + i))
             for g in inv_gamma] for i in range(len(q))]


def mmd_brute(real, fake, gamma):
    """-> (mmd2, mmd2_biased, [witness of every real row, then of every fake row]) at one bandwidth"""
    X, Y = _rows(real), _rows(fake)
    N, M = len(X), len(Y)
    k = lambda a, b: math.exp(-(float(_d(a, b)) * (1.0 / gamma)))
    sxx = math.fsum(k(X[i], X[j]) for i in range(N) for j in range(N) if i != j)
    syy = math.fsum(k(Y[i], Y[j]) for i in range(M) for j in range(M) if i != j)
    sxy = math.fsum(k(a, b) for a in X for b in Y)
    wit = [math.fsum(k(z, a) for a in X) / N - math.fsum(k(z, b) for b in Y) / M for z in X + Y]
    return (sxx / (N * (N - 1)) + syy / (M * (M - 1)) - 2 * sxy / (N * M), (sxx + N) / N ** 2 + (syy + M) / M ** 2 - 2 * sxy / (N * M), wit)


def median_unordered_brute(z):
    """the lower median over the T (T - 1) / 2 unordered pairs"""
    z = _rows(z)
    p = sorted(_d(z[i], z[j]) for i in range(len(z)) for j in range(i + 1, len(z)))
    return p[(len(p) - 1) // 2]


def digit_boundary_rows(K=32768):
    """-> (uint8 [61, K], their 61 distances from the all-zero row, ascending): 0, and 2^b - 1, 2^b for b = 1 .. 30, each written greedily
    as bytes 255 (65025 each), 16 (256 each) and 1"""
    ds = [0] + [v for b in range(1, 31) for v in (2 ** b - 1, 2 ** b)]
    rows = np.zeros((len(ds), K), np.uint8)
    for r, d in enumerate(ds):
        a, rest = divmod(d, 65025)
        b, c = divmod(rest, 256)
        assert a + b + c <= K
        rows[r, :a], rows[r, a:a + b], rows[r, a + b:a + b + c] = 255, 16, 1
    return rows, ds

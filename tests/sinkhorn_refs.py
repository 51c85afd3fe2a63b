"""The soft minimum and the debiased Sinkhorn divergence over uint8 rows, restated in numpy float64 on top of tests/knn_refs.py's
int64 distances: what ops.softmin_u8 and quality.sinkhorn must return within ``tolerance``.  The argument t = (g[j] - d) * inv_eps is
formed as the device forms it, one rounded subtraction and one rounded product, so both sides hold the same bits of t; the reference then
takes the maximum first and sums exp(t - max) exactly (math.fsum), where the device streams one running (maximum, sum) pair."""
import math

import numpy as np

import knn_refs
import mmd_refs


def softmin_d(d, g, inv_eps, self0=-1, prev=None, stats=None):
    """float64 [nq] from a distance matrix d [nq, n]: soft[i] = -(m + (log s - log |J_i|)) / inv_eps with m = max_j t_ij and
    s = sum_j exp(t_ij - m) over J_i = { j != self0 + i }; with ``prev`` the average 0.5 * prev + 0.5 * soft.  Two passes: the maximum,
    then the sum.  ``stats``: a dict that receives "tmax" = max |t_ij| over the kept pairs."""
    d = np.asarray(d).astype(np.float64)
    g, ie = np.asarray(g, np.float64), np.float64(inv_eps)
    keep = mmd_refs._kept(*d.shape, self0)
    t = (g[None, :] - d) * ie
    if stats is not None:
        stats["tmax"] = float(np.abs(t[keep]).max())
    t = np.where(keep, t, -np.inf)
    m = t.max(1)
    with np.errstate(under="ignore"):
        e = np.exp(t - m[:, None])
    s = np.array([math.fsum(row) for row in e])
    soft = -((m + (np.log(s) - np.log(keep.sum(1).astype(np.float64)))) / ie)
    return soft if prev is None else 0.5 * np.asarray(prev, np.float64) + 0.5 * soft


def softmin(q, x, g, inv_eps, self0=-1, prev=None, stats=None):
    """``softmin_d`` of the exact distances between the rows of two uint8 arrays"""
    return softmin_d(knn_refs.distances(q, x), g, inv_eps, self0, prev, stats)


def softmin_brute(q, x, g, inv_eps, self0=-1, prev=None):
    """the same by loops over Python numbers"""
    q, x = mmd_refs._rows(q), mmd_refs._rows(x)
    ie = float(inv_eps)
    out = []
    for i in range(len(q)):
        ts = [(float(g[j]) - float(mmd_refs._d(q[i], x[j]))) * ie for j in range(len(x)) if not (self0 >= 0 and j == self0 + i)]
        m = max(ts)
        s = math.fsum(math.exp(t - m) for t in ts)
        soft = -((m + (math.log(s) - math.log(float(len(ts))))) / ie)
        out.append(soft if prev is None else 0.5 * float(prev[i]) + 0.5 * soft)
    return out


def tolerance(n, eps, tmax):
    """Absolute bound of a device soft[i] (ops.softmin_u8) against ``softmin_d``'s at n database rows, temperature eps = 1 / inv_eps and
    tmax = max |t_ij| -- from the arithmetic of the two, not from what the device returned:

        eps * ((2 n + 16) * 2^-52 + 4 * 2^-53 * tmax)

    Both sides hold the same t and the same maximum m (the device's running maximum only ever takes values of t), so the difference is in
    log s and in the last three operations.

    The sum s.  Exact: sum_j w_j with w_j = exp(t_j - m) <= 1 and s >= 1.  Every exponential and logarithm of either library is within
    an ulp or two ("a few": the +16 with the merges below).  The device makes one step per offer: an addition s + e (half an ulp, 2^-53,
    of the partial sum), or a rescale fma(s, exp(m_old - m_new), 1) (an exponential and one rounding: under 1.5 * 2^-52 of the partial
    sum).  There are at most n steps, and at most 3 + slices more of the rescale kind where parts and slices are merged; the reference's
    sum is exact.  That is under 1.5 n * 2^-52 relative.  The ARGUMENTS of the exponentials are rounded differences: on the device term
    j passes through exp(t_j - m_a) exp(m_a - m_b) ... exp(m_y - m), whose arguments add up to t_j - m and carry together at most
    2^-53 x_j with x_j = m - t_j; the reference's exp(t_j - m) carries the same.  A relative x_j 2^-53 on a term of weight w_j = exp(-x_j)
    moves s by 2^-53 x_j exp(-x_j) <= 2^-53 / e, whatever tmax is: all terms together under 0.37 n * 2^-52 for the two sides.  Sum:
    under (2 n + 16) * 2^-52 relative on s, hence absolute on log s; log s - log |J_i| <= log n rounds below that.

    The last operations.  m + c, the quotient by inv_eps and (with ``prev``) the average are the same operation on both sides on inputs
    that differ by less than the above; their results round to neighbours in a grid whose spacing is 2^-52 |m| <= 2 * 2^-53 * tmax
    before the quotient and eps times that after it: 4 * 2^-53 * tmax for the sum and the quotient.  (The average halves what it is
    given before it rounds once more, at half that spacing.)

    For a whole ``sinkhorn`` the bound is iterations x the largest such figure of its calls: the soft minimum and the average are
    non-expansive in the sup norm, so the errors of the iterations add and do not grow."""
    return float(eps) * ((2 * n + 16) * 2.0 ** -52 + 4 * 2.0 ** -53 * float(tmax))


def schedule(eps, eps0, iterations, rho):
    """float64 [iterations]: eps_t = max(eps, eps0 * rho^t), the product in one rounding"""
    return np.maximum(np.float64(eps), np.float64(eps0) * np.array([float(rho) ** t for t in range(int(iterations))], np.float64))


def sinkhorn(real, fake, scale=0.1, epsilon=None, iterations=60, rho=0.5, detail=None):
    """quality.sinkhorn's dictionary with Python floats, the schedule in full: epsilon scaling from the largest pooled distance,
    symmetric (Jacobi) averaged updates of the XY problem from the OLD potentials, the two symmetric problems in place, and one more
    soft minimum without ``prev`` for the row-marginal error.  ``detail``: a dict that receives the potentials "f", "g", "p", "r", the
    "schedule" and "bound" = iterations x the largest ``tolerance`` of the loop's calls."""
    X, Y = np.asarray(real).reshape(len(real), -1), np.asarray(fake).reshape(len(fake), -1)
    N, M = len(X), len(Y)
    dxy, dxx, dyy = (knn_refs.distances(a, b) for a, b in ((X, Y), (X, X), (Y, Y)))
    pool = np.concatenate((X, Y))
    med = None
    if epsilon is None:
        med = mmd_refs.median_distance(pool)
        epsilon = float(scale) * float(med)
    eps0 = float(max(dxy.max(), dxx.max(), dyy.max()))
    sched = schedule(epsilon, eps0, iterations, rho)
    f, g, p, r = np.zeros(N), np.zeros(M), np.zeros(N), np.zeros(M)
    worst, st = 0.0, {}
    for e in sched:
        ie = 1.0 / e
        calls = ((dxy, g, f, M), (dxy.T, f, g, N), (dxx, p, p, N), (dyy, r, r, M))
        new = []
        for d, pot, prev, n in calls:
            new.append(softmin_d(d, pot, ie, -1, prev, st))
            worst = max(worst, tolerance(n, e, st["tmax"]))
        f, g, p, r = new
    ie = 1.0 / sched[-1]
    last = softmin_d(dxy, g, ie)
    marginal = float(np.mean(np.abs(np.exp((f - last) * ie) - 1.0)))
    div = float(np.mean(f - p) + np.mean(g - r))
    if detail is not None:
        detail.update(f=f, g=g, p=p, r=r, schedule=sched, bound=len(sched) * worst)
    return {"gamma_median": med, "epsilon": float(sched[-1]), "iterations": int(iterations), "divergence": div,
            "relative": None if med is None else div / med, "ot_xy": float(np.mean(f) + np.mean(g)), "ot_xx": float(2.0 * np.mean(p)),
            "ot_yy": float(2.0 * np.mean(r)), "marginal_error": marginal}


def clustered(seed=0, K=192):
    """the clustered sets of the tests: real = 200 rows around two fixed random centres, noise +-12; generated = 130 rows around those two
    and one foreign centre"""
    rng = np.random.RandomState(seed)
    centres = rng.randint(40, 216, (3, K))
    real = np.concatenate([c + rng.randint(-12, 13, (100, K)) for c in centres[:2]])
    fake = np.concatenate([c + rng.randint(-12, 13, (m, K)) for c, m in zip(centres, (50, 50, 30))])
    return real.astype(np.uint8), fake.astype(np.uint8)


def assignment_cost(real, fake):
    """mean cost of the optimal one-to-one assignment between two sets of equal size (scipy, or brute force over the permutations)"""
    d = knn_refs.distances(real, fake)
    try:
        from scipy.optimize import linear_sum_assignment
        rows, cols = linear_sum_assignment(d)
        return float(d[rows, cols].sum()) / len(d)
    except ImportError:
        import itertools
        n = len(d)
        return min(sum(int(d[i, perm[i]]) for i in range(n)) for perm in itertools.permutations(range(n))) / n

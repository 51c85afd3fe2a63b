"""Precision, recall, density and coverage over uint8 rows, restated in numpy int64 on top of tests/knn_refs.py: what
ops.ball_count_u8, quality.knn_radii and quality.prdc must return bit for bit.  The balls are CLOSED (d <= rad); every result is an
integer or a pair (numerator, denominator) of integers."""
import numpy as np

import knn_refs


def radii(s, k):
    """int64 [N]: the distance from every row to its k-th nearest OTHER row of the set"""
    return knn_refs.knn(s, s, k, self0=0)[0][:, k - 1].copy()


def ball_count(q, x, rad, self0=-1):
    """int64 [nq]: count[i] = #{ j != self0 + i : d(q[i], x[j]) <= rad[j] }"""
    d = knn_refs.distances(q, x)
    inside = d <= np.asarray(rad, np.int64)[None, :]
    if self0 >= 0:
        for i in range(len(d)):
            if self0 + i < d.shape[1]:
                inside[i, self0 + i] = False
    return inside.sum(1).astype(np.int64)


def prdc(real, fake, k):
    """-> {"precision": (num, den), "recall": ..., "density": ..., "coverage": ...} with integer numerators and denominators"""
    N, M = len(real), len(fake)
    rad_real, rad_fake = radii(real, k), radii(fake, k)
    c = ball_count(fake, real, rad_real)
    r = ball_count(real, fake, rad_fake)
    nearest = knn_refs.distances(real, fake).min(1)
    return {"precision": (int((c > 0).sum()), M), "density": (int(c.sum()), k * M), "recall": (int((r > 0).sum()), N),
            "coverage": (int((nearest <= rad_real).sum()), N)}


def _d(a, b):
    return sum((int(u) - int(v)) ** 2 for u, v in zip(a, b))


def prdc_brute(real, fake, k):
    """the same by loops over Python integers, straight from the definitions: the check of ``prdc`` on a tiny case"""
    real = [list(r) for r in np.asarray(real).reshape(len(real), -1)]
    fake = [list(f) for f in np.asarray(fake).reshape(len(fake), -1)]

    def rad(s):
        return [sorted(_d(s[j], s[o]) for o in range(len(s)) if o != j)[k - 1] for j in range(len(s))]
    rr, rf = rad(real), rad(fake)
    c = [sum(1 for j in range(len(real)) if _d(f, real[j]) <= rr[j]) for f in fake]
    rec = sum(1 for r in real if any(_d(r, fake[i]) <= rf[i] for i in range(len(fake))))
    cov = sum(1 for j, r in enumerate(real) if min(_d(r, f) for f in fake) <= rr[j])
    return {"precision": (sum(1 for v in c if v > 0), len(fake)), "density": (sum(c), k * len(fake)), "recall": (rec, len(real)),
            "coverage": (cov, len(real))}


def ball_count_brute(q, x, rad, self0=-1):
    q = np.asarray(q).reshape(len(q), -1)
    x = np.asarray(x).reshape(len(x), -1)
    return np.array([sum(1 for j in range(len(x)) if not (self0 >= 0 and j == self0 + i) and _d(q[i], x[j]) <= int(rad[j]))
                     for i in range(len(q))], np.int64)


def clustered(seed=0, K=64):
    """the clustered sets of the GPU test: real = three clusters of 50 around fixed random centres, noise +-12; generated = 131 rows
    from two of those centres and one foreign centre"""
    rng = np.random.RandomState(seed)
    centres = rng.randint(40, 216, (4, K))
    real = np.concatenate([c + rng.randint(-12, 13, (50, K)) for c in centres[:3]])
    fake = np.concatenate([c + rng.randint(-12, 13, (m, K)) for c, m in zip(centres[[0, 1, 3]], (50, 50, 31))])
    return real.astype(np.uint8), fake.astype(np.uint8)

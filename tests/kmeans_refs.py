"""k-means over uint8 rows with byte centres and the NDB score built on it, restated in numpy int64 on knn_refs.distances: what
ops.group_rows, ops.kmeans_update_u8, ops.kmeans_seed_u8, ops.kmeans_u8 and quality.ndb must return bit for bit.

The contract: a centre is a uint8 row; a row goes to the nearest centre by exact squared L2 distance, ties to the lower centre; a cell with
count > 0 gets centre[t] = (2 sum[t] + count) // (2 count) (round half up), an empty cell keeps its bytes; the seeding is k-means++ driven
by fp32 uniforms u: centre 0 = row min(floor(u[0] n), n - 1), then the lowest row whose inclusive prefix sum of mind exceeds
min(floor((double)u[j] * (double)total), total - 1).  Centres are bytes, so the inertia is not guaranteed to fall monotonically."""
import math

import numpy as np

import knn_refs

FLAG_DUPLICATES, FLAG_U = 1, 2
Z_975 = 1.959963984540054


def _flat(rows):
    rows = np.asarray(rows)
    assert rows.dtype == np.uint8
    return rows.reshape(len(rows), -1)


def assign(rows, centres):
    """-> (labels, dist), int64 [n]: the nearest centre of every row, ties to the lower centre"""
    d = knn_refs.distances(_flat(rows), _flat(centres))
    labels = d.argmin(1)                                           # the first minimum
    return labels.astype(np.int64), d[np.arange(len(d)), labels]


def group(labels, bins):
    """-> (counts [bins], offsets [bins + 1], order [n], flag): the stable counting sort; a label outside [0, bins) joins no cell, raises
    the flag and leaves a -1 at the end of order"""
    labels = np.asarray(labels, np.int64)
    ok = (labels >= 0) & (labels < bins)
    counts = np.bincount(labels[ok], minlength=bins).astype(np.int64)
    offsets = np.concatenate(([0], np.cumsum(counts)))
    rows = np.nonzero(ok)[0]
    order = np.full(len(labels), -1, np.int64)
    order[:len(rows)] = rows[np.argsort(labels[ok], kind="stable")]
    return counts, offsets, order, int(not ok.all())


def round_half_up(sums, count):
    """(2 sum + count) // (2 count) over int64"""
    sums = np.asarray(sums, np.int64)
    return (2 * sums + count) // (2 * count)


def update(rows, labels, centres):
    """-> the new centres, uint8 like ``centres``"""
    flat, out = _flat(rows).astype(np.int64), np.array(centres, copy=True)
    o = out.reshape(len(out), -1)
    for c in range(len(o)):
        member = np.asarray(labels) == c
        count = int(member.sum())
        if count:
            o[c] = round_half_up(flat[member].sum(0), count).astype(np.uint8)
    return out


def update_brute(rows, labels, centres):
    """the same over Python integers: the check of ``update`` on a tiny case"""
    flat = _flat(rows)
    out = [[int(v) for v in c] for c in _flat(centres)]
    for c in range(len(out)):
        member = [i for i, l in enumerate(labels) if int(l) == c]
        if member:
            for t in range(flat.shape[1]):
                s = sum(int(flat[i][t]) for i in member)
                out[c][t] = (2 * s + len(member)) // (2 * len(member))
    return np.array(out, np.uint8).reshape(np.asarray(centres).shape)


def first_pick(u0, n):
    return min(int(math.floor(float(np.float32(u0)) * float(n))), n - 1)


def seed_pick(mind, u):
    """-> (row, flag) of one seeding pass over the int64 distances ``mind``: total == 0 reports FLAG_DUPLICATES and row 0"""
    mind = np.asarray(mind, np.int64)
    total = int(mind.sum())
    if total == 0:
        return 0, FLAG_DUPLICATES
    assert total <= 2 ** 53
    target = min(int(math.floor(float(np.float32(u)) * float(total))), total - 1)         # ONE rounded double product
    prefix = np.cumsum(mind)
    return int(np.nonzero(prefix > target)[0][0]), 0


def seed(rows, bins, u):
    """-> (idx int64 [bins], centres uint8 [bins, ...], flag)"""
    rows = np.asarray(rows)
    flat, n = _flat(rows), len(rows)
    u = np.asarray(u, np.float32)
    assert len(u) == bins and n * 2 ** 31 <= 2 ** 53
    flag = 0 if ((u >= 0) & (u < 1)).all() else FLAG_U
    idx = [first_pick(u[0], n)]
    mind = None
    for j in range(1, bins):
        d = knn_refs.distances(flat, flat[idx[-1]:idx[-1] + 1])[:, 0]
        mind = d if mind is None else np.minimum(mind, d)
        row, f = seed_pick(mind, u[j])
        idx.append(row)
        flag |= f
    idx = np.array(idx, np.int64)
    return idx, rows[idx].copy(), flag


def seed_brute(rows, bins, u):
    """the seeding over Python integers: the check of ``seed`` on a tiny case"""
    flat = [[int(v) for v in r] for r in _flat(rows)]
    n = len(flat)
    idx = [min(int(float(np.float32(u[0])) * n), n - 1)]
    for j in range(1, bins):
        mind = [min(sum((a - b) ** 2 for a, b in zip(r, flat[c])) for c in idx) for r in flat]
        total = sum(mind)
        target = min(int(float(np.float32(u[j])) * float(total)), total - 1)
        run = 0
        for i, m in enumerate(mind):
            run += m
            if run > target:
                idx.append(i)
                break
    return idx


def kmeans(rows, bins, iterations, u=None, init=None):
    """-> (centres, labels, counts, {"inertia": int64 [iterations + 1], "changed": int64 [iterations]}, flag)"""
    rows = np.asarray(rows)
    n, flag = len(rows), 0
    if init is None:
        _, centres, flag = seed(rows, bins, u)
    else:
        init = np.asarray(init)
        centres = rows[init].copy() if init.dtype != np.uint8 else init.copy()
    inertia, changed, prev = [], [], None
    for t in range(iterations + 1):
        labels, dist = assign(rows, centres)
        inertia.append(int(dist.sum()))
        if t == iterations:
            break
        changed.append(n if prev is None else int((labels != prev).sum()))
        centres = update(rows, labels, centres)
        prev = labels
    counts = np.bincount(labels, minlength=bins).astype(np.int64)
    return centres, labels, counts, {"inertia": np.array(inertia, np.int64), "changed": np.array(changed, np.int64)}, flag


def bin_counts(rows, centres):
    return np.bincount(assign(rows, centres)[0], minlength=len(centres)).astype(np.int64)


def z_scores(a, b):
    """the two-proportion z statistic of every bin over Python floats: z = (q - p) / SE, 0 where SE == 0"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    N, M = sum(a), sum(b)
    z = []
    for x, y in zip(a, b):
        p, q, P = x / N, y / M, (x + y) / (N + M)
        se = math.sqrt(P * (1.0 - P) * (1.0 / N + 1.0 / M))
        z.append((q - p) / se if se > 0.0 else 0.0)
    return z


def js_divergence(a, b):
    """Jensen-Shannon divergence, base 2, of the two histograms: in [0, 1], 0 log 0 = 0"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    N, M = sum(a), sum(b)
    js = 0.0
    for x, y in zip(a, b):
        p, q = x / N, y / M
        m = 0.5 * (p + q)
        if p > 0.0:
            js += 0.5 * (p * math.log2(p / m))
        if q > 0.0:
            js += 0.5 * (q * math.log2(q / m))
    return min(1.0, max(0.0, js))


def ndb_stats(a, b, z_threshold=Z_975):
    """the score's dictionary without the fit's two entries, from the two count vectors"""
    z = z_scores(a, b)
    different = sum(1 for v in z if abs(v) > z_threshold)
    return {"bins": len(z), "ndb": different, "ndb_over_bins": different / len(z), "js": js_divergence(a, b),
            "empty_real": sum(1 for v in a if int(v) == 0), "empty_fake": sum(1 for v in b if int(v) == 0)}


def ndb(real, fake, bins, iterations, u, z_threshold=Z_975, centres=None):
    """-> (dictionary, z, a, b) as quality.ndb(..., terms=True) gives them; ``u``: the uniforms quality.image_bins draws"""
    if centres is None:
        centres, _, a, log, flag = kmeans(real, bins, iterations, u=u)
        assert flag == 0
        fit = {"inertia": int(log["inertia"][-1]), "changed_last": int(log["changed"][-1]) if iterations else None}
    else:
        a, fit = bin_counts(real, centres), {"inertia": None, "changed_last": None}
    b = bin_counts(fake, centres)
    out = dict(ndb_stats(a, b, z_threshold), **fit)
    return out, z_scores(a, b), a, b


def mixture(n, K, modes, seed, keep=None, spread=6):
    """n uint8 rows of K bytes around ``modes`` random byte centres (seeded apart from the rows, so two calls share the modes); ``keep``:
    only these modes are drawn from"""
    centres = np.random.RandomState(1234).randint(40, 216, (modes, K))
    rng = np.random.RandomState(seed)
    which = rng.choice(np.arange(modes) if keep is None else np.asarray(keep), n)
    return np.clip(centres[which] + rng.randint(-spread, spread + 1, (n, K)), 0, 255).astype(np.uint8)

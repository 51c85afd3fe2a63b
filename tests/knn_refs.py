"""The exact nearest-neighbour search over uint8 rows, restated in numpy int64: what ops.knn_u8 and the functions of quality.py
built on it must return bit for bit.  Distances are formed by explicit difference and square (no norm expansion, no float), neighbours are
ordered by (distance, index) with a stable sort, so equal distances go to the lower index."""
import numpy as np


def distances(q, x):
    """int64 [nq, n]: d(i, j) = sum_t (q[i][t] - x[j][t])^2 over the flattened rows of two uint8 arrays"""
    q = np.asarray(q).reshape(len(q), -1).astype(np.int64)
    x = np.asarray(x).reshape(len(x), -1).astype(np.int64)
    out = np.empty((len(q), len(x)), np.int64)
    for i in range(len(q)):                      # a row at a time: [n, K] int64 is the largest temporary
        diff = x - q[i]
        out[i] = (diff * diff).sum(1)
    return out


def knn(q, x, k, self0=-1):
    """-> (dist, idx), int64 [nq, k]: the k smallest pairs of every query in ascending (d, j); with self0 >= 0 the pair j == self0 + i is
    excluded where that row exists"""
    d = distances(q, x)
    nq, n = d.shape
    dist, idx = np.empty((nq, k), np.int64), np.empty((nq, k), np.int64)
    for i in range(nq):
        order = np.argsort(d[i], kind="stable")                  # ties: the lower index first
        if self0 >= 0 and self0 + i < n:
            order = order[order != self0 + i]
        assert len(order) >= k, "k exceeds the candidates of a query"
        idx[i] = order[:k]
        dist[i] = d[i][order[:k]]
    return dist, idx


def knn_brute(q, x, k, self0=-1):
    """the same by a double loop over Python integers and a sort of (d, j) tuples: the check of ``knn`` on a tiny case"""
    q = np.asarray(q).reshape(len(q), -1)
    x = np.asarray(x).reshape(len(x), -1)
    dist, idx = [], []
    for i in range(len(q)):
        pairs = []
        for j in range(len(x)):
            if self0 >= 0 and j == self0 + i:
                continue
            pairs.append((sum((int(a) - int(b)) ** 2 for a, b in zip(q[i], x[j])), j))
        pairs.sort()
        dist.append([p[0] for p in pairs[:k]])
        idx.append([p[1] for p in pairs[:k]])
    return np.array(dist, np.int64), np.array(idx, np.int64)


def two_sample_counts(real, fake):
    """leave-one-out 1-NN over the pooled rows, real first -> (real rows whose neighbour is real, fake rows whose neighbour is fake, N)"""
    N = len(real)
    pool = np.concatenate((np.asarray(real).reshape(N, -1), np.asarray(fake).reshape(len(fake), -1)))
    _, idx = knn(pool, pool, 1, self0=0)
    nn_real = idx[:, 0] < N
    return int(nn_real[:N].sum()), int((~nn_real[N:]).sum()), N


def to_u8(v):
    """float [-1, 1] -> the byte whose image under 2/255 u - 1 it is: v' = 0.5 v + 0.5, then clamp(v' * 255 + 0.5, 0, 255) truncated, every
    step a separately rounded fp32 operation"""
    v = np.asarray(v, np.float32)
    h, one, top = np.float32(0.5), np.float32(255.0), np.float32(0.0)
    w = (v * h).astype(np.float32) + h
    w = (w.astype(np.float32) * one).astype(np.float32) + h
    return np.clip(w.astype(np.float32), top, one).astype(np.uint8)


def grid(queries, database, idx):
    """float32 [nq (1 + k), C, H, W] in [0, 1]: query r, then its k neighbours"""
    queries, database, idx = np.asarray(queries), np.asarray(database), np.asarray(idx)
    rows = []
    for r in range(len(queries)):
        rows.append(queries[r])
        rows.extend(database[j] for j in idx[r])
    return np.stack(rows).astype(np.float32) / np.float32(255.0)

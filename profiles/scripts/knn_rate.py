"""Full-size cost of the exact nearest-neighbour search on one GPU, in its two regimes.  Prints one table; pipe it into
profiles/knn_rate.txt.

(a) a few queries against the whole dataset: 64 x [202 599, 12288] random uint8, k = 8 -- 2.49 GB read once, memory bound.  Reported: the
    achieved share of the measured HBM read rate (6.29 TB/s, the guide's float4 copy).
(b) the pooled leave-one-out call of the two-sample test: 16 384 x 16 384 rows of 12288 bytes, k = 1 -- 3.3e12 multiply-adds, MFMA bound.
    Reported: int8 TOP/s against twice the bf16 rate the project's own GEMMs reach (README: 840-1010 TFLOP/s).
Yardstick of both, same session, same protocol (device events, 2 warm-ups, median of 5): a chunked torch fp32 ``matmul`` + ``topk`` over
the same bytes.  The yardstick is NOT exact (fp32 does not hold these sums); the share of its indices that agree is printed.

    python profiles/scripts/knn_rate.py [--rows 202599] [--pool 16384]
    python profiles/scripts/knn_rate.py --trace     # one warm-up and one call per regime, nothing else: the command to put behind
                                                    # `rocprofv3 --kernel-trace --stats -d DIR --` for the per-kernel split"""
import argparse
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops = eg.ops
DEV = torch.device("cuda:0")
K = 12288
HBM_TBS = 6.29                    # measured float4 copy rate of the micro-architecture guide
BF16_TFLOPS = (840.0, 1010.0)     # what the project's own bf16 GEMMs reach (README)


def events(fn, warm=2, reps=5):
    """median, min, max milliseconds of fn() between device events"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def rows(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.empty(n, K, device=DEV, dtype=torch.uint8)
    for i in range(0, n, 16384):
        out[i:i + 16384] = torch.randint(0, 256, (min(16384, n - i), K), device=DEV, dtype=torch.uint8, generator=g)
    return out


def torch_knn(q, x, k, chunk=8192, self0=-1):
    """the yardstick: |q|^2 + |x|^2 - 2 q x^T in fp32 over chunks of the database, topk per chunk, topk of the chunks' lists"""
    qf = q.float()
    qn = (qf * qf).sum(1, keepdim=True)
    best_d, best_i = [], []
    for j in range(0, x.shape[0], chunk):
        xf = x[j:j + chunk].float()
        d = qn + (xf * xf).sum(1)[None, :] - 2.0 * (qf @ xf.T)
        if self0 >= 0:
            i = torch.arange(q.shape[0], device=DEV)
            hit = (i + self0 >= j) & (i + self0 < j + xf.shape[0])
            d[i[hit], i[hit] + self0 - j] = float("inf")
        dd, ii = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
        best_d.append(dd)
        best_i.append(ii + j)
    d, i = torch.cat(best_d, 1), torch.cat(best_i, 1)
    dd, sel = torch.topk(d, k, dim=1, largest=False)
    return dd, torch.gather(i, 1, sel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=202599)
    ap.add_argument("--pool", type=int, default=16384)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    fmt = lambda t: f"median {t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    x = rows(a.rows, 0)
    q = rows(64, 1)
    q[::2] = x[torch.arange(32, device=DEV) * (a.rows // 32)]                       # half of the queries are dataset rows
    pool = x[:a.pool]
    ops.knn_u8(q[:8], x[:1000], 8)
    ops.knn_u8(pool[:256], pool[:256], 1, 0)
    torch.cuda.synchronize()
    if a.trace:
        ops.knn_u8(q, x, 8)
        ops.knn_u8(pool, pool, 1, 0)
        torch.cuda.synchronize()
        return
    print(f"# {torch.cuda.get_device_name(0)}; rows of K = {K} bytes; tile {ops.knn_tile_queries()} queries x {ops.knn_tile_rows()} rows")

    # (a) 64 queries against the whole dataset
    n, gb = a.rows, a.rows * K / 1e9
    t = events(lambda: ops.knn_u8(q, x, 8))
    ty = events(lambda: torch_knn(q, x, 8))
    d, i = ops.knn_u8(q, x, 8)
    _, iy = torch_knn(q, x, 8)
    least = gb / HBM_TBS
    print(f"(a) eg_knn_u8, 64 x [{n}, {K}], k = 8, {ops.knn_splits(64, n)} slices: {fmt(t)}   reads {gb:.2f} GB once -> {gb / t[0]:.2f} TB/s = "
          f"{100 * least / t[0]:.0f} % of the {HBM_TBS} TB/s read rate (memory bound: least time {least:.3f} ms)")
    print(f"(a) torch fp32 matmul + topk, chunks of 8192 rows:              {fmt(ty)}   ratio torch / hand-written = {ty[0] / t[0]:.1f}")
    print(f"(a) planted rows found at distance 0: {int((d[::2, 0] == 0).sum())} of 32; indices equal to the fp32 yardstick's: "
          f"{100.0 * float((i.long() == iy).float().mean()):.2f} % (the yardstick is not exact)")

    # (b) the pooled leave-one-out call
    N = a.pool
    top = 2.0 * N * N * K / 1e12
    t = events(lambda: ops.knn_u8(pool, pool, 1, 0))
    ty = events(lambda: torch_knn(pool, pool, 1, self0=0))
    _, i = ops.knn_u8(pool, pool, 1, 0)
    _, iy = torch_knn(pool, pool, 1, self0=0)
    lo, hi = (top / (2 * r) for r in BF16_TFLOPS)
    print(f"(b) eg_knn_u8, {N} x {N} leave-one-out, k = 1, {ops.knn_splits(N, N)} slices: {fmt(t)}   {top:.2f} TOP -> {top / t[0] * 1e3:.0f} int8 TOP/s = "
          f"{100 * hi / t[0] * 1e3:.0f}-{100 * lo / t[0] * 1e3:.0f} % of twice the project's bf16 rate ({2 * BF16_TFLOPS[0]:.0f}-{2 * BF16_TFLOPS[1]:.0f})")
    print(f"(b) torch fp32 matmul + topk, chunks of 8192 rows:              {fmt(ty)}   ratio torch / hand-written = {ty[0] / t[0]:.1f}")
    print(f"(b) indices equal to the fp32 yardstick's: {100.0 * float((i[:, 0].long() == iy[:, 0]).float().mean()):.2f} % (the yardstick is not exact)")


if __name__ == "__main__":
    main()

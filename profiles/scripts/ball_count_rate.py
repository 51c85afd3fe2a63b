"""Full-size cost of the ball count behind precision / recall / density / coverage on one GPU.  Prints one table; pipe it into
profiles/ball_count_rate.txt.

Yardstick: ``eg_knn_u8`` at k = 1 on the same operands in the same session -- the same tile loop with strictly more selection work.  The
expectation is that ``eg_ball_count_u8`` takes no longer than the yardstick plus 3 % (the run-to-run spread of profiles/knn_rate.txt,
0.5 - 2 %, rounded up).  The script prints whether it held; it does not fail when it did not.

(a) 8192 x 8192 rows of 12288 bytes: the shape a run scores (MFMA bound)
(b) 64 x 202 599 rows of 12288 bytes: a few queries against the whole dataset (memory bound)
Random bytes, radii = the distance to the 5th nearest other row of the database.  Then one whole ``quality.prdc`` call on 8192 + 8192
CelebA-shaped images, and a chunked torch fp32 count at (a) for scale (NOT exact: fp32 does not hold these sums).  Device events, 2
warm-ups, median of 5.

    python profiles/scripts/ball_count_rate.py
    python profiles/scripts/ball_count_rate.py --knn-only     # the eg_knn_u8 lines alone: runs on a tree without the ball count, for the
                                                              # before / after comparison of the shared tile loop"""
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
MARGIN = 1.03


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


def torch_count(q, x, rad, chunk=8192):
    """for scale: |q|^2 + |x|^2 - 2 q x^T in fp32 over chunks of the database, compared with the radii"""
    qf = q.float()
    qn = (qf * qf).sum(1, keepdim=True)
    count = torch.zeros(q.shape[0], device=DEV, dtype=torch.int64)
    for j in range(0, x.shape[0], chunk):
        xf = x[j:j + chunk].float()
        d = qn + (xf * xf).sum(1)[None, :] - 2.0 * (qf @ xf.T)
        count += (d <= rad[j:j + chunk].float()[None, :]).sum(1)
    return count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=202599)
    ap.add_argument("--pool", type=int, default=8192)
    ap.add_argument("--knn-only", action="store_true")
    a = ap.parse_args()
    fmt = lambda t: f"median {t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    x = rows(a.rows, 0)
    shapes = (("a", rows(a.pool, 1), x[:a.pool]), ("b", rows(64, 2), x))
    print(f"# {torch.cuda.get_device_name(0)}; rows of K = {K} bytes; tile {ops.knn_tile_queries()} queries x {ops.knn_tile_rows()} rows; "
          f"eg_version {eg._lib.lib().query('eg_version')}")
    for tag, q, db in shapes:
        nq, n = q.shape[0], db.shape[0]
        top = 2.0 * nq * n * K / 1e12
        ty = events(lambda: ops.knn_u8(q, db, 1))
        print(f"({tag}) eg_knn_u8 k = 1,     {nq} x [{n}, {K}], {ops.knn_splits(nq, n)} slices: {fmt(ty)}   {top / ty[0] * 1e3:.0f} int8 TOP/s, "
              f"{n * K / 1e9 / ty[0]:.2f} TB/s of database bytes")
        if a.knn_only:
            continue
        rad = ops.knn_u8(db, db, 5, 0)[0][:, 4].contiguous()
        t = events(lambda: ops.ball_count_u8(q, db, rad))
        verdict = "holds" if t[0] <= MARGIN * ty[0] else "FAILS"
        print(f"({tag}) eg_ball_count_u8,    {nq} x [{n}, {K}], {ops.knn_splits(nq, n)} slices: {fmt(t)}   {top / t[0] * 1e3:.0f} int8 TOP/s, "
              f"{n * K / 1e9 / t[0]:.2f} TB/s of database bytes; ball count / yardstick = {t[0] / ty[0]:.3f}: the expectation "
              f"(<= {MARGIN:.2f}) {verdict}")
        count = ops.ball_count_u8(q, db, rad)
        print(f"({tag}) counts: mean {float(count.float().mean()):.3f}, max {int(count.max())}")
        if tag == "a":
            scale = (q, db, rad, count, t[0])
            tr = events(lambda: ops.knn_u8(db, db, 5, 0))
            print(f"(a) eg_knn_u8 k = 5 leave-one-out (one radii search of quality.prdc), {n} x {n}: {fmt(tr)}")
    if a.knn_only:
        return
    real = x[:a.pool].reshape(a.pool, 3, 64, 64)
    fake = shapes[0][1].reshape(a.pool, 3, 64, 64)
    t = events(lambda: eg.quality.prdc(real, fake, 5))
    print(f"quality.prdc, {a.pool} + {a.pool} images [3, 64, 64], k = 5 (five device calls, one host read): {fmt(t)}   {eg.quality.prdc(real, fake, 5)}")
    # last, so that its 400 MB fp32 temporaries and GEMMs are not between a yardstick and the call it is compared with
    q, db, rad, count, t_hand = scale
    tt = events(lambda: torch_count(q, db, rad))
    same = 100.0 * float((torch_count(q, db, rad) == count.long()).float().mean())
    print(f"(a) torch fp32 matmul + compare, chunks of 8192 rows:          {fmt(tt)}   ratio torch / hand-written = {tt[0] / t_hand:.1f}; "
          f"counts equal to the exact ones: {same:.2f} % (fp32 is not exact)")


if __name__ == "__main__":
    main()

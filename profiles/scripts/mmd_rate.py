"""Full-size cost of the two device calls behind the kernel MMD on one GPU.  Prints one table; pipe it into
profiles/mmd_rate.txt.

Yardsticks: ``eg_knn_u8`` at k = 1 and ``eg_ball_count_u8`` on the same operands, alternated with the new calls in the same session -- the
same tile loop with one integer update per distance.  Expectations, written down in DESIGN 6p before the first run:

  select      = passes x the ball count (3 passes at these row lengths): the same loop, one integer update per distance
  kernel sum  = the ball count + the fp64 work of the compiled offer loop: (21 nb + 1) fp64-rate instructions per wave and offer
                (the ISA of knn_ksum_kernel) at 4 cycles each, one wave a SIMD at a time, 1024 SIMDs at 2.4 GHz

The script prints measured / expected for each and whether it is within the 3 % run-to-run spread DESIGN 6o uses; it does not fail when
it is not.

(a) 8192 x 8192 rows of 12288 bytes: the shape a CelebA run scores
(b) 8192 x 8192 rows of 1024 bytes: an MNIST-sized row
Random bytes -- their distances concentrate as hard as distances can (every one within a few per cent of K x 10922), the worst case of the
histogram's same-bin updates.  Then one whole ``quality.mmd`` call on 8192 + 8192 CelebA-shaped images.  Device events, 2 warm-ups, median
of 5.

    python profiles/scripts/mmd_rate.py"""
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
MARGIN = 1.03
SIMDS, CLOCK_GHZ, FP64_CYCLES, EXP_INSTR = 1024, 2.4, 4, 21


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


def rows(n, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, (n, K), device=DEV, dtype=torch.uint8, generator=g)


def fp64_ms(nq, n, nb):
    """the expectation's second term: wave-offers x instructions x cycles, spread over the SIMDs"""
    return nq * n / 64.0 * (EXP_INSTR * nb + 1) * FP64_CYCLES / SIMDS / (CLOCK_GHZ * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=8192)
    a = ap.parse_args()
    fmt = lambda t: f"median {t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    verdict = lambda r: "holds" if r <= MARGIN else "MISSED"
    print(f"# {torch.cuda.get_device_name(0)}; tile {ops.knn_tile_queries()} queries x {ops.knn_tile_rows()} rows; "
          f"eg_version {eg._lib.lib().query('eg_version')}")
    N = a.pool
    for tag, K in (("a", 12288), ("b", 1024)):
        q, db = rows(N, K, 1), rows(N, K, 0)
        head = f"({tag}) {N} x [{N}, {K}], {ops.knn_splits(N, N)} slices"
        rad = ops.knn_u8(db, db, 5, 0)[0][:, 4].contiguous()
        rank = (N * N - 1) // 2
        med = ops.dist_select_u8(q, db, rank)
        igs = {nb: (med[0].double() * torch.tensor([0.5, 1.0, 2.0, 4.0][:nb], device=DEV, dtype=torch.float64)).reciprocal() for nb in (1, 3, 4)}
        ty = events(lambda: ops.knn_u8(q, db, 1))
        tb = events(lambda: ops.ball_count_u8(q, db, rad))
        ts = events(lambda: ops.dist_select_u8(q, db, rank))
        tk = {nb: events(lambda: ops.kernel_sum_u8(q, db, igs[nb])) for nb in (1, 3, 4)}
        tb2 = events(lambda: ops.ball_count_u8(q, db, rad))        # the yardstick again, after the new calls: the session's drift
        ty2 = events(lambda: ops.knn_u8(q, db, 1))
        print(f"{head}: eg_knn_u8 k = 1      {fmt(ty)}; again at the end {fmt(ty2)}")
        print(f"{head}: eg_ball_count_u8     {fmt(tb)}; again at the end {fmt(tb2)}")
        ball = 0.5 * (tb[0] + tb2[0])
        passes = 3
        print(f"{head}: eg_dist_select_u8    {fmt(ts)}   median distance {int(med[0])}; expected {passes} x ball count = {passes * ball:.3f} ms; "
              f"measured / expected = {ts[0] / (passes * ball):.3f}: {verdict(ts[0] / (passes * ball))}")
        for nb in (1, 3, 4):
            want = ball + fp64_ms(N, N, nb)
            print(f"{head}: eg_kernel_sum_u8 nb = {nb} {fmt(tk[nb])}   expected ball count + fp64 = {ball:.3f} + {fp64_ms(N, N, nb):.3f} = {want:.3f} ms; "
                  f"measured / expected = {tk[nb][0] / want:.3f}: {verdict(tk[nb][0] / want)}")
        if tag == "a":
            real, fake = db.reshape(N, 3, 64, 64), q.reshape(N, 3, 64, 64)
            t = events(lambda: eg.quality.mmd(real, fake))
            print(f"quality.mmd, {N} + {N} images [3, 64, 64], scales (0.5, 1, 2) (one select on the pool, three kernel sums, one host read): {fmt(t)}")
            print(f"    {eg.quality.mmd(real, fake)}")


if __name__ == "__main__":
    main()

"""Full-size cost of the device call behind the Sinkhorn divergence on one GPU.  Prints one table; pipe it into
profiles/sinkhorn_rate.txt.

Yardstick: ``eg_kernel_sum_u8`` at nb = 1 on the same operands, alternated with the new call in the same session -- the same tile loop
with one exponential per distance.  Expectation, written down in DESIGN 6q before the first run:

  soft minimum = the kernel sum at nb = 1 + the rest of the compiled offer: a subtraction, a product, a difference, a compare, an
                 addition and an fma at the fp64 rate and four 32-bit selects, some 7 fp64-rate instructions per wave and offer at 4
                 cycles each, one wave a SIMD at a time, 1024 SIMDs at 2.4 GHz: + 0.012 ms at 8192 x 8192, parity within the run-to-run
                 spread

The script prints measured / expected and whether it is within the 3 % run-to-run spread DESIGN 6o uses; it does not fail when it is not.

(a) 8192 x 8192 rows of 12288 bytes: the shape a CelebA run scores
(b) 8192 x 8192 rows of 1024 bytes: an MNIST-sized row
Random bytes; the potentials are spread over a tenth of the median distance, so the running maximum moves.  Then one whole
``quality.sinkhorn`` call on 8192 + 8192 CelebA-shaped random images and on the images of a fresh CelebA generator against a synthetic
dataset, with their marginal errors.  Device events, 2 warm-ups, median of 5.

    python profiles/scripts/sinkhorn_rate.py"""
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
SIMDS, CLOCK_GHZ, FP64_CYCLES, EXTRA_INSTR = 1024, 2.4, 4, 7


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


def extra_ms(nq, n):
    """the expectation's second term: wave-offers x instructions x cycles, spread over the SIMDs"""
    return nq * n / 64.0 * EXTRA_INSTR * FP64_CYCLES / SIMDS / (CLOCK_GHZ * 1e6)


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
        med = ops.dist_select_u8(q, db, (N * N - 1) // 2)[0].double()
        ig = (0.1 * med).reciprocal().reshape(1)
        g = (torch.rand(N, device=DEV, dtype=torch.float64, generator=torch.Generator(device=DEV).manual_seed(2)) - 0.5) * 0.1 * med
        prev = torch.zeros(N, device=DEV, dtype=torch.float64)
        tk = events(lambda: ops.kernel_sum_u8(q, db, ig))
        ts = events(lambda: ops.softmin_u8(q, db, g, ig, prev=prev))
        tk2 = events(lambda: ops.kernel_sum_u8(q, db, ig))          # the yardstick again, after the new call: the session's drift
        ts2 = events(lambda: ops.softmin_u8(q, db, g, ig, prev=prev))
        ksum, soft = 0.5 * (tk[0] + tk2[0]), 0.5 * (ts[0] + ts2[0])
        want = ksum + extra_ms(N, N)
        print(f"{head}: eg_kernel_sum_u8 nb = 1 {fmt(tk)}; again {fmt(tk2)}")
        print(f"{head}: eg_softmin_u8           {fmt(ts)}; again {fmt(ts2)}")
        print(f"{head}: soft minimum / kernel sum = {soft / ksum:.3f}; expected kernel sum + the rest of the offer = {ksum:.3f} + {extra_ms(N, N):.3f} = "
              f"{want:.3f} ms; measured / expected = {soft / want:.3f}: {verdict(soft / want)}")
        if tag == "a":
            real, fake = db.reshape(N, 3, 64, 64), q.reshape(N, 3, 64, 64)
            t = events(lambda: eg.quality.sinkhorn(real, fake), warm=1, reps=3)
            print(f"quality.sinkhorn, {N} + {N} random images [3, 64, 64], scale 0.1, 60 iterations (two selects on the pool, 241 soft minima, one host "
                  f"read): {fmt(t)}")
            print(f"    {eg.quality.sinkhorn(real, fake)}")
            torch.manual_seed(1)
            G = eg.celeba.Generator().to(DEV)
            band = torch.randint(96, 160, (N, 3, 64, 64), device=DEV, dtype=torch.uint8, generator=torch.Generator(device=DEV).manual_seed(5))
            t = events(lambda: eg.quality.sinkhorn_generator("celeba", G, band, n_images=N), warm=1, reps=3)
            print(f"quality.sinkhorn_generator, a fresh CelebA generator, {N} images against {N} synthetic dataset images (bytes in 96 .. 159), "
                  f"generation included: {fmt(t)}")
            print(f"    {eg.quality.sinkhorn_generator('celeba', G, band, n_images=N)}")


if __name__ == "__main__":
    main()

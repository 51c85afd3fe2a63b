"""Full-size cost of the k-means bins behind the NDB score on one GPU.  Prints one table; pipe it into
profiles/kmeans_rate.txt.

Shapes: 8192 and all 202 599 CelebA-shaped rows of 12288 random bytes, 100 bins.  Per shape, warm, device events, median of 5 (min, max):

  one seeding          ops.kmeans_seed_u8: 100 picks, 99 streaming passes over the rows; bytes = 99 n K
  one group_rows       the counting sort of the labels
  one update           ops.kmeans_update_u8 on evenly filled cells and on skewed ones (half of the rows in cell 0); bytes = n K
  one assign           ops.knn_u8(rows, centres, 1)
  one Lloyd iteration  assign + inertia + changed + group_rows + update, as ops.kmeans_u8 enqueues it
  the same in torch    fp32 matmul + argmin + index_add_ (rows converted to fp32 once, outside the timed window)
  quality.ndb          the whole call: 8192 generated rows against the real rows, 20 iterations, its one host read included

Achieved bytes/s are call times (all launches of the call, between device events) against the 6.3 TB/s a streaming copy reaches on this
chip; the issue's estimates -- about 60 ms for the 100 seeding passes and about 2 ms per Lloyd iteration at full
size -- are printed beside what was measured.

    python profiles/scripts/kmeans_rate.py"""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops = eg.ops
DEV = torch.device("cuda:0")
HBM = 6.3e12
K, BINS = 12288, 100


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
    return torch.randint(0, 256, (n, K), device=DEV, dtype=torch.uint8, generator=g)


def main():
    fmt = lambda t: f"median {t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    rate = lambda nbytes, t: f"{nbytes / (t[0] * 1e-3) / 1e12:.2f} TB/s = {nbytes / (t[0] * 1e-3) / HBM:.2f} of 6.3 TB/s"
    print(f"# {torch.cuda.get_device_name(0)}; group_rows block {ops.group_rows_block()}, update segment {ops.kmeans_segment_rows()} rows x "
          f"{ops.kmeans_column_chunk()} bytes, seeding {ops.kmeans_seed_rows()} rows a workgroup; eg_version {eg._lib.lib().query('eg_version')}")
    fake = rows(8192, 9)
    for n in (8192, 202599):
        x = rows(n, 1)
        head = f"[{n}, {K}] x {BINS} bins"
        u = eg.quality.bin_uniforms(0, BINS)
        t = events(lambda: ops.kmeans_seed_u8(x, BINS, u))
        print(f"{head}: one seeding (99 passes)      {fmt(t)}; {t[0] / 99:.4f} ms a pass; {rate(99 * n * K, t)}")
        _, centres = ops.kmeans_seed_u8(x, BINS, u)
        labels = ops.knn_u8(x, centres, 1)[1].reshape(n).contiguous()
        t = events(lambda: ops.group_rows(labels, BINS))
        print(f"{head}: one group_rows               {fmt(t)}")
        for tag, lab in (("even cells", labels), ("half of the rows in cell 0", torch.where(torch.arange(n, device=DEV) % 2 == 0, torch.zeros_like(labels), labels))):
            counts, offsets, order = ops.group_rows(lab.contiguous(), BINS)
            ws = torch.empty(ops.kmeans_update_ws_bytes(n, K, BINS) // 8 + 2, device=DEV, dtype=torch.int64)
            c2 = centres.clone()
            t = events(lambda: ops.kmeans_update_u8(x, order, offsets, counts, c2, ws=ws))
            print(f"{head}: one update, {tag:<27s}{fmt(t)}; {rate(n * K, t)}; largest cell {int(counts.max())} rows")
        t = events(lambda: ops.knn_u8(x, centres, 1))
        print(f"{head}: one assign (knn_u8, k = 1)   {fmt(t)}")
        t = events(lambda: ops.kmeans_u8(x, BINS, 1, init=centres))
        t0 = events(lambda: ops.kmeans_u8(x, BINS, 0, init=centres))
        print(f"{head}: kmeans_u8 with 1 iteration   {fmt(t)}; with 0 iterations {fmt(t0)}; one Lloyd iteration = the difference = {t[0] - t0[0]:.3f} ms")
        xf, cf = x.float(), centres.float()

        def torch_iteration():
            d = (cf * cf).sum(1)[None, :] - 2.0 * (xf @ cf.t())                # + |x|^2, constant per row
            lab = d.argmin(1)
            sums = torch.zeros(BINS, K, device=DEV, dtype=torch.float32).index_add_(0, lab, xf)
            return sums / torch.bincount(lab, minlength=BINS).clamp(min=1)[:, None]
        t = events(torch_iteration)
        print(f"{head}: the same iteration in torch (fp32 matmul + argmin + index_add_; rows already fp32, {xf.numel() * 4 / 1e9:.1f} GB) {fmt(t)}")
        del xf
        real, gen = x.reshape(n, 3, 64, 64), fake.reshape(8192, 3, 64, 64)
        t = events(lambda: eg.quality.ndb(real, gen), warm=1, reps=3)
        print(f"{head}: quality.ndb(real, 8192 generated rows), 20 iterations, one host read: {fmt(t)}")
        print(f"    {eg.quality.ndb(real, gen)}")
        if n > 8192:
            print(f"the issue's estimates at this size: 100 seeding passes about 60 ms, one Lloyd iteration about 2 ms")
        del x, real


if __name__ == "__main__":
    main()

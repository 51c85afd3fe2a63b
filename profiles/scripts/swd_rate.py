"""Full-size cost of the sliced Wasserstein distance on one GPU: CelebA shapes, N = 8192 images of 3 x 64 x 64, P = 128 patches
per image, R = 4 repeats, D = 128 directions -- columns of N P = 2^20 projections.  Prints one table; pipe it into profiles/swd_rate.txt.

1. wall time of one ``quality.swd`` call (host clock around the call, which ends in its one host read), median of --calls after one warm-up;
2. the stages alone at level 64, each between device events, median of 5 after 2 warm-ups: pyramid, patch statistics, projection, column
   sort, L1 reduction -- with the bytes each global sort pass moves against the measured rate;
3. the yardstick of the sort: ``torch.sort(x, dim=1)`` on the same [128][2^20] tensor, the same protocol, in the same session.

    python profiles/scripts/swd_rate.py [--images 8192] [--calls 3]
    python profiles/scripts/swd_rate.py --trace        # one warm-up and one swd call, nothing else: the command to put behind
                                                        # `rocprofv3 --kernel-trace --stats -d DIR --` for the per-kernel split"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops, quality = eg.ops, eg.quality
DEV = torch.device("cuda:0")


def sets(n):
    g = torch.Generator(device=DEV).manual_seed(0)
    real = torch.randint(0, 256, (n, 3, 64, 64), device=DEV, dtype=torch.uint8, generator=g).float() * (2.0 / 255.0) - 1.0
    fake = torch.tanh(torch.randn(n, 3, 64, 64, device=DEV, generator=g))
    fake = (fake + torch.roll(fake, 1, 3)) * 0.5
    return real, fake


def events(fn, warm=2, reps=5):
    """median milliseconds of fn() between device events"""
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


def sort_passes(n, T):
    """(LDS passes, global passes) eg_sort_columns_f32 launches for a column of n elements: the library's own schedule"""
    npad = 1
    while npad < n:
        npad *= 2
    lds, glob, K = 1, 0, 2 * T
    while K <= npad:
        steps = (K // (2 * T)).bit_length()          # flip(K) and the strides K/4 ... T
        glob += (steps + 1) // 2
        lds += 1
        K *= 2
    return lds, glob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--patches", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--dirs", type=int, default=128)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    N, P, Rn, D = a.images, a.patches, a.repeats, a.dirs
    real, fake = sets(N)
    kw = dict(patches_per_image=P, repeats=Rn, dirs=D, seed=0)
    res = quality.swd(real[:64], fake[:64], **kw)                    # loads every kernel
    torch.cuda.synchronize()
    if a.trace:
        print("swd", quality.swd(real, fake, **kw))
        return
    print(f"# {torch.cuda.get_device_name(0)}; N = {N}, C = 3, H = 64, P = {P}, R = {Rn}, D = {D}: columns of {N * P} projections, {len(res['levels'])} levels")
    quality.swd(real, fake, **kw)
    wall = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = quality.swd(real, fake, **kw)
        wall.append((time.perf_counter() - t0) * 1e3)
    print(f"quality.swd, one call (wall, ends in its host read): median {statistics.median(wall):.1f} ms of {a.calls} (min {min(wall):.1f}, max {max(wall):.1f})   result {res}")

    # the stages alone, level 64
    n_desc, C, H = N * P, 3, 64
    ld = ops.round_up(n_desc, 4)
    pos, dirs = quality.draw_plan(0, real.shape, P, 1, D)
    pyr = quality.laplacian_pyramid(real)
    stats = torch.empty(C, 2, device=DEV, dtype=torch.float64)
    sws = torch.empty(ops.swd_patch_stats_ws_doubles(C), device=DEV, dtype=torch.float64)
    pws = torch.empty(ops.swd_project_ws_floats(C), device=DEV)
    lws = torch.empty(ops.l1_mean_ws_doubles(), device=DEV, dtype=torch.float64)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    out = torch.zeros(1, device=DEV, dtype=torch.float64)
    proj = torch.empty(2, D, ld, device=DEV)
    fmt = lambda t: f"median {t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    t = events(lambda: quality.laplacian_pyramid(real))
    print(f"laplacian_pyramid ({N} x 3 x 64 x 64, clone + 2 down + 2 up_sub):      {fmt(t)}")
    t = events(lambda: ops.swd_patch_stats(pyr[0], pos[0], n_desc, P, C, H, sws, stats, flag))
    print(f"eg_swd_patch_stats (level 64, {n_desc * 147 / 1e6:.0f} M pixels in double):        {fmt(t)}")
    t = events(lambda: ops.swd_project(pyr[0], pos[0], n_desc, P, C, H, dirs[0][0], D, stats, pws, proj[0], ld))
    flop = 2.0 * n_desc * 147 * D
    print(f"eg_swd_project (level 64, VALU fp32, {flop / 1e9:.1f} GFLOP, writes {D * n_desc * 4 / 1e6:.0f} MB):  {fmt(t)}   {flop / t[0] / 1e9:.1f} TFLOP/s")
    ops.swd_project(pyr[0], pos[0], n_desc, P, C, H, dirs[0][0], D, stats, pws, proj[1], ld)
    keep = proj[0].clone()

    def hand():
        proj[1].copy_(keep)
        ops.sort_columns(proj[1], n_desc)

    def yard():
        proj[1].copy_(keep)
        torch.sort(proj[1], dim=1)

    tc = events(lambda: proj[1].copy_(keep))
    th, ty = events(hand), events(yard)
    assert torch.equal(proj[1][:, :n_desc].sort(dim=1).values, ops.sort_columns(keep.clone(), n_desc)[:, :n_desc])
    T = ops.sort_tile_elems()
    lds, glob = sort_passes(n_desc, T)
    per_pass = 2.0 * D * n_desc * 4
    hs, ys = th[0] - tc[0], ty[0] - tc[0]
    print(f"copy of the [{D}][{n_desc}] tensor (subtracted below):                      {fmt(tc)}")
    print(f"eg_sort_columns_f32 + that copy:                                         {fmt(th)}")
    print(f"torch.sort(x, dim=1) + that copy:                                        {fmt(ty)}")
    print(f"sort alone: hand-written {hs:.3f} ms, torch.sort {ys:.3f} ms, ratio hand / torch = {hs / ys:.2f}")
    print(f"sort passes at T = {T}: {lds} through LDS + {glob} global, each reads and writes the tensor once = {per_pass / 1e9:.3f} GB per pass, "
          f"{(lds + glob) * per_pass / 1e9:.1f} GB per sort -> {(lds + glob) * per_pass / hs / 1e9:.2f} TB/s averaged over all passes")
    t = events(lambda: ops.l1_mean(proj[0], proj[1], n_desc, D, ld, lws, out))
    print(f"eg_l1_mean_f32 (reads {per_pass / 1e9:.3f} GB):                                       {fmt(t)}   {per_pass / t[0] / 1e9:.2f} TB/s")


if __name__ == "__main__":
    main()

"""Full-size cost of the pair scores (SSIM / MS-SSIM) on one GPU.  Prints one table; pipe it into profiles/ssim_rate.txt.

Shapes: 65 536 pairs (``quality.pair_table``) of 8192 images of random bytes, 3 x 64 x 64 with L = 3 levels and 1 x 32 x 32 with L = 2, the
11-tap Gaussian.  Per shape, warm, device events around ``inner`` back-to-back calls, median of 7 windows (min, max), per call:

  ops.ssim_u8          the one launch of eg_ssim_u8
  the torch route      on the same device, in doubles: the two images of a pair gathered by indexing, the five planes x, y, x^2, y^2, x y
                       filtered by two grouped F.conv2d (the window along a row, then along a column), cs and ssim and their means, then
                       F.avg_pool2d for the next level; the conversion to double is inside the window (the kernel reads bytes too); the
                       pairs go through it in chunks of 2048 (the five planes of all 65 536 pairs would be 32 GB)
  quality.diversity_generator   the whole call at its defaults (8192 generated and 8192 real images, 16 384 pairs) on a fresh generator,
                       its one host read included

fp64 FMAs of the separable filter by the formula sum_l C 5 K (H_l n_l + n_l^2), n_l = H_l - K + 1; the rate is those x 2 flops over the
call time, against the 78.6 TFLOP/s fp64 vector peak (256 CUs x 64 lanes x 2 x 2.4 GHz).  The two routes are alternated in one session and
their results compared.

    python profiles/scripts/ssim_rate.py"""
import importlib
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops = eg.ops
DEV = torch.device("cuda:0")
PEAK = 78.6e12
CHUNK = 2048
K = 11


def events(fn, inner=1, warm=2, reps=7):
    """median, min, max milliseconds of one fn() from windows of ``inner`` calls between device events"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out), min(out), max(out)


def torch_route(x, pairs, win, L, c1, c2):
    P, C = pairs.shape[0], x.shape[1]
    out = torch.empty(P, L, 2, device=x.device, dtype=torch.float64)
    wr = win.reshape(1, 1, 1, K).repeat(5 * C, 1, 1, 1)
    wc = win.reshape(1, 1, K, 1).repeat(5 * C, 1, 1, 1)
    idx = pairs.long()
    for i in range(0, P, CHUNK):
        a, b = x[idx[i:i + CHUNK, 0]].double(), x[idx[i:i + CHUNK, 1]].double()
        for l in range(L):
            planes = torch.cat((a, b, a * a, b * b, a * b), 1)
            m = F.conv2d(F.conv2d(planes, wr, groups=5 * C), wc, groups=5 * C)
            ma, mb, eaa, ebb, eab = m.split(C, 1)
            cs = (2 * (eab - ma * mb) + c2) / (eaa - ma * ma + ebb - mb * mb + c2)
            lum = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
            out[i:i + CHUNK, l, 0] = (lum * cs).mean((1, 2, 3))
            out[i:i + CHUNK, l, 1] = cs.mean((1, 2, 3))
            if l + 1 < L:
                a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return out


def main():
    fmt = lambda t: f"median {t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    print(f"# {torch.cuda.get_device_name(0)}; eg_version {eg._lib.lib().query('eg_version')}")
    win = ops.ssim_window_table(K, 1.5, DEV)
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    P = 65536
    for N, C, H, inner in ((8192, 3, 64, 5), (8192, 1, 32, 50)):
        g = torch.Generator(device=DEV).manual_seed(N + H)
        x = torch.randint(0, 256, (N, C, H, H), device=DEV, dtype=torch.uint8, generator=g)
        pairs = eg.quality.pair_table(N, P, 0, DEV)
        L = ops.ssim_levels(H, K)
        fmas = sum(C * 5 * K * ((H >> l) * ((H >> l) - K + 1) + ((H >> l) - K + 1) ** 2) for l in range(L))
        flops = 2.0 * P * fmas
        head = f"[{P} pairs of {C} x {H} x {H}, L = {L}]"
        for _ in range(2):                                                   # alternated: kernel, torch, kernel, torch
            t = events(lambda: ops.ssim_u8(x, x, pairs, win), inner)
            print(f"{head}: ops.ssim_u8                  {fmt(t)}; {flops / (t[0] * 1e-3) / 1e12:.1f} TFLOP/s fp64 = {flops / (t[0] * 1e-3) / PEAK:.2f} of the vector peak")
            tt = events(lambda: torch_route(x, pairs, win, L, c1, c2), 1, warm=1, reps=3)
            print(f"{head}: torch conv2d + avg_pool2d    {fmt(tt)}; {tt[0] / t[0]:.2f} x the kernel's time", flush=True)
        got, ref = ops.ssim_u8(x, x, pairs[:CHUNK], win)[0], torch_route(x, pairs[:CHUNK], win, L, c1, c2)
        bound = (8 / 0.01 ** 2 + 12 / 0.03 ** 2) * (2 * K + 2) * 2.0 ** -53
        print(f"{head}: |kernel - torch| / ((8 / k1^2 + 12 / k2^2)(2 K + 2) 2^-53) over the first {CHUNK} pairs: max {float((got - ref).abs().max()) / bound:.3e}")
        t = events(lambda: eg.quality.diversity(x, n_pairs=16384), 1, warm=1, reps=5)
        print(f"{head}: quality.diversity(8192 images, 16 384 pairs), one host read: {fmt(t)}  -> {eg.quality.diversity(x, n_pairs=16384)}")
        del x
    for kind, mod, shape in (("celeba", eg.celeba, (3, 64, 64)), ("mnist", eg.mnist, (1, 32, 32))):
        torch.manual_seed(0)
        G = mod.Generator().to(DEV)
        data = torch.randint(0, 256, (8192,) + shape, device=DEV, dtype=torch.uint8, generator=torch.Generator(device=DEV).manual_seed(1))
        t = events(lambda: eg.quality.diversity_generator(kind, G, data), 1, warm=1, reps=3)
        got = eg.quality.diversity_generator(kind, G, data)
        print(f"[{kind}] quality.diversity_generator at its defaults (fresh generator, random bytes as the data): {fmt(t)}", flush=True)
        print(f"[{kind}]   -> real ms_ssim {got['real']['ms_ssim']:.6f}, fake ms_ssim {got['fake']['ms_ssim']:.6f}, gap {got['gap']:.6f}, levels {got['fake']['levels']}, "
              f"duplicates {got['fake']['duplicates']}")


if __name__ == "__main__":
    main()

"""Weight gradient of the CelebA image-side layers (3 <-> 128 channels, B = 128, bf16; T tapes batched along M) per launch, back to back:
eg_im2col_img per tape + eg_conv_wgrad over the patch rows against eg_wgrad_img_tn, which reads the images themselves.  Device events
around `inner` launches, 2 warm-up rounds, median of 5; bytes = what each path has to move (fp32 images, P, slab; the pair also writes and
reads the patch rows) divided by the time.
usage: python profiles/scripts/wgrad_img_tn_layers.py [--T 1,2,3] [--inner 10]"""
import argparse
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops = eg.ops


def timed(fn, inner, warm=2, rounds=5):
    ts = []
    for r in range(warm + rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        if r >= warm:
            ts.append(e0.elapsed_time(e1) * 1e-3 / inner)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", default="1,2,3")
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    dt, dev, B, C, S, N = ops.EG_BF16, "cuda", 128, 3, 64, 128
    g = torch.Generator(device=dev).manual_seed(1)
    for T in [int(t) for t in a.T.split(",")]:
        imgs = [torch.rand(B, C, S, S, device=dev, generator=g) * 2 - 1 for _ in range(T)]
        M, npix = T * B * 1024, B * 1024
        P = (torch.rand(M, N, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
        patches = torch.empty(M, 16 * C, device=dev, dtype=torch.bfloat16)
        c = ops.make_conv(T * B, S // 2, S // 2, 16 * C, N, 1, 1, 0)
        ns, rps = ops.wgrad_img_tn_plan(T * B, C, 0)
        slab_a, slab_b = torch.empty(ns, N, 16 * C, device=dev), torch.empty(ns, N, 16 * C, device=dev)

        def pair():
            for t, im in enumerate(imgs):
                ops.im2col_img(dt, im, patches[t * npix:(t + 1) * npix], B, C, S, S, 4, 2, 1, 16 * C)
            assert ops.conv_wgrad(c, dt, patches, P, slab_a, 0) == ns

        def direct():
            assert ops.wgrad_img_tn(dt, imgs, P, slab_b, B, C, S, S, N, 0) == ns

        t_pair, t_new = timed(pair, a.inner), timed(direct, a.inner)
        torch.cuda.synchronize()
        assert torch.equal(slab_a, slab_b)
        need = T * B * C * S * S * 4 + P.numel() * 2 + slab_a.numel() * 4
        moved = need + 2 * patches.numel() * 2
        print(f"T={T}  splits {ns:3d} x {rps // 32:3d} steps   im2col + tn {t_pair * 1e6:7.1f} us = {moved / t_pair / 1e12:5.2f} TB/s of {moved / 1e6:6.1f} MB   "
              f"wgrad_img_tn {t_new * 1e6:7.1f} us = {need / t_new / 1e12:5.2f} TB/s of {need / 1e6:6.1f} MB   x{t_pair / t_new:4.2f}", flush=True)


if __name__ == "__main__":
    main()

"""Full-size cost of the radial power spectrum on one GPU.  Prints one table; pipe it into profiles/spectrum_rate.txt.

Shapes: 8192 x 3 x 64 x 64, 8192 x 1 x 32 x 32 and all 202 599 CelebA-shaped images of random bytes.  Per shape, warm, device events around
``inner`` back-to-back calls (so that a window is tens of milliseconds), median of 7 windows (min, max), per call:

  ops.spectrum_u8      the one launch of eg_spectrum_u8, profile only and with `full`
  the torch route      torch.fft.rfft2(x.double()), the squared modulus / H^2, the channel mean, the column weights and index_add_ over the
                       ring table (the conversion to double is inside the window: the kernel reads bytes too); the 202 599 images go
                       through it in chunks of 8192, as 30 GB of doubles and half-spectra would otherwise be live at once
  quality.spectrum     the whole call on 8192 + 8192 images, its one host read included

fp64 FMAs of the direct two-stage DFT: H (H/2 + 1) H (2 + 4) per channel; the rate is those x 2 flops over the call time, against the
78.6 TFLOP/s fp64 vector peak (256 CUs x 64 lanes x 2 x 2.4 GHz).  The two routes are alternated in one session and their profiles compared.

    python profiles/scripts/spectrum_rate.py"""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops = eg.ops
DEV = torch.device("cuda:0")
PEAK = 78.6e12
CHUNK = 8192


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


def torch_route(x, tab, weight):
    N, C, H, _ = x.shape
    out = torch.empty(N, tab["rings"], device=x.device, dtype=torch.float64)
    ring = tab["cell_ring"].reshape(-1).long()
    for i in range(0, N, CHUNK):
        F = torch.fft.rfft2(x[i:i + CHUNK].double())
        P = ((F.real ** 2 + F.imag ** 2) / float(H * H)).mean(1) * weight
        sums = torch.zeros(tab["rings"], P.shape[0], device=x.device, dtype=torch.float64).index_add_(0, ring, P.reshape(P.shape[0], -1).t())
        out[i:i + CHUNK] = (sums / tab["ring_count"].double()[:, None]).t()
    return out


def main():
    fmt = lambda t: f"median {t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    print(f"# {torch.cuda.get_device_name(0)}; eg_version {eg._lib.lib().query('eg_version')}")
    for N, C, H, inner in ((8192, 3, 64, 20), (8192, 1, 32, 100), (202599, 3, 64, 1)):
        g = torch.Generator(device=DEV).manual_seed(N + H)
        x = torch.randint(0, 256, (N, C, H, H), device=DEV, dtype=torch.uint8, generator=g)
        tab = ops.spectrum_tables(H, DEV)
        weight = torch.tensor([1.0 if kx in (0, H // 2) else 2.0 for kx in range(H // 2 + 1)], device=DEV, dtype=torch.float64)
        flops = 2.0 * N * C * H * (H // 2 + 1) * H * 6
        head = f"[{N}, {C}, {H}, {H}]"
        for _ in range(2):                                                   # alternated: kernel, torch, kernel, torch
            t = events(lambda: ops.spectrum_u8(x), inner)
            print(f"{head}: ops.spectrum_u8              {fmt(t)}; {flops / (t[0] * 1e-3) / 1e12:.1f} TFLOP/s fp64 = {flops / (t[0] * 1e-3) / PEAK:.2f} of the vector peak")
            tt = events(lambda: torch_route(x, tab, weight), max(1, inner // 10), reps=5)
            print(f"{head}: torch rfft2 + index_add_     {fmt(tt)}; {tt[0] / t[0]:.2f} x the kernel's time")
        t = events(lambda: ops.spectrum_u8(x, full=True), inner)
        print(f"{head}: ops.spectrum_u8(full=True)   {fmt(t)}")
        a, b = ops.spectrum_u8(x[:CHUNK]), torch_route(x[:CHUNK], tab, weight)
        S = x[:CHUNK].reshape(CHUNK, C, -1).long().sum(2).max(1).values.double()
        print(f"{head}: |kernel - torch| / (2^-50 S^2 / H) over the first {CHUNK} images: max {float(((a - b).abs() / (2.0 ** -50 * S * S / H)[:, None]).max()):.3e}")
        if N == 8192:
            y = torch.randint(0, 256, (N, C, H, H), device=DEV, dtype=torch.uint8, generator=g)
            t = events(lambda: eg.quality.spectrum(x, y), 1, warm=1, reps=5)
            print(f"{head}: quality.spectrum(8192 + 8192 images), one host read: {fmt(t)}")
        del x


if __name__ == "__main__":
    main()

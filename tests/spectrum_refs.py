"""The radial power spectrum restated in numpy float64, sharing nothing with the kernel: the power comes from np.fft.rfft2,
the rings from the integer rule, the statistics from their definitions.  Images are uint8 arrays [N, C, H, H]."""
import math

import numpy as np

FLOOR = 1.0 / 12.0


def tables(H):
    """-> {"rings", "cell_ring" [H, H/2 + 1], "ring_start" [B + 1], "ring_cells", "ring_count" [B], "weight" [H/2 + 1]}, int32"""
    KX = H // 2 + 1
    weight = np.full(KX, 2, np.int32)
    weight[0] = weight[H // 2] = 1
    cell_ring = np.zeros((H, KX), np.int32)
    for ky in range(H):
        for kx in range(KX):
            q = min(ky, H - ky) ** 2 + kx ** 2
            s = math.isqrt(q)
            cell_ring[ky, kx] = s if q <= s * s + s else s + 1
    B = int(cell_ring.max()) + 1
    cells = [[ky * KX + kx for ky in range(H) for kx in range(KX) if cell_ring[ky, kx] == b] for b in range(B)]
    ring_start = np.cumsum([0] + [len(c) for c in cells]).astype(np.int32)
    ring_count = np.array([sum(int(weight[i % KX]) for i in c) for c in cells], np.int32)
    return {"rings": B, "cell_ring": cell_ring, "ring_start": ring_start, "ring_cells": np.array(sum(cells, []), np.int32),
            "ring_count": ring_count, "weight": weight}


def power(images):
    """-> P float64 [N, C, H, H/2 + 1] = |rfft2 of the bytes|^2 / H^2"""
    x = np.asarray(images)
    assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[2] == x.shape[3]
    F = np.fft.rfft2(x.astype(np.float64), axes=(2, 3))
    return (F.real ** 2 + F.imag ** 2) / float(x.shape[2] ** 2)


def full(images):
    """-> float64 [N, H, H/2 + 1]: the mean of P over the channels"""
    return power(images).mean(1)


def profile(images):
    """-> float64 [N, B]: profile[n, b] = sum_c sum_{cells of ring b} w P / (C ring_count[b])"""
    P = power(images)
    N, C, H, KX = P.shape
    tab = tables(H)
    wP = (P * tab["weight"].astype(np.float64)).sum(1).reshape(N, H * KX)
    member = (tab["cell_ring"].reshape(-1, 1) == np.arange(tab["rings"])).astype(np.float64)         # [cells, B] of 0 / 1
    return (wP @ member) / (C * tab["ring_count"].astype(np.float64))


def profile_tolerance(images):
    """-> float64 [N, 1]: 2^-50 S^2 / H per entry, S the image's largest per-channel byte sum (twice the derived 4 H u S^2 / H^2)"""
    x = np.asarray(images)
    S = x.reshape(x.shape[0], x.shape[1], -1).astype(np.int64).sum(2).max(1).astype(np.float64)
    return (2.0 ** -50 * S * S / x.shape[2])[:, None]


def log_db(p):
    return 10.0 * np.log10(p + FLOOR)


def db_tolerance(images, ref_profile=None):
    """-> float64 [B]: the profile's tolerance carried through 10 log10(p + 1/12), averaged over the set, + 1e-9 dB"""
    ref = profile(images) if ref_profile is None else ref_profile
    return ((10.0 / math.log(10.0)) * profile_tolerance(images) / (ref + FLOOR) + 1e-9).mean(0)


def moments(images):
    """-> (mean [B], unbiased variance [B]) over the set of the log-profiles in dB"""
    L = log_db(profile(images))
    return L.mean(0), L.var(0, ddof=1)


def statistics(mr, vr, mf, vf, H):
    mr, vr, mf, vf = (np.asarray(v, np.float64) for v in (mr, vr, mf, vf))
    B = len(mr)
    gap = mf - mr
    mag = np.abs(gap[1:])
    peak = 1 + int(np.flatnonzero(mag == mag.max())[0])
    pooled = np.sqrt(0.5 * (vr + vf))
    effect = np.where(pooled > 0.0, gap / np.where(pooled > 0.0, pooled, 1.0), 0.0)
    return {"rings": B, "real_db": mr.tolist(), "fake_db": mf.tolist(), "gap_db": gap.tolist(), "distance_db": float(np.sqrt(np.mean(gap[1:] ** 2))),
            "high_db": float(np.mean(gap[np.arange(B) > H / 4])), "peak_db": float(gap[peak]), "peak_ring": peak, "effect": effect.tolist()}


def spectrum(real, fake):
    mr, vr = moments(real)
    mf, vf = moments(fake)
    return statistics(mr, vr, mf, vf, np.asarray(real).shape[2])


def mean_spectrum(images):
    """-> float64 [H, H]: 10 log10(mean_n full + 1/12) on the full plane, zero frequency at [H/2, H/2]"""
    x = np.asarray(images).astype(np.float64)
    F = np.fft.fft2(x, axes=(2, 3))
    P = ((F.real ** 2 + F.imag ** 2) / float(x.shape[2] ** 2)).mean(1).mean(0)
    return np.fft.fftshift(log_db(P))


# ---- the inputs of the tests ------------------------------------------------------------------------------------------------------------
def pink(rng, N, C, H, std=40.0):
    """1/f-filtered noise (amplitude ~ 1 / |f|) around 128 with a standard deviation of ``std`` grey levels, clipped to bytes"""
    f = np.hypot(np.fft.fftfreq(H)[:, None], np.fft.fftfreq(H)[None, :])
    f[0, 0] = 1.0 / H
    x = np.fft.ifft2(np.fft.fft2(rng.standard_normal((N, C, H, H))) / f).real
    x = 128.0 + std * x / x.std()
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def lattice(images, levels=6):
    """+ ``levels`` grey levels on the even / even pixel lattice, clipped"""
    out = np.asarray(images).astype(np.int64)
    out[..., ::2, ::2] += levels
    return np.clip(out, 0, 255).astype(np.uint8)

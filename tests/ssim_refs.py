"""numpy restatement of the pair scores: the contract of ``eg_ssim_u8`` with plain slicing, and what quality.py builds on it.

    levels   x_l = 4^-l (integer sum of the 2^l x 2^l block of bytes), side H_l = H >> l
    moments  sum_dy win[dy] sum_dx win[dx] (.)[r + dy][q + dx] of x, y, x^2, y^2, x y over the valid positions: rows first, then columns,
             every sum in index order, in ``dtype``
    values   cs = (2 s_ab + c2) / (s_aa + s_bb + c2), lum = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1), ssim = lum cs
    stats[p][l] = (mean ssim, mean cs) over channels and positions; sse[p] = sum (a - b)^2, an exact integer

``dtype=np.longdouble`` runs the same statements in extended precision: the yardstick of the float64 run's own rounding."""
import numpy as np

K1, K2 = 0.01, 0.03
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SIDES = (16, 32, 64)


def window(K=11, sigma=1.5, dtype=np.float64):
    if sigma is None:
        return np.full(K, 1.0, dtype) / dtype(K)
    k = np.arange(K, dtype=np.float64) - (K // 2)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(dtype)              # the float64 table IS the contract's window: the long-double run filters with the same taps


def levels(H, K):
    L = 1
    while (H >> L) >= K:
        L += 1
    return L


def pooled(x, l):
    """[..., H, H] integers -> the integer block sums [..., H >> l, H >> l] of the 2^l x 2^l blocks"""
    s = 1 << l
    H = x.shape[-1]
    return x.astype(np.int64).reshape(x.shape[:-2] + (H // s, s, H // s, s)).sum((-3, -1))


def _filter(plane, w):
    """[..., S, S] -> [..., n, n]: rows first (the inner sum runs along a row), then columns, each sum in index order"""
    K = len(w)
    n = plane.shape[-1] - K + 1
    rows = w[0] * plane[..., :, 0:n]
    for dx in range(1, K):
        rows = rows + w[dx] * plane[..., :, dx:dx + n]
    out = w[0] * rows[..., 0:n, :]
    for dy in range(1, K):
        out = out + w[dy] * rows[..., dy:dy + n, :]
    return out


def stats(a, b, pairs, K=11, sigma=1.5, L=None, dtype=np.float64, k1=K1, k2=K2):
    """-> (stats ``dtype`` [P, L, 2], sse int64 [P]) for uint8 sets a [na, C, H, H], b [nb, C, H, H] and an integer table pairs [P, 2]"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    H = a.shape[-1]
    L = levels(H, K) if L is None else L
    w = window(K, sigma).astype(dtype)
    c1, c2 = dtype((k1 * 255.0) ** 2), dtype((k2 * 255.0) ** 2)
    x8, y8 = a[pairs[:, 0]], b[pairs[:, 1]]
    out = np.empty((len(pairs), L, 2), dtype)
    for l in range(L):
        x = pooled(x8, l).astype(dtype) / dtype(4 ** l)
        y = pooled(y8, l).astype(dtype) / dtype(4 ** l)
        ma, mb, eaa, ebb, eab = (_filter(p, w) for p in (x, y, x * x, y * y, x * y))
        saa, sbb, sab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
        cs = (2 * sab + c2) / (saa + sbb + c2)
        lum = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
        out[:, l, 0] = (lum * cs).mean((1, 2, 3))
        out[:, l, 1] = cs.mean((1, 2, 3))
    d = x8.astype(np.int64) - y8.astype(np.int64)
    return out, (d * d).sum((1, 2, 3))


def weights(L, w=None):
    if w is not None:
        return np.asarray(w, np.float64)
    first = np.asarray(WEIGHTS[:L], np.float64)
    return first / first.sum() if L < len(WEIGHTS) else first               # fewer than five levels: the first L over their sum


def bases(st):
    """[P, L, 2] -> [P, L]: cs of the levels below the last, ssim of the last, clamped at 0"""
    L = st.shape[1]
    return np.maximum(np.concatenate((st[:, :L - 1, 1], st[:, L - 1:, 0]), 1).astype(np.float64), 0.0)


def ms_ssim(st, w=None):
    """prod_{l < L - 1} max(cs_l, 0)^w_l * max(ssim_{L-1}, 0)^w_{L-1}; the default weights: ``weights``"""
    return np.prod(bases(st) ** weights(st.shape[1], w), 1)


def ms_ssim_rtol(st, K=11):
    """the relative tolerance of an MS-SSIM comparison, per pair: tolerance(K) / max(clamped base over the levels)"""
    return tolerance(K) / bases(st).max(1)


def psnr(sse, numel):
    sse = np.asarray(sse, np.float64)
    return np.where(sse == 0, np.inf, 10.0 * np.log10(255.0 ** 2 * numel / np.where(sse == 0, 1.0, sse)))


def pair_table_from_draws(i, jp):
    """i in [0, n), j' in [0, n - 1) -> int32 [P, 2]: (i, j' + (j' >= i)), ordered pairs of different rows"""
    i, jp = np.asarray(i, np.int64), np.asarray(jp, np.int64)
    return np.stack((i, jp + (jp >= i)), 1).astype(np.int32)


def error_bound(K, k1=K1, k2=K2):
    """|d ssim| <= (8 / k1^2 + 12 / k2^2) (2 K + 2) 2^-53: a moment is two K-term dot products with positive weights summing to 1 over
    values <= 255^2, |d moment| <= (2 K + 2) u 255^2; lum's denominator is >= c1 = k1^2 255^2, cs's is >= c2"""
    return (8.0 / k1 ** 2 + 12.0 / k2 ** 2) * (2 * K + 2) * 2.0 ** -53


def tolerance(K, k1=K1, k2=K2):
    """what the tests assert: TWICE the bound (numpy's own error and the device's FMA contraction)"""
    return 2.0 * error_bound(K, k1, k2)


# ---- test images ------------------------------------------------------------------------------------------------------------------------------
def pink(rng, N, C, H):
    """uint8 [N, C, H, H] with a 1 / f amplitude spectrum, stretched to the full byte range per image"""
    f = np.fft.fftfreq(H)
    r = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    r[0, 0] = 1.0
    x = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((N, C, H, H))) / r))
    lo, hi = x.min((1, 2, 3), keepdims=True), x.max((1, 2, 3), keepdims=True)
    return np.clip(np.rint((x - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)


def related(rng, N, C, H):
    """``pink`` images that share a half (the mean of one common image and an own one): every pair's cs stays well above 0"""
    p = pink(rng, N + 1, C, H).astype(np.int64)
    return ((p[:1] + p[1:]) // 2).astype(np.uint8)


def noisy(rng, x, amp=20):
    return np.clip(x.astype(np.int64) + rng.randint(-amp, amp + 1, x.shape), 0, 255).astype(np.uint8)


def image_sets(rng, N, C, H):
    """the kinds of image pairs the tests score -> {name: (a, b)} of uint8 [N, C, H, H]"""
    u = rng.randint(0, 256, (N, C, H, H)).astype(np.uint8)
    p = pink(rng, N, C, H)
    four = (rng.randint(0, 4, (N, C, H, H)) * 85).astype(np.uint8)
    flat = rng.randint(0, 256, (N, C, H, H)).astype(np.uint8)
    flat[N // 2] = 77
    return {"uniform": (u, rng.randint(0, 256, (N, C, H, H)).astype(np.uint8)), "pink": (p, noisy(rng, p)),
            "four": (four, (rng.randint(0, 4, (N, C, H, H)) * 85).astype(np.uint8)), "flat": (flat, u), "negative": (p, 255 - p)}

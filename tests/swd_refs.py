"""Float64 numpy restatement of the sliced Wasserstein distance of DESIGN 6m (Karras et al., "Progressive Growing of GANs", 2018), written
from its definition and not from the product code; positions and directions are explicit arguments.  Next to every stage stands the
elementwise rounding bound of an fp32 evaluation of that stage, formed from the same float64 terms.

  levels      H, H/2 ... 16; g = outer([1,4,6,4,1], [1,4,6,4,1]) / 256; border i < 0 -> -i, i >= n -> 2(n-1) - i
  down(x)     5 x 5 correlation with g, every second row and column from 0
  up(x)       x in the even positions of a zero image of twice the size, filtered with 4 g
  pyramid     pyr[l+1] = down(pyr[l]); pyr[l] -= up(pyr[l+1]); the coarsest level stays Gaussian
  descriptor  i of a level: the 7 x 7 x C patch of image i // P around (y, x) = positions[i], flattened as k = c * 49 + dy * 7 + dx
  normalise   per set, level and channel: (d - mean) / population std over all descriptors and the 49 pixels of the channel
  distance    per repeat: project on the unit columns of a [49 C, D] matrix, sort every column of each set, mean |sortedA - sortedB|;
              the level's value is the mean over repeats, reported times 1e3
"""
import numpy as np

U = 2.0 ** -24                                           # unit roundoff of fp32
TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
G = np.outer(TAPS, TAPS) / 256.0
MIN_SIDE = 16


def level_sides(H):
    sides = []
    while H >= MIN_SIDE:
        sides.append(H)
        H //= 2
    return sides


def _mirror(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _filter(x, kernel):
    """5 x 5 correlation of the last two axes of x with ``kernel`` under the mirror border, same size"""
    H, W = x.shape[-2:]
    out = np.zeros(x.shape, np.float64)
    ys, xs = np.arange(H), np.arange(W)
    for a in range(5):
        rows = x[..., _mirror(ys + a - 2, H), :]
        for b in range(5):
            out += kernel[a, b] * rows[..., :, _mirror(xs + b - 2, W)]
    return out


def down(x):
    return _filter(np.asarray(x, np.float64), G)[..., ::2, ::2]


def _zero_up(x):
    x = np.asarray(x, np.float64)
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]), np.float64)
    z[..., ::2, ::2] = x
    return z


def up(x):
    return _filter(_zero_up(x), 4.0 * G)


def down_bound(x):
    """|fp32 down(x) - down(x)| <= (25 + 1) u sum |g_k x_k|: 25 products summed in any order, each rounded once"""
    return 26 * U * down(np.abs(np.asarray(x, np.float64)))


def up_sub_bound(fine, coarse):
    """|fp32 (fine - up(coarse)) - exact| <= (10 + 1) u (sum |4 g_k z_k| + |fine|): at most 9 non-zero taps and the subtraction"""
    return 11 * U * (up(np.abs(np.asarray(coarse, np.float64))) + np.abs(np.asarray(fine, np.float64)))


def laplacian_pyramid(images):
    """[N, C, H, H] -> list of float64 levels, finest first"""
    pyr = [np.asarray(images, np.float64)]
    for _ in level_sides(pyr[0].shape[-1])[1:]:
        pyr.append(down(pyr[-1]))
        pyr[-2] = pyr[-2] - up(pyr[-1])
    return pyr


def descriptors(level, positions, P):
    """level [N, C, H, H], positions int [N * P, 2] = (y, x) centres -> [N * P, C, 7, 7]"""
    level = np.asarray(level, np.float64)
    pos = np.asarray(positions)
    H = level.shape[-1]
    assert pos.shape == (level.shape[0] * P, 2) and pos.min() >= 3 and pos.max() < H - 3
    img = np.arange(pos.shape[0]) // P
    off = np.arange(-3, 4)
    yy = pos[:, 0][:, None, None] + off[None, :, None]
    xx = pos[:, 1][:, None, None] + off[None, None, :]
    return level[img[:, None, None, None], np.arange(level.shape[1])[None, :, None, None], yy[:, None], xx[:, None]]


def stats(desc):
    """-> (mean [C], population std [C]) over descriptors and pixels"""
    return desc.mean(axis=(0, 2, 3)), desc.std(axis=(0, 2, 3))


def normalise(desc):
    mean, std = stats(desc)
    if not (np.all(np.isfinite(std)) and np.all(std > 0)):
        raise ValueError("a channel without variance")
    return (desc - mean[None, :, None, None]) / std[None, :, None, None]


def unit_columns(W):
    W = np.asarray(W, np.float64)
    return W / np.sqrt((W * W).sum(0, keepdims=True))


def project(desc, dirs, mean=None, std=None):
    """-> (projections [n_desc, D] of the normalised descriptors, bound [n_desc, D]): the projection as the device forms it,
    sum_k w'_k d_k - const with w' = w / std and const = sum_k w'_k mean_c(k); bound = (49 C + 4) u (sum |w'_k d_k| + |const|)"""
    if mean is None:
        mean, std = stats(desc)
    n, C = desc.shape[:2]
    flat = desc.reshape(n, C * 49)
    wp = np.asarray(dirs, np.float64) / np.repeat(std, 49)[:, None]
    const = (wp * np.repeat(mean, 49)[:, None]).sum(0)
    proj = flat @ wp - const[None, :]
    bound = (49 * C + 4) * U * (np.abs(flat) @ np.abs(wp) + np.abs(const)[None, :])
    return proj, bound


def sliced_distance(pa, pb):
    """projections [n, D] of the two sets -> mean |sorted columns of A - sorted columns of B|"""
    return float(np.abs(np.sort(pa, 0) - np.sort(pb, 0)).mean())


def swd_levels(levels_a, levels_b, positions, directions, P):
    """Laplacian levels of the two sets (finest first), positions[l] [N * P, 2], directions[l][r] [49 C, D] (unit columns)
    -> ({side: value * 1e3}, mean * 1e3, slack * 1e3): slack = the largest, over levels, of the sum of the two sets' largest projection
    bounds -- sorting and the mean absolute difference are 1-Lipschitz in the sup norm of the projections"""
    out, slack = {}, 0.0
    for la, lb, pos, dirs in zip(levels_a, levels_b, positions, directions):
        da, db = descriptors(la, pos, P), descriptors(lb, pos, P)
        for d in (da, db):
            normalise(d)                                  # raises on a channel without variance
        vals = []
        for W in dirs:
            (pa, ba), (pb, bb) = project(da, W), project(db, W)
            vals.append(sliced_distance(pa, pb))
            slack = max(slack, float(ba.max() + bb.max()))
        out[int(np.asarray(la).shape[-1])] = 1e3 * float(np.mean(vals))
    return out, float(np.mean(list(out.values()))), 1e3 * slack


def swd(A, B, positions, directions, P):
    """images [N, C, H, H] of the two sets -> {"levels": {side: value}, "mean": value}, times 1e3 as the paper reports them"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if A.shape != B.shape or A.ndim != 4 or A.shape[1] not in (1, 3) or A.shape[2] != A.shape[3]:
        raise ValueError("two image sets of one shape [N, C, H, H], C = 1 or 3")
    H = A.shape[-1]
    if H < MIN_SIDE or H & (H - 1):
        raise ValueError("H must be a power of two >= 16")
    levels, mean, _ = swd_levels(laplacian_pyramid(A), laplacian_pyramid(B), positions, directions, P)
    return {"levels": levels, "mean": mean}


def draw_plan(rng, shape, P, R, D):
    """positions and unit directions for image sets of ``shape`` from a numpy RandomState (host tests; the product draws its own)"""
    N, C, H, _ = shape
    positions = [rng.randint(3, s - 3, size=(N * P, 2)) for s in level_sides(H)]
    directions = [[unit_columns(rng.standard_normal((49 * C, D))) for _ in range(R)] for _ in level_sides(H)]
    return positions, directions

"""Cases, truths and yardsticks of the warp / code -> theta backward tests (tests/test_warp_grad_host.py, tests/test_gpu_warp_grad.py).

Method of tests/test_affine_refs_host.py (``H``): truth = the float64 torch reference under autograd (``R.warp``, ``R.MATRICES``), yardstick =
the same reference in float32 on the CPU, bound = ``H.bound(yardstick)`` (K = 8), metric = ``H.metric`` (element-wise for dimg, row-wise for
dtheta / dcode).

The kink.  grid_sample's derivative with respect to the sample coordinates jumps where a coordinate crosses an integer, and float32 and
float64 land on different sides of it: unmasked, the float32 dtheta of ``H.warp_inputs((5, 3, 64, 64))`` is 0.3 .. 0.95 of the row maximum
away from float64.  Every dtheta / dcode comparison therefore multiplies the upstream gradient (all channels) by ``~near``, near = a pixel
whose unclamped coordinate (from the float64 theta) lies within 1e-3 of an integer in x or y -- about 100 times the float32 coordinate
error at 64 pixels.  A row is compared only if its masked share is <= ``SHARE_CAP``; of ``H.warp_inputs`` exactly rows 0, 3, 4 (identity,
quarter turn, far shift: all coordinates integers) are left out, of the code-level cases none.  dimg is continuous: unmasked, all rows.
"""
import functools

import torch

import affine_refs as R
import test_affine_refs_host as H

NEAR = 1e-3
SHARE_CAP = 0.04
LEFT_OUT = (0, 3, 4)
MODES = ("border", "zeros")
OPS_SHAPES = ((5, 3, 64, 64), (6, 1, 32, 32), (7, 2, 24, 40), (130, 3, 16, 16))
BIG_SHAPE = (128, 3, 64, 64)
LIMIT_SHAPE = (2, 1, 128, 128)          # H * W = 16384, the largest plane eg_warp_affine_bwd takes
HOST_SHAPES = OPS_SHAPES + ((9, 3, 64, 64), BIG_SHAPE)
THETA_B = (1, 129)
# drop-in, end to end: name -> (module, matrix function of the module, kind of R.MATRICES, image shape)
E2E = {"celeba": ("celeba", "get_matrix", "rpqxy", (8, 3, 64, 64)), "mnist": ("mnist", "get_matrix", "rpqmnxy", (8, 1, 32, 32)),
       "dsprites": ("dsprites", "get_matrix", "rp", (8, 1, 64, 64)), "dsprites_pxy": ("dsprites", "get_matrix_pxy", "pxy", (8, 1, 64, 64))}
MUTANTS = ("no_border_zero", "swap_half_sizes", "first_channel")


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
def coordinates(th, Hh, W):
    """unclamped pixel coordinates (ix, iy) [B, H, W] of F.affine_grid(th, align_corners=False) un-normalised as grid_sample does"""
    xn = ((2 * torch.arange(W, dtype=th.dtype) + 1) / W - 1)[None, None, :]
    yn = ((2 * torch.arange(Hh, dtype=th.dtype) + 1) / Hh - 1)[None, :, None]
    t = lambda i, j: th[:, i, j, None, None]
    gx, gy = t(0, 0) * xn + t(0, 1) * yn + t(0, 2), t(1, 0) * xn + t(1, 1) * yn + t(1, 2)
    return ((gx + 1) * W - 1) / 2, ((gy + 1) * Hh - 1) / 2


def near_mask(th64, Hh, W):
    """-> (near [B, H, W] bool, share [B]): pixels within NEAR of the kink, and each row's share of them"""
    assert th64.dtype == torch.float64
    ix, iy = coordinates(th64, Hh, W)
    near = ((ix - ix.round()).abs() < NEAR) | ((iy - iy.round()).abs() < NEAR)
    return near, near.double().mean((1, 2))


# ---- warp level: img, theta of H.warp_inputs ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def warp_case(shape):
    """img, theta [B, 2, 3] (float32, of H.warp_inputs), the upstream gradient ``dout`` and its masked form, ``keep`` [B] bool, ``share``"""
    img, _, th = H.warp_inputs(shape)
    dout = torch.randn(shape, generator=H._gen("warpgrad", shape), dtype=torch.float64).float()
    near, share = near_mask(th.double(), shape[2], shape[3])
    return {"img": img, "theta": th, "dout": dout, "dout_masked": dout * (~near)[:, None].float(), "keep": share <= SHARE_CAP, "share": share}


def warp_grads(img, th, dout, mode):
    """autograd of R.warp in the dtype of the arguments -> (dimg, dtheta [B, 6])"""
    img, th = img.detach().clone().requires_grad_(True), th.detach().clone().requires_grad_(True)
    dimg, dth = torch.autograd.grad((R.warp(img, th, mode) * dout).sum(), (img, th))
    return dimg, dth.reshape(-1, 6)


@functools.lru_cache(maxsize=None)
def warp_truth(shape, mode):
    """float64: dimg of the unmasked upstream gradient, dtheta of the masked one, and dtheta of the unmasked one (row 4 is exactly 0)"""
    c = warp_case(shape)
    img, th = c["img"].double(), c["theta"].double()
    dimg, dth_raw = warp_grads(img, th, c["dout"].double(), mode)
    return {"dimg": dimg, "dtheta": warp_grads(img, th, c["dout_masked"].double(), mode)[1], "dtheta_unmasked": dth_raw}


@functools.lru_cache(maxsize=None)
def warp_yardstick(shape, mode):
    c, t = warp_case(shape), warp_truth(shape, mode)
    dimg = warp_grads(c["img"], c["theta"], c["dout"], mode)[0]
    dth = warp_grads(c["img"], c["theta"], c["dout_masked"], mode)[1]
    return {"dimg": H.metric(dimg, t["dimg"]), "dtheta": H.metric(dth, t["dtheta"], rows=True, keep=c["keep"])}


def manual_dtheta(img, th, dout, mode, mutant=None):
    """dtheta [B, 6] of the warp written out by hand (grid_sample's rules), float64 in -> float64 out; ``mutant``: a wrong variant --
    ``no_border_zero`` (the coordinate gradient is kept where 'border' clamps), ``swap_half_sizes`` (W / 2 and H / 2 exchanged),
    ``first_channel`` (the sum over channels takes channel 0 only)"""
    B, C, Hh, W = img.shape
    ix, iy = coordinates(th, Hh, W)
    mx, my = torch.ones_like(ix), torch.ones_like(iy)
    if mode == "border":
        if mutant != "no_border_zero":
            mx, my = ((ix > 0) & (ix < W - 1)).to(ix.dtype), ((iy > 0) & (iy < Hh - 1)).to(iy.dtype)
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, Hh - 1)
    x0, y0 = ix.floor(), iy.floor()
    wx1, wy1 = (ix - x0)[:, None], (iy - y0)[:, None]
    wx0, wy0 = 1 - wx1, 1 - wy1

    def tap(x, y):
        inside = ((x >= 0) & (x < W) & (y >= 0) & (y < Hh))[:, None]
        idx = (y.clamp(0, Hh - 1) * W + x.clamp(0, W - 1)).long().view(B, 1, -1).expand(B, C, -1)
        return img.reshape(B, C, -1).gather(2, idx).view(B, C, Hh, W) * inside
    v00, v01, v10, v11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    gx = dout * ((v01 - v00) * wy0 + (v11 - v10) * wy1)
    gy = dout * ((v10 - v00) * wx0 + (v11 - v01) * wx1)
    if mutant == "first_channel":
        gx, gy = gx[:, :1], gy[:, :1]
    sx, sy = (Hh / 2, W / 2) if mutant == "swap_half_sizes" else (W / 2, Hh / 2)
    gx, gy = gx.sum(1) * mx * sx, gy.sum(1) * my * sy
    xn = ((2 * torch.arange(W, dtype=th.dtype) + 1) / W - 1)[None, None, :]
    yn = ((2 * torch.arange(Hh, dtype=th.dtype) + 1) / Hh - 1)[None, :, None]
    return torch.stack([(gx * xn).sum((1, 2)), (gx * yn).sum((1, 2)), gx.sum((1, 2)), (gy * xn).sum((1, 2)), (gy * yn).sum((1, 2)), gy.sum((1, 2))], 1)


# ---- code -> theta ----------------------------------------------------------------------------------------------------------------------
def _theta_of(kind, c):
    return R.theta(R.MATRICES[kind][0](c)).reshape(c.shape[0], 6)


@functools.lru_cache(maxsize=None)
def theta_case(kind, B):
    """codes [B, 9] of H.matrix_inputs (the kind's codes from column 1) and the upstream gradient dtheta [B, 6]"""
    return H.matrix_inputs(kind, B), torch.randn(B, 6, generator=H._gen("thetagrad", kind, B), dtype=torch.float64).float()


def theta_grads(kind, codes, dtheta):
    n = R.MATRICES[kind][1]
    c = codes[:, 1:1 + n].detach().clone().requires_grad_(True)
    return torch.autograd.grad((_theta_of(kind, c) * dtheta).sum(), c)[0]


@functools.lru_cache(maxsize=None)
def theta_truth(kind, B):
    codes, dth = theta_case(kind, B)
    return theta_grads(kind, codes.double(), dth.double())


@functools.lru_cache(maxsize=None)
def theta_yardstick(kind, B):
    codes, dth = theta_case(kind, B)
    return H.metric(theta_grads(kind, codes, dth), theta_truth(kind, B), rows=True)


# ---- drop-in, end to end: codes -> matrix -> warp ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_case(name):
    """img in [0, 1], codes [8, 9] in [-1, 1] (the kind's codes in columns 1 .. 1 + n), the weights ``w`` of the scalar (out * w).sum() and
    their masked form (mask from the float64 theta of the codes), ``share`` [8]"""
    _, _, kind, shape = E2E[name]
    g = H._gen("warpgrad-e2e", kind)
    img = torch.rand(shape, generator=g, dtype=torch.float64).float()
    code = H._uniform(g, (shape[0], 9), 1.0)
    w = torch.randn(shape, generator=g, dtype=torch.float64).float()
    n = R.MATRICES[kind][1]
    near, share = near_mask(R.theta(R.MATRICES[kind][0](code[:, 1:1 + n].double())), shape[2], shape[3])
    return {"img": img, "code": code, "w": w, "w_masked": w * (~near)[:, None].float(), "share": share, "n": n, "kind": kind}


def e2e_grads(name, cast):
    """autograd of R.warp(img, R.theta(matrix(code))) in the dtype ``cast`` gives -> {"dimg" (w unmasked), "dcode" [8, 9] (w masked)}"""
    c = e2e_case(name)
    out = {}
    for key, w in (("dimg", c["w"]), ("dcode", c["w_masked"])):
        img, code = cast(c["img"]).requires_grad_(True), cast(c["code"]).requires_grad_(True)
        th = R.theta(R.MATRICES[c["kind"]][0](code[:, 1:1 + c["n"]]))
        dimg, dcode = torch.autograd.grad((R.warp(img, th, "border") * cast(w)).sum(), (img, code))
        out[key] = dimg if key == "dimg" else dcode
    return out


@functools.lru_cache(maxsize=None)
def e2e_truth(name):
    return e2e_grads(name, lambda t: t.double().clone())


@functools.lru_cache(maxsize=None)
def e2e_yardstick(name):
    own, t, n = e2e_grads(name, lambda t: t.clone()), e2e_truth(name), e2e_case(name)["n"]
    return {"dimg": H.metric(own["dimg"], t["dimg"]), "dcode": H.metric(own["dcode"][:, 1:1 + n], t["dcode"][:, 1:1 + n], rows=True)}

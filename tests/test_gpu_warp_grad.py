"""``eg_warp_affine_bwd`` and ``eg_theta_bwd`` through ``ops``, and the differentiable drop-in functions built on them
(``transformation_2D``, ``get_matrix`` / ``get_matrix_D`` / ``get_matrix_pxy`` / ``get_matrix_pxy_align``), against float64 autograd of the
references of tests/affine_refs.py.

Method of tests/test_gpu_affine_losses.py: bound = ``H.bound(yardstick)`` = max(8 * yardstick, 4 float32 ulps), yardstick = the same
reference in float32 on the CPU; dimg element by element with the unmasked upstream gradient, dtheta / dcode row by row with the upstream
gradient masked at the kink and the all-integer rows 0, 3, 4 of ``H.warp_inputs`` left out (tests/warp_grad_cases.py, whose host tests
show the mask's shares, the yardsticks' size and that the mutants of the backward miss these bounds by a factor of 10 at least).
Every comparison prints ``error / yardstick`` (run with -s).

Largest error / max(yardstick, floor / K) observed on an MI355X (K = 8 allows 8):
  ops.warp_affine_bwd   border: dimg 1.1, dtheta 1.4   zeros: dimg 1.0, dtheta 2.0   (all shapes, H * W = 16384 included)
  ops.theta_bwd         rpqxy 1.1   rpqmnxy 0.9   rp 1.9 at B = 1   pxy 2.1 at B = 1   pxy_align_inv 1.0
  drop-in, end to end   img.grad: celeba 0.9, mnist 1.0, dsprites 0.5, dsprites pxy 0.6   code.grad: celeba 1.5, mnist 2.3, dsprites 1.9, dsprites pxy 0.6
  transformation_2D(padding_mode="zeros") img.grad 0.9; matrix-only code.grad 0.6
Nothing needed more than K = 8; as there, the largest ratios of theta_bwd belong to one-row cases.
"""
import importlib

import pytest
import torch

import affine_refs as R
import test_affine_refs_host as H
import warp_grad_cases as WG

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 7.0
eg = None
ops = None


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops


def np32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def check(name, got, want, yard, rows=False, keep=None):
    fig = H.metric(got, want, rows, keep)
    print(f"{name}: error {fig:.3g}  yardstick {yard:.3g}  error / max(yardstick, floor / K) {fig / max(yard, H.FLOOR / H.K):.3g}  bound {H.bound(yard):.3g}")
    assert fig <= H.bound(yard), (name, fig, yard, H.bound(yard))


# ---- ops.warp_affine_bwd ------------------------------------------------------------------------------------------------------------------
def run_bwd(c, dout, shape, zeros, dimg=True, dtheta=True):
    B, C, Hh, W = shape
    di = torch.full(shape, SENTINEL, device=DEV) if dimg else None
    dt = torch.full((B, 6), SENTINEL, device=DEV) if dtheta else None
    ops.warp_affine_bwd(c["img"].to(DEV), c["theta"].to(DEV), dout.to(DEV), di, dt, B, C, Hh, W, zeros=zeros)
    torch.cuda.synchronize()
    return di, dt


@pytest.mark.parametrize("mode", WG.MODES)
@pytest.mark.parametrize("shape", WG.OPS_SHAPES + (WG.BIG_SHAPE,))
def test_warp_affine_bwd(shape, mode):
    """dimg (unmasked upstream gradient, all rows) and dtheta (masked, kept rows) against float64; every element written over the sentinel;
    dtheta of the far shift exactly 0; two calls give the same dtheta bits; a null dimg or dtheta leaves the other output unchanged."""
    c, truth, yard = WG.warp_case(shape), WG.warp_truth(shape, mode), WG.warp_yardstick(shape, mode)
    zeros = mode == "zeros"
    tag = f"warp_affine_bwd {mode} {shape}"
    dimg, dth_raw = run_bwd(c, c["dout"], shape, zeros)
    check(tag + " dimg", dimg, truth["dimg"], yard["dimg"])
    # (dimg is compared element by element over all rows: an element that kept the sentinel fails that comparison)
    assert not bool((dth_raw == SENTINEL).any()), tag + ": dtheta keeps the sentinel"
    assert bool((dth_raw[4] == 0).all()), (tag, dth_raw[4])              # the far shift: every sample clamped ('border') or outside ('zeros')
    _, dth = run_bwd(c, c["dout_masked"], shape, zeros, dimg=False)
    check(tag + " dtheta", dth, truth["dtheta"], yard["dtheta"], rows=True, keep=c["keep"])
    if shape == WG.BIG_SHAPE:
        return
    dimg2, dth_raw2 = run_bwd(c, c["dout"], shape, zeros)
    assert torch.equal(dth_raw, dth_raw2), tag + ": dtheta differs between two calls"
    check(tag + " dimg again", dimg2, truth["dimg"], yard["dimg"])
    _, dth_only = run_bwd(c, c["dout"], shape, zeros, dimg=False)
    assert torch.equal(dth_only, dth_raw), tag + ": dtheta depends on dimg being asked for"
    dimg_only, _ = run_bwd(c, c["dout"], shape, zeros, dtheta=False)
    check(tag + " dimg alone", dimg_only, truth["dimg"], yard["dimg"])


@pytest.mark.parametrize("mode", WG.MODES)
def test_warp_affine_bwd_at_the_largest_plane(mode):
    """H * W = 16384, the limit: 64 KiB of LDS a workgroup.  Rows: the identity (left out of dtheta) and the zoom-out with a shift."""
    shape = WG.LIMIT_SHAPE
    c, truth, yard = WG.warp_case(shape), WG.warp_truth(shape, mode), WG.warp_yardstick(shape, mode)
    assert c["keep"].tolist() == [False, True]
    dimg, _ = run_bwd(c, c["dout"], shape, mode == "zeros")
    check(f"warp_affine_bwd {mode} {shape} dimg", dimg, truth["dimg"], yard["dimg"])
    _, dth = run_bwd(c, c["dout_masked"], shape, mode == "zeros", dimg=False)
    check(f"warp_affine_bwd {mode} {shape} dtheta", dth, truth["dtheta"], yard["dtheta"], rows=True, keep=c["keep"])


def test_warp_affine_bwd_refuses_a_plane_above_16384_pixels():
    B, C, Hh, W = 1, 1, 128, 256
    z = torch.zeros(B, C, Hh, W, device=DEV)
    th = torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]], device=DEV)
    dimg, dth = torch.full_like(z, SENTINEL), torch.full((B, 6), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="16384"):
        ops.warp_affine_bwd(z, th, z, dimg, dth, B, C, Hh, W)
    ops.clear_errors()
    torch.cuda.synchronize()
    assert bool((dimg == SENTINEL).all()) and bool((dth == SENTINEL).all())            # nothing was launched


# ---- ops.theta_bwd --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", WG.THETA_B)
@pytest.mark.parametrize("kind", list(R.MATRICES))
def test_theta_bwd(kind, B):
    """codes from column 1 of 9-wide rows (the kernel sees the row stride 9 and its first code at the pointer): the kind's n columns against
    float64 autograd of R.MATRICES[kind], the other columns of every row exactly 0 over the sentinel, nothing written before the pointer"""
    n = R.MATRICES[kind][1]
    codes, dth = WG.theta_case(kind, B)
    flat = torch.cat((codes.reshape(-1), torch.zeros(1))).to(DEV)         # one float past the last row: the rows the kernel sees end there
    dflat = torch.full((B * 9 + 1,), SENTINEL, device=DEV)
    ops.theta_bwd(ops.THETA_KINDS[kind], flat[1:], 9, B, dth.to(DEV), dflat[1:])
    torch.cuda.synchronize()
    rows = dflat[1:].view(B, 9)
    check(f"theta_bwd {kind} B={B}", rows[:, :n], WG.theta_truth(kind, B), WG.theta_yardstick(kind, B), rows=True)
    assert bool((rows[:, n:] == 0).all()), "columns outside the codes are not cleared"
    assert float(dflat[0]) == SENTINEL


def test_theta_bwd_refuses_bad_arguments():
    c = torch.zeros(4, 9, device=DEV)
    with pytest.raises(RuntimeError, match="kind"):
        ops.theta_bwd(5, c, 9, 4, torch.zeros(4, 6, device=DEV), torch.zeros(4, 9, device=DEV))
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.theta_bwd(ops.THETA_KINDS["rpqmnxy"], c, 6, 4, torch.zeros(4, 6, device=DEV), torch.zeros(4, 9, device=DEV))
    ops.clear_errors()


# ---- the drop-in functions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WG.E2E))
def test_dropin_warp_of_a_code_matrix_end_to_end(name):
    """A = get_matrix(code); out = transformation_2D()(img, A[:, 0:2]); (out * w).sum().backward() with code and img requiring grad:
    img.grad (w unmasked) and code.grad (w masked at the kink) against float64 autograd of R.warp(img, R.theta(matrix(code)))"""
    module, fn, kind, shape = WG.E2E[name]
    c, truth, yard = WG.e2e_case(name), WG.e2e_truth(name), WG.e2e_yardstick(name)
    n = c["n"]
    get_matrix = getattr(getattr(eg, module), fn)
    trans_2D = getattr(eg, module).transformation_2D()
    grads = {}
    for key, w in (("dimg", c["w"]), ("dcode", c["w_masked"])):
        img, code = c["img"].to(DEV).requires_grad_(True), c["code"].to(DEV).requires_grad_(True)
        A = get_matrix(code[:, 1:1 + n])
        out = trans_2D(img, A[:, 0:2])
        assert out.grad_fn is not None and A.requires_grad
        (out * w.to(DEV)).sum().backward()
        grads[key] = img.grad if key == "dimg" else code.grad
    assert bool((c["share"] <= WG.SHARE_CAP).all())                       # no row is left out
    check(f"drop-in {name} img.grad", grads["dimg"], truth["dimg"], yard["dimg"])
    check(f"drop-in {name} code.grad", grads["dcode"][:, 1:1 + n], truth["dcode"][:, 1:1 + n], yard["dcode"], rows=True)
    outside = torch.cat((grads["dcode"][:, :1], grads["dcode"][:, 1 + n:]), 1)
    assert bool((outside == 0).all())


def test_get_matrix_pxy_align_under_autograd():
    """A = T(.1 c1, .1 c2): (A * w).sum().backward() gives code.grad = (0, .1 w[0, 2], .1 w[1, 2]); the in-place sign flip of the kernel's
    inverse is followed by autograd.  The values are those of the direct call."""
    B = 33
    g = H._gen("pxy-align-grad")
    code, w = H._uniform(g, (B, 3), 1.0), torch.randn(B, 3, 3, generator=g)
    c = code.to(DEV).requires_grad_(True)
    A = eg.dsprites.get_matrix_pxy_align(c)
    (A * w.to(DEV)).sum().backward()
    want = torch.stack((torch.zeros(B), w[:, 0, 2] * np32(0.1), w[:, 1, 2] * np32(0.1)), 1)
    assert torch.equal(c.grad.cpu(), want), (c.grad[:3], want[:3])
    plain = eg.dsprites.get_matrix_pxy_align(code.to(DEV))
    assert not plain.requires_grad and torch.equal(plain, A.detach())
    assert torch.equal(plain[:, 0, 2].cpu(), code[:, 1] * np32(0.1)) and torch.equal(plain[:, 1, 2].cpu(), code[:, 2] * np32(0.1))


def test_transformation_2D_zeros_is_the_zeros_kernel_and_differentiable():
    shape = (7, 2, 24, 40)
    B, C, Hh, W = shape
    c, truth, yard = WG.warp_case(shape), WG.warp_truth(shape, "zeros"), WG.warp_yardstick(shape, "zeros")
    img, th = c["img"].to(DEV), c["theta"].to(DEV)
    want = torch.empty(shape, device=DEV)
    ops.warp_affine_zeros(img, th, want, B, C, Hh, W)
    mod = eg.colored.transformation_2D(padding_mode="zeros")
    got = mod(img, th)
    assert torch.equal(got, want) and not got.requires_grad
    img_g = img.clone().requires_grad_(True)
    out = mod(img_g, th)
    assert torch.equal(out.detach(), want)
    (out * c["dout"].to(DEV)).sum().backward()
    check("transformation_2D zeros img.grad", img_g.grad, truth["dimg"], yard["dimg"])


def test_nothing_changes_without_requires_grad():
    """outputs are bit-equal to the direct ops calls and carry no grad; the matrix arrives as the non-contiguous A[:, 0:2]"""
    shape = (6, 1, 32, 32)
    B, C, Hh, W = shape
    img, code, _ = H.warp_inputs(shape)
    img, code = img.to(DEV), code.to(DEV)
    for module, fn, kind, n in (("celeba", "get_matrix", "rpqxy", 5), ("mnist", "get_matrix", "rpqmnxy", 7), ("dsprites", "get_matrix", "rp", 4),
                                ("dsprites", "get_matrix_D", "rp", 4), ("dsprites", "get_matrix_pxy", "pxy", 3)):
        A = getattr(getattr(eg, module), fn)(code[:, :n])
        th = torch.empty(B, 2, 3, device=DEV)
        cc = code[:, :n].contiguous()
        getattr(ops, "theta_" + kind)(cc, n, B, th)
        assert not A.requires_grad and A.grad_fn is None
        assert torch.equal(A[:, :2], th) and torch.equal(A[:, 2], torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(B, 3)), (module, fn)
        out = getattr(eg, module).transformation_2D()(img, A[:, 0:2])
        want = torch.empty(shape, device=DEV)
        ops.warp_affine(img, th, want, B, C, Hh, W)
        assert not out.requires_grad and out.grad_fn is None and torch.equal(out, want), (module, fn)
    with torch.no_grad():
        out = eg.celeba.transformation_2D()(img.clone().requires_grad_(True), eg.celeba.get_matrix(code)[:, 0:2])
    assert not out.requires_grad


def test_only_the_matrix_requires_grad():
    """learning the alignment: the image is data, the matrix carries the gradient (dimg is then not computed at all)"""
    name = "dsprites_pxy"
    c, truth, yard = WG.e2e_case(name), WG.e2e_truth(name), WG.e2e_yardstick(name)
    n = c["n"]
    code = c["code"].to(DEV).requires_grad_(True)
    out = eg.dsprites.transformation_2D()(c["img"].to(DEV), eg.dsprites.get_matrix_pxy(code[:, 1:1 + n])[:, 0:2])
    (out * c["w_masked"].to(DEV)).sum().backward()
    check("matrix-only code.grad", code.grad[:, 1:1 + n], truth["dcode"][:, 1:1 + n], yard["dcode"], rows=True)

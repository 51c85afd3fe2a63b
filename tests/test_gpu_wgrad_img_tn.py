"""Weight gradient of the CelebA image-side layers straight from the fp32 images (eg_wgrad_img_tn, csrc/wgrad_img_tn.hip) against the pair it
replaces, eg_im2col_img + eg_conv_wgrad over the patch rows (celebA/EAD-GAN_celebA.py:110, 90-91): one workgroup per K split of the per-tap
kernel's plan, the same operands in the same MFMA slots in the same order -> the slabs are bit-identical.

Reference at a forced split count (wgs_target > 0): eg_conv_wgrad's per-tap launches take no target, so the slab of split i is the per-tap
kernel's over the patch rows of that split alone -- a launch of fewer than 512 rows is ONE split, rows in ascending 32-row steps like any
split of a longer launch.  At wgs_target = 0 the reference is the whole launch."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from layer_refs import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, N, B = 64, 128, 2
RING = 7                      # EG_TNI_RING: stages of the kernel's LDS ring
eg = None
ops = None


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops


def _inputs(dtype, T, C, seed=3, batch=B):
    g = torch.Generator().manual_seed(seed)
    imgs = [(torch.rand(batch, C, S, S, generator=g) * 2 - 1).to(DEV) for _ in range(T)]
    P = (torch.randn(T * batch * 1024, N, generator=g) * 0.5).to(DEV).to(ops.torch_dtype(dtype))
    return imgs, P


def _patches(dtype, imgs, C, batch=B):
    npix = batch * 1024
    out = torch.empty(len(imgs) * npix, 16 * C, device=DEV, dtype=ops.torch_dtype(dtype))
    for t, im in enumerate(imgs):
        ops.im2col_img(dtype, im, out[t * npix:(t + 1) * npix], batch, C, S, S, 4, 2, 1, 16 * C)
    return out


def _reference(dtype, imgs, P, C, target, batch=B):
    """the slabs of eg_im2col_img + eg_conv_wgrad at the new op's split plan -> (slab [ns][128][16 C], rows per split)"""
    T, M, kc = len(imgs), len(imgs) * batch * 1024, 16 * C
    patches = _patches(dtype, imgs, C, batch)
    ns, rps = ops.wgrad_img_tn_plan(T * batch, C, target)
    slab = torch.full((ns, N, kc), float("nan"), device=DEV)
    if target == 0:
        got = ops.conv_wgrad(ops.make_conv(T * batch, 32, 32, kc, N, 1, 1, 0), dtype, patches, P, slab, 0)
        assert got == ns, (got, ns)
        return slab, rps
    assert rps < 512, rps                                   # one split per reference launch
    for i in range(ns):
        lo, hi = i * rps, min(M, (i + 1) * rps)
        got = ops.conv_wgrad(ops.make_conv((hi - lo) // 32, 1, 32, kc, N, 1, 1, 0), dtype, patches[lo:hi], P[lo:hi], slab[i], 0)
        assert got == 1, got
    return slab, rps


def _run(dtype, imgs, P, C, target, batch=B):
    ns, _ = ops.wgrad_img_tn_plan(len(imgs) * batch, C, target)
    slab = torch.full((ns, N, 16 * C), float("nan"), device=DEV)
    assert ops.wgrad_img_tn(dtype, imgs, P, slab, batch, C, S, S, N, target) == ns
    return slab


def _target_for(images, C, steps):
    """a wgs_target whose plan has `steps` 32-row steps per split"""
    for target in range(images * 32, 0, -1):
        if ops.wgrad_img_tn_plan(images, C, target)[1] == 32 * steps:
            return target
    raise AssertionError((images, C, steps))


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("C", [1, 3])
def test_default_plan_is_the_per_tap_launch_bit_for_bit(C, T, dtype):
    assert ops.wgrad_img_tn_ok(dtype, C, S, S, N, 4, 2, 1)
    imgs, P = _inputs(dtype, T, C)
    want, rps = _reference(dtype, imgs, P, C, 0)
    got = _run(dtype, imgs, P, C, 0)
    torch.cuda.synchronize()
    assert rps == 256 and want.shape[0] == 8 * T            # the per-tap plan at B = 2: splits of 8 steps, four per image
    assert torch.equal(got, want)


# (steps per split, tapes): one and two steps, the ring depth - 1 / depth / + 1; with two tapes of 64 steps each, 6-step splits
# straddle the tape boundary and leave a ragged last split
@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("C,T,steps", [(3, 1, 1), (3, 1, 2), (3, 2, RING - 1), (3, 2, RING), (3, 2, RING + 1), (1, 3, RING), (1, 1, 1)])
def test_forced_split_lengths_bit_for_bit(C, T, steps, dtype):
    target = _target_for(T * B, C, steps)
    imgs, P = _inputs(dtype, T, C, seed=11)
    want, rps = _reference(dtype, imgs, P, C, target)
    M = T * B * 1024
    assert rps == 32 * steps and want.shape[0] == -(-M // rps)
    assert rps % 1024 != 0                                   # split boundaries inside an image
    if steps == RING - 1:
        assert (B * 1024) % rps != 0 and T > 1               # a split across the tape boundary
        assert M % rps != 0                                  # a ragged last split
    got = _run(dtype, imgs, P, C, target)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_split_count_of_the_trainers_lanes():
    """the trainer's launches (B = 128, one to three tapes) plan 128 splits; the same count at B = 2"""
    for T in (1, 2, 3):
        assert ops.wgrad_img_tn_plan(T * 128, 3, 0)[0] == 128
    imgs, P = _inputs(1, 2, 3, seed=13)
    want, rps = _reference(1, imgs, P, 3, 128)
    assert want.shape[0] == 128 and rps == 32
    got = _run(1, imgs, P, 3, 128)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("edge", ["row0", "row63", "col0", "col63", "oy0", "oy31"])
def test_edges(edge, dtype):
    """images whose only non-zero pixels are one border row / column; P non-zero only in the first / last output row"""
    C, T = 3, 1
    imgs, P = _inputs(dtype, T, C, seed=17)
    keep = torch.zeros_like(imgs[0])
    if edge == "row0":
        keep[:, :, 0, :] = 1
    elif edge == "row63":
        keep[:, :, 63, :] = 1
    elif edge == "col0":
        keep[:, :, :, 0] = 1
    elif edge == "col63":
        keep[:, :, :, 63] = 1
    else:
        keep[:] = 1
        pk = torch.zeros(B, 32, 32, 1, device=DEV, dtype=P.dtype)
        pk[:, 0 if edge == "oy0" else 31] = 1
        P = (P.view(B, 32, 32, N) * pk).reshape(-1, N).contiguous()
    imgs = [imgs[0] * keep]
    for target in (0, _target_for(B, C, 1)):
        want, _ = _reference(dtype, imgs, P, C, target)
        got = _run(dtype, imgs, P, C, target)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert float(want.abs().sum()) > 0
    # the taps that can see the border: row 0 is read by ky >= 1 only, row 63 by ky <= 2 (columns alike)
    s = got.sum(0).view(N, C, 4, 4).abs().sum((0, 1))
    if edge == "row0":
        assert float(s[0].sum()) == 0 and float(s[1].sum()) > 0
    if edge == "row63":
        assert float(s[3].sum()) == 0 and float(s[2].sum()) > 0
    if edge == "col0":
        assert float(s[:, 0].sum()) == 0 and float(s[:, 1].sum()) > 0
    if edge == "col63":
        assert float(s[:, 3].sum()) == 0 and float(s[:, 2].sum()) > 0


@pytest.mark.parametrize("target_steps", [0, 2, RING + 1])
def test_second_launch_in_the_same_buffers_sees_no_stale_stage(target_steps):
    dtype, C, T = 1, 3, 2
    target = _target_for(T * B, C, target_steps) if target_steps else 0
    a_imgs, a_P = _inputs(dtype, T, C, seed=19)
    b_imgs, b_P = _inputs(dtype, T, C, seed=23)
    want_b, _ = _reference(dtype, b_imgs, b_P, C, target)
    imgs, P = [t.clone() for t in a_imgs], a_P.clone()
    ns = want_b.shape[0]
    slab = torch.empty(ns, N, 16 * C, device=DEV)
    ops.wgrad_img_tn(dtype, imgs, P, slab, B, C, S, S, N, target)
    for dst, src in zip(imgs, b_imgs):
        dst.copy_(src)
    P.copy_(b_P)
    ops.wgrad_img_tn(dtype, imgs, P, slab, B, C, S, S, N, target)
    torch.cuda.synchronize()
    assert torch.equal(slab, want_b)


def test_against_float64():
    """unfold + matmul in float64 on the rounded operands; 2e-3: the bound of test_celeba_b128_bf16_layerwise_kernels for the per-tap weight
    gradient, whose bits these are"""
    dtype, C, T = 1, 3, 2
    imgs, P = _inputs(dtype, T, C, seed=29)
    got = _run(dtype, imgs, P, C, 0)
    grad = torch.zeros(N * 16 * C, device=DEV)
    ops.wgrad_reduce(got, got.shape[0], N, N, 16 * C, 1, grad, accumulate=False)
    tdt = ops.torch_dtype(dtype)
    x = torch.cat(imgs).to(tdt).double()
    cols = F.unfold(x, 4, padding=1, stride=2)              # [T B][C 16][1024]
    ref = torch.einsum("bmn,bkm->nk", P.double().view(T * B, 1024, N), cols)
    e = _rel(grad.view(N, 16 * C), ref)
    print("wgrad_img_tn vs float64: relative L2 error", e)
    assert e < 2e-3, e


def test_fp32_and_other_shapes_keep_patch_rows():
    assert not ops.wgrad_img_tn_ok(0, 3, 64, 64, 128, 4, 2, 1)           # fp32
    assert not ops.wgrad_img_tn_ok(1, 3, 32, 32, 128, 4, 2, 1)           # 32 x 32 images
    assert not ops.wgrad_img_tn_ok(1, 3, 64, 64, 64, 4, 2, 1)            # 64 output channels (the dSprites layers: eg_wgrad_img)
    assert not ops.wgrad_img_tn_ok(1, 5, 64, 64, 128, 4, 2, 1)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def _train(monkeypatch, direct, capture, record=None):
    from oracle import celeba_oracle as co
    TB = 8
    with monkeypatch.context() as mp:
        mp.setattr(eg.engine, "WGRAD_IMG_TN", direct)
        orc = co.CelebAOracle(seed=21)
        G, D = eg.celeba.Generator(dtype="bf16").to(DEV), eg.celeba.Discriminator(dtype="bf16").to(DEV)
        G.load_state_dict({k: v.detach() for k, v in orc.G.items()})
        D.load_state_dict({k: v.detach() for k, v in orc.D.items()})
        tr = eg.celeba.CelebATrainer(G, D, TB, dtype="bf16")
        assert tr.ge.wgrad_tn == direct and tr.de.wgrad_tn == direct
        assert (tr.ge.patches is None) == direct and (tr.de.patches is None) == direct
        if record is not None:
            lib = eg._lib.lib()
            call = lib.call
            mp.setattr(lib, "call", lambda name, *a: (record.append(name), call(name, *a))[1])
        rng = np.random.RandomState(4)
        real = co.synthetic_real(TB, seed=9).to(DEV)
        out = []
        for i in range(2):
            z, code, labels = co.draw_step_inputs(rng, TB)
            tr.load_inputs(real, z.to(DEV), code.to(DEV), labels.to(DEV))
            if capture and i == 1:
                tr.capture()
            out.append(tr.step_resident().clone())
        torch.cuda.synchronize()
        state = [G.arena.flat, D.arena.flat, G.arena.grad, D.arena.grad, tr.mG, tr.vG, tr.mD, tr.vD, tr.miG, tr.viG, tr.miD, tr.viD, tr.steps]
        return [torch.stack(out)] + [t.clone() for t in state]


def test_trainer_iteration_is_bit_identical_with_and_without_patch_rows(monkeypatch):
    """losses, parameters, moments and gradient arenas after eager iterations with the layer-0 / last-layer weight gradients read from the
    images and from patch rows; a captured replay equals the eager iteration; no im2col launch is left on the 16-bit path"""
    names = []
    new = _train(monkeypatch, True, False, record=names)
    assert "eg_wgrad_img_tn" in names and "eg_im2col_img" not in names, sorted(set(names))
    old_names = []
    old = _train(monkeypatch, False, False, record=old_names)
    assert "eg_im2col_img" in old_names and "eg_wgrad_img_tn" not in old_names
    for a, b in zip(new, old):
        assert torch.equal(a, b)
    replay = _train(monkeypatch, True, True)
    for a, b in zip(new, replay):
        assert torch.equal(a, b)

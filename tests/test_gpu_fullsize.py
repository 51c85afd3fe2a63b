"""One iteration of every BASELINE.json configuration at its FULL batch size against the CPU oracle, learning rates 0 on both sides
(losses and the gradients the last sub-step leaves behind; BatchNorm statistics and spectral-norm vectors still advance).  The
small-batch parity tests never reach the kernels these sizes are dispatched to -- the 8-wave 256 x 128 kernel, the 128 x 128
buffer-descriptor kernel with and without a K split, the split planners of the weight-gradient GEMMs -- so each test also asserts,
through the planner's own query, that its launches are the production variants.

  CelebA 64x64     B = 128  bf16   celebA/EAD-GAN_celebA.py:297-401
  MNIST 32x32      B = 256  fp32   MNIST/EAD-GAN_rpqmnxy.py:338-446
  dSprites 64x64   B = 128  bf16   dSprites/rp.py:363-482
  colored dSprites B = 512  fp16   colored_dSprites/rp_color.py:363-516

Tolerances.  fp32 (exact-fp32 MFMA): losses 1e-4, whole-network gradients 2e-2 in relative L2 (LeakyReLU units within rounding of 0
take the other branch: DESIGN.md section 2; measured 1e-3 .. 3e-3 at these sizes).  16-bit modes compute with bf16 / fp16 MFMA operands
and fp32 accumulation against the fp32 oracle: losses 3e-2 relative; gradients 0.25 (generator: its gradient is d(img) pushed through
four 16-bit discriminator layers and four generator layers) and 0.1 (discriminator / encoder) -- the 16-bit rounding itself, not the
batch size or the kernel variant: B = 8 measures the same 0.15 / 0.05 as B = 128 (profiles/scripts/diag_fullsize_grad_error.py), and
the CelebA configuration is therefore also run in fp32 at full size, where the same planner choices must meet the tight bound."""
import importlib

import pytest
import torch

import test_gpu_celeba as tce
import test_gpu_colored as tco
import test_gpu_dsprites as tds
import test_gpu_mnist as tmn
from layer_refs import _conv_ref, _convT_ref, _rel

pytestmark = pytest.mark.gpu
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")
    for m in (tce, tco, tds, tmn):
        m.setup_module(m)


def arena_rel_err(mod, ref, skip=()):
    """relative L2 error of the module's whole gradient vs the oracle's (parameters in `skip` left out on both sides)"""
    num = den = 0.0
    for k, p in mod.named_parameters():
        if k in skip or ref[k].grad is None or k.startswith("noise_layer"):
            continue
        a, b = p.grad.detach().float().cpu().flatten(), ref[k].grad.detach().float().flatten()
        num += float(((a - b) ** 2).sum())
        den += float((b ** 2).sum())
    return (num / max(den, 1e-60)) ** 0.5


def nt_labels(convs, dtype):
    """planner labels (kernel code = label % 1000) of a list of (eg_conv, bwd) launches"""
    return {eg.ops.nt_tile_hinted(c, dtype, bwd) % 1000 for c, bwd in convs}


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_celeba_b128(dtype):
    B = 128
    orc, G, D, tr, got, want = tce.run_steps(dtype, B, 1, seed=2, lrs=(0.0, 0.0, 0.0))
    for k in ("g_loss", "d_loss", "info_loss"):
        tol = 1e-4 if dtype == "f32" else 3e-2 * max(1.0, abs(want[0][k]))
        assert abs(got[0][k] - want[0][k]) < tol, (k, got[0][k], want[0][k])
    eg_, ed = arena_rel_err(G, orc.G, tce.PRE_BN_BIAS), arena_rel_err(D, orc.D)
    assert (eg_ < 2e-2 and ed < 2e-2) if dtype == "f32" else (eg_ < 0.25 and ed < 0.1), (eg_, ed)
    for k, v in list(G.state_dict().items()) + list(D.state_dict().items()):
        if k.endswith(("running_mean", "running_var", "weight_u", "weight_v")):
            ref = orc.G[k] if k in orc.G else orc.D[k]
            assert tce.rel_err(v, ref) < (1e-4 if dtype == "f32" else 3e-2), k
    # production dispatch: discriminator convolutions at one, two and three tapes (forward and backward-data) and the generator's
    # transposed convolutions (backward-data kernels forward, forward kernels backward)
    ops, dt = eg.ops, (eg.ops.EG_BF16 if dtype == "bf16" else eg.ops.EG_F32)
    Wd, Wg = (128, 256, 512, 1024), (1024, 512, 256, 128)
    launches = []
    for T in (1, 2, 3):
        for i in range(3):
            c = ops.make_conv(T * B, 64 >> (i + 1), 64 >> (i + 1), Wd[i], Wd[i + 1], 4, 2, 1)
            launches += [(c, 0), (c, 1)]
    for i in range(3):
        c = ops.make_conv(B, 4 * 2 ** (i + 1), 4 * 2 ** (i + 1), Wg[i + 1], Wg[i], 4, 2, 1)
        launches += [(c, 0), (c, 1)]
    labels = nt_labels(launches, dt)
    # igemm_nt8s and the 128 x 128 buffer-descriptor kernel (plain and, in the 16-bit modes, with a K split; fp32 K loops are twice
    # as many K tiles long and fill the chip without)
    # 147 / 148: igemm_nt8s (plain / K splits); 151 / 152: the same design on 128 x 128 tiles (igemm_nt8h) for the single-tape layers
    assert 147 in labels and (dtype != "bf16" or labels & {148, 151, 152}), labels
    assert not labels & {16, 32, 64, 128}, labels     # nothing of this falls back to the register-staged kernels
    # the weight-gradient GEMMs split M over workgroups at this size
    assert all(ops.conv_wgrad_ws_bytes(c, dt) > 0 for c, _ in launches)


def test_mnist_b256_fp32():
    B = 256
    orc, G, D, E, tr, got, want = tmn.run_steps("f32", B, 1, seed=2, lrs=(0.0, 0.0, 0.0))
    for k in ("g_loss", "d_loss", "info_loss"):
        assert abs(got[0][k] - want[0][k]) < 1e-4, (k, got[0][k], want[0][k])
    eg_, ee = arena_rel_err(G, orc.G, tmn.PRE_BN_BIAS), arena_rel_err(E, orc.E)
    assert eg_ < 2e-2 and ee < 2e-2, (eg_, ee)
    # the generator's two 3x3 convolutions over the 2x-upsampled maps carry 97 % of the FLOPs: 128 -> 128 at 16x16, 128 -> 64 at 32x32
    ops, dt = eg.ops, eg.ops.EG_F32
    c1 = ops.make_conv(B, 8, 8, 128, 128, 3, 1, 1, 1)
    labels = nt_labels([(c1, 0)], dt)
    assert labels <= {147, 131}, labels


def _small_net_dispatch(dt, B, ch):
    """the 64-channel trunks of the dSprites networks at full batch (dSprites/rp.py:95-110,165-183): which kernels their launches are
    dispatched to, asked with the split-K scratch a trainer actually lends (eg_igemm_nt_tile_ep)"""
    ops = eg.ops
    labels = set()
    for H, ci, co in ((32, 32, 32), (16, 32, 64), (8, 64, 64)):                 # trunk convolutions 2..4 (the first reads the image)
        c = ops.make_conv(B, H, H, ci, co, 4, 2, 1)
        labels |= {ops.nt_tile(c, dt, False) % 1000, ops.nt_tile(c, dt, True) % 1000}
        assert ops.conv_wgrad_ws_bytes(c, dt) > 0                               # weight gradients split M over workgroups
    # N < 128 columns: the register-staged 128 x {32, 64} tiles; nothing may be routed to a kernel that needs 128-column tiles
    assert labels <= {32, 64, 128}, labels
    c64 = ops.make_conv(B, 8, 8, 64, 64, 4, 2, 1)
    assert ops.conv_wgrad_variant(c64, dt) == 2                                 # the 64-channel parity-class weight-gradient kernel
    for H, ci, co in ((32, 32, 32), (16, 32, 64)):                              # ... and its 32-channel instantiation (round 3)
        assert ops.conv_wgrad_variant(ops.make_conv(B, H, H, ci, co, 4, 2, 1), dt) == 2
    # the image-side layers run without patch rows / column tensors in HBM: first trunk layer forward + weight gradient, generator's last layer
    assert ops.conv_img_mfma_ok(dt, ch, 64, 64, 32, 4, 2, 1) and ops.wgrad_img_ok(dt, ch, 64, 64, 32, 4, 2, 1) and ops.convt_img_mfma_ok(dt, ch, 32, 32, 64, 4, 2, 1)


def _small_net_engines_direct(tr):
    """the trainer's own engines took those paths (not only 'the library could')"""
    for eng in (tr.de, tr.ee):
        assert eng.img_direct and eng.wgrad_direct, (eng.img_direct, eng.wgrad_direct)


def test_dsprites_b128_bf16():
    B = 128
    orc, G, D, E, tr, got, want = tds.run_steps("bf16", B, 1, seed=2, lrs=(0.0, 0.0))
    for k in tds.NAMES:
        assert abs(got[0][k] - want[0][k]) < 3e-2 * max(1.0, abs(want[0][k])), (k, got[0][k], want[0][k])
    eg_, ee = arena_rel_err(G, orc.G, tds.PRE_BN_BIAS), arena_rel_err(E, orc.E)
    assert eg_ < 0.25 and ee < 0.1, (eg_, ee)
    _small_net_dispatch(eg.ops.EG_BF16, B, 1)
    _small_net_engines_direct(tr)


def test_colored_b512_fp16():
    B = 512
    orc, G, D, E, tr, got, want = tco.run_steps("f16", B, 1, seed=2, lrs=(0.0, 0.0))
    for k in tco.NAMES:
        assert abs(got[0][k] - want[0][k]) < 3e-2 * max(1.0, abs(want[0][k])), (k, got[0][k], want[0][k])
    eg_, ee = arena_rel_err(G, orc.G, tco.PRE_BN_BIAS), arena_rel_err(E, orc.E)
    assert eg_ < 0.25 and ee < 0.1, (eg_, ee)
    _small_net_dispatch(eg.ops.EG_F16, B, 3)
    _small_net_engines_direct(tr)


def test_celeba_b128_bf16_layerwise_kernels():
    """Layer-wise teacher forcing at the production size: after one CelebA iteration at B = 128 in bf16, every big
    layer's operands are taken from the trainer's OWN buffers and the 8-wave kernel's forward / backward-data outputs and the parity-class
    kernel's weight gradient are compared with fp32 torch arithmetic on the same bf16-rounded operands (celebA/EAD-GAN_celebA.py:78-90,
    110-120).  What remains is one bf16 rounding of the output (forward / backward-data: 2^-9 per element) or fp32 summation order
    (weight gradients, checked PER TAP) -- far below the 0.25 / 0.1 end-to-end bounds above."""
    B = 128
    orc, G, D, tr, got, want = tce.run_steps("bf16", B, 1, seed=2, lrs=(0.0, 0.0, 0.0))
    ops, dt = eg.ops, eg.ops.EG_BF16
    de, ge = tr.de, tr.ge
    nchw = lambda t: t.float().permute(0, 3, 1, 2).contiguous()
    bq = lambda w: w.detach().to(torch.bfloat16).float()
    ws = eg.engine.Workspace.get(G.arena.flat.device)

    def wgrad_kernel(c, x_in, dy, Cout, Cin):
        ns = ops.conv_wgrad(c, dt, x_in, dy, ws.slab, 0)
        out = torch.zeros(Cout * Cin * 16, device="cuda")
        ops.wgrad_reduce(ws.slab, ns, Cout, Cout, Cin, 16, out, accumulate=0)
        return out.view(Cout, Cin, 4, 4)

    # ---- discriminator, layers 1..3 over the info step's three tapes (D(gen), D(scaled), D(real)) ----
    for i in range(3):
        r, m = de.mid[i], de._m(i + 1)
        Wq = bq(m.weight_orig)
        assert ops.conv_wgrad_variant(de.geo[3]["mid"][i], dt) == 2               # the parity-class kernel
        assert ops.nt_tile(de.geo[3]["mid"][i], dt, False) % 1000 in (147, 148, 151, 152) and ops.nt_tile(de.geo[3]["mid"][i], dt, True) % 1000 in (147, 148, 151, 152)
        gw_ref = torch.zeros_like(Wq)
        for t in range(3):
            sl = slice(t * B, (t + 1) * B)
            x, y, g = nchw(de.a[i][sl]), nchw(de.a[i + 1][sl]), nchw(de.dz[i + 1][sl])
            pre, cols = _conv_ref(x, Wq)
            ref = torch.nn.functional.leaky_relu(pre / de.sigma[i + 1][t] + m.bias.detach()[None, :, None, None], 0.1)
            assert _rel(y, ref) < 6e-3, ("D forward", i, t, _rel(y, ref))
            back = _convT_ref(g, Wq, x.shape[-2:]) * torch.where(x > 0, 1.0, 0.1) / de.sigma[i][t]
            assert _rel(nchw(de.dz[i][sl]), back) < 6e-3, ("D backward-data", i, t)
            gw_ref += (g.reshape(B, g.shape[1], -1) @ cols.transpose(1, 2)).sum(0).reshape(Wq.shape)
            del x, y, g, pre, cols, ref, back
        gw = wgrad_kernel(de.geo[3]["mid"][i], de.a[i], de.dz[i + 1], r.Cout, r.Cin)
        for kh in range(4):
            for kw in range(4):
                e = _rel(gw[:, :, kh, kw], gw_ref[:, :, kh, kw])
                assert e < 2e-3, ("D weight gradient", i, kh, kw, e)
    # ---- generator, ConvTranspose2d layers 1..3 (conv view: forward = backward-data kernel, input gradient = forward kernel) ----
    for i, idx in enumerate((1, 4, 7)):
        r = ge.mid[i]
        Wq = bq(ge._p(idx, "weight"))                                           # [Cin_T = conv-view Cout][Cout_T][4][4]
        x = nchw(ge.h0 if i == 0 else ge.a[i - 1])
        z = nchw(ge.z[i])
        ref = _convT_ref(x, Wq, z.shape[-2:]) + ge._p(idx, "bias").detach()[None, :, None, None]
        assert _rel(z, ref) < 6e-3, ("G forward", i, _rel(z, ref))
        dzt = nchw(ge.dz[i])
        din, cols = _conv_ref(dzt, Wq)                                          # d(input) of the transposed convolution
        got_din = nchw(ge.dh0) if i == 0 else None
        if got_din is not None:
            assert _rel(got_din, din) < 6e-3, ("G backward-data", i)
        gw_ref = (x.reshape(B, x.shape[1], -1) @ cols.transpose(1, 2)).sum(0).reshape(Wq.shape)
        gw = wgrad_kernel(r.c, ge.dz[i], ge.h0 if i == 0 else ge.a[i - 1], r.Cout, r.Cin)
        for kh in range(4):
            for kw in range(4):
                e = _rel(gw[:, :, kh, kw], gw_ref[:, :, kh, kw])
                assert e < 2e-3, ("G weight gradient", i, kh, kw, e)
        del x, z, ref, dzt, din, cols

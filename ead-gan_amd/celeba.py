"""CelebA 64x64 path of EAD-GAN on MI355X: drop-in ``Generator`` / ``Discriminator`` / ``transformation_2D`` /
``get_matrix`` / ``affine_regularzier`` (names and signatures of celebA/EAD-GAN_celebA.py:67-158 and
celebA/utils_rpqxy.py:59-116) plus the fused train-loop entry :class:`CelebATrainer` (loop body :299-401).

Everything below the Python class surface runs as hand-written HIP kernels through the C ABI
(include/eadgan_hip.h).  ``nn.ConvTranspose2d`` / ``nn.Conv2d`` / ``nn.BatchNorm2d`` objects are kept ONLY as
parameter containers so that ``state_dict()`` keys, shapes and default initialisation are the reference's
(incl. ``weight_orig`` / ``weight_u`` / ``weight_v``); their ``forward`` is never called.
"""
from __future__ import annotations

import argparse

import numpy as np

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable
from torch.nn.utils import spectral_norm

from . import affine, engine, ops
from .affine import _code_to_theta, theta_to_matrix, transformation_2D      # noqa: F401  (drop-in names of the reference script)
from .engine import (ConvRec, DeviceSampler, InputGrad, ResidentStep, SideStream, SyncScratch, Workspace, _HipModule, _require_cuda, bn_bwd_epilogue,
                     bn_train_backward, bn_train_forward, convt_img, drop_in_backward, import_adam_moments, parse_dtype, stat_buffer, to_categorical,
                     wants_input_grad, wgrad_side)      # noqa: F401
from .ops import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH

# module-level hyper-parameters, mirroring the reference's global ``opt`` (argparse defaults, :39-51)
opt = argparse.Namespace(n_epochs=50, batch_size=16, lr=0.0002, b1=0.5, b2=0.999, n_cpu=8, latent_dim=200, code_dim=8,
                         n_classes=10, img_size=64, channels=3, sample_interval=4000)

# Reference path the tests compare the production one against (they monkeypatch it; nothing else changes it; engine.IMG_GEMM and
# engine.FUSE_DRAWS are the other two).
# optimizer.step() of a convolution weight and the refresh of its packed panels as ONE launch per layer (ops.adam_pack_conv / adam_pack_rows);
# False: one Adam launch over the arena (or bucket) followed by the re-packing launches (same bits either way)
FUSE_ADAM = True


def adam_bucket(eng, arena, tag, lo, hi, m, v, lr, betas, step):
    """optimizer.step() on one gradient bucket [lo, hi) of ``arena`` and the refresh of the packed panels of its layers.  The
    bucket's big convolution weight (``eng.fused_weight(tag)``) is updated AND re-packed by one launch; the remaining parameters of the
    bucket (biases, BatchNorm affine) by plain Adam launches on their slices.  The step counter has been ticked by the caller."""
    b1, b2 = betas
    fw = eng.fused_weight(tag) if FUSE_ADAM else None
    if fw is None:
        ops.adam_step_zero(arena.flat[lo:hi], arena.grad[lo:hi], m[lo:hi], v[lo:hi], hi - lo, lr, b1, b2, 1e-8, step, False, False)
        eng.repack_bucket(tag)
        return
    name, launch = fw
    off, k = arena.slices[name]
    assert lo <= off and off + k <= hi
    launch(arena.flat[off:off + k], arena.grad[off:off + k], m[off:off + k], v[off:off + k], lr, b1, b2, step)
    for a, b in ((lo, off), (off + k, hi)):
        if b > a:
            ops.adam_step_zero(arena.flat[a:b], arena.grad[a:b], m[a:b], v[a:b], b - a, lr, b1, b2, 1e-8, step, False, False)


G_WIDTHS = (1024, 512, 256, 128)
D_WIDTHS = (128, 256, 512, 1024)
LRELU_SLOPE = 0.1
SN_EPS = 1e-12


# ================================================================================================
# Generator
# ================================================================================================
class _GenEngine:
    """Static-shape forward/backward of the generator at one batch size."""

    def __init__(self, gen: "Generator", B: int, dtype: int):
        self.gen, self.B, self.dtype = gen, B, dtype
        dev = gen.arena.flat.device
        tdt = ops.torch_dtype(dtype)
        self.ws = ws = Workspace.get(dev)
        self.cin = gen.input_dim
        self.cpad = ops.round_up(self.cin, 8)
        W = G_WIDTHS
        s = gen.init_size                                              # 4
        # L0: ConvTranspose2d(cin,1024,4,1,0) on a 1x1 input == GEMM [B,cin] x [cin, 16*1024]
        self.l0 = ConvRec(dtype, B, 1, 1, self.cpad, 16 * W[0], 1, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.l0w = ConvRec(dtype, B, 1, 1, 16 * W[0], self.cpad, 1, 1, 0, device=dev, want_fwd=False, want_bwd=False, ws=ws)
        # L1..L3: ConvTranspose2d(k4,s2,p1) in conv view (Cout_cv = ConvT in-channels)
        self.mid = [ConvRec(dtype, B, s * 2 ** (i + 1), s * 2 ** (i + 1), W[i + 1], W[i], 4, 2, 1, device=dev, ws=ws) for i in range(3)]
        self.l4 = ConvRec(dtype, B, s * 16, s * 16, gen.channels, W[3], 4, 2, 1, device=dev, want_fwd=False, want_wgrad=False, ws=ws)
        # the same layer seen from the image side as a 1x1 conv over im2col patches (K = C*16): input/weight gradients on MFMA
        self.kp = gen.channels * 16
        self.l4p = ConvRec(dtype, B, s * 8, s * 8, self.kp, W[3], 1, 1, 0, device=dev, want_bwd=False, ws=ws)
        # ... its weight gradient straight from d(img) where the streaming kernel takes it (16-bit, 64 x 64: ops.wgrad_img_tn, the bits of
        # im2col_img + conv_wgrad): no patch rows exist then
        self.wgrad_tn = engine.WGRAD_IMG_TN and ops.wgrad_img_tn_ok(dtype, gen.channels, s * 16, s * 16, W[3], 4, 2, 1)
        self.patches = None if self.wgrad_tn else torch.empty(B * (s * 8) ** 2, self.kp, device=dev, dtype=tdt)
        # forward of the same layer as ONE GEMM over the input pixels with N = 16 taps x C columns + a col2im gather (eg_col2im_img): every
        # activation is read once instead of 16 times (4 phases x 4 taps of the implicit transposed convolution)
        self.l4g = ConvRec(dtype, B, s * 8, s * 8, W[3], self.kp, 1, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.cols4 = torch.empty(B * (s * 8) ** 2, self.kp, device=dev, dtype=tdt)
        ws.need_small(B * gen.channels)
        # activations
        e = lambda *shape, dt=tdt: torch.empty(shape, device=dev, dtype=dt)
        self.inp = e(B, self.cpad)
        self.h0 = e(B, s, s, W[0])
        self.z = [e(B, s * 2 ** (i + 1), s * 2 ** (i + 1), W[i + 1]) for i in range(3)]
        self.a = [torch.empty_like(t) for t in self.z]
        self.mean = [e(W[i + 1], dt=torch.float32) for i in range(3)]
        self.invstd = [e(W[i + 1], dt=torch.float32) for i in range(3)]
        self.sync_scratch = SyncScratch(W[1:], dev)                     # synchronised BatchNorm: local (n, mean, M2) / local sums
        self.img = e(B, gen.channels, s * 16, s * 16, dt=torch.float32)
        # gradient scratch (ping-pong between layers)
        self.dimg_z = torch.empty_like(self.img)
        self.da = [torch.empty_like(t) for t in self.z]
        self.dz = [torch.empty_like(t) for t in self.z]
        self.dh0 = torch.empty_like(self.h0)
        for i in range(3):
            ws.need_small(ops.bn_ws_floats(self.z[i].numel() // W[i + 1], W[i + 1]))
        ws.need_small(ops.bias_grad_ws_floats(B * 16, W[0]))
        ws.need_sums(2 * max(W))
        self._stat = {}                                                # (kind, layer) -> (row blocks, buffer) of the fused column statistics
        # d(loss)/d(inputs) from dh0 (NHWC: n' = t*1024 + co) and the master [cin][1024][4][4]: i = t, j = co
        self.input_grad = InputGrad(dtype, B, 16, W[0], self.cin, (1, 16, 16 * W[0]), dev, 2 * max(W))
        self.repack()

    def _p(self, idx, kind):
        return getattr(self.gen.conv_blocks[idx], kind)

    def _stat_buf(self, key, c, bwd, ep, C):
        return stat_buffer(self._stat, key, c, self.dtype, bwd, ep, C, self.inp.device)

    # gradient buckets in the order the backward pass completes them: (tag of the lane chain that writes it last, parameter names)
    BUCKETS = (("G4", ("conv_blocks.10.weight", "conv_blocks.10.bias")),
               ("G3", ("conv_blocks.7.weight", "conv_blocks.7.bias", "conv_blocks.8.weight", "conv_blocks.8.bias")),
               ("G2", ("conv_blocks.4.weight", "conv_blocks.4.bias", "conv_blocks.5.weight", "conv_blocks.5.bias")),
               ("G1", ("conv_blocks.1.weight", "conv_blocks.1.bias", "conv_blocks.2.weight", "conv_blocks.2.bias")),
               ("G0", ("conv_blocks.0.weight", "conv_blocks.0.bias")))

    def repack(self):
        for tag, _ in self.BUCKETS:
            self.repack_bucket(tag)

    def fused_weight(self, tag):
        """(parameter name, launcher) of the bucket's convolution weight if Adam + re-packing of it run as one launch, else None"""
        dt = self.dtype
        if tag == "G0":
            # [cin][1024][4][4] seen as [cin][16384]: panel row (t, co) = column co * 16 + t
            return ("conv_blocks.0.weight", lambda p, g, m, v, lr, b1, b2, step: ops.adam_pack_rows(
                dt, p, g, m, v, self.l0.wp_fwd, self.cin, 16 * G_WIDTHS[0], self.l0.Kpad_fwd, 16, G_WIDTHS[0], lr, b1, b2, 1e-8, step))
        if tag in ("G1", "G2", "G3"):
            r = self.mid[int(tag[1]) - 1]
            if ops.adam_pack_conv_ok(r.c, dt, True, True):
                return (f"conv_blocks.{(1, 4, 7)[int(tag[1]) - 1]}.weight", lambda p, g, m, v, lr, b1, b2, step: ops.adam_pack_conv(
                    r.c, dt, p, g, m, v, lr, b1, b2, 1e-8, step, r.wp_fwd, r.wp_bwd))
        return None

    def repack_bucket(self, tag):
        """re-pack the panels of one gradient bucket's layers (the optimizer lane updates bucket by bucket)"""
        g, dt = self.gen, self.dtype
        if tag == "G0":
            w0 = self._p(0, "weight")                                  # [cin][1024][4][4]
            ops.pack_strided(dt, w0, self.l0.wp_fwd, 16 * G_WIDTHS[0], self.cin, self.l0.Kpad_fwd, G_WIDTHS[0], 1, 16, 16 * G_WIDTHS[0])
        elif tag in ("G1", "G2", "G3"):
            i = int(tag[1]) - 1
            self.mid[i].pack(self._p((1, 4, 7)[i], "weight"))
        else:
            self.l4.pack(self._p(10, "weight"))
            ops.pack_strided(dt, self._p(10, "weight"), self.l4p.wp_fwd, G_WIDTHS[3], self.kp, self.l4p.Kpad_fwd, 1, self.kp, 0, 1)
            # wp[t*C + c][ci] = W[ci][c][t]   (master [128][C][4][4])
            ops.pack_strided(dt, self._p(10, "weight"), self.l4g.wp_fwd, self.kp, G_WIDTHS[3], self.l4g.Kpad_fwd, g.channels, 1, 16, self.kp)

    def forward(self, noise, labels, code, training=True, sync=None, img_after=None):
        """``training=False``: BatchNorm with the running statistics, nothing updated (module.eval()).  ``sync`` (a dp.SyncBN):
        batch statistics over all ranks (synchronised BatchNorm).  ``img_after``: an event the LAST launch waits for -- the one that
        rewrites ``self.img`` -- while the layers above run ahead of it (a lane chain of the caller may still read the previous image)."""
        dt, B, W = self.dtype, self.B, G_WIDTHS
        small = self.ws.small
        ops.concat_cast(dt, noise, labels, code, self.inp, B, self.cpad)
        # ONE 128-row tile x 128 column tiles, 4 K steps (1 GFLOP): the register-staged kernel (NT_REG) runs it in ~10 us where the planner's
        # persistent pipeline takes 22-24; same bits; step -0.6 % (profiles/r03_zh_ab_g0_variant.txt)
        ops.conv_fwd(self.l0.c, dt, self.inp, self.l0.wp_fwd, self.h0, ops.epilogue(bias=self._p(0, "bias"), bias_mod=W[0], nt_variant=ops.NT_REG))
        x = self.h0
        for i, idx in enumerate((1, 4, 7)):
            r = self.mid[i]
            bn = self.gen.conv_blocks[idx + 1]
            M = self.z[i].numel() // W[i + 1]
            # BatchNorm batch statistics from the transposed convolution's epilogue where it can take them: z is read once (apply) instead of twice
            fused = self._stat_buf(("fwd", i), r.c, True, ops.epilogue(bias=self._p(idx, "bias")), W[i + 1]) if (training and sync is None) else (0, None)
            ops.conv_bwd_data(r.c, dt, x, r.wp_bwd, self.z[i],
                              ops.epilogue(bias=self._p(idx, "bias"), stat_mode=ops.STAT_MOMENTS if fused[0] else ops.STAT_NONE, stat_out=fused[1]))
            bn_train_forward(dt, self.z[i], self.a[i], M, W[i + 1], bn, self.mean[i], self.invstd[i], small, ACT_RELU, 0.0, sync, self.sync_scratch.stats[i],
                             training, fused)
            x = self.a[i]
        # the last transposed convolution + Tanh, in one launch where the kernel takes it: the GEMM's 48 columns per pixel stay in LDS
        SideStream.wait(img_after)
        convt_img(dt, x, self.l4g, self.cols4, self.l4, self._p(10, "bias"), ACT_TANH, self.img, True)
        return self.img

    def backward(self, dimg, grad, side=None, sync=None, store=False, *, dinp=None, need_wgrad=True, training=True):
        """Differentiates the LATEST forward of this engine (the activations are the engine's, one set per batch size and dtype).
        Accumulates d(loss)/d(params) into the flat gradient tensor ``grad`` (arena layout).  ``sync``: as in forward.  With ``side`` (an
        engine.SideStream) the weight/bias-gradient work of every layer is enqueued there, behind a fork taken right after
        the layer's output gradient exists; the caller joins before it reads ``grad``.
        ``store``: every slot of ``grad`` has exactly ONE writer in this pass (weights: the slab reduction; convolution biases: the column
        sums; BatchNorm affine: the statistics' final launch), so a caller that wants the gradient of this pass alone -- the trainer --
        lets each of them store instead of add: ``grad`` need not be cleared first and is never read.  The default keeps autograd's
        accumulate contract (the drop-in modules).
        ``dinp`` (fp32 [B, cin]): receives d(loss)/d(cat(noise, labels, code)) after the last launch of the pass.  ``need_wgrad=False``: no
        weight-gradient chain runs and no bias / BatchNorm parameter gradient is written (``grad`` is not touched, may be None).
        ``training=False``: the forward ran with the running statistics (``forward(training=False)``) -- BatchNorm is elementwise
        (eg_bn_bwd_eval), input gradients only: combine with ``need_wgrad=False``.  The defaults launch what they always launched."""
        dt, B, W, ws, gen = self.dtype, self.B, G_WIDTHS, self.ws, self.gen
        assert training or not need_wgrad, "eval-mode backward yields input gradients only"
        acc = not store
        batch_stats = training and sync is None         # the BatchNorm-backward epilogues form the training-mode dy and its sums
        pscr = self.input_grad.scratch                  # where parameter gradients land that nobody asked for
        gof = lambda name: gen.arena.grad_of(name, grad)
        C, S = gen.channels, self.img.shape[-1]
        direct = ops.conv_img_mfma_ok(dt, C, S, S, W[3], 4, 2, 1)
        if not direct:
            # tanh backward fused with the bias gradient of the last ConvTranspose2d
            ops.act_grad_mul_bias_nchw(dimg, self.img, self.dimg_z, B, C, S * S, ACT_TANH, 0.0, ws.small,
                                       gof("conv_blocks.10.bias") if need_wgrad else pscr[:C], accumulate=acc and need_wgrad)
            # L4 = ConvTranspose2d(128 -> C): weight / input gradients as 1x1-conv GEMMs over im2col patches of d(img)
            ops.im2col_img(dt, self.dimg_z, self.patches, B, C, S, S, 4, 2, 1, self.kp)

        def l4_wgrad(wsw):
            if direct:                                  # d(img) * tanh' only feeds the weight gradient: formed here, beside the main chain
                ops.act_grad_mul_bias_nchw(dimg, self.img, self.dimg_z, B, C, S * S, ACT_TANH, 0.0, wsw.small, gof("conv_blocks.10.bias"),
                                           accumulate=acc)
            if direct and self.wgrad_tn:                # straight from dimg_z; the split plan of the per-tap launch below (which takes no target)
                ns = ops.wgrad_img_tn(dt, [self.dimg_z], self.a[2], wsw.slab, B, C, S, S, W[3])
            else:
                if direct:
                    ops.im2col_img(dt, self.dimg_z, self.patches, B, C, S, S, 4, 2, 1, self.kp)
                ns = ops.conv_wgrad(self.l4p.c, dt, self.patches, self.a[2], wsw.slab, wsw.wgs_target)
            ops.wgrad_reduce(wsw.slab, ns, W[3], W[3], self.kp, 1, gof("conv_blocks.10.weight"), accumulate=acc)
        if need_wgrad:                                  # (direct: dimg_z and the patch rows feed nothing else)
            wgrad_side(side, ws, 0, l4_wgrad, "G4")
        bn_of = lambda i: gen.conv_blocks[(1, 4, 7)[i] + 1]
        bwd_ep = lambda fused, i: bn_bwd_epilogue(fused[1], self.z[i], self.mean[i], self.invstd[i], bn_of(i)) if fused[0] else None
        fused = (0, None)                               # (row blocks, sums) if da[i] came with its BatchNorm backward sums (then it holds dy)
        if direct:
            # d(a) = Conv2d(C -> 128, 4, 2, 1) of d(img) * tanh'(img): straight from the two fp32 images, no patch rows -- and, in the same
            # launch, dy = da * relu'(bn(z)) with the two sums of the last BatchNorm layer's backward
            if batch_stats:
                fused = stat_buffer(self._stat, "bwd2", None, dt, False, None, W[3], self.inp.device, nrb=lambda: ops.conv_img_mfma_stat_blocks(B, S, S))
            ops.conv_img_mfma(dt, [dimg], self.l4p.wp_fwd, self.da[2], B, C, S, S, bwd_ep(fused, 2), gates=[self.img], gate_act=ACT_TANH)
        else:
            ops.conv_fwd(self.l4p.c, dt, self.patches, self.l4p.wp_fwd, self.da[2], None)
        # L3..L1
        for i, idx in ((2, 7), (1, 4), (0, 1)):
            r = self.mid[i]
            M = self.z[i].numel() // W[i + 1]
            if need_wgrad:
                dgamma, dbeta = gof(f"conv_blocks.{idx + 1}.weight"), gof(f"conv_blocks.{idx + 1}.bias")
            else:
                dgamma, dbeta = pscr[:W[i + 1]], pscr[W[i + 1]:2 * W[i + 1]]
            bn_train_backward(dt, self.z[i], self.da[i], self.dz[i], M, W[i + 1], bn_of(i), self.mean[i], self.invstd[i], ACT_RELU, 0.0,
                              dgamma, dbeta, ws, sync, self.sync_scratch.sums[i], fused, acc and need_wgrad, training)
            x_in = self.a[i - 1] if i > 0 else self.h0

            def mid_wgrad(wsw, i=i, idx=idx, r=r, M=M, x_in=x_in):
                ns = ops.conv_wgrad(r.c, dt, self.dz[i], x_in, wsw.slab, wsw.wgs_target)
                ops.wgrad_reduce(wsw.slab, ns, r.Cout, r.Cout, r.Cin, 16, gof(f"conv_blocks.{idx}.weight"), accumulate=acc)
                ops.bias_grad(dt, self.dz[i], M, W[i + 1], wsw.small, gof(f"conv_blocks.{idx}.bias"), accumulate=acc)
            if need_wgrad:
                wgrad_side(side, ws, i + 1, mid_wgrad, f"G{i + 1}")
            fused = (0, None)
            if i > 0 and batch_stats:
                # the launch that produces d(a[i-1]) also forms dy = da * relu'(bn(z)) and the two sums of that layer's BatchNorm backward
                fused = self._stat_buf(("bwd", i - 1), r.c, False, ops.epilogue(), W[i])
            ops.conv_fwd(r.c, dt, self.dz[i], r.wp_fwd, self.da[i - 1] if i > 0 else self.dh0, bwd_ep(fused, i - 1))

        # L0
        def l0_wgrad(wsw):
            ns = ops.conv_wgrad(self.l0w.c, dt, self.dh0, self.inp, wsw.slab, wsw.wgs_target)
            ops.wgrad_reduce(wsw.slab, ns, self.cpad, self.cin, W[0], 16, gof("conv_blocks.0.weight"), accumulate=acc)
            ops.bias_grad(dt, self.dh0, B * 16, W[0], wsw.small, gof("conv_blocks.0.bias"), accumulate=acc)
        if need_wgrad:
            wgrad_side(side, ws, 0, l0_wgrad, "G0")
        if dinp is not None:
            self.input_grad.run(self.dh0, self._p(0, "weight"), dinp)


class Generator(_HipModule):
    """Drop-in for celebA/EAD-GAN_celebA.py:67-102.  ``forward(noise, labels, code) -> img [B,3,64,64]``."""

    def __init__(self, latent_dim=None, code_dim=None, n_classes=None, img_size=None, channels=None, dtype="f32"):
        super().__init__()
        g = lambda v, name: getattr(opt, name) if v is None else v
        self.latent_dim, self.code_dim, self.n_classes = g(latent_dim, "latent_dim"), g(code_dim, "code_dim"), g(n_classes, "n_classes")
        self.img_size, self.channels = g(img_size, "img_size"), g(channels, "channels")
        if self.img_size != 64 or self.channels > 4:
            raise ValueError("the CelebA generator is defined for 64x64 images (reference: img_size // 2**4 == 4)")
        self.input_dim = self.latent_dim + self.code_dim + self.n_classes
        self.init_size = self.img_size // 2 ** 4
        W = G_WIDTHS
        self.conv_blocks = nn.Sequential(
            nn.ConvTranspose2d(self.input_dim, W[0], 4, 1, 0),
            nn.ConvTranspose2d(W[0], W[1], 4, stride=2, padding=1), nn.BatchNorm2d(W[1]), nn.ReLU(),
            nn.ConvTranspose2d(W[1], W[2], 4, stride=2, padding=1), nn.BatchNorm2d(W[2]), nn.ReLU(),
            nn.ConvTranspose2d(W[2], W[3], 4, stride=2, padding=1), nn.BatchNorm2d(W[3]), nn.ReLU(),
            nn.ConvTranspose2d(W[3], self.channels, 4, stride=2, padding=1), nn.Tanh())
        self._init_engine_state(dtype)

    def engine(self, B) -> _GenEngine:
        self.arena
        key = (B, self.compute_dtype)
        if key not in self._engines:
            self._engines[key] = _GenEngine(self, B, self.compute_dtype)
        return self._engines[key]

    def forward(self, noise, labels, code):
        _require_cuda(noise)
        eng = self.fresh_engine(noise.shape[0])
        if not self.training and not wants_input_grad(noise, labels, code):
            # inference (generate_image.py:146-154, gen_imgs.py:106-120): running-stat BatchNorm, no autograd graph
            with torch.no_grad():
                return eng.forward(noise.float().contiguous(), labels.float().contiguous(), code.float().contiguous(), training=False).clone()
        # train mode: input and parameter gradients from one pass (batch statistics couple the samples, the gradient reflects it);
        # eval mode with an input that requires grad: the same eval forward, input gradients only
        params = [p for p in self.parameters()]
        return _GenFn.apply(eng, self.training, noise.float().contiguous(), labels.float().contiguous(), code.float().contiguous(), *params)


class _GenFn(torch.autograd.Function):
    """autograd bridge so the drop-in modules compose with torch losses/optimizers (eager mode).  The activations live in the engine:
    ``backward`` differentiates the engine's LATEST forward, so call it before the module runs again at this batch size."""

    @staticmethod
    def forward(ctx, eng, training, noise, labels, code, *params):
        ctx.eng, ctx.training = eng, training
        ctx.widths = (noise.shape[1], labels.shape[1], code.shape[1])
        return eng.forward(noise, labels, code, training=training).clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, dimg):
        ins, grads = drop_in_backward(ctx.eng, dimg, ctx.needs_input_grad[2:5], ctx.needs_input_grad[5:], ctx.training, ctx.widths)
        return (None, None, *ins, *grads)


# ================================================================================================
# Discriminator / Q network
# ================================================================================================
class _DiscEngine:
    """Static-shape forward/backward of the discriminator for up to NT "tapes" (independent forwards, each with its
    own spectral-norm power iteration).  D has no BatchNorm, so the tapes of one sub-step are batched along M into
    single launches: epilogues pick 1/sigma per tape, ONE weight-gradient GEMM runs over all tapes on gradients that
    already carry 1/sigma_tape (dzs = dz/sigma), and the rank-1 spectral-norm terms  -<G_t,W>/sigma_t^2 u_t v_t^T
    are added by a single-pass reduction whose coefficients come from activations
    (<G_t,W>/sigma_t^2 = sum dzs_t * (z_t - bias)), never from a second sweep over the weights."""

    NT = 3     # the info step runs three forwards before one backward (celebA/EAD-GAN_celebA.py:380-388)
    # gradient buckets in the order the backward pass completes them (see _GenEngine.BUCKETS)
    BUCKETS = (("D4", ("main.8.weight", "main.8.bias")), ("D3", ("main.6.bias", "main.6.weight_orig")), ("D2", ("main.4.bias", "main.4.weight_orig")),
               ("D1", ("main.2.bias", "main.2.weight_orig")), ("D0", ("main.0.bias", "main.0.weight_orig")))

    def __init__(self, disc: "Discriminator", B: int, dtype: int):
        self.disc, self.B, self.dtype = disc, B, dtype
        dev = disc.arena.flat.device
        self.ws = ws = Workspace.get(dev)
        W, C, S, NT = D_WIDTHS, disc.channels, disc.img_size, self.NT
        self.C, self.S = C, S
        self.nout = disc.n_out
        tdt = ops.torch_dtype(dtype)
        self.kp = C * 16
        self.cin = [self.kp, W[0], W[1], W[2]]                 # gathered channels of layer i (layer 0: im2col patches)
        self.hw = [S >> (i + 1) for i in range(4)]             # output extent of layer i
        # packed panels live in per-layer records built for the largest batch; geometry structs per tape count
        self.l1 = ConvRec(dtype, B, S, S, C, W[0], 4, 2, 1, device=dev, want_fwd=False, want_wgrad=False, ws=ws)       # d(img), tape 0 only
        self.l1p = ConvRec(dtype, NT * B, S // 2, S // 2, self.kp, W[0], 1, 1, 0, device=dev, want_bwd=False, ws=ws)  # image side as 1x1 conv over patches
        # d(img) as one GEMM over the layer-0 lattice with N = 16 taps x C columns + eg_col2im_img (see _GenEngine.l4g)
        self.l1g = ConvRec(dtype, B, S // 2, S // 2, W[0], self.kp, 1, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.cols1 = torch.empty(B * (S // 2) ** 2, self.kp, device=dev, dtype=tdt)
        self.mid = [ConvRec(dtype, NT * B, S >> (i + 1), S >> (i + 1), W[i], W[i + 1], 4, 2, 1, device=dev, ws=ws) for i in range(3)]
        self.head = ConvRec(dtype, NT * B, 4, 4, W[3], self.nout, 4, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.headw = ConvRec(dtype, NT * B, 1, 1, 16 * W[3], 32, 1, 1, 0, device=dev, want_fwd=False, want_bwd=False, ws=ws)
        self.geo = {}
        for T in range(1, NT + 1):
            g = {"l1p": ops.make_conv(T * B, S // 2, S // 2, self.kp, W[0], 1, 1, 0),
                 "mid": [ops.make_conv(T * B, S >> (i + 1), S >> (i + 1), W[i], W[i + 1], 4, 2, 1) for i in range(3)],
                 "headw": ops.make_conv(T * B, 1, 1, 16 * W[3], 32, 1, 1, 0)}
            self.geo[T] = g
        for i in range(4):
            ws.need_small(ops.sn_ws_floats(W[i], self.cin[i] * (16 if i else 1)))
            ws.need_small(ops.bias_grad_sn_ws_floats(NT * B * self.hw[i] ** 2, W[i], B * self.hw[i] ** 2))
        # tapes: contiguous along the batch axis
        self.img_direct = ops.conv_img_mfma_ok(dtype, C, S, S, W[0], 4, 2, 1)
        # layer 0's weight gradient straight from the tapes' images (ops.wgrad_img_tn: 16-bit, 64 x 64; the bits of im2col_img + conv_wgrad):
        # with the forward direct too, no patch rows exist
        self.wgrad_tn = engine.WGRAD_IMG_TN and self.img_direct and ops.wgrad_img_tn_ok(dtype, C, S, S, W[0], 4, 2, 1)
        self.patches = None if self.wgrad_tn else torch.empty(NT * B * (S // 2) ** 2, self.kp, device=dev, dtype=tdt)
        self.a = [torch.empty(NT * B, self.hw[i], self.hw[i], W[i], device=dev, dtype=tdt) for i in range(4)]
        self.out = torch.empty(NT * B, self.nout, device=dev, dtype=torch.float32)
        self.dz = [torch.empty_like(t) for t in self.a]
        self.dout_t = torch.empty(NT * B, 32, device=dev, dtype=tdt)
        self._head_scratch = None                       # head_losses: per-sample loss terms + arrival counter
        self.dimg = torch.empty(B, C, S, S, device=dev, dtype=torch.float32)
        kd = [self.kp] + [W[i] * 16 for i in range(3)]
        self.sigma = [torch.ones(NT, device=dev, dtype=torch.float32) for _ in range(4)]
        self.u = [torch.zeros(NT, W[i], device=dev, dtype=torch.float32) for i in range(4)]
        self.v = [torch.zeros(NT, kd[i], device=dev, dtype=torch.float32) for i in range(4)]
        self.coef = [torch.zeros(4, device=dev, dtype=torch.float32) for _ in range(4)]
        self.imgs = [None] * NT
        self.patch_ok = [False] * NT                    # tape has its patch rows (the weight gradient of layer 0 reads them)
        self._stat = {}                                 # (layer, T) -> (row blocks, buffer) of the fused bias-gradient / coefficient sums
        self._sn_arrays = None
        self._sn(0)
        self.repack()

    def _sn(self, t):
        """eg_sn_layer array of tape t (pointers are stable: module buffers and tape snapshots never move)."""
        if self._sn_arrays is None:
            self._sn_arrays = []
            for tt in range(self.NT):
                ent = [(self._m(i).weight_orig, self._m(i).weight_u, self._m(i).weight_v, self.sigma[i][tt:tt + 1], self.u[i][tt], self.v[i][tt])
                       for i in range(4)]
                self._sn_arrays.append(ops.sn_layers(ent))
            # own scratch: the power iterations may run on a side stream while the main stream uses the shared workspace
            self.sn_scratch = torch.empty(ops.sn_multi_ws_floats(self._sn_arrays[0]), device=self.ws.device, dtype=torch.float32)
        return self._sn_arrays[t]

    def _m(self, i):
        return self.disc.main[2 * i]

    def repack(self):
        for tag, _ in self.BUCKETS:
            self.repack_bucket(tag)

    def fused_weight(self, tag):
        """see _GenEngine.fused_weight"""
        if tag in ("D1", "D2", "D3"):
            i = int(tag[1])
            r = self.mid[i - 1]
            if ops.adam_pack_conv_ok(r.c, self.dtype, True, True):
                return (f"main.{2 * i}.weight_orig", lambda p, g, m, v, lr, b1, b2, step: ops.adam_pack_conv(
                    r.c, self.dtype, p, g, m, v, lr, b1, b2, 1e-8, step, r.wp_fwd, r.wp_bwd))
        return None

    def repack_bucket(self, tag):
        """re-pack the panels of one gradient bucket's layer (see _GenEngine.repack_bucket)"""
        if tag == "D0":
            self.l1.pack(self._m(0).weight_orig)
            # wp[t*C + c][co] = W[co][c][t]   (Conv2d master [128][C][4][4]; the transposed convolution reads it as [in = 128][out = C])
            ops.pack_strided(self.dtype, self._m(0).weight_orig, self.l1g.wp_fwd, self.kp, D_WIDTHS[0], self.l1g.Kpad_fwd, self.C, 1, 16, self.kp)
            ops.pack_strided(self.dtype, self._m(0).weight_orig, self.l1p.wp_fwd, D_WIDTHS[0], self.kp, self.l1p.Kpad_fwd, 1, self.kp, 0, 1)
        elif tag in ("D1", "D2", "D3"):
            i = int(tag[1]) - 1
            self.mid[i].pack(self._m(i + 1).weight_orig)
        else:
            self.head.pack(self._m(4).weight)

    def rows(self, i):
        """lattice rows of one tape at the output of layer i"""
        return self.B * self.hw[i] ** 2

    def _stat_buf(self, i, T, c, ep):
        """fused sums of layer i's bias gradient / spectral-norm coefficient in the backward-data launch that produces dzs_i (T tapes):
        (row blocks, buffer), (0, None) where that launch cannot take them (engine.stat_buffer; whole 256-row tiles per tape only)"""
        N = D_WIDTHS[i]
        return stat_buffer(self._stat, (i, T), c, self.dtype, True, ep, N, self.out.device,
                           nrb=lambda: ops.conv_stat_blocks(c, self.dtype, True, ep) if self.rows(i + 1) % 256 == 0 else 0,
                           floats=lambda nrb: N * nrb + nrb * (N // 128))

    def _sn_tape(self, t, training=True):
        ops.sn_power_iter_multi(self._sn(t), self.sn_scratch, training, SN_EPS)
        if not training:
            for i in range(4):
                self.u[i][t].copy_(self._m(i).weight_u)
                self.v[i][t].copy_(self._m(i).weight_v)

    def _im2col_tape(self, t, img):
        npix = self.B * (self.S // 2) ** 2
        ops.im2col_img(self.dtype, img, self.patches[t * npix:(t + 1) * npix], self.B, self.C, self.S, self.S, 4, 2, 1, self.kp)
        self.patch_ok[t] = True

    def prepare(self, t0, imgs, training=True):
        """Image-independent head start of ``forward(imgs, t0, prepared=...)``: the tapes' power iterations (in list order, like
        consecutive D(...) calls) and the patch rows of the images that already exist (``None`` entries are left to forward; none are
        built where the weight gradient reads the images themselves).
        The trainer runs this on a side stream while the previous sub-step is still busy."""
        for k, img in enumerate(imgs):
            self._sn_tape(t0 + k, training)
            if img is not None and not self.wgrad_tn:
                self._im2col_tape(t0 + k, img)

    def forward(self, imgs, t0=0, training=True, prepared=None, head=True):
        """Runs len(imgs) forwards as tapes t0.. (power iterations in list order, like consecutive D(...) calls).
        ``head=False``: stop in front of the head (``head_losses`` runs it together with the losses).
        ``prepared``: per-tape flags of a preceding ``prepare`` call (power iterations done for all tapes, patch rows done where
        the flag is set).  Returns the head outputs [len(imgs)*B, 19] (a view of the tape buffer)."""
        dt, B, W, ws = self.dtype, self.B, D_WIDTHS, self.ws
        T = len(imgs)
        assert 1 <= T and t0 + T <= self.NT
        for k, img in enumerate(imgs):
            t = t0 + k
            self.imgs[t] = img
            if prepared is None:
                self._sn_tape(t, training)
            if prepared is None or not prepared[k]:
                if self.img_direct:
                    self.patch_ok[t] = False            # built by the weight-gradient chain if a backward pass wants them (backward)
                else:
                    self._im2col_tape(t, img)
        g = self.geo[T]
        sl = lambda buf, i: buf[t0 * (buf.shape[0] // self.NT):]
        ep = lambda i: ops.epilogue(bias=self._m(i).bias, sigma=self.sigma[i][t0:], sigma_rows=self.rows(i), act=ACT_LRELU, slope=LRELU_SLOPE)
        if self.img_direct:
            # first layer straight from the fp32 images of the T tapes (one launch, 1/sigma per tape): no patch rows on the main chain
            ops.conv_img_mfma(dt, [im.contiguous() for im in imgs], self.l1p.wp_fwd, sl(self.a[0], 0), B, self.C, self.S, self.S, ep(0))
        else:
            ops.conv_fwd(g["l1p"], dt, sl(self.patches, 0), self.l1p.wp_fwd, sl(self.a[0], 0), ep(0))
        for i in range(3):
            ops.conv_fwd(g["mid"][i], dt, sl(self.a[i], i), self.mid[i].wp_fwd, sl(self.a[i + 1], i + 1), ep(i + 1))
        K = 16 * W[3]
        out = self.out[t0 * B:(t0 + T) * B]
        if head:
            ops.dense_small_fwd(dt, sl(self.a[3], 3), self.head.wp_fwd, self._m(4).bias, out, T * B, K, self.head.Kpad_fwd, self.nout, ws.small)
        return out

    def head_fused_ok(self, T):
        return ops.head_fused_ok(self.dtype, T, 16 * D_WIDTHS[3], self.nout)

    def head_losses(self, t0, T, dout, loss, targets=None, scales=None, info=None):
        """The head of tapes t0..t0+T-1 (after ``forward(..., head=False)``), their losses (added to ``loss[0]``), ``dout`` = d(loss)/d(head
        output) and the head's input gradient dzs_3 -- ``backward(..., head_done=True)`` continues from there -- in TWO launches (the K-sliced
        dense head; slice combine + losses + dense backward) with the bits of the five they replace."""
        B, K = self.B, 16 * D_WIDTHS[3]
        sl = lambda buf: buf[t0 * (buf.shape[0] // self.NT):]
        if self._head_scratch is None:
            self._head_scratch = (torch.empty(3 * B, device=self.out.device, dtype=torch.float32),
                                  torch.zeros(1, device=self.out.device, dtype=torch.int32))
        terms, counter = self._head_scratch
        out = self.out[t0 * B:(t0 + T) * B]
        ns = ops.dense_small_fwd_slices(self.dtype, sl(self.a[3]), self.head.wp_fwd, T * B, K, self.head.Kpad_fwd, self.nout, self.ws.small)
        ops.head_fused(self.dtype, sl(self.a[3]), self.head.wp_fwd, self._m(4).bias, self.ws.small, ns, out, dout, sl(self.dz[3]), self.sigma[3][t0:],
                       B, T, K, self.head.Kpad_fwd, self.nout, loss, terms, counter, ACT_LRELU, LRELU_SLOPE, targets=targets, scales=scales, info=info)
        return out

    def backward(self, t0, T, dout, grad, need_wgrad=True, need_dimg=False, side=None, head_done=False, store=False):
        """``dout``: d(loss)/d(head output) of tapes t0..t0+T-1, [T*B,19] fp32.  Accumulates into flat ``grad`` (arena
        layout); returns d(loss)/d(img) of tape t0 when ``need_dimg``.  With ``side`` (engine.SideStream) the weight- and
        bias-gradient work is enqueued there (see _GenEngine.backward); the caller joins before it reads ``grad``.
        ``store``: as in _GenEngine.backward -- the T tapes are batched into ONE weight-gradient GEMM, one rank-1 reduction and one column-sum
        launch per layer, so with ``need_wgrad`` every slot of ``grad`` has exactly one writer here too (without it nothing is written)."""
        dt, B, W, ws, disc = self.dtype, self.B, D_WIDTHS, self.ws, self.disc
        acc = not store
        gof = lambda name: disc.arena.grad_of(name, grad)
        g = self.geo[T]
        sl = lambda buf: buf[t0 * (buf.shape[0] // self.NT):]
        K = 16 * W[3]
        if need_wgrad:
            def head_wgrad(wsw):
                ops.cast_pad(dt, dout, self.dout_t, T * B, self.nout, 32)
                ns = ops.conv_wgrad(g["headw"], dt, sl(self.a[3]), self.dout_t, wsw.slab, wsw.wgs_target)
                ops.wgrad_reduce(wsw.slab, ns, 32, self.nout, W[3], 16, gof("main.8.weight"), accumulate=acc)
                ops.dense_small_bgrad(dout, gof("main.8.bias"), T * B, self.nout, accumulate=acc)
            wgrad_side(side, ws, 0, head_wgrad, "D4")
        # dzs_3 = (W5^T dout) * lrelu'(a3) / sigma_3[tape]
        if not head_done:
            ops.dense_small_bwd(dt, dout, self.head.wp_fwd, sl(self.a[3]), sl(self.dz[3]), T * B, K, self.head.Kpad_fwd, self.nout, ACT_LRELU, LRELU_SLOPE,
                                self.sigma[3][t0:], B)
        fused = (0, None)                               # (row blocks, sums) if dzs_i came with its column sums
        for i in (3, 2, 1, 0):
            m = self._m(i)
            geo = g["mid"][i - 1] if i > 0 else g["l1p"]
            x_in = sl(self.a[i - 1]) if i > 0 else (None if self.wgrad_tn else sl(self.patches))
            if need_wgrad:
                def layer_wgrad(wsw, i=i, m=m, geo=geo, x_in=x_in, fused=fused):
                    if i == 0 and not self.wgrad_tn:
                        for t in range(t0, t0 + T):     # patch rows of tapes whose forward ran straight from the image
                            if not self.patch_ok[t]:
                                self._im2col_tape(t, self.imgs[t])
                    # the weight-gradient GEMM first: the column sums below (only the slab reduce needs their coefficient) do not fit on a CU
                    # beside a resident GEMM workgroup and used to hold the chain's GEMM back by ~50 us
                    if i == 0 and self.wgrad_tn:
                        # straight from the tapes' images, which stay intact until the caller has this chain behind it (CelebATrainer: READERS
                        # OF ge.img); the split plan of the per-tap launch it replaces (which takes no target)
                        ns = ops.wgrad_img_tn(dt, self.imgs[t0:t0 + T], sl(self.dz[0]), wsw.slab, B, self.C, self.S, self.S, W[0])
                    else:
                        ns = ops.conv_wgrad(geo, dt, x_in, sl(self.dz[i]), wsw.slab, wsw.wgs_target)
                    if fused[0]:
                        tiles_m = fused[0] // 4         # row blocks (of 256 or 128 lattice rows: the kernel's tile height) per sub-pixel phase
                        ops.bias_grad_sn_fused(fused[1], fused[0], W[i], tiles_m, tiles_m // T, T, self.sigma[i][t0:], gof(f"main.{2 * i}.bias"), self.coef[i],
                                               accumulate=acc)
                    else:
                        ops.bias_grad_sn(dt, sl(self.dz[i]), sl(self.a[i]), m.bias, T * self.rows(i), W[i], self.rows(i), self.sigma[i][t0:], LRELU_SLOPE,
                                         wsw.small, gof(f"main.{2 * i}.bias"), self.coef[i], accumulate=acc)
                    taps = 16 if i > 0 else 1
                    ops.wgrad_reduce_rank1(wsw.slab, ns, W[i], W[i], self.cin[i], taps, gof(f"main.{2 * i}.weight_orig"), T, self.coef[i],
                                           self.u[i][t0:], self.v[i][t0:], accumulate=acc)
                wgrad_side(side, ws, i + 1, layer_wgrad, f"D{i}")
            if i > 0:
                # dzs_{i-1} = conv^T(dzs_i, W_i) * lrelu'(a_{i-1}) / sigma_{i-1}[tape]
                kw = dict(sigma=self.sigma[i - 1][t0:], sigma_rows=self.rows(i), mask=sl(self.a[i - 1]), mask_act=ACT_LRELU, mask_slope=LRELU_SLOPE)
                # ... and, from the same tile, layer i-1's bias-gradient column sums and spectral-norm coefficient
                fused = self._stat_buf(i - 1, T, geo, ops.epilogue(**kw)) if need_wgrad else (0, None)
                if fused[0]:
                    kw.update(stat_mode=ops.STAT_SN_BIAS, stat_out=fused[1], stat_p=(self._m(i - 1).bias,), stat_slope=LRELU_SLOPE)
                ops.conv_bwd_data(geo, dt, sl(self.dz[i]), self.mid[i - 1].wp_bwd, sl(self.dz[i - 1]), ops.epilogue(**kw))
        if need_dimg:
            convt_img(dt, sl(self.dz[0]), self.l1g, self.cols1, self.l1, None, ACT_NONE, self.dimg, True)
            return self.dimg
        return None


class Discriminator(_HipModule):
    """Drop-in for celebA/EAD-GAN_celebA.py:105-138.  ``forward(img) -> (cat, cont, validity)``; the one
    19-channel head plays discriminator and Q-network (cat = softmax(out[:,9:19]), cont = out[:,1:9],
    validity = sigmoid(out[:,0]))."""

    def __init__(self, code_dim=None, n_classes=None, img_size=None, channels=None, dtype="f32"):
        super().__init__()
        g = lambda v, name: getattr(opt, name) if v is None else v
        self.code_dim, self.n_classes = g(code_dim, "code_dim"), g(n_classes, "n_classes")
        self.img_size, self.channels = g(img_size, "img_size"), g(channels, "channels")
        if self.img_size != 64 or self.channels > 4:
            raise ValueError("the CelebA discriminator is defined for 64x64 images")
        self.n_out = 1 + self.n_classes + self.code_dim
        W = D_WIDTHS
        self.main = nn.Sequential(
            spectral_norm(nn.Conv2d(self.channels, W[0], 4, 2, 1)), nn.LeakyReLU(LRELU_SLOPE, inplace=True),
            spectral_norm(nn.Conv2d(W[0], W[1], 4, 2, 1)), nn.LeakyReLU(LRELU_SLOPE, inplace=True),
            spectral_norm(nn.Conv2d(W[1], W[2], 4, 2, 1)), nn.LeakyReLU(LRELU_SLOPE, inplace=True),
            spectral_norm(nn.Conv2d(W[2], W[3], 4, 2, 1)), nn.LeakyReLU(LRELU_SLOPE, inplace=True),
            nn.Conv2d(W[3], self.n_out, 4, 1, 0))
        self._init_engine_state(dtype)
        self._next_tape = 0

    def engine(self, B) -> _DiscEngine:
        self.arena
        key = (B, self.compute_dtype)
        if key not in self._engines:
            self._engines[key] = _DiscEngine(self, B, self.compute_dtype)
        return self._engines[key]

    def raw_forward(self, img):
        """head output [B,19] with autograd support (eager path)."""
        _require_cuda(img)
        eng = self.fresh_engine(img.shape[0])
        t = self._next_tape
        self._next_tape = (t + 1) % _DiscEngine.NT
        return _DiscFn.apply(eng, t, self.training, img.float().contiguous(), *list(self.parameters()))

    def forward(self, img):
        out = self.raw_forward(img)
        cd, nc = self.code_dim, self.n_classes
        validity = torch.sigmoid(out[:, 0])
        cat = torch.softmax(out[:, cd + 1: cd + 1 + nc], dim=1)
        cont = out[:, 1: cd + 1]
        return cat, cont, validity


class _DiscFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, t, training, img, *params):
        ctx.eng, ctx.t = eng, t
        ctx.need_w = any(p.requires_grad for p in params)
        ctx.need_img = img.requires_grad
        return eng.forward([img], t, training).clone()

    @staticmethod
    def backward(ctx, dout):
        eng = ctx.eng
        scratch = torch.zeros_like(eng.disc.arena.grad)
        dimg = eng.backward(ctx.t, 1, dout.contiguous(), scratch, need_wgrad=ctx.need_w, need_dimg=ctx.need_img)
        grads = [scratch[off:off + k].view(p.shape) for p, (off, k) in zip(eng.disc.parameters(), eng.disc.arena.slices.values())]
        return (None, None, None, dimg.clone() if dimg is not None else None, *grads)


# ================================================================================================
# affine utilities (celebA/utils_rpqxy.py); the STN warp and the code -> matrix functions: affine.py
# ================================================================================================
def get_matrix(code_input_raw):
    """[B,>=5] latent codes -> [B,3,3] affine matrices R(theta) Z(p,q) T(x,y)  (utils_rpqxy.py:59-80)."""
    return theta_to_matrix(_code_to_theta("rpqxy", code_input_raw))


_regularizer = affine.regularizer(lambda real, trans, ld, B, target, scale, d_real, d_trans, pred: ops.loss_affine_rpqxy(
    real, trans, ld, 0, B, target, 5, scale, None, d_real, d_trans, pred), 5)


def affine_regularzier(real_code, trans_code):
    """closed-form relative-transform recovery (utils_rpqxy.py:82-116); spelling follows the reference."""
    return _regularizer(real_code, trans_code)


# ================================================================================================
# fused train-loop entry
# ================================================================================================
def pil_bilinear_tables(in_size: int, out_size: int):
    """Coefficient tables of PIL's antialiased bilinear resample of an 8-bit image from ``in_size`` to ``out_size`` pixels (what
    transforms.Resize does to a PIL image, celebA/EAD-GAN_celebA.py:194): Pillow's precompute_coeffs + normalize_coeffs_8bpc
    (libImaging/Resample.c) in the same double arithmetic -> (bounds int32 [out,2], kk int32 [out,ksize], ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                          # bilinear filter support 1.0
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.zeros(xmax, dtype=np.float64)
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w[x] = 1.0 - a if a < 1.0 else 0.0
        ww = 0.0
        for x in range(xmax):                            # left-to-right double sum, as in C
            ww += w[x]
        if ww != 0.0:
            w = w / ww
        for x in range(xmax):
            v = w[x] * (1 << 22)
            kk[xx, x] = int(v - 0.5) if w[x] < 0 else int(v + 0.5)
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def resize_center_crop_u8(images_u8: torch.Tensor, size: int = 64) -> torch.Tensor:
    """transforms.Resize(size) + transforms.CenterCrop(size) (celebA/EAD-GAN_celebA.py:194-196) of a uint8 [N,C,H,W] device tensor, on the
    device: the smaller edge goes to ``size`` with PIL's antialiased bilinear filter (horizontal pass, 8-bit intermediate, vertical pass,
    bit-exact against Image.resize), the centre ``size`` x ``size`` window is kept.  Returns uint8 [N,C,size,size] -- what DeviceInputs
    takes.  Only the rows / columns the crop keeps are computed."""
    _require_cuda(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise ValueError("images must be a uint8 [N, C, H, W] device tensor")
    N, C, H, W = images_u8.shape
    if W <= H:
        ow, oh = size, int(size * H / W)                 # torchvision: the smaller edge matches `size`
    else:
        oh, ow = size, int(size * W / H)
    top, left = int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))
    dev = images_u8.device
    src = images_u8.contiguous()
    bh, kh, ksh = pil_bilinear_tables(W, ow)
    bv, kv, ksv = pil_bilinear_tables(H, oh)
    # horizontal pass: only the source rows the vertical pass of the kept window reads; PIL skips the pass when the size does not change
    r0 = int(bv[top, 0])
    r1 = int(bv[top + size - 1, 0] + bv[top + size - 1, 1])
    tmp = torch.empty(N * C, r1 - r0, size, device=dev, dtype=torch.uint8)
    if ow != W:
        ops.resample_u8(src[:, :, r0:r1].contiguous(), tmp, N * C, r1 - r0, W, 1, torch.from_numpy(bh).to(dev), torch.from_numpy(kh).to(dev), ksh,
                        left, size, 0, r1 - r0)
    else:
        tmp.copy_(src[:, :, r0:r1, left:left + size].reshape(N * C, r1 - r0, size))
    out = torch.empty(N, C, size, size, device=dev, dtype=torch.uint8)
    if oh != H:
        bv2 = bv.copy()
        bv2[:, 0] -= r0                                  # the intermediate starts at source row r0
        ops.resample_u8(tmp, out, N * C, r1 - r0, size, 0, torch.from_numpy(bv2).to(dev), torch.from_numpy(kv).to(dev), ksv, top, size, 0, size)
    else:
        out.copy_(tmp[:, top - r0:top - r0 + size].reshape(N, C, size, size))
    return out


class DeviceInputs(DeviceSampler):
    """Device-side replacement of the loop's host input work (celebA/EAD-GAN_celebA.py:194-206 DataLoader + RandomHorizontalFlip +
    ToTensor + Normalize(0.5, 0.5); :308-317 numpy draws of z ~ N(0,1), code ~ U(-1,1), labels ~ randint): a uint8 [N,3,64,64] dataset
    resident in HBM (resized / cropped once on the way in: ``resize_center_crop_u8``) and a counter-based generator.  ``enqueue(trainer)`` fills the trainer's
    static input slots with six launches and ticks the device step counter; inside ``trainer.capture(inputs=...)`` they become part
    of the iteration's hipGraph, so a replay needs no host work at all.  Draws are reproducible per (seed, step) and have the
    reference's distributions; they are NOT numpy's stream (parity tests keep using ``load_inputs`` with host draws)."""

    def __init__(self, dataset_u8: torch.Tensor, seed: int = 0, flip: bool = True, sampling: str = "permutation", *, rank: int = 0,
                 world: int = 1):
        """``sampling``, ``rank`` / ``world``: engine.DeviceSampler ("permutation" = DataLoader(shuffle=True) of the reference, :204-206;
        batches of constant size straddle epoch ends)"""
        _require_cuda(dataset_u8)
        if dataset_u8.dtype != torch.uint8 or dataset_u8.dim() != 4:
            raise ValueError("dataset must be a uint8 [N, C, H, W] device tensor")
        super().__init__(dataset_u8, seed, sampling, rank=rank, world=world)
        self.flip = flip

    def enqueue(self, tr: "CelebATrainer"):
        B = tr.B
        N, C, H, W = self.data.shape
        # the five draws + the one-hot labels as one launch, the counter tick inside the gather: 3 launches instead of 8 at the head of
        # the iteration's critical chain (the same values: a draw depends on (element, step, stream id, seed) only)
        self.begin_draws()
        idx = self.sample_indices(B, 1)                                 # which images: epoch permutation / uniform draws
        flips = self.buf("flips", (B,), torch.uint8)
        self.draw(ops.RNG_BERNOULLI, flips, 0.5, 0.0, 2)                # RandomHorizontalFlip(p=0.5)
        self.draw(ops.RNG_NORMAL, tr.z, 0.0, 1.0, 3)
        self.draw(ops.RNG_UNIFORM, tr.code, -1.0, 1.0, 4)
        self.labels_onehot("labels", tr.onehot, tr.G.n_classes, 5, lab=tr.labels)
        self.end_draws()
        fused = engine.FUSE_DRAWS

        def gather():                                   # ToTensor + Normalize(.5,.5)
            ops.gather_u8_images(self.data, idx, flips if self.flip else None, tr.real, B, C, H, W, 2.0 / 255.0, -1.0, tick=self.step if fused else None)
        if fused and tr.side is not None:
            tr._inputs_tail = gather                    # the pipelined body runs it on its preparation lane, in front of the warp
            return
        gather()
        if not fused:
            self.tick()


# data parallel: gradient buckets that cross the links as one message, in completion order (contiguous in the arenas)
COMM_GROUPS = {"G": (("G4", "G3", "G2"), ("G1", "G0")), "D": (("D4", "D3"), ("D2", "D1", "D0"))}


class CelebATrainer(ResidentStep):
    """One call of :meth:`train_step` == one iteration of the reference loop body
    (celebA/EAD-GAN_celebA.py:299-401): G adversarial step, D step, info+affine step, three Adams
    (lr 1e-3 / 2e-4 / 2e-4, betas (.5,.999), :211-217) -- hand-scheduled over the C ABI with dead work removed
    (no D weight gradients in the G step) and, optionally, replayed from one hipGraph.

    ``allreduce``: optional callable(flat_grad_tensor) applied after each backward pass (data parallel)."""

    def __init__(self, generator: Generator, discriminator: Discriminator, batch_size: int, dtype="bf16", allreduce=None,
                 lr_g=1e-3, lr_d=2e-4, lr_info=2e-4, betas=(0.5, 0.999), lambda_cat=1.0, lambda_con=1.0, lambda_affine=1.0, overlap=True,
                 sync_bn=None):
        self.G, self.D, self.B = generator, discriminator, batch_size
        dt = parse_dtype(dtype)
        generator.set_compute_dtype(dt)
        discriminator.set_compute_dtype(dt)
        self.ge, self.de = generator.engine(batch_size), discriminator.engine(batch_size)
        dev = generator.arena.flat.device
        self.dev = dev
        self.allreduce = allreduce
        # optional dp.SyncBN: the generator's BatchNorm statistics over the global batch (N ranks == 1 rank at equal global batch);
        # default (None): per-rank statistics, like torch DistributedDataParallel without SyncBatchNorm
        self.sync_bn = sync_bn
        self.lr = (lr_g, lr_d, lr_info)
        self.betas = betas
        self.lam = (lambda_cat, lambda_con, lambda_affine)
        ga, da = generator.arena, discriminator.arena
        z = lambda n: torch.zeros(n, device=dev, dtype=torch.float32)
        self.mG, self.vG = z(ga.numel), z(ga.numel)                     # optimizer_G
        self.mD, self.vD = z(da.numel), z(da.numel)                     # optimizer_D
        self.miG, self.viG, self.miD, self.viD = z(ga.numel), z(ga.numel), z(da.numel), z(da.numel)   # optimizer_info
        self.steps = torch.zeros(3, device=dev, dtype=torch.int32)
        self.losses = torch.zeros(4, device=dev, dtype=torch.float32)   # g, d, info
        B = batch_size
        C, S = generator.channels, generator.img_size
        self.theta = torch.empty(B, 2, 3, device=dev, dtype=torch.float32)
        self.scaled = torch.empty(B, C, S, S, device=dev, dtype=torch.float32)
        self.dout = torch.empty(3 * B, 19, device=dev, dtype=torch.float32)
        # static input slots (a captured graph reads these)
        self.real = torch.empty(B, C, S, S, device=dev, dtype=torch.float32)
        self.z = torch.empty(B, generator.latent_dim, device=dev, dtype=torch.float32)
        self.code = torch.empty(B, generator.code_dim, device=dev, dtype=torch.float32)
        self.onehot = torch.empty(B, generator.n_classes, device=dev, dtype=torch.float32)
        self.labels = torch.empty(B, device=dev, dtype=torch.int64)
        self.graph = None
        self.inputs = None
        self.log = None
        # test hook: callable(k) run on the main stream in front of the backward pass of sub-step k = 1, 2, 3, at a point where no launch of
        # an earlier pass still reads either gradient arena (tests/test_gpu_grad_store.py poisons them there).  To give it that point the
        # pipelined body adds ONE wait in front of step 2's hook (for step 1's generator update, which otherwise runs beside step 2): a run
        # with the hook set is the shipped iteration with that extra edge -- same launches, same operands, same bits.  None in production
        # and in every capture (bench.py, train.py): the branch is then never taken.
        self.before_backward = None
        # weight-gradient chains and re-packing run on a second stream beside the backward-data chain (same arithmetic, same order
        # inside every chain -> bit-identical results with and without)
        self.side = SideStream(dev, Workspace.get(dev), lanes=4) if overlap else None
        # the iteration never clears the gradient arenas (WRITER TABLE below): once here, so that whatever an earlier user of the modules
        # left in them is gone before anybody reads `.grad`
        ops.fill_f32(ga.grad)
        ops.fill_f32(da.grad)

    # -- the hot path ---------------------------------------------------------------------------------
    # WRITER TABLE of the two gradient arenas (optimizer.zero_grad() of the reference loop, :334,353,375).  A backward pass of _GenEngine /
    # _DiscEngine has exactly ONE launch per parameter slice, and every slice has one (Arena: the parameters tile it, no padding):
    #
    #   slice                                  writer (launch)                                   stream, pipelined body (SideStream.defer index)
    #   G conv_blocks.10.weight / .bias        wgrad_reduce / act_grad_mul_bias_nchw             chain G4, lane 0 (bias: main stream without conv_img_mfma)
    #   G conv_blocks.{7,4,1}.weight / .bias   wgrad_reduce / bias_grad                          chains G3,G2,G1, lanes 3,2,1: both on the layer's chain
    #   G conv_blocks.{8,5,2}.weight / .bias   bn_bwd_fused | bn_bwd | bn_bwd_sums_local         main stream
    #   G conv_blocks.0.weight / .bias         wgrad_reduce / bias_grad                          chain G0, lane 0
    #   D main.8.weight / .bias                wgrad_reduce / dense_small_bgrad                  chain D4, lane 0
    #   D main.{6,4,2,0}.weight_orig / .bias   wgrad_reduce_rank1 / bias_grad_sn[_fused]         chains D3..D0, lanes 4,3,2,1: both on the layer's chain
    #
    #   pass                      G arena                                        D arena
    #   step 1 (G adversarial)    every slice: first and only writer -> STORE    no writer (need_wgrad=False) and no reader: untouched
    #   step 2 (D)                no writer, no reader: untouched                every slice: first and only writer -> STORE
    #   step 3 (info + affine)    every slice: first and only writer -> STORE    every slice: first and only writer -> STORE
    #
    # No slice has a second writer behind the first (nothing keeps accumulate), none collects contributions from lanes that are not ordered
    # against each other (the three tapes of step 3 are batched into one GEMM and one reduction per layer), and the only slices without a
    # writer in a pass -- D's in step 1, G's in step 2 -- have no reader in it either (no all-reduce, no Adam): they keep the gradients of
    # the last pass that wrote them, as the reference's do between zero_grad() calls of the OTHER optimizer.  So the iteration has no
    # arena fill at all and no Adam launch clears its gradients.
    # Hazards a store must respect are those the read-modify-write had: a writer of pass k+1 runs behind the Adam launch (and, data
    # parallel, the all-reduce) that read the slice in pass k -- step 3's generator forward waits for evs["g"], its discriminator forward
    # joins every lane, and the iteration ends with a join.  The gradients of step 3 stay in place afterwards: callers and tests read them.
    #
    # READERS OF ge.img (the generated image; one buffer, written by the last launch of every generator forward).  With the layer-0 weight
    # gradient of D read from the images themselves (_DiscEngine.wgrad_tn; before, from patch rows copied on the preparation lane) a lane
    # chain reads it:
    #
    #   writer                         readers before the next writer                                   ordered by
    #   step 1 forward (main)          step 1 D forward / G backward (main), step 2 D forward (main)    program order of the main stream
    #                                  step 2 chain D0 (lane): wgrad_img_tn, tape 1                     step 3's LAST generator launch waits for
    #                                                                                                   the chain's done event (evs["d0"]); the
    #                                                                                                   layers above it do not wait
    #   step 3 forward (main)          step 3 D forward / G backward (main), step 3 chain D0 (lane)     the join that ends the iteration
    #
    # self.scaled and self.real are rewritten by the next iteration's preparation lane, behind that join.
    def _buckets(self, arena):
        """(tag, lo, hi) element ranges of `arena` per layer bucket, in completion order; the ranges tile the arena"""
        eng = self.ge if arena is self.G.arena else self.de
        out, covered = [], 0
        for tag, names in eng.BUCKETS:
            offs = [arena.slices[n] for n in names]
            lo, hi = min(o for o, _ in offs), max(o + k for o, k in offs)
            assert sum(k for _, k in offs) == hi - lo, (tag, "bucket parameters are not contiguous in the arena")
            out.append((tag, lo, hi))
            covered += hi - lo
        assert covered == arena.numel, "buckets do not tile the arena"
        return out

    def _adam(self, arena, m, v, lr, slot, tick):
        """optimizer.step() of one network + refresh of its packed panels (serial body)"""
        eng = self.ge if arena is self.G.arena else self.de
        if not FUSE_ADAM:
            ops.adam_step(arena.flat, arena.grad, m, v, arena.numel, lr, self.betas[0], self.betas[1], 1e-8, self.steps[slot:slot + 1], tick)
            eng.repack()
            return
        if tick:
            ops.adam_tick(self.steps[slot:slot + 1])
        for tag, lo, hi in self._buckets(arena):
            adam_bucket(eng, arena, tag, lo, hi, m, v, lr, self.betas, self.steps[slot:slot + 1])

    def _pre_backward(self, k):
        if self.before_backward is not None:
            self.before_backward(k)

    def _step_body(self):
        if self.side is not None:
            return self._step_body_pipelined()
        return self._step_body_serial()

    def _inputs_head(self):
        G, B = self.G, self.B
        # A = get_matrix(code[:, :5]); scaled = trans_2D(real, A[:, 0:2])           (:325-327)
        if engine.FUSE_DRAWS and (G.img_size * G.img_size) % 256 == 0:
            ops.warp_affine_rpqxy(self.real, self.code, G.code_dim, self.theta, self.scaled, B, G.channels, G.img_size, G.img_size, zero=self.losses)
            return
        ops.fill_f32(self.losses)
        ops.theta_rpqxy(self.code, G.code_dim, B, self.theta)
        ops.warp_affine(self.real, self.theta, self.scaled, B, G.channels, G.img_size, G.img_size)

    def _reduce(self, flat):
        """gradient average over the ranks, on the CURRENT stream (the optimizer lane: only that lane waits for the collective)"""
        engine.allreduce_finish(self.allreduce, flat, engine.allreduce_start(self.allreduce, flat))

    def _step_body_serial(self):
        """one stream, program order of the reference loop body (overlap=False; the pipelined body below is bit-identical)"""
        G, D, ge, de, B = self.G, self.D, self.ge, self.de, self.B
        ga, da = G.arena, D.arena
        cd, nc = G.code_dim, G.n_classes
        lcat, lcon, laff = self.lam
        fh1 = de.head_fused_ok(2)                        # head + losses + head backward in one launch (steps 1 and 2)
        fh3 = de.head_fused_ok(3) and cd >= 5            # ... of the info step
        self._inputs_head()
        # ---- 1) generator adversarial step (:334-345) ----
        gen = ge.forward(self.z, self.onehot, self.code, sync=self.sync_bn)
        out = de.forward([gen], 2, head=not fh1)
        if fh1:
            de.head_losses(2, 1, self.dout[2 * B:], self.losses[0:1], targets=(1.0,), scales=(1.0,))
        else:
            ops.loss_bce_sigmoid(out, 19, 0, B, 1.0, 1.0, self.losses[0:1], self.dout[2 * B:])
        self._pre_backward(1)
        dimg = de.backward(2, 1, self.dout[2 * B:], da.grad, need_wgrad=False, need_dimg=True, head_done=fh1)
        ge.backward(dimg, ga.grad, None, sync=self.sync_bn, store=True)
        self._reduce(ga.grad)
        self._adam(ga, self.mG, self.vG, self.lr[0], 0, True)
        # ---- 2) discriminator step (:353-366); gen is the (detached) output of step 1; D(scaled) then D(gen), batched ----
        out = de.forward([self.scaled, gen], 0, head=not fh1)
        if fh1:
            de.head_losses(0, 2, self.dout[:2 * B], self.losses[1:2], targets=(1.0, 0.0), scales=(0.5, 0.5))
        else:
            ops.loss_bce_sigmoid(out[:B], 19, 0, B, 1.0, 0.5, self.losses[1:2], self.dout[:B])
            ops.loss_bce_sigmoid(out[B:], 19, 0, B, 0.0, 0.5, self.losses[1:2], self.dout[B:2 * B])
        self._pre_backward(2)
        de.backward(0, 2, self.dout[:2 * B], da.grad, head_done=fh1, store=True)
        self._reduce(da.grad)
        self._adam(da, self.mD, self.vD, self.lr[1], 1, True)
        # ---- 3) info + affine step (:375-401): D(gen), D(scaled), D(real) batched as tapes 0,1,2 ----
        gen = ge.forward(self.z, self.onehot, self.code, sync=self.sync_bn)
        out = de.forward([gen, self.scaled, self.real], 0, head=not fh3)
        if fh3:
            de.head_losses(0, 3, self.dout, self.losses[2:3], info=(1, cd, nc, self.code, self.labels, lcat, lcon, laff))
        else:
            o_gen, o_trans, o_real = out[:B], out[B:2 * B], out[2 * B:]
            ops.loss_mse(o_gen, 19, 1, cd, B, self.code, cd, 0.0, lcon, self.losses[2:3], self.dout[:B])
            ops.loss_ce_softmaxed(o_gen, 19, cd + 1, nc, B, self.labels, lcat, self.losses[2:3], self.dout[:B])
            ops.loss_affine_rpqxy(o_real, o_trans, 19, 1, B, self.code, cd, laff, self.losses[2:3], self.dout[2 * B:], self.dout[B:2 * B])
        self._pre_backward(3)
        dimg = de.backward(0, 3, self.dout, da.grad, need_dimg=True, head_done=fh3, store=True)
        ge.backward(dimg, ga.grad, None, sync=self.sync_bn, store=True)
        self._reduce(da.grad)
        self._reduce(ga.grad)
        self._adam(da, self.miD, self.viD, self.lr[2], 2, True)     # optimizer_info's step counter is shared by both arenas
        self._adam(ga, self.miG, self.viG, self.lr[2], 2, False)

    def _step_body_pipelined(self):
        """The same iteration on five streams.  Main stream: the forward / backward-data chain of the three sub-steps, back to back.
        Lanes 0,1: weight-gradient GEMMs with their reductions.  Preparation lane: the next sub-step's power iterations (and patch
        rows, where the layer-0 weight gradient still reads them).  Optimizer lane:
        per network, behind ALL of its weight-gradient chains: (all-reduce over the ranks ->) Adam -> re-packing.  No gradient is cleared:
        every backward pass stores (WRITER TABLE above).
        The main stream never waits for an optimizer update it does not need: step 2 neither reads nor writes G, step 3 starts with
        the generator forward, which does not read D; it waits for single events (``mark`` / ``wait``) instead of joining every lane."""
        G, D, ge, de, B = self.G, self.D, self.ge, self.de, self.B
        ga, da = G.arena, D.arena
        cd, nc = G.code_dim, G.n_classes
        lcat, lcon, laff = self.lam
        side = self.side
        evs = {}
        fh1 = de.head_fused_ok(2)                        # head + losses + head backward in one launch (steps 1 and 2)
        fh3 = de.head_fused_ok(3) and cd >= 5            # ... of the info step

        ar = self.allreduce
        ar_async = ar is not None and hasattr(ar, "start")

        def update(arena, m, v, lr, slot, tick, eng, key=None, key_w=None, bucketed=False):
            """Queue one network's optimizer update on the optimizer lane.  Default: the whole arena in one update behind ALL of its weight-
            gradient chains (engine.SideStream.defer_opt).  ``bucketed`` (the info step's generator update, the last of the iteration,
            profiles/r02_h_ab_bucket_opt.txt): bucket by bucket in the order the backward pass completes them -- a bucket's Adam
            and panel re-packing wait only for the lane chain that completes the bucket's gradients and for the
            main-stream kernels that still read its parameters (engine.SideStream.free), so the update of the upper layers runs beside the
            backward pass of the lower ones and only the last bucket's update is behind all of it.
            Data parallel: each bucket's all-reduce is STARTED once its chain is done (RCCL's stream must only ever wait for the capture's
            origin stream: a lane that RCCL waited for and that later waits for RCCL is the stream-level back edge hipStreamEndCapture
            crashes on), and FINISHED on the optimizer lane, so the main stream waits neither for the collective nor for Adam / re-packing."""
            side.close_tags()
            buckets = self._buckets(arena)
            hs, finished = {}, set()

            def finish(tag):
                h = hs.get(tag)
                if h is not None and id(h) not in finished:
                    finished.add(id(h))
                    ar.finish(h)
            if ar is not None:
                if ar_async and not torch.cuda.is_current_stream_capturing():
                    # eager launches (the default at N > 1): the gradient arena crosses the links as TWO messages per update (COMM_GROUPS:
                    # the layers whose gradients are complete early / the rest -- every collective costs the host ~40 us and a ring its
                    # latency, five per update bought nothing), each started behind the lane chains that complete it and finished on the
                    # optimizer lane: the main stream waits for neither
                    span = {tag: (lo, hi) for tag, lo, hi in buckets}
                    for grp in COMM_GROUPS["G" if arena is ga else "D"]:
                        # started from the lane that ran the group's last chain (no further stream: eight busy streams on four hardware
                        # queues stall each other)
                        src = side.done_lane[grp[-1]].stream
                        for tag in grp:
                            src.wait_event(side.done.pop(tag))              # KeyError: a bucket whose chain was never forked
                        lo, hi = min(span[t][0] for t in grp), max(span[t][1] for t in grp)
                        assert sum(span[t][1] - span[t][0] for t in grp) == hi - lo, "a communication group must be contiguous in the arena"
                        with torch.cuda.stream(src):
                            h = ar.start(arena.grad[lo:hi])
                            started = side.mark()
                        side.opt.stream.wait_event(started)                 # (the collective's own handle orders the optimizer lane behind it too)
                        for tag in grp:
                            hs[tag] = h                 # whichever bucket of the group is updated first finishes the message
                    buckets_ar = ()
                else:
                    buckets_ar = buckets
                for tag, lo, hi in buckets_ar:
                    done = side.done.pop(tag)           # KeyError: a bucket whose chain was never forked
                    # inside a hipGraph capture RCCL's stream may only ever wait for the capture's origin stream (a lane that RCCL waited
                    # for and that later waits for RCCL is the stream-level back edge hipStreamEndCapture crashes on): started from the
                    # main stream, which therefore waits for the bucket's chain
                    side.wait(done)
                    if ar_async:
                        hs[tag] = ar.start(arena.grad[lo:hi])
                    else:
                        ar(arena.grad[lo:hi])
            if not bucketed:
                def whole(_ws):
                    for tag in hs:
                        finish(tag)
                    ops.adam_step_zero(arena.flat, arena.grad, m, v, arena.numel, lr, self.betas[0], self.betas[1], 1e-8, self.steps[slot:slot + 1],
                                       tick, False)
                    if key_w:
                        evs[key_w] = side.mark()        # master weights are new
                    eng.repack()
                    if key:
                        evs[key] = side.mark()          # panels are new, the gradients have been read
                side.done.clear()
                side.free.clear()
                side.defer_opt(whole)
                return
            last = buckets[-1][0]
            for k, (tag, lo, hi) in enumerate(buckets):
                def fn(_ws, tag=tag, lo=lo, hi=hi, first=(k == 0)):
                    finish(tag)
                    if FUSE_ADAM:
                        if tick and first:
                            ops.adam_tick(self.steps[slot:slot + 1])
                        adam_bucket(eng, arena, tag, lo, hi, m, v, lr, self.betas, self.steps[slot:slot + 1])
                        if key_w and tag == last:
                            evs[key_w] = side.mark()    # master weights are new
                    else:
                        ops.adam_step_zero(arena.flat[lo:hi], arena.grad[lo:hi], m[lo:hi], v[lo:hi], hi - lo, lr, self.betas[0], self.betas[1], 1e-8,
                                           self.steps[slot:slot + 1], tick and first, False)
                        if key_w and tag == last:
                            evs[key_w] = side.mark()    # master weights are new
                        eng.repack_bucket(tag)
                    if key and tag == last:
                        evs[key] = side.mark()          # panels are new, the gradients have been read
                side.defer_opt_after((tag,), fn)

        # the generator forward needs the draws only: the image gather (DeviceInputs) and the warp go to the preparation lane, in front of
        # step 1's power iteration -- everything that reads them (step 2, step 3, the losses the warp launch zeroes) is behind the wait
        # for that lane's event below
        tail, self._inputs_tail = getattr(self, "_inputs_tail", None), None
        # ---- 1) generator adversarial step (:334-345); D(gen) lives in tape slot 2 so that step 2's tapes can be prepared meanwhile ----

        def sn1(_ws):                                   # the power iterations only need D's weights: beside the generator forward
            if tail is not None:
                tail()
            self._inputs_head()
            de._sn_tape(2)
            evs["sn1"] = side.mark()
        side.defer_prep(sn1)
        gen = ge.forward(self.z, self.onehot, self.code, sync=self.sync_bn)
        side.wait(evs["sn1"])
        out = de.forward([gen], 2, prepared=(False,), head=not fh1)

        def prep2(_ws):                                 # step 2's power iterations (after step 1's in the u/v chain) and patch rows
            de.prepare(0, [self.scaled, gen])
            evs["prep2"] = side.mark()
        side.defer_prep(prep2)
        if fh1:
            de.head_losses(2, 1, self.dout[2 * B:], self.losses[0:1], targets=(1.0,), scales=(1.0,))
        else:
            ops.loss_bce_sigmoid(out, 19, 0, B, 1.0, 1.0, self.losses[0:1], self.dout[2 * B:])
        self._pre_backward(1)
        dimg = de.backward(2, 1, self.dout[2 * B:], da.grad, need_wgrad=False, need_dimg=True, head_done=fh1)
        ge.backward(dimg, ga.grad, side, sync=self.sync_bn, store=True)
        update(ga, self.mG, self.vG, self.lr[0], 0, True, ge, key="g")                # beside the whole of step 2
        # ---- 2) discriminator step (:353-366); gen is the (detached) output of step 1; D(scaled) then D(gen), batched ----
        side.wait(evs["prep2"])
        out = de.forward([self.scaled, gen], 0, prepared=(True, True), head=not fh1)
        if fh1:
            de.head_losses(0, 2, self.dout[:2 * B], self.losses[1:2], targets=(1.0, 0.0), scales=(0.5, 0.5))
        else:
            ops.loss_bce_sigmoid(out[:B], 19, 0, B, 1.0, 0.5, self.losses[1:2], self.dout[:B])
            ops.loss_bce_sigmoid(out[B:], 19, 0, B, 0.0, 0.5, self.losses[1:2], self.dout[B:2 * B])
        if self.before_backward is not None:
            side.wait(evs["g"])                         # test hook only (see __init__): step 1's generator update still reads G's gradients
        self._pre_backward(2)
        de.backward(0, 2, self.dout[:2 * B], da.grad, side=side, head_done=fh1, store=True)
        evs["d0"] = side.done.get("D0") if de.wgrad_tn else None                      # the chain that reads `gen` itself (READERS OF ge.img)
        update(da, self.mD, self.vD, self.lr[1], 1, True, de, key_w="dw")             # beside step 3's generator forward

        # the first layer reads the images themselves (ops.conv_img_mfma): the patch rows are only the weight gradient's operand and are built by
        # its own chain in step 3's backward -- not here, on the chain step 3's discriminator forward waits for
        lazy = de.img_direct

        def prep3(_ws):                                 # step 3's three power iterations (new weights) [, patch rows of scaled / real]
            side.wait(evs["dw"])
            de.prepare(0, [None, None, None] if lazy else [None, self.scaled, self.real])
        side.defer_prep(prep3)
        # ---- 3) info + affine step (:375-401): D(gen), D(scaled), D(real) batched as tapes 0,1,2 ----
        side.wait(evs["g"])                             # G's panels; its gradients have been read (optimizer lane, step 1): step 3 may store
        gen = ge.forward(self.z, self.onehot, self.code, sync=self.sync_bn, img_after=evs["d0"])
        side.join()                                     # D's panels, power iterations, patch rows
        out = de.forward([gen, self.scaled, self.real], 0, prepared=(False, False, False) if lazy else (False, True, True), head=not fh3)
        if fh3:
            de.head_losses(0, 3, self.dout, self.losses[2:3], info=(1, cd, nc, self.code, self.labels, lcat, lcon, laff))
        else:
            o_gen, o_trans, o_real = out[:B], out[B:2 * B], out[2 * B:]
            ops.loss_info_rpqxy(o_gen, o_trans, o_real, 19, 1, cd, nc, B, self.code, cd, self.labels, lcat, lcon, laff, self.losses[2:3], self.dout[:B],
                                self.dout[B:2 * B], self.dout[2 * B:])           # the three losses in one launch
        self._pre_backward(3)
        dimg = de.backward(0, 3, self.dout, da.grad, need_dimg=True, side=side, head_done=fh3, store=True)
        # D's update beside the generator backward; it ticks optimizer_info's counter (shared by both arenas), G's does not
        update(da, self.miD, self.viD, self.lr[2], 2, True, de)
        ge.backward(dimg, ga.grad, side, sync=self.sync_bn, store=True)
        update(ga, self.miG, self.viG, self.lr[2], 2, False, ge, bucketed=True)
        side.join()

    # -- public API -----------------------------------------------------------------------------------
    def import_adam_state(self, opt_G, opt_D, opt_info):
        """Load exp_avg / exp_avg_sq / step of three ``torch.optim.Adam`` objects built like the reference's
        (celebA/EAD-GAN_celebA.py:211-217: G params | D params | G+D params, in ``.parameters()`` order)."""
        nG, nD = len(list(self.G.parameters())), len(list(self.D.parameters()))
        s0 = import_adam_moments(opt_G, [(nG, self.mG, self.vG)])
        s1 = import_adam_moments(opt_D, [(nD, self.mD, self.vD)])
        s2 = import_adam_moments(opt_info, [(nG, self.miG, self.viG), (nD, self.miD, self.viD)])
        self.steps.copy_(torch.tensor([s0, s1, s2], dtype=torch.int32))

    def load_inputs(self, real_imgs, z, code, labels):
        self.real.copy_(real_imgs, non_blocking=True)
        self.z.copy_(z, non_blocking=True)
        self.code.copy_(code, non_blocking=True)
        self.labels.copy_(labels, non_blocking=True)
        self.onehot.zero_()
        self.onehot.scatter_(1, self.labels.view(-1, 1), 1.0)

    def capture(self, warmup: bool = False, inputs: "DeviceInputs | None" = None, log=None):
        """Capture the whole iteration into one hipGraph (inputs are read from the static slots; with ``inputs`` -- a DeviceInputs --
        the graph first draws them on the device, so a replay is a complete loop iteration without host work; with ``log`` -- an
        engine.LossLog -- the graph ends with the append of the iteration's loss row).

        At least one eager iteration must have run before (it loads every kernel and sizes the workspace);
        ``warmup=True`` runs that iteration here -- note that it IS a real training step on the current inputs.

        Gradients: an iteration never clears the gradient arenas (every backward pass stores), so ``capture(warmup=False)`` clears them
        once, outside the graph -- the gradients a previous eager iteration left in ``.grad`` are gone after this call; read them before
        capturing.  With ``warmup=True`` nothing is cleared: the arenas hold the warm-up iteration's gradients, as after any iteration."""
        if not warmup:
            # a replay clears nothing (WRITER TABLE): the arenas enter the graph's first replay cleared, as they enter the first eager iteration
            ops.fill_f32(self.G.arena.grad)
            ops.fill_f32(self.D.arena.grad)
        return super().capture(warmup, inputs, log)

    # -- full state (engine.TrainerState) -------------------------------------------------------------
    STATE_KIND = "celeba"

    def _state_modules(self):
        return {"G": self.G, "D": self.D}

    def _state_moments(self):
        return {"G": (self.mG, self.vG), "D": (self.mD, self.vD), "iG": (self.miG, self.viG), "iD": (self.miD, self.viD)}

    def _state_zero_scratch(self):
        # scratch whose contract is "left at zero" by every launch that uses it: arrival counters of the fused head.  Zero at every
        # iteration boundary already; cleared so that a load never depends on that.
        if self.de._head_scratch is not None:
            self.de._head_scratch[1].zero_()

    # step_resident() (engine.ResidentStep): one iteration on whatever is in the static input slots (or on fresh device-side draws if the
    # trainer was captured / configured with a DeviceInputs); returns the device loss tensor [g,d,info,_]

    def train_step(self, real_imgs, z, code, labels):
        """train-loop entry: real_imgs [B,3,64,64] in [-1,1], z [B,200], code [B,8], labels int64 [B]."""
        self.load_inputs(real_imgs, z, code, labels)
        l = self.step_resident().tolist()
        return {"g_loss": l[0], "d_loss": l[1], "info_loss": l[2]}

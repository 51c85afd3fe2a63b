"""dSprites 64x64 stage-2 path of EAD-GAN on MI355X: drop-in ``Encoder_pxy`` / ``Discriminator`` / ``Generator`` / ``Encoder`` /
``transformation_2D`` / ``mutual_info_loss`` / ``to_categorical`` (dSprites/rp.py:61-232), ``get_matrix`` / ``get_matrix_D`` /
``affine_regularzier`` (dSprites/utils_rp.py), ``get_matrix_pxy_align`` (dSprites/utils_pxy.py:69-87) and the fused train-loop
entry :class:`DspritesTrainer` (loop body rp.py:365-482).  torch modules are parameter containers only.
"""
from __future__ import annotations

import argparse
import itertools

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable
from torch.nn.utils import spectral_norm

from . import affine, engine, ops
from .affine import _code_to_theta, theta_to_matrix, transformation_2D      # noqa: F401
from .engine import (Arena, ConvRec, DeviceSampler, InputGrad, ResidentStep, SideStream, SyncScratch, Workspace, _HipModule, _require_cuda, bn_bwd_epilogue,
                     bn_train_backward, bn_train_forward, convt_img, drop_in_backward, import_adam_moments, parse_dtype, stat_buffer, to_categorical,
                     wants_input_grad, wgrad_side)      # noqa: F401
from .ops import ACT_LRELU, ACT_RELU, ACT_SIGMOID, EG_F32
from .trunk import Head, TrunkEngine, _TrunkFn

opt = argparse.Namespace(n_epochs=100, batch_size=128, lr=0.0001, b1=0.5, b2=0.999, n_cpu=8, latent_dim=200, code_dim=4, n_classes=3,
                         img_size=64, channels=1, sample_interval=1000)           # argparse defaults rp.py:40-51
TRUNK = (32, 32, 64, 64)
# The generator's last-layer backward straight from the image gradient -- eg_wgrad_img (N = 64) for the weight
# gradient, eg_conv_img_mfma (N = 64) with the BatchNorm-backward sums in its epilogue for the input gradient -- instead of patch rows + the
# two GEMMs over them.  Same results within fp32 summation order (tests), one launch fewer, but SLOWER in the step: dSprites 1.305 -> 1.32 ms,
# colored 2.50 -> 2.53 (profiles/r03_zzo_ab_l4_direct.txt): the statistics instantiation of the image kernel runs two workgroups per CU.
# So no engine takes it by itself (``_GenEngine.l4_direct`` starts False); the layer-wise tests set the attribute to check this form of the layer too.


def _trunk(ch, sn, slope):
    f = spectral_norm if sn else (lambda m: m)
    return nn.Sequential(f(nn.Conv2d(ch, 32, 4, 2, 1)), nn.LeakyReLU(slope, inplace=True), f(nn.Conv2d(32, 32, 4, 2, 1)), nn.LeakyReLU(slope, inplace=True),
                         f(nn.Conv2d(32, 64, 4, 2, 1)), nn.LeakyReLU(slope, inplace=True), f(nn.Conv2d(64, 64, 4, 2, 1)), nn.LeakyReLU(slope, inplace=True))


# ================================================================================================
# Encoder_pxy: frozen alignment encoder (forward only; its gradients are dead work in the reference)
# ================================================================================================
class _PxyEngine:
    def __init__(self, mod: "Encoder_pxy", B, dtype):
        self.mod, self.B, self.dtype = mod, B, dtype
        dev = next(mod.parameters()).device
        tdt = ops.torch_dtype(dtype)
        self.ws = ws = Workspace.get(dev)
        C, S = mod.channels, mod.img_size
        self.C, self.S = C, S
        self.k0 = C * 16
        self.kp = ops.round_up(self.k0, 8)
        self.l0 = ConvRec(dtype, B, S // 2, S // 2, self.kp, TRUNK[0], 1, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.mid = [ConvRec(dtype, B, S >> (i + 1), S >> (i + 1), TRUNK[i], TRUNK[i + 1], 4, 2, 1, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
                    for i in range(3)]
        self.nout = mod.fc1.weight.shape[0]
        self.head = ConvRec(dtype, B, 4, 4, TRUNK[3], self.nout, 4, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.patches = torch.zeros(B * (S // 2) ** 2, self.kp, device=dev, dtype=tdt)
        self.a = [torch.empty(B, S >> (i + 1), S >> (i + 1), TRUNK[i], device=dev, dtype=tdt) for i in range(4)]
        self.out = torch.empty(B, self.nout, device=dev, dtype=torch.float32)
        self.repack()

    @ops.batched_packs
    def repack(self):
        cb = self.mod.conv_block
        ops.pack_strided(self.dtype, cb[0].weight, self.l0.wp_fwd, TRUNK[0], self.k0, self.l0.Kpad_fwd, 1, self.k0, 0, 1)
        for i in range(3):
            self.mid[i].pack(cb[2 * (i + 1)].weight)
        self.head.pack(self.mod.fc1.weight)          # Linear over the NCHW-flattened 4x4x64 map == 4x4 conv

    def forward(self, img):
        dt, B, cb = self.dtype, self.B, self.mod.conv_block
        ep0 = ops.epilogue(bias=cb[0].bias, act=ACT_LRELU, slope=0.1)
        if self.l0.Kpad_fwd == 64 and ops.conv_img_mfma_ok(dt, self.C, self.S, self.S, TRUNK[0], 4, 2, 1):
            ops.conv_img_mfma(dt, [img], self.l0.wp_fwd, self.a[0], B, self.C, self.S, self.S, ep0, N=TRUNK[0])      # no patch rows (frozen: no weight gradient)
        else:
            ops.im2col_img(dt, img, self.patches, B, self.C, self.S, self.S, 4, 2, 1, self.kp)
            ops.conv_fwd(self.l0.c, dt, self.patches, self.l0.wp_fwd, self.a[0], ep0)
        for i in range(3):
            ops.conv_fwd(self.mid[i].c, dt, self.a[i], self.mid[i].wp_fwd, self.a[i + 1], ops.epilogue(bias=cb[2 * (i + 1)].bias, act=ACT_LRELU, slope=0.1))
        ops.dense_small_fwd(dt, self.a[3], self.head.wp_fwd, self.mod.fc1.bias, self.out, B, 16 * TRUNK[3], self.head.Kpad_fwd, self.nout, self.ws.small)
        return self.out


class Encoder_pxy(_HipModule):
    """Drop-in for rp.py:61-87 (inference only on this path: the reference loads ``encoder_pxy_50000.pt`` and freezes it)."""

    def __init__(self, img_size=None, channels=None, n_out=3, dtype="f32"):
        super().__init__()
        g = lambda v, name: getattr(opt, name) if v is None else v
        self.img_size, self.channels = g(img_size, "img_size"), g(channels, "channels")
        self.conv_block = _trunk(self.channels, False, 0.1)
        self.fc1 = nn.Linear(1024, n_out)
        self._init_engine_state(dtype)

    @property
    def arena(self):                 # frozen: parameters stay where they are, no gradient arena
        return None

    def engine(self, B) -> _PxyEngine:
        key = (B, self.compute_dtype)
        if key not in self._engines:
            _require_cuda(next(self.parameters()))
            self._engines[key] = _PxyEngine(self, B, self.compute_dtype)
        return self._engines[key]

    def forward(self, img):
        _require_cuda(img)
        return self.fresh_engine(img.shape[0]).forward(img.float().contiguous()).clone()


# ================================================================================================
# Discriminator / Encoder (spectrally-normalised trunks with hidden FC layers)
# ================================================================================================
class _TrunkModule(_HipModule):
    NT = 3

    def _convs(self):
        cb = self.conv_block
        return [cb[i] for i in (0, 2, 4, 6)], [f"conv_block.{i}" for i in (0, 2, 4, 6)]

    def engine(self, B, slot=0) -> TrunkEngine:
        self.arena
        key = (B, self.compute_dtype) if slot == 0 else (B, self.compute_dtype, slot)
        if key not in self._engines:
            convs, names = self._convs()
            fcs, fnames = self._fcs()
            self._engines[key] = TrunkEngine(self, convs, names, [None] * 4, [None] * 4, self._heads(), self.channels, self.img_size, 4, 0.2, B,
                                             self.compute_dtype, self.NT, fcs=fcs, fc_names=fnames)
        return self._engines[key]


class Discriminator(_TrunkModule):
    """Drop-in for rp.py:90-119: SN trunk -> SN-Linear(1024,128)+LeakyReLU -> Linear(128,1) -> sigmoid."""

    def __init__(self, img_size=None, channels=None, dtype="f32"):
        super().__init__()
        g = lambda v, name: getattr(opt, name) if v is None else v
        self.img_size, self.channels = g(img_size, "img_size"), g(channels, "channels")
        self.conv_block = _trunk(self.channels, True, 0.2)
        self.fc1 = nn.Sequential(spectral_norm(nn.Linear(1024, 128)), nn.LeakyReLU(0.2, inplace=True))
        self.fc2 = nn.Linear(128, 1)
        self._init_engine_state(dtype)
        self._next_tape = 0

    def _fcs(self):
        return [self.fc1[0]], ["fc1.0"]

    def _heads(self):
        return [Head("fc2", self.fc2, sn=False)]

    def forward(self, img):
        _require_cuda(img)
        eng = self.fresh_engine(img.shape[0])
        t = self._next_tape
        self._next_tape = (t + 1) % self.NT
        (logit,) = _TrunkFn.apply(eng, t, self.training, ("fc2",), img.float().contiguous(), *list(self.parameters()))
        return torch.sigmoid(logit)


class Encoder(_TrunkModule):
    """Drop-in for rp.py:160-194: SN trunk -> 2 x (SN-Linear + LeakyReLU) -> softmax(SN-Linear(128,n_classes)), SN-Linear(128,code_dim)."""

    def __init__(self, code_dim=None, n_classes=None, img_size=None, channels=None, dtype="f32"):
        super().__init__()
        g = lambda v, name: getattr(opt, name) if v is None else v
        self.code_dim, self.n_classes = g(code_dim, "code_dim"), g(n_classes, "n_classes")
        self.img_size, self.channels = g(img_size, "img_size"), g(channels, "channels")
        self.conv_block = _trunk(self.channels, True, 0.2)
        self.fc1 = nn.Sequential(spectral_norm(nn.Linear(1024, 128)), nn.LeakyReLU(0.2, inplace=True))
        self.fc2 = nn.Sequential(spectral_norm(nn.Linear(128, 128)), nn.LeakyReLU(0.2, inplace=True))
        self.cat_layer = nn.Sequential(spectral_norm(nn.Linear(128, self.n_classes)), nn.Softmax(dim=1))
        self.cont_layer = nn.Sequential(spectral_norm(nn.Linear(128, self.code_dim)))
        self._init_engine_state(dtype)
        self._next_tape = 0

    def _fcs(self):
        return [self.fc1[0], self.fc2[0]], ["fc1.0", "fc2.0"]

    def _heads(self):
        return [Head("cat_layer.0", self.cat_layer[0], sn=True), Head("cont_layer.0", self.cont_layer[0], sn=True)]

    def forward(self, img):
        _require_cuda(img)
        eng = self.fresh_engine(img.shape[0])
        t = self._next_tape
        self._next_tape = (t + 1) % self.NT
        cat, cont = _TrunkFn.apply(eng, t, self.training, ("cat_layer.0", "cont_layer.0"), img.float().contiguous(), *list(self.parameters()))
        return torch.softmax(cat, dim=1), cont


# ================================================================================================
# Generator: Linear(7,128)+ReLU -> Linear(128,1024)+ReLU -> view[B,64,4,4] -> 3 x (ConvT 4x4 s2 + BN + ReLU) -> ConvT(64,1) -> sigmoid
# ================================================================================================
class _GenEngine:
    def __init__(self, gen: "Generator", B, dtype):
        self.gen, self.B, self.dtype = gen, B, dtype
        dev = gen.arena.flat.device
        tdt = ops.torch_dtype(dtype)
        self.ws = ws = Workspace.get(dev)
        self._stat = {}                                 # fused-statistics buffers per launch (engine.stat_buffer)
        self.cin = gen.n_classes + gen.code_dim
        self.cpad = ops.round_up(self.cin, 8)
        self.CH = gen.channels
        self.f1 = ConvRec(dtype, B, 1, 1, self.cpad, 128, 1, 1, 0, device=dev, want_bwd=False, ws=ws)
        self.f2 = ConvRec(dtype, B, 1, 1, 128, 1024, 1, 1, 0, device=dev, ws=ws)
        self.mid = [ConvRec(dtype, B, 8 << i, 8 << i, 64, 64, 4, 2, 1, device=dev, ws=ws) for i in range(3)]
        self.l4 = ConvRec(dtype, B, 64, 64, self.CH, 64, 4, 2, 1, device=dev, want_fwd=False, want_wgrad=False, ws=ws)
        self.k0 = self.CH * 16
        self.kp = ops.round_up(self.k0, 8)
        self.l4p = ConvRec(dtype, B, 32, 32, self.kp, 64, 1, 1, 0, device=dev, want_bwd=False, ws=ws)
        # forward of the last ConvTranspose2d(64 -> C) as ONE GEMM over the 32x32 lattice with N = 16 taps x C columns + the col2im gather
        # (eg_col2im_img): every activation read once instead of 16 times (engine.convt_img)
        self.l4g = ConvRec(dtype, B, 32, 32, 64, self.k0, 1, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.l4_direct = False                          # the image-direct backward of the last layer: measured slower, set by tests only (module comment)
        self.cols4 = torch.empty(B * 32 * 32, self.k0, device=dev, dtype=tdt)
        e = lambda *s, dt=tdt: torch.empty(s, device=dev, dtype=dt)
        f = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
        self.inp = e(B, self.cpad)
        self.a1 = e(B, 128)
        self.bias2_perm, self.gb2_perm = f(1024), f(1024)
        self.h = e(B, 4, 4, 64)
        self.z = [e(B, 8 << i, 8 << i, 64) for i in range(3)]
        self.a = [torch.empty_like(t) for t in self.z]
        self.mean = [f(64) for _ in range(3)]
        self.invstd = [f(64) for _ in range(3)]
        self.sync_scratch = SyncScratch((64, 64, 64), dev)
        self.img = f(B, self.CH, 64, 64)
        self.dimg_z = torch.empty_like(self.img)
        self.patches = torch.zeros(B * 32 * 32, self.kp, device=dev, dtype=tdt)
        self.da = [torch.empty_like(t) for t in self.z]
        self.dz = [torch.empty_like(t) for t in self.z]
        self.dh = torch.empty_like(self.h)
        self.dz1 = torch.empty_like(self.a1)
        for i in range(3):
            ws.need_small(ops.bn_ws_floats(B * (8 << i) ** 2, 64))
        ws.need_small(ops.bias_grad_ws_floats(B, 1024))
        ws.need_small(B * self.CH)
        ws.need_sums(128)
        # d(loss)/d(inputs) from dz1 [B][128] and the master fc1.0.weight [128][cin]: one i, j = the output feature
        self.input_grad = InputGrad(dtype, B, 1, 128, self.cin, (0, self.cin, 1), dev, 2 * 64)
        self.repack()

    def _stat_buf(self, key, c, bwd, ep, C):
        return stat_buffer(self._stat, key, c, self.dtype, bwd, ep, C, self.inp.device)

    @ops.batched_packs
    def repack(self):
        dt, g = self.dtype, self.gen
        cb = g.conv_block
        w1, w2 = g.fc1[0].weight, g.fc2[0].weight
        ops.pack_strided(dt, w1, self.f1.wp_fwd, 128, self.cin, self.f1.Kpad_fwd, 1, self.cin, 0, 1)
        # fc2 rows in NHWC order n' = hw*64 + c  <-  master row f = c*16 + hw (view [B,64,4,4])
        ops.pack_strided(dt, w2, self.f2.wp_fwd, 1024, 128, self.f2.Kpad_fwd, 64, 128, 16 * 128, 1)
        # backward panel [k][n'] = W2[f(n')][k]
        ops.pack_strided2(dt, w2, self.f2.wp_bwd, 128, 1024, ops.round_up(1024, ops.bk(dt)), 1, 1, 0, 64, 128, 16 * 128)
        ops.pack_strided(EG_F32, g.fc2[0].bias, self.bias2_perm, 1024, 1, 1, 64, 1, 16, 0)
        for i, idx in enumerate((0, 3, 6)):
            self.mid[i].pack(cb[idx].weight)
        self.l4.pack(cb[9].weight)
        ops.pack_strided(dt, cb[9].weight, self.l4p.wp_fwd, 64, self.k0, self.l4p.Kpad_fwd, 1, self.k0, 0, 1)
        ops.pack_strided(dt, cb[9].weight, self.l4g.wp_fwd, self.k0, 64, self.l4g.Kpad_fwd, self.CH, 1, 16, self.k0)     # wp[t*C + c][ci] = W[ci][c][t]

    def forward(self, labels, code, training=True, sync=None):
        """z_c = cat(one-hot labels, code)  (rp.py:404-405).  ``training=False``: running-stat BatchNorm (module.eval()).  ``sync`` (a
        dp.SyncBN): batch statistics over all ranks."""
        dt, B, g, ws = self.dtype, self.B, self.gen, self.ws
        cb = g.conv_block
        ops.concat_cast(dt, labels, code, None, self.inp, B, self.cpad)
        ops.conv_fwd(self.f1.c, dt, self.inp, self.f1.wp_fwd, self.a1, ops.epilogue(bias=g.fc1[0].bias, act=ACT_RELU))
        ops.conv_fwd(self.f2.c, dt, self.a1, self.f2.wp_fwd, self.h, ops.epilogue(bias=self.bias2_perm, act=ACT_RELU))
        x = self.h
        for i, idx in enumerate((0, 3, 6)):
            r = self.mid[i]
            bn = cb[idx + 1]
            M = B * (8 << i) ** 2
            # BatchNorm batch statistics from the transposed convolution's epilogue where it can take them: two launches instead of three
            fused = self._stat_buf(("fwd", i), r.c, True, ops.epilogue(bias=cb[idx].bias), 64) if (training and sync is None) else (0, None)
            ops.conv_bwd_data(r.c, dt, x, r.wp_bwd, self.z[i],
                              ops.epilogue(bias=cb[idx].bias, stat_mode=ops.STAT_MOMENTS if fused[0] else ops.STAT_NONE, stat_out=fused[1]))
            bn_train_forward(dt, self.z[i], self.a[i], M, 64, bn, self.mean[i], self.invstd[i], ws.small, ACT_RELU, 0.0, sync, self.sync_scratch.stats[i],
                             training, fused)
            x = self.a[i]
        # GEMM + col2im gather as ONE launch (the columns stay in LDS: same bits) where the panel's K is one 64-wide step
        convt_img(dt, x, self.l4g, self.cols4, self.l4, cb[9].bias, ACT_SIGMOID, self.img, self.l4g.Kpad_fwd == 64)
        return self.img

    def backward(self, dimg, grad, sync=None, side=None, *, dinp=None, need_wgrad=True, training=True):
        """Differentiates the LATEST forward of this engine (the activations are the engine's, one set per batch size, dtype and slot).
        ``side`` (engine.SideStream): the weight- / bias-gradient chains run on side lanes; the caller joins them before reading ``grad``.
        ``dinp`` (fp32 [B, cin]): receives d(loss)/d(z_c) after the last launch of the pass.  ``need_wgrad=False``: no weight-gradient chain
        runs and no bias / BatchNorm parameter gradient is written (``grad`` is not touched, may be None).  ``training=False``: the forward
        ran with the running statistics -- BatchNorm is elementwise (eg_bn_bwd_eval), input gradients only: combine with
        ``need_wgrad=False``.  The defaults launch what they always launched."""
        dt, B, g, ws = self.dtype, self.B, self.gen, self.ws
        assert training or not need_wgrad, "eval-mode backward yields input gradients only"
        cb = g.conv_block
        gof = lambda name: g.arena.grad_of(name, grad)
        lanes = itertools.count()
        batch_stats = training and sync is None         # the BatchNorm-backward epilogues form the training-mode dy and its sums
        pscr = self.input_grad.scratch                  # where parameter gradients land that nobody asked for
        if need_wgrad:
            ops.act_grad_mul_bias_nchw(dimg, self.img, self.dimg_z, B, self.CH, 64 * 64, ACT_SIGMOID, 0.0, ws.small, gof("conv_block.9.bias"))
        else:
            ops.act_grad_mul_bias_nchw(dimg, self.img, self.dimg_z, B, self.CH, 64 * 64, ACT_SIGMOID, 0.0, ws.small, pscr[:self.CH], accumulate=False)
        # the last layer's backward straight from the image gradient (no patch rows in HBM): weight gradient by eg_wgrad_img, input gradient by
        # eg_conv_img_mfma with the BatchNorm-backward sums of the layer below in its epilogue (as celeba._GenEngine.backward)
        direct = self.l4_direct and batch_stats
        if not direct:
            ops.im2col_img(dt, self.dimg_z, self.patches, B, self.CH, 64, 64, 4, 2, 1, self.kp)

        def l4_wgrad(wsw):
            if direct:
                ns = ops.wgrad_img(dt, [self.dimg_z], self.a[2], wsw.slab, B, self.CH, 64, 64, 64)
            else:
                ns = ops.conv_wgrad(self.l4p.c, dt, self.patches, self.a[2], wsw.slab, wsw.wgs_target)
            ops.wgrad_reduce_perm(wsw.slab, ns, 64, 64, self.kp, 1, gof("conv_block.9.weight"), 0, 0, self.k0)
        if need_wgrad:
            wgrad_side(side, ws, next(lanes), l4_wgrad)

        def bn_bwd_ep(i, c):
            """((row blocks, sums), epilogue) if the launch that produces da[i] can also form dy = da * relu'(bn(z)) and the two sums of layer
            i's BatchNorm backward (engine.bn_bwd_epilogue), else ((0, None), None)"""
            fused = self._stat_buf(("bwd", i), c, False, ops.epilogue(), 64) if batch_stats else (0, None)
            return fused, bn_bwd_epilogue(fused[1], self.z[i], self.mean[i], self.invstd[i], cb[(0, 3, 6)[i] + 1]) if fused[0] else None
        if direct:
            fused = stat_buffer(self._stat, "bwd_img", None, dt, False, None, 64, self.inp.device, nrb=lambda: ops.conv_img_mfma_stat_blocks(B, 64, 64))
            ops.conv_img_mfma(dt, [self.dimg_z], self.l4p.wp_fwd, self.da[2], B, self.CH, 64, 64,
                              bn_bwd_epilogue(fused[1], self.z[2], self.mean[2], self.invstd[2], cb[7]), N=64)
        else:
            fused, ep = bn_bwd_ep(2, self.l4p.c)
            ops.conv_fwd(self.l4p.c, dt, self.patches, self.l4p.wp_fwd, self.da[2], ep)
        for i, idx in ((2, 6), (1, 3), (0, 0)):
            r = self.mid[i]
            bn = cb[idx + 1]
            M = B * (8 << i) ** 2
            if need_wgrad:
                bn_train_backward(dt, self.z[i], self.da[i], self.dz[i], M, 64, bn, self.mean[i], self.invstd[i], ACT_RELU, 0.0,
                                  gof(f"conv_block.{idx + 1}.weight"), gof(f"conv_block.{idx + 1}.bias"), ws, sync, self.sync_scratch.sums[i], fused)
            else:
                bn_train_backward(dt, self.z[i], self.da[i], self.dz[i], M, 64, bn, self.mean[i], self.invstd[i], ACT_RELU, 0.0,
                                  pscr[:64], pscr[64:128], ws, sync, self.sync_scratch.sums[i], fused, accumulate=False, training=training)
            x_in = self.a[i - 1] if i > 0 else self.h

            def mid_wgrad(wsw, i=i, idx=idx, r=r, M=M, x_in=x_in):
                ns = ops.conv_wgrad(r.c, dt, self.dz[i], x_in, wsw.slab, wsw.wgs_target)
                ops.wgrad_reduce(wsw.slab, ns, 64, 64, 64, 16, gof(f"conv_block.{idx}.weight"))
                ops.bias_grad(dt, self.dz[i], M, 64, wsw.small, gof(f"conv_block.{idx}.bias"))
            if need_wgrad:
                wgrad_side(side, ws, next(lanes), mid_wgrad)
            if i > 0:
                fused, ep = bn_bwd_ep(i - 1, r.c)
                ops.conv_fwd(r.c, dt, self.dz[i], r.wp_fwd, self.da[i - 1], ep)
            else:                                    # into the ReLU output of fc2: mask fused into the epilogue
                ops.conv_fwd(r.c, dt, self.dz[i], r.wp_fwd, self.dh, ops.epilogue(mask=self.h, mask_act=ACT_RELU))

        # fc2: dW[f][k] = sum_b dh[b][n'(f)] a1[b][k]
        def fc2_wgrad(wsw):
            ns = ops.conv_wgrad(self.f2.c, dt, self.a1, self.dh, wsw.slab, wsw.wgs_target)
            ops.wgrad_reduce_perm(wsw.slab, ns, 1024, 1024, 128, 1, gof("fc2.0.weight"), 64, 16, 0)
            ops.fill_f32(self.gb2_perm)
            ops.bias_grad(dt, self.dh, B, 1024, wsw.small, self.gb2_perm)
            ops.gather_add(gof("fc2.0.bias"), self.gb2_perm, 1024, 16, 1, 64)
        if need_wgrad:
            wgrad_side(side, ws, next(lanes), fc2_wgrad)
        ops.conv_bwd_data(self.f2.c, dt, self.dh, self.f2.wp_bwd, self.dz1, ops.epilogue(mask=self.a1, mask_act=ACT_RELU))

        # fc1
        def fc1_wgrad(wsw):
            ns = ops.conv_wgrad(self.f1.c, dt, self.inp, self.dz1, wsw.slab, wsw.wgs_target)
            ops.wgrad_reduce_perm(wsw.slab, ns, 128, 128, self.cpad, 1, gof("fc1.0.weight"), 0, 0, self.cin)
            ops.bias_grad(dt, self.dz1, B, 128, wsw.small, gof("fc1.0.bias"))
        if need_wgrad:
            wgrad_side(side, ws, next(lanes), fc1_wgrad)
        if dinp is not None:
            self.input_grad.run(self.dz1, g.fc1[0].weight, dinp)


class Generator(_HipModule):
    """Drop-in for rp.py:123-157; ``forward(z_c)`` with z_c = cat(one-hot label, code)."""

    def __init__(self, code_dim=None, n_classes=None, channels=None, dtype="f32"):
        super().__init__()
        g = lambda v, name: getattr(opt, name) if v is None else v
        self.code_dim, self.n_classes, self.channels = g(code_dim, "code_dim"), g(n_classes, "n_classes"), g(channels, "channels")
        self.img_size = 64
        self.conv_block = nn.Sequential(
            nn.ConvTranspose2d(64, 64, 4, 2, 1), nn.BatchNorm2d(64), nn.ReLU(), nn.ConvTranspose2d(64, 64, 4, 2, 1), nn.BatchNorm2d(64), nn.ReLU(),
            nn.ConvTranspose2d(64, 64, 4, 2, 1), nn.BatchNorm2d(64), nn.ReLU(), nn.ConvTranspose2d(64, self.channels, 4, 2, 1))
        self.fc1 = nn.Sequential(nn.Linear(self.n_classes + self.code_dim, 128), nn.ReLU())
        self.fc2 = nn.Sequential(nn.Linear(128, 64 * 4 * 4), nn.ReLU())
        self._init_engine_state(dtype)

    def engine(self, B, slot=0) -> _GenEngine:
        """``slot``: independent engines of one batch size (own activations and panels): the trainer's two generator forwards of an
        iteration run on different chains"""
        self.arena
        key = (B, self.compute_dtype) if slot == 0 else (B, self.compute_dtype, slot)
        if key not in self._engines:
            self._engines[key] = _GenEngine(self, B, self.compute_dtype)
        return self._engines[key]

    def forward(self, z_c):
        _require_cuda(z_c)
        z_c = z_c.float().contiguous()
        eng = self.fresh_engine(z_c.shape[0])
        if not self.training and not wants_input_grad(z_c):
            # inference (dSprites/gen_imgs.py): running-stat BatchNorm, no autograd graph
            with torch.no_grad():
                return eng.forward(z_c[:, :self.n_classes].contiguous(), z_c[:, self.n_classes:].contiguous(), training=False).clone()
        # train mode: input and parameter gradients from one pass (batch statistics couple the samples, the gradient reflects it);
        # eval mode with a z_c that requires grad: the same eval forward, input gradients only.  autograd concatenates the gradients of
        # the two slices back into d(z_c)
        return _GenFn.apply(eng, self.training, z_c[:, :self.n_classes].contiguous(), z_c[:, self.n_classes:].contiguous(), *list(self.parameters()))


class _GenFn(torch.autograd.Function):
    """autograd bridge of the drop-in generator.  The activations live in the engine: ``backward`` differentiates the engine's LATEST
    forward, so call it before the module runs again at this batch size."""

    @staticmethod
    def forward(ctx, eng, training, labels, code, *params):
        ctx.eng, ctx.training = eng, training
        ctx.widths = (labels.shape[1], code.shape[1])
        return eng.forward(labels, code, training=training).clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, dimg):
        ins, grads = drop_in_backward(ctx.eng, dimg, ctx.needs_input_grad[2:4], ctx.needs_input_grad[4:], ctx.training, ctx.widths)
        return (None, None, *ins, *grads)


# ================================================================================================
# affine utilities / losses
# ================================================================================================
def get_matrix(code_input_raw):
    """[B,>=4] codes -> [B,3,3] = R(theta) Z(p,p) T(x,y)  (utils_rp.py:94-115)."""
    return theta_to_matrix(_code_to_theta("rp", code_input_raw))


get_matrix_D = get_matrix        # identical formulas (utils_rp.py:38-59)


def get_matrix_pxy(code_input_raw):
    """[B,>=3] codes (p, x, y) -> [B,3,3] = Z(p,p) T(x,y), p = 1 + .1 c0, x, y = .1 c1, .1 c2  (utils_pxy.py:49-66)."""
    return theta_to_matrix(_code_to_theta("pxy", code_input_raw))


def get_matrix_pxy_align(code_input_raw):
    """translation-only alignment matrix T(.1 c1, .1 c2)  (utils_pxy.py:69-87)."""
    theta = _code_to_theta("pxy_align_inv", code_input_raw)
    theta[:, :, 2] = -theta[:, :, 2]             # the kernel produces the inverse the loop actually uses (rp.py:376); autograd follows the flip
    return theta_to_matrix(theta)


_regularizer = affine.regularizer(lambda real, trans, ld, B, target, scale, d_real, d_trans, pred: ops.loss_affine_rp(
    real, trans, ld, 0, B, target, 4, scale, None, d_real, d_trans, pred), 4)


def affine_regularzier(real_code, trans_code):
    """closed-form relative-transform recovery over the first 4 codes (utils_rp.py:118-147)."""
    return _regularizer(real_code, trans_code)


def mutual_info_loss(c_given_x, c):
    """rp.py:225-232 on probabilities (eager torch ops on [B,n] tensors; the fused trainer uses eg_loss_mutual_info on logits)."""
    eps = 1e-8
    return torch.mean(-torch.sum(torch.log(c_given_x + eps) * c, dim=1)) + torch.mean(-torch.sum(torch.log(c + eps) * c, dim=1))


# ================================================================================================
# fused train-loop entry
# ================================================================================================
# ================================================================================================
# Stage-1 trainer: fits Encoder_pxy (dSprites/pxy.py), whose checkpoint the stage-2 loop loads frozen
# ================================================================================================
class _PxyTrainEngine:
    """Encoder_pxy forward + backward for two batched tapes (E(img) and E(warp(img)): plain convs, no BatchNorm, so both forwards
    share every launch).  The image and the warp matrix carry no gradient (pxy.py:166-178), so the backward ends in the first conv."""

    def __init__(self, mod: "Encoder_pxy", B, dtype, arena: Arena):
        self.mod, self.B, self.dtype, self.arena = mod, B, dtype, arena
        dev = arena.flat.device
        tdt = ops.torch_dtype(dtype)
        self.ws = ws = Workspace.get(dev)
        C, S = mod.channels, mod.img_size
        self.C, self.S = C, S
        NB = 2 * B
        self.NB = NB
        self.k0 = C * 16
        self.kp = ops.round_up(self.k0, 8)
        self.l0 = ConvRec(dtype, NB, S // 2, S // 2, self.kp, TRUNK[0], 1, 1, 0, device=dev, want_bwd=False, ws=ws)
        self.mid = [ConvRec(dtype, NB, S >> (i + 1), S >> (i + 1), TRUNK[i], TRUNK[i + 1], 4, 2, 1, device=dev, ws=ws) for i in range(3)]
        self.nout = mod.fc1.weight.shape[0]
        self.head = ConvRec(dtype, NB, 4, 4, TRUNK[3], self.nout, 4, 1, 0, device=dev, want_bwd=False, want_wgrad=False, ws=ws)
        self.patches = torch.zeros(NB * (S // 2) ** 2, self.kp, device=dev, dtype=tdt)
        self.a = [torch.empty(NB, S >> (i + 1), S >> (i + 1), TRUNK[i], device=dev, dtype=tdt) for i in range(4)]
        self.dz = [torch.empty_like(t) for t in self.a]
        self.out = torch.empty(NB, self.nout, device=dev, dtype=torch.float32)
        self.repack()

    @ops.batched_packs
    def repack(self):
        cb = self.mod.conv_block
        ops.pack_strided(self.dtype, cb[0].weight, self.l0.wp_fwd, TRUNK[0], self.k0, self.l0.Kpad_fwd, 1, self.k0, 0, 1)
        for i in range(3):
            self.mid[i].pack(cb[2 * (i + 1)].weight)
        self.head.pack(self.mod.fc1.weight)

    def forward(self, img, trans_img):
        """-> codes [2B, n_out] fp32: rows [:B] of ``img``, rows [B:] of ``trans_img``"""
        dt, B, cb = self.dtype, self.B, self.mod.conv_block
        npix = B * (self.S // 2) ** 2
        ops.im2col_img(dt, img, self.patches[:npix], B, self.C, self.S, self.S, 4, 2, 1, self.kp)
        ops.im2col_img(dt, trans_img, self.patches[npix:], B, self.C, self.S, self.S, 4, 2, 1, self.kp)
        ops.conv_fwd(self.l0.c, dt, self.patches, self.l0.wp_fwd, self.a[0], ops.epilogue(bias=cb[0].bias, act=ACT_LRELU, slope=0.1))
        for i in range(3):
            ops.conv_fwd(self.mid[i].c, dt, self.a[i], self.mid[i].wp_fwd, self.a[i + 1], ops.epilogue(bias=cb[2 * (i + 1)].bias, act=ACT_LRELU, slope=0.1))
        ops.dense_small_fwd(dt, self.a[3], self.head.wp_fwd, self.mod.fc1.bias, self.out, self.NB, 16 * TRUNK[3], self.head.Kpad_fwd, self.nout, self.ws.small)
        return self.out

    def backward(self, dout, grad):
        """dout: d(loss)/d(codes) [2B, n_out] fp32; accumulates into the flat gradient ``grad`` (arena layout)."""
        dt, NB, ws, cb = self.dtype, self.NB, self.ws, self.mod.conv_block
        gof = lambda name: self.arena.grad_of(name, grad)
        K = 16 * TRUNK[3]
        ops.dense_small_wgrad(dt, dout, self.a[3], gof("fc1.weight"), gof("fc1.bias"), NB, K, self.nout, TRUNK[3], 16)
        ops.dense_small_bwd(dt, dout, self.head.wp_fwd, self.a[3], self.dz[3], NB, K, self.head.Kpad_fwd, self.nout, ACT_LRELU, 0.1)
        for i in (3, 2, 1, 0):
            idx = 2 * i
            rec = self.mid[i - 1] if i > 0 else self.l0
            x_in = self.a[i - 1] if i > 0 else self.patches
            rows = NB * (self.S >> (i + 1)) ** 2
            ops.bias_grad(dt, self.dz[i], rows, TRUNK[i], ws.small, gof(f"conv_block.{idx}.bias"))
            ns = ops.conv_wgrad(rec.c, dt, x_in, self.dz[i], ws.slab)
            if i > 0:
                ops.wgrad_reduce(ws.slab, ns, TRUNK[i], TRUNK[i], TRUNK[i - 1], 16, gof(f"conv_block.{idx}.weight"))
                ops.conv_bwd_data(rec.c, dt, self.dz[i], rec.wp_bwd, self.dz[i - 1],
                                  ops.epilogue(mask=self.a[i - 1], mask_act=ACT_LRELU, mask_slope=0.1))
            else:
                ops.wgrad_reduce_perm(ws.slab, ns, TRUNK[0], TRUNK[0], self.kp, 1, gof("conv_block.0.weight"), 0, 0, self.k0)


class PxyTrainer(ResidentStep):
    """One call == one iteration of dSprites/pxy.py:156-191 (stage-1 trainer): real_code = E(img); trans_img = warp(img,
    get_matrix_pxy(code)); trans_code = E(trans_img); loss = MSE(affine_regularzier_pxy(real_code, trans_code), code); Adam(lr 2e-4,
    betas (.5, .999), :127) on Encoder_pxy.  Its ``state_dict()`` is the ``encoder_pxy_%d.pt`` the stage-2 loop loads (:205)."""

    def __init__(self, encoder_pxy: "Encoder_pxy", batch_size, dtype="f32", lr=2e-4, betas=(0.5, 0.999), allreduce=None):
        self.P, self.B = encoder_pxy, batch_size
        dt = parse_dtype(dtype)
        encoder_pxy.set_compute_dtype(dt)
        _require_cuda(next(encoder_pxy.parameters()))
        self.arena = Arena(encoder_pxy)                  # trainable here: parameters re-homed into one flat fp32 arena
        encoder_pxy._engines = {}                        # inference engines hold panels of the old storage
        self.eng = _PxyTrainEngine(encoder_pxy, batch_size, dt, self.arena)
        dev = self.arena.flat.device
        self.dev = dev
        self.lr, self.betas, self.allreduce = lr, betas, allreduce
        z = lambda *n: torch.zeros(*n, device=dev, dtype=torch.float32)
        B, C = batch_size, encoder_pxy.channels
        self.m, self.v = z(self.arena.numel), z(self.arena.numel)
        self.steps = torch.zeros(1, device=dev, dtype=torch.int32)
        self.losses = z(4)
        self.img_u8 = torch.zeros(B, 64, 64, device=dev, dtype=torch.uint8)
        self.img, self.trans = z(B, C, 64, 64), z(B, C, 64, 64)
        self.nd = encoder_pxy.fc1.weight.shape[0]           # 3 (p, x, y); the colored variant appends three colour gains
        self.code = z(B, self.nd)
        self.theta = z(B, 2, 3)
        self.dout = z(2 * B, self.nd)
        self.graph = None

    # hooks the colored variant overrides (colored.PxyColorTrainer)
    def _make_image(self):
        ops.u8_to_f32(self.img_u8, self.img)                                           # pxy.py:161-162

    def _transform(self):
        ops.warp_affine(self.img, self.theta, self.trans, self.B, self.P.channels, 64, 64)   # :177 (padding_mode='border')

    def _step_body(self):
        B, eng, ar, nd = self.B, self.eng, self.arena, self.nd
        ops.fill_f32(self.losses)
        self._make_image()
        ops.theta_pxy(self.code, nd, B, self.theta)                                     # :176
        self._transform()
        codes = eng.forward(self.img, self.trans)                                       # :174,178
        ops.loss_affine_pxy(codes[:B], codes[B:], nd, 0, B, self.code, nd, 1.0, self.losses[0:1], self.dout[:B], self.dout[B:], ncol=nd - 3)   # :180-182
        ops.fill_f32(ar.grad)
        eng.backward(self.dout, ar.grad)
        if self.allreduce is not None:
            self.allreduce(ar.grad)
        ops.adam_step(ar.flat, ar.grad, self.m, self.v, ar.numel, self.lr, self.betas[0], self.betas[1], 1e-8, self.steps[0:1], True)
        eng.repack()

    def load_inputs(self, img_u8, code):
        self.img_u8.copy_(img_u8, non_blocking=True)
        self.code.copy_(code, non_blocking=True)

    # capture() / step_resident(): engine.ResidentStep (without ``inputs`` and ``log`` the launches of _step_body alone)

    def train_step(self, img_u8, code):
        """train-loop entry: img_u8 uint8 [B,64,64] sprites, code [B,3] ~ U(-1,1) -> {'affine_loss'}"""
        self.load_inputs(img_u8, code)
        return {"affine_loss": float(self.step_resident()[0])}

    # -- full state (engine.TrainerState) -------------------------------------------------------------
    STATE_KIND = "pxy"

    def _state_modules(self):
        return {"P": self.P}

    def _state_moments(self):
        return {"P": (self.m, self.v)}

    def _state_repack(self):
        self.eng.repack()                                # the training engine is not among the module's inference engines
        self.P.repack()


class DspritesTrainer(ResidentStep):
    """One call == one iteration of dSprites/rp.py:365-482: D step (Adam lr 2e-4), then the joint info + affine + adversarial-G +
    relative-category step over G+E (Adam lr 1e-4).  optimizer_G of the reference is never stepped and is not created.
    Dead work removed: Encoder_pxy backward, the second (identical) alignment pass, D weight gradients in the joint step."""

    def __init__(self, encoder_pxy, generator, discriminator, encoder, batch_size, dtype="f32", allreduce=None, lrs=(2e-4, 1e-4), betas=(0.5, 0.999),
                 sync_bn=None, overlap=True):
        """``sync_bn`` (a dp.SyncBN): the generator's three BatchNorm layers use the statistics of the global batch.
        ``overlap``: the iteration runs as two chains (see _step_body); single-process only -- with ``allreduce`` / ``sync_bn`` the
        collectives stay on one stream and the serial body runs."""
        self.P, self.G, self.D, self.E, self.B = encoder_pxy, generator, discriminator, encoder, batch_size
        self.sync_bn = sync_bn
        self.overlap = bool(overlap) and allreduce is None and sync_bn is None
        dt = parse_dtype(dtype)
        for m in (encoder_pxy, generator, discriminator, encoder):
            m.set_compute_dtype(dt)
        B = batch_size
        self.pe, self.ge, self.de = encoder_pxy.engine(B), generator.engine(B), discriminator.engine(B)
        dev = generator.arena.flat.device
        if self.overlap:
            # second chain: own stream, own scratch (split-K scratch included), own engines -- the encoder, and a second generator engine
            # for the joint step's forward (and backward), so that it does not wait for the D step to release the first one's buffers
            self.ws2 = Workspace(dev, register=False)
            self.chain = torch.cuda.Stream(dev)
            # weight-gradient side lanes under the two chains are slower (profiles/r02_n_ab_small_lanes.txt): two lanes for the generator
            # backward only -- the one phase in which a single chain is active -- and from batch 256 up
            # (colored dSprites B = 512: 3.47 -> 3.34 ms; dSprites B = 128: 1.71 -> 1.73, profiles/r02_z_ab_tail_lanes.txt)
            self.side_a = SideStream(dev, Workspace.get(dev), lanes=2) if B >= 256 else None
            with Workspace.scope(self.ws2):
                self.ee, self.ge2 = encoder.engine(B, slot=1), generator.engine(B, slot=1)
        else:
            self.ee, self.ge2 = encoder.engine(B), self.ge
        self.allreduce, self.lr, self.betas = allreduce, lrs, betas
        ga, da, ea = generator.arena, discriminator.arena, encoder.arena
        z = lambda *n: torch.zeros(*n, device=dev, dtype=torch.float32)
        self.mD, self.vD = z(da.numel), z(da.numel)
        self.miG, self.viG, self.miE, self.viE = z(ga.numel), z(ga.numel), z(ea.numel), z(ea.numel)
        self.steps = torch.zeros(2, device=dev, dtype=torch.int32)
        self.losses = z(8)                                    # d, g, info, affine, relative_cat
        C = generator.channels
        self.nc, self.cd = generator.n_classes, generator.code_dim
        self.img = z(B, C, 64, 64)
        self.theta, self.theta2 = z(B, 2, 3), z(B, 2, 3)
        self.align, self.trans1, self.trans2 = z(B, C, 64, 64), z(B, C, 64, 64), z(B, C, 64, 64)
        self.dimg = z(B, C, 64, 64)
        self.dout_d = z(2 * B, 1)
        self.d_cat, self.d_cont = z(3 * B, self.nc), z(3 * B, self.cd)
        self.code1, self.code2 = z(B, self.cd), z(B, self.cd)
        self.onehot1, self.onehot2 = z(B, self.nc), z(B, self.nc)
        self.graph = None

    def _adam(self, arena, m, v, lr, slot, tick):
        ops.adam_step(arena.flat, arena.grad, m, v, arena.numel, lr, self.betas[0], self.betas[1], 1e-8, self.steps[slot:slot + 1], tick)

    def import_adam_state(self, opt_D, opt_info):
        """moments and step counts of the two ``torch.optim.Adam`` the reference steps (dSprites/rp.py:270-279: D | G + E parameters,
        ``.parameters()`` order) -- teacher-forced comparisons against a CPU run of the reference loop"""
        n = lambda mod: len(list(mod.parameters()))
        s0 = import_adam_moments(opt_D, [(n(self.D), self.mD, self.vD)])
        s1 = import_adam_moments(opt_info, [(n(self.G), self.miG, self.viG), (n(self.E), self.miE, self.viE)])
        self.steps.copy_(torch.tensor([s0, s1], dtype=torch.int32))

    def _step_body(self):
        """One iteration as TWO chains.  These networks are small (0.5 GFLOP per image): the step is a chain of ~200 launches of a few
        microseconds each, bound by launch latency, not by the chip -- so independent parts run side by side:
          main chain : align -> G(code1) -> D step (D forward x2, loss, backward, Adam, re-pack) -> D(gen2) -> d(img) through D
          2nd chain  : G(code2) [second generator engine, behind G(code1): BatchNorm running statistics keep the reference's order]
                       -> transform(code2) -> E forward x3 -> info / affine / relative-category losses -> E backward -> d(img) through E
          joined     : d(img) sum -> G backward -> Adam(G), Adam(E) -> re-pack.
        The joint step's generator and encoder passes read only G and E, which the D step does not touch (rp.py:404-482).  Same kernels
        on the same operands as the serial body: bit-identical results (tests/test_gpu_dsprites.py)."""
        if not self.overlap:
            return self._step_body_serial()
        B, nc, cd = self.B, self.nc, self.cd
        ge, ge2, de, ee = self.ge, self.ge2, self.de, self.ee
        ga, da, ea = self.G.arena, self.D.arena, self.E.arena
        L = self.losses
        mark = SideStream.mark
        main, chain = torch.cuda.current_stream(), self.chain
        sa = self.side_a                                  # weight-gradient lanes of the generator backward
        ops.fill_f32(L)
        # the alignment pass in front of BOTH chains: the second chain forks from a point with no main-chain work queued behind it
        # (behind the first generator forward the replayed step ran the two chains one after the other, profiles/r03_zzh_ab_align_late.txt)
        self._align()                                                                        # :374-377
        gen = ge.forward(self.onehot1, self.code1)
        chain.wait_event(mark())
        with torch.cuda.stream(chain), self.ws2.active():
            ops.fill_f32(ga.grad)
            ops.fill_f32(ea.grad)
            gen2 = ge2.forward(self.onehot2, self.code2)
            e_gen2 = mark()
            self._transform(self.code2, self.trans2, second=True)
            eo = ee.forward([gen2, self.align, self.trans2])
            cat, cont = eo["cat_layer.0"], eo["cont_layer.0"]
            ops.fill_f32(self.d_cat)
            ops.loss_mutual_info(cat[:B], nc, 0, nc, B, self.onehot2, nc, 0, False, 1.0, L[2:3], self.d_cat[:B])
            ops.loss_mse(cont[:B], cd, 0, cd, B, self.code2, cd, 0.0, 1.0, L[2:3], self.d_cont[:B])
            self._affine_loss(cont[B:2 * B], cont[2 * B:], L[3:4], self.d_cont[B:2 * B], self.d_cont[2 * B:])
            ops.loss_mutual_info(cat[2 * B:], nc, 0, nc, B, cat[B:2 * B], nc, 0, True, 1.0, L[4:5], self.d_cat[2 * B:])
            self._log_info_terms(cat, cont)
            dimg_e = ee.backward(0, 3, {"cat_layer.0": self.d_cat, "cont_layer.0": self.d_cont}, ea.grad, need_dimg=True)
            e_dimg = mark()
            # optimizer_info's step counter is shared by G and E: it ticks here, G's update (main chain, behind this event) reads it
            self._adam(ea, self.miE, self.viE, self.lr[1], 1, True)
            ee.repack()
            e_chain = mark()
        # ---- D step (:404-419): D(trans) then D(gen.detach()) ----
        self._transform(self.code1, self.trans1)                                             # :396-400
        ops.fill_f32(da.grad)
        out = de.forward([self.trans1, gen])["fc2"]
        ops.loss_bce_sigmoid(out[:B], 1, 0, B, 1.0, 0.5, L[0:1], self.dout_d[:B])
        ops.loss_bce_sigmoid(out[B:], 1, 0, B, 0.0, 0.5, L[0:1], self.dout_d[B:])
        de.backward(0, 2, {"fc2": self.dout_d}, da.grad)
        self._adam(da, self.mD, self.vD, self.lr[0], 0, True)
        de.repack()
        # ---- joint step (:424-482): the generator's adversarial term needs the UPDATED discriminator ----
        main.wait_event(e_gen2)
        g_fake = de.forward([gen2], patches=False)["fc2"]             # (input gradient only: no weight gradient, no patch rows)
        ops.loss_bce_sigmoid(g_fake, 1, 0, B, 1.0, 1.0, L[1:2], self.dout_d[:B])
        dimg_d = de.backward(0, 1, {"fc2": self.dout_d[:B]}, da.grad, need_wgrad=False, need_dimg=True)
        main.wait_event(e_dimg)
        ops.add_f32(self.dimg, dimg_e, dimg_d)
        ge2.backward(self.dimg, ga.grad, side=sa)
        if sa is not None:
            sa.join_lanes()
        main.wait_event(e_chain)
        self._adam(ga, self.miG, self.viG, self.lr[1], 1, False)
        ge.repack()
        ge2.repack()

    def _step_body_serial(self):
        B, nc, cd = self.B, self.nc, self.cd
        pe, ge, de, ee = self.pe, self.ge, self.de, self.ee
        ga, da, ea = self.G.arena, self.D.arena, self.E.arena
        C = self.G.channels
        L = self.losses
        ops.fill_f32(L)
        self._align()                                                                        # :374-377
        self._transform(self.code1, self.trans1)                                             # :396-400
        # ---- D step (:404-419): D(trans) then D(gen.detach()) ----
        gen = ge.forward(self.onehot1, self.code1, sync=self.sync_bn)
        ops.fill_f32(da.grad)
        out = de.forward([self.trans1, gen])["fc2"]
        ops.loss_bce_sigmoid(out[:B], 1, 0, B, 1.0, 0.5, L[0:1], self.dout_d[:B])
        ops.loss_bce_sigmoid(out[B:], 1, 0, B, 0.0, 0.5, L[0:1], self.dout_d[B:])
        de.backward(0, 2, {"fc2": self.dout_d}, da.grad)
        if self.allreduce is not None:
            self.allreduce(da.grad)
        self._adam(da, self.mD, self.vD, self.lr[0], 0, True)
        de.repack()
        # ---- joint step (:424-482) ----
        ops.fill_f32(ga.grad)
        ops.fill_f32(ea.grad)
        gen = ge.forward(self.onehot2, self.code2, sync=self.sync_bn)
        self._transform(self.code2, self.trans2)
        eo = ee.forward([gen, self.align, self.trans2])
        cat, cont = eo["cat_layer.0"], eo["cont_layer.0"]
        g_fake = de.forward([gen], patches=False)["fc2"]
        ops.loss_bce_sigmoid(g_fake, 1, 0, B, 1.0, 1.0, L[1:2], self.dout_d[:B])
        dimg_d = de.backward(0, 1, {"fc2": self.dout_d[:B]}, da.grad, need_wgrad=False, need_dimg=True)
        ops.fill_f32(self.d_cat)
        ops.loss_mutual_info(cat[:B], nc, 0, nc, B, self.onehot2, nc, 0, False, 1.0, L[2:3], self.d_cat[:B])
        ops.loss_mse(cont[:B], cd, 0, cd, B, self.code2, cd, 0.0, 1.0, L[2:3], self.d_cont[:B])
        self._affine_loss(cont[B:2 * B], cont[2 * B:], L[3:4], self.d_cont[B:2 * B], self.d_cont[2 * B:])
        ops.loss_mutual_info(cat[2 * B:], nc, 0, nc, B, cat[B:2 * B], nc, 0, True, 1.0, L[4:5], self.d_cat[2 * B:])
        self._log_info_terms(cat, cont)
        dimg_e = ee.backward(0, 3, {"cat_layer.0": self.d_cat, "cont_layer.0": self.d_cont}, ea.grad, need_dimg=True)
        ops.add_f32(self.dimg, dimg_e, dimg_d)
        pending = engine.allreduce_start(self.allreduce, ea.grad)
        ge.backward(self.dimg, ga.grad, sync=self.sync_bn)
        engine.allreduce_finish(self.allreduce, ga.grad, None)
        engine.allreduce_finish(self.allreduce, ea.grad, pending)
        self._adam(ga, self.miG, self.viG, self.lr[1], 1, True)
        self._adam(ea, self.miE, self.viE, self.lr[1], 1, False)
        ge.repack()
        ee.repack()

    def _log_info_terms(self, cat, cont):
        """With a loss log attached only: cat_loss -> losses[5], cont_loss -> losses[6] (loss-only launches, no gradient).  The
        reference's progress line prints the two terms on their own (rp.py:493-495); losses[2] stays their sum."""
        if self.log is None:
            return
        B, nc, cd, L = self.B, self.nc, self.cd, self.losses
        ops.loss_mutual_info(cat[:B], nc, 0, nc, B, self.onehot2, nc, 0, False, 1.0, L[5:6], None)
        ops.loss_mse(cont[:B], cd, 0, cd, B, self.code2, cd, 0.0, 1.0, L[6:7], None)

    # -- dataset-specific pieces (overridden by the colored variant) -------------------------------------------------
    def _align(self):
        """align = warp(img, inverse(T(x,y))[:, :2]) with (p,x,y) from the frozen Encoder_pxy."""
        B, C = self.B, self.G.channels
        pcode = self.pe.forward(self.img)
        ops.theta_pxy_align_inv(pcode, pcode.shape[1], B, self.theta)
        ops.warp_affine(self.img, self.theta, self.align, B, C, 64, 64)

    def _transform(self, code, out, second=False):
        """``second``: called from the second chain -- its own theta scratch"""
        B, C = self.B, self.G.channels
        theta = self.theta2 if second else self.theta
        ops.theta_rp(code, self.cd, B, theta)
        ops.warp_affine(self.align, theta, out, B, C, 64, 64)

    def _affine_loss(self, cont_align, cont_trans, loss, d_align, d_trans):
        ops.loss_affine_rp(cont_align, cont_trans, self.cd, 0, self.B, self.code2, self.cd, 1.0, loss, d_align, d_trans)

    def load_inputs(self, img_u8, code1, labels1, code2, labels2):
        """img_u8: uint8 [B,64,64] sprites (or float [B,C,64,64]); codes [B,code_dim]; labels int64 [B]."""
        if img_u8.dtype == torch.uint8:
            ops.u8_to_f32(img_u8.contiguous(), self.img)
        else:
            self.img.copy_(img_u8.reshape(self.img.shape))
        self.code1.copy_(code1)
        self.code2.copy_(code2)
        for oh, lab in ((self.onehot1, labels1), (self.onehot2, labels2)):
            oh.zero_()
            oh.scatter_(1, lab.view(-1, 1), 1.0)

    def train_step(self, img_u8, code1, labels1, code2, labels2):
        self.load_inputs(img_u8, code1, labels1, code2, labels2)
        l = self.step_resident().tolist()
        return dict(d_loss=l[0], g_loss=l[1], info_loss=l[2], affine_loss=l[3], relative_cat_loss=l[4])

    # -- full state (engine.TrainerState) -------------------------------------------------------------
    STATE_KIND = "dsprites"

    def _state_modules(self):
        # the frozen Encoder_pxy too: a run resumes from its own file alone.  Re-packing goes through the modules: the second chain's
        # engines (``ee``, ``ge2``: own panels over the shared masters) are among ``module._engines``.
        return {"P": self.P, "G": self.G, "D": self.D, "E": self.E}

    def _state_moments(self):
        return {"D": (self.mD, self.vD), "iG": (self.miG, self.viG), "iE": (self.miE, self.viE)}


class DeviceInputs(DeviceSampler):
    """Device-side replacement of the dSprites loop's host input work (dSprites/rp.py:236-262 the uint8 sprite array + DataLoader; :389-430
    numpy draws in the reference's order: code ~ U(-1,1), labels ~ randint, then again for the joint step).  ``dataset_u8``: uint8
    [N,64,64] sprites with values {0,1}."""

    def sprites(self, tr, idx=None):
        B = tr.B
        batch = self.buf("sprites", (B,) + tuple(self.data.shape[1:]), torch.uint8)
        torch.index_select(self.data, 0, self.sample_indices(B, 1) if idx is None else idx, out=batch)
        return batch

    def codes_and_labels(self, tr, first_stream):
        self.draw(ops.RNG_UNIFORM, tr.code1, -1.0, 1.0, first_stream)
        self.labels_onehot("labels1", tr.onehot1, tr.nc, first_stream + 1)
        self.draw(ops.RNG_UNIFORM, tr.code2, -1.0, 1.0, first_stream + 2)
        self.labels_onehot("labels2", tr.onehot2, tr.nc, first_stream + 3)

    def enqueue(self, tr: "DspritesTrainer"):
        self.begin_draws()                              # sprite indices, codes and labels (+ one-hot rows): one launch
        idx = self.sample_indices(tr.B, 1)
        self.codes_and_labels(tr, 2)
        self.end_draws()
        if engine.FUSE_DRAWS and self.data.dim() == 3:
            # gather + uint8 -> float + counter tick as one launch (the gather of the MNIST / CelebA samplers; the same {0, 1} values)
            N, H, W = self.data.shape
            ops.gather_u8_images(self.data, idx, None, tr.img, tr.B, 1, H, W, 1.0, 0.0, tick=self.step)
            return
        ops.u8_to_f32(self.sprites(tr, idx), tr.img)
        self.tick()


class PxyDeviceInputs(DeviceSampler):
    """Device-side input work of the stage-1 loops (dSprites/pxy.py:157-168: the uint8 sprite DataLoader and code ~ U(-1,1);
    colored_dSprites/pxy_color.py:163-187: the colour gains ~ U(.5,1) drawn first).  ``dataset_u8``: uint8 [N,64,64] sprites."""

    def enqueue(self, tr: "PxyTrainer"):
        self.begin_draws()
        idx = self.sample_indices(tr.B, 1)
        if hasattr(tr, "gains"):
            self.draw(ops.RNG_UNIFORM, tr.gains, 0.5, 1.0, 2)
        self.draw(ops.RNG_UNIFORM, tr.code, -1.0, 1.0, 3)
        self.end_draws()
        torch.index_select(self.data, 0, idx, out=tr.img_u8)
        self.tick()

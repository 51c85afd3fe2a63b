"""Host-side building blocks shared by the per-dataset models: flat parameter arenas, the shared device
workspace, conv-layer records (geometry + packed weight panels) over the C ABI in :mod:`ops`, the module base class, and the
dispatch functions every engine goes through (BatchNorm forms, fused-statistics buffers, the image-side transposed convolution).
Imports :mod:`ops` only; :mod:`affine`, :mod:`trunk` and the workload modules import this one."""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

from . import ops
from .ops import ACT_RELU, EG_BF16, EG_F16, EG_F32, OUT_NCHW_F32

# Reference paths the tests compare the production ones against (they monkeypatch these; nothing else changes them).  Every reader, in
# whichever module, reads ``engine.<NAME>`` at call time -- never ``from .engine import <NAME>`` -- so one patch here reaches them all.
# image-side transposed convolutions (128 / 64 -> C) as one GEMM + col2im gather (True) or as the 4-phase implicit GEMM (False)
IMG_GEMM = True
# weight gradient of the CelebA image-side layers straight from the fp32 images (ops.wgrad_img_tn, True) or from patch rows (im2col_img +
# conv_wgrad, False): the same bits; read when an engine is built
WGRAD_IMG_TN = True


def to_categorical(y, num_columns, device=None):
    """one-hot float tensor (celebA/EAD-GAN_celebA.py:56-62; the same function in the MNIST and dSprites scripts)."""
    y = torch.as_tensor(np.asarray(y), dtype=torch.int64, device=device)
    return torch.nn.functional.one_hot(y, num_columns).to(torch.float32)


def _require_cuda(t):
    if not t.is_cuda:
        raise RuntimeError("ead-gan_amd runs on MI355X only: tensors must be on a HIP device (no CPU fallback)")


def parse_dtype(dtype) -> int:
    if dtype in (EG_F32, "f32", "fp32", "float32", torch.float32):
        return EG_F32
    if dtype in (EG_BF16, "bf16", "bfloat16", torch.bfloat16):
        return EG_BF16
    if dtype in (EG_F16, "f16", "fp16", "float16", "half", torch.float16):
        return EG_F16
    raise ValueError(f"unsupported compute dtype {dtype!r} (use 'f32', 'bf16' or 'f16')")


class Arena:
    """All parameters of a module re-homed into ONE flat fp32 tensor (reference ``.parameters()`` order)
    with a matching flat gradient tensor: one fused Adam launch per optimizer, one all-reduce per pass."""

    def __init__(self, module: torch.nn.Module):
        params = list(module.parameters())
        dev = params[0].device
        n = sum(p.numel() for p in params)
        self.flat = torch.empty(n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n, device=dev, dtype=torch.float32)
        self.slices = {}
        off = 0
        for name, p in module.named_parameters():
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view(p.shape)
            p.grad = self.grad[off:off + k].view(p.shape)
            self.slices[name] = (off, k)
            off += k
        self.numel = n

    def grad_of(self, name, arena_grad=None):
        off, k = self.slices[name]
        return (self.grad if arena_grad is None else arena_grad)[off:off + k]


SPLITK_WS_BYTES = 72 << 20


class Workspace:
    """Scratch shared by every engine on a device (calls are stream-ordered, so one copy suffices).
    Grown only while engines are being built -- never inside a training step."""

    _per_device = {}

    def __init__(self, device, splitk=True, register=True):
        """``register=False``: a second chain's private workspace (own split-K scratch too) -- it does not become the device default"""
        self.device = device
        self._retired = []
        # chip share hint for the weight-gradient GEMMs launched with this scratch (ops.conv_wgrad): 0 = the whole chip; a side lane's
        # workspace says 128 workgroups, its launches run beside the main chain's GEMMs (profiles/r02_i_ab_tn8_target.txt)
        self.wgs_target = 0
        self.slab = torch.empty(0, device=device, dtype=torch.float32)
        self.gtmp = torch.empty(0, device=device, dtype=torch.float32)
        self.small = torch.empty(0, device=device, dtype=torch.float32)
        self.partials = torch.empty(max(2048, ops.sn_partials()), device=device, dtype=torch.float32)
        self.sums = torch.empty(0, device=device, dtype=torch.float32)
        # split-K partial tiles of the NT kernel: the planner splits up to ~2x512 tiles of 128x128 fp32 (64 KiB each)
        if splitk:
            self.splitk = torch.zeros(SPLITK_WS_BYTES // 4, device=device, dtype=torch.float32)      # zeroed: its tail holds arrival counters
            if register:
                ops.set_splitk_workspace(self.splitk)

    _scoped = None

    @classmethod
    @contextlib.contextmanager
    def scope(cls, ws: "Workspace"):
        """engines built inside take ``ws`` as their scratch (a chain that runs beside the main one must not share its scratch)"""
        prev, cls._scoped = cls._scoped, ws
        try:
            yield ws
        finally:
            cls._scoped = prev

    @contextlib.contextmanager
    def active(self):
        """launches enqueued inside split K into THIS workspace's scratch (ops.epilogue's default), not the device default"""
        prev = ops.SPLITK_OVERRIDE
        ops.SPLITK_OVERRIDE = self.splitk
        try:
            yield self
        finally:
            ops.SPLITK_OVERRIDE = prev

    @classmethod
    def get(cls, device) -> "Workspace":
        if cls._scoped is not None:
            return cls._scoped
        key = (device.type, device.index)
        if key not in cls._per_device:
            cls._per_device[key] = cls(device)
        return cls._per_device[key]

    def _grow(self, name, floats):
        """Workspaces only ever grow, and an outgrown buffer is kept alive: a hipGraph captured earlier (another trainer, another batch
        size) has its address baked in, and memory handed back to the caching allocator would be given to somebody else."""
        t = getattr(self, name)
        if t.numel() < floats:
            if t.numel():
                self._retired.append(t)
            setattr(self, name, torch.empty(int(floats), device=self.device, dtype=torch.float32))

    def need_slab(self, nbytes):
        self._grow("slab", (nbytes + 3) // 4)

    def need_gtmp(self, floats):
        self._grow("gtmp", floats)

    def need_small(self, floats):      # bn / sn / bias-grad partial buffers
        self._grow("small", floats)

    def need_sums(self, floats):
        self._grow("sums", floats)


# workgroups the weight-gradient GEMMs of a side lane aim for (tests set 0 -- the whole chip -- for their reference run)
LANE_WGS_TARGET = 64      # 64: profiles/r03_o_lane_wgs_sweep.txt (128 in round 2)


class _Lane:
    NAMES = ("slab", "gtmp", "small", "sums", "partials")

    def __init__(self, device, like: "Workspace"):
        self.stream = torch.cuda.Stream(device)
        self.ws = Workspace(device, splitk=False)
        self.ws.wgs_target = LANE_WGS_TARGET
        self.like = like
        self.ensure()

    def ensure(self):
        """Lane scratch follows the device workspace: an engine built after the lanes (a second trainer, a larger batch) may have grown
        it, and work forked onto this lane is sized by the device workspace's reservations."""
        for name in self.NAMES:
            self.ws._grow(name, getattr(self.like, name).numel())

    def __enter__(self):
        self._ctx = torch.cuda.stream(self.stream)
        return self._ctx.__enter__()

    def __exit__(self, *a):
        return self._ctx.__exit__(*a)


class SideStream:
    """Extra HIP streams ("lanes", each with its own scratch) for work that does not feed the critical path of a training
    step: the weight-gradient GEMMs with their reductions and bias-gradient sums run beside the backward-data GEMMs of
    the layers below (consecutive layers on alternating lanes, so one layer's HBM-bound reductions overlap the next
    layer's GEMM), weight re-packing after an optimizer step and the spectral-norm power iterations of the next sub-step
    run beside the current one.  ``defer(i, fn)``: lane i runs fn behind everything enqueued on the current stream so far;
    ``join()``: the current stream waits for every lane.  Both are event record/wait pairs, capturable into the step's
    hipGraph.  Lanes never launch NT convolutions (the split-K scratch belongs to the main stream)."""

    def __init__(self, device, like: "Workspace", lanes: int = 2):
        self.lanes = [_Lane(device, like) for _ in range(lanes)]
        # optimizer lane: (gradient all-reduce ->) Adam -> gradient zeroing -> panel re-packing of one network, behind ALL of its
        # weight-gradient chains, while the main stream is already in the next sub-step.  Not part of the round robin.
        self.opt = _Lane(device, like)
        # preparation lane: the next sub-step's power iterations and patch rows.  It waits for optimizer-lane events (new weights), so
        # the optimizer lane must never wait for it: hipStreamEndCapture of ROCm 7.2 segfaults on such a stream-level back edge
        # (X waited for Y, later Y waits for X) even though the node graph is acyclic -- profiles/scripts/capture_patterns.py.  The same
        # holds for longer cycles: the waits among the non-origin streams must form a DAG (profiles/r01_timeline_notes.md item 10).
        self.prep = _Lane(device, like)
        self.done = {}                                 # tag -> event behind a tagged lane chain (defer(..., tag=))
        self.done_lane = {}                            # tag -> the lane that ran the chain
        # tag -> main-stream event behind the last main-stream kernel that reads the tagged bucket's parameters or panels: the event of
        # the NEXT tagged fork (the backward passes fork a layer's chain, then launch that layer's backward-data GEMM, then move on to
        # the layer below), or close_tags() for the last one
        self.free = {}
        self._last_tag = None

    def lane(self, i: int) -> _Lane:
        return self.lanes[i % len(self.lanes)]

    # Every defer* enqueues fn's launches at once: the lane waits for the events named below, then fn runs with the lane as the current
    # stream (and its scratch as ``ws``).  The caller's stream does not wait for the lane; it joins (join / join_lanes) or waits for one
    # event (mark / wait) where it needs the lane's results.  No lane function defers work itself.
    def defer(self, i: int, fn, tag=None):
        """lane i runs fn(lane_workspace) behind everything enqueued on the current stream so far.  ``tag``: an event is recorded on the
        lane behind fn and kept in ``self.done[tag]`` (data parallel: the gradient bucket this chain completes can be reduced as soon
        as the event fires, see CelebATrainer)."""
        ev = self.mark()
        if tag is not None:
            if self._last_tag is not None:
                self.free[self._last_tag] = ev
            self._last_tag = tag
        self._run(self.lane(i), [ev], fn, tag)

    def close_tags(self):
        """the current position of the current stream is behind every reader of the last tagged bucket"""
        if self._last_tag is not None:
            self.free[self._last_tag] = self.mark()
            self._last_tag = None

    def defer_opt_after(self, tags, fn):
        """the optimizer lane runs fn(ws) behind the tagged chains ``tags`` and the main-stream readers of their buckets ONLY (not behind
        the rest of the backward pass): bucket-wise optimizer updates start while the layers below are still in their backward pass"""
        evs = []
        for t in tags:
            d = self.done.pop(t, None)                  # None: the caller already waited for it (data parallel)
            if d is not None:
                evs.append(d)
            evs.append(self.free.pop(t))
        self._run(self.opt, evs, fn)

    def defer_opt(self, fn):
        """the optimizer lane runs fn(ws) behind the current stream AND every weight-gradient chain forked so far"""
        evs = [self.mark()]
        for ln in self.lanes:
            ev = torch.cuda.Event()
            ev.record(ln.stream)
            evs.append(ev)
        self._run(self.opt, evs, fn)

    def defer_prep(self, fn):
        self._run(self.prep, [self.mark()], fn)

    def _run(self, ln, evs, fn, tag=None):
        ln.ensure()
        for ev in evs:
            ln.stream.wait_event(ev)
        with ln:
            fn(ln.ws)
            if tag is not None:
                self.done[tag] = self.mark()
                self.done_lane[tag] = ln

    @staticmethod
    def mark() -> "torch.cuda.Event":
        """an event at the current position of the current stream (inside ``with lane:`` -- of that lane)"""
        ev = torch.cuda.Event()
        ev.record()
        return ev

    @staticmethod
    def wait(ev):
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def join_lanes(self):
        """the current stream waits for the weight-gradient lanes only (not for the optimizer / preparation lanes)"""
        self._join(self.lanes)

    def join(self):
        self._join(self.lanes + [self.opt, self.prep])

    @staticmethod
    def _join(lanes):
        cur = torch.cuda.current_stream()
        for ln in lanes:
            ev = torch.cuda.Event()
            ev.record(ln.stream)
            cur.wait_event(ev)


class SyncScratch:
    """Per-engine scratch of synchronised BatchNorm: one [3*C] statistics block and one [2*C] backward-sum block per layer."""

    def __init__(self, channels, device):
        self.stats = [torch.empty(3 * c, device=device, dtype=torch.float32) for c in channels]
        self.sums = [torch.empty(2 * c, device=device, dtype=torch.float32) for c in channels]


def bn_train_forward(dt, x, y, M, C, bn, mean, invstd, ws_small, act, slope=0.0, sync=None, stats=None, training=True, fused=(0, None)):
    """nn.BatchNorm2d forward, THE place that chooses its form.  ``training=False``: running statistics, nothing updated (module.eval()).
    ``fused`` = (row blocks, moments) that the producing convolution's epilogue left (stat_buffer): x is read once (apply) instead of
    twice.  ``sync`` (a dp.SyncBN): statistics over the global batch of all ranks -- local (n, mean, M2) -> one exchange of 3*C floats ->
    Chan-combined mean / variance.  Otherwise batch statistics of this rank; every training form updates the running statistics."""
    if not training:
        ops.bn_fwd_eval(dt, x, y, M, C, bn.weight, bn.bias, bn.eps, bn.running_mean, bn.running_var, ws_small, act, slope)
    elif fused[0]:
        ops.bn_fwd_train_fused(dt, x, y, M, C, fused[1], fused[0], M // fused[0], bn.weight, bn.bias, bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                               bn.num_batches_tracked, mean, invstd, ws_small, act, slope)
    elif sync is None:
        ops.bn_fwd_train(dt, x, y, M, C, bn.weight, bn.bias, bn.eps, bn.momentum, bn.running_mean, bn.running_var, bn.num_batches_tracked, mean, invstd,
                         ws_small, act, slope)
    else:
        ops.bn_stats_local(dt, x, M, C, ws_small, stats)
        allst = sync.gather_stats(stats)
        ops.bn_fwd_from_stats(dt, x, y, M, C, allst, sync.world, M * sync.world, bn.weight, bn.bias, bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                              bn.num_batches_tracked, mean, invstd, ws_small, act, slope)


def bn_train_backward(dt, z, da, dz, M, C, bn, mean, invstd, act, slope, dgamma, dbeta, ws, sync=None, sums=None, fused=(0, None), accumulate=True,
                      training=True):
    """Backward of bn_train_forward, THE place that chooses its form (``ws``: a Workspace).  ``fused`` = (row blocks, sums): ``da`` came
    from a launch with bn_bwd_epilogue, it already holds dy = da * act'(bn(z)) and the two sums are in the buffer.  ``sync``: the two
    per-channel sums over the global batch (one exchange of 2*C floats); dgamma / dbeta are this rank's share -- the gradient all-reduce
    averages them like every other gradient.  ``accumulate=False``: dgamma / dbeta are stored, not added to.
    ``training=False``: backward of the running-statistics forward -- elementwise, the input gradient only; dgamma / dbeta are not
    touched (may be None) and ``da`` must be the plain activation gradient (no bn_bwd_epilogue on the launch that produced it)."""
    if not training:
        assert not fused[0], "the BatchNorm-backward epilogue forms the training-mode dy"
        ops.bn_bwd_eval(dt, z, da, dz, M, C, bn.weight, bn.bias, bn.eps, bn.running_mean, bn.running_var, ws.small, act, slope)
    elif fused[0]:
        ops.bn_bwd_fused(dt, z, da, dz, M, C, fused[1], fused[0], bn.weight, bn.bias, mean, invstd, dgamma, dbeta, ws.sums, ws.small, accumulate=accumulate)
    elif sync is None:
        ops.bn_bwd(dt, z, da, dz, M, C, bn.weight, bn.bias, mean, invstd, act, slope, dgamma, dbeta, ws.sums, ws.small, accumulate=accumulate)
    else:
        ops.bn_bwd_sums_local(dt, z, da, M, C, bn.weight, bn.bias, mean, invstd, act, slope, dgamma, dbeta, sums, ws.small, accumulate=accumulate)
        sync.reduce_sums(sums)
        ops.bn_bwd_from_sums(dt, z, da, dz, M, C, sums, M * sync.world, bn.weight, bn.bias, mean, invstd, act, slope, ws.small)


class InputGrad:
    """What a generator engine needs for the gradient with respect to its inputs (ops.linear_dinput on the first layer's output gradient
    and the layer's fp32 master): the split scratch, allocated HERE -- with the engine, never at backward time: a buffer that grows later
    would move addresses under hipGraphs captured by others -- and ``scratch``, where the bias / BatchNorm parameter gradients of a pass
    with ``need_wgrad=False`` land (the kernels that form them next to an input gradient always write them)."""

    def __init__(self, dtype, B, NI, NJ, K, strides, device, scratch_floats):
        self.dtype, self.B, self.NI, self.NJ, self.K, self.strides = dtype, B, NI, NJ, K, tuple(int(s) for s in strides)
        self.ws = torch.empty(max(1, ops.linear_dinput_ws_floats(B, NI, NJ, K)), device=device, dtype=torch.float32)
        self.scratch = torch.empty(int(scratch_floats), device=device, dtype=torch.float32)

    def run(self, dH, w, dinp):
        """dinp [B, K] fp32 <- dH x w (every element stored)"""
        if dinp.dtype != torch.float32 or tuple(dinp.shape) != (self.B, self.K) or not dinp.is_contiguous():
            raise ValueError(f"dinp must be a contiguous fp32 [{self.B}, {self.K}] tensor")
        _require_cuda(dinp)
        ops.linear_dinput(self.dtype, dH, self.NI * self.NJ, w, dinp, self.B, self.NI, self.NJ, self.K, *self.strides, self.ws)


def drop_in_backward(eng, dimg, need_inputs, need_params, training, widths):
    """Backward of the generators' autograd bridges (``_GenFn`` of celeba, mnist, dsprites) -> ([input gradient or None per input],
    [parameter gradients]).  ``need_inputs`` / ``need_params``: ``ctx.needs_input_grad`` of the inputs (widths ``widths``, in the order
    the engine concatenates them) and of the parameters.  One engine pass yields both; without a parameter that needs a gradient the
    weight-gradient chains are skipped.  ``training=False`` (the forward ran with the running statistics) yields input gradients only."""
    gen = eng.gen
    wgrad = any(need_params)
    if wgrad and not training:
        raise NotImplementedError("eval-mode generators give input gradients only: a parameter requires grad -- call requires_grad_(False) on "
                                  "the module (projection, saliency), or use train mode for parameter gradients")
    scratch = torch.zeros_like(gen.arena.grad) if wgrad else None
    dinp = torch.empty(eng.B, eng.cin, device=dimg.device, dtype=torch.float32) if any(need_inputs) else None
    eng.backward(dimg.contiguous(), scratch, dinp=dinp, need_wgrad=wgrad, training=training)
    ins, col = [], 0
    for need, w in zip(need_inputs, widths):
        ins.append(dinp[:, col:col + w].clone() if need else None)
        col += w
    if wgrad:
        grads = [scratch[off:off + k].view(p.shape) for p, (off, k) in zip(gen.parameters(), gen.arena.slices.values())]
    else:
        grads = [None] * len(gen.arena.slices)
    return ins, grads


def wants_input_grad(*inputs):
    """an eval-mode drop-in forward builds a graph only for this: autograd is recording and an input requires grad"""
    return torch.is_grad_enabled() and any(t.requires_grad for t in inputs)


def stat_buffer(stat, key, c, dtype, bwd, ep, C, device, nrb=None, floats=None):
    """(row blocks, buffer) if the launch described by (c, bwd, ep) can take its column statistics in the epilogue, else (0, None).  Asked
    once per ``key`` of the engine's ``stat`` dict, with the very epilogue the launch uses (same hints, same split-K scratch).  The
    caller's own rules come as arguments: ``nrb()`` -> row blocks where ops.conv_stat_blocks of this launch is not the whole answer,
    ``floats(row blocks)`` -> buffer size where it is not the two sums per channel and block of the BatchNorm statistics."""
    if key not in stat:
        n = ops.conv_stat_blocks(c, dtype, bwd, ep) if nrb is None else nrb()
        size = 2 * C * n if floats is None else floats(n)
        stat[key] = (n, torch.empty(size, device=device, dtype=torch.float32) if n else None)
    return stat[key]


def bn_bwd_epilogue(stat, z, mean, invstd, bn):
    """epilogue of the launch that produces d(a) of a BatchNorm + ReLU layer: it also forms dy = da * relu'(bn(z)) and leaves the two sums
    of the layer's BatchNorm backward in ``stat`` (bn_train_backward(..., fused=) takes them)"""
    return ops.epilogue(stat_mode=ops.STAT_BN_BWD, stat_out=stat, stat_aux=z, stat_p=(mean, invstd, bn.weight, bn.bias), stat_act=ACT_RELU)


def convt_img(dt, x, gemm, cols, implicit, bias, act, out, fused):
    """The image-side transposed convolution (K channels -> the few of an fp32 NCHW image ``out``, + bias + activation), THE place that
    chooses its form: one launch (GEMM + gather, the columns stay in LDS) where ``fused`` -- the caller's own conditions -- and the
    kernel allow it; one GEMM over the input pixels with N = taps x C columns into ``cols`` + the col2im gather (every activation read
    once); or, with IMG_GEMM off or without a GEMM record (``gemm`` None), the 4-phase implicit GEMM of the record ``implicit``."""
    B, C = out.shape[0], out.shape[1]
    k, stride, pad = implicit.k, implicit.stride, implicit.pad
    if gemm is None or not IMG_GEMM:
        ops.conv_bwd_data(implicit.c, dt, x, implicit.wp_bwd, out, ops.epilogue(bias=bias, act=act, out_mode=OUT_NCHW_F32))
    elif fused and ops.convt_img_mfma_ok(dt, C, gemm.H, gemm.W, gemm.Cin, k, stride, pad):
        ops.convt_img_mfma(dt, x, gemm.wp_fwd, bias, out, B, C, gemm.H, gemm.W, act, 0.0, K=gemm.Cin)
    else:
        ops.conv_fwd(gemm.c, dt, x, gemm.wp_fwd, cols, None)
        ops.col2im_img(dt, cols, B, C, gemm.H, gemm.W, k, stride, pad, bias, act, 0.0, out)


def wgrad_side(side, ws, lane, fn, tag=None):
    """a layer's weight- / bias-gradient chain ``fn(workspace)``: on lane ``lane`` of ``side`` (a SideStream) when there is one, else here"""
    if side is None:
        fn(ws)
    else:
        side.defer(lane, fn, tag)


def allreduce_start(ar, flat):
    """start the gradient average of ``flat`` where the all-reduce has an asynchronous form -> handle, else None"""
    return ar.start(flat) if ar is not None and hasattr(ar, "start") else None


def allreduce_finish(ar, flat, handle):
    """wait for a started average (``handle``) or, without one, run the blocking form now"""
    if handle is not None:
        ar.finish(handle)
    elif ar is not None:
        ar(flat)


# an iteration's device-side draws as one launch and the counter tick inside the gather (same values); False: one launch per draw, the
# reference the tests compare against.  Read as ``engine.FUSE_DRAWS`` everywhere (see IMG_GEMM)
FUSE_DRAWS = True


def shard_span(numel, rank, world):
    """-> (elem0, total): the span a rank's draw of ``numel`` elements takes in the global draw of ``world`` ranks (eg_rng_fill's
    ``elem0`` / ``total``): rank r owns the elements [r * numel, (r + 1) * numel) of ``world * numel``, the rows of its slice of the
    global batch.  THE place that computes it."""
    numel, rank, world = int(numel), int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"shard_span: need world >= 1 and 0 <= rank < world, got rank {rank}, world {world}")
    return rank * numel, world * numel


class DeviceSampler:
    """Shared part of the trainers' device-side input pipelines: a uint8 dataset resident in HBM, a device step counter and
    counter-based draws (ops.rng_fill: reproducible per (seed, step, stream), the reference's distributions, NOT numpy's stream --
    parity tests keep feeding host draws through ``load_inputs``).  Sampling follows ``DataLoader(shuffle=True)``: a keyed permutation of the
    dataset per epoch, every image exactly once (``sampling="replacement"``: independent uniform draws).  Subclasses implement ``enqueue(trainer)``: fill the trainer's static input slots, then tick
    the counter; inside ``trainer.capture(inputs=...)`` those launches are part of the iteration's hipGraph.
    ``rank`` / ``world`` (data parallel): every draw is this rank's shard of the global batch's draw (``shard_span``), so the ranks'
    slots, concatenated in rank order, are the slots of one rank at the global batch, and an epoch visits every image once over all
    ranks.  ``step`` counts global iterations on every rank."""

    def __init__(self, dataset_u8: torch.Tensor, seed: int = 0, sampling: str = "permutation", *, rank: int = 0, world: int = 1):
        if not dataset_u8.is_cuda or dataset_u8.dtype != torch.uint8:
            raise ValueError("dataset must be a uint8 device tensor")
        if sampling not in ("permutation", "replacement"):
            raise ValueError("sampling must be 'permutation' (DataLoader(shuffle=True): every image once per epoch) or 'replacement'")
        shard_span(0, rank, world)
        self.rank, self.world = int(rank), int(world)
        self.data = dataset_u8.contiguous()
        self.sampling = sampling
        self.seed = int(seed)
        self.step = torch.zeros(1, device=dataset_u8.device, dtype=torch.int32)
        self._buf = {}

    def buf(self, name, shape, dtype):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._buf[name] = torch.empty(shape, device=self.data.device, dtype=dtype)
        return t

    # Draws of one iteration as ONE launch (eg_rng_fill_multi: the values of one eg_rng_fill per draw -- a value depends on (element, step,
    # stream id, seed) only, not on the launch it comes from): between begin_draws() and end_draws() the draw methods below only collect.
    _draws = None

    def begin_draws(self):
        if FUSE_DRAWS:
            self._draws = []

    def end_draws(self):
        draws, self._draws = self._draws, None
        if draws:
            ops.rng_fill_multi(draws, self.seed, self.step, self.rank, self.world)

    def draw(self, kind, out, a, b, stream_id):
        if self._draws is not None:
            self._draws.append((kind, out, a, b, stream_id))
            return
        ops.rng_fill(kind, out, a, b, self.seed, self.step, stream_id, self.rank, self.world)

    def sample_indices(self, B, stream_id=1):
        idx = self.buf("idx", (B,), torch.int64)
        if self.sampling == "permutation":               # a fresh permutation of the dataset per epoch, as the reference's DataLoader draws
            self.draw(ops.RNG_EPOCH_PERM, idx, self.data.shape[0], 0, stream_id)
        else:
            self.draw(ops.RNG_RANDINT, idx, 0, self.data.shape[0], stream_id)
        return idx

    def labels_onehot(self, name, onehot, n_classes, stream_id, lab=None):
        if lab is None:
            lab = self.buf(name, (onehot.shape[0],), torch.int64)
        if self._draws is not None:
            self._draws.append((ops.RNG_RANDINT, lab, 0, n_classes, stream_id, onehot))      # the one-hot rows written by the same launch
            return lab
        self.draw(ops.RNG_RANDINT, lab, 0, n_classes, stream_id)
        ops.onehot(lab, onehot, onehot.shape[0], n_classes)
        return lab

    def tick(self):
        ops.counter_add(self.step, 1)


def unwrap_ring(ring, head, capacity, since=0):
    """Rows of the iterations [max(since, head - capacity), head) of a ring filled by eg_runlog_append (row = iteration % capacity), in
    iteration order: -> (first iteration, array [iterations, n])"""
    first = max(int(since), int(head) - int(capacity), 0)
    idx = np.arange(first, int(head)) % int(capacity)
    return first, np.asarray(ring)[idx].copy()


class LossLog:
    """Loss history of a run kept on the device: ``append()`` enqueues eg_runlog_append on the current stream (row ``head % capacity`` of
    the ring <- ``trainer.losses``; inside a trainer's captured iteration it is a node of the hipGraph), ``flush_async()`` copies ring,
    head and the non-finite flag into a pinned host mirror on a copy stream behind an event, so reading losses never drains the
    queued iterations.  The caller flushes at least once per ``capacity`` appends (train.TrainRun does); rows older than that are
    overwritten."""

    def __init__(self, trainer, capacity=1024, _host_only_n=None):
        self.capacity = int(capacity)
        if self.capacity <= 0:
            raise ValueError("LossLog: capacity must be positive")
        self.trainer = trainer
        self._pending = None
        self.mirror_head, self.mirror_flag = 0, 0
        if _host_only_n is not None:                    # a mirror without a device side (reading a saved ring; host tests)
            self.n = int(_host_only_n)
            self.mirror = np.zeros((self.capacity, self.n), np.float32)
            return
        self.losses = trainer.losses
        self.n = self.losses.numel()
        dev = self.losses.device
        self.ring = torch.zeros(self.capacity, self.n, device=dev, dtype=torch.float32)
        self.head = torch.zeros(1, device=dev, dtype=torch.int32)
        self.first_nonfinite = torch.zeros(1, device=dev, dtype=torch.int32)
        self._ring_host = torch.zeros(self.capacity, self.n, dtype=torch.float32).pin_memory()
        self._hf_host = torch.zeros(2, dtype=torch.int32).pin_memory()
        self.mirror = self._ring_host.numpy()
        self.copy_stream = torch.cuda.Stream(dev)

    @classmethod
    def host_mirror(cls, n, capacity):
        return cls(None, capacity, _host_only_n=n)

    def append(self):
        ops.runlog_append(self.losses, self.n, self.ring, self.capacity, self.head, self.first_nonfinite)

    def landed(self) -> bool:
        """no copy is in flight (a finished one is taken into the mirror's head / flag here)"""
        if self._pending is not None and self._pending.query():
            self._take()
        return self._pending is None

    def _take(self):
        self._pending = None
        self.mirror_head, self.mirror_flag = int(self._hf_host[0]), int(self._hf_host[1])

    def wait(self):
        """block until the copy in flight (if any) has landed -- the only host wait the log can cause"""
        if self._pending is not None:
            self._pending.synchronize()
            self._take()

    def flush_async(self):
        """Snapshot behind everything enqueued on the current stream so far.  Head and flag are copied BEFORE the ring: the ring then
        holds every row below the copied head (appends that run during the copy only touch the slots of the oldest rows)."""
        self.wait()
        ev = torch.cuda.Event()
        ev.record()
        self.copy_stream.wait_event(ev)
        with torch.cuda.stream(self.copy_stream):
            self._hf_host[0:1].copy_(self.head, non_blocking=True)
            self._hf_host[1:2].copy_(self.first_nonfinite, non_blocking=True)
            self._ring_host.copy_(self.ring, non_blocking=True)
            self._pending = torch.cuda.Event()
            self._pending.record()

    def rows(self, since=0):
        """the rows that have landed, [iterations, n] in iteration order (the last ``capacity`` at most; from iteration ``since``)"""
        self.landed()
        return unwrap_ring(self.mirror, self.mirror_head, self.capacity, since)[1]

    def first_row(self, since=0):
        return max(int(since), self.mirror_head - self.capacity, 0)

    def load(self, head, first_nonfinite):
        """continue a saved run's numbering (trainer.load_state_dict): in place, the captured append keeps its addresses"""
        self.wait()
        self.head.fill_(int(head))
        self.first_nonfinite.fill_(int(first_nonfinite))
        self.mirror_head, self.mirror_flag = int(head), int(first_nonfinite)


def ema_decay(beta, ramp, t):
    """The decay eg_ema_update applies in its update number ``t`` (0-based), as the float32 the kernel forms: ``beta`` when ``ramp == 0``,
    else min(beta, (1 + t) / (ramp + t)) -- the same three fp32 operations in the same order (a warm-up: early updates follow the
    weights closely, from some t on the decay is ``beta`` for good)."""
    beta, ramp = np.float32(beta), np.float32(ramp)
    if ramp == 0:
        return beta
    tf = np.float32(int(t))
    return np.minimum(beta, (np.float32(1) + tf) / (ramp + tf))


class WeightEMA:
    """Exponential moving average of the weights of some of a trainer's modules, kept by ONE launch per iteration
    (``update()``: eg_ema_update over a device-resident segment table built here, once; inside a trainer's captured iteration it is a
    node of the hipGraph).  Per module the shadow is one flat fp32 tensor the size of ``module.arena.flat`` (one lerp segment, however
    many parameters; a module without an arena of its own -- Encoder_pxy -- gives one segment per parameter) and one clone per buffer: ``running_mean`` / ``running_var`` are averaged, every other buffer (``num_batches_tracked``,
    the spectral-norm vectors -- an average of unit vectors is no unit vector) is copied bit for bit.  At construction the shadow equals
    the modules' current state and no update has been done.  The shadow has no packed panels: it is never an operand of a convolution;
    ``copy_to`` loads it into a module that is."""

    LERP_BUFFERS = ("running_mean", "running_var")

    def __init__(self, modules, beta=0.999, ramp=0.0):
        self.beta, self.ramp = float(beta), float(ramp)
        if not 0.0 <= self.beta < 1.0 or not self.ramp >= 0.0:
            raise ValueError(f"WeightEMA: need 0 <= beta < 1 and ramp >= 0, got beta = {beta!r}, ramp = {ramp!r}")
        if not modules:
            raise ValueError("WeightEMA: no module to track")
        self.names = tuple(modules)
        self._flat, self._buffers, self._layout = {}, {}, {}
        segments = []
        for name, mod in modules.items():
            arena = mod.arena                           # None: a module whose parameters were not re-homed by itself (Encoder_pxy)
            params = dict(mod.named_parameters())
            if arena is not None:
                spans = dict(arena.slices)
                _require_cuda(arena.flat)
                flat = arena.flat.detach().clone()
                segments.append((arena.flat, flat, ops.EMA_LERP))
            else:                                       # one lerp segment per parameter, the shadow flat all the same
                spans, off = {}, 0
                for key, p in params.items():
                    spans[key] = (off, p.numel())
                    off += p.numel()
                p0 = next(iter(params.values()))
                _require_cuda(p0)
                flat = torch.empty(off, device=p0.device, dtype=torch.float32)
                for key, p in params.items():
                    live = p.detach()
                    if not live.is_contiguous():
                        raise ValueError(f"WeightEMA: parameter {name}.{key} is not contiguous")
                    o, k = spans[key]
                    flat[o:o + k].copy_(live.reshape(-1))
                    segments.append((live.reshape(-1), flat[o:o + k], ops.EMA_LERP))
            bufs, layout = {}, []
            for key, v in mod.state_dict().items():
                if key in spans:
                    layout.append((key, spans[key], tuple(v.shape)))
                    continue
                live = v.detach()
                if not live.is_contiguous():
                    raise ValueError(f"WeightEMA: buffer {name}.{key} is not contiguous")
                bufs[key] = live.clone()
                layout.append((key, None, None))
                segments.append((live, bufs[key], ops.EMA_LERP if key.endswith(self.LERP_BUFFERS) else ops.EMA_COPY))
            self._flat[name], self._buffers[name], self._layout[name] = flat, bufs, layout
        self.updates = torch.zeros(2, device=segments[0][0].device, dtype=torch.int32)      # (updates done, arrival counter)
        self._segments = segments                                                           # the table holds their addresses
        self.table, self.chunk_first, self.nseg = ops.ema_plan(segments)

    def update(self):
        ops.ema_update(self.table, self.chunk_first, self.nseg, self.beta, self.ramp, self.updates)

    def state_dict(self, name):
        """the averaged weights of module ``name`` under the module's own keys in the module's own order (what ``module.state_dict()``
        gives, so sampling.load_generator / score.load_encoders read a file of it); the values are views of the shadow"""
        flat, bufs = self._flat[name], self._buffers[name]
        out = {}
        for key, span, shape in self._layout[name]:
            out[key] = bufs[key] if span is None else flat[span[0]:span[0] + span[1]].view(shape)
        return out

    def copy_to(self, name, module):
        """load the shadow of ``name`` into ``module`` (same class), in place; its engines' panels are re-packed"""
        module.load_state_dict(self.state_dict(name))
        return module

    def state_tensors(self):
        out = {f"ema.{name}.{k}": v for name in self.names for k, v in self.state_dict(name).items()}
        out["ema.updates"] = self.updates
        return out

    def meta(self):
        return [self.beta, self.ramp, list(self.names)]

    def loaded(self):
        """after the shadow was written from a saved state: the arrival counter's contract is "left at zero" by every launch; cleared so
        that a load never depends on that"""
        self.updates[1:2].zero_()


DTYPE_NAMES = {EG_F32: "f32", EG_BF16: "bf16", EG_F16: "f16"}
STATE_FORMAT = 1


def validate_state(sd, kind, spec):
    """Checks of ``load_state_dict`` that need no device: ``spec`` maps every expected key to the shape of its tensor (a tuple) or to
    None for a plain value.  Raises ValueError naming the first offending key; nothing has been written when it does."""
    if not isinstance(sd, dict):
        raise ValueError("state: not a dict")
    if sd.get("meta.kind") != kind:
        raise ValueError(f"meta.kind: state of a {sd.get('meta.kind')!r} trainer cannot be loaded into a {kind!r} trainer")
    if sd.get("meta.format") != STATE_FORMAT:
        raise ValueError(f"meta.format: {sd.get('meta.format')!r} (this build reads format {STATE_FORMAT})")
    for key, shape in spec.items():
        if key not in sd:
            raise ValueError(f"{key}: missing from the state")
        v = sd[key]
        if shape is None:
            if isinstance(v, torch.Tensor):
                raise ValueError(f"{key}: expected a plain value, found a tensor")
        else:
            if not isinstance(v, torch.Tensor):
                raise ValueError(f"{key}: expected a tensor of shape {tuple(shape)}")
            if tuple(v.shape) != tuple(shape):
                raise ValueError(f"{key}: shape {tuple(v.shape)} in the state, {tuple(shape)} in the trainer")


class TrainerState:
    """``state_dict()`` / ``load_state_dict()`` of the fused trainers: everything an iteration reads that an earlier iteration wrote --
    module parameters and buffers (fp32 masters, BatchNorm running statistics, spectral-norm vectors), Adam moments and the device step
    counters, the sampler's (seed, step), the loss log's head.  A flat dict of CPU tensors and plain values (``torch.load(...,
    weights_only=True)`` reads it).  Loading copies IN PLACE -- a captured hipGraph holds the addresses -- and re-packs the engines'
    weight panels; it works on a trainer that has been captured and used.  Batch size and compute dtype are not state.
    Subclasses provide ``STATE_KIND``, ``_state_modules()`` ({name: module}), ``_state_moments()`` ({name: (m, v)}) and may add
    ``_state_extra_tensors()`` ({key: device tensor}), ``_state_repack()``, ``_state_zero_scratch()``."""

    STATE_KIND = None
    inputs = None
    log = None
    ema = None                                          # a WeightEMA (ResidentStep.attach_ema); None: the state holds no ``ema.*`` key

    def _state_extra_tensors(self):
        return {}

    def _state_repack(self):
        for mod in self._state_modules().values():
            mod.repack()

    def _state_zero_scratch(self):
        pass

    def _state_tensors(self):
        """{key: device tensor} of every tensor the state holds, in a fixed order"""
        out = {}
        for name, mod in self._state_modules().items():
            for k, v in mod.state_dict().items():
                out[f"modules.{name}.{k}"] = v
        out.update(self._state_extra_tensors())
        for name, (m, v) in self._state_moments().items():
            out[f"adam.{name}.m"] = m
            out[f"adam.{name}.v"] = v
        out["adam.steps"] = self.steps
        if self.ema is not None:
            out.update(self.ema.state_tensors())
        return out

    def _state_spec(self):
        spec = {k: tuple(v.shape) for k, v in self._state_tensors().items()}
        if self.inputs is not None:
            spec.update({"inputs.seed": None, "inputs.step": None, "inputs.sampling": None, "inputs.flip": None})
        if self.log is not None:
            spec.update({"log.head": None, "log.first_nonfinite": None})
        if self.ema is not None:
            spec["meta.ema"] = None
        return spec

    def _state_dtype(self):
        return next(iter(self._state_modules().values())).compute_dtype

    def state_dict(self):
        torch.cuda.synchronize()
        sd = {k: v.detach().to("cpu", copy=True) for k, v in self._state_tensors().items()}
        if self.inputs is not None:
            sd["inputs.seed"] = int(self.inputs.seed)
            sd["inputs.step"] = int(self.inputs.step.item())
            sd["inputs.sampling"] = str(self.inputs.sampling)
            sd["inputs.flip"] = int(bool(getattr(self.inputs, "flip", False)))
        if self.log is not None:
            sd["log.head"] = int(self.log.head.item())
            sd["log.first_nonfinite"] = int(self.log.first_nonfinite.item())
        if self.ema is not None:
            sd["meta.ema"] = self.ema.meta()
        lr = self.lr if isinstance(self.lr, (tuple, list)) else (self.lr,)
        sd.update({"meta.kind": self.STATE_KIND, "meta.dtype": DTYPE_NAMES[self._state_dtype()], "meta.lr": [float(x) for x in lr],
                   "meta.betas": [float(x) for x in self.betas], "meta.format": STATE_FORMAT})
        return sd

    def load_state_dict(self, sd, _skip_repack=False):
        """``_skip_repack``: test-only -- leaves the packed panels as they are, to show that they are state of their own"""
        validate_state(sd, self.STATE_KIND, self._state_spec())
        if self.inputs is not None:
            # the seed and the sampling mode are host values baked into a captured iteration: they must agree, only the counter moves
            for key, have in (("inputs.seed", int(self.inputs.seed)), ("inputs.sampling", str(self.inputs.sampling)),
                              ("inputs.flip", int(bool(getattr(self.inputs, "flip", False))))):
                if sd[key] != have:
                    raise ValueError(f"{key}: {sd[key]!r} in the state, {have!r} in the attached sampler")
        if self.ema is None:
            # dropping an average silently would be data loss
            if "meta.ema" in sd or any(isinstance(k, str) and k.startswith("ema.") for k in sd):
                raise ValueError("meta.ema: the state carries averaged weights (ema.*), this trainer has none attached: call attach_ema(...) "
                                 f"with (beta, ramp, modules) = {sd.get('meta.ema')!r} before loading")
        else:
            # decay, ramp and the tracked modules are host values baked into a captured iteration, like inputs.seed
            got, have = sd["meta.ema"], self.ema.meta()
            try:
                same = len(got) == 3 and float(got[0]) == have[0] and float(got[1]) == have[1] and list(got[2]) == have[2]
            except (TypeError, ValueError):             # not [number, number, [names]] at all
                same = False
            if not same:
                raise ValueError(f"meta.ema: {got!r} in the state, {have!r} attached")
        torch.cuda.synchronize()
        with torch.no_grad():
            for k, dst in self._state_tensors().items():
                dst.copy_(sd[k].to(dst.dtype))
            if self.inputs is not None:
                self.inputs.step.fill_(int(sd["inputs.step"]))
            if self.log is not None:
                self.log.load(sd["log.head"], sd["log.first_nonfinite"])
            if self.ema is not None:
                self.ema.loaded()
            self._state_zero_scratch()
        if not _skip_repack:
            self._state_repack()
        torch.cuda.synchronize()


class ResidentStep(TrainerState):
    """capture / replay plumbing shared by the small-network trainers (``_step_body`` = one iteration on the static input slots)"""

    inputs = None
    graph = None
    log = None

    def _step_with_inputs(self):
        if self.inputs is not None:
            self.inputs.enqueue(self)
        self._step_body()
        if self.log is not None:                        # behind the body's joins, on the main stream: the row of THIS iteration
            self.log.append()
        if self.ema is not None:                        # behind the joins too: every optimizer lane has written this iteration's weights
            self.ema.update()

    def attach_ema(self, beta=0.999, ramp=0.0, modules=("G",)):
        """Keep an exponential moving average of the weights of ``modules`` (names of ``_state_modules()``): from now on every iteration
        ends with one more launch (WeightEMA.update), and the state carries ``ema.*`` / ``meta.ema``.  Before ``capture()`` only: a
        graph cannot grow a node.  -> the WeightEMA (also ``self.ema``)"""
        if self.graph is not None:
            raise RuntimeError("attach_ema: this trainer's iteration is already captured -- attach the average before capture()")
        have = self._state_modules()
        names = tuple(modules)
        for name in names:
            if name not in have:
                raise ValueError(f"attach_ema: unknown module {name!r} (this trainer has {', '.join(have)})")
        if len(set(names)) != len(names):
            raise ValueError(f"attach_ema: a module is named twice in {names!r}")
        self.ema = WeightEMA({name: have[name] for name in names}, beta, ramp)
        return self.ema

    def capture(self, warmup=False, inputs=None, log=None):
        """Capture the iteration into one hipGraph; with ``inputs`` (a DeviceSampler of this trainer's module) the graph first draws
        the batch on the device, so a replay is a complete loop iteration without host work.  ``log`` (a LossLog): the graph ends with
        the append of the iteration's loss row."""
        if warmup:
            self._step_body()
        if inputs is not None:
            self.inputs = inputs
        if log is not None:
            self.log = log
        return capture_step(self, self._step_with_inputs)

    def step_resident(self):
        check_usable(self)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step_with_inputs()
        return self.losses


class CaptureFailed(RuntimeError):
    """A hipGraph capture of a training iteration failed.  THE PROCESS IS NOT USABLE FOR GPU WORK AFTERWARDS: on ROCm 7.2 every stream
    that was forked into the capture (weight-gradient lanes, optimizer / preparation lanes, a second chain, the input sampler's and a
    collective's internal streams) stays attached to the invalidated capture, and launching on them, destroying them or merely letting
    them be garbage-collected crashes the runtime a little later (observed: SIGSEGV three seconds after an `in-process recovery' that
    restored the stream, drained the sticky error and replaced the lanes -- gpurun_out/r02_z_dp2.err).  There is no in-process
    recovery; the contract is: report the reason and end the process (``engine.exit_after_capture_failure``).  Callers that want an
    eager fallback decide graph-vs-eager BEFORE they touch the GPU, by probing the capture in a child process (bench.py does)."""


def exit_after_capture_failure(exc, code=3):
    """Print the reason and end the process at once (os._exit: no destructors run over streams that still belong to the invalidated
    capture -- that is where the crash comes from)."""
    import sys
    print(f"[ead-gan_amd] hipGraph capture failed: {exc}\n[ead-gan_amd] this process cannot use the GPU any more; exiting with code {code} "
          f"(launch eagerly instead: a trainer without capture(), bench.py --no-graph)", file=sys.stderr, flush=True)
    os._exit(code)


def capture_step(trainer, body):
    """Capture ``body()`` (one whole training iteration) into a hipGraph and store it as ``trainer.graph``.  A capture that fails
    raises :class:`CaptureFailed` and marks the trainer unusable (``step_resident`` refuses to launch): see the exception's text for
    why no eager fallback is offered inside the same process."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            body()
    except Exception as exc:
        trainer.graph = None
        trainer.capture_failed = f"{type(exc).__name__}: {exc}"
        raise CaptureFailed(trainer.capture_failed) from exc
    trainer.graph = graph
    return trainer


def check_usable(trainer):
    why = getattr(trainer, "capture_failed", None)
    if why is not None:
        raise CaptureFailed(f"this trainer's hipGraph capture failed earlier ({why}); the process must not launch GPU work any more")


class ConvRec:
    """One conv-view layer at a fixed batch size: geometry, packed panels, workspace reservations."""

    def __init__(self, dtype, B, H, W, Cin, Cout, k, stride, pad, up=0, device=None, want_fwd=True, want_bwd=True,
                 want_wgrad=True, ws: Workspace | None = None):
        self.dtype = dtype
        self.c = ops.make_conv(B, H, W, Cin, Cout, k, stride, pad, up)
        self.B, self.H, self.W, self.Cin, self.Cout, self.k, self.stride, self.pad = B, H, W, Cin, Cout, k, stride, pad
        self.OH = ((H << up) + 2 * pad - k) // stride + 1
        self.OW = ((W << up) + 2 * pad - k) // stride + 1
        tdt = ops.torch_dtype(dtype)
        self.wp_fwd = torch.empty(ops.pack_fwd_elems(self.c, dtype), device=device, dtype=tdt) if want_fwd else None
        self.wp_bwd = torch.empty(ops.pack_bwd_elems(self.c, dtype), device=device, dtype=tdt) if want_bwd else None
        self.Kpad_fwd = ops.round_up(k * k * Cin, ops.bk(dtype))
        if ws is not None:
            if want_wgrad:
                ws.need_slab(ops.conv_wgrad_ws_bytes(self.c, dtype))
                ws.need_gtmp(Cout * Cin * k * k)
            ws.need_small(ops.bias_grad_ws_floats(B * max(self.OH * self.OW, (H << up) * (W << up)), max(Cin, Cout)))

    def pack(self, w_master):
        if self.wp_fwd is not None or self.wp_bwd is not None:
            ops.pack_conv(self.c, self.dtype, w_master, self.wp_fwd, self.wp_bwd)


class _HipModule(torch.nn.Module):
    """Shared plumbing of the drop-in modules: flat arena, per-batch engines, invalidation when the module is moved."""

    compute_dtype = EG_F32

    def _init_engine_state(self, dtype):
        self.compute_dtype = parse_dtype(dtype)
        self._arena = None
        self._engines = {}

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._arena, self._engines = None, {}
        return out

    @property
    def arena(self) -> Arena:
        if self._arena is None:
            p = next(self.parameters())
            _require_cuda(p)
            self._arena = Arena(self)
            self._engines = {}
        return self._arena

    def set_compute_dtype(self, dtype):
        self.compute_dtype = parse_dtype(dtype)

    def repack(self):
        """Refresh the packed (kernel-layout, compute-dtype) weight panels after the fp32 masters changed."""
        for e in self._engines.values():
            e.repack()

    def fresh_engine(self, B):
        """The engine for batch size B with panels re-packed from the masters: the drop-in forward path.  The kernels read packed
        copies of the convolution weights, and the masters can change behind the module's back in ways nothing reports --
        ``optimizer.step()`` bumps a version counter, ``module.apply(weights_init_normal)`` writes through ``.data`` and does not -- so
        every drop-in forward re-packs first (2 small launches per layer, asynchronous).  The fused trainers keep masters and panels in
        step themselves and never come through here."""
        eng = self.engine(B)
        eng.repack()
        return eng

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self.repack()
        return out


def import_adam_moments(opt, arenas):
    """exp_avg / exp_avg_sq of a ``torch.optim.Adam`` built over the parameters of one or more modules in ``.parameters()`` order (the
    reference's optimizers: celebA/EAD-GAN_celebA.py:211-217, MNIST/EAD-GAN_rpqmnxy.py:206-217, dSprites/rp.py:270-279) into the flat
    moment tensors of a fused trainer.  ``arenas``: [(number of parameters of the module, m, v)] in the optimizer's parameter order.
    Returns the optimizer's step count (0 if it has not stepped yet)."""
    params = opt.param_groups[0]["params"]
    step, i = 0, 0
    for count, m, v in arenas:
        off = 0
        for p in params[i:i + count]:
            st = opt.state.get(p, {})
            n = p.numel()
            if st:
                m[off:off + n].copy_(st["exp_avg"].reshape(-1))
                v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                step = int(st["step"])
            off += n
        assert off == m.numel(), "optimizer parameters do not tile the arena"
        i += count
    assert i == len(params)
    return step

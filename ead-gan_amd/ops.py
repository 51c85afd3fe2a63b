"""Thin torch-tensor front end of the C ABI (include/eadgan_hip.h).

Every function enqueues hand-written HIP kernels on torch's current stream and returns immediately.
torch is used for device memory and streams only.  No function here has a CPU or eager fallback.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, EG_BF16, EG_F16, EG_F32, NT_AUTO, NT_BUF128,
                   NT_PERS, NT_REG, NT_S8, NT_S8H, NT_S8P, OUT_NCHW_F32, OUT_NHWC, STAT_BN_BWD, STAT_MOMENTS, STAT_NONE, STAT_SN_BIAS, EgConv, EgEpilogue,
                   EgEmaSeg, EgHead, EgRngSeg, EgSnLayer, lib)

__all__ = ["EG_F32", "EG_BF16", "EG_F16", "ACT_NONE", "ACT_LRELU", "ACT_RELU", "ACT_TANH", "ACT_SIGMOID", "OUT_NHWC",
           "OUT_NCHW_F32"]


def torch_dtype(dtype: int):
    return {EG_F32: torch.float32, EG_BF16: torch.bfloat16, EG_F16: torch.float16}[dtype]


def vec(dtype: int) -> int:
    return 4 if dtype == EG_F32 else 8


def bk(dtype: int) -> int:
    return 32 if dtype == EG_F32 else 64


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def make_conv(B, H, W, Cin, Cout, k, stride, pad, up=0) -> EgConv:
    return EgConv(B, H, W, Cin, Cout, k, stride, pad, up)


# scratch lent to every conv launch for split-K (engine.Workspace owns and sizes it while engines are built)
SPLITK_WS = {}
SPLITK_OVERRIDE = None          # set while a second chain enqueues its launches (engine.Workspace.active)


def set_splitk_workspace(t):
    SPLITK_WS[t.device.index] = t


def conv_splitk_ws_bytes(c, dtype, bwd):
    return lib().query("eg_conv_splitk_ws_bytes", ctypes.byref(c), dtype, int(bwd))


def epilogue(bias=None, bias_mod=0, sigma=None, act=ACT_NONE, slope=0.0, mask=None, mask_act=ACT_NONE,
             mask_slope=0.0, out_mode=OUT_NHWC, sigma_rows=0, nt_variant=0, nt_splitk=0, splitk_ws="default",
             stat_mode=STAT_NONE, stat_out=None, stat_aux=None, stat_p=(), stat_act=ACT_NONE, stat_slope=0.0) -> EgEpilogue:
    """``nt_variant`` / ``nt_splitk``: per-call kernel hints (NT_* in _lib.py; 0 = the planner decides).  ``splitk_ws``: scratch
    tensor lent for K splits (default: the device's registered workspace; None = never split).  ``stat_*``: column statistics of
    the stored tile fused into the epilogue (eg_epilogue in the header; only where ``conv_stat_blocks`` answers > 0)."""
    ws = splitk_ws
    if isinstance(ws, str):
        ws = SPLITK_OVERRIDE if SPLITK_OVERRIDE is not None else (SPLITK_WS.get(torch.cuda.current_device()) if SPLITK_WS else None)
    sp = [_p(t) for t in stat_p] + [None] * (4 - len(stat_p))
    return EgEpilogue(_p(bias), bias_mod, _p(sigma), act, slope, _p(mask), mask_act, mask_slope, out_mode, sigma_rows,
                      _p(ws), ws.numel() * ws.element_size() if ws is not None else 0, nt_variant, nt_splitk,
                      stat_mode, _p(stat_out), _p(stat_aux), sp[0], sp[1], sp[2], sp[3], stat_act, stat_slope)


def nt_tile(c, dtype, bwd, ep=None) -> int:
    """BM * 1000 + kernel code of the kernel THIS call (its hints, its split-K scratch) is dispatched to (eg_igemm_nt_tile in the header)"""
    if ep is None:
        ep = epilogue()
    return lib().query("eg_igemm_nt_tile_ep", ctypes.byref(c), dtype, int(bwd), ctypes.byref(ep))


def nt_tile_hinted(c, dtype, bwd, variant=0, splitk=0) -> int:
    """the same label for the bare hints, with unlimited split-K scratch (profiling labels and the kernel tests); -1 = ``variant`` cannot run it"""
    return lib().query("eg_igemm_nt_tile", ctypes.byref(c), dtype, int(bwd), variant, splitk)


def conv_stat_blocks(c, dtype, bwd, ep=None) -> int:
    """row blocks of the fused column statistics this exact call (geometry, hints, scratch of ``ep``) would write; 0 = it cannot fuse them"""
    if ep is None:
        ep = epilogue()
    return lib().query("eg_conv_stat_blocks", ctypes.byref(c), dtype, int(bwd), ctypes.byref(ep))


# ---- implicit-GEMM family ------------------------------------------------------------------------
def pack_fwd_elems(c, dtype):
    return lib().query("eg_pack_fwd_elems", ctypes.byref(c), dtype)


def pack_bwd_elems(c, dtype):
    return lib().query("eg_pack_bwd_elems", ctypes.byref(c), dtype)


def pack_fwd(c, dtype, w_master, wp):
    lib().call("eg_pack_fwd", ctypes.byref(c), dtype, _p(w_master), _p(wp), _stream())


def pack_bwd(c, dtype, w_master, wp):
    lib().call("eg_pack_bwd", ctypes.byref(c), dtype, _p(w_master), _p(wp), _stream())


def pack_conv(c, dtype, w_master, wp_fwd, wp_bwd):
    lib().call("eg_pack_conv", ctypes.byref(c), dtype, _p(w_master), _p(wp_fwd), _p(wp_bwd), _stream())


def pack_strided(dtype, w, wp, N, K, Kpad, n_div, s_hi, s_lo, s_k):
    lib().call("eg_pack_strided", dtype, _p(w), _p(wp), N, K, Kpad, n_div, s_hi, s_lo, s_k, _stream())


def pack_strided2(dtype, w, wp, N, K, Kpad, n_div, s_hi, s_lo, k_div, s_khi, s_klo):
    lib().call("eg_pack_strided2", dtype, _p(w), _p(wp), N, K, Kpad, n_div, s_hi, s_lo, k_div, s_khi, s_klo, _stream())


def linear_dinput_ws_floats(B, NI, NJ, K) -> int:
    """floats of split scratch ``linear_dinput`` needs for this shape (0: one split, the result is stored directly)"""
    return lib().query("eg_linear_dinput_ws_floats", B, NI, NJ, K)


def linear_dinput(dtype, dH, ldh, w, dX, B, NI, NJ, K, s_i, s_j, s_k, ws=None):
    """dX[b][k] = sum_ij dH[b][i*NJ + j] * w[i*s_i + j*s_j + k*s_k]: the input gradient of a first layer from its fp32 master ``w``
    (argument style of ``pack_strided``; ``ws``: fp32 scratch of at least ``linear_dinput_ws_floats`` elements)"""
    lib().call("eg_linear_dinput", dtype, _p(dH), ldh, _p(w), _p(dX), B, NI, NJ, K, s_i, s_j, s_k, _p(ws), ws.numel() if ws is not None else 0, _stream())


# Optional launch recorder (bench.py's roofline pass): when set to a list, every implicit-GEMM launch is bracketed by HIP
# events on the launch stream and appends (kernel label, algorithmic FLOPs, start event, end event, shape string).
# Never set on the training path.
RECORDER = None


_SPACER_CYCLES = None


def _spacer(us=25.0):
    """A spin kernel of ~25 us in front of a timed launch (torch.cuda._sleep, calibrated once): the start event, the launch and the end event
    are enqueued while the GPU is still spinning, so the bracket holds the kernel and not the host's launch time -- eager launches behind a
    run of short kernels find the GPU idle otherwise (bench.py's table read 77 us for a 44 us launch, profiles/r03_no_overlap_gemm_by_grid.txt).
    It touches no memory: the cache state the timed kernel sees is the step's own."""
    global _SPACER_CYCLES
    if _SPACER_CYCLES is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(100000)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(1000000)
        b.record()
        torch.cuda.synchronize()
        _SPACER_CYCLES = max(1000, int(us * 1e-3 * 1000000 / max(a.elapsed_time(b), 1e-3)))
    torch.cuda._sleep(_SPACER_CYCLES)


def _out_hw(c):
    return ((c.H << c.up) + 2 * c.pad - c.k) // c.stride + 1, ((c.W << c.up) + 2 * c.pad - c.k) // c.stride + 1


def _timed(kind, c, dtype, args, ep=None):
    """RECORDER entry: (kernel label, algorithmic FLOPs, start event, end event, shape string, algorithmic bytes).  Algorithmic bytes =
    every input element, weight and output element of the launch once, in its storage type (plus the activation-gradient mask the
    epilogue reads): what the launch would move with perfect reuse."""
    oh, ow = _out_hw(c)
    M = c.B * oh * ow
    flops = 2.0 * M * c.Cout * c.Cin * c.k * c.k
    es = 4 if dtype == EG_F32 else 2
    x_elems, y_elems, w_elems = c.B * c.H * c.W * c.Cin, M * c.Cout, c.Cout * c.Cin * c.k * c.k
    tname = {EG_F32: "float", EG_BF16: "bf16", EG_F16: "f16"}[dtype]
    if kind == "tn":
        label = f"igemm_tn8_kernel<{tname}>" if lib().query("eg_conv_wgrad_variant", ctypes.byref(c), dtype) == 2 else f"igemm_tn_kernel<{tname}>"
        nbytes = (x_elems + y_elems) * es + w_elems * 4                     # activations + output gradients in, fp32 weight gradient out
    else:
        tile = nt_tile(c, dtype, kind == "bwd", ep)
        bm, bn = tile // 1000, tile % 1000
        label = {131: f"igemm_nt_buf_kernel<{tname}>", 132: f"igemm_nt_buf_kernel<{tname}>+splitk",
                 135: f"igemm_nt_pers_kernel<{tname}>",
                 147: f"igemm_nt8s_kernel<{tname},im2col>", 148: f"igemm_nt8s_kernel<{tname},im2col>+splitk",
                 149: f"igemm_nt8s_kernel<{tname},patch>", 150: f"igemm_nt8s_kernel<{tname},patch>+splitk",
                 151: f"igemm_nt8h_kernel<{tname}>", 152: f"igemm_nt8h_kernel<{tname}>+splitk"}.get(bn, f"igemm_nt_kernel<{tname},{bm},{bn}>")
        nbytes = (x_elems + y_elems + w_elems) * es
        if ep is not None and ep.mask:
            nbytes += (x_elems if kind == "bwd" else y_elems) * es
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    _spacer()
    e0.record()
    lib().call(*args, _stream())
    e1.record()
    RECORDER.append((label, flops, e0, e1, f"{kind} B{c.B} H{c.H} Cin{c.Cin} Cout{c.Cout} k{c.k} s{c.stride}", float(nbytes)))


def conv_fwd(c, dtype, X, wp, Y, ep=None):
    if ep is None:
        ep = epilogue()          # carries the split-K scratch
    args = ("eg_conv_fwd", ctypes.byref(c), dtype, _p(X), _p(wp), _p(Y), ctypes.byref(ep) if ep is not None else None)
    if RECORDER is not None:
        return _timed("fwd", c, dtype, args, ep)
    lib().call(*args, _stream())


def conv_bwd_data(c, dtype, dY, wp, dX, ep=None):
    if ep is None:
        ep = epilogue()
    args = ("eg_conv_bwd_data", ctypes.byref(c), dtype, _p(dY), _p(wp), _p(dX), ctypes.byref(ep) if ep is not None else None)
    if RECORDER is not None:
        return _timed("bwd", c, dtype, args, ep)
    lib().call(*args, _stream())


def conv_wgrad_ws_bytes(c, dtype):
    return lib().query("eg_conv_wgrad_ws_bytes", ctypes.byref(c), dtype)


def conv_wgrad(c, dtype, X, dY, slab, wgs_target=0) -> int:
    """``wgs_target``: workgroups the parity-class kernel aims for (0: one per CU; 128 for launches forked beside the main chain)"""
    ns = ctypes.c_int(0)
    args = ("eg_conv_wgrad", ctypes.byref(c), dtype, _p(X), _p(dY), _p(slab), ctypes.addressof(ns), wgs_target)
    if RECORDER is not None:
        _timed("tn", c, dtype, args)
    else:
        lib().call(*args, _stream())
    return ns.value


def conv_wgrad_variant(c, dtype) -> int:
    """2: the parity-class kernel (igemm_tn8) runs this weight gradient, 1: the per-tap kernel"""
    return lib().query("eg_conv_wgrad_variant", ctypes.byref(c), dtype)


# Gradient writers take ``accumulate``: True adds to the slot (autograd's .grad contract, the default), False stores the value that would
# have been added and never reads the slot (include/eadgan_hip.h, "gradient writers with a store mode").
def wgrad_reduce(slab, nsplit, n_slab, n_rows, C, T, grad, accumulate=True):
    lib().call("eg_wgrad_reduce", _p(slab), nsplit, n_slab, n_rows, C, T, _p(grad), int(accumulate), _stream())


def wgrad_reduce_perm(slab, nsplit, n_slab, n_rows, C, T, grad, row_div=0, row_mul=0, c_row=0, accumulate=True):
    lib().call("eg_wgrad_reduce_perm", _p(slab), nsplit, n_slab, n_rows, C, T, _p(grad), row_div, row_mul, c_row, int(accumulate), _stream())


def gather_add(out, src, n, div, s_div, s_mod):
    lib().call("eg_gather_add", _p(out), _p(src), n, div, s_div, s_mod, _stream())


def sumpool2x2(dtype, x, y, B, H, W, C):
    lib().call("eg_sumpool2x2", dtype, _p(x), _p(y), B, H, W, C, _stream())


def wgrad_c1_ok(dtype, C, H, W, Cout, k, stride, pad) -> bool:
    return bool(lib().query("eg_wgrad_c1_ok", dtype, C, H, W, Cout, k, stride, pad))


def wgrad_c1_splits(B, H) -> int:
    return lib().query("eg_wgrad_c1_splits", B, H)


def wgrad_c1(dtype, x, dy, slab, B, H, W, C) -> int:
    """weight gradient of Conv2d(64, 1, 3, 1, 1) with the activation read once -> number of slabs [split][9][64] in ``slab``"""
    ns = ctypes.c_int(0)
    lib().call("eg_wgrad_c1", dtype, _p(x), _p(dy), _p(slab), B, H, W, C, ctypes.byref(ns), _stream())
    return ns.value


def up3_expand(w3, w4t, Cout, Cin):
    """effective ConvTranspose2d(4, 2, 1) master [Cin][Cout][4][4] of Upsample(2) + Conv2d(Cin -> Cout, 3, 1, 1) (MNIST/EAD-GAN_rpqmnxy.py:81-82)"""
    lib().call("eg_up3_expand", _p(w3), _p(w4t), Cout, Cin, _stream())


def up3_contract(dw4t, dw3, Cout, Cin, accumulate=True):
    """the transposed convolution's weight gradient [Cin][Cout][4][4] back onto the 3x3 master's gradient [Cout][Cin][3][3]"""
    lib().call("eg_up3_contract", _p(dw4t), _p(dw3), Cout, Cin, int(accumulate), _stream())


def sn_partials():
    return lib().query("eg_sn_partials")


def wgrad_reduce_sn(c, slab, nsplit, w_orig, sigma, u, v, gtmp, partials, grad, accumulate=True):
    lib().call("eg_wgrad_reduce_sn", ctypes.byref(c), _p(slab), nsplit, _p(w_orig), _p(sigma), _p(u), _p(v), _p(gtmp), _p(partials), _p(grad),
               int(accumulate), _stream())


def bias_grad_ws_floats(rows, N):
    return lib().query("eg_bias_grad_ws_floats", rows, N)


def bias_grad(dtype, dY, rows, N, partials, gb, bias_mod=0, accumulate=True):
    lib().call("eg_bias_grad", dtype, _p(dY), rows, N, bias_mod, _p(partials), _p(gb), int(accumulate), _stream())


def bias_grad_sn_ws_floats(rows, N, rows_per_tape):
    return lib().query("eg_bias_grad_sn_ws_floats", rows, N, rows_per_tape)


def bias_grad_sn(dtype, dzs, a, bias, rows, N, rows_per_tape, sigma, slope, ws, gb, coef, accumulate=True):
    lib().call("eg_bias_grad_sn", dtype, _p(dzs), _p(a), _p(bias), rows, N, rows_per_tape, _p(sigma), slope, _p(ws), _p(gb), _p(coef),
               int(accumulate), _stream())


def bias_grad_sn_fused(stat, nrb, N, tiles_m, tiles_per_tape, ntapes, sigma, gb, coef, accumulate=True):
    lib().call("eg_bias_grad_sn_fused", _p(stat), nrb, N, tiles_m, tiles_per_tape, ntapes, _p(sigma), _p(gb), _p(coef), int(accumulate), _stream())


def wgrad_reduce_rank1(slab, nsplit, n_slab, n_rows, C, T, grad, ntapes, coef, u, v, c_row=0, accumulate=True):
    lib().call("eg_wgrad_reduce_rank1", _p(slab), nsplit, n_slab, n_rows, C, T, _p(grad), ntapes, _p(coef), _p(u), _p(v), c_row, int(accumulate),
               _stream())


# ---- image side / heads ----------------------------------------------------------------------------
def conv_img_fwd(dtype, img, w_master, out, B, CI, H, W, N, k, stride, pad, ep=None):
    lib().call("eg_conv_img_fwd", dtype, _p(img), _p(w_master), _p(out), B, CI, H, W, N, k, stride, pad,
               ctypes.byref(ep) if ep is not None else None, _stream())


def conv_img_wgrad_ws_bytes(B, CI, N, k):
    return lib().query("eg_conv_img_wgrad_ws_bytes", B, CI, N, k)


def conv_img_wgrad(dtype, dz, img, slab, B, CI, H, W, N, k, stride, pad):
    lib().call("eg_conv_img_wgrad", dtype, _p(dz), _p(img), _p(slab), B, CI, H, W, N, k, stride, pad, _stream())


def im2col_img(dtype, img, out, B, CI, H, W, k, stride, pad, Kp):
    lib().call("eg_im2col_img", dtype, _p(img), _p(out), B, CI, H, W, k, stride, pad, Kp, _stream())


def conv_img_mfma_ok(dtype, C, H, W, N, k, stride, pad) -> bool:
    return bool(lib().query("eg_conv_img_mfma_ok", dtype, C, H, W, N, k, stride, pad))


def conv_img_mfma_stat_blocks(B, H, W, ntapes=1) -> int:
    return lib().query("eg_conv_img_mfma_stat_blocks", B, H, W, ntapes)


def conv_img_mfma(dtype, imgs, wp, out, B, C, H, W, ep=None, gates=None, gate_act=ACT_NONE, gate_slope=0.0, N=128):
    """Conv2d(C -> N = 128 / 64 / 32, 4, 2, 1) of up to three fp32 NCHW image tensors (tapes) straight on the MFMA units, no patch rows in HBM"""
    im = [_p(t) for t in imgs] + [None] * (3 - len(imgs))
    ga = [_p(t) for t in (gates or [])] + [None] * (3 - len(gates or []))
    lib().call("eg_conv_img_mfma", dtype, im[0], im[1], im[2], ga[0], ga[1], ga[2], len(imgs), _p(wp), _p(out), B, C, H, W, N,
               ctypes.byref(ep) if ep is not None else None, gate_act, gate_slope, _stream())


def wgrad_img_ok(dtype, C, H, W, N, k, stride, pad) -> bool:
    return bool(lib().query("eg_wgrad_img_ok", dtype, C, H, W, N, k, stride, pad))


def wgrad_img_splits(images, N=32) -> int:
    return lib().query("eg_wgrad_img_splits", images, N)


def wgrad_img(dtype, imgs, P, slab, B, C, H, W, N) -> int:
    """weight gradient of an image-side 4x4 / stride-2 layer straight from the fp32 images of up to three tapes (no patch rows in HBM) ->
    number of slabs [N][16 C] written to ``slab``"""
    im = [_p(t) for t in imgs] + [None] * (3 - len(imgs))
    ns = ctypes.c_int(0)
    lib().call("eg_wgrad_img", dtype, im[0], im[1], im[2], len(imgs), _p(P), _p(slab), B, C, H, W, N, ctypes.byref(ns), _stream())
    return ns.value


def wgrad_img_tn_ok(dtype, C, H, W, N, k, stride, pad) -> bool:
    return bool(lib().query("eg_wgrad_img_tn_ok", dtype, C, H, W, N, k, stride, pad))


def wgrad_img_tn_plan(images, C, wgs_target=0):
    """(splits, rows per split) of a ``wgrad_img_tn`` launch over ``images`` = tapes x batch images: the per-tap kernel's plan for their patch rows"""
    rps = ctypes.c_int(0)
    return lib().query("eg_wgrad_img_tn_plan", images, C, wgs_target, ctypes.byref(rps)), rps.value


def wgrad_img_tn(dtype, imgs, P, slab, B, C, H, W, N=128, wgs_target=0) -> int:
    """weight gradient of a CelebA image-side layer straight from the fp32 images of up to three tapes, the bits of ``im2col_img`` (Kp = 16 C) +
    ``conv_wgrad`` over the patch rows -> number of slabs [N][16 C] written to ``slab``.  ``wgs_target``: 0 = the split plan ``conv_wgrad``
    uses for those rows, > 0 = that many splits"""
    im = [_p(t) for t in imgs] + [None] * (3 - len(imgs))
    ns = ctypes.c_int(0)
    args = ("eg_wgrad_img_tn", dtype, im[0], im[1], im[2], len(imgs), _p(P), _p(slab), B, C, H, W, N, wgs_target, ctypes.addressof(ns))
    if RECORDER is None:
        lib().call(*args, _stream())
        return ns.value
    M = len(imgs) * B * (H // 2) * (W // 2)
    tname = {EG_BF16: "bf16", EG_F16: "f16"}[dtype]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    _spacer()
    e0.record()
    lib().call(*args, _stream())
    e1.record()
    # fp32 images + P in, fp32 weight gradient out
    RECORDER.append((f"wgrad_img_tn_kernel<{tname}>", 2.0 * M * N * 16 * C, e0, e1, f"tn_img B{len(imgs) * B} H{H} C{C} N{N}",
                     float(len(imgs) * B * C * H * W * 4 + M * N * 2 + N * 16 * C * 4)))
    return ns.value


def convt_img_mfma_ok(dtype, C, Hin, Win, K, k, stride, pad) -> bool:
    return bool(lib().query("eg_convt_img_mfma_ok", dtype, C, Hin, Win, K, k, stride, pad))


def convt_img_mfma(dtype, a, wp, bias, out, B, C, Hin, Win, act=ACT_NONE, slope=0.0, K=128):
    """ConvTranspose2d(K = 128 / 64 -> C <= 3, 4, 2, 1) (+ bias + activation) from 16-bit NHWC activations to an fp32 NCHW image in one launch"""
    lib().call("eg_convt_img_mfma", dtype, _p(a), _p(wp), _p(bias), _p(out), B, C, Hin, Win, K, act, slope, _stream())


def cast_pad(dtype, src, dst, rows, n, npad):
    lib().call("eg_cast_pad", dtype, _p(src), _p(dst), rows, n, npad, _stream())


def act_grad_mul_bias_nchw(g, a, out, B, C, HW, act, slope, partial, gb, accumulate=True):
    lib().call("eg_act_grad_mul_bias_nchw", _p(g), _p(a), _p(out), B, C, HW, act, slope, _p(partial), _p(gb), int(accumulate), _stream())


def head_fused_ok(dtype, T, K, N):
    return bool(lib().cdll.eg_head_fused_ok(dtype, T, K, N))


class PackBatch:
    """The pack launches issued by ``fn()`` as ONE launch (eg_pack_record_begin / _end / eg_pack_multi).  Eager calls record again (host
    work only) and re-upload the job table if a pointer or a geometry changed; inside a hipGraph capture the table of the last eager call
    is launched as it is (the capture contract: an eager iteration has run on the same buffers)."""
    MAX_JOBS = 64

    def __init__(self):
        self.host = None
        self.dev = None
        self.n = self.nb = 0

    def run(self, fn):
        if not (self.dev is not None and torch.cuda.is_current_stream_capturing()):
            jb = lib().cdll.eg_pack_job_bytes()
            cap = self.MAX_JOBS * jb
            buf = ctypes.create_string_buffer(cap)
            n, nb = ctypes.c_int(0), ctypes.c_int(0)
            lib().call("eg_pack_record_begin")
            try:
                fn()
            finally:
                lib().call("eg_pack_record_end", buf, cap, ctypes.byref(n), ctypes.byref(nb))
            host = buf.raw[:n.value * jb]
            if host != self.host:
                self.host, self.n, self.nb = host, n.value, nb.value
                self.dev = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(torch.device("cuda", torch.cuda.current_device())) if host else None
        if self.dev is not None and self.n:
            lib().call("eg_pack_multi", _p(self.dev), self.n, self.nb, _stream())


def batched_packs(fn):
    """decorator of an engine's ``repack...`` method: its pack launches run as one (PackBatch per method and argument tuple)"""
    def wrapper(self, *a):
        batches = self.__dict__.setdefault("_pack_batches", {})
        key = (fn.__name__,) + a
        b = batches.get(key)
        if b is None:
            b = batches[key] = PackBatch()
        return b.run(lambda: fn(self, *a))
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


def dense_small_fwd_slices(dtype, x, wp, B, K, Kpad, N, ws):
    """the K-slice sums of dense_small_fwd (no combine launch) -> number of slices in ``ws`` [slice][B][N]"""
    ns = ctypes.c_int(0)
    lib().call("eg_dense_small_fwd_slices", dtype, _p(x), _p(wp), B, K, Kpad, N, _p(ws), ws.numel(), ctypes.byref(ns), _stream())
    return ns.value


def head_fused(dtype, x, wp, bias, partials, nslice, y, dout, dx, sigma, B, T, K, Kpad, N, loss, terms, counter, mask_act, mask_slope, targets=None,
               scales=None, info=None):
    """Behind dense_small_fwd_slices: slice combine, losses and head input gradient of the T rows of every sample in one launch
    (eg_head_fused).  ``targets`` / ``scales``: the adversarial BCE term of each tape; ``info`` = (c_cont, n_cont, n_cat, code, labels, lcat,
    lcon, laff): the info step's three losses (tapes: generated, transformed, real)."""
    h = EgHead()
    h.x, h.wp, h.bias, h.y, h.dout, h.dx, h.sigma = _p(x), _p(wp), _p(bias), _p(y), _p(dout), _p(dx), _p(sigma)
    h.partials, h.nslice = _p(partials), nslice
    h.B, h.T, h.K, h.Kpad, h.N = B, T, K, Kpad, N
    h.loss, h.terms, h.counter, h.mask_act, h.mask_slope = _p(loss), _p(terms), _p(counter), mask_act, float(mask_slope)
    if info is None:
        h.mode = 0
        for t in range(T):
            h.target[t], h.scale[t] = float(targets[t]), float(scales[t])
    else:
        h.mode = 1
        c_cont, n_cont, n_cat, code, labels, lcat, lcon, laff = info
        h.c_cont, h.n_cont, h.n_cat, h.code, h.ldc, h.labels = c_cont, n_cont, n_cat, _p(code), code.stride(0), _p(labels)
        h.lcat, h.lcon, h.laff = float(lcat), float(lcon), float(laff)
    lib().call("eg_head_fused", dtype, ctypes.byref(h), _stream())


def dense_small_bgrad(dy, gb, B, N, accumulate=True):
    lib().call("eg_dense_small_bgrad", _p(dy), _p(gb), B, N, int(accumulate), _stream())


def flat_reduce(slab, nslab, total, grad, accumulate=True):
    lib().call("eg_flat_reduce", _p(slab), nslab, total, _p(grad), int(accumulate), _stream())


def dense_small_fwd(dtype, x, wp, bias, y, B, K, Kpad, N, ws=None):
    lib().call("eg_dense_small_fwd", dtype, _p(x), _p(wp), _p(bias), _p(y), B, K, Kpad, N, _p(ws), ws.numel() if ws is not None else 0, _stream())


def dense_small_fwd_sn(dtype, x, wp, bias, y, B, K, Kpad, N, sigma, sigma_rows, ws=None):
    lib().call("eg_dense_small_fwd_sn", dtype, _p(x), _p(wp), _p(bias), _p(y), B, K, Kpad, N, _p(sigma), sigma_rows,
               _p(ws), ws.numel() if ws is not None else 0, _stream())


def head_prep_sn(dtype, dy, ldy, y, ldyy, bias, rows, N, sigma, rows_per_tape, dys, npad, col0, gb, coef, dys32=None, ld32=0):
    lib().call("eg_head_prep_sn", dtype, _p(dy), ldy, _p(y), ldyy, _p(bias), rows, N, _p(sigma), rows_per_tape, _p(dys), npad, col0, _p(gb), _p(coef),
               _p(dys32), ld32, _stream())


def dense_small_bwd(dtype, dy, wp, mask, dx, B, K, Kpad, N, mask_act=ACT_NONE, mask_slope=0.0, sigma=None, sigma_rows=0):
    lib().call("eg_dense_small_bwd", dtype, _p(dy), _p(wp), _p(mask), _p(dx), B, K, Kpad, N, mask_act, mask_slope, _p(sigma), sigma_rows, _stream())


def dense_small_wgrad(dtype, dy, x, gw, gb, B, K, N, Cin, taps):
    lib().call("eg_dense_small_wgrad", dtype, _p(dy), _p(x), _p(gw), _p(gb), B, K, N, Cin, taps, _stream())


# ---- norm / spectral norm / optimiser -----------------------------------------------------------------
def bn_ws_floats(M, C):
    return lib().query("eg_bn_ws_floats", M, C)


def bn_fwd_eval(dtype, x, y, M, C, gamma, beta, eps, running_mean, running_var, ws, act=ACT_NONE, slope=0.0):
    lib().call("eg_bn_fwd_eval", dtype, _p(x), _p(y), M, C, _p(gamma), _p(beta), float(eps), _p(running_mean), _p(running_var), _p(ws),
               act, float(slope), _stream())


def bn_bwd_eval(dtype, z, da, dz, M, C, gamma, beta, eps, running_mean, running_var, ws, act=ACT_NONE, slope=0.0):
    """backward of ``bn_fwd_eval`` with respect to its input (elementwise; no parameter gradients)"""
    lib().call("eg_bn_bwd_eval", dtype, _p(z), _p(da), _p(dz), M, C, _p(gamma), _p(beta), float(eps), _p(running_mean), _p(running_var), _p(ws),
               act, float(slope), _stream())


def bn_stats_local(dtype, x, M, C, ws, stats):
    lib().call("eg_bn_stats_local", dtype, _p(x), M, C, _p(ws), _p(stats), _stream())


def bn_fwd_from_stats(dtype, x, y, M_local, C, stats_all, nranks, M_global, gamma, beta, eps, momentum, rmean, rvar, nbt, save_mean, save_invstd, ws,
                      act=ACT_NONE, slope=0.0):
    lib().call("eg_bn_fwd_from_stats", dtype, _p(x), _p(y), M_local, C, _p(stats_all), nranks, M_global, _p(gamma), _p(beta), float(eps),
               float(momentum if momentum is not None else 0.1), _p(rmean), _p(rvar), _p(nbt), _p(save_mean), _p(save_invstd), _p(ws), act, float(slope),
               _stream())


def bn_bwd_sums_local(dtype, z, da, M, C, gamma, beta, save_mean, save_invstd, act, slope, dgamma, dbeta, sums, ws, accumulate=True):
    lib().call("eg_bn_bwd_sums_local", dtype, _p(z), _p(da), M, C, _p(gamma), _p(beta), _p(save_mean), _p(save_invstd), act, float(slope),
               _p(dgamma), _p(dbeta), _p(sums), _p(ws), int(accumulate), _stream())


def bn_bwd_from_sums(dtype, z, da, dz, M_local, C, sums_global, M_global, gamma, beta, save_mean, save_invstd, act, slope, ws):
    lib().call("eg_bn_bwd_from_sums", dtype, _p(z), _p(da), _p(dz), M_local, C, _p(sums_global), M_global, _p(gamma), _p(beta), _p(save_mean),
               _p(save_invstd), act, float(slope), _p(ws), _stream())


def bn_fwd_train(dtype, x, y, M, C, gamma, beta, eps, momentum, rmean, rvar, nbt, save_mean, save_invstd, ws, act=ACT_NONE, slope=0.0):
    lib().call("eg_bn_fwd_train", dtype, _p(x), _p(y), M, C, _p(gamma), _p(beta), eps, momentum, _p(rmean), _p(rvar), _p(nbt),
               _p(save_mean), _p(save_invstd), _p(ws), act, slope, _stream())


def bn_fwd_train_fused(dtype, x, y, M, C, stat, nrb, rows_per_block, gamma, beta, eps, momentum, rmean, rvar, nbt, save_mean, save_invstd, ws,
                       act=ACT_NONE, slope=0.0):
    lib().call("eg_bn_fwd_train_fused", dtype, _p(x), _p(y), M, C, _p(stat), nrb, rows_per_block, _p(gamma), _p(beta), eps, momentum, _p(rmean), _p(rvar),
               _p(nbt), _p(save_mean), _p(save_invstd), _p(ws), act, slope, _stream())


def bn_bwd_fused(dtype, z, dy, dz, M, C, stat, nrb, gamma, beta, save_mean, save_invstd, dgamma, dbeta, sums, ws, accumulate=True):
    lib().call("eg_bn_bwd_fused", dtype, _p(z), _p(dy), _p(dz), M, C, _p(stat), nrb, _p(gamma), _p(beta), _p(save_mean), _p(save_invstd),
               _p(dgamma), _p(dbeta), _p(sums), _p(ws), int(accumulate), _stream())


def bn_bwd(dtype, z, da, dz, M, C, gamma, beta, save_mean, save_invstd, act, slope, dgamma, dbeta, sums, ws, accumulate=True):
    lib().call("eg_bn_bwd", dtype, _p(z), _p(da), _p(dz), M, C, _p(gamma), _p(beta), _p(save_mean), _p(save_invstd), act, slope,
               _p(dgamma), _p(dbeta), _p(sums), _p(ws), int(accumulate), _stream())


def bn_bwd_post(dtype, z, da, dz, M, C, gamma, beta, save_mean, save_invstd, dgamma, dbeta, sums, ws, post_act, post_slope, post_sigma):
    lib().call("eg_bn_bwd_post", dtype, _p(z), _p(da), _p(dz), M, C, _p(gamma), _p(beta), _p(save_mean), _p(save_invstd), _p(dgamma), _p(dbeta),
               _p(sums), _p(ws), post_act, post_slope, _p(post_sigma), _stream())


def sn_ws_floats(R, Kd):
    return lib().query("eg_sn_ws_floats", R, Kd)


def sn_power_iter(w_orig, R, Kd, u, v, sigma, u_snap, v_snap, ws, training=True, eps=1e-12):
    lib().call("eg_sn_power_iter", _p(w_orig), R, Kd, _p(u), _p(v), _p(sigma), _p(u_snap), _p(v_snap), _p(ws), int(training), eps, _stream())


def sn_layers(entries):
    """entries: list of (w_orig, u, v, sigma, u_snap, v_snap) tensors -> ctypes array of eg_sn_layer (keep it alive)."""
    arr = (EgSnLayer * len(entries))()
    for i, (w, u, v, sg, us, vs) in enumerate(entries):
        arr[i] = EgSnLayer(_p(w), _p(u), _p(v), _p(sg), _p(us), _p(vs), w.shape[0], w.numel() // w.shape[0])
    return arr


def sn_multi_ws_floats(arr):
    return lib().query("eg_sn_multi_ws_floats", arr, len(arr))


def sn_power_iter_multi(arr, ws, training=True, eps=1e-12):
    lib().call("eg_sn_power_iter_multi", arr, len(arr), _p(ws), int(training), eps, _stream())


def adam_step(p, g, m, v, n, lr, b1, b2, eps, step, tick=True):
    lib().call("eg_adam_step", _p(p), _p(g), _p(m), _p(v), n, lr, b1, b2, eps, _p(step), int(tick), _stream())


def adam_step_zero(p, g, m, v, n, lr, b1, b2, eps, step, tick=True, zero_grad=False):
    """Adam on a slice (views of the arena tensors), optionally clearing the gradient slice in the same pass"""
    lib().call("eg_adam_step_zero", _p(p), _p(g), _p(m), _p(v), n, lr, b1, b2, eps, _p(step), int(tick), int(zero_grad), _stream())


def adam_tick(step):
    lib().call("eg_adam_tick", _p(step), _stream())


def adam_pack_conv_ok(c, dtype, has_fwd, has_bwd) -> bool:
    return bool(lib().query("eg_adam_pack_conv_ok", ctypes.byref(c), dtype, int(has_fwd), int(has_bwd)))


def adam_pack_conv(c, dtype, p, g, m, v, lr, b1, b2, eps, step, wp_fwd, wp_bwd):
    """optimizer.step() on one convolution weight (slices of the four arenas) + refresh of its packed panels, one launch"""
    lib().call("eg_adam_pack_conv", ctypes.byref(c), dtype, _p(p), _p(g), _p(m), _p(v), lr, b1, b2, eps, _p(step), _p(wp_fwd), _p(wp_bwd), _stream())


def adam_pack_rows(dtype, p, g, m, v, wp, K, N, Kpad, n_mod, n_mul, lr, b1, b2, eps, step):
    lib().call("eg_adam_pack_rows", dtype, _p(p), _p(g), _p(m), _p(v), _p(wp), K, N, Kpad, n_mod, n_mul, lr, b1, b2, eps, _p(step), _stream())


def clear_errors():
    return lib().query("eg_clear_errors")


def fill_f32(t, val=0.0):
    lib().call("eg_fill_f32", _p(t), t.numel(), val, _stream())


# ---- utilities ------------------------------------------------------------------------------------------
def concat_cast(dtype, a, b, c, out, B, Cpad):
    wa = a.shape[1]
    wb = b.shape[1] if b is not None else 0
    wc = c.shape[1] if c is not None else 0
    lib().call("eg_concat_cast", dtype, _p(a), wa, _p(b), wb, _p(c), wc, B, Cpad, _p(out), _stream())


# ---- affine / warp / losses --------------------------------------------------------------------------------
def theta_rpqxy(code, ldc, B, theta):
    lib().call("eg_theta_rpqxy", _p(code), ldc, B, _p(theta), _stream())


def warp_affine(img, theta, out, B, C, H, W):
    lib().call("eg_warp_affine", _p(img), _p(theta), _p(out), B, C, H, W, _stream())


def warp_affine_rpqxy(img, code, ldc, theta_out, out, B, C, H, W, zero=None):
    """theta_rpqxy + warp_affine in one launch; ``zero``: a small fp32 tensor the launch clears first"""
    lib().call("eg_warp_affine_rpqxy", _p(img), _p(code), ldc, _p(theta_out), _p(out), B, C, H, W, _p(zero), zero.numel() if zero is not None else 0, _stream())


def mlp_rpqmnxy_floats():
    return lib().query("eg_mlp_rpqmnxy_floats")


def theta_rpqmnxy(code, ldc, B, theta):
    lib().call("eg_theta_rpqmnxy", _p(code), ldc, B, _p(theta), _stream())


def loss_affine_rpqmnxy(o_real, o_trans, ld, c0, B, code, ldc, mlp, scale, loss, d_real, d_trans, pred_out, ws):
    lib().call("eg_loss_affine_rpqmnxy", _p(o_real), _p(o_trans), ld, c0, B, _p(code), ldc, _p(mlp), scale, _p(loss), _p(d_real), _p(d_trans),
               _p(pred_out), _p(ws), _stream())


def theta_rp(code, ldc, B, theta):
    lib().call("eg_theta_rp", _p(code), ldc, B, _p(theta), _stream())


def theta_pxy_align_inv(code, ldc, B, theta):
    lib().call("eg_theta_pxy_align_inv", _p(code), ldc, B, _p(theta), _stream())


def loss_affine_rp(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred_out=None):
    lib().call("eg_loss_affine_rp", _p(o_real), _p(o_trans), ld, c0, B, _p(code), ldc, scale, _p(loss), _p(d_real), _p(d_trans), _p(pred_out), _stream())


def loss_mutual_info(o, ld, c0, n, B, tgt, ldt, t0, target_logits, scale, loss, dout):
    lib().call("eg_loss_mutual_info", _p(o), ld, c0, n, B, _p(tgt), ldt, t0, int(target_logits), scale, _p(loss), _p(dout), _stream())


def u8_colorize(sprites, gain, out, B, C, HW):
    lib().call("eg_u8_colorize", _p(sprites), _p(gain), _p(out), B, C, HW, _stream())


def color_scale(inp, code, ldc, c0, factor, divide, out, B, C, HW):
    lib().call("eg_color_scale", _p(inp), _p(code), ldc, c0, factor, int(divide), _p(out), B, C, HW, _stream())


def loss_affine_rp_color(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred_out=None):
    lib().call("eg_loss_affine_rp_color", _p(o_real), _p(o_trans), ld, c0, B, _p(code), ldc, scale, _p(loss), _p(d_real), _p(d_trans), _p(pred_out), _stream())


def add_f32(out, a, b):
    lib().call("eg_add_f32", _p(out), _p(a), _p(b), out.numel(), _stream())


def u8_to_f32(x, y):
    lib().call("eg_u8_to_f32", _p(x), _p(y), y.numel(), _stream())


def loss_bce_sigmoid(o, ld, col, B, target, scale, loss, dout, zero_rows=True):
    lib().call("eg_loss_bce_sigmoid", _p(o), ld, col, B, target, scale, _p(loss), _p(dout), int(zero_rows), _stream())


def loss_mse(o, ld, col0, n, B, tgt, ldt, tconst, scale, loss, dout, zero_rows=True):
    lib().call("eg_loss_mse", _p(o), ld, col0, n, B, _p(tgt), ldt, tconst, scale, _p(loss), _p(dout), int(zero_rows), _stream())


def loss_ce_softmaxed(o, ld, c0, n, B, labels, scale, loss, dout):
    lib().call("eg_loss_ce_softmaxed", _p(o), ld, c0, n, B, _p(labels), scale, _p(loss), _p(dout), _stream())


def loss_affine_rpqxy(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred_out=None):
    lib().call("eg_loss_affine_rpqxy", _p(o_real), _p(o_trans), ld, c0, B, _p(code), ldc, scale, _p(loss), _p(d_real), _p(d_trans), _p(pred_out), _stream())


def loss_info_rpqxy(o_gen, o_trans, o_real, ld, c_cont, n_cont, n_cat, B, code, ldc, labels, lcat, lcon, laff, loss, d_gen, d_trans, d_real):
    """loss_mse + loss_ce_softmaxed + loss_affine_rpqxy of the CelebA info step as one launch (same numbers)"""
    lib().call("eg_loss_info_rpqxy", _p(o_gen), _p(o_trans), _p(o_real), ld, c_cont, n_cont, n_cat, B, _p(code), ldc, _p(labels), lcat, lcon, laff,
               _p(loss), _p(d_gen), _p(d_trans), _p(d_real), _stream())


# ---- device-side input pipeline -------------------------------------------------------------------
RNG_UNIFORM, RNG_NORMAL, RNG_RANDINT, RNG_BERNOULLI, RNG_EPOCH_PERM = 0, 1, 2, 3, 4


def _shard_span(numel, rank, world):
    from .engine import shard_span              # engine imports this module
    return shard_span(numel, rank, world)


def rng_fill(kind, out, a, b, seed, step, stream_id, rank=0, world=1):
    """out <- kind(a, b) from Philox4x32-10 keyed by ``seed``, counted by (element, device counter ``step``, ``stream_id``).
    ``rank`` / ``world``: ``out`` is this rank's shard of a draw of ``world * out.numel()`` elements -- the ranks' outputs, concatenated,
    are the one-rank draw of the global batch (engine.shard_span)"""
    elem0, total = _shard_span(out.numel(), rank, world)
    lib().call("eg_rng_fill", kind, _p(out), out.numel(), float(a), float(b), int(seed), _p(step), int(stream_id), elem0, total, _stream())


def rng_fill_multi(draws, seed, step, rank=0, world=1):
    """several draws in ONE launch, the values of one rng_fill each: draws = [(kind, out, a, b, stream_id[, onehot tensor])]"""
    arr = (EgRngSeg * len(draws))()
    for i, d in enumerate(draws):
        kind, out, a, b, sid = d[:5]
        oh = d[5] if len(d) > 5 else None
        elem0, total = _shard_span(out.numel(), rank, world)
        arr[i] = EgRngSeg(kind, _p(out), out.numel(), float(a), float(b), int(sid), _p(oh), oh.shape[1] if oh is not None else 0, elem0, total)
    lib().call("eg_rng_fill_multi", arr, len(draws), int(seed), _p(step), _stream())


def counter_add(counter, v=1):
    lib().call("eg_counter_add", _p(counter), int(v), _stream())


# ---- weight averaging -------------------------------------------------------------------
EMA_LERP, EMA_COPY = 0, 1


def ema_chunk_words() -> int:
    """32-bit words one workgroup of eg_ema_update moves at a time: the unit eg_ema_plan counts in"""
    return lib().query("eg_ema_chunk_words")


def ema_plan(segments):
    """segments = [(src, dst, kind)]: contiguous device tensors of equal byte size (a multiple of 4), kind EMA_LERP (fp32) or EMA_COPY.
    -> (device table, device chunk_first, nseg) for ``ema_update``: validated by eg_ema_plan on the host, then copied to the device
    once.  The table holds the tensors' addresses: the caller keeps them alive and in place."""
    n = len(segments)
    arr = (EgEmaSeg * max(n, 1))()
    for i, (src, dst, kind) in enumerate(segments):
        nbytes = src.numel() * src.element_size()
        if not (src.is_cuda and dst.is_cuda and src.device == dst.device and src.is_contiguous() and dst.is_contiguous()):
            raise ValueError(f"ema_plan: segment {i}: src and dst must be contiguous tensors on one HIP device")
        if nbytes != dst.numel() * dst.element_size() or nbytes % 4 or src.dtype != dst.dtype:
            raise ValueError(f"ema_plan: segment {i}: src and dst must have one dtype and one size, a multiple of 4 bytes")
        if int(kind) == EMA_LERP and src.dtype != torch.float32:
            raise ValueError(f"ema_plan: segment {i}: a lerp segment is fp32, got {src.dtype}")
        arr[i] = EgEmaSeg(_p(src), _p(dst), nbytes // 4, int(kind))
    first = (ctypes.c_uint * (n + 1))()
    lib().call("eg_ema_plan", arr, n, first)
    dev = segments[0][0].device
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    chunk_first = torch.frombuffer(bytearray(bytes(first)), dtype=torch.int32).to(dev)
    return table, chunk_first, n


def ema_update(table, chunk_first, nseg, beta, ramp, updates):
    """one launch over the whole table (eg_ema_update in the header); ``updates``: device int32[2] = (updates done, arrival counter)"""
    lib().call("eg_ema_update", _p(table), _p(chunk_first), int(nseg), float(beta), float(ramp), _p(updates), _stream())


def gather_u8_images(data, idx, flip, out, B, C, H, W, scale, shift, tick=None):
    """``tick``: device step counter incremented by this launch (the iteration's draws, earlier on the stream, have read it)"""
    if tick is None:
        lib().call("eg_gather_u8_images", _p(data), _p(idx), _p(flip), _p(out), B, C, H, W, float(scale), float(shift), _stream())
    else:
        lib().call("eg_gather_u8_images_tick", _p(data), _p(idx), _p(flip), _p(out), B, C, H, W, float(scale), float(shift), _p(tick), _stream())


def resample_u8(src, dst, planes, in_h, in_w, axis, bounds, kk, ksize, o0, on, c0, cn):
    lib().call("eg_resample_u8", _p(src), _p(dst), planes, in_h, in_w, axis, _p(bounds), _p(kk), ksize, o0, on, c0, cn, _stream())


def onehot(labels, out, B, n):
    lib().call("eg_onehot", _p(labels), _p(out), B, n, _stream())


# ---- stage-1 (Encoder_pxy) trainer ------------------------------------------------------------------
def theta_pxy(code, ldc, B, theta):
    lib().call("eg_theta_pxy", _p(code), ldc, B, _p(theta), _stream())


def loss_affine_pxy(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred_out=None, ncol=0):
    lib().call("eg_loss_affine_pxy", _p(o_real), _p(o_trans), ld, c0, B, _p(code), ldc, ncol, float(scale), _p(loss), _p(d_real), _p(d_trans),
               _p(pred_out), _stream())


def warp_affine_zeros(img, theta, out, B, C, H, W):
    lib().call("eg_warp_affine_zeros", _p(img), _p(theta), _p(out), B, C, H, W, _stream())


def warp_affine_bwd(img, theta, dout, dimg, dtheta, B, C, H, W, zeros=False):
    """backward of warp_affine (``zeros``: of warp_affine_zeros): writes every element of ``dimg`` [B,C,H,W] and ``dtheta`` [B,6]; either may
    be None.  H * W <= 16384."""
    lib().call("eg_warp_affine_bwd", _p(img), _p(theta), _p(dout), _p(dimg), _p(dtheta), B, C, H, W, int(bool(zeros)), _stream())


# kind argument of theta_bwd; theta_<name>(code, ldc, B, theta) is the forward
THETA_KINDS = {"rpqxy": 0, "rpqmnxy": 1, "rp": 2, "pxy": 3, "pxy_align_inv": 4}


def theta_bwd(kind, code, ldc, B, dtheta, dcode):
    """dcode [B, ldc] = J^T dtheta of theta_<kind> (``kind``: a value of THETA_KINDS); columns past the kind's codes are written 0"""
    lib().call("eg_theta_bwd", kind, _p(code), ldc, B, _p(dtheta), _p(dcode), _stream())


def affine_para_rpqmnxy(code, ldc, B, para):
    lib().call("eg_affine_para_rpqmnxy", _p(code), ldc, B, _p(para), _stream())


def make_grid(img, B, C, H, W, nrow, padding, pad_value, rng2, grid):
    lib().call("eg_make_grid", _p(img), B, C, H, W, nrow, padding, pad_value, _p(rng2), _p(grid), _stream())


def minmax_ws_floats():
    return lib().query("eg_minmax_ws_floats")


def minmax_f32(x, n, ws, out2):
    lib().call("eg_minmax_f32", _p(x), n, _p(ws), _p(out2), _stream())


def quantize_u8(x, C, H, W, rng2, out):
    lib().call("eg_quantize_u8", _p(x), C, H, W, _p(rng2), _p(out), _stream())


def col2im_img(dtype, cols, B, C, Hin, Win, k, stride, pad, bias, act, slope, out):
    lib().call("eg_col2im_img", dtype, _p(cols), B, C, Hin, Win, k, stride, pad, _p(bias), act, slope, _p(out), _stream())


# ---- disentanglement scores (score.hip) ------------------------------------------------------------------------------------------
def score_stage_u8(data, idx, gain, out, B, C, HW):
    lib().call("eg_score_stage_u8", _p(data), _p(idx), _p(gain), _p(out), B, C, HW, _stream())


def score_rows(cat, ldcat, ncat, cont, ldcont, pxy, ldpxy, B, out):
    lib().call("eg_score_rows", _p(cat), ldcat, ncat, _p(cont), ldcont, _p(pxy), ldpxy, B, _p(out), _stream())


def score_digitize(codes, n, ncode, nbins, bins, lohi=None):
    lib().call("eg_score_digitize", _p(codes), n, ncode, nbins, _p(bins), _p(lohi), _stream())


def score_mig_ws_ints(ncode, nf, kmax, nbins):
    return lib().query("eg_score_mig_ws_ints", ncode, nf, kmax, nbins)


def score_mig(bins, ncode, ys, nf, n, kmax, nbins, ws, mi):
    lib().call("eg_score_mig", _p(bins), ncode, _p(ys), nf, n, kmax, nbins, _p(ws), _p(mi), _stream())


def score_col_std(x, n, ncol, out):
    lib().call("eg_score_col_std", _p(x), n, ncol, _p(out), _stream())


def score_fvae_votes(x, L, M, ncol, eval_std, labels, nlab, predict, votes):
    lib().call("eg_score_fvae_votes", _p(x), L, M, ncol, _p(eval_std), _p(labels), nlab, _p(predict), _p(votes), _stream())


def score_pair_absdiff_mean(x, L, M, ncol, feat):
    lib().call("eg_score_pair_absdiff_mean", _p(x), L, M, ncol, _p(feat), _stream())


def score_logreg_accuracy(X, y, n, d, K, W, predict, correct):
    lib().call("eg_score_logreg_accuracy", _p(X), _p(y), n, d, K, _p(W), _p(predict), _p(correct), _stream())


# info[..., 3] of eg_score_svc1_fit
SVC_STATUS = {0: "converged", 1: "max_iter reached", 2: "line search failed", 4: "a label outside 0..K-1 or a class without a sample",
              5: "non-finite objective or gradient"}


def score_sq_corr(codes, n, k, fv, nf, R):
    lib().call("eg_score_sq_corr", _p(codes), n, k, _p(fv), nf, _p(R), _stream())


def score_svc1_fit(X, y, n, P, K, C, max_iter, gtol, W, info):
    lib().call("eg_score_svc1_fit", _p(X), _p(y), n, P, K, C, max_iter, gtol, _p(W), _p(info), _stream())


def score_svc1_accuracy(X, y, n, P, K, W, predict, correct):
    lib().call("eg_score_svc1_accuracy", _p(X), _p(y), n, P, K, _p(W), _p(predict), _p(correct), _stream())


# info[3] of eg_score_softmax_fit
SOFTMAX_STATUS = {0: "converged", 1: "max_iter reached", 2: "line search failed", 3: "Hessian not positive definite",
                  4: "a label outside 0..K-1", 5: "non-finite gradient", 6: "a class without a sample"}


def score_softmax_ws_bytes(n, d, K):
    return lib().query("eg_score_softmax_ws_bytes", n, d, K)


def score_softmax_fit(X, y, n, d, K, inv_C, max_iter, gtol, ws, W, info):
    """blocks: the host reads the solver's decision record after every trial (the one entry point that synchronises)"""
    lib().call("eg_score_softmax_fit", _p(X), _p(y), n, d, K, inv_C, max_iter, gtol, _p(ws), _p(W), _p(info), _stream())


def score_softmax_proba(X, n, d, K, W, proba):
    lib().call("eg_score_softmax_proba", _p(X), n, d, K, _p(W), _p(proba), _stream())


def score_auc_ovr(scores, order, offsets, n, K, max_class_rows, less, equal):
    lib().call("eg_score_auc_ovr", _p(scores), _p(order), _p(offsets), n, K, int(max_class_rows), _p(less), _p(equal), _stream())


# status[0] bits of eg_score_norm_gram
NORM_GRAM_ZERO_VAR, NORM_GRAM_NONFINITE = 1, 2


def score_norm_gram_ws_bytes(n, k, nf):
    return lib().query("eg_score_norm_gram_ws_bytes", n, k, nf)


def score_norm_gram(codes, fv, n, k, nf, ws, mean, std, G, status):
    lib().call("eg_score_norm_gram", _p(codes), _p(fv), n, k, nf, _p(ws), _p(mean), _p(std), _p(G), _p(status), _stream())


# info[..., 3] of eg_score_lasso_gram_fit
LASSO_STATUS = {0: "converged", 1: "max_sweeps reached", 2: "non-finite", 3: "non-positive diagonal"}


def score_lasso_gram_fit(G, k, nf, alpha, max_sweeps, tol, W, info):
    lib().call("eg_score_lasso_gram_fit", _p(G), k, nf, float(alpha), int(max_sweeps), float(tol), _p(W), _p(info), _stream())


# ---- device loss log of a training run (engine.LossLog) ----------------------------------------------
def runlog_append(losses, n, ring, capacity, head, first_nonfinite):
    """row head % capacity of ring[capacity][n] <- losses[:n]; head += 1; the first non-finite iteration (1-based) latched"""
    lib().call("eg_runlog_append", _p(losses), int(n), _p(ring), int(capacity), _p(head), _p(first_nonfinite), _stream())


# ---- sliced Wasserstein distance ---------------------------------------------------------
SWD_FLAG_ZERO_STD, SWD_FLAG_NONFINITE, SWD_FLAG_POSITION = 1, 2, 4


def pyr_down(fine, coarse, planes, H):
    """coarse [planes, H/2, H/2] <- the 5 x 5 binomial filter of fine [planes, H, H] at the even positions (mirror border)"""
    lib().call("eg_pyr_down", _p(fine), _p(coarse), planes, H, _stream())


def pyr_up_sub(fine, coarse, planes, H):
    """fine [planes, H, H] -= up(coarse [planes, H/2, H/2]), in place"""
    lib().call("eg_pyr_up_sub", _p(fine), _p(coarse), planes, H, _stream())


def swd_patch_stats_ws_doubles(C) -> int:
    return lib().query("eg_swd_patch_stats_ws_doubles", C)


def swd_patch_stats(img, pos, n_desc, P, C, H, ws, stats, flag):
    """stats [C, 2] float64 <- (mean, population std) of the gathered patch pixels per channel; flag (int32, zeroed by the caller) |= SWD_FLAG_*"""
    lib().call("eg_swd_patch_stats", _p(img), _p(pos), n_desc, P, C, H, _p(ws), _p(stats), _p(flag), _stream())


def swd_unit_columns(dirs, K, D):
    lib().call("eg_swd_unit_columns", _p(dirs), K, D, _stream())


def swd_project_ws_floats(C) -> int:
    return lib().query("eg_swd_project_ws_floats", C)


def swd_project(img, pos, n_desc, P, C, H, dirs, D, stats, ws, out, ld):
    """out [D, ld] <- projections of the normalised 7 x 7 x C descriptors on the columns of dirs [49 C, D], one direction per row"""
    lib().call("eg_swd_project", _p(img), _p(pos), n_desc, P, C, H, _p(dirs), D, _p(stats), _p(ws), _p(out), ld, _stream())


def sort_tile_elems() -> int:
    """elements of a column that eg_sort_columns_f32 sorts inside LDS: columns longer than this take global merge passes"""
    return lib().query("eg_sort_tile_elems")


def sort_columns(x, n=None):
    """x [cols, ld] fp32 (rows contiguous): the first ``n`` (default: all) elements of every row sorted ascending, in place"""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError("sort_columns: x must be a 2-D fp32 device tensor with contiguous rows")
    cols, ld = x.shape[0], x.stride(0) if x.shape[0] > 1 else x.shape[1]
    n = x.shape[1] if n is None else int(n)
    if not 1 <= n <= x.shape[1]:
        raise ValueError(f"sort_columns: n must be in 1..{x.shape[1]}")
    lib().call("eg_sort_columns_f32", _p(x), n, cols, ld, _stream())
    return x


def l1_mean_ws_doubles() -> int:
    return lib().query("eg_l1_mean_ws_doubles")


def l1_mean(a, b, n, cols, ld, ws, out):
    """out[0] (float64) <- mean |a - b| over the first n elements of the cols rows (row stride ld) of two fp32 arrays"""
    lib().call("eg_l1_mean_f32", _p(a), _p(b), n, cols, ld, _p(ws), _p(out), _stream())


# ---- exact nearest neighbours over uint8 rows ---------------------------------------------
def knn_tile_queries() -> int:
    """queries per workgroup tile of eg_knn_u8 (from four such tiles of queries on a workgroup owns two)"""
    return lib().query("eg_knn_tile_queries")


def knn_tile_rows() -> int:
    """database rows per tile of eg_knn_u8"""
    return lib().query("eg_knn_tile_rows")


def knn_splits(nq, n) -> int:
    """database slices eg_knn_u8 launches for (nq, n)"""
    return lib().query("eg_knn_splits", int(nq), int(n))


def knn_u8(queries, database, k, self0=-1, out=None):
    """-> (dist, idx), int32 [nq, k] on the device: per row of ``queries`` the ``k`` nearest rows of ``database`` by exact squared L2
    distance, ascending in (distance, index) -- equal distances go to the lower index.  Both are contiguous uint8 device tensors whose
    trailing dimensions flatten to the same K (a multiple of 64 in 64 .. 32768).  ``self0 >= 0``: query i is database row self0 + i and
    does not find itself.  ``out``: an int32 (dist, idx) pair of [nq, k] views with contiguous rows to write instead of new tensors."""
    for name, t in (("queries", queries), ("database", database)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() >= 2 and t.is_contiguous()):
            raise ValueError(f"knn_u8: {name} must be a contiguous uint8 device tensor [rows, ...]")
    nq, n = int(queries.shape[0]), int(database.shape[0])
    K = queries[0].numel() if nq else 0
    if nq < 1 or n < 1 or database[0].numel() != K or queries.device != database.device:
        raise ValueError(f"knn_u8: queries {tuple(queries.shape)} and database {tuple(database.shape)} must have rows of one length on one device")
    k, self0 = int(k), int(self0)
    if K % 64 or not 64 <= K <= 32768:
        raise ValueError(f"knn_u8: the row length must be a multiple of 64 in 64 .. 32768, got {K}")
    if not 1 <= k <= 16 or k > n - (1 if 0 <= self0 < n else 0):
        raise ValueError(f"knn_u8: k = {k} must be in 1 .. 16 and no more than the candidates of a query ({n} rows, self0 = {self0})")
    if out is None:
        dist = torch.empty(nq, k, device=queries.device, dtype=torch.int32)
        idx = torch.empty(nq, k, device=queries.device, dtype=torch.int32)
    else:
        dist, idx = out
        for t in (dist, idx):
            if not (t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (nq, k) and t.is_contiguous()):
                raise ValueError(f"knn_u8: out must be two contiguous int32 device tensors [{nq}, {k}]")
    ws = torch.empty(lib().query("eg_knn_ws_bytes", nq, n, k) // 8, device=queries.device, dtype=torch.int64)
    lib().call("eg_knn_u8", _p(queries), nq, _p(database), n, K, k, self0, _p(ws), _p(dist), _p(idx), _stream())
    return dist, idx


# ---- how many balls contain a row ---------------------------------------------------------
def ball_count_ws_bytes(nq, n) -> int:
    """bytes of the per-slice counts eg_ball_count_u8 needs for (nq, n): knn_splits(nq, n) * nq * 4"""
    return lib().query("eg_ball_count_ws_bytes", int(nq), int(n))


def ball_count_u8(queries, database, radii, self0=-1, out=None):
    """-> count, int32 [nq] on the device: per row of ``queries`` the number of rows j of ``database`` whose CLOSED ball contains it,
    d(query, database[j]) <= radii[j], by the exact squared L2 distance of ``knn_u8``.  ``radii``: a contiguous int32 device tensor [n];
    a negative radius is an empty ball.  ``self0 >= 0``: query i is database row self0 + i and is not counted in its own ball.
    ``out``: a contiguous int32 device tensor [nq] to write instead of a new one."""
    for name, t in (("queries", queries), ("database", database)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() >= 2 and t.is_contiguous()):
            raise ValueError(f"ball_count_u8: {name} must be a contiguous uint8 device tensor [rows, ...]")
    nq, n = int(queries.shape[0]), int(database.shape[0])
    K = queries[0].numel() if nq else 0
    if nq < 1 or n < 1 or database[0].numel() != K or queries.device != database.device:
        raise ValueError(f"ball_count_u8: queries {tuple(queries.shape)} and database {tuple(database.shape)} must have rows of one length on one device")
    if K % 64 or not 64 <= K <= 32768:
        raise ValueError(f"ball_count_u8: the row length must be a multiple of 64 in 64 .. 32768, got {K}")
    if not (isinstance(radii, torch.Tensor) and radii.is_cuda and radii.dtype == torch.int32 and tuple(radii.shape) == (n,) and radii.is_contiguous()
            and radii.device == database.device):
        raise ValueError(f"ball_count_u8: radii must be a contiguous int32 device tensor [{n}], one radius per database row")
    if out is None:
        out = torch.empty(nq, device=queries.device, dtype=torch.int32)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (nq,) and out.is_contiguous()):
        raise ValueError(f"ball_count_u8: out must be a contiguous int32 device tensor [{nq}]")
    ws = torch.empty(lib().query("eg_ball_count_ws_bytes", nq, n) // 4, device=queries.device, dtype=torch.int32)
    lib().call("eg_ball_count_u8", _p(queries), nq, _p(database), n, K, _p(radii), int(self0), _p(ws), _p(out), _stream())
    return out


# ---- kernel sums and the distance select --------------------------------------------------
def kernel_sum_ws_bytes(nq, n, nb) -> int:
    """bytes of the per-slice sums eg_kernel_sum_u8 needs for (nq, n, nb): knn_splits(nq, n) * nq * nb * 8"""
    return lib().query("eg_kernel_sum_ws_bytes", int(nq), int(n), int(nb))


def dist_select_ws_bytes(nq, n) -> int:
    """bytes of the state and the per-workgroup histograms eg_dist_select_u8 needs for (nq, n)"""
    return lib().query("eg_dist_select_ws_bytes", int(nq), int(n))


def _u8_pair(what, queries, database):
    """the checks of ``knn_u8`` on its two operands, shape and dtype first and the device last -> (nq, n, K)"""
    for name, t in (("queries", queries), ("database", database)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() >= 2 and t.is_contiguous()):
            raise ValueError(f"{what}: {name} must be a contiguous uint8 device tensor [rows, ...]")
    nq, n = int(queries.shape[0]), int(database.shape[0])
    K = queries[0].numel() if nq else 0
    if nq < 1 or n < 1 or database[0].numel() != K or queries.device != database.device:
        raise ValueError(f"{what}: queries {tuple(queries.shape)} and database {tuple(database.shape)} must have rows of one length on one device")
    if K % 64 or not 64 <= K <= 32768:
        raise ValueError(f"{what}: the row length must be a multiple of 64 in 64 .. 32768, got {K}")
    return nq, n, K


def _on_device(what, queries):
    if not queries.is_cuda:
        raise ValueError(f"{what}: queries and database must be contiguous uint8 device tensors (there is no CPU path)")


def kernel_sum_u8(queries, database, inv_gamma, self0=-1, out=None, flag=None):
    """-> float64 [nq, nb] on the device: out[i, b] = the sum over the rows j of ``database`` of exp(-d(queries[i], database[j]) *
    inv_gamma[b]), d the exact squared L2 distance of ``knn_u8`` (operands, row lengths and ``self0`` as there: with ``self0 >= 0`` query i
    is database row self0 + i and its own term is left out).  ``inv_gamma``: a contiguous float64 DEVICE tensor [nb], 1 <= nb <= 4, so a
    bandwidth can come from ``dist_select_u8`` without a host read.  ``out``: a contiguous float64 device tensor [nq, nb] to write instead
    of a new one.  ``flag``: an int32 device tensor [1] that is WRITTEN (not or-ed): bit b says inv_gamma[b] is no finite positive number;
    without it the word is not reported.  Sums in a fixed order: two calls give the same bits."""
    nq, n, K = _u8_pair("kernel_sum_u8", queries, database)
    if not (isinstance(inv_gamma, torch.Tensor) and inv_gamma.dtype == torch.float64 and inv_gamma.dim() == 1 and 1 <= inv_gamma.shape[0] <= 4
            and inv_gamma.is_contiguous() and inv_gamma.device == queries.device):
        raise ValueError("kernel_sum_u8: inv_gamma must be a contiguous float64 device tensor [nb] with 1 <= nb <= 4, beside the queries")
    nb = int(inv_gamma.shape[0])
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and tuple(out.shape) == (nq, nb) and out.is_contiguous()
                                and out.device == queries.device):
        raise ValueError(f"kernel_sum_u8: out must be a contiguous float64 device tensor [{nq}, {nb}]")
    if flag is not None and not (isinstance(flag, torch.Tensor) and flag.dtype == torch.int32 and flag.numel() == 1 and flag.is_contiguous()
                                 and flag.device == queries.device):
        raise ValueError("kernel_sum_u8: flag must be an int32 device tensor of one element")
    _on_device("kernel_sum_u8", queries)
    if out is None:
        out = torch.empty(nq, nb, device=queries.device, dtype=torch.float64)
    if flag is None:
        flag = torch.empty(1, device=queries.device, dtype=torch.int32)
    ws = torch.empty(lib().query("eg_kernel_sum_ws_bytes", nq, n, nb) // 8, device=queries.device, dtype=torch.float64)
    lib().call("eg_kernel_sum_u8", _p(queries), nq, _p(database), n, K, _p(inv_gamma), nb, int(self0), _p(ws), _p(out), _p(flag), _stream())
    return out


def _f64(what, name, t, shape, like):
    """``t`` must be a contiguous float64 tensor of ``shape`` on the device of ``like``"""
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == like.device):
        raise ValueError(f"{what}: {name} must be a contiguous float64 device tensor {list(shape)}, beside the queries")


# ---- the soft minimum ---------------------------------------------------------------------
def softmin_ws_bytes(nq, n) -> int:
    """bytes of the per-slice (maximum, sum) pairs eg_softmin_u8 needs for (nq, n): knn_splits(nq, n) * nq * 16"""
    return lib().query("eg_softmin_ws_bytes", int(nq), int(n))


def softmin_u8(queries, database, g, inv_eps, self0=-1, prev=None, out=None, flag=None):
    """-> float64 [nq] on the device: the soft minimum over the rows j of ``database`` of d(queries[i], database[j]) - g[j] at the
    temperature 1 / inv_eps, soft[i] = -(log sum_j exp((g[j] - d) * inv_eps) - log #j) / inv_eps, d the exact squared L2 distance of
    ``knn_u8`` (operands, row lengths and ``self0`` as there: with ``self0 >= 0`` query i is database row self0 + i and that row is left
    out; at least one row must remain) -- one half-iteration of a Sinkhorn loop, as a streaming log-sum-exp that neither overflows nor
    underflows.  ``g``: float64 [n]; ``inv_eps``: a float64 DEVICE tensor of one element, so a whole epsilon schedule is enqueued without
    a host read.  ``prev``: float64 [nq]; the result is then 0.5 * prev + 0.5 * soft.  ``out``: float64 [nq] to write instead of a new
    tensor; ``prev``, ``g`` and ``out`` may be one tensor.  ``flag``: an int32 device tensor [1] that is WRITTEN: bit 0 says inv_eps is no
    finite positive number.  A fixed merge order: two calls give the same bits."""
    nq, n, K = _u8_pair("softmin_u8", queries, database)
    _f64("softmin_u8", "g", g, (n,), queries)
    if not (isinstance(inv_eps, torch.Tensor) and inv_eps.dtype == torch.float64 and inv_eps.numel() == 1 and inv_eps.is_contiguous()
            and inv_eps.device == queries.device):
        raise ValueError("softmin_u8: inv_eps must be a float64 device tensor of one element, beside the queries")
    if prev is not None:
        _f64("softmin_u8", "prev", prev, (nq,), queries)
    if out is not None:
        _f64("softmin_u8", "out", out, (nq,), queries)
    if flag is not None and not (isinstance(flag, torch.Tensor) and flag.dtype == torch.int32 and flag.numel() == 1 and flag.is_contiguous()
                                 and flag.device == queries.device):
        raise ValueError("softmin_u8: flag must be an int32 device tensor of one element")
    self0 = int(self0)
    if n - (1 if 0 <= self0 < n else 0) < 1:
        raise ValueError(f"softmin_u8: a query has no candidate ({n} rows, self0 = {self0}): n - 1 >= 1 is needed where a row is excluded")
    _on_device("softmin_u8", queries)
    if out is None:
        out = torch.empty(nq, device=queries.device, dtype=torch.float64)
    if flag is None:
        flag = torch.empty(1, device=queries.device, dtype=torch.int32)
    ws = torch.empty(lib().query("eg_softmin_ws_bytes", nq, n) // 8, device=queries.device, dtype=torch.float64)
    lib().call("eg_softmin_u8", _p(queries), nq, _p(database), n, K, _p(g), _p(inv_eps), self0, _p(prev), _p(ws), _p(out), _p(flag), _stream())
    return out


def dist_select_u8(queries, database, rank, self0=-1):
    """-> int32 [2] on the device: [0] = the element of 0-based ``rank`` of all distances d(queries[i], database[j]), j != self0 + i, in
    ascending order (operands, d and ``self0`` as for ``knn_u8``); [1] = 1 if ``rank`` is not below the number of pairs ([0] is then the
    largest distance), else 0.  A radix select over histogram passes of the search's tile loop: no distance is stored, nothing is read
    back between the passes."""
    nq, n, K = _u8_pair("dist_select_u8", queries, database)
    rank = int(rank)
    if not 0 <= rank < 2 ** 64:
        raise ValueError(f"dist_select_u8: rank = {rank} must be in 0 .. 2^64 - 1")
    _on_device("dist_select_u8", queries)
    out = torch.empty(2, device=queries.device, dtype=torch.int32)
    ws = torch.empty(lib().query("eg_dist_select_ws_bytes", nq, n) // 8, device=queries.device, dtype=torch.int64)
    lib().call("eg_dist_select_u8", _p(queries), nq, _p(database), n, K, int(self0), rank, _p(ws), _p(out), _stream())
    return out


# ---- k-means over uint8 rows --------------------------------------------------------------
GROUP_FLAG_LABEL = 1                                  # eg_group_rows: a label outside [0, bins)
SEED_FLAG_DUPLICATES, SEED_FLAG_U = 1, 2              # eg_kmeans_seed_u8: fewer than bins distinct rows; a u outside [0, 1)
KMEANS_MAX_BINS = 1024


def group_rows_block() -> int:
    """labels per workgroup of eg_group_rows' count and scatter kernels"""
    return lib().query("eg_group_rows_block")


def kmeans_segment_rows() -> int:
    """member rows per segment of eg_kmeans_update_u8"""
    return lib().query("eg_kmeans_segment_rows")


def kmeans_column_chunk() -> int:
    """bytes of a row one workgroup of eg_kmeans_update_u8 sums"""
    return lib().query("eg_kmeans_column_chunk")


def kmeans_seed_rows() -> int:
    """rows per workgroup of eg_kmeans_seed_u8's streaming kernel"""
    return lib().query("eg_kmeans_seed_rows")


def group_rows_ws_bytes(n, bins) -> int:
    return lib().query("eg_group_rows_ws_bytes", int(n), int(bins))


def kmeans_update_ws_bytes(n, K, bins) -> int:
    return lib().query("eg_kmeans_update_ws_bytes", int(n), int(K), int(bins))


def kmeans_seed_ws_bytes(n) -> int:
    return lib().query("eg_kmeans_seed_ws_bytes", int(n))


def _ws_bytes(ws, need, what, like):
    """a workspace of at least ``need`` bytes: ``ws`` (a contiguous device tensor, 16-byte aligned) or a new one"""
    if ws is None:
        return torch.empty((need + 15) // 16 * 2, device=like.device, dtype=torch.int64)
    if not (isinstance(ws, torch.Tensor) and ws.is_contiguous() and ws.device == like.device and ws.numel() * ws.element_size() >= need
            and ws.data_ptr() % 16 == 0):
        raise ValueError(f"{what}: ws must be a contiguous 16-byte aligned device tensor of at least {need} bytes")
    return ws


def _check_bins(what, bins):
    bins = int(bins)
    if not 1 <= bins <= KMEANS_MAX_BINS:
        raise ValueError(f"{what}: bins = {bins} must be in 1 .. {KMEANS_MAX_BINS}")
    return bins


def _u8_table(what, rows):
    """the checks of ``knn_u8`` on one operand -> (n, K)"""
    if not (isinstance(rows, torch.Tensor) and rows.dtype == torch.uint8 and rows.dim() >= 2 and rows.is_contiguous()):
        raise ValueError(f"{what}: rows must be a contiguous uint8 device tensor [n, ...]")
    n = int(rows.shape[0])
    K = rows[0].numel() if n else 0
    if n < 1:
        raise ValueError(f"{what}: rows {tuple(rows.shape)} holds no row")
    if K % 64 or not 64 <= K <= 32768:
        raise ValueError(f"{what}: the row length must be a multiple of 64 in 64 .. 32768, got {K}")
    if not rows.is_cuda:
        raise ValueError(f"{what}: rows must be a contiguous uint8 device tensor (there is no CPU path)")
    return n, K


def _i32(what, name, t, shape, like):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == like.device):
        raise ValueError(f"{what}: {name} must be a contiguous int32 device tensor {list(shape)}, beside the rows")


def group_rows(labels, bins, ws=None, flag=None):
    """-> (counts [bins], offsets [bins + 1], order [n]), int32 on the device: a stable counting sort of the int32 device labels [n] into
    ``bins`` cells (1 .. 1024).  The rows of cell c are ``order[offsets[c]:offsets[c + 1]]``, ascending.  A label outside [0, bins) joins
    no cell: ``offsets[bins]`` counts the rows that joined one, the tail of ``order`` holds -1 and bit ``GROUP_FLAG_LABEL`` of ``flag``
    (an int32 device tensor [1], WRITTEN; not reported without it) is raised.  Three launches, no host read."""
    if not (isinstance(labels, torch.Tensor) and labels.dtype == torch.int32 and labels.dim() == 1 and labels.is_contiguous() and labels.shape[0] >= 1):
        raise ValueError("group_rows: labels must be a contiguous int32 device tensor [n], n >= 1")
    if not labels.is_cuda:
        raise ValueError("group_rows: labels must be on the device (there is no CPU path)")
    bins, n = _check_bins("group_rows", bins), int(labels.shape[0])
    if flag is None:
        flag = torch.empty(1, device=labels.device, dtype=torch.int32)
    else:
        _i32("group_rows", "flag", flag, (1,), labels)
    ws = _ws_bytes(ws, group_rows_ws_bytes(n, bins), "group_rows", labels)
    counts = torch.empty(bins, device=labels.device, dtype=torch.int32)
    offsets = torch.empty(bins + 1, device=labels.device, dtype=torch.int32)
    order = torch.empty(n, device=labels.device, dtype=torch.int32)
    lib().call("eg_group_rows", _p(labels), n, bins, _p(ws), _p(counts), _p(offsets), _p(order), _p(flag), _stream())
    return counts, offsets, order


def _check_centres(what, centres, bins, K, like):
    if not (isinstance(centres, torch.Tensor) and centres.dtype == torch.uint8 and centres.dim() >= 2 and centres.is_contiguous()
            and centres.shape[0] == bins and centres[0].numel() == K and centres.device == like.device):
        raise ValueError(f"{what}: centres must be a contiguous uint8 device tensor [{bins}, ...] with rows of {K} bytes, beside the rows")


def kmeans_update_u8(rows, order, offsets, counts, centres, ws=None):
    """centres [bins, ...] (uint8, IN PLACE) <- the rounded means of the cells ``group_rows`` made of ``rows`` [n, ...]: for a cell with
    count > 0, centre[t] = (2 sum[t] + count) // (2 count) -- round half up from exact int32 column sums, so n * 255 < 2^31 --; a cell
    with count == 0 keeps its bytes.  Returns ``centres``.  Three launches, no host read."""
    n, K = _u8_table("kmeans_update_u8", rows)
    if n * 255 >= 2 ** 31:
        raise ValueError(f"kmeans_update_u8: n = {n} rows: n * 255 must stay below 2^31 (the column sums are int32)")
    if not (isinstance(counts, torch.Tensor) and counts.dim() == 1):
        raise ValueError("kmeans_update_u8: counts must be a contiguous int32 device tensor [bins]")
    bins = _check_bins("kmeans_update_u8", counts.shape[0])
    _i32("kmeans_update_u8", "counts", counts, (bins,), rows)
    _i32("kmeans_update_u8", "offsets", offsets, (bins + 1,), rows)
    _i32("kmeans_update_u8", "order", order, (n,), rows)
    _check_centres("kmeans_update_u8", centres, bins, K, rows)
    ws = _ws_bytes(ws, kmeans_update_ws_bytes(n, K, bins), "kmeans_update_u8", rows)
    lib().call("eg_kmeans_update_u8", _p(rows), n, K, _p(order), _p(offsets), _p(counts), bins, _p(ws), _p(centres), _stream())
    return centres


def kmeans_seed_u8(rows, bins, u, flag=None):
    """-> (idx int32 [bins], centres uint8 [bins, ...]) on the device: k-means++ seeding of ``rows`` [n, ...] driven by ``u``, a
    contiguous fp32 device tensor of ``bins`` uniforms in [0, 1).  Centre 0 is row min(floor(u[0] n), n - 1); for j >= 1, with mind[i]
    the exact squared distance from row i to its nearest chosen centre and total its int64 sum, the pick is the lowest row whose
    inclusive prefix sum of mind exceeds min(floor((double)u[j] * (double)total), total - 1): a copy of a chosen centre is never picked.
    ``flag`` (int32 device tensor [1], WRITTEN; not reported without it): ``SEED_FLAG_DUPLICATES`` = fewer than ``bins`` distinct rows,
    ``SEED_FLAG_U`` = a u outside [0, 1).  n * 2^31 <= 2^53.  All 2 bins - 1 launches are enqueued at once, no host read."""
    n, K = _u8_table("kmeans_seed_u8", rows)
    bins = _check_bins("kmeans_seed_u8", bins)
    if n > 2 ** 22:
        raise ValueError(f"kmeans_seed_u8: n = {n} rows: n * 2^31 must not exceed 2^53 (the sum of the distances is exact in a double)")
    if not (isinstance(u, torch.Tensor) and u.dtype == torch.float32 and tuple(u.shape) == (bins,) and u.is_contiguous() and u.device == rows.device):
        raise ValueError(f"kmeans_seed_u8: u must be a contiguous fp32 device tensor [{bins}], beside the rows")
    if flag is None:
        flag = torch.empty(1, device=rows.device, dtype=torch.int32)
    else:
        _i32("kmeans_seed_u8", "flag", flag, (1,), rows)
    ws = _ws_bytes(None, kmeans_seed_ws_bytes(n), "kmeans_seed_u8", rows)
    idx = torch.empty(bins, device=rows.device, dtype=torch.int32)
    centres = torch.empty((bins,) + tuple(rows.shape[1:]), device=rows.device, dtype=torch.uint8)
    lib().call("eg_kmeans_seed_u8", _p(rows), n, K, bins, _p(u), _p(ws), _p(idx), _p(centres), _p(flag), _stream())
    return idx, centres


def kmeans_u8(rows, bins, iterations=20, u=None, init=None, flag=None):
    """Lloyd's k-means over uint8 rows with byte centres -> (centres uint8 [bins, ...], labels int32 [n], counts int32 [bins], log), all
    on the device; log = {"inertia": int64 [iterations + 1], "changed": int32 [iterations]}.

    The centres start from ``kmeans_seed_u8(rows, bins, u)`` or from ``init``: int row indices [bins] or uint8 centres [bins, ...].  For
    t < iterations: labels_t = the nearest centre (``knn_u8(rows, centres_t, 1)``: exact distances, ties to the lower centre),
    inertia[t] = the sum of the rows' distances to their centres, changed[t] = the rows whose label differs from labels_{t-1} (n at
    t = 0), centres_{t+1} = ``kmeans_update_u8``.  A last assignment gives the returned labels, counts and inertia[iterations].  The
    iteration count is fixed: after changed == 0 the remaining iterations are fixed points.  Centres are bytes, so the inertia need not
    fall monotonically.  ``flag`` (int32 device tensor [1], WRITTEN): the seeding's flag word, 0 with ``init``.  Every launch is
    enqueued up front; there is no host read."""
    n, K = _u8_table("kmeans_u8", rows)
    bins, iterations = _check_bins("kmeans_u8", bins), int(iterations)
    if iterations < 0:
        raise ValueError(f"kmeans_u8: iterations = {iterations} must be >= 0")
    if n * 255 >= 2 ** 31:
        raise ValueError(f"kmeans_u8: n = {n} rows: n * 255 must stay below 2^31 (the column sums are int32)")
    if (u is None) == (init is None):
        raise ValueError("kmeans_u8: pass either u (the seeding's uniforms) or init (row indices or centres)")
    dev = rows.device
    if flag is None:
        flag = torch.empty(1, device=dev, dtype=torch.int32)
    else:
        _i32("kmeans_u8", "flag", flag, (1,), rows)
    if init is None:
        _, centres = kmeans_seed_u8(rows, bins, u, flag=flag)
    else:
        if not (isinstance(init, torch.Tensor) and init.device == dev):
            raise ValueError("kmeans_u8: init must be a device tensor beside the rows: int row indices [bins] or uint8 centres [bins, ...]")
        if init.dtype in (torch.int32, torch.int64) and tuple(init.shape) == (bins,):
            centres = rows[init.long()].contiguous()                # an index outside the rows is torch's device-side assertion
        else:
            _check_centres("kmeans_u8", init, bins, K, rows)
            centres = init.clone()
        flag.zero_()
    inertia = torch.empty(iterations + 1, device=dev, dtype=torch.int64)
    changed = torch.empty(iterations, device=dev, dtype=torch.int32)
    group_ws = _ws_bytes(None, group_rows_ws_bytes(n, bins), "kmeans_u8", rows)
    update_ws = _ws_bytes(None, kmeans_update_ws_bytes(n, K, bins), "kmeans_u8", rows)
    pair = [(torch.empty(n, 1, device=dev, dtype=torch.int32), torch.empty(n, 1, device=dev, dtype=torch.int32)) for _ in range(2)]
    gflag = torch.empty(1, device=dev, dtype=torch.int32)
    prev = None
    for t in range(iterations + 1):
        dist, idx = knn_u8(rows, centres, 1, out=pair[t & 1])
        labels = idx.reshape(n)
        inertia[t] = dist.sum(dtype=torch.int64)
        if t == iterations:
            break
        changed[t] = n if prev is None else (labels != prev).sum()
        counts, offsets, order = group_rows(labels, bins, ws=group_ws, flag=gflag)
        kmeans_update_u8(rows, order, offsets, counts, centres, ws=update_ws)
        prev = labels
    counts = group_rows(labels, bins, ws=group_ws, flag=gflag)[0]
    return centres, labels, counts, {"inertia": inertia, "changed": changed}


# ---- radial power spectrum of uint8 images -------------------------------------------------
SPECTRUM_SIDES = {16: 12, 32: 24, 64: 46}             # image side -> rings
SPECTRUM_MAX_C = 4
_SPECTRUM_TABLES = {}


def spectrum_host_tables(H):
    """the integer ring tables and the twiddle table of ``eg_spectrum_u8`` for side ``H`` (16, 32 or 64) as numpy arrays ->
    {"rings": B, "cell_ring": int32 [H, H/2 + 1], "ring_start": int32 [B + 1], "ring_cells": int32 [H (H/2 + 1)], "ring_count":
    int32 [B], "weight": int32 [H/2 + 1], "cos_sin": float64 [2, H]}.  The ring of cell (ky, kx): fy = min(ky, H - ky), q = fy^2 + kx^2,
    s = isqrt(q), b = s if q <= s^2 + s else s + 1 -- integers only.  ``ring_cells`` lists the cells ky (H/2 + 1) + kx of ring 0, then
    of ring 1 ..., each ascending; ``ring_count[b]`` = the sum of the column weights (1 for kx in {0, H/2}, else 2) over the ring."""
    import math
    import numpy as np
    H = int(H)
    if H not in SPECTRUM_SIDES:
        raise ValueError(f"spectrum: the image side must be one of {sorted(SPECTRUM_SIDES)}, got {H}")
    KX = H // 2 + 1
    weight = np.array([1 if kx in (0, H // 2) else 2 for kx in range(KX)], np.int32)
    cell_ring = np.empty((H, KX), np.int32)
    for ky in range(H):
        fy = min(ky, H - ky)
        for kx in range(KX):
            q = fy * fy + kx * kx
            s = math.isqrt(q)
            cell_ring[ky, kx] = s if q <= s * s + s else s + 1
    B = int(cell_ring.max()) + 1
    assert B == SPECTRUM_SIDES[H]
    flat = cell_ring.reshape(-1)
    ring_cells = np.argsort(flat, kind="stable").astype(np.int32)            # stable: ascending (ky, kx) inside a ring
    sizes = np.bincount(flat, minlength=B)
    ring_start = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    ring_count = np.bincount(flat, weights=np.tile(weight, H), minlength=B).astype(np.int32)
    k = np.arange(H, dtype=np.float64)
    cos_sin = np.stack((np.cos(2.0 * np.pi * k / H), np.sin(2.0 * np.pi * k / H)))
    return {"rings": B, "cell_ring": cell_ring, "ring_start": ring_start, "ring_cells": ring_cells, "ring_count": ring_count,
            "weight": weight, "cos_sin": cos_sin}


def spectrum_tables(H, device):
    """``spectrum_host_tables(H)`` on ``device``, built once per (H, device): {"rings", "cell_ring", "ring_start", "ring_cells",
    "ring_count", "cos_sin"} (the tables as contiguous device tensors)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("spectrum_tables: the tables live on the GPU (there is no CPU path)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(H), device)
    if key not in _SPECTRUM_TABLES:
        host = spectrum_host_tables(H)
        _SPECTRUM_TABLES[key] = {k: (v if k == "rings" else torch.from_numpy(v).contiguous().to(device)) for k, v in host.items()}
    return _SPECTRUM_TABLES[key]


def spectrum_u8(images, full=False):
    """-> profile, float64 [N, B] on the device, or (profile, full [N, H, H/2 + 1]) with ``full=True``: the azimuthally averaged power
    spectrum of uint8 device images [N, C, H, H] (H = 16, 32 or 64 -> B = 12, 24 or 46 rings; C = 1 .. 4), ``eg_spectrum_u8``.
    P = |DFT of the bytes|^2 / H^2; profile[n, b] = the weighted mean of P over ring b and the channels, full[n] = the mean of P over the
    channels on the half spectrum kx = 0 .. H/2.  One launch, one workgroup per image, no host read; the bits of an image's row depend
    on its bytes alone."""
    if not (isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and images.dim() == 4 and images.is_contiguous()):
        raise ValueError("spectrum_u8: images must be a contiguous uint8 device tensor [N, C, H, H]")
    if not images.is_cuda:
        raise ValueError("spectrum_u8: images must be a contiguous uint8 device tensor (there is no CPU path)")
    N, C, H, W = (int(v) for v in images.shape)
    if H != W or H not in SPECTRUM_SIDES:
        raise ValueError(f"spectrum_u8: the images must be square with a side in {sorted(SPECTRUM_SIDES)}, got {H} x {W}")
    if not 1 <= C <= SPECTRUM_MAX_C:
        raise ValueError(f"spectrum_u8: C = {C} channels must be in 1 .. {SPECTRUM_MAX_C}")
    if not 1 <= N < 2 ** 31:
        raise ValueError(f"spectrum_u8: images {tuple(images.shape)} holds no image (or 2^31 and more)")
    tab = spectrum_tables(H, images.device)
    profile = torch.empty(N, tab["rings"], device=images.device, dtype=torch.float64)
    whole = torch.empty(N, H, H // 2 + 1, device=images.device, dtype=torch.float64) if full else None
    lib().call("eg_spectrum_u8", _p(images), N, C, H, _p(tab["cos_sin"]), _p(tab["cell_ring"]), _p(tab["ring_start"]), _p(tab["ring_cells"]),
               _p(tab["ring_count"]), _p(profile), _p(whole) if full else None, _stream())
    return (profile, whole) if full else profile


# ---- structural similarity between pairs of uint8 images ---------------------------------------
SSIM_SIDES = (16, 32, 64)
SSIM_MAX_C = 4
SSIM_MAX_K = 11
SSIM_FLAG_PAIR = 2                                    # eg_ssim_u8: a pair with a row index outside its set
_SSIM_WINDOWS = {}


def _ssim_taps(K, what):
    if not (isinstance(K, int) and 3 <= K <= SSIM_MAX_K and K % 2 == 1):
        raise ValueError(f"{what}: the window must have an odd number of taps K in 3 .. {SSIM_MAX_K}, got {K!r}")
    return K


def ssim_window(K=11, sigma=1.5):
    """-> numpy float64 [K]: the one-dimensional window of ``eg_ssim_u8``, exp(-(k - K // 2)^2 / (2 sigma^2)) divided by its sum (Wang et
    al.: K = 11, sigma = 1.5); ``sigma=None``: the uniform window 1 / K.  K odd, 3 .. 11.  The library evaluates no exp: the table is the
    caller's."""
    import numpy as np
    K = _ssim_taps(K, "ssim_window")
    if sigma is None:
        return np.full(K, 1.0 / K, np.float64)
    sigma = float(sigma)
    if not (sigma > 0.0 and sigma < float("inf")):
        raise ValueError(f"ssim_window: sigma = {sigma} must be positive and finite (None: the uniform window)")
    k = np.arange(K, dtype=np.float64) - (K // 2)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum()


def ssim_window_table(K, sigma, device):
    """``ssim_window(K, sigma)`` on ``device`` as a contiguous float64 tensor, built once per (K, sigma, device)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("ssim_window_table: the table lives on the GPU (there is no CPU path)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(K), None if sigma is None else float(sigma), device)
    if key not in _SSIM_WINDOWS:
        _SSIM_WINDOWS[key] = torch.from_numpy(ssim_window(K, sigma)).contiguous().to(device)
    return _SSIM_WINDOWS[key]


def ssim_levels(H, K):
    """-> the largest number of levels L of ``eg_ssim_u8`` for side ``H`` (16, 32 or 64) and a K-tap window: the largest L with
    H >> (L - 1) >= K (64 px: 3 at K = 11; 32 px: 2; 16 px: 1)"""
    H, K = int(H), _ssim_taps(K, "ssim_levels")
    if H not in SSIM_SIDES:
        raise ValueError(f"ssim_levels: the image side must be one of {list(SSIM_SIDES)}, got {H}")
    L = 1
    while (H >> L) >= K:
        L += 1
    return L


def ssim_u8(a, b, pairs, window=None, levels=None, k1=0.01, k2=0.03, flag=None):
    """-> (stats float64 [P, L, 2], sse int64 [P]) on the device, ``eg_ssim_u8``: for every row (i, j) of the int32 device table ``pairs``
    [P, 2], image a[i] against image b[j] of the uint8 device sets a [na, C, H, H] and b [nb, C, H, H] (H = 16, 32 or 64; C = 1 .. 4; a
    may be b).  stats[p, l] = (mean SSIM, mean contrast-structure term cs) over channels and valid window positions of level l of a 2 x 2
    mean pyramid, with c1 = (k1 255)^2, c2 = (k2 255)^2; sse[p] = sum (a - b)^2 over the bytes, exact.  ``window``: a numpy / torch table
    [K] of the one-dimensional window, K odd in 3 .. 11, normalised by the caller (None: the 11-tap Gaussian of ``ssim_window``);
    ``levels``: L with H >> (L - 1) >= K (None: ``ssim_levels``).  A pair with an index outside its set gets NaN and -1 and sets
    ``SSIM_FLAG_PAIR`` in ``flag`` (an int32 device tensor [1], ZEROED BY THE CALLER; not reported without it).  One workgroup per pair,
    no host read; the bits of a pair depend on its two images and the arguments alone."""
    import math
    for name, t in (("a", a), ("b", b)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 4 and t.is_contiguous()):
            raise ValueError(f"ssim_u8: {name} must be a contiguous uint8 device tensor [N, C, H, H]")
        if not t.is_cuda:
            raise ValueError(f"ssim_u8: {name} must be a contiguous uint8 device tensor (there is no CPU path)")
    na, C, H, W = (int(v) for v in a.shape)
    nb = int(b.shape[0])
    if H != W or H not in SSIM_SIDES:
        raise ValueError(f"ssim_u8: the images must be square with a side in {list(SSIM_SIDES)}, got {H} x {W}")
    if not 1 <= C <= SSIM_MAX_C:
        raise ValueError(f"ssim_u8: C = {C} channels must be in 1 .. {SSIM_MAX_C}")
    if tuple(b.shape[1:]) != (C, H, H) or b.device != a.device:
        raise ValueError(f"ssim_u8: the two sets must hold images of one shape on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    if not (1 <= na < 2 ** 31 and 1 <= nb < 2 ** 31):
        raise ValueError(f"ssim_u8: a {tuple(a.shape)} or b {tuple(b.shape)} holds no image (or 2^31 and more)")
    if not (isinstance(pairs, torch.Tensor) and pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.is_contiguous()
            and pairs.device == a.device and 1 <= pairs.shape[0] < 2 ** 31):
        raise ValueError("ssim_u8: pairs must be a contiguous int32 device tensor [P, 2], P >= 1, beside the images")
    P = int(pairs.shape[0])
    if window is None:
        win = ssim_window_table(11, 1.5, a.device)
    else:
        if not isinstance(window, torch.Tensor):
            import numpy as np
            window = torch.from_numpy(np.ascontiguousarray(np.asarray(window, dtype=np.float64)))
        if window.dim() != 1 or not window.is_floating_point():
            raise ValueError("ssim_u8: window must be a floating-point table [K]")
        win = window.detach().to(device=a.device, dtype=torch.float64).contiguous()
    K = _ssim_taps(int(win.shape[0]), "ssim_u8")
    top = ssim_levels(H, K)
    L = top if levels is None else int(levels)
    if not 1 <= L <= top:
        raise ValueError(f"ssim_u8: levels = {L} must be in 1 .. {top} (H >> (L - 1) >= K with H = {H}, K = {K})")
    c1, c2 = (float(k1) * 255.0) ** 2, (float(k2) * 255.0) ** 2
    if not (c1 > 0.0 and c2 > 0.0 and math.isfinite(c1) and math.isfinite(c2)):
        raise ValueError(f"ssim_u8: k1 = {k1} and k2 = {k2} must be positive and finite")
    if flag is None:
        flag = torch.zeros(1, device=a.device, dtype=torch.int32)
    else:
        _i32("ssim_u8", "flag", flag, (1,), a)
    stats = torch.empty(P, L, 2, device=a.device, dtype=torch.float64)
    sse = torch.empty(P, device=a.device, dtype=torch.int64)
    lib().call("eg_ssim_u8", _p(a), na, _p(b), nb, C, H, _p(pairs), P, _p(win), K, L, c1, c2, _p(stats), _p(sse), _p(flag), _stream())
    return stats, sse

"""Affine utilities shared by the four workloads: latent codes -> affine matrices (``ops.theta_<kind>``), the STN warp
(``transformation_2D``, celebA/EAD-GAN_celebA.py:144-158 and its twins) and the autograd bridge of the closed-form regularisers.
All differentiable once; the arithmetic is in the HIP kernels behind :mod:`ops`."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops
from .engine import _require_cuda


class _ThetaFn(torch.autograd.Function):
    """code [B, ld] -> theta [B, 2, 3] by ``ops.theta_<kind>``; backward: ``ops.theta_bwd`` (no double backward)"""

    @staticmethod
    def forward(ctx, code, kind):
        B, ld = code.shape
        theta = torch.empty(B, 2, 3, device=code.device, dtype=torch.float32)
        getattr(ops, "theta_" + kind)(code, ld, B, theta)
        ctx.save_for_backward(code)
        ctx.kind = kind
        return theta

    @staticmethod
    @once_differentiable
    def backward(ctx, dtheta):
        code, = ctx.saved_tensors
        dcode = torch.empty_like(code)
        ops.theta_bwd(ops.THETA_KINDS[ctx.kind], code, code.shape[1], code.shape[0], dtheta.float().contiguous(), dcode)
        return dcode, None


def _code_to_theta(kind, code_input_raw):
    """rows 0, 1 of the kind's matrix, differentiable with respect to the codes"""
    _require_cuda(code_input_raw)
    return _ThetaFn.apply(code_input_raw.float().contiguous(), kind)


def theta_to_matrix(theta):
    """[B,2,3] -> [B,3,3] with the row (0, 0, 1) appended"""
    A = torch.zeros(theta.shape[0], 3, 3, device=theta.device, dtype=torch.float32)
    A[:, :2] = theta
    A[:, 2, 2] = 1.0
    return A


class _WarpFn(torch.autograd.Function):
    """``ops.warp_affine`` / ``ops.warp_affine_zeros``; backward: ``ops.warp_affine_bwd`` for the inputs that need it (no double backward)"""

    @staticmethod
    def forward(ctx, img, theta, zeros):
        out = torch.empty_like(img)
        B, C, H, W = img.shape
        (ops.warp_affine_zeros if zeros else ops.warp_affine)(img, theta, out, B, C, H, W)
        ctx.save_for_backward(img, theta)
        ctx.zeros = zeros
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        img, theta = ctx.saved_tensors
        B, C, H, W = img.shape
        dimg = torch.empty_like(img) if ctx.needs_input_grad[0] else None
        dtheta = torch.empty_like(theta) if ctx.needs_input_grad[1] else None
        ops.warp_affine_bwd(img, theta, dout.float().contiguous(), dimg, dtheta, B, C, H, W, ctx.zeros)
        return dimg, dtheta, None


class transformation_2D(nn.Module):
    """affine_grid + grid_sample(bilinear, ``padding_mode`` 'border' or 'zeros', align_corners=False) as one HIP kernel
    (celebA/EAD-GAN_celebA.py:144-158; 'zeros': colored_dSprites/pxy_color.py:90); differentiable with respect to the image and the matrix."""

    def __init__(self, padding_mode="border"):
        super().__init__()
        if padding_mode not in ("border", "zeros"):
            raise ValueError("transformation_2D: padding_mode must be 'border' or 'zeros'")
        self.padding_mode = padding_mode

    def stn(self, x, matrix_2D):
        _require_cuda(x)
        return _WarpFn.apply(x.float().contiguous(), matrix_2D.float().contiguous(), self.padding_mode == "zeros")

    def forward(self, img, matrix_2D):
        return self.stn(img, matrix_2D)


# The regularizer kernels return the gradient of an MSE, gs * (pred - target) * J with gs = 2 * scale / (n B); the drop-in backward gets J^T dpred
# out of them with target = pred - dpred * (n B / 2).  The kernel then recovers dpred * n B / 2 as a float32 difference of two numbers of size
# |pred|: relative error 2^-24 * |pred| / (|dpred| n B / 2), 2e-4 for an upstream gradient of 1e-6 at B = 128.  Both the target's offset and
# 1 / scale therefore carry the factor GRAD_UP, a power of two (exact in both places): the difference is then GRAD_UP times larger than the
# rounding of pred, and once it exceeds |pred| its error is its own rounding, 2^-24 relative.  Overflow would need |dpred| n B / 2 > 7e28.
GRAD_UP = 2.0 ** 32


def regularizer(kernel, n):
    """-> ``f(real_code, trans_code) -> pred [B, n]``, the drop-in form of a closed-form regulariser, differentiable with respect to both
    codes.  ``kernel(real, trans, ld, B, target, scale, d_real, d_trans, pred)`` wraps the workload's ``ops.loss_affine_*``.  Forward: the
    kernel with a zero target writes ``pred`` (saved).  Backward: d/dcode of sum_j dpred_j * pred_j == the gradient of the kernel's MSE
    with target = pred - dpred * (n B / 2); target and scale carry the power of two GRAD_UP (see there)."""

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, real_code, trans_code):
            B, ld = real_code.shape
            pred = torch.empty(B, n, device=real_code.device, dtype=torch.float32)
            kernel(real_code, trans_code, ld, B, torch.zeros(B, n, device=real_code.device, dtype=torch.float32), 1.0, None, None, pred)
            ctx.save_for_backward(real_code, trans_code, pred)
            return pred

        @staticmethod
        def backward(ctx, dpred):
            real_code, trans_code, pred = ctx.saved_tensors
            B, ld = real_code.shape
            tgt = (pred - dpred.float() * (GRAD_UP * n * B / 2.0)).contiguous()
            d_real, d_trans = torch.empty_like(real_code), torch.empty_like(trans_code)
            kernel(real_code, trans_code, ld, B, tgt, 1.0 / GRAD_UP, d_real, d_trans, None)
            return d_real, d_trans

    def apply(real_code, trans_code):
        _require_cuda(real_code)
        return Fn.apply(real_code.float().contiguous(), trans_code.float().contiguous())
    return apply

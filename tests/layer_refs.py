"""Plain torch references of the layers the HIP kernels compute, for the layer-wise tests: convolutions as unfold / fold + matmul (no MIOpen:
nothing to tune or look up, and the same arithmetic on every device), their per-tap weight gradients, and the spectral-norm Linear / dense
forms.  ``dtype=torch.float64`` runs the same helpers in double precision (references that only the kernel's fp32 summation order may miss)."""
import torch
import torch.nn.functional as F


def _rel(a, b):
    """relative L2 error of ``a`` against the reference ``b`` (computed in the wider of fp32 and the operands' own type)"""
    dt = torch.float64 if torch.float64 in (a.dtype, b.dtype) else torch.float32
    a, b = a.to(dt), b.to(dt)
    return float((a - b).norm() / (b.norm() + 1e-30))


def _conv_ref(x, w, stride=2, pad=1, dtype=torch.float32):
    """Conv2d(x, w) as unfold + matmul in ``dtype``; x [B,Ci,H,W], w [Co,Ci,k,k] -> ([B,Co,OH,OW], cols [B, Ci*k*k, L])"""
    x, w = x.to(dtype), w.to(dtype)
    B, Ci, H, W = x.shape
    Co, _, k, _ = w.shape
    cols = F.unfold(x, k, padding=pad, stride=stride)                       # [B, Ci*k*k, L]
    OH = (H + 2 * pad - k) // stride + 1
    OW = (W + 2 * pad - k) // stride + 1
    return (w.reshape(Co, -1) @ cols).reshape(B, Co, OH, OW), cols


def _convT_ref(g, w, out_hw, stride=2, pad=1, dtype=torch.float32):
    """ConvTranspose2d(g, w) = fold(w^T g) in ``dtype``; g [B,Co,OH,OW], w [Co,Ci,k,k] (conv view) -> [B,Ci,H,W]"""
    g, w = g.to(dtype), w.to(dtype)
    B, Co, OH, OW = g.shape
    k = w.shape[-1]
    cols = w.reshape(Co, -1).t() @ g.reshape(B, Co, OH * OW)                # [B, Ci*k*k, L]
    return F.fold(cols, tuple(out_hw), k, padding=pad, stride=stride)


def _wgrad_ref(dy, x, k=4, stride=2, pad=1, dtype=torch.float64, chunk=64):
    """weight gradient of Conv2d(x -> y) for the output gradient dy: sum_b dY_b . cols_b^T, per tap, in ``dtype``; dy [B,Co,OH,OW],
    x [B,Ci,H,W] -> [Co,Ci,k,k].  Summed ``chunk`` images at a time (the column tensor of a whole 512-image batch in fp64 is GiBs)."""
    B, Co = dy.shape[:2]
    Ci = x.shape[1]
    out = torch.zeros(Co, Ci * k * k, device=dy.device, dtype=dtype)
    for b0 in range(0, B, chunk):
        cols = F.unfold(x[b0:b0 + chunk].to(dtype), k, padding=pad, stride=stride)          # [b, Ci*k*k, L]
        d = dy[b0:b0 + chunk].to(dtype).reshape(cols.shape[0], Co, -1)                   # [b, Co, L]
        out += (d @ cols.transpose(1, 2)).sum(0)
    return out.reshape(Co, Ci, k, k)


def _linear_ref(x, w, bias=None, sigma=None, dtype=torch.float32):
    """y = x w^T / sigma + bias (nn.Linear; spectral norm: the weight is w_orig / sigma); x [B,K], w [N,K]"""
    y = x.to(dtype) @ w.to(dtype).t()
    if sigma is not None:
        y = y / sigma
    return y if bias is None else y + bias.to(dtype)


def _linear_wgrad_ref(dy, x, dtype=torch.float64):
    """sum_b dy_b x_b^T; dy [B,N], x [B,K] -> [N,K]"""
    return dy.to(dtype).t() @ x.to(dtype)


def _sn_rank1(coef, u, v, dtype=torch.float64):
    """sum_t coef[t] u_t v_t^T -- the spectral-norm term of d(loss)/d(w_orig) (coef[t] = <G_t, w_orig> / sigma_t^2 with G_t = dL/dW of tape t);
    u [T,N], v [T,K] -> [N,K]"""
    return (coef.to(dtype)[:, None, None] * u.to(dtype)[:, :, None] * v.to(dtype)[:, None, :]).sum(0)


def _sn_sigma(w, u, v, dtype=torch.float64):
    """sigma = u^T w v (torch.nn.utils.spectral_norm, after the power iteration); w [N, ...] flattened to [N, K]"""
    return float(u.to(dtype) @ (w.reshape(w.shape[0], -1).to(dtype) @ v.to(dtype)))


def _lrelu_mask(a, slope):
    """d lrelu / dz from the stored activation (its sign is the sign of z)"""
    return torch.where(a.float() > 0, 1.0, slope)

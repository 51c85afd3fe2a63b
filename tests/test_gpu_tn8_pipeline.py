"""igemm_tn8's software-pipelined K loop at the shapes where a pipelined loop can go wrong: every prologue / tail length (1, 2, 3, 4, 5, 7
K steps per split, a shorter last split), every patch geometry, every channel width, both 16-bit types, both split targets -- against the
autograd weight gradient of the same 16-bit-rounded operands (computed once per shape on the CPU), per tap, with the tolerances of
test_gpu_kernels.py::test_conv_wgrad_parity_class_kernel; plus two back-to-back launches on different inputs in the same buffers, which
is what a fragment read from a stale ring stage breaks."""
import ctypes
import functools
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

eg = None
ops = None
DEV = "cuda"


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops


def tol(dtype, K):
    """test_gpu_kernels.tol for the 16-bit types"""
    return 3e-2, 2e-2 * math.sqrt(max(K, 1)) / 8


def rq(x, dtype):
    return x.to(torch.bfloat16 if dtype == 1 else torch.float16).float()


def nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV).to(ops.torch_dtype(dtype))


# (B, H (input), Cin, Cout) -> K steps of 64 lattice rows = B * (H / 2)^2 / 64; under 8 steps there is one split, 9 steps split 5 + 4
CASES = [
    # one image per step (8x8 lattice): 1, 2, 3, 4, 5, 7 steps and 5 + 4
    (1, 16, 128, 128), (2, 16, 128, 128), (3, 16, 128, 128), (4, 16, 128, 128), (5, 16, 128, 128), (7, 16, 128, 128), (9, 16, 128, 128),
    (5, 16, 256, 128), (9, 16, 64, 64), (7, 16, 32, 32),
    # four images per step (4x4 lattice): 1 .. 7 steps and 5 + 4
    (4, 8, 32, 32), (8, 8, 64, 64), (12, 8, 128, 128), (16, 8, 32, 32), (20, 8, 64, 64), (28, 8, 128, 128), (36, 8, 64, 64),
    # two lattice rows per step (32x32 lattice): splits of 4 steps (of 4, 8 and 12 with the split target 16)
    (1, 64, 32, 32), (2, 64, 64, 64), (3, 64, 128, 128),
    # a band of 4 rows per step (16x16 lattice): 4 steps
    (1, 32, 128, 128), (1, 32, 64, 64), (1, 32, 32, 32),
]
STEPS = {1: (1,), 2: (2,), 3: (3,), 4: (4,), 5: (5,), 7: (7,), 9: (5, 4)}       # K steps of the case -> K steps per split (lattices below 32x32)


@functools.lru_cache(maxsize=None)
def reference(case, dtype, seed=31):
    """(x, dy, autograd weight gradient) of the 16-bit-rounded operands, fp32 on the CPU; shared by the tests, never written"""
    B, H, Cin, Cout = case
    g = torch.Generator().manual_seed(seed)
    x = rq(torch.randn(B, Cin, H, H, generator=g), dtype)
    w = (torch.randn(Cout, Cin, 4, 4, generator=g) * 0.1).requires_grad_(True)
    y = F.conv2d(x, w, None, 2, 1)
    dy = rq(torch.randn(y.shape, generator=g), dtype)
    y.backward(dy)
    return x, dy, w.grad.detach()


def check_taps(got, want, case, dtype, what=""):
    B, H, _, _ = case
    rt, at = tol(dtype, B * (H // 2) ** 2)
    for t in range(16):
        torch.testing.assert_close(got[:, :, t // 4, t % 4], want[:, :, t // 4, t % 4], rtol=rt, atol=at * 4, msg=lambda m, t=t: f"{what}tap {t}: {m}")


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("case", CASES)
def test_tn8_pipeline(case, dtype):
    B, H, Cin, Cout = case
    x, dy, want = reference(case, dtype)
    c = ops.make_conv(B, H, H, Cin, Cout, 4, 2, 1)
    assert eg._lib.lib().query("eg_conv_wgrad_variant", ctypes.byref(c), dtype) == 2
    xd, dyd = nhwc(x, dtype), nhwc(dy, dtype)
    nbytes = ops.conv_wgrad_ws_bytes(c, dtype)
    steps = B * (H // 2) ** 2 // 64
    for target in (0, 16):
        slab = torch.full((nbytes // 4,), float("nan"), device=DEV)
        ns = ops.conv_wgrad(c, dtype, xd, dyd, slab, target)
        if H < 64:
            assert ns == len(STEPS[steps]), (ns, steps)
        used = slab[: ns * Cout * 16 * Cin]
        grad = torch.zeros(Cout, Cin, 4, 4, device=DEV)
        ops.wgrad_reduce(slab, ns, Cout, Cout, Cin, 16, grad, accumulate=True)
        slab2 = torch.full_like(slab, float("nan"))
        assert ops.conv_wgrad(c, dtype, xd, dyd, slab2, target) == ns
        torch.cuda.synchronize()
        assert not torch.isnan(used).any(), f"target {target}: slab rows left unwritten"
        check_taps(grad.cpu(), want, case, dtype, f"target {target} ")
        assert torch.equal(used, slab2[: used.numel()]), f"target {target}: two launches differ"


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("case", [(5, 16, 128, 128), (9, 16, 64, 64), (28, 8, 128, 128), (2, 64, 64, 64), (1, 32, 32, 32)])
def test_tn8_back_to_back_launches_on_new_inputs(case, dtype):
    """launch A on x1, then -- nothing synchronised in between -- x2 copied into the same buffers on the stream and launch B: the LDS of a
    CU still holds launch A's stages when B's workgroup starts, so a fragment read that runs ahead of its stage's landing wait gives A's
    numbers.  Each result must match its own reference."""
    B, H, Cin, Cout = case
    x1, dy1, want1 = reference(case, dtype)
    x2, dy2, want2 = reference(case, dtype, seed=32)
    c = ops.make_conv(B, H, H, Cin, Cout, 4, 2, 1)
    xa, dya = nhwc(x1, dtype), nhwc(dy1, dtype)
    xb, dyb = nhwc(x2, dtype), nhwc(dy2, dtype)
    xbuf, dybuf = xa.clone(), dya.clone()
    slab = torch.full((ops.conv_wgrad_ws_bytes(c, dtype) // 4,), float("nan"), device=DEV)
    g1, g2 = torch.zeros(Cout, Cin, 4, 4, device=DEV), torch.zeros(Cout, Cin, 4, 4, device=DEV)
    torch.cuda.synchronize()
    ns = ops.conv_wgrad(c, dtype, xbuf, dybuf, slab)
    ops.wgrad_reduce(slab, ns, Cout, Cout, Cin, 16, g1, accumulate=True)
    xbuf.copy_(xb)
    dybuf.copy_(dyb)
    assert ops.conv_wgrad(c, dtype, xbuf, dybuf, slab) == ns
    ops.wgrad_reduce(slab, ns, Cout, Cout, Cin, 16, g2, accumulate=True)
    torch.cuda.synchronize()
    check_taps(g1.cpu(), want1, case, dtype, "launch A ")
    check_taps(g2.cpu(), want2, case, dtype, "launch B ")

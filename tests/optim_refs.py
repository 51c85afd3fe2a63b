"""float64 restatements for the optimizer-lane tests (tests/test_optim_refs_host.py, tests/test_gpu_optim_lane.py), written for that purpose
from the formulas of include/eadgan_hip.h and the semantics of torch.optim.Adam and torch.nn.utils.spectral_norm -- no code of the package
is used:

* ``adam``: the element update of eg_adam_step (exp_avg.lerp_, exp_avg_sq, bias correction from the step counter AFTER the tick), with mutants;
* ``power_iter``: one spectral-norm power iteration (v from W^T u, u from W v, sigma from the updated pair) or the eval form, with mutants;
* ``fwd_panel`` / ``rows_panel``: the closed forms of the packed panels eg_adam_pack_conv / eg_adam_pack_rows refresh;
* the case tables of the two tests and the cached cases (inputs, float64 results, float32 yardsticks) they share.

The C ABI takes lr, the betas and eps as ``float``: every restatement rounds them through float32 first, whatever it computes in."""
import functools
import math

import torch

from input_grad_refs import K, MUTANT_FACTOR, TORCH_DTYPE, dist           # noqa: F401  (the tests read them from here)

LR, BETAS, EPS = 2e-4, (0.5, 0.999), 1e-8          # celebA/EAD-GAN_celebA.py:211-217
BETAS_TORCH = (0.9, 0.999)                         # torch.optim.Adam's defaults (the projection loop): the other branch of lerp
SN_EPS = 1e-12
GRAD_SCALES = (1e-6, 1e-3, 10.0)

# ---- case tables ---------------------------------------------------------------------------------------------------------------------------
# flat Adam: below the alignment head, around one and two float4, one either side of a 256-thread block, several blocks with ragged ends;
# the large length needs more float4 than 2048 blocks of 256 threads hold, so the grid-stride loop runs
ADAM_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 255, 257, 1027)
ADAM_LARGE = 2097152 + 5
ADAM_T0 = (0, 4, 100000)
ADAM_OFFSETS = (0, 1, 2, 3)                        # floats between a 16-byte boundary and p
ADAM_ALIGN = {"same": (0, 0, 0), "g+1": (1, 0, 0), "mv+2": (0, 2, 2)}           # extra floats of offset of g, m, v against p
ADAM_LARGE_RUNS = ((0, "same"), (3, "same"), (0, "g+1"))
FILL_LENGTHS = (0, 1, 255, 4096 * 256 + 3)         # the last one: past the 4096-block cap
# (Cout, Cin, k, stride, pad)
CONV_LAYERS = ((16, 32, 4, 2, 1), (48, 64, 4, 2, 1), (16, 32, 3, 1, 1), (32, 32, 4, 1, 0))
CONV_LAYER_MAYBE = (32, 32, 3, 2, 1)               # run where eg_adam_pack_conv_ok accepts it (it does), else its refusal is asserted
CONV_LAYER_REFUSED = (16, 24, 4, 2, 1)             # Cin no multiple of 32
CONV_WAYS = {"both": (True, True), "fwd": (True, False), "bwd": (False, True)}
# (K, Cout): N = 16 * Cout, n_mod = 16, n_mul = Cout
ROWS_CASES = ((8, 16), (13, 24), (218, 16), (5, 16))
SN_CASES = ((1, 1), (1, 257), (7, 255), (8, 256), (9, 1025), (17, 9), (64, 4096))
SN_EXTRA = (3, 5)                                  # the eighth layer of the multi launch
SN_ITERS = 3


def f32(x):
    """a Python float rounded through float32 (what a ``float`` argument of the C ABI holds)"""
    return float(torch.tensor(x, dtype=torch.float32))


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, t0, steps, lr, b1, b2, eps, dtype=torch.float64, mutant=None):
    """``steps`` updates with the gradients g[0..steps) from the step counter ``t0`` -> (p, m, v) in ``dtype``.  Update k ticks the counter to
    t = t0 + k + 1 and corrects with it.  Mutants: ``stale_step`` (correction from t - 1), ``no_bc2`` (second moment uncorrected),
    ``eps_in_sqrt`` (eps added under the root), ``swapped_lerp`` (m moved toward g by b1, not by 1 - b1)"""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    T = lambda x: torch.tensor(x, dtype=dtype)
    p, m, v = p.to(dtype).clone(), m.to(dtype).clone(), v.to(dtype).clone()
    w = T(1.0) - T(b1)
    for k in range(steps):
        t = t0 + k + 1
        tc = t - 1 if mutant == "stale_step" else t
        bc1, bc2 = 1.0 - b1 ** tc, 1.0 - b2 ** tc                       # in double, like the kernels' coefficients
        step_size, bc2_sqrt = T(lr / bc1), T(1.0 if mutant == "no_bc2" else math.sqrt(bc2))
        gk = g[k].to(dtype)
        m = torch.lerp(m, gk, T(b1) if mutant == "swapped_lerp" else w)
        v = v * T(b2) + (T(1.0) - T(b2)) * gk * gk
        denom = torch.sqrt(v / (bc2_sqrt * bc2_sqrt) + T(eps)) if mutant == "eps_in_sqrt" else torch.sqrt(v) / bc2_sqrt + T(eps)
        p = p - step_size * (m / denom)
    return p, m, v


def adam_yardstick(c, betas=BETAS):
    """(float64 p, m, v; the case's yardstick): the worst of the three distances of the float32 restatement"""
    args = (c["p"], c["g"], c["m"], c["v"], c["t0"], c["g"].shape[0], LR, betas[0], betas[1], EPS)
    want = adam(*args)
    return want, max(dist(a, b) for a, b in zip(adam(*args, dtype=torch.float32), want))


def adam_inputs(n, t0, scales=GRAD_SCALES, seed=0):
    """float32 operands of an Adam case: DCGAN-sized parameters, one gradient per scale, and the moments ``t0`` earlier gradients of the first
    scale would have left (zero at t0 = 0, where torch creates them)"""
    gen = torch.Generator().manual_seed(100003 * seed + 31 * n + t0 % 1009 + len(scales))
    p = 0.02 * torch.randn(n, generator=gen)
    g = torch.stack([s * torch.randn(n, generator=gen) for s in scales])
    if t0 == 0:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = 0.5 * scales[0] * torch.randn(n, generator=gen)
        v = scales[0] ** 2 * (1.0 - BETAS[1] ** t0) * (0.5 + torch.rand(n, generator=gen))
    return dict(p=p, g=g, m=m, v=v, t0=t0)


@functools.lru_cache(maxsize=None)
def adam_case(n, t0, scales=GRAD_SCALES, betas=BETAS, seed=0):
    c = adam_inputs(n, t0, scales, seed)
    c["want"], c["yard"] = adam_yardstick(c, betas)
    return c


def adam_mutants(t0, scales, betas):
    """the mutants a host case declares: a stale counter shows only while the corrections still move (and t - 1 = 0 divides by zero), the
    missing second correction while it differs from 1, eps under the root where the root is small, the exchanged weight where b1 != 1 - b1"""
    out = []
    if t0 in (1, 4):
        out.append("stale_step")
    if t0 in (0, 1, 4):
        out.append("no_bc2")
    if scales == (1e-6,):
        out.append("eps_in_sqrt")
    if betas[0] != 0.5:
        out.append("swapped_lerp")
    return out


# (t0, scales, betas): every t0 of the GPU test plus t0 = 1; the GPU test's sequence and each of its scales alone; both beta pairs
ADAM_HOST_CASES = tuple((t0, sc, b) for t0 in (0, 1, 4, 100000) for sc in (GRAD_SCALES,) + tuple((s,) for s in GRAD_SCALES)
                        for b in (BETAS, BETAS_TORCH))
ADAM_HOST_N = 1027


# ---- spectral norm -------------------------------------------------------------------------------------------------------------------------
def normalize(x, eps):
    """F.normalize(x, dim=0, eps=eps)"""
    return x / x.norm().clamp_min(eps)


def power_iter(W, u, v, eps, training, dtype=torch.float64, mutant=None):
    """one power iteration of torch.nn.utils.spectral_norm on W [R, Kd] -> (u, v, sigma); ``training`` False: u and v as they are,
    sigma = u . (W v).  Mutants: ``sigma_from_old_u`` (sigma with the u of before the iteration), ``u_from_old_v`` (u from W v_old)"""
    W, u, v = W.to(dtype), u.to(dtype), v.to(dtype)
    if not training:
        return u, v, torch.dot(u, torch.mv(W, v))
    vn = normalize(torch.mv(W.t(), u), eps)
    un = normalize(torch.mv(W, v if mutant == "u_from_old_v" else vn), eps)
    return un, vn, torch.dot(u if mutant == "sigma_from_old_u" else un, torch.mv(W, vn))


def sn_inputs(R, Kd, seed=0):
    """W like a DCGAN-initialised layer, u and v unit vectors like torch's spectral_norm draws them"""
    gen = torch.Generator().manual_seed(7919 * seed + 131 * R + Kd)
    W = 0.02 * torch.randn(R, Kd, generator=gen)
    u = normalize(torch.randn(R, generator=gen), SN_EPS)
    v = normalize(torch.randn(Kd, generator=gen), SN_EPS)
    return W, u, v


def sigma_orders(W, u, v, dtype):
    """the eval form's sigma = u . (W v) in ``dtype`` with its R x Kd products summed in four orders: rows first (W v, then u), columns
    first (W^T u, then v), and both again with every product u_r W_rk v_k formed before any sum.  The eval form has this one scalar as its
    whole output, and a scalar has a single rounding error that one order can hit or miss by luck (the same order gives 3e-9 on one CPU and
    8e-8 on another at R = 17); a kernel may sum in any order, so the eval yardstick is the worst of these float32 restatements."""
    W, u, v = W.to(dtype), u.to(dtype), v.to(dtype)
    prods = u[:, None] * W * v[None, :]
    return [torch.dot(u, torch.mv(W, v)), torch.dot(torch.mv(W.t(), u), v), prods.sum(1).sum(), prods.sum(0).sum()]


def sn_yardstick(got, want):
    """the worst of the distances of u, v and sigma"""
    return max(dist(a, b) for a, b in zip(got, want))


@functools.lru_cache(maxsize=None)
def sn_case(R, Kd, seed=0):
    """inputs, the float64 (u, v, sigma) after each of SN_ITERS training iterations with the float32 restatement's yardstick of that
    iteration, and the same for the eval form on the initial u and v"""
    W, u, v = sn_inputs(R, Kd, seed)
    c = dict(W=W, u=u, v=v, train=[], eval=None)
    s64, s32 = (u, v), (u, v)
    for _ in range(SN_ITERS):
        r64, r32 = power_iter(W, *s64, SN_EPS, True), power_iter(W, *s32, SN_EPS, True, dtype=torch.float32)
        c["train"].append((r64, sn_yardstick(r32, r64)))
        s64, s32 = r64[:2], r32[:2]
    e64 = power_iter(W, u, v, SN_EPS, False)
    c["eval"] = (e64, max(dist(s32, e64[2]) for s32 in sigma_orders(W, u, v, torch.float32)))
    return c


def sn_mutants(R, Kd):
    """with one row u stays +-1, so the old u gives the same sigma; with one column v_old and v_new are both +-1"""
    return (["sigma_from_old_u"] if R > 1 else []) + (["u_from_old_v"] if Kd > 1 else [])


# ---- packed panels -------------------------------------------------------------------------------------------------------------------------
def fwd_panel(w, Cout, Cin, T):
    """wp[n][t*Cin + c] = w[n][c][t] of the conv-view master [Cout][Cin][T]"""
    return w.reshape(Cout, Cin, T).permute(0, 2, 1).reshape(Cout, T * Cin)


def rows_panel(w, Kr, N, Kpad, n_mod, n_mul):
    """wp[(n % n_mod)*n_mul + n / n_mod][k] = w[k][n] of the master [Kr][N], zero for k >= Kr"""
    n = torch.arange(N)
    out = torch.zeros(N, Kpad, dtype=w.dtype)
    out[(n % n_mod) * n_mul + n // n_mod, :Kr] = w.reshape(Kr, N).t()
    return out


def pack_inputs(n, seed):
    """operands of a fused Adam + pack case: two updates from t0 = 0 with gradients of the 1e-3 scale"""
    return adam_inputs(n, 0, (1e-3, 1e-3), seed)


@functools.lru_cache(maxsize=None)
def pack_case(n, seed):
    c = pack_inputs(n, seed)
    c["want"], c["yard"] = adam_yardstick(c)
    return c

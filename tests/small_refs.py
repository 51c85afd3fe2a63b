"""float64 restatements for the skinny-end tests (tests/test_small_refs_host.py, tests/test_gpu_small.py), written for that purpose from the
formulas of include/eadgan_hip.h and the comments of csrc/small.hip -- no code of the package is used:

* the small-N dense head: ``dense_fwd`` (y = x Wp^T / sigma[tape] + bias), ``dense_bwd`` (dx = (dy Wp) * act'(mask) / sigma[tape]),
  ``dense_wgrad`` (gw[n][ci][t] += sum_b dy[b][n] x[b][t*Cin + ci]), ``bgrad`` and ``head_prep`` (eg_head_prep_sn);
* the image side: ``patches`` (one gather of the k x k windows) and on it ``conv_img`` (eg_conv_img_fwd with its epilogue),
  ``conv_img_wgrad`` (the per-image slab) and ``im2col``; ``col2im`` (eg_col2im_img);
* the helpers ``act_grad_bias``, ``flat_reduce``, ``cast_pad`` and ``wgrad_c1`` (the per-unit slabs of eg_wgrad_c1);
* the launch arithmetic of the launchers as pure functions (``ns_of``, ``kper_of``, ``gy_of``, ``cpt_of``, ``maxt_of``, ...);
* the case tables of the two tests and the cached cases (operands, float64 results, float32 yardsticks) they share.

Every restatement takes ``dtype=`` (float64, or float32 for the yardstick) and ``mutant=`` (a plausible kernel mistake).  Operands are
pre-rounded to the compute dtype and kept as float32 tensors that hold values of that dtype.  Every output has a yardstick of its own (gw
and gb; dys, coef and gb; out and gb), in the dtype the kernel stores THAT output in.  Two departures, each for outputs of a few numbers:
the dense-head forward and backward have one yardstick per case, the worst over the variants (bias, sigma forms, masks) the GPU test runs on
it -- at (1, 1, 1) a variant has 1 to 8 outputs, and with 16-bit operands eight exact products without a bias are exact in float32: such a
yardstick is luck or zero, and says nothing about a correct kernel that adds in another order; eg_head_prep_sn's coef and gb take the worst
of three float32 summation orders (``yard_orders``).  A copy (one row stored, no activation, no sigma in f32) has the yardstick zero."""
import functools

import torch
import torch.nn.functional as F

from input_grad_refs import K, MUTANT_FACTOR, TORCH_DTYPE, dist           # noqa: F401  (the tests read them from here)

DTYPES = ("f32", "bf16", "f16")
VEC = {"f32": 4, "bf16": 8, "f16": 8}              # elements of a 16-byte vector
BK = {"f32": 32, "bf16": 64, "f16": 64}            # the engines' K block (ops.bk): the unit of the panels' K padding
SLOPE = 0.2
DS_ROWS = 4                                         # EG_DS_ROWS: batch rows per workgroup of the dense head
SIGMAS = (1.7, 0.6, 2.3)                            # one spectral norm per tape


def rq(x, dtype):
    """``x`` rounded to the dtype, as float32"""
    return x.to(TORCH_DTYPE[dtype]).float()


def stored(x, dtype):
    """a float32 result as the kernel stores it in ``dtype``"""
    return x.float().to(TORCH_DTYPE[dtype]).float()


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(v, m):
    return cdiv(v, m) * m


def act(v, name, slope=SLOPE):
    if name == "lrelu":
        return torch.where(v > 0, v, v * slope)
    if name == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    if name == "tanh":
        return torch.tanh(v)
    if name == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-v))
    return v


def act_grad_from_out(a, name, slope=SLOPE):
    """act'(z) expressed through the output a = act(z)"""
    one = torch.ones_like(a)
    if name == "lrelu":
        return torch.where(a > 0, one, one * slope)
    if name == "relu":
        return torch.where(a > 0, one, torch.zeros_like(a))
    if name == "tanh":
        return 1.0 - a * a
    if name == "sigmoid":
        return a * (1.0 - a)
    return one


def worst(got, want):
    return max(dist(a, b) for a, b in zip(got, want))


def each(got, want):
    """one distance per output"""
    return tuple(dist(a, b) for a, b in zip(got, want))


ORDERS = ("torch", "ascending", "descending")


def sum_rows(x, order="torch"):
    """sum over dim 0: torch's blocked sum, or one row after the other from either end"""
    if order == "torch":
        return x.sum(0)
    acc = torch.zeros_like(x[0])
    for r in (x if order == "ascending" else x.flip(0)):
        acc = acc + r
    return acc


def yard_orders(fn, want):
    """per output the worst distance of the float32 restatement ``fn(order)`` over ORDERS.  Used for eg_head_prep_sn, whose coef is ONE
    scalar per tape and whose gb has as few as one column: a scalar has a single rounding error that one order can hit or miss by luck,
    and a kernel may add in any order (the rule optim_refs.sigma_orders follows for the scalar sigma)"""
    ds = [each(fn(o), want) for o in ORDERS]
    return tuple(max(d[i] for d in ds) for i in range(len(want)))


# ---- launch arithmetic (the launchers' formulas, restated) -----------------------------------------------------------------------------
def ns_of(B, Kd, vec, ws_floats, N):
    """K slices of the dense forward: doubled while the row groups do not fill 256 workgroups and a slice keeps a full 256-vector sweep,
    halved until ns * B * N floats fit the workspace; 1 without a workspace"""
    if not ws_floats:
        return 1
    groups, ns = cdiv(B, DS_ROWS), 1
    while ns < 16 and groups * ns < 256 and Kd // (ns * 2) >= 256 * vec:
        ns *= 2
    while ns > 1 and ns * B * N > ws_floats:
        ns //= 2
    return ns


def kper_of(Kd, vec, ns):
    """elements of one K slice: whole vectors"""
    return Kd if ns == 1 else cdiv(cdiv(Kd, vec), ns) * vec


def kblocks_of(Kd, vec):
    return cdiv(Kd, 256 * vec)


def gy_of(B, Kd, vec):
    """workgroups along K of the dense backward"""
    groups, kb, gy = cdiv(B, DS_ROWS), kblocks_of(Kd, vec), 1
    while gy * 2 <= kb and groups * gy < 512:
        gy *= 2
    return gy


def conv_out(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def cpt_of(H, W, N, k, s, p):
    """output channels per thread of eg_conv_img_fwd, or None where the launcher refuses"""
    _, OW = conv_out(H, W, k, s, p)
    if OW > 256 or 256 % OW:
        return None
    groups = 256 // OW
    if N % groups and N >= groups:
        return None
    cpt = N // groups if N >= groups else 1
    return cpt if cpt in (1, 2, 4, 8, 16) else None


def wgrad_lds_bytes(CI, H, W, p):
    return CI * (H + 2 * p) * (W + 2 * p) * 4


def maxt_of(CI, N, k):
    """taps per thread of eg_conv_img_wgrad"""
    return cdiv(CI * k * k, 256 // N)


def maxt_bucket(maxt):
    """the MAXT template the launcher picks, None past 24"""
    for b in (1, 2, 3, 6, 12, 24):
        if maxt <= b:
            return b
    return None


def im2col_blocks(B, CI, H, W, k, s, p, Kp, vec):
    """(output vectors, workgroups of 256 threads): capped at 8192"""
    OH, OW = conv_out(H, W, k, s, p)
    total = B * OH * OW * (Kp // vec)
    return total, min(cdiv(total, 256), 8192)


def im2col_template(k):
    return k if k in (3, 4) else 0


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------
# dense head, (B, q, N) with K = q * VEC
DENSE_CASES = ((1, 1, 1), (5, 257, 9), (6, 512, 19), (6, 513, 19), (3, 2051, 64), (130, 1024, 8))
DENSE_CLIPPED = (3, 2051, 64)                       # also run with exactly 2 * B * N workspace floats
# what the issue quotes: case -> (ns with a full workspace, kblocks, gy)
DENSE_LAUNCH = {(1, 1, 1): (1, 1, 1), (5, 257, 9): (1, 2, 2), (6, 512, 19): (2, 2, 2), (6, 513, 19): (2, 3, 2), (3, 2051, 64): (8, 9, 8),
                (130, 1024, 8): (4, 4, 4)}
# (B, K, N, Cin, taps)
DENSE_WGRAD_CASES = ((1, 8, 1, 8, 1), (5, 40, 9, 8, 5), (6, 1024, 19, 64, 16), (7, 264, 32, 264, 1), (512, 8, 32, 8, 1))
BGRAD_CASES = ((1, 1), (7, 19), (8, 64), (9, 33), (1000, 19))
# (rows, rows_per_tape, N, npad, col0) and the variant each case runs besides the full one
HEAD_PREP_CASES = ((4, 4, 1, 8, 0), (6, 2, 9, 16, 7), (12, 4, 19, 32, 8), (300, 100, 33, 64, 16), (256, 128, 64, 64, 0))
HEAD_PREP_EXTRA = ("no_sigma", "no_coef", "no_gb", "dys32", "dys32")
# (B, CI, H, W, N, k, s, p) -> channels per thread
CONV_IMG_CASES = {(2, 1, 4, 4, 32, 4, 1, 0): 1, (2, 3, 12, 16, 64, 4, 2, 1): 2, (2, 3, 32, 32, 64, 4, 2, 1): 4, (2, 1, 64, 64, 64, 4, 2, 1): 8,
                  (2, 3, 64, 64, 128, 4, 2, 1): 16, (3, 1, 32, 32, 16, 3, 2, 1): 1, (2, 4, 8, 8, 64, 3, 1, 1): 2, (2, 2, 6, 8, 4, 3, 1, 1): 1,
                  (2, 2, 5, 8, 32, 3, 1, 1): 1}
CONV_IMG_REFUSED = ((2, 3, 32, 32, 24, 4, 2, 1), (1, 1, 128, 128, 128, 4, 2, 1))        # N = 24 with OW = 16; cpt = 32
CONV_IMG_EPILOGUES = ("plain", "bias_sigma_lrelu", "mask")
# B = 3, (CI, H, W, N, k, s, p) -> taps per thread
CONV_WGRAD_B = 3
CONV_WGRAD_CASES = {(1, 8, 8, 1, 4, 2, 1): 1, (1, 8, 8, 16, 4, 2, 1): 1, (3, 8, 8, 8, 4, 2, 1): 2, (1, 8, 8, 64, 3, 2, 1): 3,
                    (4, 8, 8, 32, 3, 1, 1): 5, (3, 8, 8, 32, 4, 2, 1): 6, (2, 8, 8, 128, 3, 1, 1): 9, (3, 64, 64, 64, 4, 2, 1): 12,
                    (1, 8, 8, 256, 4, 2, 1): 16, (2, 8, 8, 256, 3, 1, 1): 18, (3, 12, 16, 128, 4, 2, 1): 24}
CONV_WGRAD_REFUSED = ((4, 8, 8, 128, 4, 2, 1), (4, 64, 64, 32, 4, 2, 1))                # 32 taps; 69 696 bytes of LDS
# (B, CI, H, W, k, s, p, Kp); the last one in fp32 only: more vectors than 8192 blocks of 256 threads hold
IM2COL_CASES = ((2, 1, 7, 9, 3, 1, 1, 16), (2, 2, 8, 8, 5, 1, 2, 56), (2, 4, 6, 6, 2, 2, 0, 16))
IM2COL_LARGE = (43, 3, 128, 128, 4, 2, 1, 48)
# (C, B, Hin, Win, k, s, p)
COL2IM_CASES = ((3, 2, 5, 8, 4, 2, 1), (1, 3, 4, 6, 3, 2, 1), (3, 1, 1, 1, 4, 1, 0))
COL2IM_ACTS = ("none", "tanh", "sigmoid")
ACT_GRAD_CASES = ((1, 1, 1), (9, 3, 100), (7, 33, 300), (130, 64, 16))
ACT_GRAD_ACTS = ("none", "lrelu", "tanh", "sigmoid")
FLAT_REDUCE_CASES = ((1, 1), (3, 255), (4, 257), (2, 1024 * 256 + 5))
CAST_PAD_CASES = ((1, 1, 1), (7, 19, 32), (300, 3, 8), (5, 0, 8))
WGRAD_C1_CASES = ((1, 8, 8), (1, 8, 128), (2, 16, 8))
WGRAD_C1_REFUSED = ((8, 136), (12, 8))              # (H, W)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ---- dense head ----------------------------------------------------------------------------------------------------------------------------
def tape_of(B, sigma_rows, mutant=None):
    """index into sigma of every row: b / sigma_rows, 0 for sigma_rows == 0"""
    if not sigma_rows or mutant == "sigma0":
        return torch.zeros(B, dtype=torch.long)
    return torch.arange(B) // sigma_rows


def dense_fwd(x, w, bias, sigma, sigma_rows, dtype=torch.float64, mutant=None, vec=4, ns=1):
    """y[b][n] = sum_k x[b][k] w[n][k] / sigma[b / sigma_rows] + bias[n].  Mutants: ``drop_tail`` (K ends at the last full sweep of 256
    vectors), ``double_boundary`` (the first element of every K slice but the first is counted twice), ``sigma0`` (sigma[0] for every
    tape)"""
    x, w = x.to(dtype), w.to(dtype)
    B, Kd = x.shape
    if mutant == "drop_tail":
        kk = Kd // (256 * vec) * (256 * vec)
        y = x[:, :kk] @ w[:, :kk].t()
    else:
        y = x @ w.t()
    if mutant == "double_boundary":
        kper = kper_of(Kd, vec, ns)
        for z in range(1, ns):
            y = y + x[:, z * kper, None] * w[None, :, z * kper]
    if sigma is not None:
        y = y / sigma.to(dtype)[tape_of(B, sigma_rows, mutant)][:, None]
    return y if bias is None else y + bias.to(dtype)


def dense_bwd(dy, w, mask, mask_act, sigma, sigma_rows, dtype=torch.float64, mutant=None):
    """dx[b][k] = (sum_n dy[b][n] w[n][k]) * act'(mask[b][k]) / sigma[b / sigma_rows].  Mutant ``mul_sigma``: multiplied by sigma"""
    dx = dy.to(dtype) @ w.to(dtype)
    if mask is not None:
        dx = dx * act_grad_from_out(mask.to(dtype), mask_act)
    if sigma is not None:
        s = sigma.to(dtype)[tape_of(dy.shape[0], sigma_rows)][:, None]
        dx = dx * s if mutant == "mul_sigma" else dx / s
    return dx


def dense_wgrad(dy, x, gw0, gb0, Cin, taps, dtype=torch.float64, mutant=None):
    """gw[n][ci][t] = gw0 + sum_b dy[b][n] x[b][t*Cin + ci], gb = gb0 + sum_b dy -> (gw, gb); gb0 None: no bias gradient.  Mutants:
    ``k_ci_major`` (k taken as ci*taps + t), ``store`` (gw0 overwritten)"""
    N = dy.shape[1]
    g = dy.to(dtype).t() @ x.to(dtype)                                   # [N][K]
    g = g.reshape(N, Cin, taps) if mutant == "k_ci_major" else g.reshape(N, taps, Cin).permute(0, 2, 1)
    gw = g if mutant == "store" else gw0.to(dtype) + g
    return gw, (None if gb0 is None else gb0.to(dtype) + dy.to(dtype).sum(0))


def bgrad(dy, gb0, accumulate, dtype=torch.float64, mutant=None):
    """gb[n] (+)= sum_b dy[b][n].  Mutant ``full_strides``: the rows past the last full stride of the 8 row groups are missed"""
    rows = dy.shape[0] // 8 * 8 if mutant == "full_strides" else dy.shape[0]
    s = dy[:rows].to(dtype).sum(0)
    return gb0.to(dtype) + s if accumulate else s


def head_prep(dy, y, bias, sigma, rows_per_tape, gb0, dtype=torch.float64, mutant=None, order="torch"):
    """dys = dy / sigma[tape], coef[tape] = sum dys * (y - bias), gb = gb0 + sum_rows dy -> (dys, coef, gb).  Mutant ``lane_tail``: the
    column sums of gb miss the rows past the last full stride of the 256 / Np row lanes (Np = N rounded up to a power of two)"""
    rows, N = dy.shape
    dy, y, bias = dy.to(dtype), y.to(dtype), bias.to(dtype)
    tape = torch.arange(rows) // rows_per_tape
    dys = dy if sigma is None else dy / sigma.to(dtype)[tape][:, None]
    coef = sum_rows((dys * (y - bias)).sum(1).reshape(rows // rows_per_tape, rows_per_tape).t(), order)
    used = rows
    if mutant == "lane_tail":
        Np = 1
        while Np < N:
            Np *= 2
        used = rows // (256 // Np) * (256 // Np)
    return dys, coef, gb0.to(dtype) + sum_rows(dy[:used], order)


def dense_variants(B):
    """(with bias, sigma form) of the forward and (mask activation, sigma form) of the backward; sigma form None: no sigma, 0: sigma[0] for
    all rows, 2: one sigma per tape of 2 rows (B = 6 = 3 tapes)"""
    fwd = [(True, None), (False, None), (True, 0), (False, 0)] + ([(True, 2)] if B == 6 else [])
    bwd = [(None, None), ("lrelu", None), ("relu", 0), (None, 0)] + ([("lrelu", 2), (None, 2)] if B == 6 else [])
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def dense_case(case, dtype):
    """operands of a dense-head case, the float64 result of every variant and the case's two yardsticks (forward: y fp32; backward: dx in
    the dtype)"""
    B, q, N = case
    Kd = q * VEC[dtype]
    g = _gen(B, q, N, DTYPES.index(dtype))
    c = dict(x=rq(torch.randn(B, Kd, generator=g), dtype), w=rq(0.05 * torch.randn(N, Kd, generator=g), dtype),
             bias=0.1 * torch.randn(N, generator=g), dy=torch.randn(B, N, generator=g), mask=rq(torch.randn(B, Kd, generator=g), dtype),
             sigma=torch.tensor(SIGMAS), K=Kd, fwd={}, bwd={})
    fv, bv = dense_variants(B)
    yf = yb = 0.0
    for has_bias, sf in fv:
        args = (c["x"], c["w"], c["bias"] if has_bias else None, None if sf is None else c["sigma"], sf or 0)
        c["fwd"][(has_bias, sf)] = dense_fwd(*args)
        yf = max(yf, dist(dense_fwd(*args, dtype=torch.float32), c["fwd"][(has_bias, sf)]))
    for ma, sf in bv:
        args = (c["dy"], c["w"], None if ma is None else c["mask"], ma, None if sf is None else c["sigma"], sf or 0)
        c["bwd"][(ma, sf)] = dense_bwd(*args)
        yb = max(yb, dist(stored(dense_bwd(*args, dtype=torch.float32), dtype), c["bwd"][(ma, sf)]))
    c["yard_fwd"], c["yard_bwd"] = yf, yb
    return c


@functools.lru_cache(maxsize=None)
def dense_wgrad_case(case, dtype):
    B, Kd, N, Cin, taps = case
    g = _gen(B, Kd, N, Cin, taps, DTYPES.index(dtype))
    c = dict(dy=torch.randn(B, N, generator=g), x=rq(torch.randn(B, Kd, generator=g), dtype), gw0=torch.randn(N, Cin, taps, generator=g),
             gb0=torch.randn(N, generator=g))
    args = (c["dy"], c["x"], c["gw0"], c["gb0"], Cin, taps)
    c["want"] = dense_wgrad(*args)
    c["yard"] = each(dense_wgrad(*args, dtype=torch.float32), c["want"])                                    # (gw, gb)
    return c


@functools.lru_cache(maxsize=None)
def bgrad_case(case):
    B, N = case
    g = _gen(B, N, 41)
    c = dict(dy=torch.randn(B, N, generator=g), gb0=torch.randn(N, generator=g), want={}, yard={})
    for acc in (0, 1):
        c["want"][acc] = bgrad(c["dy"], c["gb0"], acc)
        c["yard"][acc] = dist(bgrad(c["dy"], c["gb0"], acc, dtype=torch.float32), c["want"][acc])
    return c


HEAD_PREP_VARIANTS = ("full", "no_sigma", "no_coef", "no_gb", "dys32")


def head_prep_sigma(c, variant):
    return None if variant == "no_sigma" else c["sigma"]


@functools.lru_cache(maxsize=None)
def head_prep_case(case, dtype):
    """operands (dense [rows][N]; the GPU test spreads them to the row strides ldy and ldyy) and, with and without sigma, the float64
    (dys, coef, gb) and one yardstick for each of the three: dys as stored in the dtype, coef and gb (fp32 in every dtype) as float32
    gives them"""
    rows, rpt, N, npad, col0 = case
    g = _gen(rows, rpt, N, npad, col0, DTYPES.index(dtype))
    c = dict(dy=torch.randn(rows, N, generator=g), y=torch.randn(rows, N, generator=g), bias=0.1 * torch.randn(N, generator=g),
             sigma=0.5 + torch.rand(rows // rpt, generator=g) * 2, gb0=torch.randn(N, generator=g), want={}, yard={}, yard32={})
    for key, sigma in (("sigma", c["sigma"]), ("plain", None)):
        args = (c["dy"], c["y"], c["bias"], sigma, rpt, c["gb0"])
        c["want"][key] = head_prep(*args)
        def f32(o, args=args):
            d32, c32, g32 = head_prep(*args, dtype=torch.float32, order=o)
            return stored(d32, dtype), c32, g32
        c["yard"][key] = yard_orders(f32, c["want"][key])               # (dys, coef, gb)
        c["yard32"][key] = dist(head_prep(*args, dtype=torch.float32)[0], c["want"][key][0])          # of the fp32 copy dys32
    return c


# ---- image side ----------------------------------------------------------------------------------------------------------------------------
def patches(img, k, s, p):
    """the k x k windows of the zero-padded image: [B][OH][OW][CI][k][k]"""
    x = F.pad(img, (p, p, p, p))
    return x.unfold(2, k, s).unfold(3, k, s).permute(0, 2, 3, 1, 4, 5)


def conv_img(img, w, s, p, bias=None, sigma=None, act_name="none", slope=SLOPE, mask=None, mask_act="none", dtype=torch.float64, mutant=None):
    """out[b][oy][ox][n] = act(conv(img, w) / sigma + bias) * act'(mask), NHWC.  Mutants: ``swap_khkw`` (the weight's kh and kw exchanged),
    ``bias_before_sigma`` (the bias divided by sigma too)"""
    w = w.transpose(2, 3) if mutant == "swap_khkw" else w
    z = torch.einsum("bhwcij,ncij->bhwn", patches(img.to(dtype), w.shape[-1], s, p), w.to(dtype))
    if mutant == "bias_before_sigma" and bias is not None:
        z = z + bias.to(dtype)
    if sigma is not None:
        z = z / sigma.to(dtype)
    if mutant != "bias_before_sigma" and bias is not None:
        z = z + bias.to(dtype)
    z = act(z, act_name, slope)
    return z if mask is None else z * act_grad_from_out(mask.to(dtype), mask_act, slope)


def conv_img_wgrad(dz, img, k, s, p, dtype=torch.float64, mutant=None):
    """slab[b][n][ci][kh][kw] = sum_{oy,ox} dz[b][oy][ox][n] * img[b][ci][oy*s - p + kh][ox*s - p + kw] per image.  Mutant ``swap_khkw``"""
    P = patches(img.to(dtype), k, s, p)
    if mutant == "swap_khkw":
        P = P.transpose(4, 5)
    return torch.einsum("bhwn,bhwcij->bncij", dz.to(dtype), P)


def im2col(img, k, s, p, Kp, mutant=None):
    """patch rows [B*OH*OW][Kp], column t = (ci*k + kh)*k + kw, zero from CI*k*k on.  Mutant ``swap_khkw``"""
    P = patches(img, k, s, p)
    if mutant == "swap_khkw":
        P = P.transpose(4, 5)
    rows = P.reshape(-1, img.shape[1] * k * k)
    return F.pad(rows, (0, Kp - rows.shape[1]))


def col2im(cols, B, C, Hin, Win, k, s, p, bias, act_name, dtype=torch.float64, mutant=None):
    """out[b][c][oy][ox] = act(bias[c] + sum of cols[(b,iy,ix)][t*C + c] over the taps t = kh*k + kw with oy = iy*s - p + kh,
    ox = ix*s - p + kw).  Mutant ``tap_parity``: every tap lands where its neighbour of the other parity belongs (kh ^ 1, kw ^ 1)"""
    cols = cols.to(dtype).reshape(B, Hin, Win, k * k, C)
    canvas = torch.zeros(B, C, (Hin - 1) * s + k + 1, (Win - 1) * s + k + 1, dtype=dtype)
    for kh in range(k):
        for kw in range(k):
            a, b = (kh ^ 1, kw ^ 1) if mutant == "tap_parity" else (kh, kw)
            canvas[:, :, a:a + (Hin - 1) * s + 1:s, b:b + (Win - 1) * s + 1:s] += cols[:, :, :, kh * k + kw, :].permute(0, 3, 1, 2)
    OH, OW = (Hin - 1) * s - 2 * p + k, (Win - 1) * s - 2 * p + k
    out = canvas[:, :, p:p + OH, p:p + OW]
    if bias is not None:
        out = out + bias.to(dtype)[None, :, None, None]
    return act(out, act_name)


CONV_IMG_SIGMA = 4.0


def conv_img_epilogue(c, name):
    """keyword arguments of ``conv_img`` for an epilogue of the table"""
    if name == "bias_sigma_lrelu":
        return dict(bias=c["bias"], sigma=c["sigma"], act_name="lrelu")
    if name == "mask":
        return dict(mask=c["mask"], mask_act="lrelu")
    return {}


@functools.lru_cache(maxsize=None)
def conv_img_case(case, dtype):
    """img and the master weight stay fp32 (the kernel computes in fp32 from both); the mask holds values of the output dtype.  One
    yardstick per epilogue (fp32 operands: no variant is exact).  sigma = 4 and a bias of unit scale, so that a bias divided by sigma too
    stands out of a 16-bit output's rounding"""
    B, CI, H, W, N, k, s, p = case
    OH, OW = conv_out(H, W, k, s, p)
    g = _gen(*case, DTYPES.index(dtype))
    c = dict(img=torch.randn(B, CI, H, W, generator=g), w=0.2 * torch.randn(N, CI, k, k, generator=g), bias=torch.randn(N, generator=g),
             sigma=torch.tensor([CONV_IMG_SIGMA]), mask=rq(torch.randn(B, OH, OW, N, generator=g), dtype), want={}, yard={})
    for name in CONV_IMG_EPILOGUES:
        kw = conv_img_epilogue(c, name)
        c["want"][name] = conv_img(c["img"], c["w"], s, p, **kw)
        c["yard"][name] = dist(stored(conv_img(c["img"], c["w"], s, p, dtype=torch.float32, **kw), dtype), c["want"][name])
    return c


@functools.lru_cache(maxsize=None)
def conv_wgrad_case(case, dtype):
    CI, H, W, N, k, s, p = case
    B = CONV_WGRAD_B
    OH, OW = conv_out(H, W, k, s, p)
    g = _gen(*case, DTYPES.index(dtype), 5)
    c = dict(img=torch.randn(B, CI, H, W, generator=g), dz=rq(torch.randn(B, OH, OW, N, generator=g), dtype))
    c["want"] = conv_img_wgrad(c["dz"], c["img"], k, s, p)
    # per image: each slab against its own largest magnitude
    c["yard"] = worst(conv_img_wgrad(c["dz"], c["img"], k, s, p, dtype=torch.float32), c["want"])
    return c


@functools.lru_cache(maxsize=None)
def col2im_case(case, dtype):
    C, B, Hin, Win, k, s, p = case
    g = _gen(*case, DTYPES.index(dtype), 11)
    c = dict(cols=rq(torch.randn(B * Hin * Win, k * k * C, generator=g), dtype), bias=0.3 * torch.randn(C, generator=g), want={}, yard={})
    for a in COL2IM_ACTS:
        args = (c["cols"], B, C, Hin, Win, k, s, p, c["bias"], a)
        c["want"][a] = col2im(*args)
        c["yard"][a] = dist(col2im(*args, dtype=torch.float32), c["want"][a])
    return c


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------
def act_grad_bias(g, a, act_name, gb0, accumulate, dtype=torch.float64, mutant=None):
    """out = g * act'(a) on [B][C][HW], gb[c] (+)= sum_{b,hw} out -> (out, gb).  Mutant ``grad_of_input``: a taken for the activation's
    input instead of its output"""
    g, a = g.to(dtype), a.to(dtype)
    out = g * act_grad_from_out(act(a, act_name) if mutant == "grad_of_input" else a, act_name)
    s = out.sum((0, 2))
    return out, (gb0.to(dtype) + s if accumulate else s)


def flat_reduce(slab, g0, accumulate, dtype=torch.float64, mutant=None):
    """out[i] (+)= sum_z slab[z][i].  Mutant ``last_slab``: the last slab is left out"""
    s = (slab[:-1] if mutant == "last_slab" else slab).to(dtype).sum(0)
    return g0.to(dtype) + s if accumulate else s


def cast_pad(src, npad, dtype_name, mutant=None):
    """dst[r][0:n] = src[r][0:n] in the dtype, dst[r][n:npad] = 0.  Mutant ``padded_stride``: src read with the row stride npad"""
    rows, n = src.shape
    if mutant == "padded_stride":
        src = F.pad(src.flatten(), (0, rows * npad))[:rows * npad].view(rows, npad)[:, :n]
    return rq(F.pad(src, (0, npad - n)), dtype_name)


def wgrad_c1(x, dy, dtype_name, dtype=torch.float64, mutant=None):
    """per work unit (8 image rows of one image) slab[u][t][c] = sum over the unit's input pixels (iy, ix) of
    x[b][iy][ix][c] * dyT[b][iy - ty + 1][ix - tx + 1], t = ty*3 + tx, dyT = dy rounded through the compute dtype (zero outside the image).
    Mutant ``flip_taps``: taps mirrored (ty -> 2 - ty, tx -> 2 - tx)"""
    B, H, W, C = x.shape
    x = x.to(dtype)
    P = F.pad(rq(dy, dtype_name).to(dtype), (1, 1, 1, 1))
    out = torch.zeros(B * (H // 8), 9, C, dtype=dtype)
    for ty in range(3):
        for tx in range(3):
            a, b = (2 - ty, 2 - tx) if mutant == "flip_taps" else (ty, tx)
            out[:, ty * 3 + tx] = (x * P[:, 2 - a:2 - a + H, 2 - b:2 - b + W, None]).reshape(B * (H // 8), 8 * W, C).sum(1)
    return out


@functools.lru_cache(maxsize=None)
def act_grad_case(case, act_name):
    B, C, HW = case
    g = _gen(B, C, HW, ACT_GRAD_ACTS.index(act_name), 13)
    a = torch.randn(B, C, HW, generator=g)
    c = dict(g=torch.randn(B, C, HW, generator=g), a=act(a, act_name) if act_name in ("tanh", "sigmoid") else a,
             gb0=torch.randn(C, generator=g), want={}, yard={})
    for acc in (0, 1):
        c["want"][acc] = act_grad_bias(c["g"], c["a"], act_name, c["gb0"], acc)
        c["yard"][acc] = each(act_grad_bias(c["g"], c["a"], act_name, c["gb0"], acc, dtype=torch.float32), c["want"][acc])      # (out, gb)
    return c


@functools.lru_cache(maxsize=None)
def flat_reduce_case(case):
    nslab, total = case
    g = _gen(nslab, total, 37)
    c = dict(slab=torch.randn(nslab, total, generator=g), g0=torch.randn(total, generator=g), want={}, yard={})
    for acc in (0, 1):
        c["want"][acc] = flat_reduce(c["slab"], c["g0"], acc)
        c["yard"][acc] = dist(flat_reduce(c["slab"], c["g0"], acc, dtype=torch.float32), c["want"][acc])
    return c


def cast_pad_src(case):
    rows, n, _ = case
    return torch.randn(rows, n, generator=_gen(rows, n, 19))


@functools.lru_cache(maxsize=None)
def wgrad_c1_case(case, dtype):
    B, H, W = case
    g = _gen(B, H, W, DTYPES.index(dtype), 23)
    c = dict(x=rq(torch.randn(B, H, W, 64, generator=g), dtype), dy=torch.randn(B, H, W, generator=g))
    c["want"] = wgrad_c1(c["x"], c["dy"], dtype)
    c["yard"] = dist(wgrad_c1(c["x"], c["dy"], dtype, dtype=torch.float32), c["want"])
    return c


def wgrad_c1_ok(H, W):
    """eg_wgrad_c1_ok for 64 -> 1 channels, 3 x 3 / stride 1 / pad 1"""
    return H >= 8 and H % 8 == 0 and W >= 8 and W % 8 == 0 and W <= 128


def im2col_img(case):
    B, CI, H, W = case[:4]
    return torch.randn(B, CI, H, W, generator=_gen(*case, 29))

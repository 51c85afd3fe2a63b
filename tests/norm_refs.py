"""float64 restatements for the BatchNorm tests (tests/test_norm_refs_host.py, tests/test_gpu_norm.py), written for that purpose from the
formulas of include/eadgan_hip.h and the comments of csrc/norm.hip -- no code of the package is used:

* ``stats`` (count, mean, M2 per channel), ``block_triples`` / ``chan`` (the per-row-block or per-rank triples and their combination),
  ``fwd_train``, ``fwd_eval``, ``fwd_from_stats``;
* ``bwd`` (dz, the two sums, dgamma / dbeta stored or accumulated, the activation mask decided on y), ``bwd_post``, ``bwd_sums_local``,
  ``bwd_from_sums``, ``bwd_eval``;
* ``block_moments`` / ``block_sums``: the [2][C][nrb] tables the fused finalisers read, and ``fused_stats`` / ``fused_sums`` on them;
* the launch arithmetic of the launchers as pure functions (``gx_of``, ``rpb_of``, ``nrb_of``, ``apply_blocks_of``, ``ws_floats_of``);
* the case table of the two tests and the cached operands they share.

Every restatement takes ``dtype=`` (float64, or float32 for the yardstick) and ``mutant=`` (a plausible kernel mistake).  Operands are
pre-rounded to the compute dtype and kept as float32 tensors that hold values of that dtype; save_mean / save_invstd enter the backwards
as the float32 roundings of their float64 values.  Every output has a yardstick of its own, in the dtype the kernel stores it in.

The float32 yardstick of y and dz is the documented two-coefficient form (y = x * A + B, dz = A * dy - Bz * z - Cc) with the coefficients
formed in float32 from float64-exact statistics rounded to float32: that form is the contract (the backwards decide act'(y) on that very
y) and it loses digits that (x - mean) * invstd would keep -- at an offset of 100 sigma a yardstick of the other form would fail a correct
kernel.  The yardstick of the statistics is the float32 mean and the float32 two-pass variance on the CPU, computed in float32 arithmetic
(``stats``), and never less than the unit roundoff of float32 (``yard32``)."""
import functools
import math

import torch

from input_grad_refs import EXCLUDE_CAP, K, MUTANT_FACTOR, TORCH_DTYPE, Y_EXCLUDE, dist           # noqa: F401  (the tests read them from here)

DTYPES = ("f32", "bf16", "f16")
VEC = {"f32": 4, "bf16": 8, "f16": 8}              # elements of a 16-byte vector
ACTS = {"none": 0, "lrelu": 1, "relu": 2}          # EG_ACT_* codes the family accepts
ACT_CODES = (0, 1, 2, 3, 4)                         # every EG_ACT_* code (post_act of eg_bn_bwd_post)
SLOPE = 0.2
EPS = 1e-5
MOMENTUM = 0.1
NBT0 = 41                                           # num_batches_tracked starts here
POST_SIGMA = 1.7
BN_RPB = 256
WIDE_NRB = 1024                                     # row blocks from which the fused finalisers take a workgroup per channel
U32 = 2.0 ** -24                                    # unit roundoff of float32


def f32(v):
    """a Python float as the ABI passes it (float)"""
    return float(torch.tensor(v, dtype=torch.float32))


def rq(x, dtype):
    """``x`` rounded to the dtype, as float32"""
    return x.to(TORCH_DTYPE[dtype]).float()


def stored(x, dtype):
    """a float32 result as the kernel stores it in ``dtype``"""
    return x.float().to(TORCH_DTYPE[dtype]).float()


def cdiv(a, b):
    return (a + b - 1) // b


def yard32(got32, want):
    """the yardstick of an output stored in float32: what the float32 restatement misses float64 by, but not less than the unit roundoff
    of float32.  Less is luck or exactness (the float32 mean of 16 or 64 operands of 8 or 11 bits is exact; at M = 1 the mean is the
    operand) and says nothing about a correct kernel that adds in another order and rounds once where the restatement rounds never"""
    return max(dist(got32, want), U32)


# ---- launch arithmetic (the launchers' formulas, restated) -----------------------------------------------------------------------------
def cpr_of(C, dtype):
    """16-byte chunks per row"""
    return C // VEC[dtype]


def gx_of(C, dtype):
    """column blocks of the partial kernels: 256 chunk columns each"""
    cpr = cpr_of(C, dtype)
    return cdiv(cpr, min(cpr, 256))


def rpb_of(M, gx):
    """rows per workgroup of the partial kernels: 256, halved (down to 16) until the launch has >= 512 workgroups"""
    rpb = BN_RPB
    while rpb > 16 and gx * cdiv(M, rpb) < 512:
        rpb //= 2
    return rpb


def nrb_of(M, C, dtype):
    return cdiv(M, rpb_of(M, gx_of(C, dtype)))


def lanes_of(C, dtype):
    """row lanes of a partial workgroup"""
    return 256 // min(cpr_of(C, dtype), 256)


def apply_blocks_of(nrows, cpr):
    """workgroups of the apply kernels: one thread per chunk, capped at 2048, rounded up so that the thread count is a multiple of cpr"""
    want = min(cdiv(nrows * cpr, 256), 2048)
    mult = cpr // math.gcd(cpr, 256)
    return cdiv(want, mult) * mult


def ws_floats_of(M, C):
    """eg_bn_ws_floats: room for max(ceil(M / 256), 1024) row blocks of 3*C floats and the 5*C coefficients"""
    return max(cdiv(M, BN_RPB), 1024) * 3 * C + 5 * C


# ---- case table ------------------------------------------------------------------------------------------------------------------------
# name -> (M, C in f32 (twice that in the 16-bit dtypes: the same chunks per row), offset of x, dtypes)
CASES = {
    "m1": (1, 4, 0.5, DTYPES),                      # one row, cpr = 1 (256 row lanes, one column); var = 0, unbiased = biased
    "m15": (15, 12, 0.5, DTYPES),                   # cpr = 3: 85 lanes and one idle thread, apply grid a multiple of 3; one ragged block
    "m16": (16, 12, 0.5, DTYPES),                   # one full block
    "m17": (17, 12, 0.5, DTYPES),                   # a second block of 1 row
    "nrb65": (1025, 24, 0.5, DTYPES),               # the finaliser's lane loop takes a second round
    "cpr256": (33, 1024, 0.5, DTYPES),              # one row lane
    "cpr257": (33, 1028, 0.5, DTYPES),              # gx = 2, the second column block has one live chunk
    "nrb1022": (16352, 8, 0.5, DTYPES),             # rpb = 16: the largest partial table under the 1024 bound
    "capped": (16353, 132, 0.5, DTYPES),            # rpb = 32 with a 1-row last block; apply grid capped, threads take two rows
    "rpb256": (130817, 8, 0.5, ("f32", "bf16")),    # rpb = 256, 1-row last block
    "offset": (1025, 24, 200.0, ("f32",)),          # 100 sigma off zero: forward only
}
# what the issue quotes: name -> (cpr, gx, rpb, nrb, rows of the last block, apply workgroups)
LAUNCH = {"m1": (1, 1, 16, 1, 1, 1), "m15": (3, 1, 16, 1, 15, 3), "m16": (3, 1, 16, 1, 16, 3), "m17": (3, 1, 16, 2, 1, 3),
          "nrb65": (6, 1, 16, 65, 1, 27), "cpr256": (256, 1, 16, 3, 1, 33), "cpr257": (257, 2, 16, 3, 1, 257),
          "nrb1022": (2, 1, 16, 1022, 16, 128), "capped": (33, 1, 32, 512, 1, 2079), "rpb256": (2, 1, 256, 512, 1, 1023),
          "offset": (6, 1, 16, 65, 1, 27)}
BWD_CASES = tuple(n for n in CASES if n != "offset")
EVAL_BWD_CASES = ("m15", "m16", "m17", "capped")     # cpr = 3 and cpr = 33
FUSED_NRB = (1, 63, 64, 65, 1023, 1024, 1025)
FUSED_RPB = 2
FUSED_CASES = tuple((nrb, 8, dt) for nrb in FUSED_NRB for dt in DTYPES) + ((1024, 12, "f32"),)
DP_SHARDS = {1: (64,), 3: (1, 17, 46), 65: tuple(1 + (i * 7) % 3 for i in range(65))}
DP_C = 12
# seeds moved on where the first one leaves more than EXCLUDE_CAP of a case with |y| < Y_EXCLUDE (in the small cases: a single element)
SEED_BUMP = {"m16": 1, 3: 1}


def dims(name, dtype):
    M, C, _, _ = CASES[name]
    return M, C * (1 if dtype == "f32" else 2)


def launch_of(name, dtype):
    """the LAUNCH row of a case, re-derived"""
    M, C = dims(name, dtype)
    cpr, gx = cpr_of(C, dtype), gx_of(C, dtype)
    rpb = rpb_of(M, gx)
    nrb = cdiv(M, rpb)
    return cpr, gx, rpb, nrb, M - (nrb - 1) * rpb, apply_blocks_of(M, cpr)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def make_case(M, C, dtype, offset=0.5, seed=0):
    """operands: x = randn * 2 + offset, gamma ~ N(1, 0.2), beta ~ N(0, 0.2), da = randn, rounded to the dtype where the kernel reads them in
    it; running statistics and parameter gradients start at random values (a lost (1 - momentum) or a store for an add shows)"""
    g = _gen(M, C, DTYPES.index(dtype), seed)
    return dict(M=M, C=C, dtype=dtype, x=rq(torch.randn(M, C, generator=g) * 2 + offset, dtype), da=rq(torch.randn(M, C, generator=g), dtype),
                gamma=1 + 0.2 * torch.randn(C, generator=g), beta=0.2 * torch.randn(C, generator=g),
                rm0=torch.randn(C, generator=g), rv0=0.5 + torch.rand(C, generator=g), dgamma0=torch.randn(C, generator=g),
                dbeta0=torch.randn(C, generator=g), eps=f32(EPS), momentum=f32(MOMENTUM), nbt0=NBT0, sigma=torch.tensor([POST_SIGMA]))


@functools.lru_cache(maxsize=4)
def bn_case(name, dtype):
    M, C = dims(name, dtype)
    c = make_case(M, C, dtype, CASES[name][2], seed=list(CASES).index(name) + 131 * SEED_BUMP.get(name, 0))
    c["name"] = name
    return c


# ---- activations ---------------------------------------------------------------------------------------------------------------------------
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
    """act'(z) expressed through the output a = act(z); for none / relu / lrelu also act' decided on the pre-activation value"""
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


def keep_of(y64, name):
    """elements whose act' does not hang on rounding (all of them without an activation)"""
    return torch.ones_like(y64, dtype=torch.bool) if name == "none" else y64.abs() >= Y_EXCLUDE


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------
BLOCK_MUTANTS = ("ragged_full", "ragged_drop_row", "first64")


def block_triples(x, rpb, dtype=torch.float64, mutant=None):
    """[nrb][3][C]: (count, mean, M2) of each block of ``rpb`` rows in the partial kernel's pivot form.  Mutants: ``ragged_full`` (a ragged
    last block counted as ``rpb`` rows), ``ragged_drop_row`` (the last row of a ragged block missed by the sums)"""
    out = []
    for r0 in range(0, x.shape[0], rpb):
        blk = x[r0:r0 + rpb].to(dtype)
        n = blk.shape[0]
        cnt = rpb if (mutant == "ragged_full" and n < rpb) else n
        used = blk[:-1] if (mutant == "ragged_drop_row" and n < rpb) else blk
        d = used - blk[0]
        ts, tq = d.sum(0), (d * d).sum(0)
        out.append(torch.stack((torch.full_like(ts, cnt), blk[0] + ts / cnt, (tq - ts * ts / cnt).clamp_min(0))))
    return torch.stack(out)


def chan(triples, dtype=torch.float64, mutant=None):
    """Chan's combination of [n][3][C] triples in closed form: n = sum n_b, mean = sum n_b mean_b / n,
    M2 = sum M2_b + sum n_b (mean_b - mean)^2.  Mutant ``first64``: only the first 64 triples (one round of the lane loop) are combined"""
    t = (triples[:64] if mutant == "first64" else triples).to(dtype)
    n = t[:, 0].sum(0)
    mean = (t[:, 0] * t[:, 1]).sum(0) / n
    return n, mean, t[:, 2].sum(0) + (t[:, 0] * (t[:, 1] - mean) ** 2).sum(0)


def stats(x, dtype=torch.float64, mutant=None, rpb=16):
    """(count, mean, M2) per channel of the rows of x (eg_bn_stats_local).  Mutants: those of ``block_triples`` and ``chan`` with row blocks of
    ``rpb`` rows; ``sumsq_f32``: the variance as E[x^2] - E[x]^2 in float32"""
    M = x.shape[0]
    if mutant == "sumsq_f32":
        x32 = x.float()
        mean = x32.mean(0)
        return torch.full_like(mean, M).to(dtype), mean.to(dtype), (((x32 * x32).mean(0) - mean * mean).clamp_min(0) * M).to(dtype)
    if mutant in BLOCK_MUTANTS:
        return chan(block_triples(x, rpb, dtype, mutant), dtype, mutant)
    xd = x.to(dtype)
    mean = xd.mean(0)
    # two passes in ``dtype`` itself: torch.var on a float32 CPU tensor accumulates in double and rounds once at the end, which is no
    # float32 computation (its error is the final rounding alone, whatever M is) and would be no yardstick for one
    return torch.full_like(mean, M), mean, ((xd - mean) ** 2).sum(0)


def finalise(mean, m2, M, c, dtype=torch.float64, mutant=None):
    """save_mean, save_invstd, the running statistics (unbiased variance: M2 / (M - 1), M2 / M for M = 1) and num_batches_tracked.
    Mutant ``biased_running_var``"""
    var = m2 / M
    unb = m2 / (M - 1) if (M > 1 and mutant != "biased_running_var") else var
    mom = torch.tensor(c["momentum"], dtype=dtype)
    return dict(save_mean=mean, save_invstd=1.0 / torch.sqrt(var + torch.tensor(c["eps"], dtype=dtype)),
                running_mean=(1 - mom) * c["rm0"].to(dtype) + mom * mean, running_var=(1 - mom) * c["rv0"].to(dtype) + mom * unb,
                nbt=c["nbt0"] + 1)


def coef_apply(x, mean, istd, gamma, beta, name):
    """y of the two-coefficient form in float32: A = gamma * invstd, B = beta - mean * gamma * invstd, y = act(x * A + B)"""
    mean, istd, gamma, beta = mean.float(), istd.float(), gamma.float(), beta.float()
    return act(x.float() * (gamma * istd) + (beta - mean * gamma * istd), name)


def normalise(x, mean, istd, gamma, beta, name, dtype=torch.float64):
    """y = act((x - mean) * invstd * gamma + beta) in float64; the two-coefficient form for float32"""
    if dtype == torch.float32:
        return coef_apply(x, mean, istd, gamma, beta, name)
    t = lambda v: v.to(dtype)
    return act((t(x) - t(mean)) * t(istd) * t(gamma) + t(beta), name)


def fwd_train(c, name="none", dtype=torch.float64, mutant=None, rpb=16, x=None, M_stat=None, st=None):
    """eg_bn_fwd_train on the operands of ``c`` -> dict(y, save_mean, save_invstd, running_mean, running_var, nbt).  ``st(dtype)``: the
    statistics (count, mean, M2) from elsewhere (the fused form: from the table).  float32: the statistics as float32 mean / var give
    them, y in the two-coefficient form from the float64 statistics rounded to float32"""
    x = c["x"] if x is None else x
    M = x.shape[0] if M_stat is None else M_stat
    _, mean, m2 = stats(x, dtype, mutant, rpb) if st is None else st(dtype)
    out = finalise(mean.to(dtype), m2.to(dtype), M, c, dtype, mutant)
    if dtype == torch.float32:
        _, mean64, m264 = stats(x) if st is None else st(torch.float64)
        e = finalise(mean64, m264, M, c)
        out["y"] = coef_apply(x, e["save_mean"], e["save_invstd"], c["gamma"], c["beta"], name)
    else:
        out["y"] = normalise(x, out["save_mean"], out["save_invstd"], c["gamma"], c["beta"], name, dtype)
    return out


def fwd_eval(c, name="none", dtype=torch.float64, mutant=None):
    """y = act((x - running_mean) / sqrt(running_var + eps) * gamma + beta).  Mutant ``raw_var``: the variance used without eps and root"""
    t = lambda v: v.to(dtype)
    rv = t(c["rv0"])
    istd = 1.0 / rv if mutant == "raw_var" else 1.0 / torch.sqrt(rv + torch.tensor(c["eps"], dtype=dtype))
    if dtype == torch.float32:
        a = c["gamma"] * istd
        return act(c["x"] * a + (c["beta"] - c["rm0"] * a), name)
    return normalise(c["x"], c["rm0"], istd, c["gamma"], c["beta"], name, dtype)


def fwd_from_stats(c, x_local, triples, M_global, name="none", dtype=torch.float64, mutant=None):
    """eg_bn_fwd_from_stats: Chan's combination of the per-rank triples [nranks][3][C], then the local rows normalised with the statistics
    of the M_global rows.  Mutants: ``m_local`` (the local row count where the global one belongs), ``first64`` (of ``chan``)"""
    st = chan(triples, torch.float64 if dtype == torch.float32 else dtype, mutant)
    M = x_local.shape[0] if mutant == "m_local" else M_global
    if dtype == torch.float32:
        n, mean, m2 = chan(triples.float(), torch.float32)
        out = finalise(mean, m2, M, c, dtype)
        e = finalise(st[1], st[2], M, c)
        out["y"] = coef_apply(x_local, e["save_mean"], e["save_invstd"], c["gamma"], c["beta"], name)
        return out
    out = finalise(st[1], st[2], M, c, dtype)
    out["y"] = normalise(x_local, out["save_mean"], out["save_invstd"], c["gamma"], c["beta"], name, dtype)
    return out


def saved(c, x=None):
    """save_mean and save_invstd of the case as the backwards read them: the float64 values rounded to float32"""
    _, mean, m2 = stats(c["x"] if x is None else x)
    e = finalise(mean, m2, (c["x"] if x is None else x).shape[0], c)
    return e["save_mean"].float(), e["save_invstd"].float()


# ---- backward ------------------------------------------------------------------------------------------------------------------------------
def bwd_dy(c, z, da, mean, istd, name, dtype=torch.float64, mutant=None):
    """(dy, xhat, y): dy = da * act'(y) with y = xhat * gamma + beta.  Mutant ``mask_on_z``: act' decided on z.  float32: y as the apply kernel
    forms it, z * P + Q with P = gamma * invstd, Q = beta - mean * gamma * invstd"""
    t = lambda v: v.to(dtype)
    xhat = (t(z) - t(mean)) * t(istd)
    if dtype == torch.float32:
        y = coef_apply(z, mean, istd, c["gamma"], c["beta"], "none")
    else:
        y = xhat * t(c["gamma"]) + t(c["beta"])
    return t(da) * act_grad_from_out(t(z) if mutant == "mask_on_z" else y, name), xhat, y


def dz_of(c, z, dy, xhat, s1, s2, M, mean, istd, dtype=torch.float64, mutant=None):
    """dz = gamma * invstd * (dy - sum(dy) / M - xhat * sum(dy * xhat) / M); float32: A * dy - Bz * z - Cc with the coefficients in float32.
    Mutant ``drop_mean_term``: without sum(dy) / M"""
    t = lambda v: v.to(dtype)
    g, i = t(c["gamma"]), t(istd)
    if mutant == "drop_mean_term":
        s1 = torch.zeros_like(s1)
    if dtype == torch.float32:
        s1, s2, mu, invM = s1.float(), s2.float(), mean.float(), torch.tensor(1.0 / M, dtype=torch.float32)
        return (g * i) * dy - (g * i * i * s2 * invM) * z.float() - g * i * (s1 * invM - mu * i * s2 * invM)
    return g * i * (dy - t(s1) / M - xhat * t(s2) / M)


def bwd(c, name="none", accumulate=1, dtype=torch.float64, mutant=None, z=None, da=None, M_div=None, sums=None, mean=None, istd=None):
    """eg_bn_bwd -> dict(dz, s1, s2, dgamma, dbeta, y).  ``da``: the gradient actually passed (the GPU test zeroes it where |y| is below
    Y_EXCLUDE).  ``sums`` = (s1, s2) from outside and ``M_div`` (the divisor): the data-parallel stage 2.  float32: the sums as float32
    adds them; dz in the two-coefficient form from the float64 sums rounded to float32.  Mutants: ``drop_mean_term``, ``mask_on_z``,
    ``store_dgamma`` (dgamma / dbeta stored where they must accumulate)"""
    z = c["x"] if z is None else z
    da = c["da"] if da is None else da
    if mean is None:
        mean, istd = saved(c, z)
    M = z.shape[0] if M_div is None else M_div
    dy, xhat, y = bwd_dy(c, z, da, mean, istd, name, dtype, mutant)
    loc1, loc2 = dy.sum(0), (dy * xhat).sum(0)
    if dtype == torch.float32:
        if sums is None:
            dy64, xh64, _ = bwd_dy(c, z, da, mean, istd, name)
            ex1, ex2 = dy64.sum(0), (dy64 * xh64).sum(0)
        else:
            ex1, ex2 = sums
        dz = dz_of(c, z, dy, xhat, ex1, ex2, M, mean, istd, dtype, mutant)
    else:
        s1, s2 = (loc1, loc2) if sums is None else sums
        dz = dz_of(c, z, dy, xhat, s1, s2, M, mean, istd, dtype, mutant)
    acc = accumulate and mutant != "store_dgamma"
    return dict(dz=dz, s1=loc1, s2=loc2, y=y, dgamma=c["dgamma0"].to(dtype) + loc2 if acc else loc2,
                dbeta=c["dbeta0"].to(dtype) + loc1 if acc else loc1)


def bwd_post(c, post_name="lrelu", sigma=True, dtype=torch.float64, mutant=None):
    """eg_bn_bwd_post: eg_bn_bwd without an activation, dz times act'(z as an activation OUTPUT) / post_sigma; dgamma / dbeta always
    accumulate.  Mutant ``mul_sigma``: multiplied by post_sigma"""
    out = bwd(c, "none", 1, dtype)
    f = act_grad_from_out(c["x"].to(dtype), post_name)
    if sigma:
        s = c["sigma"].to(dtype)
        f = f * s if mutant == "mul_sigma" else f / s
    out["dz"] = out["dz"] * f
    return out


def bwd_sums_local(c, z, da, mean, istd, name="none", accumulate=1, dtype=torch.float64, mutant=None):
    """eg_bn_bwd_sums_local on the rows (z, da) of one rank -> (s1, s2, dgamma, dbeta)"""
    o = bwd(c, name, accumulate, dtype, mutant, z=z, da=da, mean=mean, istd=istd)
    return o["s1"], o["s2"], o["dgamma"], o["dbeta"]


def bwd_from_sums(c, z, da, sums, M_global, mean, istd, name="none", dtype=torch.float64, mutant=None):
    """eg_bn_bwd_from_sums: dz of the local rows from the global sums and the global row count.  Mutant ``m_local``"""
    M = z.shape[0] if mutant == "m_local" else M_global
    return bwd(c, name, 1, dtype, None, z=z, da=da, M_div=M, sums=sums, mean=mean, istd=istd)["dz"]


def bwd_eval(c, name="none", dtype=torch.float64):
    """eg_bn_bwd_eval: dz = da * act'(y) * gamma / sqrt(running_var + eps), y of ``fwd_eval`` before the activation -> (dz, y)"""
    y = fwd_eval(c, "none", dtype)
    t = lambda v: v.to(dtype)
    a = t(c["gamma"]) / torch.sqrt(t(c["rv0"]) + torch.tensor(c["eps"], dtype=dtype))
    return t(c["da"]) * act_grad_from_out(y, name) * a, y


# ---- the tables of the fused finalisers ---------------------------------------------------------------------------------------------------
def block_moments(x, nrb, dtype=torch.float64):
    """[2][C][nrb]: (mean_b, M2_b) of nrb row blocks of M / nrb rows each, what eg_bn_fwd_train_fused reads (EG_STAT_MOMENTS)"""
    M, C = x.shape
    b = x.to(dtype).reshape(nrb, M // nrb, C)
    mean = b.mean(1)
    return torch.stack((mean.t(), ((b - mean[:, None]) ** 2).sum(1).t())).contiguous()


def block_sums(dy, xhat, nrb, dtype=torch.float64):
    """[2][C][nrb]: (sum dy, sum dy * xhat) per row block, what eg_bn_bwd_fused reads (EG_STAT_BN_BWD)"""
    M, C = dy.shape
    d, h = dy.to(dtype).reshape(nrb, M // nrb, C), xhat.to(dtype).reshape(nrb, M // nrb, C)
    return torch.stack((d.sum(1).t(), (d * h).sum(1).t())).contiguous()


def fused_stats(stat, cnt, dtype=torch.float64, mutant=None):
    """(count, mean, M2) from a [2][C][nrb] table of blocks of ``cnt`` rows each.  Mutant ``first64``"""
    s = (stat[:, :, :64] if mutant == "first64" else stat).to(dtype)
    mean = s[0].mean(1)
    return torch.full_like(mean, cnt * s.shape[2]), mean, s[1].sum(1) + cnt * ((s[0] - mean[:, None]) ** 2).sum(1)


def fused_sums(stat, dtype=torch.float64, mutant=None):
    """(s1, s2) from a [2][C][nrb] table.  Mutant ``first64``"""
    s = (stat[:, :, :64] if mutant == "first64" else stat).to(dtype)
    return s[0].sum(1), s[1].sum(1)


@functools.lru_cache(maxsize=4)
def fused_case(nrb, C, dtype):
    """operands of a fused-finaliser case: M = nrb * FUSED_RPB rows, the float32 tables synthesised from float64 (no convolution), and the
    gradient dy (it carries the activation gradient already)"""
    c = make_case(nrb * FUSED_RPB, C, dtype, seed=1000 + nrb)
    c["nrb"] = nrb
    c["stat_fwd"] = block_moments(c["x"], nrb).float()
    c["st"] = fused_stats(c["stat_fwd"], FUSED_RPB)                              # statistics of the ROUNDED table: the kernel's operands
    e = finalise(c["st"][1], c["st"][2], c["M"], c)
    c["mean"], c["istd"] = e["save_mean"].float(), e["save_invstd"].float()
    xhat = (c["x"].double() - c["mean"].double()) * c["istd"].double()
    c["stat_bwd"] = block_sums(c["da"], xhat, nrb).float()
    return c


def dp_case(nranks, dtype):
    """the data-parallel case: one batch cut into the shards of DP_SHARDS -> (case of the whole batch, row ranges)"""
    sizes = DP_SHARDS[nranks]
    c = make_case(sum(sizes), DP_C * (1 if dtype == "f32" else 2), dtype, seed=2000 + nranks + 131 * SEED_BUMP.get(nranks, 0))
    edges = [0]
    for s in sizes:
        edges.append(edges[-1] + s)
    return c, list(zip(edges[:-1], edges[1:]))

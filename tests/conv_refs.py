"""float64 restatements for the convolution tests (tests/test_conv_refs_host.py, tests/test_gpu_conv.py), written for that purpose from
include/eadgan_hip.h and the comments of csrc/ (igemm.hip, igemm_tn.hip, igemm_tn8.hip, pack.hip, conv_geom.h) -- no code of the package is
used:

* ``conv_fwd`` (eg_conv_fwd: nearest-2x ``up``, k, stride, pad, H != W) as ONE product of the gathered rows ``im2col`` with the weights in
  tap-major K order; ``conv_bwd_data`` (eg_conv_bwd_data) as a transposed convolution -- every dY pixel scattered through every tap, not
  phase by phase; ``epilogue`` (v = acc / sigma[tape] + bias[n % bias_mod], act, * act'(mask); tape = lattice_row / sigma_rows; NHWC in the
  compute dtype or NCHW fp32); ``wgrad_slab`` (slab[split][Cout][k*k][Cin], split boundaries from the restated plans); ``panels_fwd`` and
  ``panels_bwd`` (the packed weights, K padded with zeros to Kpad, the backward phases in (ry, rx) order);
* the launch arithmetic as pure functions: ``kpad_of``, ``bwd_axis`` / ``bwd_phases`` (tap counts), ``pack_fwd_elems`` / ``pack_bwd_elems``,
  ``tn_tiles`` / ``tn_plan`` (eg_tn_plan), ``tn8_plan`` (eg_tn8_plan: acceptance and split), ``splitk_bytes`` (the partial tiles of a K split);
* the case tables of the two tests and the cached cases they share.

Every restatement takes ``dtype=`` (float64, or float32 for the yardstick) and ``mutant=`` (a plausible kernel mistake).  Each case has two
operand sets.  ``int``: entries in {-1, 0, 1}, about one in four non-zero, sigma / bias / slopes small powers of two and integers -- every
partial sum and every result is exact in the storage dtype, the yardstick is zero and the GPU must give float64's value bit for bit (tanh
and sigmoid have no exact results: those epilogues run the random set only).  ``rand``: randn rounded to the compute dtype, the weights times
0.1 -- the result may miss float64 by K = 8 times what the float32 restatement misses it by (rounded to the output dtype where the kernel
stores that dtype).

The planner of the NT kernels is not restated (tests/test_nt_plan_host.py pins it); every NT launch of the tables carries the label
eg_igemm_nt_tile_ep must answer for it, and the host test checks the labels without a GPU."""
import collections
import functools

import torch

from input_grad_refs import K, MUTANT_FACTOR, TORCH_DTYPE, dist           # noqa: F401  (the tests read them from here)

DTYPES = ("f32", "bf16", "f16")
VEC = {"f32": 4, "bf16": 8, "f16": 8}
BK = {"f32": 32, "bf16": 64, "f16": 64}
ESIZE = {"f32": 4, "bf16": 2, "f16": 2}
ACTS = ("none", "lrelu", "relu", "tanh", "sigmoid")        # EG_ACT_* codes by position
NT_AUTO, NT_REG, NT_BUF128, NT_PERS, NT_S8, NT_S8P, NT_S8H = range(7)
NT_NAME = {NT_AUTO: "auto", NT_REG: "reg", NT_BUF128: "buf128", NT_PERS: "pers", NT_S8: "s8", NT_S8P: "s8p", NT_S8H: "s8h"}
CNT_BYTES = 4096                                           # the arrival counters at the tail of a split-K scratch
SLOPE = {"int": (0.5, 0.25), "rand": (0.2, 0.2)}           # (act slope, mask slope)
SIGMAS = {"int": (1.0, 0.5, 0.25), "rand": (1.7, 0.6, 2.3)}
INT_BOUND = 256


def rq(x, dtype):
    """``x`` rounded to the dtype, as float32"""
    return x.to(TORCH_DTYPE[dtype]).float()


def stored(x, dtype):
    """a result as the kernel stores it in ``dtype``"""
    return x.float().to(TORCH_DTYPE[dtype]).float()


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(v, m):
    return cdiv(v, m) * m


def ilog2_exact(v):
    return v.bit_length() - 1 if v > 0 and v & (v - 1) == 0 else -1


# ---- geometry and launch arithmetic ------------------------------------------------------------------------------------------------------
def geom(case):
    """(XH, XW, OH, OW): the extents the taps walk (H << up) and the output extents"""
    B, H, W, Cin, Cout, k, s, p, up = case
    XH, XW = H << up, W << up
    return XH, XW, (XH + 2 * p - k) // s + 1, (XW + 2 * p - k) // s + 1


def rows_of(case):
    _, _, OH, OW = geom(case)
    return case[0] * OH * OW


def conv_ok(case, dtype, need_cin=True, need_cout=True):
    """check_conv: what every entry point refuses"""
    B, H, W, Cin, Cout, k, s, p, up = case
    if min(B, k, s, Cin, Cout, H, W) <= 0 or p < 0 or up not in (0, 1):
        return False
    _, _, OH, OW = geom(case)
    if min(ilog2_exact(H), ilog2_exact(W), ilog2_exact(OH), ilog2_exact(OW)) < 0 or B * OH * OW >= 2 ** 31:
        return False
    return (not need_cin or Cin % VEC[dtype] == 0) and (not need_cout or Cout % VEC[dtype] == 0)


def bwd_ok(case, dtype):
    """geom_bwd: stride 1 or 2, k >= stride, OH == (H << up) / stride; the gathered channels (Cout) in whole vectors"""
    B, H, W, Cin, Cout, k, s, p, up = case
    XH, XW, OH, OW = geom(case)
    return (conv_ok(case, dtype, need_cin=False) and s in (1, 2) and k >= s and XH % s == 0 and XW % s == 0 and XH // s == OH
            and XW // s == OW)


def kpad_of(Kd, dtype):
    return round_up(max(Kd, 1), BK[dtype])


def bwd_axis(k, s, p, r):
    """(first kernel index, tap count, source offset of tap 0) of output residue r along one axis; the source steps -1 per tap"""
    k0 = (r + p) % s
    return k0, ((k - k0 + s - 1) // s if k0 < k else 0), (r + p - k0) // s


def bwd_phases(case):
    """[(ry, rx, ay, ax)] in geom_bwd's order"""
    k, s, p = case[5:8]
    return [(ry, rx, bwd_axis(k, s, p, ry), bwd_axis(k, s, p, rx)) for ry in range(s) for rx in range(s)]


def bwd_taps(case):
    return [ay[1] * ax[1] for _, _, ay, ax in bwd_phases(case)]


def pack_fwd_elems(case, dtype):
    B, H, W, Cin, Cout, k, s, p, up = case
    return Cout * kpad_of(k * k * Cin, dtype)


def pack_bwd_elems(case, dtype):
    Cin, Cout = case[3], case[4]
    return sum(Cin * kpad_of(t * Cout, dtype) for t in bwd_taps(case))


def tn_tiles(case):
    Cin, Cout = case[3], case[4]
    t = lambda c: 128 if c >= 128 else (64 if c > 32 else 32)
    return t(Cout), t(Cin)


def tn_plan(case, wgs_target=0):
    """eg_tn_plan: (splits, rows per split -- a multiple of 32) of the per-tap weight-gradient kernel"""
    B, H, W, Cin, Cout, k, s, p, up = case
    M = rows_of(case)
    bnt, bct = tn_tiles(case)
    base = cdiv(Cout, bnt) * cdiv(Cin, bct) * k * k
    want = 1 if base >= 768 else cdiv(768, base)
    want = min(want, max(M // 256, 1), 512 if bnt * bct <= 64 * 64 else 128)
    if wgs_target > 0:
        want = min(wgs_target, max(1, M // 32))
    rps = round_up(cdiv(M, want), 32)
    return cdiv(M, rps), rps


def tn_rows_per_step(case, dtype):
    """64 rows per K step where one output tile is the whole launch (16-bit, BNT + BCT <= 192), else 32"""
    B, H, W, Cin, Cout, k, s, p, up = case
    bnt, bct = tn_tiles(case)
    return 64 if cdiv(Cout, bnt) * cdiv(Cin, bct) * k * k == 1 and dtype != "f32" and bnt + bct <= 192 else 32


def tn8_plan(case, dtype, wgs_target=0):
    """eg_tn8_plan: None where the parity-class kernel does not take the convolution, else dict(ch, nsplit, rps, nimg, OHt)"""
    B, H, W, Cin, Cout, k, s, p, up = case
    if dtype == "f32" or (k, s, p, up) != (4, 2, 1, 0):
        return None
    ch = next((c for c in (128, 64, 32) if Cin % c == 0 and Cout % c == 0), 0)
    if ch == 0 or H & 1 or W & 1:
        return None
    OH, OW = H // 2, W // 2
    M = B * OH * OW
    if ilog2_exact(OH) < 0 or ilog2_exact(OW) < 0 or OW > 64 or M % 64:
        return None
    if B * H * W * Cin * 2 >= 0x7fffffff or M * Cout * 2 >= 0x7fffffff:
        return None
    nimg, OHt = (1, 64 // OW) if OH * OW >= 64 else (64 // (OH * OW), OH)
    npix = nimg * (OHt + 1) * (OW + 1)
    rpp = 1024 // (ch * 2)                                 # patch pixels per DMA piece
    if round_up(npix, rpp) > 136 or cdiv(cdiv(npix, rpp), 8) > 5:
        return None
    base = (Cout // ch) * (Cin // ch) * 4
    target = min(wgs_target, 256) if wgs_target > 0 else 256
    steps = M // 64
    want = min(1 if base >= target else cdiv(target, base), max(1, steps // 4))
    sps = cdiv(steps, want)
    return dict(ch=ch, nsplit=cdiv(steps, sps), rps=sps * 64, nimg=nimg, OHt=OHt)


def wgrad_variant(case, dtype):
    if not conv_ok(case, dtype):
        return -1
    return 2 if tn8_plan(case, dtype) else 1


def wgrad_splits(case, dtype, wgs_target=0):
    """(variant, [(m0, m1)]) of eg_conv_wgrad: the per-tap launches take no target"""
    p8 = tn8_plan(case, dtype, wgs_target)
    ns, rps = (p8["nsplit"], p8["rps"]) if p8 else tn_plan(case, 0)
    M = rows_of(case)
    return (2 if p8 else 1), [(i * rps, min(M, (i + 1) * rps)) for i in range(ns)]


def wgrad_ws_bytes(case, dtype):
    if not conv_ok(case, dtype):
        return 0
    B, H, W, Cin, Cout, k, s, p, up = case
    return len(wgrad_splits(case, dtype, 0)[1]) * Cout * k * k * Cin * 4


def nphase_of(case, bwd):
    return case[6] ** 2 if bwd else 1


def splitk_bytes(case, bwd, bm, ns):
    """bytes of a split-K scratch for ns splits of bm-row tiles: ns partial-tile sets of nphase * cdiv(M, bm) * bm * N fp32 + the counters"""
    N = case[3] if bwd else case[4]
    return ns * nphase_of(case, bwd) * cdiv(rows_of(case), bm) * bm * N * 4 + CNT_BYTES


# ---- activations --------------------------------------------------------------------------------------------------------------------------
def act(v, name, slope):
    if name == "lrelu":
        return torch.where(v > 0, v, v * slope)
    if name == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    if name == "tanh":
        return torch.tanh(v)
    if name == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-v))
    return v


def act_grad_from_out(a, name, slope, mutant=None):
    """act'(z) through the output a = act(z).  Mutant ``mask_wrong_sign``: the slope on the positive side"""
    one = torch.ones_like(a)
    if name in ("lrelu", "relu"):
        neg = one * (slope if name == "lrelu" else 0.0)
        return torch.where(a > 0, neg, one) if mutant == "mask_wrong_sign" else torch.where(a > 0, one, neg)
    if name == "tanh":
        return 1.0 - a * a
    if name == "sigmoid":
        return a * (1.0 - a)
    return one


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------
def swap_hw(x):
    """mutant: the pixel index taken as iy * H + ix (H and W exchanged; the identity on square tensors), kept inside the image"""
    B, H, W = x.shape[:3]
    idx = (torch.arange(H).view(H, 1) * H + torch.arange(W).view(1, W)) % (H * W)
    return x.reshape(B, H * W, -1)[:, idx.flatten()].reshape(x.shape)


def source(x, case, mutant=None):
    """what the taps read: x [B, H, W, C] upsampled by ``up`` inside a zero border of ``pad`` pixels.  Mutants: ``swap_hw``; ``up_last``
    (the last upsampled row and column are lost); ``clamp_border`` (a border tap reads the nearest pixel instead of zero)"""
    B, H, W, Cin, Cout, k, s, p, up = case
    if mutant == "swap_hw":
        x = swap_hw(x)
    if up:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
        if mutant == "up_last":
            x = x.clone()
            x[:, -1] = 0
            x[:, :, -1] = 0
    XH, XW = x.shape[1:3]
    if mutant == "clamp_border":
        iy = (torch.arange(XH + 2 * p) - p).clamp(0, XH - 1)
        ix = (torch.arange(XW + 2 * p) - p).clamp(0, XW - 1)
        return x[:, iy][:, :, ix]
    xp = x.new_zeros(B, XH + 2 * p, XW + 2 * p, x.shape[3])
    xp[:, p:p + XH, p:p + XW] = x
    return xp


def im2col(x, case, mutant=None):
    """A [M][(ty * k + tx) * Cin + c]: the gathered rows in the kernels' tap-major K order.  Mutant ``swap_tap``: ty and tx exchanged"""
    B, H, W, Cin, Cout, k, s, p, up = case
    _, _, OH, OW = geom(case)
    xp = source(x, case, mutant)
    cols = []
    for ty in range(k):
        for tx in range(k):
            a, b = (tx, ty) if mutant == "swap_tap" else (ty, tx)
            cols.append(xp[:, a:a + s * (OH - 1) + 1:s, b:b + s * (OW - 1) + 1:s].reshape(B * OH * OW, -1))
    return torch.cat(cols, 1)


def wmat(w):
    """[Cout][(ty * k + tx) * Cin + c] of the master [Cout][Cin][k][k]"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def conv_fwd(x, w, case, dtype=torch.float64, mutant=None, cdt=None, nsplit=1):
    """acc [M][Cout] of eg_conv_fwd before its epilogue; x [B, H, W, Cin], w [Cout, Cin, k, k].  ``cdt`` (the compute dtype's name) and
    ``nsplit`` place the K tiles and K splits for the mutants ``drop_last_ktile`` and ``round_partial`` (every split's partial tile passed
    through the compute dtype)"""
    A, Wm = im2col(x.to(dtype), case, mutant), wmat(w.to(dtype))
    if mutant == "drop_last_ktile":
        A = A.clone()
        A[:, kpad_of(A.shape[1], cdt) - BK[cdt]:] = 0
    if mutant == "round_partial" and nsplit > 1:
        per = cdiv(kpad_of(A.shape[1], cdt) // BK[cdt], nsplit) * BK[cdt]
        return sum(stored(A[:, i * per:(i + 1) * per] @ Wm[:, i * per:(i + 1) * per].t(), cdt).to(dtype) for i in range(nsplit))
    return A @ Wm.t()


def conv_bwd_data(dy, w, case, dtype=torch.float64, mutant=None):
    """acc [B * XH * XW][Cin] of eg_conv_bwd_data in pixel order: dX[y][x] += dY[oy][ox] W[ky][kx] at y = oy * s - p + ky.  Mutants:
    ``swap_hw`` (of dY's pixel index), ``swap_tap``, ``swap_oo`` (a phase's results stored at the transposed sub-pixel offset)"""
    B, H, W, Cin, Cout, k, s, p, up = case
    XH, XW, OH, OW = geom(case)
    dy, w = dy.to(dtype), w.to(dtype)
    if mutant == "swap_hw":
        dy = swap_hw(dy)
    buf = dy.new_zeros(B, XH + 2 * p + k, XW + 2 * p + k, Cin)
    for ky in range(k):
        for kx in range(k):
            a, b = (kx, ky) if mutant == "swap_tap" else (ky, kx)
            buf[:, ky:ky + s * (OH - 1) + 1:s, kx:kx + s * (OW - 1) + 1:s] += torch.einsum("bhwo,oi->bhwi", dy, w[:, :, a, b])
    dx = buf[:, p:p + XH, p:p + XW]
    if mutant == "swap_oo" and s == 2:
        out = dx.clone()
        for ry in range(2):
            for rx in range(2):
                out[:, rx::2, ry::2] = dx[:, ry::2, rx::2]
        dx = out
    return dx.reshape(B * XH * XW, Cin)


def lattice_rows(case, bwd):
    """the lattice row (b, ly, lx) of every output pixel, in output pixel order: the identity for the forward pass; a backward launch
    walks dY's grid, and output pixel (y, x) belongs to lattice pixel (y / s, x / s)"""
    B, H, W, Cin, Cout, k, s, p, up = case
    XH, XW, OH, OW = geom(case)
    if not bwd:
        return torch.arange(B * OH * OW)
    b = torch.arange(B).view(B, 1, 1)
    y = torch.arange(XH).view(1, XH, 1)
    x = torch.arange(XW).view(1, 1, XW)
    return ((b * OH + y // s) * OW + x // s).flatten()


def epilogue(acc, rows, e, mutant=None):
    """v = acc / sigma[tape] + bias[n % bias_mod]; v = act(v); v *= act'(mask).  ``e``: dict(sigma, sigma_rows, bias, bias_mod, act, slope,
    mask, mask_act, mask_slope) with None / 0 for what is absent; bias has one entry per column whatever bias_mod is.  Mutants:
    ``bias_before_sigma``, ``tape_tile_first`` (the tape of the first row of the 128-row tile), ``ignore_bias_mod``, ``mask_wrong_sign``"""
    dt, N = acc.dtype, acc.shape[1]
    v, sg, bs = acc, None, None
    if e.get("sigma") is not None:
        r = rows // 128 * 128 if mutant == "tape_tile_first" else rows
        tape = r // e["sigma_rows"] if e.get("sigma_rows") else torch.zeros_like(r)
        sg = e["sigma"].to(dt)[tape].unsqueeze(1)
    if e.get("bias") is not None:
        n = torch.arange(N)
        bs = e["bias"].to(dt)[n % e["bias_mod"] if e.get("bias_mod") and mutant != "ignore_bias_mod" else n]
    if mutant == "bias_before_sigma" and sg is not None and bs is not None:
        v = (v + bs) / sg
    else:
        v = v / sg if sg is not None else v
        v = v + bs if bs is not None else v
    v = act(v, e.get("act", "none"), e.get("slope", 0.0))
    if e.get("mask") is not None:
        v = v * act_grad_from_out(e["mask"].to(dt), e["mask_act"], e["mask_slope"], mutant)
    return v


def to_nchw(v, case, bwd):
    """[rows][N] in pixel order -> [B][N][DH][DW] (EG_OUT_NCHW_F32)"""
    XH, XW, OH, OW = geom(case)
    DH, DW = (XH, XW) if bwd else (OH, OW)
    return v.view(case[0], DH, DW, -1).permute(0, 3, 1, 2).contiguous()


def wgrad_slab(x, dy, case, splits, dtype=torch.float64, mutant=None):
    """slab [split][Cout][k*k][Cin]: per split the sum over its lattice rows of dY[m][n] * A[m][t * Cin + c].  Mutants: ``swap_hw``,
    ``swap_tap``, ``clamp_border``, ``up_last`` (of the gather), ``drop_first_row``, ``double_last_row`` (of every split), ``transpose_tc``
    (a split stored [c][t])"""
    B, H, W, Cin, Cout, k, s, p, up = case
    A = im2col(x.to(dtype), case, mutant)
    P = dy.to(dtype).reshape(A.shape[0], Cout)
    out = []
    for a, b in splits:
        Pa, Aa = P[a:b], A[a:b]
        if mutant == "drop_first_row":
            Pa, Aa = Pa[1:], Aa[1:]
        if mutant == "double_last_row":
            Pa, Aa = torch.cat((Pa, Pa[-1:])), torch.cat((Aa, Aa[-1:]))
        S = (Pa.t() @ Aa).view(Cout, k * k, Cin)
        if mutant == "transpose_tc":
            S = S.transpose(1, 2).reshape(Cout, k * k, Cin)
        out.append(S)
    return torch.stack(out)


def panels_fwd(w, case, dtype, mutant=None):
    """[Cout][Kpad] of eg_pack_fwd: the master rounded to ``dtype`` (as float32) in tap-major K order, zeros in [K, Kpad).  Mutant
    ``pad_unwritten``: the padding keeps what the buffer held (NaN)"""
    Wm = rq(wmat(w.float()), dtype)
    out = torch.full((Wm.shape[0], kpad_of(Wm.shape[1], dtype)), float("nan") if mutant == "pad_unwritten" else 0.0)
    out[:, :Wm.shape[1]] = Wm
    return out


def panels_bwd(w, case, dtype, mutant=None):
    """the backward panels of eg_pack_bwd, flat: per phase (ry outer, rx inner) [Cin][Kpad] with K index (ty * TW + tx) * Cout + co holding
    W[co][ci][k0y + ty * s][k0x + tx * s]"""
    B, H, W, Cin, Cout, k, s, p, up = case
    wr = rq(w.float(), dtype)
    out = []
    for ry, rx, (ky0, TH, _), (kx0, TW, _) in bwd_phases(case):
        Kd = TH * TW * Cout
        pan = torch.full((Cin, kpad_of(Kd, dtype)), float("nan") if mutant == "pad_unwritten" else 0.0)
        for ty in range(TH):
            for tx in range(TW):
                pan[:, (ty * TW + tx) * Cout:(ty * TW + tx + 1) * Cout] = wr[:, :, ky0 + ty * s, kx0 + tx * s].t()
        out.append(pan.flatten())
    return torch.cat(out)


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def seed_of(*key):
    h = 0
    for c in str(key):
        h = (h * 131 + ord(c)) % (2 ** 31 - 1)
    return h


def draw(shape, g, kind, dtype, scale=1.0, one_in=4):
    if kind == "int":
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        return sign * (torch.randint(0, one_in, shape, generator=g) == 0).float()
    return rq(torch.randn(shape, generator=g) * scale, dtype)


THIN = {}           # case -> one non-zero in THIN[case] entries of the integer set (default 4), for cases whose results would pass INT_BOUND


@functools.lru_cache(maxsize=None)
def operands(case, dtype, kind):
    """x [B, H, W, Cin], w [Cout, Cin, k, k] (the master: fp32, NOT rounded -- packing rounds it) and its rounded values wr, dy
    [B, OH, OW, Cout]: float32 tensors holding values of the compute dtype"""
    B, H, W, Cin, Cout, k, s, p, up = case
    _, _, OH, OW = geom(case)
    g = torch.Generator().manual_seed(seed_of(case, kind))
    one_in = THIN.get(case, 4)
    x = draw((B, H, W, Cin), g, kind, dtype, 1.0, one_in)
    w = draw((Cout, Cin, k, k), g, kind, "f32", 0.1, one_in)
    dy = draw((B, OH, OW, Cout), g, kind, dtype, 1.0, one_in)
    return dict(x=x, w=w, wr=rq(w, dtype), dy=dy)


EPS = {
    "plain": {},
    "full": dict(bias=True, sigma=True, act="lrelu", mask="relu"),
    "nchw_tanh": dict(bias=True, act="tanh", nchw=True),
    "act_none": dict(bias=True, act="none"),
    "act_lrelu": dict(bias=True, act="lrelu"),
    "act_relu": dict(bias=True, act="relu"),
    "act_tanh": dict(bias=True, act="tanh"),
    "act_sigmoid": dict(bias=True, act="sigmoid"),
    "mask_lrelu": dict(mask="lrelu"),
    "mask_relu": dict(mask="relu"),
    "tapes": dict(sigma=True),
    "bias_mod": dict(bias=True, bias_mod=6),
}


def ep_exact(ep):
    """the integer set has exact results under this epilogue"""
    return EPS[ep].get("act", "none") not in ("tanh", "sigmoid")


@functools.lru_cache(maxsize=None)
def ep_operands(case, bwd, ep, dtype, kind):
    """the epilogue's operands for ``epilogue``: three tapes of cdiv(M, 3) lattice rows where it has a sigma; the mask in the output's
    layout and type"""
    cfg = EPS[ep]
    B, H, W, Cin, Cout, k, s, p, up = case
    XH, XW, OH, OW = geom(case)
    N = Cin if bwd else Cout
    R = B * XH * XW if bwd else B * OH * OW
    g = torch.Generator().manual_seed(seed_of(case, bwd, ep, kind))
    e = dict(act=cfg.get("act", "none"), slope=SLOPE[kind][0], nchw=bool(cfg.get("nchw")))
    if cfg.get("bias"):
        e["bias"] = torch.randint(-2, 3, (N,), generator=g).float() if kind == "int" else torch.randn(N, generator=g)
        e["bias_mod"] = cfg.get("bias_mod", 0)
    if cfg.get("sigma"):
        e["sigma"] = torch.tensor(SIGMAS[kind])
        e["sigma_rows"] = cdiv(rows_of(case), 3)
    if cfg.get("mask"):
        e["mask"] = draw((R, N), g, kind, "f32" if e["nchw"] else dtype)
        e["mask_act"], e["mask_slope"] = cfg["mask"], SLOPE[kind][1]
    return e


@functools.lru_cache(maxsize=None)
def nt_ref(case, bwd, ep, dtype, kind):
    """(want float64, yardstick) of one NT launch in its output layout: [rows][N] in pixel order, or [B][N][DH][DW] for EG_OUT_NCHW_F32"""
    o, e = operands(case, dtype, kind), ep_operands(case, bwd, ep, dtype, kind)
    rows = lattice_rows(case, bwd)

    def run(dt):
        acc = conv_bwd_data(o["dy"], o["wr"], case, dt) if bwd else conv_fwd(o["x"], o["wr"], case, dt)
        v = epilogue(acc, rows, e)
        return to_nchw(v, case, bwd) if e["nchw"] else v
    want = run(torch.float64)
    if kind == "int":
        return want, 0.0
    return want, dist(stored(run(torch.float32), "f32" if e["nchw"] else dtype), want)


@functools.lru_cache(maxsize=None)
def wgrad_ref(case, dtype, kind, wgs_target=0):
    """(variant, want float64 slab, yardstick)"""
    o = operands(case, dtype, kind)
    variant, splits = wgrad_splits(case, dtype, wgs_target)
    want = wgrad_slab(o["x"], o["dy"], case, splits)
    return variant, want, (0.0 if kind == "int" else dist(wgrad_slab(o["x"], o["dy"], case, splits, torch.float32), want))


# ---- the case tables: (B, H, W, Cin, Cout, k, stride, pad, up) ----------------------------------------------------------------------------
# one NT launch: ``ws``: None (no split-K scratch), "exact" (the restated bytes of ``splitk`` splits), "short" (4 bytes less: the planner
# must halve the split), "query" (eg_conv_splitk_ws_bytes); ``label``: what eg_igemm_nt_tile_ep must answer (None: the planner's choice, not
# pinned here); ``vs_reg``: the result must have the bits of EG_NT_REG on the same case
Launch = collections.namedtuple("Launch", "case bwd variant splitk ep ws label vs_reg")
DMA_LABEL = {NT_BUF128: (128131, 128132), NT_PERS: (128135, 128135), NT_S8: (256147, 256148), NT_S8P: (256149, 256150), NT_S8H: (128151, 128152)}
TILE_ROWS = {NT_REG: 128, NT_BUF128: 128, NT_PERS: 128, NT_S8: 256, NT_S8P: 256, NT_S8H: 128}


def reg_bn(case, bwd, forced):
    """column tile of the register-staged kernel: 16 / 32 / 64 by N, 128 above -- under EG_NT_AUTO 64 while there are fewer than 512 tiles"""
    N = case[3] if bwd else case[4]
    if N <= 64:
        return 16 if N <= 16 else (32 if N <= 32 else 64)
    tiles = cdiv(rows_of(case), 128) * cdiv(N, 128) * nphase_of(case, bwd)
    return 64 if not forced and tiles < 512 else 128


def reg_launches(case, dtype, eps=("plain",), bwd_too=True, auto_label=True):
    """EG_NT_REG forced and EG_NT_AUTO once, forward and -- where geom_bwd admits the case -- backward-data.  (The cases that use this have
    N % 128 != 0, a ragged channel count or an NCHW output: the planner leaves those to the register-staged kernel.)"""
    out = []
    for bwd in ((False, True) if bwd_too else (False,)):
        if bwd and not bwd_ok(case, dtype):
            continue
        if not bwd and case[3] % VEC[dtype]:
            continue
        for i, ep in enumerate(eps):
            out.append(Launch(case, bwd, NT_REG, 0, ep, None, 128000 + reg_bn(case, bwd, True), False))
            if i == 0:
                out.append(Launch(case, bwd, NT_AUTO, 0, ep, None, 128000 + reg_bn(case, bwd, False) if auto_label else None, False))
    return out


def dma_launches(case, dtype, variants, eps=("plain", "full"), bwd=False, splitk=0, ws=None):
    out = []
    for v in variants:
        for ep in eps:
            out.append(Launch(case, bwd, v, splitk, ep, ws, DMA_LABEL[v][1 if splitk > 1 and ws == "exact" else 0],
                              splitk <= 1 and v != NT_S8P))
    return out


ALL_DMA = (NT_BUF128, NT_PERS, NT_S8, NT_S8P, NT_S8H)
SPLIT_DMA = (NT_BUF128, NT_S8, NT_S8P, NT_S8H)


@functools.lru_cache(maxsize=None)
def nt_groups(dtype):
    """{group name: [Launch]}: the NT table of the issue.  vec and bk scale the channel counts with the dtype"""
    v, bk = VEC[dtype], BK[dtype]
    G = collections.OrderedDict()
    # -- the register-staged kernel
    G["one_element"] = reg_launches((1, 1, 1, v, 1, 1, 1, 0, 0), dtype)
    for Cout in (8, 19, 24, 40, 160):                     # column tiles 16, 32, 32, 64, 128 (64 under auto) with ragged N
        G[f"cols_{Cout}_m96"] = reg_launches((6, 4, 4, 24, Cout, 3, 1, 1, 0), dtype)
        G[f"cols_{Cout}_m320"] = reg_launches((5, 8, 8, 24, Cout, 3, 1, 1, 0), dtype)
    G["nonsquare_4x16"] = reg_launches((3, 4, 16, 24, 40, 3, 1, 1, 0), dtype, ("plain", "full"))
    G["nonsquare_16x4"] = reg_launches((3, 16, 4, 24, 40, 3, 1, 1, 0), dtype, ("plain", "full"))
    G["k3_up"] = reg_launches((2, 4, 8, 16, 24, 3, 1, 1, 1), dtype)
    G["k1"] = reg_launches((2, 8, 4, 16, 24, 1, 1, 0, 0), dtype)
    G["k4_s1_p0"] = reg_launches((3, 4, 4, 16, 24, 4, 1, 0, 0), dtype)
    G["k3_s2"] = reg_launches((2, 8, 16, 16, 24, 3, 2, 1, 0), dtype)          # backward phases of 1, 2, 2 and 4 taps
    G["k_below_bk"] = reg_launches((2, 4, 4, v, 24, 1, 1, 0, 0), dtype)       # K = vec < bk: the rest of the K tile is padding
    G["nchw_fwd"] = reg_launches((2, 8, 4, 16, 3, 3, 1, 1, 0), dtype, ("nchw_tanh",), bwd_too=False)
    G["nchw_bwd_3"] = [l for l in reg_launches((2, 4, 8, 3, 16, 4, 2, 1, 0), dtype, ("nchw_tanh",)) if l.bwd]
    G["nchw_bwd_1"] = [l for l in reg_launches((2, 4, 8, 1, 16, 4, 2, 1, 0), dtype, ("nchw_tanh",)) if l.bwd]
    G["epilogues"] = reg_launches((6, 4, 8, 16, 24, 3, 1, 1, 0), dtype,       # M = 192: tapes of 64 rows, a boundary inside a row tile
                                  ("act_none", "act_lrelu", "act_relu", "act_tanh", "act_sigmoid", "mask_lrelu", "mask_relu", "tapes",
                                   "bias_mod", "full"))
    for N in (32, 64):                                    # the K split of the register-staged kernel: M = 32, K = 16 * 64
        c = (2, 8, 8, 64, N, 4, 2, 1, 0)
        G[f"reg_split_{N}"] = [Launch(c, False, NT_REG, 8, ep, "exact", 128000 + N, False) for ep in ("plain", "full")]
    # -- the DMA variants: N % 128 == 0, Cin % bk == 0 or a single tap
    G["ragged_132"] = dma_launches((33, 4, 4, bk, 128, 4, 2, 1, 0), dtype, (NT_BUF128, NT_PERS, NT_S8H))
    # (EG_NT_S8P cannot run these two: a 4 x 4 / stride-2 kernel over 2 x 2 or 2 x 4 outputs puts 64 x 9 or 32 x 15 patch pixels into a tile,
    #  past its 448 slots -- the label check says -1; its ragged row tile is s8p_4px below, M = 280)
    G["ragged_260"] = dma_launches((65, 4, 4, bk, 128, 4, 2, 1, 0), dtype, (NT_S8,))
    G["ragged_136_4x8"] = dma_launches((17, 4, 8, bk, 128, 4, 2, 1, 0), dtype, (NT_BUF128, NT_PERS, NT_S8H))
    G["ragged_264_4x8"] = dma_launches((33, 4, 8, bk, 128, 4, 2, 1, 0), dtype, (NT_S8,))
    for nk in (1, 2, 3, 4):
        G[f"kloop_{nk}"] = dma_launches((3, 4, 8, nk * bk, 128, 1, 1, 0, 0), dtype, ALL_DMA if nk > 1 else ALL_DMA[1:], ("plain",))
    G["kloop_16"] = dma_launches((3, 8, 16, bk, 128, 4, 2, 1, 0), dtype, ALL_DMA, ("plain",))
    G["n256"] = dma_launches((3, 4, 16, bk, 256, 3, 1, 1, 0), dtype, ALL_DMA)
    G["dma_up"] = dma_launches((2, 8, 8, bk, 128, 3, 1, 1, 1), dtype, ALL_DMA)
    G["dma_bwd_k4"] = dma_launches((3, 8, 16, 128, bk, 4, 2, 1, 0), dtype, ALL_DMA, bwd=True)
    G["dma_bwd_k3"] = dma_launches((3, 8, 16, 128, bk, 3, 2, 1, 0), dtype, ALL_DMA, bwd=True)       # K loops of 1, 2, 2 and 4 tiles
    G["pers_bwd_k2"] = dma_launches((3, 8, 4, 128, v, 2, 2, 0, 0), dtype, (NT_PERS,), bwd=True)    # four single-tap phases, Cout = vec
    G["pers_second_round"] = dma_launches((513, 8, 8, v, 256, 1, 1, 0, 0), dtype, (NT_PERS,), ("full",))   # 514 tiles on 512 workgroups
    G["s8p_4px"] = dma_launches((70, 2, 2, 2 * bk, 128, 1, 1, 0, 0), dtype, (NT_S8P,))    # OH * OW = 4: 64 images per tile, B = 64 + 6 (k = 1:
                                                                                          # the only patch of 64 images that fits the slots)
    G["s8p_16x16"] = dma_launches((1, 16, 16, bk, 128, 3, 1, 1, 0), dtype, (NT_S8P,), ("plain",))
    G["s8p_16x32"] = dma_launches((1, 16, 32, bk, 128, 3, 1, 1, 0), dtype, (NT_S8P,), ("plain",))
    G["s8p_4x64"] = dma_launches((2, 4, 64, bk, 128, 3, 1, 1, 0), dtype, (NT_S8P,), ("plain",))
    G["s8p_k4_s2"] = dma_launches((2, 16, 32, bk, 128, 4, 2, 1, 0), dtype, (NT_S8P,), ("plain",))
    # -- K splits
    for ns in (2, 4):
        G[f"split_{ns}"] = dma_launches((5, 8, 8, bk, 128, 4, 2, 1, 0), dtype, SPLIT_DMA, splitk=ns, ws="exact")
    G["split_2_short"] = dma_launches((5, 8, 8, bk, 128, 4, 2, 1, 0), dtype, SPLIT_DMA, ("plain",), splitk=2, ws="short")
    G["split_3_tiles_in_2"] = dma_launches((3, 4, 8, 3 * bk, 128, 1, 1, 0, 0), dtype, SPLIT_DMA, ("plain",), splitk=2, ws="exact")
    G["split_5_tiles_in_4"] = dma_launches((65, 1, 2, 5 * bk, 128, 1, 1, 0, 0), dtype, SPLIT_DMA, splitk=4, ws="exact")   # M = 130
    G["split_bwd"] = dma_launches((3, 8, 16, 128, bk, 4, 2, 1, 0), dtype, SPLIT_DMA, ("full",), bwd=True, splitk=2, ws="exact")
    G["auto_query"] = [Launch((33, 4, 4, bk, 128, 4, 2, 1, 0), False, NT_AUTO, 0, "full", "query", None, False),
                       Launch((2, 4, 4, 16 * bk, 128, 4, 2, 1, 0), False, NT_AUTO, 0, "full", "query", None, False)]
    return G


def s8p_refused_case(dtype):
    """OW = 256 under a 3 x 3 kernel: the patch of one output row (3 x 258 pixels) is past the kernel's 448 slots -- the query answers -1"""
    return (1, 2, 256, BK[dtype], 128, 3, 1, 1, 0)


def nt_cases(dtype):
    """every distinct (case, bwd, ep) of the NT table"""
    return sorted({(l.case, l.bwd, l.ep) for ls in nt_groups(dtype).values() for l in ls})


def scratch_bytes(l):
    """bytes of the split-K scratch of a launch with ws == "exact" / "short" """
    b = splitk_bytes(l.case, l.bwd, TILE_ROWS[l.variant], l.splitk)
    return b - 4 if l.ws == "short" else b


# weight gradient, per-tap kernel: (case, dtypes)
SIXTEEN = ("bf16", "f16")
TN_CASES = tuple(((2, 4, 8, Cin, Cout, 3, 1, 1, 0), DTYPES) for Cout in (32, 64, 128) for Cin in (32, 64, 128)) + (   # the nine tile configurations
    ((2, 4, 8, 24, 40, 3, 1, 1, 0), DTYPES),               # ragged channels: Cout = 40 on a 64 tile, Cin = 24 on a 32 tile
    ((2, 4, 8, 72, 40, 3, 1, 1, 0), DTYPES),               # Cin = 72: two 64 tiles, the second ragged
    ((3, 2, 2, 64, 128, 1, 1, 0, 0), DTYPES),              # M = 12; in 16-bit the single-output-tile launch with 64 rows per step
    ((208, 2, 2, 64, 128, 1, 1, 0, 0), DTYPES),            # M = 832: splits of 288, 288 and 256 rows
    ((209, 2, 2, 64, 128, 1, 1, 0, 0), DTYPES),            # M = 836: the last split ends 4 rows into a step
    ((209, 2, 2, 24, 40, 3, 1, 1, 0), DTYPES),             # the same rows under 9 taps and 32-row steps
    ((2, 4, 16, 32, 32, 3, 1, 1, 0), DTYPES),              # non-square
    ((2, 16, 4, 32, 32, 3, 1, 1, 0), DTYPES),
    ((2, 4, 8, 32, 32, 3, 1, 1, 1), DTYPES),               # up
    ((12, 4, 4, 32, 32, 4, 1, 0, 0), DTYPES),              # k = 4, s = 1, p = 0: M = 12
    ((2, 8, 16, 32, 64, 4, 2, 1, 0), ("f32",)),            # k = 4, s = 2, p = 1 (16-bit: the parity-class kernel)
    ((2, 8, 16, 24, 40, 4, 2, 1, 0), DTYPES),              # ... and with channel counts the parity-class kernel refuses
)
TN_ROWS = {(208, 2, 2, 64, 128, 1, 1, 0, 0): (288, 288, 256), (209, 2, 2, 64, 128, 1, 1, 0, 0): (288, 288, 260),
           (209, 2, 2, 24, 40, 3, 1, 1, 0): (288, 288, 260), (3, 2, 2, 64, 128, 1, 1, 0, 0): (12,)}

# weight gradient, parity-class kernel (16-bit, k = 4, s = 2, p = 1): (case, wgs_targets, (channel tile, rows of each split at target 0)).
# The short cases sit on 8 x 8 inputs, not 4 x 4: 2 x 2 outputs put 16 images of 3 x 3 patch pixels into a K step, 144 slots of the stage's
# 136, and eg_tn8_plan refuses them at every channel tile (TN8_SMALL_REFUSED; the per-tap kernel runs them)
TN8_CASES = (
    ((4, 8, 8, 32, 32, 4, 2, 1, 0), (0,), (32, (64,))),                        # one K step
    ((20, 8, 8, 64, 64, 4, 2, 1, 0), (0,), (64, (320,))),                      # 5 steps in one split
    ((36, 8, 8, 128, 128, 4, 2, 1, 0), (0, 128, 1), (128, (320, 256))),       # 9 steps in two splits of 5 and 4
    ((128, 8, 8, 96, 96, 4, 2, 1, 0), (0, 128, 1), (32, (256,) * 8)),          # 32 steps: 8 splits, 4 at a target of 128, 1 at 1
    ((8, 4, 16, 32, 32, 4, 2, 1, 0), (0,), (32, (128,))),                      # H = 4, W = 16: 4 images per step
    ((2, 32, 8, 64, 64, 4, 2, 1, 0), (0,), (64, (128,))),                      # H = 32, W = 8: one image per step
    ((1, 16, 32, 128, 128, 4, 2, 1, 0), (0,), (128, (128,))),                  # H = 16, W = 32: two steps per image
    ((2, 2, 128, 128, 128, 4, 2, 1, 0), (0,), (128, (128,))),                  # OW = 64, the widest row: admitted at 128 channels ...
    ((4, 8, 8, 64, 192, 4, 2, 1, 0), (0,), (64, (64,))),                       # mixed tiles: one along Cin, three along Cout
)
TN8_SMALL_REFUSED = ((16, 4, 4, 32, 32, 4, 2, 1, 0), (16, 4, 4, 128, 128, 4, 2, 1, 0))
TN8_REFUSED = (2, 2, 128, 32, 32, 4, 2, 1, 0)                                  # ... and refused at 32 (the per-tap kernel runs it)


def all_conv_cases(dtype):
    """every convolution of the tables (the packing tests run them all)"""
    cs = {c for c, _, _ in nt_cases(dtype)} | {c for c, dts in TN_CASES if dtype in dts}
    if dtype != "f32":
        cs |= {c for c, _, _ in TN8_CASES} | {TN8_REFUSED} | set(TN8_SMALL_REFUSED)
    return sorted(cs)


def pack_keys(dtype):
    """the tables' distinct (Cin, Cout, k, s, p): all that packing depends on"""
    return sorted({c[3:8] for c in all_conv_cases(dtype)})

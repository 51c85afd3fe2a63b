"""The skinny-end kernels of csrc/small.hip on the MI355X against float64 (tests/small_refs.py) at their launch edges: the small-N dense head
(eg_dense_small_fwd, _fwd_sn, _fwd_slices, _bwd, _wgrad, _bgrad, eg_head_prep_sn), the image-side convolution (eg_conv_img_fwd,
eg_conv_img_wgrad, eg_im2col_img, eg_col2im_img), the helpers (eg_act_grad_mul_bias_nchw, eg_flat_reduce, eg_cast_pad) and eg_wgrad_c1.

Every tensor a kernel writes is a slice of a larger buffer prefilled with NaN: after the call every element of the slice is written (a NaN
left over fails the comparison) and everything outside it is still NaN.  Operands the kernels must not read are NaN too: the K padding of
the weight panels, the gaps of the row strides ldy and ldyy.  Every launch is made twice on fresh buffers and gives the same bits.  Values
follow the project's rule: a result may miss float64, computed on the pre-rounded operands, by K = 8 times what the float32 restatement on
the CPU misses it by (rounded to the output dtype where the kernel stores that dtype); the figure and the yardstick are printed before they
are compared.  Copies (eg_im2col_img, eg_cast_pad) are compared bit for bit.

eg_conv_img_wgrad and eg_wgrad_c1 add one long sequential chain per thread (OH * OW = 1024 terms at most here; 2 * W = 256), where torch's
blocked float32 sums could have been a yardstick no correct kernel meets.  They are not: measured on the MI355X the worst figures are 3.88
yardsticks (eg_conv_img_wgrad, f32, (3, 64, 64, 64, 4, 2, 1): 1.34e-06 of 3.44e-07) and 2.88 (eg_wgrad_c1, f32, (1, 8, 128): 4.15e-07 of
1.44e-07), so every case keeps the plain float32 restatement as its yardstick (profiles/skinny_ends_float64.txt has all figures)."""
import importlib

import pytest
import torch

import small_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = -7.25                    # sentinel of the columns eg_head_prep_sn must keep (exact in every dtype)
GUARD = 64                      # sentinel elements either side of a slice (a multiple of 16 bytes in every dtype)
eg = None
ops = None
ACT = None


def setup_module(module):
    global eg, ops, ACT
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops
    ACT = {None: ops.ACT_NONE, "none": ops.ACT_NONE, "lrelu": ops.ACT_LRELU, "relu": ops.ACT_RELU, "tanh": ops.ACT_TANH, "sigmoid": ops.ACT_SIGMOID}
    torch.set_num_threads(16)


def types(dtype):
    dt = eg.engine.parse_dtype(dtype)
    assert ops.vec(dt) == R.VEC[dtype] and ops.bk(dt) == R.BK[dtype]
    return dt, R.TORCH_DTYPE[dtype]


def dev(t, tdt=None):
    t = t.to(DEV)
    return t.contiguous() if tdt is None else t.to(tdt).contiguous()


def arena(shape, tdt=torch.float32, init=None, fill=NAN):
    """(buffer, view): a contiguous tensor of ``shape`` on a 16-byte boundary with NaN all around, filled with ``fill`` or ``init``"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), NAN, dtype=tdt, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD:GUARD + n].view(shape)
    if init is not None:
        view.copy_(init.reshape(shape))
    elif fill == fill:
        view.fill_(fill)
    return buf, view


def intact(buf, view):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + view.numel():]).all())


def all_nan(t):
    return bool(torch.isnan(t).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def check(group, dtype, what, got, want, yard):
    """print, then assert, the distance of ``got`` from float64 against K yardsticks; ``got`` / ``want`` may be tuples (the worst counts)"""
    fig = R.worst(got, want) if isinstance(got, (tuple, list)) else R.dist(got, want)
    print(f"SMALL {group} {dtype} {what}: error {fig:.3g} = {fig / yard if yard else 0.0:.2f} yardsticks of {yard:.3g}, bound {R.K * yard:.3g}")
    assert fig <= R.K * yard, (group, dtype, what, fig, yard)
    return fig


def check_each(group, dtype, what, names, got, want, yards):
    """every output against its own yardstick"""
    for name, g, w, y in zip(names, got, want, yards):
        check(group, dtype, f"{what} {name}", g, w, y)


def twice(run):
    """``run()`` -> tuple of output tensors, called on fresh buffers twice: the same bits"""
    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(same_bits(x, y) for x, y in zip(a, b)), "a second launch gives other bits"
    return a


# ---- 1. the small-N dense head -------------------------------------------------------------------------------------------------------------
def dense_operands(case, dtype):
    """x, the [N][Kpad] panel in k = t*Cin + ci order with NaN in its pad columns, bias, sigma, dy, mask on the device"""
    dt, tdt = types(dtype)
    c = R.dense_case(case, dtype)
    Kd, N = c["K"], case[2]
    Kpad = ops.round_up(Kd, ops.bk(dt)) + ops.bk(dt)
    wp = torch.full((N, Kpad), NAN, dtype=tdt, device=DEV)
    wp[:, :Kd] = dev(c["w"], tdt)
    return dt, tdt, c, Kd, Kpad, dict(x=dev(c["x"], tdt), wp=wp, bias=dev(c["bias"]), sigma=dev(c["sigma"]), dy=dev(c["dy"]), mask=dev(c["mask"], tdt))


def ws_sizes(case):
    B, _, N = case
    return [None, 16 * B * N] + ([2 * B * N] if case == R.DENSE_CLIPPED else [])


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_small_fwd_against_float64(dtype, case):
    """eg_dense_small_fwd and _fwd_sn without a workspace (one slice), with 16 B N floats (the K split of small_refs.DENSE_LAUNCH) and, for
    (3, 2051, 64), with 2 B N floats (two slices); with and without bias; sigma absent, sigma[0] for all rows, one sigma per tape of 2 rows"""
    B, q, N = case
    dt, tdt, c, Kd, Kpad, o = dense_operands(case, dtype)
    for wsn in ws_sizes(case):
        for has_bias, sf in R.dense_variants(B)[0]:
            bufs = []

            def run():
                by, y = arena((B, N))
                bw, ws = (None, None) if wsn is None else arena(wsn)
                bias = o["bias"] if has_bias else None
                if sf is None:
                    ops.dense_small_fwd(dt, o["x"], o["wp"], bias, y, B, Kd, Kpad, N, ws)
                else:
                    ops.dense_small_fwd_sn(dt, o["x"], o["wp"], bias, y, B, Kd, Kpad, N, o["sigma"], sf, ws)
                assert intact(by, y) and (ws is None or intact(bw, ws))
                bufs.append(ws)
                return (y,)
            y, = twice(run)
            ns = R.ns_of(B, Kd, R.VEC[dtype], wsn or 0, N)
            if bufs[0] is not None and ns > 1:
                assert all_nan(bufs[0][ns * B * N:]) and not bool(torch.isnan(bufs[0][:ns * B * N]).any()), "workspace use is not ns * B * N"
            check("dense_small_fwd" + ("" if sf is None else "_sn"), dtype, f"{case} ws={wsn} ns={ns} bias={has_bias} sigma_rows={sf}", y,
                  c["fwd"][(has_bias, sf)], c["yard_fwd"])


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_small_fwd_slices_are_the_sums_of_the_forward(dtype, case):
    """the slice count is the one small_refs.ns_of states; the slices added in float32 in slice order, plus the bias, are the bits of
    eg_dense_small_fwd with the same workspace; and their sum is within the bound of float64"""
    B, q, N = case
    dt, tdt, c, Kd, Kpad, o = dense_operands(case, dtype)
    for wsn in ws_sizes(case)[1:]:
        bw, ws = arena(wsn)
        ns = ops.dense_small_fwd_slices(dt, o["x"], o["wp"], B, Kd, Kpad, N, ws)
        want_ns = R.ns_of(B, Kd, R.VEC[dtype], wsn, N)
        assert ns == want_ns and (wsn != 16 * B * N or ns == R.DENSE_LAUNCH[case][0]), (ns, want_ns)
        parts = ws[:ns * B * N].view(ns, B, N)
        assert intact(bw, ws) and all_nan(ws[ns * B * N:]) and not bool(torch.isnan(parts).any())
        tot = torch.zeros(B, N, device=DEV)
        for z in range(ns):
            tot = tot + parts[z]
        by, y = arena((B, N))
        bw2, ws2 = arena(wsn)
        ops.dense_small_fwd(dt, o["x"], o["wp"], o["bias"], y, B, Kd, Kpad, N, ws2)
        assert same_bits(tot + o["bias"], y), "slices + bias are not the forward's bits"
        if ns > 1:
            assert same_bits(ws2[:ns * B * N], ws[:ns * B * N]), "the forward's own slices differ"
        check("dense_small_fwd_slices", dtype, f"{case} ws={wsn} ns={ns}", tot, c["fwd"][(False, None)], c["yard_fwd"])


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_small_bwd_against_float64(dtype, case):
    """mask absent, LeakyReLU 0.2 and ReLU (the mask is an operand drawn in the dtype); sigma absent, sigma[0], one per tape"""
    B, q, N = case
    dt, tdt, c, Kd, Kpad, o = dense_operands(case, dtype)
    gy = R.gy_of(B, Kd, R.VEC[dtype])
    assert gy == R.DENSE_LAUNCH[case][2]
    for ma, sf in R.dense_variants(B)[1]:
        def run():
            bx, dx = arena((B, Kd), tdt)
            ops.dense_small_bwd(dt, o["dy"], o["wp"], None if ma is None else o["mask"], dx, B, Kd, Kpad, N, ACT[ma], R.SLOPE,
                                None if sf is None else o["sigma"], sf or 0)
            assert intact(bx, dx)
            return (dx,)
        dx, = twice(run)
        assert bool(torch.isfinite(dx.float()).all()), "dx is not finite everywhere"
        check("dense_small_bwd", dtype, f"{case} gy={gy} mask={ma} sigma_rows={sf}", dx.float(), c["bwd"][(ma, sf)], c["yard_bwd"])


@pytest.mark.parametrize("case", R.DENSE_WGRAD_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_small_wgrad_accumulates_against_float64(dtype, case):
    """gw starts from random values (the kernel adds to it); gb absent and given (added to as well), each form launched twice; gw and gb
    have a yardstick each.  (512, 8, 32, 8, 1) stages exactly
    64 KiB of dy in LDS, the most the entry point accepts"""
    B, Kd, N, Cin, taps = case
    dt, tdt = types(dtype)
    c = R.dense_wgrad_case(case, dtype)
    dy, x = dev(c["dy"]), dev(c["x"], tdt)
    for with_gb in (False, True):
        def run():
            bw, gw = arena((N, Cin, taps), init=dev(c["gw0"]))
            bb, gb = arena(N, init=dev(c["gb0"]))
            ops.dense_small_wgrad(dt, dy, x, gw, gb if with_gb else None, B, Kd, N, Cin, taps)
            assert intact(bw, gw) and intact(bb, gb)
            return gw, gb
        gw, gb = twice(run)
        if with_gb:
            check_each("dense_small_wgrad", dtype, f"{case}", ("gw", "gb"), (gw, gb), c["want"], c["yard"])
        else:
            assert same_bits(gb, c["gb0"]), "a bias gradient that was not passed was written"
            check("dense_small_wgrad", dtype, f"{case} gb=None gw", gw, c["want"][0], c["yard"][0])


@pytest.mark.parametrize("acc", (0, 1))
@pytest.mark.parametrize("case", R.BGRAD_CASES, ids=str)
def test_dense_small_bgrad_against_float64(case, acc):
    """store mode on a NaN-filled gb (the slot is not read), accumulate mode on random values"""
    B, N = case
    c = R.bgrad_case(case)
    dy = dev(c["dy"])

    def run():
        bb, gb = arena(N, init=dev(c["gb0"]) if acc else None)
        ops.dense_small_bgrad(dy, gb, B, N, accumulate=bool(acc))
        assert intact(bb, gb)
        return (gb,)
    gb, = twice(run)
    check("dense_small_bgrad", "f32", f"{case} accumulate={acc}", gb, c["want"][acc], c["yard"][acc])


@pytest.mark.parametrize("case", R.HEAD_PREP_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_head_prep_sn_against_float64(dtype, case):
    """dy and y with row strides N + 3 and N + 5 and NaN in the gaps; dys written at column col0 of a [rows][npad] buffer whose other
    columns keep a sentinel bit for bit; gb starts non-zero; each case also runs once without sigma, coef or gb, or with the fp32 copy
    dys32 (row stride npad + 4)"""
    rows, rpt, N, npad, col0 = case
    dt, tdt = types(dtype)
    c = R.head_prep_case(case, dtype)
    ldy, ldyy, ld32 = N + 3, N + 5, npad + 4
    dyb, yb = torch.full((rows, ldy), NAN, device=DEV), torch.full((rows, ldyy), NAN, device=DEV)
    dyb[:, :N], yb[:, :N] = dev(c["dy"]), dev(c["y"])
    bias, sigma = dev(c["bias"]), dev(c["sigma"])
    keep = torch.ones(npad, dtype=torch.bool)
    keep[col0:col0 + N] = False
    for variant in ("full", R.HEAD_PREP_EXTRA[R.HEAD_PREP_CASES.index(case)]):
        key = "plain" if variant == "no_sigma" else "sigma"

        def run():
            bd, dys = arena((rows, npad), tdt, fill=SENT)
            bg, gb = arena(N, init=dev(c["gb0"]))
            bc, coef = arena(rows // rpt)
            b32, dys32 = arena((rows, ld32), fill=SENT)
            ops.head_prep_sn(dt, dyb, ldy, yb, ldyy, bias, rows, N, None if variant == "no_sigma" else sigma, rpt, dys, npad, col0,
                             None if variant == "no_gb" else gb, None if variant == "no_coef" else coef, dys32 if variant == "dys32" else None,
                             ld32 if variant == "dys32" else 0)
            assert intact(bd, dys) and intact(bg, gb) and intact(bc, coef) and intact(b32, dys32)
            return dys, gb, coef, dys32
        dys, gb, coef, dys32 = twice(run)
        sent = torch.full((rows, int(keep.sum())), SENT)
        assert same_bits(dys.cpu()[:, keep], sent.to(tdt)), "a column of dys outside [col0, col0 + N) changed"
        yd, yc, yg = c["yard"][key]                                      # one yardstick per output
        names, got, want, yards = ["dys"], [dys[:, col0:col0 + N].float()], [c["want"][key][0]], [yd]
        if variant == "no_gb":
            assert same_bits(gb, c["gb0"])
        else:
            names.append("gb"), got.append(gb), want.append(c["want"][key][2]), yards.append(yg)
        if variant == "no_coef":
            assert all_nan(coef)
        else:
            names.append("coef"), got.append(coef), want.append(c["want"][key][1]), yards.append(yc)
        if variant == "dys32":
            k32 = torch.ones(ld32, dtype=torch.bool)
            k32[col0:col0 + N] = False
            assert same_bits(dys32.cpu()[:, k32], torch.full((rows, int(k32.sum())), SENT)), "a column of dys32 outside [col0, col0 + N) changed"
            # (no bit comparison of dys with dys32 rounded to the dtype: for f16 the product is rounded once, straight to 16 bits)
            check("head_prep_sn", dtype, f"{case} {variant} dys32", dys32[:, col0:col0 + N], c["want"][key][0], c["yard32"][key])
        else:
            assert same_bits(dys32, torch.full((rows, ld32), SENT)), "a dys32 that was not passed was written"
        check_each("head_prep_sn", dtype, f"{case} {variant}", names, got, want, yards)


# ---- 2. the image side ---------------------------------------------------------------------------------------------------------------------
def conv_img_epilogue(c, name, tdt):
    """(the eg_epilogue, the device tensors it points to)"""
    if name == "bias_sigma_lrelu":
        hold = (dev(c["bias"]), dev(c["sigma"]))
        return ops.epilogue(bias=hold[0], sigma=hold[1], act=ops.ACT_LRELU, slope=R.SLOPE, splitk_ws=None), hold
    if name == "mask":
        hold = (dev(c["mask"], tdt),)
        return ops.epilogue(mask=hold[0], mask_act=ops.ACT_LRELU, mask_slope=R.SLOPE, splitk_ws=None), hold
    return None, ()


@pytest.mark.parametrize("case", list(R.CONV_IMG_CASES), ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_conv_img_fwd_against_float64(dtype, case):
    """1, 2, 4, 8 and 16 output channels per thread; OW = 1; a last row strip cut short (OH = 6, OH = 5); a floor in the output size; CI = 4;
    N below and equal to the count of thread groups -- each without an epilogue, with bias + sigma + LeakyReLU, and with a mask"""
    B, CI, H, W, N, k, s, p = case
    dt, tdt = types(dtype)
    c = R.conv_img_case(case, dtype)
    OH, OW = R.conv_out(H, W, k, s, p)
    img, w = dev(c["img"]), dev(c["w"])
    for name in R.CONV_IMG_EPILOGUES:
        ep, hold = conv_img_epilogue(c, name, tdt)

        def run():
            bo, out = arena((B, OH, OW, N), tdt)
            ops.conv_img_fwd(dt, img, w, out, B, CI, H, W, N, k, s, p, ep)
            assert intact(bo, out)
            return (out,)
        out, = twice(run)
        check("conv_img_fwd", dtype, f"{case} cpt={R.CONV_IMG_CASES[case]} {name}", out.float(), c["want"][name], c["yard"][name])


@pytest.mark.parametrize("case", R.CONV_IMG_REFUSED, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_conv_img_fwd_refuses_what_it_cannot_tile(dtype, case):
    """N = 24 against 16 thread groups, and 32 channels per thread: an error return, nothing written"""
    B, CI, H, W, N, k, s, p = case
    dt, tdt = types(dtype)
    OH, OW = R.conv_out(H, W, k, s, p)
    img, w = torch.ones(B, CI, H, W, device=DEV), torch.ones(N, CI, k, k, device=DEV)
    bo, out = arena((B, OH, OW, N), tdt)
    with pytest.raises(RuntimeError, match="eg_conv_img_fwd"):
        ops.conv_img_fwd(dt, img, w, out, B, CI, H, W, N, k, s, p, None)
    torch.cuda.synchronize()
    assert all_nan(bo)


@pytest.mark.parametrize("case", list(R.CONV_WGRAD_CASES), ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_conv_img_wgrad_against_float64(dtype, case):
    """every MAXT bucket of the launcher (1, 2, 3, 6, 12, 24 taps per thread), inside and at the top of a bucket, N from 1 to 256, the
    largest image that fits LDS, a non-square image; the slab is compared image by image"""
    CI, H, W, N, k, s, p = case
    B = R.CONV_WGRAD_B
    dt, tdt = types(dtype)
    c = R.conv_wgrad_case(case, dtype)
    img, dz = dev(c["img"]), dev(c["dz"], tdt)
    assert ops.conv_img_wgrad_ws_bytes(B, CI, N, k) == B * N * CI * k * k * 4

    def run():
        bs, slab = arena((B, N, CI, k, k))
        ops.conv_img_wgrad(dt, dz, img, slab, B, CI, H, W, N, k, s, p)
        assert intact(bs, slab)
        return (slab,)
    slab, = twice(run)
    maxt = R.CONV_WGRAD_CASES[case]
    check("conv_img_wgrad", dtype, f"{case} taps={maxt} MAXT={R.maxt_bucket(maxt)}", list(slab), list(c["want"]), c["yard"])


@pytest.mark.parametrize("case", R.CONV_WGRAD_REFUSED, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_conv_img_wgrad_refuses_too_many_taps_and_too_large_an_image(dtype, case):
    CI, H, W, N, k, s, p = case
    B = R.CONV_WGRAD_B
    dt, tdt = types(dtype)
    OH, OW = R.conv_out(H, W, k, s, p)
    img, dz = torch.ones(B, CI, H, W, device=DEV), torch.ones(B, OH, OW, N, device=DEV, dtype=tdt)
    bs, slab = arena((B, N, CI, k, k))
    with pytest.raises(RuntimeError, match="eg_conv_img_wgrad"):
        ops.conv_img_wgrad(dt, dz, img, slab, B, CI, H, W, N, k, s, p)
    torch.cuda.synchronize()
    assert all_nan(bs)


def run_im2col(dtype, case):
    B, CI, H, W, k, s, p, Kp = case
    dt, tdt = types(dtype)
    img = R.im2col_img(case)
    OH, OW = R.conv_out(H, W, k, s, p)
    want = R.im2col(img, k, s, p, Kp).to(tdt)
    imgd = dev(img)

    def run():
        bo, out = arena((B * OH * OW, Kp), tdt)
        ops.im2col_img(dt, imgd, out, B, CI, H, W, k, s, p, Kp)
        assert intact(bo, out)
        return (out,)
    out, = twice(run)
    assert same_bits(out, want), "not F.unfold's values rounded to the dtype with exact zeros in the pad columns"
    total, blocks = R.im2col_blocks(*case, R.VEC[dtype])
    print(f"SMALL im2col_img {dtype} {case} template k={R.im2col_template(k)} vectors={total} blocks={blocks}: exact")


@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_im2col_img_is_exact(dtype, case):
    """k = 3 (compile-time), k = 5 and k = 2 (the run-time-k template), each with K padding; a copy, so exact"""
    run_im2col(dtype, case)


def test_im2col_img_grid_stride():
    """the compile-time k = 4 template with 2 113 536 output vectors against 8192 blocks of 256 threads: the grid-stride loop runs"""
    run_im2col("f32", R.IM2COL_LARGE)


@pytest.mark.parametrize("case", R.COL2IM_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_col2im_img_against_float64(dtype, case):
    C, B, Hin, Win, k, s, p = case
    dt, tdt = types(dtype)
    c = R.col2im_case(case, dtype)
    cols, bias = dev(c["cols"], tdt), dev(c["bias"])
    OH, OW = (Hin - 1) * s - 2 * p + k, (Win - 1) * s - 2 * p + k
    for a in R.COL2IM_ACTS:
        def run():
            bo, out = arena((B, C, OH, OW))
            ops.col2im_img(dt, cols, B, C, Hin, Win, k, s, p, bias, ACT[a], 0.0, out)
            assert intact(bo, out)
            return (out,)
        out, = twice(run)
        check("col2im_img", dtype, f"{case} {a}", out, c["want"][a], c["yard"][a])


# ---- 3. helpers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", (0, 1))
@pytest.mark.parametrize("name", R.ACT_GRAD_ACTS)
@pytest.mark.parametrize("case", R.ACT_GRAD_CASES, ids=str)
def test_act_grad_mul_bias_nchw_against_float64(case, name, acc):
    B, C, HW = case
    c = R.act_grad_case(case, name)
    g, a = dev(c["g"]), dev(c["a"])

    def run():
        bo, out = arena((B, C, HW))
        bp, part = arena(B * C)
        bg, gb = arena(C, init=dev(c["gb0"]) if acc else None)
        ops.act_grad_mul_bias_nchw(g, a, out, B, C, HW, ACT[name], R.SLOPE, part, gb, accumulate=bool(acc))
        assert intact(bo, out) and intact(bp, part) and intact(bg, gb)
        return out, gb
    got = twice(run)
    check_each("act_grad_mul_bias_nchw", "f32", f"{case} {name} accumulate={acc}", ("out", "gb"), got, c["want"][acc], c["yard"][acc])


@pytest.mark.parametrize("acc", (0, 1))
@pytest.mark.parametrize("case", R.FLAT_REDUCE_CASES, ids=str)
def test_flat_reduce_against_float64(case, acc):
    """one element, either side of one block, and more floats than 1024 blocks of 256 threads hold (the grid-stride loop)"""
    nslab, total = case
    c = R.flat_reduce_case(case)
    slab = dev(c["slab"])

    def run():
        bg, grad = arena(total, init=dev(c["g0"]) if acc else None)
        ops.flat_reduce(slab, nslab, total, grad, accumulate=bool(acc))
        assert intact(bg, grad)
        return (grad,)
    grad, = twice(run)
    check("flat_reduce", "f32", f"{case} accumulate={acc}", grad, c["want"][acc], c["yard"][acc])


@pytest.mark.parametrize("case", R.CAST_PAD_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_cast_pad_is_exact(dtype, case):
    rows, n, npad = case
    dt, tdt = types(dtype)
    src = R.cast_pad_src(case)
    srcd = dev(src) if n else torch.full((1,), NAN, device=DEV)          # (an empty tensor has no address)

    def run():
        bo, out = arena((rows, npad), tdt)
        ops.cast_pad(dt, srcd, out, rows, n, npad)
        assert intact(bo, out)
        return (out,)
    out, = twice(run)
    assert same_bits(out, R.cast_pad(src, npad, dtype).to(tdt))


# ---- 4. eg_wgrad_c1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.WGRAD_C1_CASES, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_wgrad_c1_against_float64(dtype, case):
    """one unit, the widest row the entry point accepts, and four units: every unit's slab against the restatement that rounds dy through
    the dtype as the kernel does"""
    B, H, W = case
    dt, tdt = types(dtype)
    c = R.wgrad_c1_case(case, dtype)
    x, dy = dev(c["x"], tdt), dev(c["dy"])
    units = B * (H // 8)
    assert ops.wgrad_c1_ok(dt, 64, H, W, 1, 3, 1, 1) and ops.wgrad_c1_splits(B, H) == units

    def run():
        bs, slab = arena((units, 9, 64))
        assert ops.wgrad_c1(dt, x, dy, slab, B, H, W, 64) == units
        assert intact(bs, slab)
        return (slab,)
    slab, = twice(run)
    check("wgrad_c1", dtype, f"{case} units={units}", slab, c["want"], c["yard"])


@pytest.mark.parametrize("hw", R.WGRAD_C1_REFUSED, ids=str)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_wgrad_c1_refuses_a_wide_row_and_a_ragged_height(dtype, hw):
    H, W = hw
    dt, tdt = types(dtype)
    assert not R.wgrad_c1_ok(H, W) and not ops.wgrad_c1_ok(dt, 64, H, W, 1, 3, 1, 1)
    x, dy = torch.ones(1, H, W, 64, device=DEV, dtype=tdt), torch.ones(1, H, W, device=DEV)
    bs, slab = arena((2, 9, 64))
    with pytest.raises(RuntimeError, match="eg_wgrad_c1"):
        ops.wgrad_c1(dt, x, dy, slab, 1, H, W, 64)
    torch.cuda.synchronize()
    assert all_nan(bs)

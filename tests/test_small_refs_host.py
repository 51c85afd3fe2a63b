"""Host side of tests/test_gpu_small.py: the float64 restatements of tests/small_refs.py are what torch computes (F.linear, F.conv2d and
their autograd, F.unfold, F.fold); for every GPU case the float32 yardstick is measured (finite and non-zero, which also shows the case
tables consistent without a GPU); each mutant misses float64 by at least ``MUTANT_FACTOR * K`` yardsticks on at least one case of its table
-- so a kernel with that mistake cannot pass the GPU test's bound there; and the launch arithmetic the case tables were chosen for is
pinned, so a launcher change that moves an edge fails here by name."""
import math

import pytest
import torch
import torch.nn.functional as F

import small_refs as R

F64 = torch.float64
TIE = 1e-12


def ok_yard(y):
    return math.isfinite(y) and y > 0.0


# ---- the restatements are torch's semantics -----------------------------------------------------------------------------------------------
def test_dense_restatements_equal_torch_linear_and_its_autograd():
    B, N, Cin, taps = 6, 5, 4, 3
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Cin * taps, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(N, Cin * taps, generator=g, dtype=F64).requires_grad_(True)
    bias = torch.randn(N, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(B, N, generator=g, dtype=F64)
    sigma = torch.tensor(R.SIGMAS, dtype=F64)
    pre = x.detach().clone().requires_grad_(True)                       # the head's input is the LeakyReLU output of the layer before
    y = F.linear(F.leaky_relu(pre, R.SLOPE), w / sigma[0], bias)
    assert R.dist(R.dense_fwd(F.leaky_relu(pre, R.SLOPE).detach(), w.detach(), bias.detach(), sigma, 0), y) < TIE
    y.backward(dy)
    mask = F.leaky_relu(pre, R.SLOPE).detach()
    assert R.dist(R.dense_bwd(dy, w.detach(), mask, "lrelu", sigma, 0), pre.grad) < TIE
    # one sigma per tape of 2 rows
    per = torch.cat([F.linear(x[2 * t:2 * t + 2], w / sigma[t], bias) for t in range(3)])
    assert R.dist(R.dense_fwd(x.detach(), w.detach(), bias.detach(), sigma, 2), per) < TIE
    x.grad = None
    per.backward(dy)
    assert R.dist(R.dense_bwd(dy, w.detach(), None, None, sigma, 2), x.grad) < TIE
    # weight and bias gradient: the panel column k = t*Cin + ci is the master element [n][ci][t]
    master = torch.randn(N, Cin, taps, generator=g, dtype=F64).requires_grad_(True)
    b2 = torch.zeros(N, dtype=F64, requires_grad=True)
    F.linear(x.detach(), master.permute(0, 2, 1).reshape(N, taps * Cin), b2).backward(dy)
    gw0, gb0 = torch.randn(N, Cin, taps, generator=g, dtype=F64), torch.randn(N, generator=g, dtype=F64)
    gw, gb = R.dense_wgrad(dy, x.detach(), gw0, gb0, Cin, taps)
    assert R.dist(gw - gw0, master.grad) < TIE and R.dist(gb - gb0, b2.grad) < TIE
    assert R.dist(R.bgrad(dy, gb0, 1), gb0 + b2.grad) < TIE and R.dist(R.bgrad(dy, gb0, 0), b2.grad) < TIE


def test_head_prep_restatement_equals_autograd_of_a_spectrally_normalised_head():
    """y = x (W / sigma_t)^T + bias per tape: dys = d(loss)/d(x W^T), gb = d(loss)/d(bias), and coef_t = sum dy (x W^T) / sigma_t^2
    is minus d(loss)/d(sigma_t)"""
    rows, rpt, N, Kd = 6, 2, 5, 7
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(rows, Kd, generator=g, dtype=F64), torch.randn(N, Kd, generator=g, dtype=F64)
    bias = torch.randn(N, generator=g, dtype=F64).requires_grad_(True)
    sigma = (0.5 + torch.rand(rows // rpt, generator=g, dtype=F64)).requires_grad_(True)
    dy = torch.randn(rows, N, generator=g, dtype=F64)
    u = (x @ w.t()).requires_grad_(True)
    y = u / sigma.repeat_interleave(rpt)[:, None] + bias
    y.backward(dy)
    gb0 = torch.randn(N, generator=g, dtype=F64)
    dys, coef, gb = R.head_prep(dy, y.detach(), bias.detach(), sigma.detach(), rpt, gb0)
    assert R.dist(dys, u.grad) < TIE and R.dist(gb - gb0, bias.grad) < TIE
    assert R.dist(-coef, sigma.grad) < TIE
    plain = R.head_prep(dy, y.detach(), bias.detach(), None, rpt, gb0)
    assert torch.equal(plain[0], dy) and R.dist(plain[2], gb) < TIE


@pytest.mark.parametrize("geom", [(3, 7, 9, 4, 3, 2, 1), (2, 6, 8, 5, 4, 2, 1), (1, 5, 5, 2, 2, 1, 0)], ids=str)
def test_image_side_restatements_equal_torch_conv2d_unfold_and_autograd(geom):
    CI, H, W, N, k, s, p = geom
    B = 2
    g = torch.Generator().manual_seed(3)
    img = torch.randn(B, CI, H, W, generator=g, dtype=F64)
    w = torch.randn(N, CI, k, k, generator=g, dtype=F64).requires_grad_(True)
    bias, sigma = torch.randn(N, generator=g, dtype=F64), torch.tensor([1.5], dtype=F64)
    z = F.conv2d(img, w, None, s, p)
    want = F.leaky_relu(z / sigma + bias[None, :, None, None], R.SLOPE)
    got = R.conv_img(img, w.detach(), s, p, bias=bias, sigma=sigma, act_name="lrelu")
    assert R.dist(got, want.permute(0, 2, 3, 1)) < TIE
    # the mask: the input gradient through a LeakyReLU whose output is the mask
    OH, OW = R.conv_out(H, W, k, s, p)
    pre = torch.randn(B, OH, OW, N, generator=g, dtype=F64).requires_grad_(True)
    (F.leaky_relu(pre, R.SLOPE) * z.detach().permute(0, 2, 3, 1)).sum().backward()
    assert R.dist(R.conv_img(img, w.detach(), s, p, mask=F.leaky_relu(pre, R.SLOPE).detach(), mask_act="lrelu"), pre.grad) < TIE
    # the weight gradient, per image
    dz = torch.randn(B, OH, OW, N, generator=g, dtype=F64)
    slab = R.conv_img_wgrad(dz, img, k, s, p)
    for b in range(B):
        w.grad = None
        F.conv2d(img[b:b + 1], w, None, s, p).backward(dz[b:b + 1].permute(0, 3, 1, 2))
        assert R.dist(slab[b], w.grad) < TIE
    # the patch rows
    Kp = R.round_up(CI * k * k, 8) + 8
    rows = R.im2col(img, k, s, p, Kp)
    want = F.unfold(img, k, padding=p, stride=s).transpose(1, 2).reshape(B * OH * OW, CI * k * k)
    assert torch.equal(rows[:, :CI * k * k], want) and not bool(rows[:, CI * k * k:].any())


@pytest.mark.parametrize("case", R.COL2IM_CASES + ((3, 2, 4, 5, 3, 1, 1),), ids=str)
def test_col2im_restatement_equals_torch_fold(case):
    C, B, Hin, Win, k, s, p = case
    g = torch.Generator().manual_seed(4)
    cols = torch.randn(B * Hin * Win, k * k * C, generator=g, dtype=F64)
    bias = torch.randn(C, generator=g, dtype=F64)
    OH, OW = (Hin - 1) * s - 2 * p + k, (Win - 1) * s - 2 * p + k
    fin = cols.view(B, Hin * Win, k * k, C).permute(0, 3, 2, 1).reshape(B, C * k * k, Hin * Win)
    want = F.fold(fin, (OH, OW), k, padding=p, stride=s) + bias[None, :, None, None]
    for a, fn in (("none", lambda v: v), ("tanh", torch.tanh), ("sigmoid", torch.sigmoid)):
        assert R.dist(R.col2im(cols, B, C, Hin, Win, k, s, p, bias, a), fn(want)) < TIE
    # and a transposed convolution through its GEMM columns
    x, wt = torch.randn(B, 6, Hin, Win, generator=g, dtype=F64), torch.randn(6, C, k, k, generator=g, dtype=F64)
    gemm = torch.einsum("bihw,icjl->bhwjlc", x, wt).reshape(B * Hin * Win, k * k * C)
    assert R.dist(R.col2im(gemm, B, C, Hin, Win, k, s, p, bias, "none"), F.conv_transpose2d(x, wt, bias, s, p)) < TIE


@pytest.mark.parametrize("name", R.ACT_GRAD_ACTS)
def test_act_grad_bias_restatement_equals_autograd(name):
    B, C, HW = 3, 4, 10
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, C, HW, generator=g, dtype=F64).requires_grad_(True)
    bias = torch.zeros(C, dtype=F64, requires_grad=True)
    a = R.act(z + bias[None, :, None], name)
    gr = torch.randn(B, C, HW, generator=g, dtype=F64)
    a.backward(gr)
    gb0 = torch.randn(C, generator=g, dtype=F64)
    out, gb = R.act_grad_bias(gr, a.detach(), name, gb0, 1)
    assert R.dist(out, z.grad) < TIE and R.dist(gb - gb0, bias.grad) < TIE
    assert R.dist(R.act_grad_bias(gr, a.detach(), name, gb0, 0)[1], bias.grad) < TIE
    ref = {"none": lambda v: v, "lrelu": lambda v: F.leaky_relu(v, R.SLOPE), "tanh": torch.tanh, "sigmoid": torch.sigmoid}[name]
    assert R.dist(R.act(z.detach(), name), ref(z.detach())) < TIE


def test_flat_reduce_and_cast_pad_restatements():
    g = torch.Generator().manual_seed(6)
    slab, g0 = torch.randn(3, 17, generator=g, dtype=F64), torch.randn(17, generator=g, dtype=F64)
    assert R.dist(R.flat_reduce(slab, g0, 1), g0 + slab[0] + slab[1] + slab[2]) < TIE
    assert R.dist(R.flat_reduce(slab, g0, 0), slab[0] + slab[1] + slab[2]) < TIE
    src = torch.randn(5, 3, generator=g)
    for name in R.DTYPES:
        out = R.cast_pad(src, 8, name)
        assert torch.equal(out[:, :3], src.to(R.TORCH_DTYPE[name]).float()) and not bool(out[:, 3:].any()) and out.shape == (5, 8)


@pytest.mark.parametrize("name", R.DTYPES)
def test_wgrad_c1_restatement_equals_autograd_of_conv2d(name):
    B, H, W = 2, 16, 8
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, 64, generator=g, dtype=F64)
    dy = torch.randn(B, H, W, generator=g)
    w = torch.zeros(1, 64, 3, 3, dtype=F64, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), w, None, 1, 1).backward(R.rq(dy, name).to(F64)[:, None])
    slab = R.wgrad_c1(x, dy, name)
    assert slab.shape == (B * H // 8, 9, 64)
    assert R.dist(slab.sum(0), w.grad[0].permute(1, 2, 0).reshape(9, 64)) < TIE


# ---- every GPU case has a yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_head_cases_have_yardsticks(dtype):
    for case in R.DENSE_CASES:
        c = R.dense_case(case, dtype)
        assert ok_yard(c["yard_fwd"]) and ok_yard(c["yard_bwd"]), (case, c["yard_fwd"], c["yard_bwd"])
        assert all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in list(c["fwd"].values()) + list(c["bwd"].values()))
    for case in R.DENSE_WGRAD_CASES:
        assert case[3] * case[4] == case[1] and case[2] <= 32 and case[0] * case[2] * 4 <= 65536
        ygw, ygb = R.dense_wgrad_case(case, dtype)["yard"]                                              # gw and gb, one each
        # one row: gb is gb0 plus one number, an addition float32 may do exactly (a correct kernel does the same one)
        assert ok_yard(ygw) and (ok_yard(ygb) or (ygb == 0.0 and case[0] == 1)), (case, ygw, ygb)
    for case, extra in zip(R.HEAD_PREP_CASES, R.HEAD_PREP_EXTRA):
        rows, rpt, N, npad, col0 = case
        assert rows % rpt == 0 and col0 + N <= npad and N <= 64 and extra in R.HEAD_PREP_VARIANTS
        c = R.head_prep_case(case, dtype)
        assert all(ok_yard(y) for y in c["yard"]["sigma"]) and ok_yard(c["yard32"]["sigma"]), (case, c["yard"])        # dys, coef, gb
        # without sigma dys is dy: in f32 a copy, whose yardstick is zero (the kernel must then give dy's bits)
        yd, yc, yg = c["yard"]["plain"]
        assert ok_yard(yc) and ok_yard(yg) and (ok_yard(yd) if dtype != "f32" else yd == 0.0), (case, c["yard"])
    assert set(R.HEAD_PREP_EXTRA) >= {"no_sigma", "no_coef", "no_gb", "dys32"}


def test_bgrad_and_helper_cases_have_yardsticks():
    for case in R.BGRAD_CASES:
        c = R.bgrad_case(case)
        # one row: a copy (store) or a single addition, which float32 does exactly for this pair -- a correct kernel does the same one
        assert all(ok_yard(c["yard"][acc]) or (case[0] == 1 and c["yard"][acc] == 0.0) for acc in (0, 1)), case
    for case in R.ACT_GRAD_CASES:
        for name in R.ACT_GRAD_ACTS:
            c = R.act_grad_case(case, name)
            for acc in (0, 1):
                yo, yg = c["yard"][acc]
                # without an activation out is g, a copy; gb stored from one element is a copy too: their yardstick is zero
                assert (yo == 0.0) if name == "none" else ok_yard(yo), (case, name, acc, yo)
                assert ok_yard(yg) or (yg == 0.0 and name == "none" and not acc and case[0] * case[2] == 1), (case, name, acc, yg)
    for case in R.FLAT_REDUCE_CASES:
        c = R.flat_reduce_case(case)
        assert ok_yard(c["yard"][1]) and (ok_yard(c["yard"][0]) or case[0] == 1), case
    for case in R.CAST_PAD_CASES:
        assert R.cast_pad(R.cast_pad_src(case), case[2], "bf16").shape == (case[0], case[2])


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_image_side_cases_have_yardsticks(dtype):
    for case in R.CONV_IMG_CASES:
        assert all(ok_yard(y) for y in R.conv_img_case(case, dtype)["yard"].values()), case
    for case in R.CONV_WGRAD_CASES:
        c = R.conv_wgrad_case(case, dtype)
        assert ok_yard(c["yard"]) and c["want"].shape == (R.CONV_WGRAD_B, case[3], case[0], case[4], case[4]), case
    for case in R.COL2IM_CASES:
        c = R.col2im_case(case, dtype)
        assert all(ok_yard(c["yard"][a]) for a in R.COL2IM_ACTS), (case, c["yard"])
    for case in R.WGRAD_C1_CASES:
        assert R.wgrad_c1_ok(case[1], case[2]) and ok_yard(R.wgrad_c1_case(case, dtype)["yard"]), case
    for case in R.IM2COL_CASES + (R.IM2COL_LARGE,):
        B, CI, H, W, k, s, p, Kp = case
        assert Kp >= CI * k * k and Kp % R.VEC[dtype] == 0, case


# ---- the mutants miss ---------------------------------------------------------------------------------------------------------------------
def misses(mutant64, want, yard):
    return R.dist(mutant64, want) >= R.MUTANT_FACTOR * R.K * yard


def assert_some(hits, what):
    print(f"mutant {what}: caught on {[h for h in hits if h[1]]}")
    assert any(h[1] for h in hits), f"mutant {what} stays within the bound on every case: {hits}"


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_forward_mutants_miss(dtype):
    vec = R.VEC[dtype]
    for mutant in ("drop_tail", "double_boundary", "sigma0"):
        hits = []
        for case in R.DENSE_CASES:
            B, q, N = case
            c = R.dense_case(case, dtype)
            ns = R.ns_of(B, c["K"], vec, 16 * B * N, N)
            if mutant == "sigma0" and B != 6:
                continue
            sf = 2 if mutant == "sigma0" else 0
            got = R.dense_fwd(c["x"], c["w"], c["bias"], c["sigma"], sf, mutant=mutant, vec=vec, ns=ns)
            hits.append((case, misses(got, c["fwd"][(True, sf)], c["yard_fwd"])))
        assert_some(hits, mutant)
        if mutant == "drop_tail":                                        # every case whose K is no multiple of a sweep shows it
            assert all(h for (B, q, N), h in hits if q % 256), hits
        if mutant == "double_boundary":                                  # every case with a K split shows it
            assert all(h for case, h in hits if R.DENSE_LAUNCH[case][0] > 1), hits


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_backward_and_gradient_mutants_miss(dtype):
    hits = []
    for case in R.DENSE_CASES:
        c = R.dense_case(case, dtype)
        hits.append((case, misses(R.dense_bwd(c["dy"], c["w"], None, None, c["sigma"], 0, mutant="mul_sigma"), c["bwd"][(None, 0)], c["yard_bwd"])))
    assert_some(hits, "mul_sigma")
    assert all(h for _, h in hits), hits
    for mutant in ("k_ci_major", "store"):
        hits = []
        for case in R.DENSE_WGRAD_CASES:
            c = R.dense_wgrad_case(case, dtype)
            got = R.dense_wgrad(c["dy"], c["x"], c["gw0"], c["gb0"], case[3], case[4], mutant=mutant)
            hits.append((case, R.dist(got[0], c["want"][0]) >= R.MUTANT_FACTOR * R.K * c["yard"][0]))
        assert_some(hits, mutant)
        if mutant == "store":
            assert all(h for _, h in hits), hits
    hits = []
    for case, extra in zip(R.HEAD_PREP_CASES, R.HEAD_PREP_EXTRA):
        c = R.head_prep_case(case, dtype)
        got = R.head_prep(c["dy"], c["y"], c["bias"], c["sigma"], case[1], c["gb0"], mutant="lane_tail")
        hits.append((case, R.dist(got[2], c["want"]["sigma"][2]) >= R.MUTANT_FACTOR * R.K * c["yard"]["sigma"][2]))       # gb's own yardstick
    assert_some(hits, "lane_tail")


def test_bgrad_and_helper_mutants_miss():
    hits = [(case, misses(R.bgrad(R.bgrad_case(case)["dy"], R.bgrad_case(case)["gb0"], 1, mutant="full_strides"), R.bgrad_case(case)["want"][1],
                          R.bgrad_case(case)["yard"][1])) for case in R.BGRAD_CASES]
    assert_some(hits, "full_strides")
    hits = []
    for case in R.ACT_GRAD_CASES:
        for name in ("tanh", "sigmoid"):
            c = R.act_grad_case(case, name)
            got = R.act_grad_bias(c["g"], c["a"], name, c["gb0"], 1, mutant="grad_of_input")
            hits.append(((case, name), R.dist(got[0], c["want"][1][0]) >= R.MUTANT_FACTOR * R.K * c["yard"][1][0]))
    assert_some(hits, "grad_of_input")
    hits = [(case, misses(R.flat_reduce(R.flat_reduce_case(case)["slab"], R.flat_reduce_case(case)["g0"], 1, mutant="last_slab"),
                          R.flat_reduce_case(case)["want"][1], R.flat_reduce_case(case)["yard"][1])) for case in R.FLAT_REDUCE_CASES]
    assert_some(hits, "last_slab")
    hits = [(case, not torch.equal(R.cast_pad(R.cast_pad_src(case), case[2], "f32", mutant="padded_stride"), R.cast_pad(R.cast_pad_src(case), case[2], "f32")))
            for case in R.CAST_PAD_CASES]
    assert_some(hits, "padded_stride")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_image_side_mutants_miss(dtype):
    for mutant, ep in (("swap_khkw", "plain"), ("bias_before_sigma", "bias_sigma_lrelu")):
        hits = []
        for case in R.CONV_IMG_CASES:
            c = R.conv_img_case(case, dtype)
            got = R.conv_img(c["img"], c["w"], case[6], case[7], mutant=mutant, **R.conv_img_epilogue(c, ep))
            hits.append((case, misses(got, c["want"][ep], c["yard"][ep])))
        assert_some(hits, f"conv_img {mutant}")
    hits = []
    for case in R.CONV_WGRAD_CASES:
        c = R.conv_wgrad_case(case, dtype)
        hits.append((case, R.worst(R.conv_img_wgrad(c["dz"], c["img"], case[4], case[5], case[6], mutant="swap_khkw"), c["want"]) >= R.MUTANT_FACTOR * R.K * c["yard"]))
    assert_some(hits, "conv_img_wgrad swap_khkw")
    assert all(h for _, h in hits), hits
    hits = []
    for case in R.IM2COL_CASES:
        img = R.im2col_img(case)
        hits.append((case, not torch.equal(R.im2col(img, *case[4:], mutant="swap_khkw"), R.im2col(img, *case[4:]))))
    assert all(h for _, h in hits), hits
    hits = []
    for case in R.COL2IM_CASES:
        c = R.col2im_case(case, dtype)
        C, B, Hin, Win, k, s, p = case
        hits.append((case, misses(R.col2im(c["cols"], B, C, Hin, Win, k, s, p, c["bias"], "none", mutant="tap_parity"), c["want"]["none"], c["yard"]["none"])))
    assert_some(hits, "tap_parity")
    hits = []
    for case in R.WGRAD_C1_CASES:
        c = R.wgrad_c1_case(case, dtype)
        hits.append((case, misses(R.wgrad_c1(c["x"], c["dy"], dtype, mutant="flip_taps"), c["want"], c["yard"])))
    assert_some(hits, "flip_taps")
    assert all(h for _, h in hits), hits


# ---- the launch arithmetic the cases were chosen for ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dense_head_launch_arithmetic(dtype):
    vec = R.VEC[dtype]
    for case, (ns, kblocks, gy) in R.DENSE_LAUNCH.items():
        B, q, N = case
        Kd = q * vec
        assert R.ns_of(B, Kd, vec, 0, N) == 1
        assert R.ns_of(B, Kd, vec, 16 * B * N, N) == ns, f"{case}: the K split of the forward moved"
        assert R.kblocks_of(Kd, vec) == kblocks and R.gy_of(B, Kd, vec) == gy, f"{case}: the K grid of the backward moved"
    B, q, N = R.DENSE_CLIPPED
    assert R.ns_of(B, q * vec, vec, 2 * B * N, N) == 2, "the clipped workspace no longer gives two slices"
    assert R.kper_of(513 * vec, vec, 2) == 257 * vec and 513 * vec - 257 * vec == 256 * vec          # slices of unequal length
    assert R.kper_of(2051 * vec, vec, 8) == 257 * vec and 2051 - 7 * 257 == 252                      # a short last slice
    assert R.kper_of(512 * vec, vec, 2) == 256 * vec                                                 # exact halves
    assert R.cdiv(130, R.DS_ROWS) == 33 and R.cdiv(5, R.DS_ROWS) == 2 and 5 % R.DS_ROWS == 1
    # (6, 513, 19) backward: two workgroups along K over three blocks of 256 vectors: the first one takes a second pass
    assert R.kblocks_of(513 * vec, vec) > R.gy_of(6, 513 * vec, vec)
    assert {v[0] for v in R.DENSE_LAUNCH.values()} == {1, 2, 4, 8} and {v[2] for v in R.DENSE_LAUNCH.values()} == {1, 2, 4, 8}


def test_image_side_launch_arithmetic():
    for case, cpt in R.CONV_IMG_CASES.items():
        B, CI, H, W, N, k, s, p = case
        assert R.cpt_of(H, W, N, k, s, p) == cpt, f"{case}: channels per thread moved"
        assert (CI * k * k * N + CI * k * (W + 2 * p)) * 4 <= 65536
    assert set(R.CONV_IMG_CASES.values()) == {1, 2, 4, 8, 16}
    for case in R.CONV_IMG_REFUSED:
        assert R.cpt_of(*case[2:]) is None, case
    assert R.conv_out(4, 4, 4, 1, 0) == (1, 1) and R.conv_out(12, 16, 4, 2, 1) == (6, 8) and R.conv_out(5, 8, 3, 1, 1) == (5, 8)
    assert R.conv_out(32, 32, 3, 2, 1) == (16, 16)                       # floor((32 + 2 - 3) / 2) + 1
    assert 256 // R.conv_out(6, 8, 3, 1, 1)[1] == 32 > 4 and 256 // R.conv_out(5, 8, 3, 1, 1)[1] == 32
    for case, maxt in R.CONV_WGRAD_CASES.items():
        CI, H, W, N, k, s, p = case
        assert R.maxt_of(CI, N, k) == maxt, f"{case}: taps per thread moved"
        assert R.wgrad_lds_bytes(CI, H, W, p) <= 65536
    assert {R.maxt_bucket(m) for m in R.CONV_WGRAD_CASES.values()} == {1, 2, 3, 6, 12, 24}
    assert R.maxt_bucket(5) == 6 and R.maxt_bucket(9) == 12 and R.maxt_bucket(16) == 24 and R.maxt_bucket(18) == 24
    assert R.wgrad_lds_bytes(3, 64, 64, 1) == 52272
    (a, b) = R.CONV_WGRAD_REFUSED
    assert R.maxt_of(a[0], a[3], a[4]) == 32 and R.maxt_bucket(32) is None
    assert R.wgrad_lds_bytes(b[0], b[1], b[2], b[6]) == 69696 > 65536
    assert [R.im2col_template(c[4]) for c in R.IM2COL_CASES] == [3, 0, 0] and R.im2col_template(R.IM2COL_LARGE[4]) == 4
    total, blocks = R.im2col_blocks(*R.IM2COL_LARGE, 4)
    assert total == 2113536 and blocks == 8192 and total > blocks * 256
    for case in R.IM2COL_CASES:
        assert all(R.im2col_blocks(*case, R.VEC[dt])[1] < 8192 for dt in R.DTYPES)
    assert all(not R.wgrad_c1_ok(H, W) for H, W in R.WGRAD_C1_REFUSED)
    B, Kd, N, _, _ = R.DENSE_WGRAD_CASES[-1]
    assert B * N * 4 == 65536

"""Host side of tests/test_gpu_conv.py.  Without a GPU: the convolution entry points refuse what they cannot run, through the queries that
cannot launch (and through the launch entry points only in the style of test_argument_errors_do_not_abort: refused before anything is
enqueued); the launch arithmetic restated in tests/conv_refs.py is what the library's queries answer; every NT launch of the tables reaches
the kernel it is meant for (eg_igemm_nt_tile_ep); the integer operand sets stay within 256 and are exact in the storage dtype; the float64
restatements are torch.nn.functional and its autograd; and each mutant misses float64 by at least ``MUTANT_FACTOR * K`` yardsticks on at
least one case of its table -- the H / W swap on the non-square cases ONLY: on every square case it is the identity, which is why the square
suite could not see such a kernel."""
import ctypes
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

import conv_refs as R

F64 = torch.float64
TIE = 1e-12
DT = {"f32": 0, "bf16": 1, "f16": 2}
FAKE = 4096                     # a non-null, aligned address that is never dereferenced: nothing here launches


def _pkg():
    return importlib.import_module("ead-gan_amd")


def conv(case):
    return _pkg().ops.make_conv(*case)


def query(name, *args):
    return _pkg()._lib.lib().query(name, *args)


def ep_of(**kw):
    e = _pkg()._lib.EgEpilogue()
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def launch_ep(l, dtype):
    """the eg_epilogue of a table launch as far as the planner reads it: hints, output mode, split-K scratch"""
    c = conv(l.case)
    nbytes = {None: 0, "query": query("eg_conv_splitk_ws_bytes", ctypes.byref(c), DT[dtype], int(l.bwd))}.get(l.ws)
    if nbytes is None:
        nbytes = R.scratch_bytes(l)
    return ep_of(nt_variant=l.variant, nt_splitk=l.splitk, out_mode=int(bool(R.EPS[l.ep].get("nchw"))),
                 splitk_ws=FAKE if nbytes else None, splitk_ws_bytes=nbytes)


def answers(c, dt, ep=None):
    """every query that cannot launch, on one convolution"""
    p = None if c is None else ctypes.byref(c)
    e = ctypes.byref(ep if ep is not None else ep_of())
    return dict(tile=[query("eg_igemm_nt_tile", p, dt, b, v, 0) for b in (0, 1) for v in (R.NT_AUTO, R.NT_REG)],
                tile_ep=[query("eg_igemm_nt_tile_ep", p, dt, b, e) for b in (0, 1)],
                stat=[query("eg_conv_stat_blocks", p, dt, b, e) for b in (0, 1)],
                splitk=[query("eg_conv_splitk_ws_bytes", p, dt, b) for b in (0, 1)],
                variant=query("eg_conv_wgrad_variant", p, dt), wgrad_ws=query("eg_conv_wgrad_ws_bytes", p, dt))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
REFUSED = {"zero Cin": (2, 4, 4, 0, 8, 3, 1, 1, 0), "zero Cout": (2, 4, 4, 8, 0, 3, 1, 1, 0), "negative Cin": (2, 4, 4, -8, 8, 3, 1, 1, 0),
           "zero H": (2, 0, 4, 8, 8, 1, 1, 0, 0), "zero W": (2, 4, 0, 8, 8, 1, 1, 0, 0), "zero B": (0, 4, 4, 8, 8, 1, 1, 0, 0),
           "2^32 rows": (1 << 20, 64, 64, 8, 8, 1, 1, 0, 0), "2^31 rows": (1 << 19, 64, 64, 8, 8, 1, 1, 0, 0),
           "ragged extent": (2, 12, 12, 8, 8, 4, 2, 1, 0), "up = 2": (2, 4, 4, 8, 8, 3, 1, 1, 2)}


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_refused_convolutions_answer_minus_one_and_zero(dtype):
    dt = DT[dtype]
    for what, case in list(REFUSED.items()) + [("null", None)]:
        a = answers(None if case is None else conv(case), dt)
        assert set(a["tile"]) == {-1} and set(a["tile_ep"]) == {-1} and a["variant"] == -1, (what, a)
        assert set(a["stat"]) == {0} and set(a["splitk"]) == {0} and a["wgrad_ws"] == 0, (what, a)
        if case is not None:
            assert not R.conv_ok(case, dtype), what
    good = (2, 8, 8, 8, 8, 4, 2, 1, 0)
    a = answers(conv(good), dt)
    assert min(a["tile"]) > 0 and min(a["tile_ep"]) > 0 and a["variant"] == 1 and a["wgrad_ws"] > 0, a
    assert query("eg_igemm_nt_tile", ctypes.byref(conv(good)), 7, 0, 0, 0) == -1 and query("eg_conv_wgrad_ws_bytes", ctypes.byref(conv(good)), 7) == 0


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_backward_data_refuses_a_stride_above_k(dtype):
    """k = 1, stride 2 leaves three of the four sub-pixel phases without a tap: the forward pass and the weight gradient run, the
    backward-data pass is refused"""
    case = (2, 8, 8, 8, 8, 1, 2, 0, 0)
    assert R.conv_ok(case, dtype) and not R.bwd_ok(case, dtype) and 0 in R.bwd_taps(case)
    a = answers(conv(case), DT[dtype])
    assert a["tile"][:2] == [128016, 128016] and a["tile"][2:] == [-1, -1] and a["tile_ep"][0] > 0 and a["tile_ep"][1] == -1, a
    assert a["stat"][1] == 0 and a["splitk"][1] == 0 and a["variant"] == 1 and a["wgrad_ws"] == R.wgrad_ws_bytes(case, dtype) > 0


BAD_EPILOGUES = (dict(act=5), dict(act=-1), dict(mask_act=5), dict(mask_act=-2), dict(out_mode=2), dict(out_mode=-1), dict(bias_mod=-1),
                 dict(sigma_rows=-1), dict(stat_mode=1, stat_act=7, stat_out=FAKE))


def test_epilogue_fields_outside_their_contract_are_refused():
    c = conv((4, 16, 16, 64, 128, 4, 2, 1, 0))
    assert min(answers(c, 1)["tile_ep"]) > 0
    for bad in BAD_EPILOGUES:
        a = answers(c, 1, ep_of(**bad))
        assert set(a["tile_ep"]) == {-1} and set(a["stat"]) == {0}, (bad, a)
    for fine in (dict(act=4, mask_act=4, out_mode=1, bias_mod=3, sigma_rows=5), dict(stat_act=7)):       # stat_act is read with a stat_mode only
        assert min(answers(c, 1, ep_of(**fine))["tile_ep"]) > 0, fine


def test_launch_entry_points_refuse_before_anything_runs():
    lib = _pkg()._lib.lib()
    one, ns = ctypes.c_void_p(FAKE), ctypes.c_int(0)
    good = conv((2, 8, 8, 8, 8, 4, 2, 1, 0))
    for what, match in (("zero Cin", "positive"), ("zero Cout", "positive"), ("zero H", "positive"), ("2^31 rows", "2\\^31"), ("zero B", "bad field")):
        c = conv(REFUSED[what])
        for name in ("eg_conv_fwd", "eg_conv_bwd_data"):
            with pytest.raises(RuntimeError, match=match):
                lib.call(name, ctypes.byref(c), 0, one, one, one, None, None)
        with pytest.raises(RuntimeError, match=match):
            lib.call("eg_conv_wgrad", ctypes.byref(c), 0, one, one, one, ctypes.addressof(ns), 0, None)
    with pytest.raises(RuntimeError, match="k >= stride"):
        lib.call("eg_conv_bwd_data", ctypes.byref(conv((2, 8, 8, 8, 8, 1, 2, 0, 0))), 0, one, one, one, None, None)
    for bad, match in ((dict(act=5), "act"), (dict(mask_act=-2), "mask_act"), (dict(out_mode=2), "out_mode"), (dict(bias_mod=-1), "negative"),
                       (dict(sigma_rows=-1), "negative")):
        for name in ("eg_conv_fwd", "eg_conv_bwd_data"):
            with pytest.raises(RuntimeError, match=match):
                lib.call(name, ctypes.byref(good), 0, one, one, one, ctypes.byref(ep_of(**bad)), None)


# ---- the restated arithmetic is the library's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_restated_arithmetic_equals_the_queries(dtype):
    dt = DT[dtype]
    assert R.kpad_of(0, dtype) == R.BK[dtype] == R.kpad_of(R.BK[dtype], dtype) and R.kpad_of(R.BK[dtype] + 1, dtype) == 2 * R.BK[dtype]
    assert R.bwd_taps((2, 8, 16, 16, 24, 3, 2, 1, 0)) == [1, 2, 2, 4] and R.bwd_taps((1, 8, 8, 8, 8, 4, 2, 1, 0)) == [4, 4, 4, 4]
    assert R.bwd_taps((1, 8, 8, 8, 8, 2, 2, 0, 0)) == [1, 1, 1, 1] and R.bwd_taps((1, 8, 8, 8, 8, 3, 1, 1, 0)) == [9]
    for case in R.all_conv_cases(dtype):
        c = ctypes.byref(conv(case))
        assert query("eg_pack_fwd_elems", c, dt) == R.pack_fwd_elems(case, dtype), case
        assert query("eg_pack_bwd_elems", c, dt) == R.pack_bwd_elems(case, dtype), case
        for bwd in (0, 1):
            ok = R.bwd_ok(case, dtype) if bwd else R.conv_ok(case, dtype, need_cout=False)
            assert (query("eg_igemm_nt_tile", c, dt, bwd, R.NT_REG, 0) > 0) == ok, (case, bwd)
        assert query("eg_conv_wgrad_variant", c, dt) == R.wgrad_variant(case, dtype), case
        assert query("eg_conv_wgrad_ws_bytes", c, dt) == R.wgrad_ws_bytes(case, dtype), case


def test_weight_gradient_plans_are_the_ones_the_tables_were_chosen_for():
    nine = {R.tn_tiles(c) for c, _ in R.TN_CASES[:9]}
    assert nine == {(a, b) for a in (32, 64, 128) for b in (32, 64, 128)}
    assert R.tn_tiles((2, 4, 8, 24, 40, 3, 1, 1, 0)) == (64, 32) and R.tn_tiles((2, 4, 8, 72, 40, 3, 1, 1, 0)) == (64, 64)
    for case, rows in R.TN_ROWS.items():
        for dtype in R.DTYPES:
            variant, splits = R.wgrad_splits(case, dtype)
            assert variant == 1 and tuple(b - a for a, b in splits) == rows, (case, splits)
    assert R.tn_rows_per_step((209, 2, 2, 64, 128, 1, 1, 0, 0), "bf16") == 64 and R.tn_rows_per_step((209, 2, 2, 64, 128, 1, 1, 0, 0), "f32") == 32
    assert R.tn_rows_per_step((209, 2, 2, 24, 40, 3, 1, 1, 0), "f16") == 32
    for dtype in R.SIXTEEN:
        for case, targets, (ch, rows) in R.TN8_CASES:
            plan = R.tn8_plan(case, dtype)
            assert plan and plan["ch"] == ch and tuple(b - a for a, b in R.wgrad_splits(case, dtype)[1]) == rows, (case, plan)
            assert query("eg_conv_wgrad_variant", ctypes.byref(conv(case)), DT[dtype]) == 2
            for t in targets:
                assert R.tn8_plan(case, dtype, t)["nsplit"] <= plan["nsplit"], (case, t)
        assert [R.tn8_plan((128, 8, 8, 96, 96, 4, 2, 1, 0), dtype, t)["nsplit"] for t in (0, 128, 1, 1000)] == [8, 4, 1, 8]
        assert [R.tn8_plan((36, 8, 8, 128, 128, 4, 2, 1, 0), dtype, t)["nsplit"] for t in (0, 128, 1)] == [2, 2, 1]
        assert [R.tn8_plan(c, dtype)["nimg"] for c in ((8, 4, 16, 32, 32, 4, 2, 1, 0), (2, 32, 8, 64, 64, 4, 2, 1, 0))] == [4, 1]
        # the widest row, OW = 64: 130 patch pixels are 33 pieces of 4 at 128 channels, and 9 pieces of 16 (144 slots of 136) at 32
        assert R.tn8_plan((2, 2, 128, 128, 128, 4, 2, 1, 0), dtype) and R.tn8_plan(R.TN8_REFUSED, dtype) is None
        assert query("eg_conv_wgrad_variant", ctypes.byref(conv(R.TN8_REFUSED)), DT[dtype]) == 1
        for c in R.TN8_SMALL_REFUSED:
            assert R.tn8_plan(c, dtype) is None and query("eg_conv_wgrad_variant", ctypes.byref(conv(c)), DT[dtype]) == 1, c
    assert R.tn8_plan((16, 4, 4, 32, 32, 4, 2, 1, 0), "f32") is None


# ---- every NT launch of the tables reaches its kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_nt_launches_reach_the_kernels_they_are_meant_for(dtype):
    dt = DT[dtype]
    seen = set()
    for group, launches in R.nt_groups(dtype).items():
        assert launches, group
        for l in launches:
            label = query("eg_igemm_nt_tile_ep", ctypes.byref(conv(l.case)), dt, int(l.bwd), ctypes.byref(launch_ep(l, dtype)))
            assert label > 0 and (l.label is None or label == l.label), (group, l, label)
            seen.add(label)
    assert seen >= {128016, 128032, 128064, 128128, 128131, 128132, 128135, 256147, 256148, 256149, 256150, 128151, 128152}, sorted(seen)
    assert query("eg_igemm_nt_tile", ctypes.byref(conv(R.s8p_refused_case(dtype))), dt, 0, R.NT_S8P, 0) == -1
    assert query("eg_igemm_nt_tile", ctypes.byref(conv(R.s8p_refused_case(dtype))), dt, 0, R.NT_S8, 0) == 256147


def test_the_tables_hold_the_edges_of_the_issue():
    for dtype in R.DTYPES:
        G = R.nt_groups(dtype)
        rows = {g: R.rows_of(ls[0].case) for g, ls in G.items()}
        assert (rows["one_element"], rows["cols_19_m96"], rows["cols_160_m320"], rows["ragged_132"], rows["ragged_260"]) == (1, 96, 320, 132, 260)
        assert (rows["ragged_136_4x8"], rows["ragged_264_4x8"], rows["split_5_tiles_in_4"], rows["reg_split_32"]) == (136, 264, 130, 32)
        assert R.cdiv(rows["pers_second_round"], 128) * 2 == 514 and rows["pers_second_round"] % 128 == 64
        assert rows["s8p_4px"] == 280 and R.geom(G["s8p_16x32"][0].case)[2:] == (16, 32) and R.geom(G["s8p_4x64"][0].case)[2:] == (4, 64)
        assert R.ep_operands(G["epilogues"][0].case, False, "tapes", dtype, "rand")["sigma_rows"] == 64
        assert {l.case[5] * l.case[5] * l.case[3] // R.BK[dtype] for g in ("kloop_1", "kloop_2", "kloop_3", "kloop_4", "kloop_16") for l in G[g]} == {1, 2, 3, 4, 16}
        assert any(c[1] != c[2] for c in R.all_conv_cases(dtype)) and any(c[1] == c[2] for c in R.all_conv_cases(dtype))


# ---- the integer sets are exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_integer_operand_sets_stay_exact(dtype):
    worst = 0.0
    for case, bwd, ep in R.nt_cases(dtype):
        if not R.ep_exact(ep):
            continue
        want, yard = R.nt_ref(case, bwd, ep, dtype, "int")
        m = float(want.abs().max())
        worst = max(worst, m)
        assert yard == 0.0 and m <= R.INT_BOUND, (case, bwd, ep, m)
        assert torch.equal(R.stored(want, "f32" if R.EPS[ep].get("nchw") else dtype).double(), want), (case, bwd, ep)
    for case, dts in R.TN_CASES:
        if dtype in dts:
            assert float(R.wgrad_ref(case, dtype, "int")[1].abs().max()) <= R.INT_BOUND, case
    if dtype != "f32":
        for case, targets, _ in R.TN8_CASES:
            for t in targets:
                assert float(R.wgrad_ref(case, dtype, "int", t)[1].abs().max()) <= R.INT_BOUND, case
    print(f"CONV int {dtype}: largest NT result {worst:g}")
    assert worst > 8


# ---- the restatements are torch's semantics -----------------------------------------------------------------------------------------------
TORCH_CASES = ((2, 4, 8, 3, 4, 3, 1, 1, 0), (2, 8, 4, 3, 4, 4, 2, 1, 0), (2, 4, 8, 3, 4, 3, 1, 1, 1), (2, 8, 16, 3, 4, 3, 2, 1, 0),
               (3, 4, 4, 2, 4, 4, 1, 0, 0), (2, 4, 2, 3, 4, 1, 1, 0, 0), (2, 4, 8, 3, 4, 2, 2, 0, 0), (1, 8, 4, 2, 4, 4, 2, 1, 1))


@pytest.mark.parametrize("case", TORCH_CASES, ids=str)
def test_restatements_equal_torch_conv2d_and_its_autograd(case):
    B, H, W, Cin, Cout, k, s, p, up = case
    XH, XW, OH, OW = R.geom(case)
    g = torch.Generator().manual_seed(R.seed_of(case))
    x = torch.randn(B, H, W, Cin, generator=g, dtype=F64)
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(B, OH, OW, Cout, generator=g, dtype=F64)
    xu = x.permute(0, 3, 1, 2)
    xu = (F.interpolate(xu, scale_factor=2, mode="nearest") if up else xu).clone().requires_grad_(True)
    y = F.conv2d(xu, w, None, s, p)
    assert y.shape == (B, Cout, OH, OW)
    assert R.dist(R.conv_fwd(x, w.detach(), case), y.permute(0, 2, 3, 1).reshape(-1, Cout)) < TIE
    y.backward(dy.permute(0, 3, 1, 2))
    assert R.dist(R.conv_bwd_data(dy, w.detach(), case), xu.grad.permute(0, 2, 3, 1).reshape(-1, Cin)) < TIE
    M = B * OH * OW
    for splits in ([(0, M)], [(0, M // 3), (M // 3, M - 1), (M - 1, M)]):
        slab = R.wgrad_slab(x, dy, case, splits)
        assert slab.shape == (len(splits), Cout, k * k, Cin)
        assert R.dist(slab.sum(0).view(Cout, k, k, Cin).permute(0, 3, 1, 2), w.grad) < TIE
    if R.bwd_ok(case, "f32"):
        assert R.dist(R.conv_bwd_data(dy, w.detach(), case), F.conv_transpose2d(dy.permute(0, 3, 1, 2), w.detach(), None, s, p, XH - ((OH - 1) * s - 2 * p + k)).permute(0, 2, 3, 1).reshape(-1, Cin)) < TIE


@pytest.mark.parametrize("case", [c for c in TORCH_CASES if R.bwd_ok(c, "f32")], ids=str)
def test_backward_panels_walked_phase_by_phase_are_the_transposed_convolution(case):
    """the layout of panels_bwd and the phases' offsets, as the kernels use them: lattice pixel (ly, lx) of phase (ry, rx) is output pixel
    (ly * s + ry, lx * s + rx) and reads dY at (ly + d0y - ty, lx + d0x - tx) for tap (ty, tx), zero outside"""
    B, H, W, Cin, Cout, k, s, p, up = case
    XH, XW, OH, OW = R.geom(case)
    g = torch.Generator().manual_seed(R.seed_of(case, "panels"))
    w = torch.randn(Cout, Cin, k, k, generator=g)
    dy = torch.randn(B, OH, OW, Cout, generator=g, dtype=F64)
    flat, off = R.panels_bwd(w, case, "f32").double(), 0
    assert flat.numel() == R.pack_bwd_elems(case, "f32")
    dx = torch.full((B, XH, XW, Cin), float("nan"), dtype=F64)
    pad = k
    dyp = F.pad(dy, (0, 0, pad, pad, pad, pad))
    for ry, rx, (_, TH, d0y), (_, TW, d0x) in R.bwd_phases(case):
        Kd, Kpad = TH * TW * Cout, R.kpad_of(TH * TW * Cout, "f32")
        pan = flat[off:off + Cin * Kpad].view(Cin, Kpad)
        off += Cin * Kpad
        assert not bool(pan[:, Kd:].any())
        rows = torch.cat([dyp[:, pad + d0y - ty:pad + d0y - ty + OH, pad + d0x - tx:pad + d0x - tx + OW] for ty in range(TH) for tx in range(TW)], 3)
        dx[:, ry::s, rx::s] = rows @ pan[:, :Kd].t()
    assert off == flat.numel()
    assert R.dist(dx.reshape(-1, Cin), R.conv_bwd_data(dy, w.double(), case)) < TIE


def test_forward_panel_and_epilogue_element_by_element():
    case = (1, 2, 2, 3, 2, 2, 1, 0, 0)
    w = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).view(2, 3, 2, 2)
    pan = R.panels_fwd(w, case, "f32")
    assert pan.shape == (2, 32) and R.pack_fwd_elems(case, "f32") == 64 and not bool(pan[:, 12:].any())
    for n in range(2):
        for ty in range(2):
            for tx in range(2):
                for c in range(3):
                    assert pan[n, (ty * 2 + tx) * 3 + c] == w[n, c, ty, tx]
    assert bool(torch.isnan(R.panels_fwd(w, case, "f32", mutant="pad_unwritten")[:, 12:]).all())
    g = torch.Generator().manual_seed(3)
    acc, mask = torch.randn(6, 5, generator=g, dtype=F64), torch.randn(6, 5, generator=g, dtype=F64)
    e = dict(sigma=torch.tensor([2.0, 0.5, 4.0]), sigma_rows=2, bias=torch.tensor([1.0, -2.0, 3.0, 9.0, 9.0]), bias_mod=3, act="lrelu", slope=0.2,
             mask=mask, mask_act="relu", mask_slope=0.0)
    rows = torch.tensor([4, 5, 0, 1, 2, 3])                  # any order: the tape comes from the lattice row, not from the position
    got = R.epilogue(acc, rows, e)
    for i in range(6):
        for n in range(5):
            v = float(acc[i, n]) / float(e["sigma"][int(rows[i]) // 2]) + float(e["bias"][n % 3])
            v = v if v > 0 else 0.2 * v
            assert abs(float(got[i, n]) - (v if mask[i, n] > 0 else 0.0)) < 1e-12
    assert R.to_nchw(torch.arange(2 * 2 * 4 * 3.0).view(-1, 3), (2, 2, 4, 3, 3, 1, 1, 0, 0), False)[1, 2, 1, 3] == ((1 * 2 + 1) * 4 + 3) * 3 + 2
    assert torch.equal(R.lattice_rows((1, 2, 4, 8, 8, 4, 2, 1, 0), True).view(2, 4), torch.tensor([[0, 0, 1, 1], [0, 0, 1, 1]]))


# ---- the mutants miss ---------------------------------------------------------------------------------------------------------------------
def misses(got, want, yard):
    return bool(torch.isnan(got).any()) or R.dist(got, want) >= R.MUTANT_FACTOR * R.K * yard


def plain_cases(dtype, bwd):
    return [c for c, b, ep in R.nt_cases(dtype) if b == bwd and ep == "plain"]


def square(case):
    return case[1] == case[2]


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_gather_mutants_miss_and_the_hw_swap_passes_every_square_case(dtype):
    for mutant in ("swap_hw", "swap_tap", "clamp_border", "up_last", "drop_last_ktile"):
        hits = {}
        for case in plain_cases(dtype, False):
            o = R.operands(case, dtype, "rand")
            want, yard = R.nt_ref(case, False, "plain", dtype, "rand")
            hits[case] = misses(R.conv_fwd(o["x"], o["wr"], case, mutant=mutant, cdt=dtype), want, yard)
            if mutant == "swap_hw" and square(case):
                assert torch.equal(R.conv_fwd(o["x"], o["wr"], case, mutant=mutant), want), case
        assert any(hits.values()), mutant
        if mutant == "swap_hw":
            assert not any(h for c, h in hits.items() if square(c)) and all(h for c, h in hits.items() if not square(c) and min(c[1], c[2]) > 1), hits
    for mutant in ("swap_hw", "swap_tap", "swap_oo"):
        hits = {}
        for case in plain_cases(dtype, True):
            o = R.operands(case, dtype, "rand")
            want, yard = R.nt_ref(case, True, "plain", dtype, "rand")
            hits[case] = misses(R.conv_bwd_data(o["dy"], o["wr"], case, mutant=mutant), want, yard)
        assert any(hits.values()), mutant
        if mutant == "swap_hw":
            assert not any(h for c, h in hits.items() if R.geom(c)[2] == R.geom(c)[3]), hits
        if mutant == "swap_oo":
            assert all(h for c, h in hits.items() if c[6] == 2), hits


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_epilogue_mutants_miss(dtype):
    case = R.nt_groups(dtype)["epilogues"][0].case
    rows = R.lattice_rows(case, False)
    o = R.operands(case, dtype, "rand")
    acc = R.conv_fwd(o["x"], o["wr"], case)
    for mutant, eps in (("bias_before_sigma", ("full",)), ("tape_tile_first", ("tapes", "full")), ("ignore_bias_mod", ("bias_mod",)),
                        ("mask_wrong_sign", ("mask_lrelu", "mask_relu", "full"))):
        for ep in eps:
            want, yard = R.nt_ref(case, False, ep, dtype, "rand")
            assert misses(R.epilogue(acc, rows, R.ep_operands(case, False, ep, dtype, "rand"), mutant=mutant), want, yard), (mutant, ep)
            # ... and the integer set shows it as a plain inequality
            wi, _ = R.nt_ref(case, False, ep, dtype, "int")
            oi = R.operands(case, dtype, "int")
            assert not torch.equal(R.epilogue(R.conv_fwd(oi["x"], oi["wr"], case), rows, R.ep_operands(case, False, ep, dtype, "int"), mutant=mutant), wi), (mutant, ep)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_weight_gradient_mutants_miss(dtype):
    cases = [(c, 0) for c, dts in R.TN_CASES if dtype in dts] + ([(c, 0) for c, _, _ in R.TN8_CASES] if dtype != "f32" else [])
    for mutant in ("swap_hw", "swap_tap", "clamp_border", "up_last", "drop_first_row", "double_last_row", "transpose_tc"):
        hits = {}
        for case, t in cases:
            if mutant in ("drop_first_row", "double_last_row") and R.rows_of(case) > 1024:
                continue                                    # (one row in 2048 is below the bound by design: the short cases carry these two)
            o = R.operands(case, dtype, "rand")
            _, want, yard = R.wgrad_ref(case, dtype, "rand", t)
            hits[case] = misses(R.wgrad_slab(o["x"], o["dy"], case, R.wgrad_splits(case, dtype, t)[1], mutant=mutant), want, yard)
        assert any(hits.values()), mutant
        if mutant == "swap_hw":
            assert not any(h for c, h in hits.items() if square(c)) and any(h for c, h in hits.items() if not square(c)), hits
        if mutant == "transpose_tc":
            assert all(h for c, h in hits.items() if c[5] > 1), hits


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_a_partial_tile_rounded_to_the_compute_dtype(dtype):
    """The mutant the K = 8 rule cannot see behind a 16-bit store: a split's partial tile passed through 16 bits costs about 2^-9, the
    store of the result costs the same, and the yardstick IS that store.  It is measured here against the value before the store (fp32,
    where a kernel that keeps its partial tiles in fp32 is within the float32 yardstick) and must miss that by the mutants' factor; in f32
    the mutant is the identity."""
    figs = []
    for group in ("split_2", "split_4", "split_5_tiles_in_4", "split_3_tiles_in_2"):
        l = R.nt_groups(dtype)[group][0]
        o = R.operands(l.case, dtype, "rand")
        want = R.conv_fwd(o["x"], o["wr"], l.case)
        yard32 = R.dist(R.conv_fwd(o["x"], o["wr"], l.case, torch.float32), want)
        got = R.conv_fwd(o["x"], o["wr"], l.case, mutant="round_partial", cdt=dtype, nsplit=l.splitk)
        figs.append((group, R.dist(got, want), yard32, R.nt_ref(l.case, False, "plain", dtype, "rand")[1]))
        print(f"CONV round_partial {dtype} {group}: error {figs[-1][1]:.3g}, fp32 yardstick {yard32:.3g}, stored yardstick {figs[-1][3]:.3g}")
    if dtype == "f32":
        assert all(f[1] <= R.K * f[2] for f in figs), figs
    else:
        assert all(f[1] >= R.MUTANT_FACTOR * R.K * f[2] for f in figs), figs


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_panels_have_padding_to_leave_unwritten(dtype):
    """``pad_unwritten``: the tables hold forward and backward panels with K < Kpad, where the mutant leaves NaN"""
    fwd = bwd = 0
    for Cin, Cout, k, s, p in R.pack_keys(dtype):
        case = (1, 8, 8, Cin, Cout, k, s, p, 0)
        w = R.operands(case, dtype, "rand")["w"]
        a, b = R.panels_fwd(w, case, dtype, mutant="pad_unwritten"), R.panels_bwd(w, case, dtype, mutant="pad_unwritten")
        assert a.numel() == R.pack_fwd_elems(case, dtype) and b.numel() == R.pack_bwd_elems(case, dtype)
        fwd += bool(torch.isnan(a).any())
        bwd += bool(torch.isnan(b).any())
        assert not bool(torch.isnan(R.panels_fwd(w, case, dtype)).any()) and not bool(torch.isnan(R.panels_bwd(w, case, dtype)).any())
    assert fwd > 3 and bwd > 3 and math.isfinite(fwd)

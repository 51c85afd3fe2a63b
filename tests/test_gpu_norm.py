"""The eleven BatchNorm entry points of csrc/norm.hip on the MI355X against float64 (tests/norm_refs.py) at their launch edges: the case
table of norm_refs.CASES (one row; 85 row lanes with an idle thread; a second block of one row; the finaliser's second lane round; one row
lane; two column blocks; the largest partial table; the capped apply grid; 256-row blocks; an offset of 100 sigma), the fused finalisers
on synthetic tables either side of the workgroup-per-channel switch, and the data-parallel pair on shards of unequal sizes.

Every tensor a kernel writes is a slice of a larger buffer prefilled with NaN: after the call everything outside the slice is still NaN.
Workspaces are sized exactly by ``ops.bn_ws_floats`` (2*C or 5*C floats where the header says so).  Operands and results are compared on
the CPU in float64: a result may miss float64 by K = 8 yardsticks of its own output (the float32 restatement, stored in the output's dtype);
the figure and the yardstick are printed before they are compared.  Where an activation is involved, the elements with |y| < Y_EXCLUDE
(act'(y) hangs on rounding) are left out of y, and their ``da`` is zero for the kernel and the reference alike: at most EXCLUDE_CAP of a
case.  Where the float64 answer is exactly zero (M = 1: dz, sum(dy * xhat), M2) the bound is K * 2^-23 of the scale of the terms that
cancel.

Worst figures of one run, in yardsticks (f32 / bf16 / f16): fwd_train 4.84 / 4.16 / 3.56, stats_local 6.05 / 3.17 / 5.15, fwd_eval and
bwd_eval 1.00 (the bits of the float32 restatement), fwd_train_fused 2.50 / 1.00 / 1.05, fwd_from_stats 2.87 / 1.75 / 1.92, bwd 3.62 /
3.18 / 1.98, bwd_post 2.07 / 1.87 / 1.98, bwd_fused 2.58 / 1.33 / 1.32, bwd_sums_local 3.14 / 1.99 / 1.78, bwd_from_sums 1.00.  The
largest, M2 of stats_local at 33 rows x 1028 channels, is the single-pass pivot form with one row lane: its two float32 sums are
amplified by 1 + (pivot - mean)^2 / var of the block before they cancel (comment of bn_stats_partial_kernel)."""
import importlib

import pytest
import torch

import norm_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 64                      # sentinel elements either side of a slice (a multiple of 16 bytes in every dtype)
F32 = torch.float32
eg = None
ops = None


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops
    torch.set_num_threads(16)


def arena(n, dtype=torch.float32, init=None):
    """(buffer, slice): ``n`` elements on a 16-byte boundary, NaN all around (and inside unless ``init`` is given)"""
    buf = torch.full((GUARD + n + GUARD,), NAN, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD:GUARD + n]
    if init is not None:
        view.copy_(init.reshape(-1))
    return buf, view


def intact(buf, view):
    """everything of ``buf`` outside ``view`` is still the sentinel"""
    lo = view.storage_offset()
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())


def all_intact(slots):
    torch.cuda.synchronize()
    return all(intact(b, v) for b, v in slots.values())


def all_nan(t):
    return bool(torch.isnan(t).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def counter(t0):
    """num_batches_tracked with a marked neighbour either side"""
    buf = torch.tensor([-7, t0, -7], dtype=torch.int64, device=DEV)
    return buf, buf[1:2]


def check(entry, dtype, case, output, got, want, yard, zero_scale=None):
    """print the figure and its yardstick, then compare.  An answer that is exactly zero has no scale of its own: the figure is then taken
    against ``zero_scale`` (the size of the terms that cancel) and the yardstick is 2^-23, a float32 rounding of either term"""
    got, want = got.detach().double().cpu().reshape(want.shape), want.double()
    if float(want.abs().max()) == 0.0:
        assert zero_scale is not None and bool(torch.isfinite(got).all()), (entry, dtype, case, output)
        fig, yard, of = float(got.abs().max()) / zero_scale, 2 * R.U32, "the cancelling terms' scale"
    else:
        fig, of = R.dist(got, want), "its float32 restatement"
    ratio = fig / yard if yard else (0.0 if fig == 0 else float("inf"))
    print(f"BNORM {entry} {dtype} {case} {output}: error {fig:.3g} = {ratio:.2f} yardsticks of {yard:.3g} ({of})")
    assert fig <= R.K * yard, (entry, dtype, case, output, fig, yard)


def dev(t, dtype=None):
    return t.to(DEV, R.TORCH_DTYPE[dtype] if dtype else None).contiguous()


def kept(c, y_pre, act):
    """the elements that are compared / carry a gradient, with the share left out asserted"""
    keep = R.keep_of(y_pre, act)
    assert 1.0 - float(keep.double().mean()) <= R.EXCLUDE_CAP, (c.get("name"), act)
    return keep


def cases_of(names):
    return [pytest.param(n, d, id=f"{n}-{d}") for n in names for d in R.CASES[n][3]]


# ---- 1. eg_bn_fwd_train, eg_bn_stats_local, eg_bn_fwd_eval -----------------------------------------------------------------------------
STAT_KEYS = ("save_mean", "save_invstd", "running_mean", "running_var")


def fwd_slots(c, ws_floats):
    M, C, tdt = c["M"], c["C"], R.TORCH_DTYPE[c["dtype"]]
    return dict(y=arena(M * C, tdt), save_mean=arena(C), save_invstd=arena(C), running_mean=arena(C, init=c["rm0"]),
                running_var=arena(C, init=c["rv0"]), ws=arena(ws_floats))


def check_forward(entry, c, case, act, s, nbuf, want, y32, pre):
    """the six outputs of a training forward against ``want``; ``y32``: the float32 restatement, ``pre``: y before the activation"""
    dtype = c["dtype"]
    assert all_intact(s), (entry, case, act)
    assert nbuf.tolist() == [-7, want["nbt"], -7], nbuf.tolist()
    for k in STAT_KEYS:
        check(entry, dtype, f"{case} {act}", k, s[k][1], want[k], R.yard32(y32[k], want[k]))
    keep = kept(c, pre, act)
    got = torch.where(keep, s["y"][1].double().cpu().reshape(want["y"].shape), want["y"])
    check(entry, dtype, f"{case} {act}", "y", got, want["y"], R.dist(R.stored(y32["y"], dtype), want["y"]))


@pytest.mark.parametrize("name,dtype", cases_of(R.CASES))
def test_fwd_train_against_float64(name, dtype):
    c = R.bn_case(name, dtype)
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    x, gamma, beta = dev(c["x"], dtype), dev(c["gamma"]), dev(c["beta"])
    assert R.launch_of(name, dtype) == R.LAUNCH[name]
    pre = R.fwd_train(c)["y"]
    for act in R.ACTS:
        want, y32 = R.fwd_train(c, act), R.fwd_train(c, act, dtype=F32)
        runs = []
        for _ in range(2):
            s = fwd_slots(c, ops.bn_ws_floats(M, C))
            nbuf, nbt = counter(c["nbt0"])
            ops.bn_fwd_train(dt, x, s["y"][1], M, C, gamma, beta, c["eps"], c["momentum"], s["running_mean"][1], s["running_var"][1], nbt,
                             s["save_mean"][1], s["save_invstd"][1], s["ws"][1], R.ACTS[act], R.SLOPE)
            runs.append(s)
        assert same_bits(x, dev(c["x"], dtype)), "the input changed"
        check_forward("fwd_train", c, name, act, s, nbuf, want, y32, pre)
        for k in STAT_KEYS + ("y",):
            assert same_bits(runs[0][k][1], runs[1][k][1]), f"{k}: two runs give different bits (statistics are deterministic)"
    # running_mean = running_var = num_batches_tracked = NULL: the other three outputs keep their bits
    s0 = fwd_slots(c, ops.bn_ws_floats(M, C))
    ops.bn_fwd_train(dt, x, s0["y"][1], M, C, gamma, beta, c["eps"], c["momentum"], None, None, None, s0["save_mean"][1], s0["save_invstd"][1],
                     s0["ws"][1], R.ACTS[act], R.SLOPE)
    assert all_intact(s0)
    assert all(same_bits(s0[k][1], s[k][1]) for k in ("y", "save_mean", "save_invstd"))
    assert same_bits(s0["running_mean"][1], c["rm0"]) and same_bits(s0["running_var"][1], c["rv0"])


@pytest.mark.parametrize("name,dtype", cases_of(R.CASES))
def test_stats_local_against_float64(name, dtype):
    c = R.bn_case(name, dtype)
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    s = dict(stats=arena(3 * C), ws=arena(ops.bn_ws_floats(M, C)))
    ops.bn_stats_local(dt, dev(c["x"], dtype), M, C, s["ws"][1], s["stats"][1])
    assert all_intact(s)
    got = s["stats"][1].cpu().view(3, C)
    want, y32 = R.stats(c["x"]), R.stats(c["x"], F32)
    assert bool((got[0] == M).all()), "count"
    check("stats_local", dtype, name, "mean", got[1], want[1], R.yard32(y32[1], want[1]))
    check("stats_local", dtype, name, "M2", got[2], want[2], R.yard32(y32[2], want[2]) if M > 1 else 0.0, zero_scale=float(c["x"].abs().max()) ** 2)


@pytest.mark.parametrize("name,dtype", cases_of(R.BWD_CASES))
def test_fwd_eval_against_float64(name, dtype):
    c = R.bn_case(name, dtype)
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    ins = [dev(c[k]) for k in ("gamma", "beta", "rm0", "rv0")]
    x = dev(c["x"], dtype)
    pre = R.fwd_eval(c)
    for act in R.ACTS:
        s = dict(y=arena(M * C, R.TORCH_DTYPE[dtype]), ws=arena(2 * C))
        ops.bn_fwd_eval(dt, x, s["y"][1], M, C, ins[0], ins[1], c["eps"], ins[2], ins[3], s["ws"][1], R.ACTS[act], R.SLOPE)
        assert all_intact(s)
        assert all(same_bits(t, c[k]) for t, k in zip(ins, ("gamma", "beta", "rm0", "rv0"))) and same_bits(x, dev(c["x"], dtype)), "an input changed"
        want = R.act(pre, act)
        got = torch.where(kept(c, pre, act), s["y"][1].double().cpu().view(M, C), want)
        check("fwd_eval", dtype, f"{name} {act}", "y", got, want, R.dist(R.stored(R.fwd_eval(c, act, F32), dtype), want))


# ---- 2. eg_bn_bwd, eg_bn_bwd_post, eg_bn_bwd_eval ----------------------------------------------------------------------------------------
def bwd_slots(c, ws_floats, acc):
    M, C = c["M"], c["C"]
    return dict(dz=arena(M * C, R.TORCH_DTYPE[c["dtype"]]), sums=arena(2 * C), dgamma=arena(C, init=c["dgamma0"] if acc else None),
                dbeta=arena(C, init=c["dbeta0"] if acc else None), ws=arena(ws_floats))


def check_backward(entry, c, case, s, want, y32, mean, istd, da):
    """dz, the two sums and the two parameter gradients; the scales of what cancels at M = 1"""
    dtype, C = c["dtype"], c["C"]
    a_dy = float((c["gamma"] * istd * da).abs().max())
    check(entry, dtype, case, "dz", s["dz"][1], want["dz"], R.dist(R.stored(y32["dz"], dtype), want["dz"]) if float(want["dz"].abs().max()) else 0.0,
          zero_scale=a_dy)
    sums = s["sums"][1].cpu()
    zs = max(float(da.abs().max()), 1e-30)
    for k, got in (("s1", sums[:C]), ("s2", sums[C:]), ("dgamma", s["dgamma"][1]), ("dbeta", s["dbeta"][1])):
        check(entry, dtype, case, k, got, want[k], R.yard32(y32[k], want[k]) if float(want[k].abs().max()) else 0.0, zero_scale=zs)


@pytest.mark.parametrize("name,dtype", cases_of(R.BWD_CASES))
def test_bwd_against_float64(name, dtype):
    c = R.bn_case(name, dtype)
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    mean, istd = R.saved(c)
    z, gamma, beta, dmean, distd = dev(c["x"], dtype), dev(c["gamma"]), dev(c["beta"]), dev(mean), dev(istd)
    pre = R.bwd(c)["y"]
    for act in R.ACTS:
        da = c["da"] * kept(c, pre, act)
        dda = dev(da, dtype)
        both = R.bwd(c, act, 1, da=da), R.bwd(c, act, 1, dtype=F32, da=da)
        for acc in (0, 1):
            want, y32 = both if acc else (dict(o, dgamma=o["s2"], dbeta=o["s1"]) for o in both)      # stored: the sums themselves
            s = bwd_slots(c, ops.bn_ws_floats(M, C), acc)
            ops.bn_bwd(dt, z, dda, s["dz"][1], M, C, gamma, beta, dmean, distd, R.ACTS[act], R.SLOPE, s["dgamma"][1], s["dbeta"][1], s["sums"][1],
                       s["ws"][1], accumulate=bool(acc))
            assert all_intact(s), (name, act, acc)
            assert same_bits(z, dev(c["x"], dtype)) and same_bits(dda, dev(da, dtype)), "an input changed"
            check_backward("bwd", c, f"{name} {act} accumulate={acc}", s, want, y32, mean, istd, da)
        # dgamma = dbeta = NULL: dz and the sums keep their bits
        s0 = bwd_slots(c, ops.bn_ws_floats(M, C), 0)
        ops.bn_bwd(dt, z, dda, s0["dz"][1], M, C, gamma, beta, dmean, distd, R.ACTS[act], R.SLOPE, None, None, s0["sums"][1], s0["ws"][1])
        assert all_intact(s0) and all_nan(s0["dgamma"][0]) and all_nan(s0["dbeta"][0])
        assert same_bits(s0["dz"][1], s["dz"][1]) and same_bits(s0["sums"][1], s["sums"][1])


@pytest.mark.parametrize("name,dtype", cases_of(R.BWD_CASES))
def test_bwd_post_against_float64(name, dtype):
    """post_act = LeakyReLU on z as an activation output, with and without post_sigma; dgamma / dbeta always accumulate"""
    c = R.bn_case(name, dtype)
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    mean, istd = R.saved(c)
    z, dda, sigma = dev(c["x"], dtype), dev(c["da"], dtype), dev(c["sigma"])
    for with_sigma in (True, False):
        want, y32 = R.bwd_post(c, "lrelu", with_sigma), R.bwd_post(c, "lrelu", with_sigma, dtype=F32)
        s = bwd_slots(c, ops.bn_ws_floats(M, C), 1)
        ops.bn_bwd_post(dt, z, dda, s["dz"][1], M, C, dev(c["gamma"]), dev(c["beta"]), dev(mean), dev(istd), s["dgamma"][1], s["dbeta"][1], s["sums"][1],
                        s["ws"][1], R.ACTS["lrelu"], R.SLOPE, sigma if with_sigma else None)
        assert all_intact(s), (name, with_sigma)
        assert same_bits(sigma, c["sigma"])
        check_backward("bwd_post", c, f"{name} sigma={int(with_sigma)}", s, want, y32, mean, istd, c["da"])


@pytest.mark.parametrize("name,dtype", cases_of(R.EVAL_BWD_CASES))
def test_bwd_eval_against_float64(name, dtype):
    c = R.bn_case(name, dtype)
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    for act in R.ACTS:
        cc = dict(c, da=c["da"] * kept(c, R.fwd_eval(c), act))
        s = dict(dz=arena(M * C, R.TORCH_DTYPE[dtype]), ws=arena(2 * C))
        ops.bn_bwd_eval(dt, dev(c["x"], dtype), dev(cc["da"], dtype), s["dz"][1], M, C, dev(c["gamma"]), dev(c["beta"]), c["eps"], dev(c["rm0"]),
                        dev(c["rv0"]), s["ws"][1], R.ACTS[act], R.SLOPE)
        assert all_intact(s)
        want = R.bwd_eval(cc, act)[0]
        check("bwd_eval", dtype, f"{name} {act}", "dz", s["dz"][1], want, R.dist(R.stored(R.bwd_eval(cc, act, F32)[0], dtype), want))


# ---- 3. the fused finalisers on synthetic tables -----------------------------------------------------------------------------------------
FUSED = [pytest.param(nrb, C, d, id=f"nrb{nrb}-C{C}-{d}") for nrb, C, d in R.FUSED_CASES]


@pytest.mark.parametrize("nrb,C0,dtype", FUSED)
def test_fwd_train_fused_against_float64(nrb, C0, dtype):
    """the table is synthesised on the CPU (norm_refs.block_moments, rounded to float32): no convolution is involved.  nrb either side of
    64 (the wave's lane loop) and of 1024 (a workgroup per channel instead of a wave)"""
    c = R.fused_case(nrb, C0, dtype)
    st = lambda dt_: R.fused_stats(c["stat_fwd"], R.FUSED_RPB, dt_)
    pre = R.fwd_train(c, st=st)["y"]
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    x, stat, gamma, beta = dev(c["x"], dtype), dev(c["stat_fwd"]), dev(c["gamma"]), dev(c["beta"])
    for act in R.ACTS:
        want, y32 = R.fwd_train(c, act, st=st), R.fwd_train(c, act, dtype=F32, st=st)
        s = fwd_slots(c, 2 * C)
        nbuf, nbt = counter(c["nbt0"])
        ops.bn_fwd_train_fused(dt, x, s["y"][1], M, C, stat, nrb, R.FUSED_RPB, gamma, beta, c["eps"], c["momentum"], s["running_mean"][1],
                               s["running_var"][1], nbt, s["save_mean"][1], s["save_invstd"][1], s["ws"][1], R.ACTS[act], R.SLOPE)
        assert same_bits(stat, c["stat_fwd"]), "the table changed"
        check_forward("fwd_train_fused", c, f"nrb={nrb} C={C}", act, s, nbuf, want, y32, pre)
    # nrb * rows_per_block != M: refused, nothing written
    s = fwd_slots(c, 2 * C)
    nbuf, nbt = counter(c["nbt0"])
    with pytest.raises(RuntimeError, match="eg_bn_fwd_train_fused: nrb \\* rows_per_block must be M"):
        ops.bn_fwd_train_fused(dt, x, s["y"][1], M, C, stat, nrb, R.FUSED_RPB + 1, gamma, beta, c["eps"], c["momentum"], s["running_mean"][1],
                               s["running_var"][1], nbt, s["save_mean"][1], s["save_invstd"][1], s["ws"][1], 0, 0.0)
    assert all_intact(s) and nbuf.tolist() == [-7, c["nbt0"], -7]
    assert all(all_nan(s[k][1]) for k in ("y", "save_mean", "save_invstd", "ws")) and same_bits(s["running_var"][1], c["rv0"])


@pytest.mark.parametrize("nrb,C0,dtype", FUSED)
def test_bwd_fused_against_float64(nrb, C0, dtype):
    """dy carries the activation gradient already; the two sums come from the table (norm_refs.block_sums, rounded to float32)"""
    c = R.fused_case(nrb, C0, dtype)
    M, C, dt = c["M"], c["C"], eg.engine.parse_dtype(dtype)
    mean, istd = c["mean"], c["istd"]
    tab = R.fused_sums(c["stat_bwd"])
    tab32 = R.fused_sums(c["stat_bwd"], F32)
    for acc in (0, 1):
        want, y32 = R.bwd(c, "none", acc, sums=tab, mean=mean, istd=istd), R.bwd(c, "none", acc, dtype=F32, sums=tab, mean=mean, istd=istd)
        for o, t in ((want, tab), (y32, tab32)):                         # the sums and the parameter gradients are the table's, not the rows'
            o["s1"], o["s2"] = t
            o["dbeta"], o["dgamma"] = (c["dbeta0"].to(t[0].dtype) + t[0], c["dgamma0"].to(t[0].dtype) + t[1]) if acc else t
        s = bwd_slots(c, 5 * C, acc)
        stat = dev(c["stat_bwd"])
        ops.bn_bwd_fused(dt, dev(c["x"], dtype), dev(c["da"], dtype), s["dz"][1], M, C, stat, nrb, dev(c["gamma"]), dev(c["beta"]), dev(mean), dev(istd),
                         s["dgamma"][1], s["dbeta"][1], s["sums"][1], s["ws"][1], accumulate=bool(acc))
        assert all_intact(s) and same_bits(stat, c["stat_bwd"])
        check_backward("bwd_fused", c, f"nrb={nrb} C={C} accumulate={acc}", s, want, y32, mean, istd, c["da"])


# ---- 4. the data-parallel pair -------------------------------------------------------------------------------------------------------------
DP = [pytest.param(n, d, id=f"ranks{n}-{d}") for n in R.DP_SHARDS for d in R.DTYPES]


@pytest.mark.parametrize("nranks,dtype", DP)
def test_data_parallel_forward_against_float64(nranks, dtype):
    """eg_bn_stats_local per shard, the triples gathered on the host, eg_bn_fwd_from_stats per shard with M_global: every rank ends with
    the whole batch's statistics and its share of the whole batch's y"""
    c, ranges = R.dp_case(nranks, dtype)
    M, C, dt, act = c["M"], c["C"], eg.engine.parse_dtype(dtype), "lrelu"
    xs = [dev(c["x"][a:b], dtype) for a, b in ranges]
    gamma, beta = dev(c["gamma"]), dev(c["beta"])
    triples = []
    for x, (a, b) in zip(xs, ranges):
        s = dict(stats=arena(3 * C), ws=arena(ops.bn_ws_floats(b - a, C)))
        ops.bn_stats_local(dt, x, b - a, C, s["ws"][1], s["stats"][1])
        assert all_intact(s)
        triples.append(s["stats"][1].cpu())
    stats_all = dev(torch.stack(triples))
    want = R.fwd_train(c, act)
    t32 = torch.stack([torch.stack(R.stats(c["x"][a:b], F32)) for a, b in ranges])
    o32 = [R.fwd_from_stats(c, c["x"][a:b], t32, M, act, F32) for a, b in ranges]
    ys, first = [], None
    for x, (a, b) in zip(xs, ranges):
        cs = dict(c, M=b - a)
        s = fwd_slots(cs, ops.bn_ws_floats(b - a, C))
        nbuf, nbt = counter(c["nbt0"])
        ops.bn_fwd_from_stats(dt, x, s["y"][1], b - a, C, stats_all, nranks, M, gamma, beta, c["eps"], c["momentum"], s["running_mean"][1],
                              s["running_var"][1], nbt, s["save_mean"][1], s["save_invstd"][1], s["ws"][1], R.ACTS[act], R.SLOPE)
        assert all_intact(s) and nbuf.tolist() == [-7, c["nbt0"] + 1, -7]
        first = first or s
        assert all(same_bits(s[k][1], first[k][1]) for k in STAT_KEYS), "the ranks disagree on the statistics"
        ys.append(s["y"][1].cpu().view(b - a, C))
    for k in STAT_KEYS:
        check("fwd_from_stats", dtype, f"ranks={nranks} {act}", k, first[k][1], want[k], R.yard32(o32[0][k], want[k]))
    keep = kept(c, R.fwd_train(c)["y"], act)
    got = torch.where(keep, torch.cat(ys).double(), want["y"])
    check("fwd_from_stats", dtype, f"ranks={nranks} {act}", "y", got, want["y"], R.dist(R.stored(torch.cat([o["y"] for o in o32]), dtype), want["y"]))


@pytest.mark.parametrize("nranks,dtype", DP)
def test_data_parallel_backward_against_float64(nranks, dtype):
    """eg_bn_bwd_sums_local per shard (dgamma / dbeta take the LOCAL sums), the sums added on the host in float32, eg_bn_bwd_from_sums per
    shard with M_global: the shards' dz are the whole batch's"""
    c, ranges = R.dp_case(nranks, dtype)
    M, C, dt, act = c["M"], c["C"], eg.engine.parse_dtype(dtype), "lrelu"
    mean, istd = R.saved(c)
    da = c["da"] * kept(c, R.fwd_train(c)["y"], act)
    want = R.bwd(c, act, 1, da=da)
    gamma, beta, dmean, distd = dev(c["gamma"]), dev(c["beta"]), dev(mean), dev(istd)
    zs, das = [dev(c["x"][a:b], dtype) for a, b in ranges], [dev(da[a:b], dtype) for a, b in ranges]
    local, local32 = [], []
    for z, d, (a, b) in zip(zs, das, ranges):
        s = dict(sums=arena(2 * C), dgamma=arena(C, init=c["dgamma0"]), dbeta=arena(C, init=c["dbeta0"]), ws=arena(ops.bn_ws_floats(b - a, C)))
        ops.bn_bwd_sums_local(dt, z, d, b - a, C, gamma, beta, dmean, distd, R.ACTS[act], R.SLOPE, s["dgamma"][1], s["dbeta"][1], s["sums"][1], s["ws"][1])
        assert all_intact(s)
        w = R.bwd_sums_local(c, c["x"][a:b], da[a:b], mean, istd, act)
        w32 = R.bwd_sums_local(c, c["x"][a:b], da[a:b], mean, istd, act, dtype=F32)
        if nranks != 65 or (a, b) in (ranges[0], ranges[-1]):
            for i, (k, got) in enumerate((("s1", s["sums"][1][:C]), ("s2", s["sums"][1][C:]), ("dgamma", s["dgamma"][1]), ("dbeta", s["dbeta"][1]))):
                check("bwd_sums_local", dtype, f"ranks={nranks} rows {a}:{b}", k, got, w[i], R.yard32(w32[i], w[i]), zero_scale=1.0)
        local.append(s["sums"][1].cpu())
        local32.append(torch.cat(w32[:2]))
    sums = torch.stack(local).sum(0)                                     # the all-reduce, in float32 on the host
    s32 = torch.stack(local32).sum(0)
    dsums = dev(sums)
    dzs, dz32 = [], []
    for z, d, (a, b) in zip(zs, das, ranges):
        s = dict(dz=arena((b - a) * C, R.TORCH_DTYPE[dtype]), ws=arena(ops.bn_ws_floats(b - a, C)))
        ops.bn_bwd_from_sums(dt, z, d, s["dz"][1], b - a, C, dsums, M, gamma, beta, dmean, distd, R.ACTS[act], R.SLOPE, s["ws"][1])
        assert all_intact(s)
        dzs.append(s["dz"][1].cpu().view(b - a, C))
        dz32.append(R.bwd_from_sums(c, c["x"][a:b], da[a:b], (s32[:C], s32[C:]), M, mean, istd, act, dtype=F32))
    assert same_bits(dsums, sums)
    check("bwd_from_sums", dtype, f"ranks={nranks} {act}", "dz", torch.cat(dzs), want["dz"], R.dist(R.stored(torch.cat(dz32), dtype), want["dz"]))

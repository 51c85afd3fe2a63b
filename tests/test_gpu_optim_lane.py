"""The optimizer-lane kernels on the MI355X against float64 (tests/optim_refs.py) at their launch edges: the flat Adam update (eg_adam_step,
eg_adam_step_zero, eg_adam_tick, eg_fill_f32), Adam fused with re-packing (eg_adam_pack_conv, eg_adam_pack_rows) and the spectral-norm power
iteration (eg_sn_power_iter, eg_sn_power_iter_multi).

Every tensor a kernel writes is a slice of a larger buffer prefilled with NaN: after the call everything outside the slice is still NaN.
Workspaces are sized exactly by the project's ``*_ws_floats`` queries.  Values follow the project's rule: a result may miss float64 by
K = 8 times what the float32 restatement on the CPU misses it by (one yardstick per case: the worst of its outputs); the figure and the
yardstick are printed before they are compared.  Bit comparisons are made on the integer view of the bytes."""
import importlib

import pytest
import torch

import optim_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 64                      # sentinel elements either side of a slice (a multiple of 16 bytes in every dtype)
eg = None
ops = None


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops
    torch.set_num_threads(16)


def arena(n, off=0, dtype=torch.float32, init=None):
    """(buffer, slice): ``n`` elements ``off`` elements behind a 16-byte boundary, NaN all around (and inside unless ``init`` is given)"""
    buf = torch.full((GUARD + off + n + GUARD,), NAN, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + off:GUARD + off + n]
    if init is not None:
        view.copy_(init.reshape(-1))
    return buf, view


def intact(buf, view):
    """everything of ``buf`` outside ``view`` is still the sentinel"""
    lo = view.storage_offset()
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())


def all_nan(t):
    return bool(torch.isnan(t).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def counter(t0):
    """a device step counter with a marked neighbour either side"""
    buf = torch.tensor([-7, t0, -7], dtype=torch.int32, device=DEV)
    return buf, buf[1:2]


def record(group, dtype, what, fig, yard):
    print(f"OPTLANE {group} {dtype} {what}: error {fig:.3g} = {fig / yard if yard else 0.0:.2f} yardsticks of {yard:.3g}")


def worst(got, want):
    return max(R.dist(a, b) for a, b in zip(got, want))


# ---- 1. flat Adam -------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("step", "zero1", "zero0")           # eg_adam_step; eg_adam_step_zero with and without clearing the gradient


def run_flat(c, off, align, entry, betas=R.BETAS, tick=True, start=None):
    """all updates of the case ``c`` through one entry point, the four slices at element offsets off (+ the alignment's extra) -> p, m, v"""
    n, t0 = c["p"].numel(), c["t0"]
    dg, dm, dv = R.ADAM_ALIGN[align]
    bp, p = arena(n, off, init=c["p"])
    bg, g = arena(n, off + dg)
    bm, m = arena(n, off + dm, init=c["m"])
    bv, v = arena(n, off + dv, init=c["v"])
    sbuf, step = counter(t0 if start is None else start)
    grads = c["g"].to(DEV)
    for k in range(grads.shape[0]):
        g.copy_(grads[k])
        if entry == "step":
            ops.adam_step(p, g, m, v, n, R.LR, betas[0], betas[1], R.EPS, step, tick)
        else:
            ops.adam_step_zero(p, g, m, v, n, R.LR, betas[0], betas[1], R.EPS, step, tick, entry == "zero1")
        if entry == "zero1":
            assert not bool(g.any()), "the gradient slice is not exactly zero"
        else:
            assert same_bits(g, grads[k]), "the gradient slice changed"
    assert intact(bp, p) and intact(bg, g) and intact(bm, m) and intact(bv, v), (n, off, align, entry)
    want_t = (t0 if start is None else start) + (grads.shape[0] if tick else 0)
    assert sbuf.tolist() == [-7, want_t, -7], sbuf.tolist()
    return p.cpu(), m.cpu(), v.cpu()


def check_flat(c, runs, what):
    """every run gives the same bits (vector path, scalar path, either kernel), and those are within the bound of float64"""
    first = None
    for off, align, entry in runs:
        got = run_flat(c, off, align, entry, c.get("betas", R.BETAS))
        if first is None:
            first = got
        assert all(same_bits(a, b) for a, b in zip(got, first)), (what, off, align, entry)
    fig = worst(first, c["want"])
    record("flat_adam", "f32", what, fig, c["yard"])
    assert fig <= R.K * c["yard"], (what, fig, c["yard"])


@pytest.mark.parametrize("t0", R.ADAM_T0)
@pytest.mark.parametrize("n", R.ADAM_LENGTHS)
def test_flat_adam_against_float64(n, t0):
    """every offset of p from a 16-byte boundary, the other three slices aligned like p (float2 middle + scalar ends) or not (scalar path)"""
    c = R.adam_case(n, t0)
    check_flat(c, [(off, al, e) for off in R.ADAM_OFFSETS for al in R.ADAM_ALIGN for e in ENTRIES], f"n={n} t0={t0}")


@pytest.mark.parametrize("t0", R.ADAM_T0)
def test_flat_adam_grid_stride(t0):
    """more work than 2048 blocks hold: the grid-stride loops of the vector path (aligned, unaligned ends) and of the scalar path"""
    c = R.adam_case(R.ADAM_LARGE, t0)
    check_flat(c, [(off, al, e) for off, al in R.ADAM_LARGE_RUNS for e in ("step", "zero1")], f"n={R.ADAM_LARGE} t0={t0}")


@pytest.mark.parametrize("t0", R.ADAM_T0)
@pytest.mark.parametrize("n", (5, 1027))
def test_flat_adam_with_torch_default_betas(n, t0):
    """b1 = 0.9 (the projection loop): the other side of the two-sided lerp"""
    c = dict(R.adam_case(n, t0, R.GRAD_SCALES, R.BETAS_TORCH), betas=R.BETAS_TORCH)
    check_flat(c, [(1, al, e) for al in R.ADAM_ALIGN for e in ("step", "zero1")], f"n={n} t0={t0} betas={R.BETAS_TORCH}")


@pytest.mark.parametrize("entry", ENTRIES)
def test_flat_adam_without_tick_leaves_the_counter(entry):
    """tick = 0: the counter stays, and the update is the one a tick from the step before gives"""
    for t0 in R.ADAM_T0:
        c = R.adam_case(257, t0, (1e-3,))
        for off, align in ((0, "same"), (3, "same"), (1, "g+1")):
            ticked = run_flat(c, off, align, entry)
            plain = run_flat(c, off, align, entry, tick=False, start=t0 + 1)
            assert all(same_bits(a, b) for a, b in zip(ticked, plain))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("align", list(R.ADAM_ALIGN))
def test_flat_adam_of_an_empty_slice_only_ticks(entry, align):
    """n == 0 with equally and differently aligned pointers: the call succeeds, nothing is written, the counter advances with ``tick`` alone"""
    dg, dm, dv = R.ADAM_ALIGN[align]
    x = torch.arange(1.0, 9.0)
    bufs = [arena(8, 1 + d, init=x) for d in (0, dg, dm, dv)]
    before = [b.clone() for b, _ in bufs]
    (_, p), (_, g), (_, m), (_, v) = bufs
    sbuf, step = counter(4)
    for tick, want in ((True, 5), (False, 5), (True, 6)):
        if entry == "step":
            ops.adam_step(p, g, m, v, 0, R.LR, *R.BETAS, R.EPS, step, tick)
        else:
            ops.adam_step_zero(p, g, m, v, 0, R.LR, *R.BETAS, R.EPS, step, tick, entry == "zero1")
        torch.cuda.synchronize()
        assert sbuf.tolist() == [-7, want, -7]
    assert all(same_bits(b, b0) for (b, _), b0 in zip(bufs, before))


@pytest.mark.parametrize("n", R.FILL_LENGTHS)
def test_fill_f32(n):
    for off in (0, 1):
        buf, view = arena(n + 1, off)              # (one element more than is filled: an empty tensor has no address)
        eg._lib.lib().call("eg_fill_f32", view.data_ptr(), n, 1.5, torch.cuda.current_stream().cuda_stream)
        assert bool((view[:n] == 1.5).all()) and all_nan(view[n:]) and intact(buf, view)
    if n:
        buf, view = arena(n, 3)
        ops.fill_f32(view)
        assert not bool(view.any()) and intact(buf, view)


@pytest.mark.parametrize("t0", (0, 2 ** 31 - 2))
def test_adam_tick(t0):
    sbuf, step = counter(t0)
    ops.adam_tick(step)
    assert sbuf.tolist() == [-7, t0 + 1, -7]


# ---- 2. eg_adam_pack_conv -----------------------------------------------------------------------------------------------------------------
DTYPES = ("f32", "bf16", "f16")


def conv_of(layer):
    Cout, Cin, k, stride, pad = layer
    return ops.make_conv(1, 8, 8, Cin, Cout, k, stride, pad)


def pack_conv_setup(layer, dtype, shift, seed):
    Cout, Cin, k, _, _ = layer
    dt, tdt, cv = eg.engine.parse_dtype(dtype), R.TORCH_DTYPE[dtype], conv_of(layer)
    c = R.pack_case(Cout * Cin * k * k, seed)
    masters = [arena(c["p"].numel(), shift, init=None if key == "g" else c[key]) for key in ("p", "g", "m", "v")]
    fwd, bwd = arena(ops.pack_fwd_elems(cv, dt), 0, tdt), arena(ops.pack_bwd_elems(cv, dt), 0, tdt)
    return dt, tdt, cv, c, masters, fwd, bwd


def run_pack_conv(layer, dtype, way, shift, seed):
    Cout, Cin, k, _, _ = layer
    has_fwd, has_bwd = R.CONV_WAYS[way]
    dt, tdt, cv, c, masters, (bf, wf), (bb, wb) = pack_conv_setup(layer, dtype, shift, seed)
    (bp, p), (bg, g), (bm, m), (bv, v) = masters
    n = p.numel()
    Kf = k * k * Cin
    Kpad = ops.round_up(Kf, ops.bk(dt))                   # (16, 32, 3, 1, 1) and the 16-bit (32, 32, 3, 2, 1) have K padding
    assert wf.numel() == Cout * Kpad
    pf, mf, vf = c["p"].to(DEV), c["m"].to(DEV), c["v"].to(DEV)
    sbuf, step = counter(0)
    sbuf_f, step_f = counter(0)
    grads = c["g"].to(DEV)
    for i in range(2):
        g.copy_(grads[i])
        ops.adam_tick(step)
        ops.adam_pack_conv(cv, dt, p, g, m, v, R.LR, *R.BETAS, R.EPS, step, wf if has_fwd else None, wb if has_bwd else None)
        assert same_bits(g, grads[i]), "the gradient slice changed"
        ops.adam_step_zero(pf, grads[i].clone(), mf, vf, n, R.LR, *R.BETAS, R.EPS, step_f, True, False)
    assert sbuf.tolist() == [-7, 2, -7]
    assert all(intact(b, s) for b, s in masters) and intact(bf, wf) and intact(bb, wb)
    assert same_bits(p, pf) and same_bits(m, mf) and same_bits(v, vf), "not the bits of the flat kernel"
    fig = worst((p, m, v), c["want"])
    ref_f, ref_b = torch.full_like(wf, NAN), torch.full_like(wb, NAN)
    master = p.clone()
    ops.pack_fwd(cv, dt, master, ref_f)
    ops.pack_bwd(cv, dt, master, ref_b)
    if has_fwd:
        panel = wf.view(Cout, Kpad).cpu()
        assert same_bits(panel[:, :Kf], R.fwd_panel(p.cpu(), Cout, Cin, k * k).to(tdt)), "forward panel: not the closed form"
        assert bool((panel[:, Kf:].float() == 0).all()), "forward panel: K padding is not zero"
        assert same_bits(wf, ref_f), "forward panel: not the gather kernel's bytes"
    else:
        assert all_nan(wf), "a forward panel that was not passed was written"
    if has_bwd:
        assert same_bits(wb, ref_b), "backward panels: not the gather kernel's bytes"
    else:
        assert all_nan(wb), "a backward panel that was not passed was written"
    return fig, c["yard"]


def assert_pack_conv_refused(layer, dtype, way, seed):
    """the call comes back as an argument error and nothing is written: masters, gradient, counter and both panels are as before"""
    has_fwd, has_bwd = R.CONV_WAYS[way]
    dt, tdt, cv, c, masters, (bf, wf), (bb, wb) = pack_conv_setup(layer, dtype, 0, seed)
    before = [b.clone() for b, _ in masters]
    sbuf, step = counter(1)
    with pytest.raises(RuntimeError, match="eg_adam_pack_conv"):
        ops.adam_pack_conv(cv, dt, *(s for _, s in masters), R.LR, *R.BETAS, R.EPS, step, wf if has_fwd else None, wb if has_bwd else None)
    torch.cuda.synchronize()
    assert all(same_bits(b, b0) for (b, _), b0 in zip(masters, before))
    assert all_nan(bf) and all_nan(bb) and sbuf.tolist() == [-7, 1, -7]


@pytest.mark.parametrize("way", list(R.CONV_WAYS))
@pytest.mark.parametrize("layer", R.CONV_LAYERS, ids=str)
@pytest.mark.parametrize("dtype", DTYPES)
def test_adam_pack_conv_against_float64(dtype, layer, way):
    """4x4 layers: the float4 form (aligned master slices) and the scalar 16-tap form (slices one float behind); 3x3: the run-time-tap form.
    The panels of (16, 32, 3, 1, 1) have K padding (backward K = 9 * 16 = 144, forward K = 9 * 32 = 288 against K blocks of 32 and 64): the
    kernel writes it as zeros, which the byte comparison with the gather kernels on NaN-filled panels checks."""
    cv, dt = conv_of(layer), eg.engine.parse_dtype(dtype)
    assert ops.adam_pack_conv_ok(cv, dt, *R.CONV_WAYS[way]), f"eg_adam_pack_conv_ok refuses {layer} {dtype} {way}"
    for shift in (0, 1):
        fig, yard = run_pack_conv(layer, dtype, way, shift, R.CONV_LAYERS.index(layer))
        record("adam_pack_conv", dtype, f"{layer} {way} shift={shift}", fig, yard)
        assert fig <= R.K * yard, (layer, dtype, way, shift, fig, yard)


@pytest.mark.parametrize("way", list(R.CONV_WAYS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_adam_pack_conv_of_the_strided_3x3_layer(dtype, way):
    """(32, 32, 3, 2, 1): run like the others where eg_adam_pack_conv_ok accepts it (it does, the 16-bit panels with their K padding
    included); were it not to, the refusal is what is asserted"""
    layer, seed = R.CONV_LAYER_MAYBE, len(R.CONV_LAYERS)
    if ops.adam_pack_conv_ok(conv_of(layer), eg.engine.parse_dtype(dtype), *R.CONV_WAYS[way]):
        for shift in (0, 1):
            fig, yard = run_pack_conv(layer, dtype, way, shift, seed)
            record("adam_pack_conv", dtype, f"{layer} {way} shift={shift}", fig, yard)
            assert fig <= R.K * yard, (layer, dtype, way, shift, fig, yard)
    else:
        print(f"OPTLANE adam_pack_conv {dtype} {layer} {way}: refused by eg_adam_pack_conv_ok")
        assert_pack_conv_refused(layer, dtype, way, seed)


@pytest.mark.parametrize("way", list(R.CONV_WAYS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_adam_pack_conv_refuses_a_ragged_channel_count(dtype, way):
    layer = R.CONV_LAYER_REFUSED
    assert not ops.adam_pack_conv_ok(conv_of(layer), eg.engine.parse_dtype(dtype), *R.CONV_WAYS[way])
    assert_pack_conv_refused(layer, dtype, way, 9)


# ---- 3. eg_adam_pack_rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ROWS_CASES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES)
def test_adam_pack_rows_against_float64(dtype, case):
    """the panel is first filled by eg_pack_strided (which writes the zeros of the K padding), then refreshed by two fused updates"""
    Kr, Cout = case
    N = 16 * Cout
    dt, tdt = eg.engine.parse_dtype(dtype), R.TORCH_DTYPE[dtype]
    Kpad = ops.round_up(Kr, ops.bk(dt))
    c = R.pack_case(Kr * N, 100 + R.ROWS_CASES.index(case))
    grads = c["g"].to(DEV)
    for shift in (0, 1):
        masters = [arena(Kr * N, shift, init=None if key == "g" else c[key]) for key in ("p", "g", "m", "v")]
        (bp, p), (bg, g), (bm, m), (bv, v) = masters
        bw, wp = arena(N * Kpad, 0, tdt)
        ops.pack_strided(dt, p, wp, N, Kr, Kpad, Cout, 1, 16, N)
        assert same_bits(wp.view(N, Kpad), R.rows_panel(c["p"], Kr, N, Kpad, 16, Cout).to(tdt))
        pf, mf, vf = c["p"].to(DEV), c["m"].to(DEV), c["v"].to(DEV)
        sbuf, step = counter(0)
        sbuf_f, step_f = counter(0)
        for i in range(2):
            g.copy_(grads[i])
            ops.adam_tick(step)
            ops.adam_pack_rows(dt, p, g, m, v, wp, Kr, N, Kpad, 16, Cout, R.LR, *R.BETAS, R.EPS, step)
            assert same_bits(g, grads[i]), "the gradient slice changed"
            ops.adam_step_zero(pf, grads[i].clone(), mf, vf, Kr * N, R.LR, *R.BETAS, R.EPS, step_f, True, False)
        assert sbuf.tolist() == [-7, 2, -7]
        assert all(intact(b, s) for b, s in masters) and intact(bw, wp)
        assert same_bits(p, pf) and same_bits(m, mf) and same_bits(v, vf), "not the bits of the flat kernel"
        fig = worst((p, m, v), c["want"])
        record("adam_pack_rows", dtype, f"{case} shift={shift}", fig, c["yard"])
        assert fig <= R.K * c["yard"], (case, dtype, fig, c["yard"])
        panel = wp.view(N, Kpad).cpu()
        assert same_bits(panel, R.rows_panel(p.cpu(), Kr, N, Kpad, 16, Cout).to(tdt)), "panel: not the closed form of the updated master"
        assert not bool(panel[:, Kr:].float().any()), "the K padding is no longer zero"


# ---- 4. spectral norm ---------------------------------------------------------------------------------------------------------------------
def sn_state(c, Rr, Kd, snaps=True):
    """device slices (one float behind a 16-byte boundary) of u, v, sigma and the snapshots of a case"""
    s = dict(u=arena(Rr, 1, init=c["u"]), v=arena(Kd, 1, init=c["v"]), sigma=arena(1, 1))
    s["us"], s["vs"] = (arena(Rr, 1), arena(Kd, 1)) if snaps else ((None, None), (None, None))
    return s


def sn_intact(s):
    return all(intact(b, x) for b, x in s.values() if b is not None)


def sn_got(s):
    return s["u"][1].cpu(), s["v"][1].cpu(), s["sigma"][1].cpu()[0]


@pytest.mark.parametrize("case", R.SN_CASES, ids=str)
def test_sn_power_iter_training_against_float64(case):
    Rr, Kd = case
    c = R.sn_case(Rr, Kd)
    W = c["W"].to(DEV)
    s, bare = sn_state(c, Rr, Kd), sn_state(c, Rr, Kd, snaps=False)
    bws, ws = arena(ops.sn_ws_floats(Rr, Kd))
    for it, (want, yard) in enumerate(c["train"]):
        ops.sn_power_iter(W, Rr, Kd, s["u"][1], s["v"][1], s["sigma"][1], s["us"][1], s["vs"][1], ws, True, R.SN_EPS)
        ops.sn_power_iter(W, Rr, Kd, bare["u"][1], bare["v"][1], bare["sigma"][1], None, None, ws, True, R.SN_EPS)
        got = sn_got(s)
        fig = worst(got, want)
        record("sn_power_iter_train", "f32", f"{case} iteration {it}", fig, yard)
        assert fig <= R.K * yard, (case, it, fig, yard)
        assert same_bits(s["us"][1], s["u"][1]) and same_bits(s["vs"][1], s["v"][1]), "snapshots are not the updated u and v"
        assert all(same_bits(a, b) for a, b in zip(got, sn_got(bare))), "the launch without snapshots gives other bits"
        assert sn_intact(s) and sn_intact(bare) and intact(bws, ws)


@pytest.mark.parametrize("case", R.SN_CASES, ids=str)
def test_sn_power_iter_eval_against_float64(case):
    Rr, Kd = case
    c = R.sn_case(Rr, Kd)
    s = sn_state(c, Rr, Kd)
    bws, ws = arena(ops.sn_ws_floats(Rr, Kd))
    ops.sn_power_iter(c["W"].to(DEV), Rr, Kd, s["u"][1], s["v"][1], s["sigma"][1], s["us"][1], s["vs"][1], ws, False, R.SN_EPS)
    want, yard = c["eval"]
    u, v, sigma = sn_got(s)
    assert same_bits(u, c["u"]) and same_bits(v, c["v"]), "eval changed u or v"
    assert all_nan(s["us"][0]) and all_nan(s["vs"][0]), "eval wrote a snapshot"
    fig = R.dist(sigma, want[2])
    record("sn_power_iter_eval", "f32", f"{case}", fig, yard)
    assert fig <= R.K * yard, (case, fig, yard)
    assert sn_intact(s) and intact(bws, ws)


def test_sn_power_iter_of_a_zero_matrix():
    """W = 0: the norms are clamped by eps, so u, v and sigma come out zero, not NaN"""
    Rr, Kd = 8, 16
    _, u0, v0 = R.sn_inputs(Rr, Kd)
    s = sn_state(dict(u=u0, v=v0), Rr, Kd)
    bws, ws = arena(ops.sn_ws_floats(Rr, Kd))
    ops.sn_power_iter(torch.zeros(Rr, Kd, device=DEV), Rr, Kd, s["u"][1], s["v"][1], s["sigma"][1], s["us"][1], s["vs"][1], ws, True, R.SN_EPS)
    for key in ("u", "v", "sigma", "us", "vs"):
        assert bool((s[key][1] == 0).all()), key
    assert sn_intact(s) and intact(bws, ws)


SN_EIGHT = R.SN_CASES + (R.SN_EXTRA,)
SN_SETS = {"eight": SN_EIGHT, "eight_reversed": SN_EIGHT[::-1], "one": ((7, 255),)}


def sn_multi_setup(cases):
    cs = [R.sn_case(Rr, Kd) for Rr, Kd in cases]
    states = [sn_state(c, Rr, Kd) for c, (Rr, Kd) in zip(cs, cases)]
    Ws = [c["W"].to(DEV) for c in cs]
    arr = ops.sn_layers([(W, s["u"][1], s["v"][1], s["sigma"][1], s["us"][1], s["vs"][1]) for W, s in zip(Ws, states)])
    return cs, states, Ws, arr


@pytest.mark.parametrize("name", list(SN_SETS))
def test_sn_power_iter_multi_training_against_float64(name):
    """SN_MAXL layers in one launch per stage, the largest R and Kd first or last (blocks beyond a layer's own extent return early), and one
    layer alone: each layer against float64, the workspace exactly eg_sn_multi_ws_floats long"""
    cases = SN_SETS[name]
    cs, states, Ws, arr = sn_multi_setup(cases)
    bws, ws = arena(ops.sn_multi_ws_floats(arr))
    assert ws.numel() == sum(8 * Kd + Rr for Rr, Kd in cases)
    for it in range(2):
        ops.sn_power_iter_multi(arr, ws, True, R.SN_EPS)
        for case, c, s in zip(cases, cs, states):
            want, yard = c["train"][it]
            fig = worst(sn_got(s), want)
            record("sn_power_iter_multi_train", "f32", f"{name} {case} iteration {it}", fig, yard)
            assert fig <= R.K * yard, (name, case, it, fig, yard)
            assert same_bits(s["us"][1], s["u"][1]) and same_bits(s["vs"][1], s["v"][1]), "snapshots are not the updated u and v"
            assert sn_intact(s)
        assert intact(bws, ws)


@pytest.mark.parametrize("name", list(SN_SETS))
def test_sn_power_iter_multi_eval_against_float64(name):
    cases = SN_SETS[name]
    cs, states, Ws, arr = sn_multi_setup(cases)
    bws, ws = arena(ops.sn_multi_ws_floats(arr))
    ops.sn_power_iter_multi(arr, ws, False, R.SN_EPS)
    for case, c, s in zip(cases, cs, states):
        want, yard = c["eval"]
        u, v, sigma = sn_got(s)
        assert same_bits(u, c["u"]) and same_bits(v, c["v"]), "eval changed u or v"
        assert all_nan(s["us"][0]) and all_nan(s["vs"][0]), "eval wrote a snapshot"
        fig = R.dist(sigma, want[2])
        record("sn_power_iter_multi_eval", "f32", f"{name} {case}", fig, yard)
        assert fig <= R.K * yard, (name, case, fig, yard)
        assert sn_intact(s)
    assert intact(bws, ws)


@pytest.mark.parametrize("training", (True, False))
def test_sn_power_iter_multi_refuses_nine_layers(training):
    cases = SN_EIGHT + ((3, 5),)
    cs, states, Ws, arr = sn_multi_setup(cases)
    bws, ws = arena(ops.sn_multi_ws_floats(arr))
    with pytest.raises(RuntimeError, match="eg_sn_power_iter_multi"):
        ops.sn_power_iter_multi(arr, ws, training, R.SN_EPS)
    torch.cuda.synchronize()
    for c, s in zip(cs, states):
        assert same_bits(s["u"][1], c["u"]) and same_bits(s["v"][1], c["v"])
        assert all_nan(s["sigma"][0]) and all_nan(s["us"][0]) and all_nan(s["vs"][0]) and sn_intact(s)
    assert all_nan(bws)

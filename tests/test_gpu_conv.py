"""The convolution kernels on the MI355X against float64 (tests/conv_refs.py) at their launch edges: eg_conv_fwd and eg_conv_bwd_data on every
NT kernel (register-staged, buffer-descriptor, persistent, the 8-wave kernels with and without the input patch, their K splits),
eg_conv_wgrad on the per-tap and the parity-class kernel, and eg_pack_fwd / eg_pack_bwd / eg_pack_conv.

Every tensor a kernel writes -- Y, dX, the slab, the split-K scratch, the panels -- is a slice of a larger buffer prefilled with NaN: after
the call every element of the slice is written (a NaN left over fails the comparison) and everything outside it is still NaN.  The operands
sit in such buffers too, so a read past their end shows as NaN in the result.  Slabs are exactly eg_conv_wgrad_ws_bytes, scratches exactly
the restated (or queried) size, zeroed once, and their last 4 KiB are zero again after every launch.  Every launch is made twice on fresh
buffers and gives the same bits.  The weight panels the NT launches read are the restated ones (conv_refs.panels_fwd / panels_bwd); the pack
kernels are compared with those bit for bit.

Each case runs two operand sets (conv_refs): the integer set must give float64's value exactly, whatever the storage dtype; the random
set may miss float64 by K = 8 times what the float32 restatement on the CPU misses it by, and the figure and the yardstick are printed
before they are compared.  Unsplit launches of the buffer-descriptor, persistent and 8-wave kernels (not the input-patch variant) must
also give the bits of the register-staged kernel, as the header promises."""
import importlib

import pytest
import torch

import conv_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 64                      # NaN elements either side of a slice (a multiple of 16 bytes in every dtype)
eg = None
ops = None


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops
    torch.set_num_threads(16)


def types(dtype):
    dt = eg.engine.parse_dtype(dtype)
    assert ops.vec(dt) == R.VEC[dtype] and ops.bk(dt) == R.BK[dtype]
    return dt, R.TORCH_DTYPE[dtype]


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


def sync():
    """wait for the device; a device error ends the session (nothing more is launched on a GPU that has reported one)"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"the GPU reported an error, stopping: {err}", returncode=3)


def intact(pairs):
    return all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + v.numel():]).all()) for b, v in pairs if b is not None)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def twice(run):
    a, b = run(), run()
    sync()
    assert all(same_bits(x, y) for x, y in zip(a, b)), "a second launch gives other bits"
    return a


def check(what, kind, got, want, yard):
    """the integer set: float64's value exactly; the random set: print, then assert, the distance from float64 against K yardsticks"""
    got = got.detach().double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: an element was not written (or an operand was read past its end)"
    if kind == "int":
        assert torch.equal(got, want), (what, "integer set", float((got - want).abs().max()))
        return 0.0
    fig = R.dist(got, want)
    print(f"CONV {what}: error {fig:.3g} = {fig / yard if yard else 0.0:.2f} yardsticks of {yard:.3g}, bound {R.K * yard:.3g}")
    assert fig <= R.K * yard, (what, fig, yard)
    return fig


# ---- 1. eg_conv_fwd / eg_conv_bwd_data ---------------------------------------------------------------------------------------------------
def nt_run(l, dtype, kind):
    """one launch of the table on fresh guarded buffers, twice: the output tensor"""
    dt, tdt = types(dtype)
    B, H, W, Cin, Cout, k, s, p, up = l.case
    XH, XW, OH, OW = R.geom(l.case)
    o, e = R.operands(l.case, dtype, kind), R.ep_operands(l.case, l.bwd, l.ep, dtype, kind)
    c = ops.make_conv(*l.case)
    N = Cin if l.bwd else Cout
    rows = B * XH * XW if l.bwd else B * OH * OW
    src = o["dy"] if l.bwd else o["x"]
    panel = R.panels_bwd(o["w"], l.case, dtype) if l.bwd else R.panels_fwd(o["w"], l.case, dtype)
    assert panel.numel() == (ops.pack_bwd_elems if l.bwd else ops.pack_fwd_elems)(c, dt)
    assert not (e["nchw"] and e.get("mask") is not None)
    if l.ws == "query":
        nbytes = ops.conv_splitk_ws_bytes(c, dt, l.bwd)
    else:
        nbytes = R.scratch_bytes(l) if l.ws else 0

    def run():
        held = [arena(src.shape, tdt, init=src), arena(panel.numel(), tdt, init=panel)]
        out = arena((B, N, XH if l.bwd else OH, XW if l.bwd else OW), torch.float32) if e["nchw"] else arena((rows, N), tdt)
        t = {}
        for name in ("bias", "sigma"):
            if e.get(name) is not None:
                held.append(arena(e[name].shape, torch.float32, init=e[name]))
                t[name] = held[-1][1]
        if e.get("mask") is not None:
            held.append(arena((rows, N), tdt, init=e["mask"]))
            t["mask"] = held[-1][1]
        ws = arena(nbytes // 4, torch.float32, fill=0.0) if nbytes else (None, None)
        ep = ops.epilogue(bias=t.get("bias"), bias_mod=e.get("bias_mod", 0), sigma=t.get("sigma"), act=R.ACTS.index(e["act"]), slope=e["slope"],
                          mask=t.get("mask"), mask_act=R.ACTS.index(e.get("mask_act", "none")), mask_slope=e.get("mask_slope", 0.0),
                          out_mode=ops.OUT_NCHW_F32 if e["nchw"] else ops.OUT_NHWC, sigma_rows=e.get("sigma_rows", 0),
                          nt_variant=l.variant, nt_splitk=l.splitk, splitk_ws=ws[1])
        label = ops.nt_tile(c, dt, l.bwd, ep)
        assert label > 0 and (l.label is None or label == l.label), (l, label)
        (ops.conv_bwd_data if l.bwd else ops.conv_fwd)(c, dt, held[0][1], held[1][1], out[1], ep)
        sync()
        assert intact(held + [out, ws]), (l, "a guard was overwritten")
        if nbytes:
            assert not bool(ws[1][-(R.CNT_BYTES // 4):].any()), (l, "the arrival counters are not back at zero")
            assert bool(torch.isfinite(ws[1]).all())
            if l.ws == "exact" and kind == "rand":
                assert bool(ws[1][:-(R.CNT_BYTES // 4)].any()), (l, "the launch was to split K and left its scratch untouched")
        return (out[1],)
    return twice(run)[0]


GROUPS = tuple(R.nt_groups("f32").keys())


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_nt_launches_against_float64(dtype, group):
    reg = {}
    for l in R.nt_groups(dtype)[group]:
        for kind in ("int", "rand"):
            if kind == "int" and not R.ep_exact(l.ep):
                continue
            want, yard = R.nt_ref(l.case, l.bwd, l.ep, dtype, kind)
            got = nt_run(l, dtype, kind)
            what = (f"{'bwd_data' if l.bwd else 'fwd'} {R.NT_NAME[l.variant]}{'/%d' % l.splitk if l.splitk else ''}"
                    f"{'' if l.ws in (None, 'exact') else '/' + l.ws} {dtype} {group} {l.case} {l.ep}")
            check(what, kind, got, want, yard)
            if l.vs_reg:
                key = (l.case, l.bwd, l.ep, kind)
                if key not in reg:
                    reg[key] = nt_run(R.Launch(l.case, l.bwd, R.NT_REG, 0, l.ep, None, None, False), dtype, kind)
                assert same_bits(got, reg[key]), (what, "not the bits of EG_NT_REG")


# ---- 2. eg_conv_wgrad ----------------------------------------------------------------------------------------------------------------------
def wgrad_run(case, dtype, kind, wgs_target):
    dt, tdt = types(dtype)
    B, H, W, Cin, Cout, k, s, p, up = case
    o = R.operands(case, dtype, kind)
    c = ops.make_conv(*case)
    variant, want, yard = R.wgrad_ref(case, dtype, kind, wgs_target)
    assert ops.conv_wgrad_variant(c, dt) == variant
    nbytes = ops.conv_wgrad_ws_bytes(c, dt)
    per = Cout * k * k * Cin
    assert nbytes == R.wgrad_ws_bytes(case, dtype) and nbytes >= want.shape[0] * per * 4

    def run():
        held = [arena(o["x"].shape, tdt, init=o["x"]), arena(o["dy"].shape, tdt, init=o["dy"])]
        slab = arena(nbytes // 4, torch.float32)
        ns = ops.conv_wgrad(c, dt, held[0][1], held[1][1], slab[1], wgs_target)
        sync()
        assert ns == want.shape[0], (case, ns, want.shape)
        assert intact(held + [slab]) and bool(torch.isnan(slab[1][ns * per:]).all()), (case, "written outside the slab's splits")
        return (slab[1][:ns * per],)
    got = twice(run)[0]
    return check(f"wgrad {'tn8' if variant == 2 else 'tn'}{'/%d' % wgs_target if wgs_target else ''} {dtype} {case}", kind, got, want, yard)


@pytest.mark.parametrize("dtype,case", [(d, c) for d in R.DTYPES for c, dts in R.TN_CASES if d in dts], ids=str)
def test_wgrad_per_tap_against_float64(dtype, case):
    for kind in ("int", "rand"):
        wgrad_run(case, dtype, kind, 0)


@pytest.mark.parametrize("case", [c for c, _, _ in R.TN8_CASES] + [R.TN8_REFUSED] + list(R.TN8_SMALL_REFUSED), ids=str)
@pytest.mark.parametrize("dtype", R.SIXTEEN)
def test_wgrad_parity_class_against_float64(dtype, case):
    """the parity-class kernel at 0, 128 and 1 target workgroups; the shapes it refuses run on the per-tap kernel"""
    targets = {c: t for c, t, _ in R.TN8_CASES}.get(case, (0,))
    for t in targets:
        for kind in ("int", "rand"):
            wgrad_run(case, dtype, kind, t)


# ---- 3. packing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_pack_kernels_give_the_restated_panels(dtype):
    """eg_pack_fwd, eg_pack_bwd and eg_pack_conv (both panels, and either one alone) into NaN-filled panels: the bits of panels_fwd /
    panels_bwd, zeros in the K padding, nothing outside the panel"""
    dt, tdt = types(dtype)
    for Cin, Cout, k, s, p in R.pack_keys(dtype):
        case = (1, 8, 8, Cin, Cout, k, s, p, 0)
        c = ops.make_conv(*case)
        w = R.operands(case, dtype, "rand")["w"]
        want = {"fwd": R.panels_fwd(w, case, dtype).to(tdt), "bwd": R.panels_bwd(w, case, dtype).to(tdt)}
        assert want["fwd"].numel() == ops.pack_fwd_elems(c, dt) and want["bwd"].numel() == ops.pack_bwd_elems(c, dt)
        for which in ("fwd", "bwd", "both", "conv_fwd", "conv_bwd"):
            wm = arena(w.shape, torch.float32, init=w)
            pf, pb = arena(want["fwd"].numel(), tdt), arena(want["bwd"].numel(), tdt)
            if which == "fwd":
                ops.pack_fwd(c, dt, wm[1], pf[1])
            elif which == "bwd":
                ops.pack_bwd(c, dt, wm[1], pb[1])
            else:
                ops.pack_conv(c, dt, wm[1], pf[1] if which != "conv_bwd" else None, pb[1] if which != "conv_fwd" else None)
            sync()
            assert intact([wm, pf, pb]), (case, which)
            for name, (_, view) in (("fwd", pf), ("bwd", pb)):
                if which in (name, "both", "conv_" + name):
                    assert same_bits(view, want[name].flatten()), (case, which, name)
                else:
                    assert bool(torch.isnan(view).all()), (case, which, name, "the other panel was touched")

"""The kernels of ``csrc/affine_loss.hip`` (all but ``eg_head_fused``) through ``ops`` against the float64 references of
tests/affine_refs.py, at the batch sizes, strides and edges the trainers launch them with.

Bound of every comparison: ``H.bound(yardstick)`` = max(K * yardstick, 4 float32 ulps) with K = 8 and the yardstick the error of the same
reference evaluated in float32 on the CPU on the same inputs (tests/test_affine_refs_host.py, which also shows that every mutant of the
references misses these bounds by a factor of 10 at least).  Every comparison prints ``error / yardstick`` (run with -s).

Largest error / max(yardstick, floor / K) observed on an MI355X (K = 8 allows 8; B, layout and n run over all cases):
  regularizers   rpqxy 2.6 (wide 4.2)   rp 2.6 (wide 3.2)   rp_color 3.6 (wide 3.2)   pxy 5.1 at B = 1 (wide 3.5)   pxy_color 1.3 (wide 2.0)
                 rpqmnxy 3.6            eg_loss_info_rpqxy 1.1      drop-in functions: rpqxy 1.6, rp 1.7, rp_color 1.4, rpqmnxy 3.2
  heads          bce 1.2   mse 1.9   ce 1.0   mutual information 1.7 (probabilities), 2.8 (logits)
  matrices       rpqxy 1.1   rpqmnxy 1.0   rp 1.3   pxy 1.0   pxy_align_inv 0.1   affine_para 1.0      color_scale 1.0 (u8_colorize: exact)
  warps          border 1.1   zeros 1.3   one-launch 1.0 (bit-equal to eg_theta_rpqxy + eg_warp_affine on every shape)
Nothing needed more than K = 8; the largest ratios belong to one-row cases, where the yardstick is the rounding luck of a single row.
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import affine_refs as R
import test_affine_refs_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 7.0
PRESET = 3.25
eg = None
ops = None
MLP_BLOB = None


def setup_module(module):
    global eg, ops, MLP_BLOB
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops
    MLP_BLOB = eg.mnist.load_approximator(H.mlp(), DEV)


def check(name, got, want, yard, rows=False, keep=None):
    fig = H.metric(got, want, rows, keep)
    print(f"{name}: error {fig:.3g}  yardstick {yard:.3g}  error / max(yardstick, floor / K) {fig / max(yard, H.FLOOR / H.K):.3g}  bound {H.bound(yard):.3g}")
    assert fig <= H.bound(yard), (name, fig, yard, H.bound(yard))


def embed(x, ld, c0, g):
    """x [B, n] as columns c0 .. c0 + n of a [B, ld] device tensor whose other columns hold noise the kernel must not read"""
    full = torch.randn(x.shape[0], ld, generator=g) * 3
    full[:, c0:c0 + x.shape[1]] = x
    return full.to(DEV)


# ---- regularizers ------------------------------------------------------------------------------------------------------------------------
def launch_reg(kind, o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred):
    if kind == "rpqxy":
        ops.loss_affine_rpqxy(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred)
    elif kind == "rp":
        ops.loss_affine_rp(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred)
    elif kind == "rp_color":
        ops.loss_affine_rp_color(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred)
    elif kind in ("pxy", "pxy_color"):
        ops.loss_affine_pxy(o_real, o_trans, ld, c0, B, code, ldc, scale, loss, d_real, d_trans, pred, ncol=3 if kind == "pxy_color" else 0)
    else:
        ops.loss_affine_rpqmnxy(o_real, o_trans, ld, c0, B, code, ldc, MLP_BLOB, scale, loss, d_real, d_trans, pred, torch.empty(B, device=DEV))


def layouts(n):
    """(ld, c0, ldc): contiguous rows; the CelebA head's 19-wide rows with the codes from column 1 and its 8-wide code rows; a third with
    other offsets and a code stride above the code width"""
    return {"contiguous": (n, 0, n), "head19": (19, 1, max(n, 8)), "padded": (n + 3, 2, n + 4)}


REG_CASES = [(k, w) for k in H.REG_KINDS for w in (False, True) if not w or k in H.WIDE_KINDS]


@pytest.mark.parametrize("layout", ["contiguous", "head19", "padded"])
@pytest.mark.parametrize("B", H.REG_B)
@pytest.mark.parametrize("kind,wide", REG_CASES)
def test_affine_regularizer(kind, wide, B, layout):
    """eg_loss_affine_rpqxy / _rp / _rp_color / _pxy (ncol 0, 3) / _rpqmnxy: value, pred and both gradient blocks against float64; the
    columns outside the codes cleared; loss added to; the loss-only and the pred-less calls; two calls give the same bits."""
    n = R.REGS[kind][1]
    ld, c0, ldc = layouts(n)[layout]
    real, trans, code, keep = H.reg_inputs(kind, B, wide)
    truth, yard = H.reg_truth(kind, B, wide), H.reg_yardstick(kind, B, wide)
    g = H._gen("embed", kind, wide, B, layout)
    o_real, o_trans, codes = embed(real, ld, c0, g), embed(trans, ld, c0, g), embed(code, ldc, 0, g)

    def call(preset, grads=True, pred=True):
        loss = torch.full((3,), preset, device=DEV)
        d_real = torch.full((B, ld), SENTINEL, device=DEV) if grads else None
        d_trans = torch.full((B, ld), SENTINEL, device=DEV) if grads else None
        p = torch.full((B, n), SENTINEL, device=DEV) if pred else None
        launch_reg(kind, o_real, o_trans, ld, c0, B, codes, ldc, H.SCALE, loss[1:2], d_real, d_trans, p)
        torch.cuda.synchronize()
        return loss.cpu(), d_real, d_trans, p

    loss, d_real, d_trans, pred = call(0.0)
    tag = f"{kind}{' wide' if wide else ''} B={B} {layout}"
    assert float(loss[0]) == 0.0 and float(loss[2]) == 0.0
    if "value" in yard:
        check(tag + " value", loss[1:2], truth["value"].reshape(1), yard["value"])
    check(tag + " pred", pred, truth["pred"], yard["pred"], keep=keep)
    for name, d in (("d_real", d_real), ("d_trans", d_trans)):
        check(f"{tag} {name}", d[:, c0:c0 + n], truth[name], yard[name], rows=True, keep=keep)
        outside = torch.cat((d[:, :c0], d[:, c0 + n:]), 1)
        assert float(outside.abs().max()) == 0.0 if outside.numel() else True, f"{tag}: {name} columns outside the codes are not cleared"
        assert not bool((d[:, c0:c0 + n] == SENTINEL).any()), f"{tag}: {name} keeps the sentinel"
    # the same call again: the same bits
    loss2, d_real2, d_trans2, pred2 = call(0.0)
    assert torch.equal(loss, loss2) and torch.equal(d_real, d_real2) and torch.equal(d_trans, d_trans2) and torch.equal(pred, pred2)
    # loss is added to: preset + value in float32, exactly
    loss3, d_real3, d_trans3, _ = call(PRESET, pred=False)
    assert torch.equal(loss3, torch.tensor([PRESET, np.float32(PRESET) + loss[1].numpy(), PRESET])), (loss3, loss)
    assert torch.equal(d_real3, d_real) and torch.equal(d_trans3, d_trans)
    # the drop-in modules' forward: no gradients, no loss
    loss4, _, _, pred4 = call(0.0, grads=False)
    assert torch.equal(loss4, loss) and torch.equal(pred4, pred)
    p5 = torch.full((B, n), SENTINEL, device=DEV)
    launch_reg(kind, o_real, o_trans, ld, c0, B, codes, ldc, H.SCALE, None, None, None, p5)
    torch.cuda.synchronize()
    assert torch.equal(p5, pred)


@pytest.mark.parametrize("B", [37, 128, 300])
def test_info_losses_in_one_launch_against_float64(B):
    """eg_loss_info_rpqxy: lcon * MSE(cont, code) + lcat * CE(softmax(cat), labels) on D(gen), laff * MSE(regularizer(D(real), D(trans)),
    code[:, :5]) -- the float64 sum of the three references (yardstick: the same sum in float32)."""
    cd, nc, ld, c0 = 8, 10, 19, 1
    lcat, lcon, laff = (float(np.float32(v)) for v in (1.3, 0.7, 0.9))
    real, trans, code5, keep = H.reg_inputs("rpqxy", B, False)
    g = H._gen("info", B)
    code = torch.cat((code5, H._uniform(g, (B, cd - 5), 1.0)), 1)
    gen = torch.randn(B, ld, generator=g) * 2
    labels = torch.randint(0, nc, (B,), generator=g)
    o_real, o_trans = embed(real, ld, c0, g), embed(trans, ld, c0, g)

    def refs(cast):
        mse = R.head_eval("mse", cast(gen[:, c0:c0 + cd]), lcon, tgt=cast(code))
        ce = R.head_eval("ce", cast(gen[:, c0 + cd:c0 + cd + nc]), lcat, labels=labels)
        aff = R.reg_eval("rpqxy", cast(real), cast(trans), cast(code5), laff)
        d_gen = torch.zeros(B, ld, dtype=mse["dout"].dtype)
        d_gen[:, c0:c0 + cd] = mse["dout"]
        d_gen[:, c0 + cd:c0 + cd + nc] = ce["dout"]
        return {"value": (mse["value"] + ce["value"] + aff["value"]).reshape(1), "d_gen": d_gen, "d_real": aff["d_real"], "d_trans": aff["d_trans"]}
    want, own = refs(lambda t: t.double()), refs(lambda t: t)
    loss = torch.full((3,), PRESET, device=DEV)
    loss[1] = 0
    d = torch.full((3 * B, ld), SENTINEL, device=DEV)
    ops.loss_info_rpqxy(gen.to(DEV), o_trans, o_real, ld, c0, cd, nc, B, code.to(DEV), cd, labels.to(DEV), lcat, lcon, laff, loss[1:2], d[:B], d[B:2 * B],
                        d[2 * B:])
    torch.cuda.synchronize()
    assert float(loss[0]) == PRESET and float(loss[2]) == PRESET
    tag = f"info B={B}"
    check(tag + " value", loss[1:2], want["value"], H.metric(own["value"], want["value"]))
    # d_gen: the MSE and the CE columns are separate rows of separate scales
    for name, sl in (("d_gen mse", slice(c0, c0 + cd)), ("d_gen ce", slice(c0 + cd, c0 + cd + nc))):
        check(f"{tag} {name}", d[:B, sl], want["d_gen"][:, sl], H.metric(own["d_gen"][:, sl], want["d_gen"][:, sl], rows=True), rows=True)
    assert float(d[:B, :c0].abs().max()) == 0.0
    for name, blk in (("d_trans", d[B:2 * B]), ("d_real", d[2 * B:])):
        check(f"{tag} {name}", blk[:, c0:c0 + 5], want[name], H.metric(own[name], want[name], rows=True), rows=True)
        assert float(blk[:, :c0].abs().max()) == 0.0 and float(blk[:, c0 + 5:].abs().max()) == 0.0


# ---- drop-in autograd functions ----------------------------------------------------------------------------------------------------------
def dropin(kind):
    return {"rpqxy": eg.celeba.affine_regularzier, "rp": eg.dsprites.affine_regularzier, "rp_color": eg.colored.affine_color_regularzier,
            "rpqmnxy": eg.mnist.affine_regularizer}[kind]


@pytest.mark.parametrize("upstream", [1.0, 1e-3, 1e-6])
@pytest.mark.parametrize("kind,B", [("rpqxy", 128), ("rp", 128), ("rp_color", 512), ("rpqmnxy", 256)])
def test_dropin_regularizers_against_float64_autograd(kind, B, upstream):
    """``affine_regularzier(real, trans)`` of the four drop-in modules under autograd with a random upstream gradient of size ``upstream``.
    Their backward hands the MSE kernel the target pred - dpred * UP * (n B / 2) and the scale 1 / UP (UP = 2^32), so that the kernel
    recovers dpred * UP * n B / 2 as a float32 difference: relative error about 2^-24 * |pred| / (UP * |dpred| * n B / 2), far below float32
    rounding for every upstream gradient down to 1e-9.  (With UP = 1, as before, that is 2e-4 at |dpred| = 1e-6 and B = 128.)"""
    n = R.REGS[kind][1]
    real, trans, _, _ = H.reg_inputs(kind, B, False)
    w = (torch.randn(B, n, generator=H._gen("dropin", kind)) * upstream).float()
    want = R.reg_vjp(kind, real.double(), trans.double(), w.double(), H.mlp())
    own = R.reg_vjp(kind, real, trans, w, H.mlp())
    rc, tc = real.to(DEV).requires_grad_(True), trans.to(DEV).requires_grad_(True)
    pred = dropin(kind)(rc, tc)
    (pred * w.to(DEV)).sum().backward()
    tag = f"drop-in {kind} B={B} upstream={upstream:g}"
    print(f"{tag}: 2^-24 |pred| / (|dpred| n B / 2) = {2.0 ** -24 * float(pred.detach().abs().mean()) / (float(w.abs().mean()) * n * B / 2):.3g} before the 2^32")
    check(tag + " pred", pred, want["pred"], H.metric(own["pred"], want["pred"]))
    check(tag + " d_real", rc.grad, want["d_real"], H.metric(own["d_real"], want["d_real"], rows=True), rows=True)
    check(tag + " d_trans", tc.grad, want["d_trans"], H.metric(own["d_trans"], want["d_trans"], rows=True), rows=True)


# ---- loss heads ------------------------------------------------------------------------------------------------------------------------------
def launch_head(kind, o, ld, c0, n, B, kw, loss, dout, zero_rows=True):
    if kind == "bce":
        ops.loss_bce_sigmoid(o, ld, c0, B, kw["target"], H.SCALE, loss, dout, zero_rows)
    elif kind == "mse":
        tgt = kw.get("tgt")
        ops.loss_mse(o, ld, c0, n, B, tgt, tgt.shape[1] if tgt is not None else 0, kw.get("target", 0.0), H.SCALE, loss, dout, zero_rows)
    elif kind == "ce":
        ops.loss_ce_softmaxed(o, ld, c0, n, B, kw["labels"], H.SCALE, loss, dout)
    else:
        ops.loss_mutual_info(o, ld, c0, n, B, kw["tgt"], kw["tgt"].shape[1], 1, kw["target_logits"], H.SCALE, loss, dout)


@pytest.mark.parametrize("B", H.HEAD_B)
@pytest.mark.parametrize("kind,n,variant", H.HEAD_CASES)
def test_loss_head(kind, n, variant, B):
    """eg_loss_bce_sigmoid (zero_rows both ways), eg_loss_mse (tensor / constant target, zero_rows both ways), eg_loss_ce_softmaxed and
    eg_loss_mutual_info (both ADD to dout) on 19-wide rows: value and gradient against float64, the other columns untouched or cleared."""
    ld, c0 = 19, 2
    kw = H.head_inputs(kind, n, variant, B)
    truth, yard = H.head_truth(kind, n, variant, B), H.head_yardstick(kind, n, variant, B)
    g = H._gen("head-embed", kind, n, variant, B)
    o = embed(kw["o"], ld, c0, g)
    dkw = {k: v for k, v in kw.items() if k != "o"}
    if kind == "mi":
        dkw["tgt"] = embed(kw["tgt"], n + 2, 1, g)            # ldt = n + 2, t0 = 1
    elif "tgt" in dkw:
        dkw["tgt"] = dkw["tgt"].to(DEV)
    if "labels" in dkw:
        dkw["labels"] = dkw["labels"].to(DEV)
    tag = f"{kind} n={n} {variant} B={B}"
    adds = kind in ("ce", "mi")
    prefill = torch.randn(B, ld, generator=g).to(DEV)
    for zero_rows in ((True,) if adds else (True, False)):
        loss = torch.tensor([PRESET, 0.0, PRESET], device=DEV)
        dout = prefill.clone()
        launch_head(kind, o, ld, c0, n, B, dkw, loss[1:2], dout, zero_rows)
        torch.cuda.synchronize()
        assert float(loss[0]) == PRESET and float(loss[2]) == PRESET
        check(tag + " value", loss[1:2], truth["value"].reshape(1), yard["value"])
        written = dout[:, c0:c0 + n]
        outside = torch.cat((dout[:, :c0], dout[:, c0 + n:]), 1)
        pre_out = torch.cat((prefill[:, :c0], prefill[:, c0 + n:]), 1)
        if adds:
            # dout = prefill + gradient in float32: the rounding of that sum (half an ulp of the sum) is not the kernel's error
            grad = written.double() - prefill[:, c0:c0 + n].double()
            slack = (written.abs().amax(1) * 2.0 ** -24 / truth["dout"].abs().amax(1).to(DEV)).max().item()
            fig = H.metric(grad, truth["dout"], rows=True)
            print(f"{tag} dout (added): error {fig:.3g}  yardstick {yard['dout']:.3g}  rounding of the sum {slack:.3g}")
            assert fig <= H.bound(yard["dout"]) + slack, (tag, fig, yard["dout"], slack)
            assert torch.equal(outside, pre_out)
            # and into a zero buffer, where the sum is exact
            dz = torch.zeros(B, ld, device=DEV)
            launch_head(kind, o, ld, c0, n, B, dkw, torch.zeros(1, device=DEV), dz)
            torch.cuda.synchronize()
            check(tag + " dout", dz[:, c0:c0 + n], truth["dout"], yard["dout"], rows=True)
        else:
            check(f"{tag} dout zero_rows={zero_rows}", written, truth["dout"], yard["dout"], rows=True)
            assert torch.equal(outside, torch.zeros_like(outside) if zero_rows else pre_out)
        # loss is added to, and a second call gives the same bits
        loss2 = torch.tensor([PRESET, PRESET, PRESET], device=DEV)
        d2 = prefill.clone()
        launch_head(kind, o, ld, c0, n, B, dkw, loss2[1:2], d2, zero_rows)
        torch.cuda.synchronize()
        assert float(loss2[1]) == float(np.float32(PRESET) + loss[1].cpu().numpy()) and torch.equal(d2, dout)
    lossonly = torch.zeros(1, device=DEV)
    launch_head(kind, o, ld, c0, n, B, dkw, lossonly, None)
    torch.cuda.synchronize()
    assert float(lossonly) == float(loss[1])


@pytest.mark.parametrize("target", [0.0, 1.0])
def test_bce_on_saturated_logits(target):
    """logits of +-20 and +-90: sigmoid rounds to 0 or 1 in float32 and torch's clamps decide the result, so the reference here is torch's
    own float32 BCELoss(sigmoid(o)) with its autograd on the CPU, not float64.  Everything stays finite."""
    B = 257
    g = H._gen("saturated")
    o = (torch.randn(B, generator=g) * 2)
    o[::4] = torch.tensor([20.0, -20.0, 90.0, -90.0]).repeat(B)[:o[::4].numel()]
    oc = o.clone().requires_grad_(True)
    val = H.SCALE * F.binary_cross_entropy(torch.sigmoid(oc), torch.full((B,), target))
    (grad,) = torch.autograd.grad(val, oc)
    loss, dout = torch.zeros(1, device=DEV), torch.full((B, 1), SENTINEL, device=DEV)
    ops.loss_bce_sigmoid(o.to(DEV).view(B, 1), 1, 0, B, target, H.SCALE, loss, dout, True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dout).all())
    sat = torch.zeros(B, dtype=torch.bool)
    sat[::4] = True
    # the value: a float32 sum of 257 terms up to 100 against another float32 sum of the same terms: both within B * 2^-24 of the exact sum
    assert abs(float(loss) - float(val)) <= 2 * B * 2.0 ** -24 * max(1.0, abs(float(val))), (float(loss), float(val))
    got, want = dout.cpu()[:, 0], grad
    # every gradient entry is scale / B * (p - t), at most scale / B in size, and the device's sigmoid may differ from the CPU's by one
    # rounding of p (which 1 - p turns into an ABSOLUTE error of an ulp of 1): K roundings of the entry's scale scale / B
    tol = H.bound(H.ULP) * H.SCALE / B
    err = (got - want).abs()
    print(f"saturated bce target={target}: largest gradient error {float(err.max()):.3g}, on saturated rows {float(err[sat].max()):.3g}, tolerance {tol:.3g}")
    assert bool((err <= tol).all()), (got[sat][:8], want[sat][:8])


# ---- matrices and colour ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", H.MAT_B)
@pytest.mark.parametrize("kind", H.MATRIX_KINDS)
def test_code_to_matrix_kernels(kind, B):
    """eg_theta_rpqxy / _rpqmnxy / _rp / _pxy / _pxy_align_inv and eg_affine_para_rpqmnxy on codes that start at column 1 of 9-wide rows"""
    codes = H.matrix_inputs(kind, B).to(DEV)
    view = codes.view(-1)[1:]                                   # the kernel sees the row stride 9 and the first code at column 1
    out = torch.full((B, 7 if kind == "para_rpqmnxy" else 6), SENTINEL, device=DEV)
    fn = {"rpqxy": ops.theta_rpqxy, "rpqmnxy": ops.theta_rpqmnxy, "rp": ops.theta_rp, "pxy": ops.theta_pxy, "pxy_align_inv": ops.theta_pxy_align_inv,
          "para_rpqmnxy": ops.affine_para_rpqmnxy}[kind]
    fn(view, 9, B, out)
    torch.cuda.synchronize()
    check(f"matrix {kind} B={B}", out, H.matrix_truth(kind, B), H.matrix_yardstick(kind, B))


@pytest.mark.parametrize("shape", H.COLOR_SHAPES)
def test_colour_kernels(shape):
    """eg_color_scale (multiply and divide by code * 0.5 + 1, codes from column 4 of 9) under the yardstick rule; eg_u8_colorize exactly:
    an 8-bit integer times a float32 gain is ONE float32 rounding of an exact product (the float64 product is exact: 8 + 24 bits), so the
    kernel's output equals the float64 reference rounded to float32, bit for bit -- within half an ulp of the exact value."""
    B, C, HW = shape
    x, code, sprites, gain = H.color_inputs(shape)
    for divide in (False, True):
        out = torch.full(shape, SENTINEL, device=DEV)
        ops.color_scale(x.to(DEV), code.to(DEV), 9, 4, 0.5, divide, out, B, C, HW)
        torch.cuda.synchronize()
        check(f"color_scale {shape} divide={divide}", out, R.color_scale(x.double(), code.double(), 4, 0.5, divide), H.color_yardstick(shape, divide))
    out = torch.full(shape, SENTINEL, device=DEV)
    ops.u8_colorize(sprites.to(DEV), gain.to(DEV), out, B, C, HW)
    torch.cuda.synchronize()
    exact = R.u8_colorize(sprites, gain.double())
    assert torch.equal(out.cpu(), exact.float())
    assert bool(((out.cpu().double() - exact).abs() <= 0.5 * H.ULP * exact.abs()).all())          # half an ulp (ulp(x) <= 2^-23 |x|)


# ---- warps ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.WARP_SHAPES)
def test_warps(shape):
    """eg_warp_affine (border), eg_warp_affine_zeros and eg_warp_affine_rpqxy against float64 grid_sample, element by element; the one-launch
    form is the two stand-alone launches bit for bit and clears its ``zero`` buffer; it refuses H * W that is not a multiple of 256."""
    B, C, Hh, W = shape
    img, code, th = H.warp_inputs(shape)
    dimg, dcode, dth = img.to(DEV), code.to(DEV), th.to(DEV)
    outs = {}
    for mode, fn in (("border", ops.warp_affine), ("zeros", ops.warp_affine_zeros)):
        out = torch.full(shape, SENTINEL, device=DEV)
        fn(dimg, dth, out, B, C, Hh, W)
        torch.cuda.synchronize()
        check(f"warp {mode} {shape}", out, H.warp_truth(shape, mode), H.warp_yardstick(shape, mode))
        outs[mode] = out
    if min(B, 5) == 5:
        assert torch.equal(outs["zeros"][4], torch.zeros_like(outs["zeros"][4]))          # the far shift: every tap outside
    theta_out, out, zero = torch.full((B, 6), SENTINEL, device=DEV), torch.full(shape, SENTINEL, device=DEV), torch.full((5,), SENTINEL, device=DEV)
    if (Hh * W) % 256:
        with pytest.raises(RuntimeError, match="multiple of 256"):
            ops.warp_affine_rpqxy(dimg, dcode, 8, theta_out, out, B, C, Hh, W, zero)
        ops.clear_errors()
        return
    ops.warp_affine_rpqxy(dimg, dcode, 8, theta_out, out, B, C, Hh, W, zero)
    th2, out2 = torch.empty(B, 6, device=DEV), torch.empty(shape, device=DEV)
    ops.theta_rpqxy(dcode, 8, B, th2)
    ops.warp_affine(dimg, th2, out2, B, C, Hh, W)
    torch.cuda.synchronize()
    assert float(zero.abs().max()) == 0.0
    check(f"warp fused {shape}", out, H.warp_truth(shape, "fused"), H.warp_yardstick(shape, "fused"))
    check(f"warp fused theta {shape}", theta_out, R.theta(R.matrix_rpqxy(code[:, :5].double())).reshape(B, 6),
          H.metric(R.theta(R.matrix_rpqxy(code[:, :5])).reshape(B, 6), R.theta(R.matrix_rpqxy(code[:, :5].double())).reshape(B, 6)))
    assert torch.equal(theta_out, th2), "theta of the one-launch warp differs from eg_theta_rpqxy"
    diff = (out != out2).nonzero()
    assert diff.numel() == 0, f"one-launch warp differs from theta + warp at {diff.shape[0]} elements, first {diff[:4].tolist()}"

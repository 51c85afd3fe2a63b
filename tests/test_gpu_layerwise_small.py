"""Layer-wise teacher forcing of the dSprites / colored dSprites networks at the batch sizes they are benchmarked at (dSprites B = 128 bf16,
colored dSprites B = 512 fp16: BASELINE configs[4]).  The full-size tests of test_gpu_fullsize.py hold these configurations only to whole-network
bounds (0.25 / 0.1) against the fp32 oracle; a kernel that moved one layer by a few percent would pass them.  Here the trainer's own engines
(D.engine(B), E.engine(B), G.engine(B)) run one forward and one backward, every layer's operands are taken from the engine's own buffers, and
each kernel's output is compared with plain torch arithmetic (tests/layer_refs.py: unfold / fold + matmul) on the same rounded operands.

Bounds (relative L2 unless said otherwise; the worst measured value of each is recorded with the change that set it):

  forward / backward-data (16-bit outputs): one rounding of the output, relative L2 2^-t / sqrt(3) with t = 9 (bf16) / 12 (fp16), plus fp32
      summation order: 6e-3 for bf16 (as the CelebA layer-wise test), 2e-3 for fp16.
  weight gradients, checked PER TAP, bias gradients, BatchNorm batch / running statistics and gamma / beta gradients: references in fp64 from
      the same stored 16-bit operands, with the spectral-norm rank-1 term built from the engine's OWN coef / u / v (the coefficient is checked
      on its own, below).  The MFMA products of 16-bit operands are exact in fp32 and the fused epilogue sums (EG_STAT_SN_BIAS / BN_BWD) see
      the values that are stored; only fp32 summation order remains: WGRAD_TOL = 2e-5.  The conv biases in front of the generator's
      BatchNorms have a gradient that is zero up to rounding: their error is taken relative to the absolute column sums.
  spectral-norm coefficient coef[t] = <G_t, W_orig> / sigma_t^2 (G_t = dL/dW of tape t = sigma_t dzs_t x_t^T) against its definition
      computed in fp64 from W_orig.  The kernels rebuild it from the stored 16-bit activation (LeakyReLU inverted: z - bias), so every term
      dzs (z - b) carries a rounding of dzs and of the activation, and z itself one of the weights the forward used.  coef is a signed sum
      of many terms, so the error is measured in units of the scale of that noise, rms = sqrt(2 sum (dzs z)^2 + sum (W_orig Gs)^2 / sigma^2):
      independent roundings of relative size <= u/2 (u = 2^-8 bf16, 2^-11 fp16) give an error of about 0.3 u rms.  COEF_TOL = 2u.  It bites:
      the test asserts the bound is below |coef_ref[t]| / rms (coef = 0 or of the wrong sign) and below |coef_ref[t] - coef_ref[t']| / rms
      (another tape's coefficient).
  sigma_t against u_t^T W_orig v_t in fp64: a few fp32 ulps of the power iteration: SIGMA_TOL = 2e-7.  It bites: below the relative
      difference between the sigma of W_orig and of its 16-bit rounding, asserted for every layer and tape.

Each weight-gradient bound must be able to bite: from the layer's slab and its reference the test computes how far the gradient would move if
the reduction dropped one split, left out the rank-1 term, transposed (kh, kw) or (generator fc2) left the rows in the panel's order, and
asserts the bound is below the smallest of these.  The split count of every weight-gradient launch is asserted as well.  (The
per-tap maximum of a perturbation's relative error is at least its whole-layer relative error, so such a mutant fails the per-tap check.)"""
import importlib

import pytest
import torch
import torch.nn.functional as F

import test_gpu_colored as tco
import test_gpu_dsprites as tds
from layer_refs import _conv_ref, _convT_ref, _linear_ref, _linear_wgrad_ref, _lrelu_mask, _rel, _sn_rank1, _sn_sigma, _wgrad_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None
ops = None
F64 = torch.float64

FWD_TOL = {"bf16": 6e-3, "f16": 2e-3}
WGRAD_TOL = 2e-5
COEF_TOL = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}
SIGMA_TOL = 2e-7
SLOPE = 0.2                     # LeakyReLU of the dSprites trunks (dSprites/rp.py:95-110)

# (module of the network helpers, compute dtype, batch, image channels, tapes of D / E)
CONFIGS = {"dsprites_b128_bf16": (tds, "bf16", 128, 1), "colored_b512_fp16": (tco, "f16", 512, 3)}
# weight-gradient splits: the trunks' layers 1..3 and the generator's three transposed convolutions (parity-class kernel, eg_tn8_plan: about 256
# workgroups, >= 4 K steps per split; the dSprites generator's first one, 8 splits, is the only one on the lean reduction), the SN-Linear layers,
# the combined heads, the generator's fc2 and last layer (per-tap kernel, tn_plan); eg_wgrad_img (trunk layer 0, the generator's last layer in its
# image-direct form) runs min(8 x images, 1024) splits
SPLITS = {"dsprites_b128_bf16": {"D": (64, 32, 16), "E": (64, 32, 24), "G": (8, 32, 64), "D.fc": (1,), "E.fc": (1, 1), "D.head": 1, "E.head": 1,
                                 "G.fc2": 1, "G.convT3": 512},
          "colored_b512_fp16": {"D": (64, 32, 64), "E": (64, 32, 64), "G": (32, 64, 64), "D.fc": (4,), "E.fc": (6, 6), "D.head": 4, "E.head": 6,
                                "G.fc2": 2, "G.convT3": 512}}
TAPES = {"D": 2, "E": 3}


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops
    for m in (tco, tds):
        m.setup_module(m)


class Checks:
    """every comparison of a test, reported together (the worst value of each kind is what the bounds are set from)"""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def err(self, name, err, bound):
        self.rows.append((name, float(err), float(bound), "err"))

    def bite(self, name, bound, margins, assert_=True):
        """the bound is below every perturbation's error (margins: {mutation: error it would cause, in the units of the bound});
        ``assert_=False``: a figure that is only reported"""
        m = min(margins.values())
        self.rows.append((name + " can bite (" + ", ".join(f"{k} {v:.3g}" for k, v in margins.items()) + ")", float(bound), m,
                          "bite" if assert_ else "figure"))

    def split(self, name, ns, expected):
        """the weight-gradient launch split its rows as the planner is expected to at this size"""
        self.rows.append((name, ns, expected, "split"))

    def finish(self):
        print(f"\n[{self.tag}]")
        worst = {}                                  # per kind: the largest error / bound (or bound / smallest mutant error)
        for name, e, b, kind in self.rows:
            if kind in ("figure", "split"):
                continue
            key = (kind, name.split(" ")[0], b) if kind == "err" else kind
            if e / b > worst.get(key, (-1.0, ""))[0]:
                worst[key] = (e / b, f"{name}: {e:.3g} < {b:.3g}")
        for _, line in sorted(worst.values(), key=lambda x: -x[0]):
            print("  " + line)
        for name, e, b, kind in self.rows:
            if kind == "split":
                print(f"  split: {name}: nsplit {e} (expected {b})")
            elif kind != "err":
                print(f"  {kind}: {name}: {e:.3g} < {b:.3g}")
        bad = [r for r in self.rows if (r[3] == "split" and r[1] != r[2]) or (r[3] in ("err", "bite") and not r[1] < r[2])]
        assert not bad, bad


def nchw(t):
    return t.permute(0, 3, 1, 2)


def per_tap(ck, name, got, ref, bound):
    """per-tap relative error of a [N][C][k][k] (or [N][C][taps]) gradient; reports the worst tap"""
    g, r = got.reshape(got.shape[0], got.shape[1], -1), ref.reshape(ref.shape[0], ref.shape[1], -1)
    e = max(_rel(g[:, :, t], r[:, :, t]) for t in range(r.shape[2]))
    ck.err(name, e, bound)


def slab_margins(slab, ref, T, C, rank1=None, crow=None):
    """relative L2 errors of two mutants of a reduction into ``ref`` ([N][crow][T] in master order) from ``slab`` ([split][N][T][C]): one split
    dropped, the rank-1 term left out"""
    ns, N = slab.shape[0] // (ref.shape[0] * T * C), ref.shape[0]
    crow = crow or C
    s = slab.reshape(ns, N, T, C)[:, :, :, :crow].permute(0, 1, 3, 2).to(F64)          # [split][n][c][t]
    rn = ref.reshape(N, crow, T).norm()
    out = {"drop a split": float(min(s[z].norm() for z in range(ns)) / rn)}
    if rank1 is not None:
        out["no rank-1"] = float(rank1.norm() / rn)
    return out


def transposed(ref):
    """relative L2 error of the gradient with (kh, kw) swapped ([N][C][k][k])"""
    return {"(kh,kw) transposed": _rel(ref.transpose(2, 3), ref)}


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _check_trunk(ck, name, mod, eng, imgs, douts, dt_name, dt, B):
    T = len(imgs)
    tdt = ops.torch_dtype(dt)
    fwd = FWD_TOL[dt_name]
    q = lambda w: w.detach().to(tdt).float()
    assert eng.img_direct and eng.wgrad_direct, (eng.img_direct, eng.wgrad_direct)
    eng.forward(imgs)
    grad = torch.zeros_like(mod.arena.grad)
    dimg = eng.backward(0, T, douts, grad, need_wgrad=True, need_dimg=True)
    torch.cuda.synchronize()
    gof = lambda k: mod.arena.grad_of(k, grad)
    tp = lambda buf, t: buf[t * B:(t + 1) * B]
    ws = eng.ws
    convs, L = eng.convs, eng.L
    fused = {i: bool(eng._stat.get((i, T), (0, None))[0]) for i in range(L)}
    imq = [im.to(tdt).float() for im in imgs]

    def sn_checks(lname, Wo, sig, u, v, coef, Gs, act_var):
        """sigma_t = u_t^T W_orig v_t; coef[t] = <G_t, W_orig> / sigma_t^2 = <Gs_t, W_orig> / sigma_t (Gs_t = G_t / sigma_t: the gradient of the
        tape's dzs), its error in units of the rounding noise's scale rms_t (coef_rms); can it bite: the bound is below |coef_ref[t]| (coef = 0,
        or of the wrong sign) and below |coef_ref[t] - coef_ref[t']| (another tape's coefficient)"""
        Wd = Wo.reshape(Gs[0].shape).to(F64)
        c_ref = [float((Gs[t] * Wd).sum()) / float(sig[t]) for t in range(T)]
        for t in range(T):
            s_ref = _sn_sigma(Wo, u[t], v[t])
            ck.err(f"sigma {lname} t{t}", abs(float(sig[t]) - s_ref) / abs(s_ref), SIGMA_TOL)
            ck.bite(f"sigma {lname} t{t}", SIGMA_TOL, {"sigma of the 16-bit weights": abs(_sn_sigma(q(Wo), u[t], v[t]) - s_ref) / abs(s_ref)})
            rms = coef_rms(act_var[t], Wd, Gs[t], sig[t])
            ck.err(f"coef {lname} t{t}", abs(float(coef[t]) - c_ref[t]) / rms, COEF_TOL[dt_name])
            m = {"coef = 0": abs(c_ref[t]) / rms}
            if T > 1:
                m["another tape's coef"] = min(abs(c_ref[t] - c_ref[k]) for k in range(T) if k != t) / rms
            ck.bite(f"coef {lname} t{t}", COEF_TOL[dt_name], m)

    def act_var(dzs, z):
        """sum (dzs z)^2: the scale of the rounding noise of dzs and of the stored activation in coef = sum dzs (z - b)"""
        return float(((dzs.to(F64) * z.to(F64)) ** 2).sum())

    def coef_rms(av, Wd, Gs, sig):
        """sqrt(2 sum (dzs z)^2 + sum (W_orig Gs)^2 / sigma^2): one rounding of dzs and of the activation per term, one of each weight (the forward
        used the 16-bit weights); independent rounding errors of relative size <= u / 2 give coef an error of about 0.3 u rms"""
        return (2 * av + float(((Wd * Gs) ** 2).sum()) / float(sig) ** 2) ** 0.5

    # ---- convolution layers: forward, backward-data, SN pieces, weight / bias gradients ----
    for i in range(L):
        c = convs[i]
        Wo, Wq, b = c.weight_orig.detach(), q(c.weight_orig), c.bias.detach()
        Gs, avs = [], []
        for t in range(T):
            x = imq[t] if i == 0 else nchw(tp(eng.a[i - 1], t)).float()
            pre = _conv_ref(x, Wq)[0]
            z = pre / eng.sigma[i][t] + b[None, :, None, None]
            ref = F.leaky_relu(z, SLOPE)
            ck.err(f"fwd {name}.conv{i} t{t}", _rel(nchw(tp(eng.a[i], t)), ref), fwd)
            dzs = nchw(tp(eng.dz[i], t))
            if i > 0:
                back = _convT_ref(dzs.float(), Wq, x.shape[-2:]) * _lrelu_mask(x, SLOPE) / eng.sigma[i - 1][t]
                ck.err(f"bwd-data {name}.conv{i}->conv{i - 1} t{t}", _rel(nchw(tp(eng.dz[i - 1], t)), back), fwd)
            elif t == 0:
                ck.err(f"bwd-data {name}.dimg", _rel(dimg, _convT_ref(dzs.float(), Wq, x.shape[-2:])), fwd)
            Gs.append(_wgrad_ref(dzs, x).reshape(Wo.shape[0], -1))
            avs.append(act_var(dzs, z))
            del x, pre, z, ref, dzs
        sn_checks(f"{name}.conv{i}", Wo, eng.sigma[i], eng.u[i], eng.v[i], eng.coef[i], Gs, avs)
        r1 = _sn_rank1(eng.coef[i][:T], eng.u[i][:T], eng.v[i][:T])
        ref = (sum(Gs) - r1).reshape(Wo.shape)
        got = gof(eng.conv_names[i] + ".weight_orig").view(Wo.shape)
        per_tap(ck, f"wgrad {name}.conv{i}", got, ref, WGRAD_TOL)
        gb = sum(float(eng.sigma[i][t]) * nchw(tp(eng.dz[i], t)).to(F64).sum((0, 2, 3)) for t in range(T))
        ck.err(f"bias{'(fused)' if fused[i] else ''} {name}.conv{i}", _rel(gof(eng.conv_names[i] + ".bias"), gb), WGRAD_TOL)
        # dispatch: the split count of the weight-gradient launch and the reduction it feeds; can the bound bite?
        if i == 0:
            ns = ops.wgrad_img(dt, imgs, eng._sl(eng.dz[0], 0), ws.slab, B, eng.in_ch, eng.S, eng.S, eng.W[0])
            ck.split(f"{name}.conv0 (eg_wgrad_img)", ns, 1024)
            Ct, taps = eng.kp, 1
        else:
            ns = ops.conv_wgrad(eng.geo[T]["mid"][i - 1], dt, eng._inp(i, 0), eng._sl(eng.dz[i], 0), ws.slab, ws.wgs_target)
            ck.split(f"{name}.conv{i}", ns, SPLITS[ck.tag][name][i - 1])
            Ct, taps = eng.W[i - 1], 16
        torch.cuda.synchronize()
        slab = ws.slab[:ns * eng.W[i] * taps * Ct]
        ck.bite(f"wgrad {name}.conv{i} (nsplit {ns})", WGRAD_TOL, slab_margins(slab, ref, taps, Ct, r1, eng.k0 if i == 0 else None) | transposed(ref))
        del Gs, ref, got, slab

    # ---- hidden SN-Linear layers (the first over the NCHW-flattened 4x4x64 map) ----
    nf = len(eng.fcs)
    xs = [torch.cat([nchw(tp(eng.a[L - 1], t)).reshape(B, -1) for t in range(T)]).float()]     # [T*B, 1024], column f = c*16 + hw
    for j in range(nf):
        f = eng.fcs[j]
        Wo, Wq = f.weight_orig.detach(), q(f.weight_orig)
        x = xs[j]
        Gs, avs = [], []
        for t in range(T):
            z = _linear_ref(tp(x, t), Wq, f.bias.detach(), eng.fsigma[j][t])
            ref = F.leaky_relu(z, SLOPE)
            ck.err(f"fwd {name}.fc{j} t{t}", _rel(tp(eng.fa[j], t), ref), fwd)
            dzs = tp(eng.fdz[j], t)
            back = dzs.float() @ Wq
            if j > 0:
                back = back * _lrelu_mask(tp(eng.fa[j - 1], t), SLOPE) / eng.fsigma[j - 1][t]
                ck.err(f"bwd-data {name}.fc{j}->fc{j - 1} t{t}", _rel(tp(eng.fdz[j - 1], t), back), fwd)
            else:
                a3 = nchw(tp(eng.a[L - 1], t))
                back = back.reshape(a3.shape) * _lrelu_mask(a3, SLOPE) / eng.sigma[L - 1][t]
                ck.err(f"bwd-data {name}.fc0->conv{L - 1} t{t}", _rel(nchw(tp(eng.dz[L - 1], t)), back), fwd)
            Gs.append(_linear_wgrad_ref(dzs, tp(x, t)))
            avs.append(act_var(dzs, z))
        xs.append(eng.fa[j][:T * B].float())
        sn_checks(f"{name}.fc{j}", Wo, eng.fsigma[j], eng.fu[j], eng.fv[j], eng.fcoef[j], Gs, avs)
        r1 = _sn_rank1(eng.fcoef[j][:T], eng.fu[j][:T], eng.fv[j][:T])
        ref = sum(Gs) - r1
        taps = eng.hk * eng.hk if j == 0 else 1
        per_tap(ck, f"wgrad {name}.fc{j}", gof(eng.fc_names[j] + ".weight_orig").view(Wo.shape[0], -1, taps), ref.reshape(Wo.shape[0], -1, taps), WGRAD_TOL)
        gb = sum(float(eng.fsigma[j][t]) * tp(eng.fdz[j], t).to(F64).sum(0) for t in range(T))
        ck.err(f"bias {name}.fc{j}", _rel(gof(eng.fc_names[j] + ".bias"), gb), WGRAD_TOL)
        ns = ops.conv_wgrad(eng.geo[T]["fc"][j], dt, eng._inp(L, 0) if j == 0 else eng.fa[j - 1], eng.fdz[j], ws.slab, ws.wgs_target)
        torch.cuda.synchronize()
        ck.split(f"{name}.fc{j}", ns, SPLITS[ck.tag][name + ".fc"][j])
        C = eng.W[-1] if j == 0 else eng.fK[j]
        slab = ws.slab[:ns * eng.fN[j] * taps * C]
        ck.bite(f"wgrad {name}.fc{j} (nsplit {ns})", WGRAD_TOL, slab_margins(slab, ref, taps, C, r1)
                | (transposed(ref.reshape(ref.shape[0], C, 4, 4)) if j == 0 else {}))

    # ---- heads ----
    x = xs[-1]
    x16 = eng.fa[-1]
    dfeat = torch.zeros(T * B, eng.K, device=DEV)
    for h in eng.heads:
        if not h.compute:
            continue
        w = h.module.weight_orig if h.sn else h.module.weight
        Wo, Wq, hb = w.detach(), q(w), h.module.bias.detach()
        dout = douts[h.name]
        Gs, G32 = [], []
        for t in range(T):
            sig = eng.hsigma[h.name][t] if h.sn else None
            z = _linear_ref(tp(x, t), Wq, hb, sig)
            ck.err(f"fwd {name}.{h.name} t{t}", _rel(tp(eng.outs[h.name], t), z), fwd)
            dys = tp(eng.dys_t, t)[:, h.off:h.off + h.N]
            want = tp(dout, t) / (sig if h.sn else 1.0)
            ck.err(f"dys {name}.{h.name} t{t}", _rel(dys, want), fwd)
            dfeat[t * B:(t + 1) * B] += tp(eng.dys32, t)[:, h.off:h.off + h.N] @ Wq
            Gs.append(_linear_wgrad_ref(dys, tp(x, t)))
            d32 = tp(eng.dys32, t)[:, h.off:h.off + h.N]
            G32.append(_linear_wgrad_ref(d32, tp(x, t)))
        ref = sum(Gs)
        r1 = None
        if h.sn:
            sn_checks(f"{name}.{h.name}", Wo, eng.hsigma[h.name], eng.hu[h.name], eng.hv[h.name], eng.hcoef[h.name], G32, [0.0] * T)
            r1 = _sn_rank1(eng.hcoef[h.name][:T], eng.hu[h.name][:T], eng.hv[h.name][:T])
            ref = ref - r1
        ck.err(f"wgrad {name}.{h.name}", _rel(gof(h.name + (".weight_orig" if h.sn else ".weight")), ref.flatten()), WGRAD_TOL)
        ns = ops.conv_wgrad(eng.geo[T]["headw"], dt, x16, eng.dys_t, ws.slab, ws.wgs_target)
        torch.cuda.synchronize()
        ck.split(f"{name}.heads", ns, SPLITS[ck.tag][name + ".head"])
        slab = ws.slab[:ns * 32 * eng.K].view(ns, 32, eng.K)[:, h.off:h.off + h.N].reshape(-1)
        ck.bite(f"wgrad {name}.{h.name} (nsplit {ns})", WGRAD_TOL, slab_margins(slab, ref, 1, eng.K, r1))
        ck.err(f"bias {name}.{h.name}", _rel(gof(h.name + ".bias"), dout[:T * B].to(F64).sum(0)), WGRAD_TOL)
    for t in range(T):
        back = tp(dfeat, t) * _lrelu_mask(tp(eng.fa[-1], t), SLOPE) / eng.fsigma[-1][t]
        ck.err(f"bwd-data {name}.heads->fc{nf - 1} t{t}", _rel(tp(eng.fdz[-1], t), back), fwd)


def _trunk_inputs(mod, B, ch, T, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.rand(B, ch, 64, 64, generator=g).to(DEV) for _ in range(T)]
    douts = {h.name: torch.randn(T * B, h.N, generator=g).to(DEV) for h in mod.engine(B).heads if h.compute}
    return imgs, douts


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _check_generator(ck, G, ge, B, dt_name, dt, direct):
    tdt = ops.torch_dtype(dt)
    fwd = FWD_TOL[dt_name]
    q = lambda w: w.detach().to(tdt).float()
    cb = G.conv_block
    ws = ge.ws
    g = torch.Generator().manual_seed(11)
    labels = F.one_hot(torch.randint(0, G.n_classes, (B,), generator=g), G.n_classes).float().to(DEV)
    code = (torch.rand(B, G.code_dim, generator=g) * 2 - 1).to(DEV)
    dimg = torch.randn(B, G.channels, 64, 64, generator=g).to(DEV)
    bns = [cb[idx + 1] for idx in (0, 3, 6)]
    run0 = [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in bns]
    ge.forward(labels, code)
    ge.l4_direct = direct
    grad = torch.zeros_like(G.arena.grad)
    ge.backward(dimg, grad)
    torch.cuda.synchronize()
    gof = lambda k: G.arena.grad_of(k, grad)
    sfx = " (l4 direct)" if direct else ""
    # ---- forward ----
    inp = torch.cat((labels, code), 1).to(tdt).float()
    ck.err("fwd G.inp", _rel(ge.inp[:, :ge.cin], inp), fwd)
    W1, W2 = G.fc1[0].weight, G.fc2[0].weight
    a1 = ge.a1.float()
    ck.err("fwd G.fc1", _rel(a1, F.relu(_linear_ref(inp, q(W1), G.fc1[0].bias.detach()))), fwd)
    h = nchw(ge.h).float()                                                  # [B,64,4,4]: row f = c*16 + hw of fc2
    ck.err("fwd G.fc2 (permuted rows)", _rel(h, F.relu(_linear_ref(a1, q(W2), G.fc2[0].bias.detach())).view(B, 64, 4, 4)), fwd)
    xs = [h] + [nchw(a).float() for a in ge.a]
    zs = []
    for i, idx in enumerate((0, 3, 6)):
        bn = bns[i]
        z = nchw(ge.z[i]).float()
        zs.append(z)
        S = 8 << i
        ck.err(f"fwd G.convT{i}", _rel(z, _convT_ref(xs[i], q(cb[idx].weight), (S, S)) + cb[idx].bias.detach()[None, :, None, None]), fwd)
        zd = z.to(F64)
        mean, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
        ck.err(f"bn mean G.bn{i}", _rel(ge.mean[i], mean), WGRAD_TOL)
        ck.err(f"bn invstd G.bn{i}", _rel(ge.invstd[i], (var + bn.eps).rsqrt()), WGRAD_TOL)
        rm0, rv0, nb0 = run0[i]
        m = bn.momentum
        n = zd.numel() // zd.shape[1]
        ck.err(f"bn running_mean G.bn{i}", _rel(bn.running_mean, (1 - m) * rm0.to(F64) + m * mean), WGRAD_TOL)
        ck.err(f"bn running_var G.bn{i}", _rel(bn.running_var, (1 - m) * rv0.to(F64) + m * var * n / (n - 1)), WGRAD_TOL)
        assert int(bn.num_batches_tracked) == nb0 + 1
        y = F.relu((z - ge.mean[i][None, :, None, None]) * ge.invstd[i][None, :, None, None] * bn.weight.detach()[None, :, None, None]
                   + bn.bias.detach()[None, :, None, None])
        ck.err(f"fwd G.bn{i}+relu", _rel(xs[i + 1], y), fwd)
    W4 = cb[9].weight
    img_ref = torch.sigmoid(_convT_ref(xs[3], q(W4), (64, 64)) + cb[9].bias.detach()[None, :, None, None])
    ck.err("fwd G.img (sigmoid)", _rel(ge.img, img_ref), fwd)
    # ---- backward ----
    dz4 = dimg * ge.img * (1 - ge.img)
    ck.err("bwd G.dimg_z" + sfx, _rel(ge.dimg_z, dz4), 1e-5)
    ck.err("bias G.convT3" + sfx, _rel(gof("conv_block.9.bias"), ge.dimg_z.to(F64).sum((0, 2, 3))), WGRAD_TOL)
    dz4q = ge.dimg_z.to(tdt).float()
    gw4 = _wgrad_ref(xs[3], dz4q)                                            # [64 in][C out][4][4]: ConvTranspose2d master
    per_tap(ck, "wgrad G.convT3" + sfx, gof("conv_block.9.weight").view(W4.shape), gw4, WGRAD_TOL)
    da = _conv_ref(dz4q, q(W4))[0]
    for i in (2, 1, 0):
        idx = (0, 3, 6)[i]
        bn = bns[i]
        mask = (xs[i + 1] > 0).float()
        ck.err(f"bwd-data G.da{i}" + sfx, _rel(nchw(ge.da[i]).float() * mask, da * mask), fwd)
        dy = (nchw(ge.da[i]).to(F64) * mask)
        xhat = (zs[i].to(F64) - ge.mean[i].to(F64)[None, :, None, None]) * ge.invstd[i].to(F64)[None, :, None, None]
        dgam, dbet = (dy * xhat).sum((0, 2, 3)), dy.sum((0, 2, 3))
        ck.err(f"bias(fused) G.bn{i}.gamma" + sfx, _rel(gof(f"conv_block.{idx + 1}.weight"), dgam), WGRAD_TOL)
        ck.err(f"bias(fused) G.bn{i}.beta" + sfx, _rel(gof(f"conv_block.{idx + 1}.bias"), dbet), WGRAD_TOL)
        n = dy.numel() // dy.shape[1]
        dzr = (bn.weight.detach().to(F64) * ge.invstd[i].to(F64))[None, :, None, None] * (dy - (dbet / n)[None, :, None, None] - xhat * (dgam / n)[None, :, None, None])
        dz = nchw(ge.dz[i]).float()
        ck.err(f"bwd-data G.bn{i} dz" + sfx, _rel(dz, dzr), fwd)
        Wq = q(cb[idx].weight)
        gw = _wgrad_ref(xs[i], dz)
        per_tap(ck, f"wgrad G.convT{i}" + sfx, gof(f"conv_block.{idx}.weight").view(Wq.shape), gw, WGRAD_TOL)
        # (the BatchNorm behind it makes this gradient zero up to rounding: measured against the absolute column sums)
        gbz = gof(f"conv_block.{idx}.bias").to(F64) - dz.to(F64).sum((0, 2, 3))
        ck.err(f"bias(pre-BN) G.convT{i}" + sfx, float(gbz.norm() / dz.to(F64).abs().sum((0, 2, 3)).norm()), WGRAD_TOL)
        if not direct:
            ns = ops.conv_wgrad(ge.mid[i].c, dt, ge.dz[i], ge.a[i - 1] if i > 0 else ge.h, ws.slab, ws.wgs_target)
            ck.split(f"G.convT{i}", ns, SPLITS[ck.tag]["G"][i])
            torch.cuda.synchronize()
            ck.bite(f"wgrad G.convT{i} (nsplit {ns})", WGRAD_TOL, slab_margins(ws.slab[:ns * 64 * 16 * 64], gw, 16, 64) | transposed(gw))
        da = _conv_ref(dz, Wq)[0]
    dh = nchw(ge.dh).float()
    ck.err("bwd-data G.convT0->fc2" + sfx, _rel(dh, da * (h > 0)), fwd)
    dhf = dh.reshape(B, 1024)                                                # column f = c*16 + hw
    gw2 = _linear_wgrad_ref(dhf, a1)
    ck.err("wgrad G.fc2 (permuted rows)" + sfx, _rel(gof("fc2.0.weight"), gw2.flatten()), WGRAD_TOL)
    ck.err("bias G.fc2 (gathered)" + sfx, _rel(gof("fc2.0.bias"), dhf.to(F64).sum(0)), WGRAD_TOL)
    dz1 = ge.dz1.float()
    ck.err("bwd-data G.fc2->fc1" + sfx, _rel(dz1, (dhf @ q(W2)) * (a1 > 0)), fwd)
    gw1 = _linear_wgrad_ref(dz1, inp)
    ck.err("wgrad G.fc1" + sfx, _rel(gof("fc1.0.weight"), gw1.flatten()), WGRAD_TOL)
    ck.err("bias G.fc1" + sfx, _rel(gof("fc1.0.bias"), dz1.to(F64).sum(0)), WGRAD_TOL)
    if not direct:
        ns = ops.conv_wgrad(ge.f2.c, dt, ge.a1, ge.dh, ws.slab, ws.wgs_target)
        torch.cuda.synchronize()
        ck.split("G.fc2", ns, SPLITS[ck.tag]["G.fc2"])
        unperm = gw2.view(64, 16, 128).transpose(0, 1).reshape(1024, 128)  # rows left in the panel's n' = hw*64 + c order
        ck.bite(f"wgrad G.fc2 (nsplit {ns})", WGRAD_TOL, slab_margins(ws.slab[:ns * 1024 * 128], gw2, 1, 128) | {"rows not permuted": _rel(unperm, gw2)})
        ns = ops.conv_wgrad(ge.l4p.c, dt, ge.patches, ge.a[2], ws.slab, ws.wgs_target)
        torch.cuda.synchronize()
        ck.split("G.convT3", ns, SPLITS[ck.tag]["G.convT3"])
        ck.bite(f"wgrad G.convT3 (nsplit {ns})", WGRAD_TOL, slab_margins(ws.slab[:ns * 64 * ge.kp], gw4, 1, ge.kp, None, ge.k0)
                | transposed(gw4))
    else:                                                                   # the last layer's weight gradient straight from the image gradient
        ns = ops.wgrad_img(dt, [ge.dimg_z], ge.a[2], ws.slab, B, G.channels, 64, 64, 64)
        torch.cuda.synchronize()
        ck.split("G.convT3 (eg_wgrad_img)", ns, 1024)
        ck.bite(f"wgrad G.convT3 direct (nsplit {ns})", WGRAD_TOL, slab_margins(ws.slab[:ns * 64 * ge.kp], gw4, 1, ge.kp, None, ge.k0)
                | transposed(gw4))


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_trunks_layerwise(cfg):
    """Discriminator (two tapes) and Encoder (three tapes) trunks: every conv / SN-Linear / head layer's forward, backward-data, spectral-norm
    sigma and coefficient, and every parameter's slice of the gradient vector"""
    mod_, dt_name, B, ch = CONFIGS[cfg]
    dt = eg.engine.parse_dtype(dt_name)
    orc, P, G, D, E = mod_.build(2, dt_name)
    ck = Checks(cfg)
    with torch.no_grad():
        for name, mod in (("D", D), ("E", E)):
            eng = mod.engine(B)
            imgs, douts = _trunk_inputs(mod, B, ch, TAPES[name], seed=3 + TAPES[name])
            _check_trunk(ck, name, mod, eng, imgs, douts, dt_name, dt, B)
    ck.finish()


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_generator_layerwise(cfg):
    """Generator: fc1, fc2 (rows permuted to NHWC), three ConvTranspose2d + BatchNorm + ReLU (batch and running statistics), the Sigmoid image;
    backward through every layer with the fused BatchNorm-backward sums, every parameter's gradient slice -- on the production path for the last
    layer (patch rows + GEMMs) and on its image-direct form (eg_wgrad_img + eg_conv_img_mfma with the BatchNorm-backward epilogue)"""
    mod_, dt_name, B, ch = CONFIGS[cfg]
    dt = eg.engine.parse_dtype(dt_name)
    orc, P, G, D, E = mod_.build(2, dt_name)
    ck = Checks(cfg)
    with torch.no_grad():
        ge = G.engine(B)
        assert not ge.l4_direct, "the production path of the last layer is patch rows + GEMMs"
        assert ops.conv_img_mfma_ok(dt, ch, 64, 64, 64, 4, 2, 1) and ops.wgrad_img_ok(dt, ch, 64, 64, 64, 4, 2, 1)
        _check_generator(ck, G, ge, B, dt_name, dt, direct=False)
        ge.ws.need_slab(ops.wgrad_img_splits(B, 64) * 64 * ge.kp * 4)
        _check_generator(ck, G, ge, B, dt_name, dt, direct=True)
        ge.l4_direct = False
    ck.finish()

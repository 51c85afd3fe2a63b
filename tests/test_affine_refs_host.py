"""Host side of the affine / loss kernel tests (tests/test_gpu_affine_losses.py): the seeded input sets, the error metric, the
float32-vs-float64 YARDSTICK of every compared quantity on every input set, and the checks that tie tests/affine_refs.py to the oracle
and to the recorded golden files and show that every mutant of affine_refs lies far outside the bound the GPU tests use.

Metric (``metric``): gradient blocks are compared row by row, |got - want| over the row's largest |want| entry; everything else element
by element, |got - want| / max(1, |want|).  The figure of a comparison is the largest such ratio.
Bound (``bound``) of a comparison: max(K * yardstick, FLOOR); yardstick = the figure of the SAME reference function evaluated in float32
on the CPU against its float64 evaluation on the same inputs, K = 8 (one margin for all: the device's sinf / cosf / atanf / expf / logf,
its fused multiply-adds and its summation order differ from the CPU's float32), FLOOR = 4 float32 ulps of the quantity's scale (a
float32 evaluation can be exact on a small input set by luck; the device's need not be).
"""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import affine_refs as R
from conftest import GOLDEN
from oracle import celeba_oracle as co
from oracle import dsprites_oracle as do
from oracle import mnist_oracle as mo

K = 8.0
ULP = 2.0 ** -23
FLOOR = 4 * ULP
MUTANT_FACTOR = 10.0                    # every mutant misses its bound by at least this factor
SCALE = float(np.float32(0.7))          # the `scale` argument of every loss call (a C float)
PARENT = 1000                           # rows of a parent input set; a case of batch B takes its first B rows
EXCLUDE_T2 = 0.1                        # rpqxy: rows with |t2| below this are left out of the wide set's comparison
EXCLUDE_CAP = 0.05

REG_B = (1, 5, 8, 9, 127, 128, 129, 136, 256, 512, 1000)
REG_KINDS = tuple(R.REGS)
WIDE_KINDS = ("rpqxy", "rp", "rp_color", "pxy", "pxy_color")
HEAD_B = (1, 37, 256, 257, 512, 1000)
MAT_B = (1, 127, 128, 129, 1000)
WARP_SHAPES = ((128, 3, 64, 64), (256, 1, 32, 32), (512, 3, 64, 64), (3, 2, 24, 40))
ROW_QUANTITIES = ("d_real", "d_trans", "dout")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _uniform(g, shape, r):
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * r).float()


@functools.lru_cache(maxsize=None)
def mlp():
    return mo.make_approximator()


# ---- metric and bound -------------------------------------------------------------------------------------------------------------------
def metric(got, want, rows=False, keep=None):
    """largest error ratio of ``got`` against the float64 ``want`` (see the module docstring); ``keep``: boolean row mask"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    if rows:
        ratio = err.amax(1) / want.abs().amax(1).clamp_min(1e-300)
    else:
        ratio = err / want.abs().clamp_min(1.0)
    if keep is not None:
        ratio = ratio[keep]
    assert bool(torch.isfinite(ratio).all()), "non-finite value in a comparison"
    return float(ratio.max()) if ratio.numel() else 0.0


def bound(yard):
    return max(K * yard, FLOOR)


def figures(got, want, keep=None):
    """{quantity: figure} of two result dicts of affine_refs (common keys)"""
    out = {}
    for q in want:
        if q in got:
            if q == "value" and keep is not None and not bool(keep.all()):
                continue                    # the scalar sums over rows that are left out: compared on the [-1, 1] sets only
            out[q] = metric(got[q], want[q], rows=q in ROW_QUANTITIES, keep=None if q == "value" else keep)
    return out


# ---- input sets ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reg_parent(kind, wide):
    n = R.REGS[kind][1]
    g = _gen("reg", kind, wide)
    r = 1.5 if wide else 1.0
    return _uniform(g, (PARENT, n), r), _uniform(g, (PARENT, n), r), _uniform(g, (PARENT, n), r)


def reg_inputs(kind, B, wide=False):
    """float32 (real, trans, code) [B, n], uniform in [-1, 1] (wide: [-1.5, 1.5]) and ``keep``: the rows that are compared"""
    real, trans, code = (t[:B].clone() for t in _reg_parent(kind, wide))
    keep = torch.ones(B, dtype=torch.bool)
    if kind == "rpqxy":
        keep = R.rpqxy_t2(real.double(), trans.double()).abs() >= EXCLUDE_T2
    return real, trans, code, keep


@functools.lru_cache(maxsize=None)
def reg_truth(kind, B, wide=False):
    real, trans, code, _ = reg_inputs(kind, B, wide)
    return R.reg_eval(kind, real.double(), trans.double(), code.double(), SCALE, mlp())


@functools.lru_cache(maxsize=None)
def reg_yardstick(kind, B, wide=False):
    real, trans, code, keep = reg_inputs(kind, B, wide)
    return figures(R.reg_eval(kind, real, trans, code, SCALE, mlp()), reg_truth(kind, B, wide), keep)


HEAD_CASES = (("bce", 1, "t1"), ("bce", 1, "t0"), ("mse", 8, "tensor"), ("mse", 5, "const"), ("ce", 3, ""), ("ce", 10, ""), ("ce", 16, ""),
              ("mi", 3, "prob"), ("mi", 10, "prob"), ("mi", 16, "prob"), ("mi", 3, "logits"), ("mi", 10, "logits"), ("mi", 16, "logits"))


@functools.lru_cache(maxsize=None)
def head_inputs(kind, n, variant, B):
    """keyword arguments of affine_refs.head_eval in float32 (labels int64): logits o ~ 2 N(0, 1)"""
    g = _gen("head", kind, n, variant)
    o = (torch.randn(PARENT, n, generator=g, dtype=torch.float64) * 2).float()[:B]
    kw = {"o": o}
    if kind == "bce":
        kw["target"] = 1.0 if variant == "t1" else 0.0
    elif kind == "mse":
        if variant == "tensor":
            kw["tgt"] = _uniform(g, (PARENT, n), 1.0)[:B]
        else:
            kw["target"] = 0.25
    elif kind == "ce":
        kw["labels"] = torch.randint(0, n, (PARENT,), generator=g)[:B]
    else:
        t = torch.randn(PARENT, n, generator=g, dtype=torch.float64).float()
        if variant == "prob":           # even rows: a soft distribution, odd rows: one-hot (what the trainers pass)
            hot = torch.nn.functional.one_hot(torch.randint(0, n, (PARENT,), generator=g), n).float()
            t = torch.softmax(t, 1)
            t[1::2] = hot[1::2]
        kw["tgt"] = t[:B]
        kw["target_logits"] = variant == "logits"
    return kw


def _to64(kw):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in kw.items()}


@functools.lru_cache(maxsize=None)
def head_truth(kind, n, variant, B):
    return R.head_eval(kind, scale=SCALE, **_to64(head_inputs(kind, n, variant, B)))


@functools.lru_cache(maxsize=None)
def head_yardstick(kind, n, variant, B):
    return figures(R.head_eval(kind, scale=SCALE, **head_inputs(kind, n, variant, B)), head_truth(kind, n, variant, B))


def matrix_inputs(kind, B):
    return _uniform(_gen("matrix", kind), (PARENT, 9), 1.0)[:B].contiguous()          # codes sit in columns 1 .. 1 + n of 9 (strided)


def _matrix_fn(kind):
    return R.affine_para_rpqmnxy if kind == "para_rpqmnxy" else (lambda c: R.theta(R.MATRICES[kind][0](c)).reshape(c.shape[0], 6))


MATRIX_KINDS = tuple(R.MATRICES) + ("para_rpqmnxy",)


@functools.lru_cache(maxsize=None)
def matrix_truth(kind, B):
    return _matrix_fn(kind)(matrix_inputs(kind, B)[:, 1:].double())


@functools.lru_cache(maxsize=None)
def matrix_yardstick(kind, B):
    return metric(_matrix_fn(kind)(matrix_inputs(kind, B)[:, 1:]), matrix_truth(kind, B))


@functools.lru_cache(maxsize=None)
def warp_inputs(shape):
    """img [B, C, H, W] in [0, 1], codes [B, 8] (five are read) and theta [B, 2, 3] = float32(matrix_rpqxy(codes)), with rows 0 .. 4 set to:
    the identity, a 3x zoom-out with a shift (samples fall outside), a 5x zoom-in, a quarter turn, a far shift (everything outside)"""
    B = shape[0]
    g = _gen("warp", shape)
    img = torch.rand(shape, generator=g, dtype=torch.float64).float()
    code = _uniform(g, (B, 8), 1.0)
    special = torch.tensor([[0, 0, 0, 0, 0], [0.5, 10, 10, 12, -9], [-0.25, -4, -4, 1, 1], [4.5, 0, 0, 0, 0], [0, 0, 0, 40, 40]], dtype=torch.float32)
    code[:min(B, 5), :5] = special[:B]
    th = R.theta(R.matrix_rpqxy(code[:, :5].double())).float()
    return img, code, th


@functools.lru_cache(maxsize=None)
def warp_truth(shape, mode):
    """mode 'border' / 'zeros': from the float32 theta;  'fused': from the codes (theta is part of the computation)"""
    img, code, th = warp_inputs(shape)
    th64 = R.theta(R.matrix_rpqxy(code[:, :5].double())) if mode == "fused" else th.double()
    return R.warp(img.double(), th64, "border" if mode == "fused" else mode)


@functools.lru_cache(maxsize=None)
def warp_yardstick(shape, mode):
    img, code, th = warp_inputs(shape)
    th32 = R.theta(R.matrix_rpqxy(code[:, :5])) if mode == "fused" else th
    return metric(R.warp(img, th32, "border" if mode == "fused" else mode), warp_truth(shape, mode))


COLOR_SHAPES = ((512, 3, 64 * 64), (7, 3, 37))


def color_inputs(shape):
    g = _gen("color", shape)
    B, C, HW = shape
    return (_uniform(g, shape, 1.0), _uniform(g, (B, 9), 1.5), torch.randint(0, 256, (B, HW), generator=g, dtype=torch.int32).to(torch.uint8),
            _uniform(g, (B, C), 1.0) * 0.5 + 1)


def color_yardstick(shape, divide):
    x, code, _, _ = color_inputs(shape)
    return metric(R.color_scale(x, code, 4, 0.5, divide), R.color_scale(x.double(), code.double(), 4, 0.5, divide))


# ---- the references against the oracle and the recorded files -------------------------------------------------------------------------------
N_ORACLE = 4096


def _codes(name, n, r=1.0):
    g = _gen("oracle", name)
    return _uniform(g, (N_ORACLE, n), r), _uniform(g, (N_ORACLE, n), r), torch.randn(N_ORACLE, n, generator=g, dtype=torch.float64).float()


def _check(name, got, want64, own32, rows=False):
    """an fp32 function of the oracle against the float64 reference: within K times the error of the reference's own float32 evaluation"""
    fig, yard = metric(got, want64, rows), metric(own32, want64, rows)
    print(f"{name}: oracle-vs-f64 {fig:.3g}  f32-vs-f64 yardstick {yard:.3g}  bound {bound(yard):.3g}")
    assert fig <= bound(yard), (name, fig, yard)


@pytest.mark.parametrize("name,ofn,rfn,n", [
    ("celeba.get_matrix", co.get_matrix, R.matrix_rpqxy, 5), ("mnist.get_matrix", mo.get_matrix, R.matrix_rpqmnxy, 7),
    ("dsprites.get_matrix", do.get_matrix, R.matrix_rp, 4), ("dsprites.get_matrix_pxy", do.get_matrix_pxy, R.matrix_pxy, 3),
    ("dsprites.get_matrix_pxy_align", do.get_matrix_pxy_align, R.matrix_pxy_align, 3),
    ("mnist.latent_to_affine_para", mo.latent_to_affine_para, R.affine_para_rpqmnxy, 7)])
def test_matrix_references_agree_with_the_oracle(name, ofn, rfn, n):
    c = _codes(name, n)[0]
    _check(name, ofn(c), rfn(c.double()), rfn(c))


def test_pxy_align_inverse_is_the_inverse_of_the_oracle_matrix():
    c = _codes("align", 3)[0]
    prod = do.get_matrix_pxy_align(c).double() @ R.matrix_pxy_align_inv(c.double())
    assert metric(prod, torch.eye(3, dtype=torch.float64).expand_as(prod)) <= FLOOR


ORACLE_REGS = {"rpqxy": co.affine_regularzier, "rp": do.affine_regularzier, "rp_color": do.affine_color_regularzier,
               "pxy": do.affine_regularzier_pxy, "pxy_color": do.affine_regularzier_pxy_color,
               "rpqmnxy": lambda r, t: mo.affine_regularizer(mlp(), r, t)}


@pytest.mark.parametrize("kind", REG_KINDS)
def test_regularizer_references_agree_with_the_oracle(kind):
    """prediction and both vector-Jacobian products (random upstream gradient) of the oracle's fp32 function on 4096 samples in [-1, 1]"""
    n = R.REGS[kind][1]
    real, trans, w = _codes(kind, n)
    want = R.reg_vjp(kind, real.double(), trans.double(), w.double(), mlp())
    own = R.reg_vjp(kind, real, trans, w, mlp())
    r, t = real.clone().requires_grad_(True), trans.clone().requires_grad_(True)
    pred = ORACLE_REGS[kind](r, t)
    d_real, d_trans = torch.autograd.grad((pred * w).sum(), (r, t))
    _check(kind + " pred", pred, want["pred"], own["pred"])
    _check(kind + " d_real", d_real, want["d_real"], own["d_real"], rows=True)
    _check(kind + " d_trans", d_trans, want["d_trans"], own["d_trans"], rows=True)


@pytest.mark.parametrize("fname,kind,mfn", [("celeba_affine.npz", "rpqxy", R.matrix_rpqxy), ("mnist_affine.npz", "rpqmnxy", R.matrix_rpqmnxy)])
def test_references_agree_with_the_recorded_files(fname, kind, mfn):
    """files recorded from the reference's own functions (oracle/make_golden.py)"""
    gold = np.load(os.path.join(GOLDEN, fname))
    n = R.REGS[kind][1]
    t = lambda k: torch.tensor(gold[k])
    code = t("code")[:, :n]
    _check(fname + " A", t("A"), mfn(code.double()), mfn(code))
    real, trans, w = t("real_code")[:, :n], t("trans_code")[:, :n], t("w")
    m = mo.make_approximator(int(gold["mlp_seed"])) if kind == "rpqmnxy" else None
    want, own = R.reg_vjp(kind, real.double(), trans.double(), w.double(), m), R.reg_vjp(kind, real, trans, w, m)
    _check(fname + " pred", t("pred"), want["pred"], own["pred"])
    _check(fname + " d_real", t("d_real")[:, :n], want["d_real"], own["d_real"], rows=True)
    _check(fname + " d_trans", t("d_trans")[:, :n], want["d_trans"], own["d_trans"], rows=True)
    if fname == "celeba_affine.npz":
        img = co.synthetic_real(4, seed=int(gold["img_seed"]))
        th = t("A")[:4, :2]
        _check(fname + " warped", t("warped"), R.warp(img.double(), th.double(), "border"), R.warp(img, th, "border"))


@pytest.mark.parametrize("mode,ofn", [("border", co.warp), ("zeros", do.warp_zeros)])
def test_warp_references_agree_with_the_oracle(mode, ofn):
    img, _, th = warp_inputs(WARP_SHAPES[3])
    _check("warp " + mode, ofn(img, th), warp_truth(WARP_SHAPES[3], mode), R.warp(img, th, mode))


def test_mutual_info_reference_agrees_with_the_oracle():
    kw = head_inputs("mi", 10, "prob", 257)
    o = kw["o"].clone().requires_grad_(True)
    val = SCALE * do.mutual_info_loss(torch.softmax(o, 1), kw["tgt"])
    (dout,) = torch.autograd.grad(val, o)
    want, own = head_truth("mi", 10, "prob", 257), R.head_eval("mi", scale=SCALE, **kw)
    _check("mi value", val.detach().reshape(1), want["value"].reshape(1), own["value"].reshape(1))
    _check("mi dout", dout, want["dout"], own["dout"], rows=True)


# ---- the input sets -----------------------------------------------------------------------------------------------------------------------
def test_rpqxy_exclusion_shares():
    """the wide rpqxy set leaves out at most 5 % of its rows (|t2| < 0.1), the [-1, 1] set none.  A case of batch B is the first B rows of
    the 1000-row set: the share is asserted for the whole set and for every case of at least 100 rows; below that one row is already
    more than 5 % (B <= 9: more than 11 %), so those cases may leave out one row at most."""
    for B in REG_B:
        assert bool(reg_inputs("rpqxy", B, False)[3].all())
        left_out = int((~reg_inputs("rpqxy", B, True)[3]).sum())
        print(f"wide rpqxy set, B = {B}: {left_out} rows left out")
        assert left_out <= (EXCLUDE_CAP * B if B >= 100 else 1), (B, left_out)
    assert int((~reg_inputs("rpqxy", PARENT, True)[3]).sum()) <= EXCLUDE_CAP * PARENT


# ---- every mutant is far outside the bound the GPU test uses ---------------------------------------------------------------------------------
def _worst_ratio(mutant_result, truth, yard, keep=None):
    """the largest (figure of the mutant) / (bound of the quantity) over the compared quantities"""
    fig = figures(mutant_result, truth, keep)
    return max(fig[q] / bound(yard[q]) for q in fig)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("kind", REG_KINDS)
def test_every_regularizer_mutant_misses_the_bound(kind, wide):
    if wide and kind not in WIDE_KINDS:
        return
    smallest = (float("inf"), None)
    for B in REG_B:
        real, trans, code, keep = reg_inputs(kind, B, wide)
        truth, yard = reg_truth(kind, B, wide), reg_yardstick(kind, B, wide)
        if not bool(keep.any()):
            continue
        for m in R.reg_mutants(kind):
            ratio = _worst_ratio(R.reg_eval(kind, real.double(), trans.double(), code.double(), SCALE, mlp(), mutant=m), truth, yard, keep)
            smallest = min(smallest, (ratio, (m, B)))
            assert ratio >= MUTANT_FACTOR, (kind, wide, B, m, ratio)
    print(f"{kind} wide={wide}: smallest mutant error / bound = {smallest[0]:.3g} at {smallest[1]}")


@pytest.mark.parametrize("kind,n,variant", HEAD_CASES)
def test_every_head_mutant_misses_the_bound(kind, n, variant):
    smallest = (float("inf"), None)
    for B in HEAD_B:
        kw, truth, yard = _to64(head_inputs(kind, n, variant, B)), head_truth(kind, n, variant, B), head_yardstick(kind, n, variant, B)
        for m in R.HEAD_MUTANTS[kind]:
            ratio = _worst_ratio(R.head_eval(kind, scale=SCALE, mutant=m, **kw), truth, yard)
            smallest = min(smallest, (ratio, (m, B)))
            assert ratio >= MUTANT_FACTOR, (kind, n, variant, B, m, ratio)
    print(f"{kind} n={n} {variant}: smallest mutant error / bound = {smallest[0]:.3g} at {smallest[1]}")


def test_yardsticks_are_float32_sized():
    """a yardstick far above float32 rounding would make the GPU bound meaningless: all of them are below 1e-3 even on the wide sets (the
    largest belong to the wide rpqxy set, whose kept rows reach |t2| = 0.1), and the [-1, 1] regularizer sets stay below 1e-4"""
    worst = {}
    for kind in REG_KINDS:
        for wide in (False, True):
            if wide and kind not in WIDE_KINDS:
                continue
            for B in REG_B:
                for q, v in reg_yardstick(kind, B, wide).items():
                    worst[(kind, wide, q)] = max(worst.get((kind, wide, q), 0.0), v)
    for k, v in sorted(worst.items()):
        print("yardstick", k, f"{v:.3g}")
        assert v < (1e-3 if k[1] else 1e-4), (k, v)

"""Host side of tests/test_gpu_input_grad.py: the two input-gradient entry points are declared, exported and bound; their argument errors
come back as RuntimeError; the float64 contraction of tests/input_grad_refs.py with the stride rows of the header equals autograd of the
reference-shaped first layers (this pins the layout table); each mutant of the restatements misses the GPU test's bound by
``MUTANT_FACTOR``; the seeds of the BatchNorm cases leave out less than the cap."""
import ctypes
import importlib
import inspect

import pytest
import torch

import input_grad_refs as R


def _pkg():
    return importlib.import_module("ead-gan_amd")


def test_entry_points_are_declared_exported_and_bound():
    eg = _pkg()
    protos = eg._lib.parse_header()
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    for name, nargs in (("eg_linear_dinput", 15), ("eg_linear_dinput_ws_floats", 4), ("eg_bn_bwd_eval", 15)):
        assert name in protos, f"{name} is not declared in include/eadgan_hip.h"
        assert len(protos[name][1]) == nargs, (name, len(protos[name][1]))
        assert hasattr(cdll, name), f"{name} is not exported by the library"
    assert eg._lib.lib().query("eg_version") >= 109
    assert callable(eg.ops.linear_dinput) and callable(eg.ops.bn_bwd_eval) and callable(eg.sampling.project_images)
    for mod in (eg.celeba, eg.mnist, eg.dsprites):
        sig = inspect.signature(mod._GenEngine.backward).parameters
        assert sig["dinp"].default is None and sig["need_wgrad"].default is True and sig["training"].default is True
    assert eg.colored.Generator.__mro__[1] is eg.dsprites.Generator
    assert inspect.signature(eg.engine.bn_train_backward).parameters["training"].default is True
    # split scratch of the production shapes (B = 128): ceil(chunks of 128 reductions / 4) partial tiles of B x cin, none for one split
    assert eg.ops.linear_dinput_ws_floats(128, 16, 1024, 218) == 32 * 128 * 218
    assert eg.ops.linear_dinput_ws_floats(128, 64, 128, 79) == 16 * 128 * 79
    assert eg.ops.linear_dinput_ws_floats(128, 1, 128, 7) == 0
    assert eg.ops.linear_dinput_ws_floats(8, 1, 12, 7) == 0            # a shape the launch refuses


def test_argument_errors_do_not_abort():
    eg = _pkg()
    call = eg._lib.lib().call
    one = ctypes.c_void_p(16)                       # a non-null, 16-byte aligned address: every case is refused before anything is launched
    with pytest.raises(RuntimeError, match="null pointer"):
        call("eg_linear_dinput", 0, None, 128, None, None, 2, 1, 128, 7, 0, 7, 1, None, 0, None)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        call("eg_linear_dinput", 0, one, 12, one, one, 2, 1, 12, 7, 0, 7, 1, None, 0, None)
    with pytest.raises(RuntimeError, match="dtype"):
        call("eg_linear_dinput", 7, one, 128, one, one, 2, 1, 128, 7, 0, 7, 1, None, 0, None)
    with pytest.raises(RuntimeError, match="positive"):
        call("eg_linear_dinput", 0, one, 128, one, one, 0, 1, 128, 7, 0, 7, 1, None, 0, None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call("eg_linear_dinput", 1, one, 100, one, one, 2, 1, 128, 7, 0, 7, 1, None, 0, None)
    with pytest.raises(RuntimeError, match="workspace"):          # 32 splits need their scratch
        call("eg_linear_dinput", 1, one, 16384, one, one, 2, 16, 1024, 7, 1, 16, 16384, None, 0, None)
    with pytest.raises(RuntimeError, match="workspace"):
        call("eg_linear_dinput", 1, one, 16384, one, one, 2, 16, 1024, 7, 1, 16, 16384, one, 32 * 2 * 7 - 1, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        call("eg_bn_bwd_eval", 0, None, None, None, 4, 8, None, None, 1e-5, None, None, None, 0, 0.0, None)
    with pytest.raises(RuntimeError, match="multiple"):
        call("eg_bn_bwd_eval", 1, one, one, one, 4, 12, one, one, 1e-5, one, one, one, 0, 0.0, None)
    with pytest.raises(RuntimeError, match="EG_ACT_NONE, EG_ACT_RELU or EG_ACT_LRELU"):
        call("eg_bn_bwd_eval", 0, one, one, one, 4, 8, one, one, 1e-5, one, one, one, eg.ops.ACT_TANH, 0.0, None)
    with pytest.raises(RuntimeError, match="MI355X only|GPU"):
        eg.sampling.project_images("celeba", eg.celeba.Generator().eval(), torch.zeros(1, 3, 64, 64), torch.zeros(1, 10), 1, 0.1)
    with pytest.raises(ValueError, match="eval"):
        eg.sampling.project_images("celeba", eg.celeba.Generator(), torch.zeros(1, 3, 64, 64), torch.zeros(1, 10), 1, 0.1)
    with pytest.raises(ValueError, match="families"):
        eg.sampling.project_images("cifar", eg.celeba.Generator().eval(), torch.zeros(1, 3, 64, 64), torch.zeros(1, 10), 1, 0.1)


@pytest.mark.parametrize("kind,cin", [("celeba", 218), ("mnist", 79), ("dsprites", 7), ("colored", 10)])
def test_contraction_equals_autograd_of_the_reference_first_layer(kind, cin):
    """the stride rows of the header / DESIGN 6k: with them the float64 contraction IS the input gradient of the reference's first layer, its
    output flattened the way the engines store dh0 / dh / dz1"""
    B = 3
    fn, w, (NI, NJ, s_i, s_j, s_k) = R.first_layer(kind, cin)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, cin, generator=g, dtype=torch.float64).requires_grad_(True)
    h = fn(x)
    assert h.shape == (B, NI * NJ)
    dH = torch.randn(h.shape, generator=g, dtype=torch.float64)
    h.backward(dH)
    got = R.contraction(dH, w, NI, NJ, cin, s_i, s_j, s_k)
    assert R.dist(got, x.grad) < 1e-13
    assert (s_i, s_j, s_k) == R.strides_of(NI, NJ, cin)[:3]


@pytest.mark.parametrize("case", R.LINEAR_CASES)
def test_contraction_mutants_miss_the_bound(case):
    """exchanged strides and a result read with the padded row length of the engines' ``inp``: both miss the GPU test's bound (K x the
    float32 yardstick) by MUTANT_FACTOR wherever they change anything (one row hides the padded stride)"""
    B, NI, NJ, Kc = case
    c = R.linear_case(case, "f32")
    want = R.contraction(c["dH"], c["Wr"], NI, NJ, Kc, *c["strides"])
    yard = R.dist(R.contraction(c["dH"], c["Wr"], NI, NJ, Kc, *c["strides"], dtype=torch.float32), want)
    assert 0 < yard < 1e-5, yard
    cpad = (Kc + 7) // 8 * 8
    changes = {"swap_strides": True, "padded_columns": B > 1 and cpad != Kc}
    for m, changed in changes.items():
        ratio = R.dist(R.contraction(c["dH"], c["Wr"], NI, NJ, Kc, *c["strides"], mutant=m, cpad=cpad), want) / (R.K * yard)
        print(f"{case} mutant {m}: error / bound = {ratio:.3g}")
        if changed:
            assert ratio >= R.MUTANT_FACTOR, (case, m, ratio)


@pytest.mark.parametrize("name", list(R.ACTS))
@pytest.mark.parametrize("case", R.BN_CASES)
def test_bn_eval_backward_yardstick_mutant_and_excluded_share(case, name):
    """float32 torch stays close to float64 on the kept elements, the seeds leave out at most EXCLUDE_CAP of a case, and the mutant that
    divides by the raw running variance misses the bound by MUTANT_FACTOR"""
    c = R.bn_case(case, "f32")
    want, y64 = R.bn_eval_bwd(c, name)
    keep = R.bn_keep(y64, name)
    share = 1.0 - float(keep.float().mean())
    assert share <= R.EXCLUDE_CAP, share
    for dt in ("bf16", "f16"):                      # the 16-bit operands of the GPU cases are other values: their shares count too
        c16 = R.bn_case(case, dt)
        assert 1.0 - float(R.bn_keep(R.bn_eval_bwd(c16, name)[1], name).float().mean()) <= R.EXCLUDE_CAP
    y32 = R.bn_eval_act(c["z"], c, "none", torch.float32)          # the float32 restatement agrees on every kept sign
    assert bool(((y32 > 0) == (y64 > 0))[keep].all())
    yard = R.dist(R.bn_eval_bwd(c, name, torch.float32)[0] * keep, want * keep)
    print(f"{case} {name}: left out {share:.5f}, float32 yardstick {yard:.3g}")
    assert 0 < yard < 1e-5, yard
    ratio = R.dist(R.bn_eval_bwd(c, name, mutant="raw_var")[0] * keep, want * keep) / (R.K * yard)
    assert ratio >= R.MUTANT_FACTOR, ratio

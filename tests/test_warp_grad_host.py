"""Host side of tests/test_gpu_warp_grad.py: the two backward entry points exist in the header and in the built library, the kink mask of
tests/warp_grad_cases.py leaves out what it says and no more, the masked yardsticks are float32-sized, the hand-written float64 backward
agrees with autograd and each of its mutants misses the GPU test's bound by ``H.MUTANT_FACTOR``."""
import ctypes
import importlib

import pytest
import torch

import test_affine_refs_host as H
import warp_grad_cases as WG


def test_backward_entry_points_are_declared_and_exported():
    eg = importlib.import_module("ead-gan_amd")
    protos = eg._lib.parse_header()
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    for name, nargs in (("eg_warp_affine_bwd", 11), ("eg_theta_bwd", 7)):
        assert name in protos, f"{name} is not declared in include/eadgan_hip.h"
        assert len(protos[name][1]) == nargs, (name, len(protos[name][1]))
        assert hasattr(cdll, name), f"{name} is not exported by the library"
    assert eg.ops.THETA_KINDS == {"rpqxy": 0, "rpqmnxy": 1, "rp": 2, "pxy": 3, "pxy_align_inv": 4}
    assert callable(eg.ops.warp_affine_bwd) and callable(eg.ops.theta_bwd) and callable(eg.dsprites.get_matrix_pxy)


def test_cpu_tensors_are_refused():
    eg = importlib.import_module("ead-gan_amd")
    with pytest.raises(RuntimeError, match="MI355X only"):
        eg.celeba.transformation_2D()(torch.zeros(1, 1, 4, 4, requires_grad=True), torch.zeros(1, 2, 3))
    for fn in (eg.celeba.get_matrix, eg.mnist.get_matrix, eg.dsprites.get_matrix, eg.dsprites.get_matrix_D, eg.dsprites.get_matrix_pxy,
               eg.dsprites.get_matrix_pxy_align):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(torch.zeros(2, 7, requires_grad=True))
    with pytest.raises(ValueError):
        eg.celeba.transformation_2D(padding_mode="reflection")


@pytest.mark.parametrize("shape", WG.HOST_SHAPES)
def test_mask_shares_of_the_warp_inputs(shape):
    """exactly rows 0, 3, 4 (identity, quarter turn, far shift) are left out; every kept row's masked share is at most 0.016"""
    c = WG.warp_case(shape)
    left_out = tuple(int(i) for i in (~c["keep"]).nonzero().flatten())
    kept = float(c["share"][c["keep"]].max())
    print(f"{shape}: left out {left_out}, shares of them {[round(float(c['share'][i]), 3) for i in left_out]}, largest kept share {kept:.4f}")
    assert left_out == WG.LEFT_OUT
    assert kept <= 0.016 <= WG.SHARE_CAP


@pytest.mark.parametrize("name", WG.E2E)
def test_mask_shares_of_the_code_level_cases(name):
    share = WG.e2e_case(name)["share"]
    print(f"{name}: largest masked share {float(share.max()):.4f}")
    assert bool((share <= WG.SHARE_CAP).all()), share


def test_masked_yardsticks_are_float32_sized():
    """dtheta / dcode with the mask and the code -> theta gradients: below 1e-4.  dimg (unmasked) is printed and held below 1e-3, the
    limit tests/test_affine_refs_host.py sets for its widest sets: under 'border' a zoomed-out sample adds thousands of clamped output
    pixels into one border pixel of dimg, a float32 sum whose error the element's size does not scale away (1.1e-4 at (9, 3, 64, 64))."""
    masked, dimg = {}, {}
    for shape in WG.HOST_SHAPES:
        for mode in WG.MODES:
            y = WG.warp_yardstick(shape, mode)
            masked[(shape, mode)], dimg[(shape, mode)] = y["dtheta"], y["dimg"]
    for name in WG.E2E:
        y = WG.e2e_yardstick(name)
        masked[name], dimg[name] = y["dcode"], y["dimg"]
    for kind in WG.R.MATRICES:
        for B in WG.THETA_B:
            masked[("theta_bwd", kind, B)] = WG.theta_yardstick(kind, B)
    for k, v in masked.items():
        print(f"yardstick {k}: dtheta / dcode {v:.3g}" + (f"  dimg {dimg[k]:.3g}" if k in dimg else ""))
        assert v < 1e-4, (k, v)
    assert max(dimg.values()) < 1e-3, dimg


def test_unmasked_dtheta_is_not_comparable():
    """what the mask is for: unmasked, float32 autograd misses float64 by far more than any float32 rounding on the kept rows too"""
    shape = (5, 3, 64, 64)
    c = WG.warp_case(shape)
    raw = WG.warp_grads(c["img"], c["theta"], c["dout"], "border")[1]
    fig = H.metric(raw, WG.warp_truth(shape, "border")["dtheta_unmasked"], rows=True)
    print(f"unmasked float32 dtheta against float64: {fig:.3g}")
    assert fig > 1e-2


@pytest.mark.parametrize("mode", WG.MODES)
@pytest.mark.parametrize("shape", WG.OPS_SHAPES)
def test_manual_backward_and_its_mutants(shape, mode):
    """the hand-written float64 dtheta equals autograd's (masked upstream gradient, kept rows); each mutant misses the bound of the GPU
    test by MUTANT_FACTOR where it changes anything: ``no_border_zero`` in 'border' mode, ``swap_half_sizes`` on the non-square shape,
    ``first_channel`` with more than one channel"""
    c, truth, yard = WG.warp_case(shape), WG.warp_truth(shape, mode), WG.warp_yardstick(shape, mode)
    args = (c["img"].double(), c["theta"].double(), c["dout_masked"].double(), mode)
    fig = H.metric(WG.manual_dtheta(*args), truth["dtheta"], rows=True, keep=c["keep"])
    assert fig <= 1e-12, fig
    assert bool((WG.manual_dtheta(c["img"].double(), c["theta"].double(), c["dout"].double(), mode)[4] == 0).all())       # the far shift
    changes = {"no_border_zero": mode == "border", "swap_half_sizes": shape[2] != shape[3], "first_channel": shape[1] > 1}
    for m in WG.MUTANTS:
        ratio = H.metric(WG.manual_dtheta(*args, mutant=m), truth["dtheta"], rows=True, keep=c["keep"]) / H.bound(yard["dtheta"])
        print(f"{shape} {mode} mutant {m}: error / bound = {ratio:.3g}")
        if changes[m]:
            assert ratio >= H.MUTANT_FACTOR, (shape, mode, m, ratio)

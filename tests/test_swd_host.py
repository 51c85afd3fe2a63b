"""The sliced Wasserstein distance without a GPU: the float64 restatement tests/swd_refs.py against scipy and against the
properties the definition implies, the new entry points of the C ABI, and the argument checks of quality.py that run before any launch."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import swd_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eg_pyr_down", "eg_pyr_up_sub", "eg_swd_patch_stats_ws_doubles", "eg_swd_patch_stats", "eg_swd_unit_columns", "eg_swd_project_ws_floats",
       "eg_swd_project", "eg_sort_tile_elems", "eg_sort_columns_f32", "eg_l1_mean_ws_doubles", "eg_l1_mean_f32")


def _pkg():
    return importlib.import_module("ead-gan_amd")


def _sets(seed, shape=(3, 3, 32, 32)):
    rng = np.random.RandomState(seed)
    return rng.standard_normal(shape), rng.uniform(-1, 1, shape)


def test_down_and_up_are_scipys_mirror_convolution():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(0)
    for side in (16, 32):
        x = rng.standard_normal((2, 3, side, side))
        want = np.stack([[ndimage.convolve(p, R.G, mode="mirror") for p in img] for img in x])[..., ::2, ::2]
        assert np.abs(R.down(x) - want).max() <= 1e-14
        z = np.zeros((2, 3, 2 * side, 2 * side))
        z[..., ::2, ::2] = x
        want = np.stack([[ndimage.convolve(p, 4 * R.G, mode="mirror") for p in img] for img in z])
        assert np.abs(R.up(x) - want).max() <= 1e-14
    # numpy's reflect padding is the same border rule
    x = rng.standard_normal((5, 8))
    pad = np.pad(x, 2, mode="reflect")
    want = sum(R.G[a, b] * pad[a:a + 5, b:b + 8] for a in range(5) for b in range(5))
    assert np.abs(R._filter(x, R.G) - want).max() == 0.0


def test_pyramid_levels_rebuild_the_gaussian_levels():
    x = np.random.RandomState(1).standard_normal((2, 3, 64, 64))
    pyr = R.laplacian_pyramid(x)
    assert [p.shape[-1] for p in pyr] == [64, 32, 16] == R.level_sides(64)
    gauss = [x, R.down(x), R.down(R.down(x))]
    assert np.abs(pyr[2] - gauss[2]).max() == 0.0                       # the coarsest level stays Gaussian
    for l in (1, 0):
        assert np.abs(R.up(gauss[l + 1]) + pyr[l] - gauss[l]).max() <= 1e-13


def test_distance_of_a_set_to_itself_is_zero_and_to_another_is_not():
    A, B = _sets(2)
    pos, dirs = R.draw_plan(np.random.RandomState(3), A.shape, 6, 2, 16)
    same = R.swd(A, A, pos, dirs, 6)
    assert same["mean"] == 0.0 and all(v == 0.0 for v in same["levels"].values()) and sorted(same["levels"]) == [16, 32]
    other = R.swd(A, B, pos, dirs, 6)
    assert all(v > 0 for v in other["levels"].values())
    assert other["mean"] == pytest.approx(np.mean(list(other["levels"].values())), rel=1e-15)


def test_distance_is_invariant_under_a_per_channel_rescale_of_either_set():
    A, B = _sets(4)
    pos, dirs = R.draw_plan(np.random.RandomState(5), A.shape, 6, 2, 16)
    want = R.swd(A, B, pos, dirs, 6)
    a, b = np.array([0.5, 3.0, 7.0])[None, :, None, None], np.array([-2.0, 0.25, 10.0])[None, :, None, None]
    for got in (R.swd(a * A + b, B, pos, dirs, 6), R.swd(A, b + a * B, pos, dirs, 6)):
        for side, v in want["levels"].items():
            assert abs(got["levels"][side] - v) <= 1e-10 * max(1.0, abs(v))
        assert abs(got["mean"] - want["mean"]) <= 1e-10 * max(1.0, abs(want["mean"]))


def test_last_stage_by_hand():
    n = 37
    col = np.arange(n, dtype=np.float64)[::-1]
    pa = np.stack([col, col], 1)
    assert R.sliced_distance(pa, pa + 0.5) == 0.5                      # unsorted input: the sort is part of the stage
    assert R.sliced_distance(pa, pa[::-1]) == 0.0


def test_a_constant_channel_raises():
    A, B = _sets(6)
    B[:, 1] = 0.25
    pos, dirs = R.draw_plan(np.random.RandomState(7), A.shape, 6, 2, 16)
    with pytest.raises(ValueError, match="variance"):
        R.swd(A, B, pos, dirs, 6)
    with pytest.raises(ValueError):
        R.swd(A[:, :2], B[:, :2], pos, dirs, 6)                         # C = 2
    with pytest.raises(ValueError):
        R.swd(A[..., :24, :24], B[..., :24, :24], pos, dirs, 6)         # no power of two


def test_projection_folds_the_normalisation():
    A, _ = _sets(8)
    pos, dirs = R.draw_plan(np.random.RandomState(9), A.shape, 6, 1, 16)
    d = R.descriptors(A + 3.0, pos[0], 6)
    proj, bound = R.project(d, dirs[0][0])
    want = R.normalise(d).reshape(d.shape[0], -1) @ dirs[0][0]
    assert np.abs(proj - want).max() <= 1e-12 and bound.min() > 0
    assert np.abs(np.sqrt((dirs[0][0] ** 2).sum(0)) - 1).max() <= 1e-15


def test_entry_points_are_declared_exported_and_bound():
    eg = _pkg()
    protos = eg._lib.parse_header()
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    src = open(os.path.join(ROOT, "ead-gan_amd", "ops.py")).read()
    for name in NEW:
        assert name in protos and hasattr(cdll, name), name
        assert re.search(rf"""["']{name}["']""", src), f"{name} is not bound in ops.py"
    assert eg._lib.lib().query("eg_version") >= 111
    T = eg.ops.sort_tile_elems()
    assert T >= 2 and T & (T - 1) == 0
    assert eg.ops.swd_patch_stats_ws_doubles(3) > 0 and eg.ops.swd_project_ws_floats(3) >= (3 * 49 + 1) * 128 and eg.ops.l1_mean_ws_doubles() > 0
    assert callable(eg.ops.sort_columns) and "quality" in eg.__all__


def test_argument_errors_come_before_any_launch():
    eg = _pkg()
    q = eg.quality
    assert q.level_sides(64) == [64, 32, 16] == R.level_sides(64) and q.level_sides(16) == [16]
    for bad in (8, 48, 0):
        with pytest.raises(ValueError, match="power of two"):
            q.level_sides(bad)
    with pytest.raises(ValueError, match="multiple of batch"):
        q.generate("mnist", None, 12, 8)
    for kind in ("dsprites", "colored_train", "pxy"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            q.generate(kind, None, 16, 8)
        with pytest.raises(ValueError, match="disentanglement scores"):
            q.real_images(kind, None, 16)
    with pytest.raises(ValueError, match="'mnist' or 'celeba'"):
        q.generate("cifar", None, 16, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        import torch
        q.swd(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))
    assert q.SWDPlan(16) == (16, 0, 128, 4, 128)
    assert eg.train.swd_seed(3, 10) == eg.train.swd_seed(3, 10) != eg.train.swd_seed(3, 20)
    lib = eg._lib.lib()
    with pytest.raises(RuntimeError, match="power of two"):
        lib.call("eg_pyr_down", 1, 1, 1, 16, None)                      # the coarse side would be 8
    with pytest.raises(RuntimeError, match="ld >= n"):
        lib.call("eg_sort_columns_f32", 1, 8, 1, 4, None)
    with pytest.raises(RuntimeError, match="D <= 128"):
        lib.call("eg_swd_project", 1, 1, 8, 8, 1, 32, 1, 129, 1, 1, 1, 8, None)

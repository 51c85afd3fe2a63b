"""The kernel MMD without a GPU: the numpy restatement tests/mmd_refs.py against loops over Python numbers, the figures of that
restatement on the sets the GPU tests use, the four new entry points of the C ABI, the argument errors that come back before any launch,
and the run's seed."""
import ctypes
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import knn_refs
import mmd_refs as MR
import prdc_refs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eg_kernel_sum_ws_bytes", "eg_kernel_sum_u8", "eg_dist_select_ws_bytes", "eg_dist_select_u8")
PTR = 1 << 20           # a non-null, aligned address no failing call ever follows


def _pkg():
    return importlib.import_module("ead-gan_amd")


def _tiny(seed, n, m, K=5, hi=3):
    rng = np.random.RandomState(seed)
    return rng.randint(0, hi, (n, K)).astype(np.uint8), rng.randint(0, hi, (m, K)).astype(np.uint8)


def test_restated_select_equals_a_sorted_list_of_python_integers():
    real, fake = _tiny(0, 9, 7)
    fake[2], real[8] = real[4], real[1]
    for q, x, self0 in ((real, fake, -1), (real, real, 0), (real[3:7], real, 3), (real[7:], real, 7), (fake, real, 8), (fake, real, 20)):
        want = MR.pairs_brute(q, x, self0)
        assert MR.pairs(q, x, self0).tolist() == want, self0
        for rank in (0, len(want) // 2, len(want) - 1):
            assert MR.select(q, x, rank, self0) == (want[rank], 0)
        assert MR.select(q, x, len(want), self0) == (want[-1], 1) and MR.select(q, x, 10 ** 9, self0) == (want[-1], 1)
    assert MR.select(real[:1], real[:1], 0, self0=0) == (0, 1)


def test_ordered_pair_rank_is_the_lower_median_over_unordered_pairs():
    for seed, T in ((1, 2), (2, 3), (3, 8), (4, 9), (5, 12), (6, 13)):
        z, _ = _tiny(seed, T, 1, K=4, hi=2)                        # bytes in {0, 1}: at most five distinct distances, heavy ties
        P_ = T * (T - 1)
        assert MR.median_rank(T) == (P_ - 1) // 2
        ordered = MR.pairs_brute(z, z, 0)
        assert len(ordered) == P_ and ordered[(P_ - 1) // 2] == MR.median_unordered_brute(z) == MR.median_distance(z), T


def test_restated_sums_estimators_and_witness_equal_loops_with_math_exp():
    real, fake = _tiny(7, 6, 5, K=6, hi=4)
    fake[1] = real[2]
    for gamma in (0.7, 9.0, 400.0):
        ig = [1.0 / gamma, 1.0 / (3.0 * gamma)]
        for q, x, self0 in ((real, fake, -1), (real, real, 0), (fake[1:4], fake, 1), (fake, real, 4)):
            got, want = MR.kernel_sums(q, x, ig, self0), np.array(MR.kernel_sums_brute(q, x, ig, self0))
            assert np.abs(got - want).max() <= 4 * 2.0 ** -52 * want.max()
        u, b, wit = MR.mmd_brute(real, fake, gamma)
        got = MR.mmd(real, fake, bandwidths=[gamma])
        assert got["gamma_median"] is None and got["bandwidths"] == [gamma]
        assert abs(got["mmd2"][0] - u) <= 1e-15 and abs(got["mmd2_biased"][0] - b) <= 1e-15 and got["mean"] == got["mmd2"][0]
        assert np.abs(MR.witness(real, fake, np.concatenate((real, fake)), gamma) - np.array(wit)).max() <= 1e-15
    got = MR.mmd(real, fake, scales=(0.5, 2.0))
    med = MR.median_distance(np.concatenate((real, fake)))
    assert got["gamma_median"] == med > 0 and got["bandwidths"] == [0.5 * med, 2.0 * med] and got["mean"] == sum(got["mmd2"]) / 2
    # the biased estimate is a squared norm, the unbiased one of a set against itself is not positive on average: here, two copies
    same = MR.mmd(real, real.copy(), bandwidths=[9.0])
    assert same["mmd2_biased"][0] == 0.0 and same["mmd2"][0] < 0


def test_digit_boundary_rows_hold_the_distances_they_are_built_for():
    rows, ds = MR.digit_boundary_rows()
    assert rows.shape == (61, 32768) and ds == sorted(ds) and ds[:5] == [0, 1, 2, 3, 4] and ds[-2:] == [2 ** 30 - 1, 2 ** 30]
    assert knn_refs.distances(np.zeros((1, 32768), np.uint8), rows)[0].tolist() == ds
    for width in (8, 10, 11):                                      # whatever a pass's width, both sides of every digit boundary are there
        for shift in range(width, 31, width):
            assert 2 ** shift - 1 in ds and 2 ** shift in ds


def test_restated_figures_on_the_sets_of_the_gpu_test():
    a, b = P.clustered()
    got = MR.mmd(a, b)
    assert got["gamma_median"] == 320436 and got["bandwidths"] == [160218.0, 320436.0, 640872.0]
    assert [round(v, 6) for v in got["mmd2"]] == [0.137202, 0.104315, 0.066488] and round(got["mean"], 6) == 0.102668
    assert all(bi > un > 0 for bi, un in zip(got["mmd2_biased"], got["mmd2"]))
    halves = MR.mmd(a[0::2], a[1::2])                              # two disjoint halves of the real set: the same distribution
    assert halves["gamma_median"] == 313690 and all(abs(v) < 0.02 for v in halves["mmd2"])
    assert all(g > 5 * abs(h) for g, h in zip(got["mmd2"], halves["mmd2"])) and got["mean"] > 5 * abs(halves["mean"])
    back = MR.mmd(b, a)                                            # the estimate is symmetric in its two sets
    assert back["gamma_median"] == got["gamma_median"] and all(abs(u - v) < 1e-14 for u, v in zip(back["mmd2"], got["mmd2"]))
    w = MR.witness(a, b, np.concatenate((a, b)), float(got["gamma_median"]))
    assert (w[100:150] > 0).all() and (w[250:] < 0).all() and abs(w[:100].mean()) < 0.2 * w[100:150].mean()
    dup = np.concatenate((np.repeat(a[7:8], 40, 0), a[:6]))
    assert MR.median_distance(np.concatenate((dup, dup))) == 0
    assert MR.tolerance(150) == 158 * 2.0 ** -52 < 4e-14


def test_entry_points_are_declared_exported_and_bound():
    eg = _pkg()
    protos = eg._lib.parse_header()
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    src = open(os.path.join(ROOT, "ead-gan_amd", "ops.py")).read()
    for name in NEW:
        assert name in protos and hasattr(cdll, name), name
        assert re.search(rf"""["']{name}["']""", src), f"{name} is not bound in ops.py"
    assert eg._lib.lib().query("eg_version") >= 114
    ks, ds = protos["eg_kernel_sum_u8"][1], protos["eg_dist_select_u8"][1]
    assert len(ks) == 12 and ks[6] is ctypes.c_int and ks[7] is ctypes.c_longlong                 # nb, self0
    assert len(ds) == 10 and ds[5] is ctypes.c_longlong and ds[6] is ctypes.c_ulonglong           # self0, rank
    assert len(protos["eg_kernel_sum_ws_bytes"][1]) == 3 and len(protos["eg_dist_select_ws_bytes"][1]) == 2
    for fn in ("median_distance", "mmd", "mmd_sums", "mmd_witness", "mmd_generator", "MMDPlan"):
        assert callable(getattr(eg.quality, fn)), fn
    assert eg.quality.MMDPlan(16) == (16, (0.5, 1.0, 2.0), 0)
    assert "6p" in eg.quality.__doc__ and "mmd_witness" in eg.quality.__doc__


def test_workspaces():
    ops = _pkg().ops
    Tq, Tr = ops.knn_tile_queries(), ops.knn_tile_rows()
    for nq, n in ((1, 1), (64, 202599), (8192, 8192), (17, 300), (1, Tr + 1), (4 * Tq, 5 * Tr)):
        for nb in (1, 3, 4):
            assert ops.kernel_sum_ws_bytes(nq, n, nb) == ops.knn_splits(nq, n) * nq * nb * 8, (nq, n, nb)
        wgs = -(-nq // (2 * Tq if nq >= 4 * Tq else Tq)) * ops.knn_splits(nq, n)
        assert ops.dist_select_ws_bytes(nq, n) == 64 + 32 * 8192 + wgs * 4096, (nq, n)
    assert ops.kernel_sum_ws_bytes(0, 5, 1) == 0 and ops.kernel_sum_ws_bytes(5, 5, 0) == 0 and ops.dist_select_ws_bytes(5, 0) == 0


def test_argument_errors_of_the_library_come_back_without_a_gpu():
    lib = _pkg()._lib.lib()

    def ksum(nq=4, n=8, K=64, nb=3, self0=-1, q=PTR, x=PTR, ig=PTR, ws=PTR, out=PTR, flag=PTR):
        lib.call("eg_kernel_sum_u8", q, nq, x, n, K, ig, nb, self0, ws, out, flag, None)

    def select(nq=4, n=8, K=64, self0=-1, rank=0, q=PTR, x=PTR, ws=PTR, out=PTR):
        lib.call("eg_dist_select_u8", q, nq, x, n, K, self0, rank, ws, out, None)

    for call, pointers in ((ksum, ("q", "x", "ig", "ws", "out", "flag")), (select, ("q", "x", "ws", "out"))):
        for K in (65, 32832, 0, 32):
            with pytest.raises(RuntimeError, match="row length"):
                call(K=K)
        for name in pointers:
            with pytest.raises(RuntimeError, match="null pointer"):
                call(**{name: None})
        with pytest.raises(RuntimeError, match="nq >= 1"):
            call(nq=0)
        with pytest.raises(RuntimeError, match="n >= 1"):
            call(n=0)
        for name in ("q", "x"):
            with pytest.raises(RuntimeError, match="16-byte"):
                call(**{name: PTR + 8})
    for nb in (0, 5, -1):
        with pytest.raises(RuntimeError, match="1 <= nb <= 4"):
            ksum(nb=nb)
    for name in ("ig", "ws", "out"):
        with pytest.raises(RuntimeError, match="8-byte"):
            ksum(**{name: PTR + 4})
    with pytest.raises(RuntimeError, match="4-byte"):
        ksum(flag=PTR + 2)
    with pytest.raises(RuntimeError, match="8-byte"):
        select(ws=PTR + 4)
    with pytest.raises(RuntimeError, match="4-byte"):
        select(out=PTR + 2)


def test_every_value_error_of_the_front_ends_from_cpu_tensors():
    eg = _pkg()
    ops = eg.ops
    z = torch.zeros(4, 64, dtype=torch.uint8)
    ig = torch.ones(3, dtype=torch.float64)
    for call in (lambda a, b: ops.kernel_sum_u8(a, b, ig), lambda a, b: ops.dist_select_u8(a, b, 0)):
        for bad in (z.float(), z[:, 0], z[:, ::2], None):
            with pytest.raises(ValueError, match="contiguous uint8 device tensor"):
                call(bad, z)
            with pytest.raises(ValueError, match="contiguous uint8 device tensor"):
                call(z, bad)
        with pytest.raises(ValueError, match="one length"):
            call(z, torch.zeros(4, 128, dtype=torch.uint8))
        with pytest.raises(ValueError, match="one length"):
            call(z[:0], z)
        for K in (63, 32, 32832):
            with pytest.raises(ValueError, match="row length"):
                call(torch.zeros(2, K, dtype=torch.uint8), torch.zeros(3, K, dtype=torch.uint8))
        with pytest.raises(ValueError, match="no CPU path"):       # everything else is in order: the device is asked last
            call(z, z)
    for bad in (ig.float(), torch.ones(5, dtype=torch.float64), torch.ones(0, dtype=torch.float64), ig.reshape(3, 1), torch.ones(6, dtype=torch.float64)[::2],
                [1.0, 2.0], None):
        with pytest.raises(ValueError, match="inv_gamma must be"):
            ops.kernel_sum_u8(z, z, bad)
    for bad in (torch.zeros(4, 2, dtype=torch.float64), torch.zeros(4, 3), torch.zeros(3, 4, dtype=torch.float64).t(), 5):
        with pytest.raises(ValueError, match="out must be"):
            ops.kernel_sum_u8(z, z, ig, out=bad)
    for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 0):
        with pytest.raises(ValueError, match="flag must be"):
            ops.kernel_sum_u8(z, z, ig, flag=bad)
    for rank in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="rank"):
            ops.dist_select_u8(z, z, rank)
    # quality: the image sets
    u = z.reshape(4, 1, 8, 8)
    for fn in (lambda: eg.quality.mmd(u, u), lambda: eg.quality.median_distance(u), lambda: eg.quality.mmd_witness(u, u, u, 1.0),
               lambda: eg.quality.mmd(torch.zeros(4, 1, 8, 8), u)):
        with pytest.raises(ValueError, match="device tensor"):
            fn()
    for kind in ("dsprites", "colored_train", "pxy"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.mmd_generator(kind, None, None)
    for name, bad in (("scales", ()), ("scales", (1, 2, 3, 4, 5)), ("scales", (0.0,)), ("scales", (1.0, -2.0)), ("scales", (math.inf,)),
                      ("scales", (math.nan,)), ("scales", 3), ("bandwidth", (0.0,))):
        with pytest.raises(ValueError, match=f"{name} must be"):
            eg.quality._positive(bad, "mmd", name)
    assert eg.quality._positive((0.5, 2), "mmd", "scales") == [0.5, 2.0]


def test_plan_validation_of_a_run_needs_no_gpu():
    eg = _pkg()
    Plan = eg.quality.MMDPlan

    def check(plan, kind="mnist", n_dataset=20, batch=8):
        return eg.train.check_plan("mmd", plan, Plan, kind, n_dataset, batch)

    assert check(Plan(16)) == (16, (0.5, 1.0, 2.0), 0) and check((16, (1.0,), 4)) == Plan(16, (1.0,), 4) and check(Plan(4), batch=8) == Plan(4)
    for kind in ("pxy", "dsprites", "colored"):
        with pytest.raises(ValueError, match="mmd: only 'mnist' and 'celeba'"):
            check(Plan(16), kind=kind)
    with pytest.raises(ValueError, match="mmd: n_images = 64, the dataset has 20 images"):
        check(Plan(64))
    with pytest.raises(ValueError, match="mmd: n_images = 0, the dataset has"):
        check(Plan(0))
    with pytest.raises(ValueError, match="mmd: n_images = 12 is no multiple of the trainer's batch size 8"):
        check(Plan(12))
    with pytest.raises(ValueError, match="mmd: n_images = 1, the estimate needs at least 2"):
        check(Plan(1))
    for scales in ((), (1, 2, 3, 4, 5), (0.0,), (1.0, -1.0), (math.nan,)):
        with pytest.raises(ValueError, match="mmd: .*scales must be"):
            check(Plan(16, scales))


def test_the_run_seeds_its_scores_apart_from_the_other_draws():
    train = _pkg().train
    for seed, it in ((0, 0), (3, 10), (7, 4000)):
        assert len({train.mmd_seed(seed, it), train.nn_seed(seed, it), train.swd_seed(seed, it), train.sample_seed(seed, it)}) == 4
        assert 0 <= train.mmd_seed(seed, it) < 2 ** 32
    assert train.mmd_seed(3, 10) == train.mmd_seed(3, 10) != train.mmd_seed(3, 20)
    assert train.mmd_seed(3, 10, 1) != train.mmd_seed(3, 10) != train.mmd_seed(4, 10)

"""The Sinkhorn divergence without a GPU: the numpy restatement tests/sinkhorn_refs.py against loops over Python numbers and
against the properties the definition implies (one image a set, equal sets, the exact assignment as epsilon -> 0), the two new entry
points of the C ABI, the argument errors that come back before any launch, and the run's plan and seed."""
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
import sinkhorn_refs as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eg_softmin_ws_bytes", "eg_softmin_u8")
PTR = 1 << 20           # a non-null, aligned address no failing call ever follows


def _pkg():
    return importlib.import_module("ead-gan_amd")


def _tiny(seed, n, m, K=5, hi=3):
    rng = np.random.RandomState(seed)
    return rng.randint(0, hi, (n, K)).astype(np.uint8), rng.randint(0, hi, (m, K)).astype(np.uint8)


def test_restated_softmin_equals_loops_over_python_numbers():
    real, fake = _tiny(0, 9, 7, K=6, hi=5)
    rng = np.random.RandomState(1)
    for ie in (3.0, 0.05, 40.0):                                   # t spans a fraction of a unit, and hundreds of units
        for q, x, self0 in ((real, fake, -1), (real, real, 0), (real[3:7], real, 3), (real[7:], real, 7), (fake, real, 8), (fake, real, 20)):
            g = rng.uniform(-30.0, 30.0, len(x))
            prev = rng.uniform(-5.0, 5.0, len(q))
            st = {}
            got, want = SR.softmin(q, x, g, ie, self0, stats=st), np.array(SR.softmin_brute(q, x, g, ie, self0))
            scale = (st["tmax"] + math.log(len(x))) / ie           # the size of a result: a handful of roundings at that size
            assert np.abs(got - want).max() <= 8 * 2.0 ** -53 * scale, (ie, self0)
            avg = SR.softmin(q, x, g, ie, self0, prev)
            assert np.abs(avg - np.array(SR.softmin_brute(q, x, g, ie, self0, prev))).max() <= 8 * 2.0 ** -53 * (scale + 5.0)
            assert np.array_equal(avg, 0.5 * prev + 0.5 * got)
    # the soft minimum lies between the minimum and the mean of d - g, and tends to the minimum as the temperature falls
    d = knn_refs.distances(real, fake).astype(np.float64)
    g = rng.uniform(-3.0, 3.0, len(fake))
    cold, warm = SR.softmin(real, fake, g, 200.0), SR.softmin(real, fake, g, 1e-4)
    assert ((d - g).min(1) <= cold).all() and (cold <= (d - g).min(1) + math.log(7) / 200.0 + 1e-12).all()
    gap = (d - g).mean(1) - warm                                   # mean - var / (2 eps) to second order
    assert (gap >= 0).all() and (gap <= 1e-4 * (d - g).var(1)).all() and (cold <= warm).all()


def test_one_image_a_set_gives_the_distance_between_the_two():
    a, b = _tiny(3, 1, 1, K=64, hi=256)
    d = int(knn_refs.distances(a, b)[0, 0])
    det = {}
    got = SR.sinkhorn(a, b, detail=det)
    assert got["gamma_median"] == d > 0 and got["epsilon"] == 0.1 * d and got["iterations"] == 60
    assert abs(got["ot_xy"] - d) <= det["bound"] and abs(got["divergence"] - d) <= det["bound"] and det["bound"] < 1e-9 * d
    assert got["ot_xx"] == 0.0 and got["ot_yy"] == 0.0 and got["relative"] == got["divergence"] / d
    assert got["marginal_error"] < 1e-12


def test_small_epsilon_reaches_the_exact_assignment():
    rng = np.random.RandomState(5)
    X = rng.randint(60, 196, (6, 64)).astype(np.uint8)
    Y = (X[rng.permutation(6)].astype(np.int64) + rng.randint(-55, 56, (6, 64))).astype(np.uint8)
    d = knn_refs.distances(X, Y)
    want = SR.assignment_cost(X, Y)
    # well separated: a row's partner is far nearer than its second choice, and yet not so near that the entropy of the plan, eps log 6,
    # exceeds the 1 % asked of ot_xy
    assert 0.18 * MR.median_distance(np.concatenate((X, Y))) < want < 0.35 * np.sort(d, 1)[:, 1].min()
    got = SR.sinkhorn(X, Y, scale=1e-3, iterations=400)
    print(want, got)
    assert abs(got["ot_xy"] - want) <= 0.01 * want
    assert got["marginal_error"] < 1e-6
    assert abs(got["divergence"] - want) <= 1e-9 * want            # the debiasing takes the entropy term out


def test_equal_sets_give_exactly_zero_and_other_sets_a_positive_divergence():
    a, b = SR.clustered()
    det = {}
    same = SR.sinkhorn(a[::4], a[::4].copy(), detail=det)
    assert same["divergence"] == 0.0 and same["relative"] == 0.0 and same["ot_xy"] == same["ot_xx"] == same["ot_yy"]
    assert np.array_equal(det["f"], det["g"]) and np.array_equal(det["f"], det["p"]) and np.array_equal(det["f"], det["r"])
    got = SR.sinkhorn(a[::4], b[::3], detail=det)                  # 50 + 44 rows, two against three clusters
    assert got["divergence"] > 0 and got["ot_xy"] > 0.5 * (got["ot_xx"] + got["ot_yy"]) and got["marginal_error"] < 1e-2
    assert abs(got["divergence"] - (got["ot_xy"] - 0.5 * got["ot_xx"] - 0.5 * got["ot_yy"])) <= 1e-9 * got["ot_xy"]
    assert got["epsilon"] == 0.1 * got["gamma_median"] == det["schedule"][-1] and det["schedule"][0] == knn_refs.distances(
        np.concatenate((a[::4], b[::3])), np.concatenate((a[::4], b[::3]))).max()
    assert (np.diff(det["schedule"]) <= 0).all()
    share_y = det["g"] - det["r"]                                  # the samples around the foreign centre are the ones far from the data
    assert share_y[-10:].min() > 3 * np.abs(share_y[:-10]).max()
    fixed = SR.sinkhorn(a[::4], b[::3], epsilon=20000.0)
    assert fixed["gamma_median"] is None and fixed["relative"] is None and fixed["epsilon"] == 20000.0
    halves = SR.sinkhorn(a[0::2], a[1::2])                         # two halves of one distribution: far below two different ones
    far = SR.sinkhorn(a, b)
    assert 0 <= halves["divergence"] < 0.05 * far["divergence"]
    assert SR.tolerance(130, 1000.0, 300.0) == 1000.0 * (276 * 2.0 ** -52 + 1200 * 2.0 ** -53) < 2e-10


def test_entry_points_are_declared_exported_and_bound():
    eg = _pkg()
    protos = eg._lib.parse_header()
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    src = open(os.path.join(ROOT, "ead-gan_amd", "ops.py")).read()
    for name in NEW:
        assert name in protos and hasattr(cdll, name), name
        assert re.search(rf"""["']{name}["']""", src), f"{name} is not bound in ops.py"
    assert eg._lib.lib().query("eg_version") >= 115
    sm = protos["eg_softmin_u8"][1]
    assert len(sm) == 13 and sm[7] is ctypes.c_longlong and len(protos["eg_softmin_ws_bytes"][1]) == 2      # self0
    for fn in ("sinkhorn", "sinkhorn_generator", "SinkhornPlan"):
        assert callable(getattr(eg.quality, fn)), fn
    assert eg.quality.SinkhornPlan(16) == (16, 0.1, 60, 0)
    assert "6q" in eg.quality.__doc__ and "sinkhorn_generator" in eg.quality.__doc__
    ops = eg.ops
    Tq, Tr = ops.knn_tile_queries(), ops.knn_tile_rows()
    for nq, n in ((1, 1), (64, 202599), (8192, 8192), (17, 300), (1, Tr + 1), (4 * Tq, 5 * Tr)):
        assert ops.softmin_ws_bytes(nq, n) == ops.knn_splits(nq, n) * nq * 16, (nq, n)
    assert ops.softmin_ws_bytes(0, 5) == 0 and ops.softmin_ws_bytes(5, 0) == 0


def test_argument_errors_of_the_library_come_back_without_a_gpu():
    lib = _pkg()._lib.lib()

    def call(nq=4, n=8, K=64, self0=-1, q=PTR, x=PTR, g=PTR, ie=PTR, prev=None, ws=PTR, out=PTR, flag=PTR):
        lib.call("eg_softmin_u8", q, nq, x, n, K, g, ie, self0, prev, ws, out, flag, None)

    for K in (65, 32832, 0, 32):
        with pytest.raises(RuntimeError, match="row length"):
            call(K=K)
    for name in ("q", "x", "g", "ie", "ws", "out", "flag"):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(**{name: None})
    with pytest.raises(RuntimeError, match="nq >= 1"):
        call(nq=0)
    with pytest.raises(RuntimeError, match="n >= 1"):
        call(n=0)
    for nq in (1, 4):                                              # query 0 is the database's only row
        with pytest.raises(RuntimeError, match="no candidate"):
            call(nq=nq, n=1, self0=0)
    for name in ("q", "x"):
        with pytest.raises(RuntimeError, match="16-byte"):
            call(**{name: PTR + 8})
    for name in ("g", "ie", "prev", "ws", "out"):
        with pytest.raises(RuntimeError, match="8-byte"):
            call(**{name: PTR + 4})
    with pytest.raises(RuntimeError, match="4-byte"):
        call(flag=PTR + 2)


def test_every_value_error_of_the_front_ends_from_cpu_tensors():
    eg = _pkg()
    ops = eg.ops
    z = torch.zeros(4, 64, dtype=torch.uint8)
    g, ie = torch.zeros(4, dtype=torch.float64), torch.ones(1, dtype=torch.float64)
    call = lambda a, b: ops.softmin_u8(a, b, g, ie)
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
            call(torch.zeros(2, K, dtype=torch.uint8), torch.zeros(4, K, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU path"):           # everything else is in order: the device is asked last
        call(z, z)
    for bad in (g.float(), torch.zeros(5, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)[::2], g.reshape(4, 1), [0.0] * 4, None):
        with pytest.raises(ValueError, match="g must be"):
            ops.softmin_u8(z, z, bad, ie)
    for bad in (ie.float(), torch.ones(2, dtype=torch.float64), 1.0, None):
        with pytest.raises(ValueError, match="inv_eps must be"):
            ops.softmin_u8(z, z, g, bad)
    for name in ("prev", "out"):
        for bad in (g.float(), torch.zeros(3, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)[::2], 5):
            with pytest.raises(ValueError, match=f"{name} must be"):
                ops.softmin_u8(z, z, g, ie, **{name: bad})
    for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 0):
        with pytest.raises(ValueError, match="flag must be"):
            ops.softmin_u8(z, z, g, ie, flag=bad)
    with pytest.raises(ValueError, match="no candidate"):
        ops.softmin_u8(z[:1], z[:1], g[:1], ie, self0=0)
    # quality: the image sets
    u = z.reshape(4, 1, 8, 8)
    for fn in (lambda: eg.quality.sinkhorn(u, u), lambda: eg.quality.sinkhorn(torch.zeros(4, 1, 8, 8), u)):
        with pytest.raises(ValueError, match="device tensor"):
            fn()
    for kind in ("dsprites", "colored_train", "pxy"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.sinkhorn_generator(kind, None, None)


def test_plan_validation_of_a_run_needs_no_gpu():
    eg = _pkg()
    Plan = eg.quality.SinkhornPlan

    def check(plan, kind="mnist", n_dataset=20, batch=8):
        return eg.train.check_plan("sinkhorn", plan, Plan, kind, n_dataset, batch)

    assert check(Plan(16)) == (16, 0.1, 60, 0) and check((16, 0.5, 10, 4)) == Plan(16, 0.5, 10, 4) and check(Plan(4), batch=8) == Plan(4)
    for kind in ("pxy", "dsprites", "colored"):
        with pytest.raises(ValueError, match="sinkhorn: only 'mnist' and 'celeba'"):
            check(Plan(16), kind=kind)
    with pytest.raises(ValueError, match="sinkhorn: n_images = 64, the dataset has 20 images"):
        check(Plan(64))
    with pytest.raises(ValueError, match="sinkhorn: n_images = 12 is no multiple of the trainer's batch size 8"):
        check(Plan(12))
    with pytest.raises(ValueError, match="sinkhorn: n_images = 1, the divergence needs at least 2"):
        check(Plan(1))
    for scale in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="sinkhorn: .*scale must be"):
            check(Plan(16, scale))
    with pytest.raises(ValueError, match="sinkhorn: iterations = 0"):
        check(Plan(16, 0.1, 0))


def test_the_run_seeds_its_scores_apart_from_the_other_draws():
    train = _pkg().train
    for seed, it in ((0, 0), (3, 10), (7, 4000)):
        seeds = {train.sinkhorn_seed(seed, it), train.mmd_seed(seed, it), train.nn_seed(seed, it), train.swd_seed(seed, it), train.sample_seed(seed, it)}
        assert len(seeds) == 5 and 0 <= train.sinkhorn_seed(seed, it) < 2 ** 32
    assert train.sinkhorn_seed(3, 10) == train.sinkhorn_seed(3, 10) != train.sinkhorn_seed(3, 20)
    assert train.sinkhorn_seed(3, 10, 1) != train.sinkhorn_seed(3, 10) != train.sinkhorn_seed(4, 10)

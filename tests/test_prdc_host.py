"""Precision, recall, density and coverage without a GPU: the int64 restatement tests/prdc_refs.py against loops over Python
integers, the two new entry points of the C ABI, the argument errors that come back before any launch, and the run's seed."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import knn_refs
import prdc_refs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eg_ball_count_ws_bytes", "eg_ball_count_u8")
PTR = 1 << 20           # a non-null, aligned address no failing call ever follows


def _pkg():
    return importlib.import_module("ead-gan_amd")


def test_restatement_equals_loops_over_python_integers():
    rng = np.random.RandomState(0)
    real = rng.randint(0, 3, (9, 5)).astype(np.uint8)              # small values: many equal distances, the <= edge is hit
    fake = rng.randint(0, 3, (7, 5)).astype(np.uint8)
    fake[2] = real[4]
    real[8] = real[1]
    for k in (1, 2, 3, 6):
        assert P.prdc(real, fake, k) == P.prdc_brute(real, fake, k), k
        assert P.prdc(fake, real, k) == P.prdc_brute(fake, real, k), k
    rad = P.radii(real, 2)
    assert np.array_equal(rad, [sorted(int(v) for j, v in enumerate(row) if j != i)[1] for i, row in enumerate(knn_refs.distances(real, real))])
    for self0 in (-1, 0, 3, 8, 20):
        q = real[self0:self0 + 4] if 0 <= self0 < 9 else fake
        assert np.array_equal(P.ball_count(q, real, rad, self0), P.ball_count_brute(q, real, rad, self0)), self0
    d = knn_refs.distances(fake, real)
    assert (d == rad[None, :]).any()                               # the data does reach the edge
    assert np.array_equal(P.ball_count(fake, real, rad), (d <= rad[None, :]).sum(1))
    assert not np.array_equal(P.ball_count(fake, real, rad), (d < rad[None, :]).sum(1))
    assert not P.ball_count(fake, real, np.full(9, -1)).any()      # a negative radius is an empty ball
    assert P.ball_count(real[1:2], real, np.zeros(9, np.int64)).tolist() == [2]        # rad = 0: the row and its copy
    assert P.ball_count(real[1:2], real, np.zeros(9, np.int64), self0=1).tolist() == [1]


def test_restated_scores_on_sets_whose_answer_is_known():
    a, b = P.clustered()
    assert a.shape == (150, 64) and b.shape == (131, 64)
    same = P.prdc(a, a, 5)
    assert same["precision"] == (150, 150) and same["recall"] == (150, 150) and same["coverage"] == (150, 150)
    one = np.repeat(a[7:8], 131, 0)
    got = P.prdc(a, one, 5)
    assert got["precision"] == (131, 131) and got["recall"] == (1, 150)            # every copy has radius 0 and holds row 7 alone
    far = P.prdc((a // 4).astype(np.uint8), (192 + b // 4).astype(np.uint8), 5)
    assert [v[0] for v in far.values()] == [0, 0, 0, 0]
    got = P.prdc(a, b, 5)
    assert all(0 < num < den for num, den in got.values()) and got != P.prdc(a, b, 3)


def test_entry_points_are_declared_exported_and_bound():
    eg = _pkg()
    protos = eg._lib.parse_header()
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    src = open(os.path.join(ROOT, "ead-gan_amd", "ops.py")).read()
    for name in NEW:
        assert name in protos and hasattr(cdll, name), name
        assert re.search(rf"""["']{name}["']""", src), f"{name} is not bound in ops.py"
    assert eg._lib.lib().query("eg_version") >= 113
    assert protos["eg_ball_count_u8"][1][6] is ctypes.c_longlong        # self0
    assert len(protos["eg_ball_count_u8"][1]) == 10 and len(protos["eg_ball_count_ws_bytes"][1]) == 2
    for fn in ("knn_radii", "prdc", "prdc_generator", "NNPlan"):
        assert callable(getattr(eg.quality, fn)), fn
    assert "CLOSED" in eg.quality.prdc.__doc__ and "CLOSED" in eg.ops.ball_count_u8.__doc__
    assert eg.quality.NNPlan(16) == (16, 5, 0)


def test_workspace_is_one_int_per_slice_and_query():
    ops = _pkg().ops
    Tr = ops.knn_tile_rows()
    for nq, n in ((1, 1), (64, 202599), (8192, 8192), (17, 300), (1, Tr + 1)):
        assert ops.ball_count_ws_bytes(nq, n) == ops.knn_splits(nq, n) * nq * 4, (nq, n)
    assert ops.ball_count_ws_bytes(0, 5) == 0


def test_argument_errors_come_back_without_a_gpu():
    eg = _pkg()
    lib = eg._lib.lib()

    def call(nq=4, n=8, K=64, self0=-1, q=PTR, x=PTR, rad=PTR, ws=PTR, count=PTR):
        lib.call("eg_ball_count_u8", q, nq, x, n, K, rad, self0, ws, count, None)

    for K in (65, 32832, 0, 32):
        with pytest.raises(RuntimeError, match="row length"):
            call(K=K)
    for name in ("q", "x", "rad", "ws", "count"):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(**{name: None})
    with pytest.raises(RuntimeError, match="nq >= 1"):
        call(nq=0)
    with pytest.raises(RuntimeError, match="n >= 1"):
        call(n=0)
    for name in ("q", "x"):
        with pytest.raises(RuntimeError, match="16-byte"):
            call(**{name: PTR + 8})
    for name in ("rad", "ws", "count"):
        with pytest.raises(RuntimeError, match="4-byte"):
            call(**{name: PTR + 2})
    z = torch.zeros(4, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        eg.ops.ball_count_u8(z, z, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="device tensor"):
        eg.quality.prdc(z.reshape(4, 1, 8, 8), z.reshape(4, 1, 8, 8))
    with pytest.raises(ValueError, match="device tensor"):
        eg.quality.knn_radii(torch.zeros(4, 1, 8, 8))
    for kind in ("dsprites", "colored_train", "pxy"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.prdc_generator(kind, None, None)


def test_the_run_seeds_its_scores_apart_from_the_other_draws():
    train = _pkg().train
    for seed, it in ((0, 0), (3, 10), (7, 4000)):
        assert len({train.nn_seed(seed, it), train.swd_seed(seed, it), train.sample_seed(seed, it)}) == 3
        assert 0 <= train.nn_seed(seed, it) < 2 ** 32
    assert train.nn_seed(3, 10) == train.nn_seed(3, 10) != train.nn_seed(3, 20)
    assert train.nn_seed(3, 10, 1) != train.nn_seed(3, 10) != train.nn_seed(4, 10)

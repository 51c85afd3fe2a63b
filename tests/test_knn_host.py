"""The exact nearest-neighbour search without a GPU: the int64 restatement tests/knn_refs.py against a brute-force double loop,
the new entry points of the C ABI, their tile and split queries, and the argument errors that come back before any launch."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import knn_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eg_knn_tile_queries", "eg_knn_tile_rows", "eg_knn_splits", "eg_knn_ws_bytes", "eg_knn_u8")
PTR = 1 << 20           # a non-null, aligned address no failing call ever follows


def _pkg():
    return importlib.import_module("ead-gan_amd")


def test_restatement_equals_a_brute_force_double_loop():
    rng = np.random.RandomState(0)
    x = rng.randint(0, 256, (9, 6)).astype(np.uint8)
    x[5] = x[2]                                         # a tie at distance 0 for query rows 2 and 5
    x[7, :] = 255
    x[8, :] = 0
    q = x[1:7]
    for k, self0 in ((1, -1), (3, -1), (4, 1), (8, 1), (9, -1), (3, 6)):
        d, i = R.knn(q, x, k, self0)
        bd, bi = R.knn_brute(q, x, k, self0)
        assert np.array_equal(d, bd) and np.array_equal(i, bi), (k, self0)
    d, i = R.knn(q, x, 2, 1)                            # q[i] = x[1 + i]: nobody finds itself, row 2 finds its copy 5 and 5 finds 2
    assert not np.any(i == np.arange(1, 7)[:, None]) and i[1, 0] == 5 and i[4, 0] == 2 and d[1, 0] == 0
    d, i = R.knn(q, x, 1)
    assert np.array_equal(i[:, 0], [1, 2, 3, 4, 2, 6]) and not d.any()          # ties go to the lower index: query 4 (= row 5) finds row 2
    assert R.distances(x[7:8], x[8:9])[0, 0] == 255 * 255 * 6


def test_restated_two_sample_counts_grid_and_bytes():
    a = np.zeros((4, 1, 2, 2), np.uint8) + np.arange(4, dtype=np.uint8)[:, None, None, None]
    b = a + 200
    assert R.two_sample_counts(a, b) == (4, 4, 4)
    assert R.two_sample_counts(a, a) == (0, 0, 4)       # every row's nearest other row is its copy in the other set
    assert R.two_sample_counts(a[[0, 0, 1, 1]], a[[0, 0, 1, 1]]) == (4, 0, 4)      # duplicated rows tie at 0: the lower (real) index wins
    g = R.grid(a[:2], b, np.array([[3, 0], [1, 1]]))
    assert g.shape == (6, 1, 2, 2) and g.dtype == np.float32
    assert np.array_equal((g[:, 0, 0, 0] * 255).round(), [0, 203, 200, 1, 201, 201])
    u = np.arange(256, dtype=np.float32)
    for v in (np.float32(2.0 / 255.0) * u - np.float32(1.0), np.float32(np.float64(np.float32(2.0 / 255.0)) * u - 1.0)):       # with and without an fma
        assert np.array_equal(R.to_u8(v), np.arange(256))
    assert np.array_equal(R.to_u8([-3.0, -1.0, 1.0, 7.5]), [0, 0, 255, 255])


def test_entry_points_are_declared_exported_and_bound():
    eg = _pkg()
    protos = eg._lib.parse_header()
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    src = open(os.path.join(ROOT, "ead-gan_amd", "ops.py")).read()
    for name in NEW:
        assert name in protos and hasattr(cdll, name), name
        assert re.search(rf"""["']{name}["']""", src), f"{name} is not bound in ops.py"
    assert eg._lib.lib().query("eg_version") >= 112
    assert protos["eg_knn_u8"][1][6] is ctypes.c_longlong               # self0
    for fn in ("to_u8", "nearest_neighbours", "nn_two_sample", "neighbour_grid", "save_neighbours", "nearest_training_images", "nn_generator"):
        assert callable(getattr(eg.quality, fn)), fn
    assert "lower index" in eg.quality.nn_two_sample.__doc__


def test_tile_and_split_queries_are_positive_and_stable():
    ops = _pkg().ops
    Tq, Tr = ops.knn_tile_queries(), ops.knn_tile_rows()
    assert Tq >= 16 and Tr >= 16 and (Tq, Tr) == (ops.knn_tile_queries(), ops.knn_tile_rows())
    lib = _pkg()._lib.lib()
    for nq, n in ((1, 1), (64, 202599), (16384, 16384), (17, 300), (1, Tr), (1, Tr + 1), (5 * Tq, 10 * Tr)):
        s = ops.knn_splits(nq, n)
        assert 1 <= s <= -(-n // Tr) and s == ops.knn_splits(nq, n), (nq, n, s)       # a slice is at least one tile
        for k in (1, 16):
            assert lib.query("eg_knn_ws_bytes", nq, n, k) >= s * nq * k * 8
    assert ops.knn_splits(1, Tr) == 1
    assert ops.knn_splits(64, 202599) >= 2              # 64 queries are one tile of queries: only slices of the database fill the chip


def test_argument_errors_come_back_without_a_gpu():
    eg = _pkg()
    lib = eg._lib.lib()

    def call(nq=4, n=8, K=64, k=2, self0=-1, q=PTR, x=PTR, ws=PTR, dist=PTR, idx=PTR):
        lib.call("eg_knn_u8", q, nq, x, n, K, k, self0, ws, dist, idx, None)

    for K in (65, 32832, 0, 32):
        with pytest.raises(RuntimeError, match="row length"):
            call(K=K)
    for k in (0, 17):
        with pytest.raises(RuntimeError, match="1 <= k <= 16"):
            call(k=k)
    with pytest.raises(RuntimeError, match="candidates"):
        call(n=8, k=8, self0=0)                         # k = n with a row excluded
    with pytest.raises(RuntimeError, match="candidates"):
        call(n=8, k=9)
    for name in ("q", "x", "ws", "dist", "idx"):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(**{name: None})
    with pytest.raises(RuntimeError, match="nq >= 1"):
        call(nq=0)
    import torch
    z = torch.zeros(4, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        eg.ops.knn_u8(z, z, 1)
    with pytest.raises(ValueError, match="device tensor"):
        eg.quality.to_u8(torch.zeros(2, 1, 8, 8))
    with pytest.raises(ValueError, match="device"):
        eg.quality.nearest_neighbours(torch.zeros(2, 1, 8, 8), z.reshape(4, 1, 8, 8))
    for kind in ("dsprites", "colored_train", "pxy"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.nearest_training_images(kind, None, None)
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.nn_generator(kind, None, None)

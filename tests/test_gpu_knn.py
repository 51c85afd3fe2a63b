"""The exact nearest-neighbour search on the MI355X: ops.knn_u8 and the functions of quality.py built on it against the int64
restatement tests/knn_refs.py.  The distances are integers and the order (distance, index) is total, so every comparison is torch.equal /
==: there is no tolerance anywhere in this file."""
import importlib

import numpy as np
import pytest
import torch

import knn_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _tiles():
    ops = importlib.import_module("ead-gan_amd").ops
    return ops.knn_tile_queries(), ops.knn_tile_rows()


def _rand(shape, seed, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, shape).astype(np.uint8)


def _check(q, x, k, self0=-1, want=None):
    """one call against the restatement (or a prefix of one computed before); returns the device results"""
    dist, idx = eg.ops.knn_u8(torch.from_numpy(q).to(DEV), torch.from_numpy(x).to(DEV), k, self0)
    assert dist.dtype == torch.int32 and idx.dtype == torch.int32 and tuple(dist.shape) == tuple(idx.shape) == (len(q), k)
    wd, wi = R.knn(q, x, k, self0) if want is None else want
    assert torch.equal(idx.cpu().long(), torch.from_numpy(wi)), (q.shape, x.shape, k, self0)
    assert torch.equal(dist.cpu().long(), torch.from_numpy(wd)), (q.shape, x.shape, k, self0)
    return dist, idx


# ---- 1. lane map and sign handling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 192])
def test_lane_map_and_sign_handling_on_asymmetric_data(K):
    nq, n, k = 16, 48, 5
    t = np.arange(K)
    q = ((7 * np.arange(nq)[:, None] + 3 * t) % 251).astype(np.uint8)
    x = ((5 * np.arange(n)[:, None] + 11 * t + 1) % 253).astype(np.uint8)
    for row, v in ((3, 0), (7, 255), (11, 127), (13, 128)):
        q[row] = v
    for row, v in ((2, 255), (17, 0), (30, 128), (41, 127), (47, 0)):
        x[row] = v
    _check(q, x, k)


# ---- 2. the int32 edge ------------------------------------------------------------------------------------------------------------------
def test_the_largest_distance_an_int32_holds():
    K = 32768
    q = np.stack([np.zeros(K, np.uint8), np.full(K, 255, np.uint8)])
    x = np.stack([np.full(K, 255, np.uint8), np.zeros(K, np.uint8), np.full(K, 128, np.uint8)])
    dist, idx = _check(q, x, 3)
    assert dist.cpu().tolist() == [[0, 128 * 128 * K, 2130739200], [0, 127 * 127 * K, 2130739200]]
    assert idx.cpu().tolist() == [[1, 2, 0], [0, 2, 1]]


# ---- 3. tile edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("which", range(5))
def test_tile_edges(which, k):
    Tq, Tr = _tiles()
    n = [k, Tr - 1, Tr, Tr + 1, 3 * Tr + 5][which]
    x = _rand((n, 64), 100 + which)
    q = _rand((Tq + 1, 64), 200 + which)
    q[::3] = x[(5 * np.arange(len(q[::3]))) % n]                   # some queries are database rows: distance 0
    want = R.knn(q, x, k)                                          # no exclusion: the result of a prefix of the queries is a prefix
    for nq in (1, 15, 17, Tq - 1, Tq + 1):
        _check(q[:nq], x, k, want=(want[0][:nq], want[1][:nq]))


@pytest.mark.parametrize("k", [1, 16])
def test_wide_workgroups_from_four_query_tiles_on(k):
    """from 4 T_q queries on a workgroup owns two query tiles (another kernel instantiation, another wave layout): the threshold and the
    edges of the doubled tile, over a database of several slices with a ragged last one"""
    Tq, Tr = _tiles()
    W, n = 4 * Tq, 3 * Tr + 5
    x = _rand((n, 64), 110 + k)
    q = _rand((W + 2 * Tq + 1, 64), 210 + k)
    q[::3] = x[(5 * np.arange(len(q[::3]))) % n]
    want = R.knn(q, x, k)
    for nq in (W - 1, W, W + 1, W + 2 * Tq - 1, W + 2 * Tq + 1):
        _check(q[:nq], x, k, want=(want[0][:nq], want[1][:nq]))
    t = np.arange(192)
    qa = ((7 * np.arange(W + 5)[:, None] + 3 * t) % 251).astype(np.uint8)           # the lane-map data of the first test on this layout
    xa = ((5 * np.arange(n)[:, None] + 11 * t + 1) % 253).astype(np.uint8)
    xa[2], xa[17], xa[130], xa[n - 1] = 255, 0, 128, 127
    _check(qa, xa, k)


def test_celeba_row_length_across_tile_edges():
    q, x = _rand((17, 3, 64, 64), 1), _rand((300, 3, 64, 64), 2)
    x[250] = q[4]
    x[7] = x[299] = q[9]
    dist, idx = _check(q, x, 4)
    assert idx[4, 0] == 250 and idx[9, :2].tolist() == [7, 299] and dist[9, :2].tolist() == [0, 0]


# ---- 4. splits --------------------------------------------------------------------------------------------------------------------------
def _first_split_n(nq):
    Tq, Tr = _tiles()
    for n in range(1, 64 * Tr):
        if eg.ops.knn_splits(nq, n) >= 2:
            return n
    raise AssertionError("the split policy does not cut a database of 64 tiles for so few queries")


@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("nq", [5, 70])
def test_database_slices_and_their_merge(nq, k):
    Tq, Tr = _tiles()
    n0 = _first_split_n(nq)
    q = _rand((nq, 64), 7)
    for n in (n0, n0 + 1, n0 + Tr + 3):                            # the last slice is ragged
        assert eg.ops.knn_splits(nq, n) >= 2
        x = _rand((n, 64), 300 + n, 0, 4)                          # few distinct distances: the slices' lists interleave
        x[n - 1] = q[0]                                            # the best row of query 0 is the last of the last slice
        _check(q, x, k)


def test_many_slices():
    Tq, Tr = _tiles()
    n = 40 * Tr + 9
    assert eg.ops.knn_splits(3, n) >= 8
    q, x = _rand((3, 128), 8), _rand((n, 128), 9)
    _check(q, x, 16)


# ---- 5. ties ----------------------------------------------------------------------------------------------------------------------------
def test_massive_ties_go_to_the_lower_index():
    Tq, Tr = _tiles()
    n = 3 * Tr + 5
    q, x = _rand((Tq + 1, 64), 11, 0, 2), _rand((n, 64), 12, 0, 2)          # distances in 0 .. 64
    dist, idx = _check(q, x, 16)
    assert len(set(dist.cpu().reshape(-1).tolist())) < 40


def test_every_row_three_times_at_scattered_indices():
    Tq, Tr = _tiles()
    base = _rand((Tr + 7, 64), 13)
    rng = np.random.RandomState(14)
    x = np.concatenate((base, base, base))[rng.permutation(3 * len(base))]
    q = x[rng.permutation(len(x))[:Tq + 1]]
    dist, idx = _check(q, x, 16)
    assert not dist[:, :3].any() and bool((idx[:, 0] < idx[:, 1]).all() and (idx[:, 1] < idx[:, 2]).all())
    _check(q[:20], x, 16, self0=0)


# ---- 6. exclusion -----------------------------------------------------------------------------------------------------------------------
def test_leave_one_out_excludes_the_row_itself():
    Tq, Tr = _tiles()
    n = 2 * Tr + 9
    x = _rand((n, 64), 15, 0, 3)
    x[n - 1] = x[0]
    dist, idx = _check(x, x, 4, self0=0)
    assert not (idx.cpu() == torch.arange(n)[:, None]).any()
    assert idx[0, 0] == n - 1 and idx[n - 1, 0] == 0 and dist[0, 0] == 0
    nq = Tq + 6
    _check(x[37:37 + nq], x, 4, self0=37)
    _check(x[n - 3:], x, 3, self0=n - 3)                                   # the last three rows: each excludes itself
    q = np.concatenate((x[n - 3:], _rand((5, 64), 16, 0, 3)))              # nq = 8: rows 3 .. 7 have self0 + i >= n and exclude nothing
    _check(q, x, 16, self0=n - 3)
    _check(x[:nq], x, 4, self0=-1)
    d0, i0 = eg.ops.knn_u8(torch.from_numpy(x[:nq]).to(DEV), torch.from_numpy(x).to(DEV), 1)
    assert not d0.any()                                                    # without the exclusion every row finds itself or an equal row
    assert bool((i0[:, 0].cpu() <= torch.arange(nq)).all())


# ---- 7. output hygiene ------------------------------------------------------------------------------------------------------------------
def test_nothing_outside_the_results_is_written_and_two_calls_agree():
    Tq, Tr = _tiles()
    nq, n, k, guard = Tq + 3, 2 * Tr + 1, 7, 64
    q, x = torch.from_numpy(_rand((nq, 64), 17)).to(DEV), torch.from_numpy(_rand((n, 64), 18)).to(DEV)
    bufs = [torch.full((nq * k + 2 * guard,), fill, device=DEV, dtype=torch.int32) for fill in (-7, -9)]
    out = tuple(b[guard:guard + nq * k].view(nq, k) for b in bufs)
    dist, idx = eg.ops.knn_u8(q, x, k, out=out)
    assert dist.data_ptr() == out[0].data_ptr() and idx.data_ptr() == out[1].data_ptr()
    for b, fill in zip(bufs, (-7, -9)):
        assert bool((b[:guard] == fill).all() and (b[guard + nq * k:] == fill).all())
    wd, wi = R.knn(q.cpu().numpy(), x.cpu().numpy(), k)
    assert torch.equal(dist.cpu().long(), torch.from_numpy(wd)) and torch.equal(idx.cpu().long(), torch.from_numpy(wi))
    d2, i2 = eg.ops.knn_u8(q, x, k)
    assert torch.equal(d2, dist) and torch.equal(i2, idx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d3, i3 = eg.ops.knn_u8(q, x, k)
    side.synchronize()
    assert torch.equal(d3, dist) and torch.equal(i3, idx)


def test_shape_and_dtype_errors_of_the_front_end():
    q = torch.zeros(4, 1, 8, 8, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="row length"):
        eg.ops.knn_u8(q[:, :, :, :7].contiguous(), q[:, :, :, :7].contiguous(), 1)
    with pytest.raises(ValueError, match="one length"):
        eg.ops.knn_u8(q, torch.zeros(4, 128, device=DEV, dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="contiguous uint8"):
        eg.ops.knn_u8(q.float(), q, 1)
    with pytest.raises(ValueError, match="contiguous uint8"):
        eg.ops.knn_u8(q[::2], q, 1)
    for k, self0 in ((0, -1), (17, -1), (5, -1), (4, 0)):
        with pytest.raises(ValueError, match="candidates"):
            eg.ops.knn_u8(q, q, k, self0)
    d, i = eg.ops.knn_u8(q, q.reshape(4, 64), 4)                   # trailing dimensions flatten
    assert not d.any() and i.tolist() == [[0, 1, 2, 3]] * 4


# ---- 8. to_u8 ---------------------------------------------------------------------------------------------------------------------------
def test_to_u8_inverts_the_trainers_scaling_for_all_256_values():
    data = torch.arange(256, dtype=torch.uint8).repeat(4).reshape(1, 1, 32, 32).repeat(3, 1, 1, 1)
    data[1] = data[1].flip(-1)
    data[2] = torch.from_numpy(_rand((1, 32, 32), 19))
    data = data.to(DEV)
    real = eg.quality.real_images("mnist", data, 3)
    back = eg.quality.to_u8(real)
    assert back.dtype == torch.uint8 and torch.equal(back, data)
    assert torch.equal(eg.quality.to_u8(data.float() * (2.0 / 255.0) - 1.0), data)          # the unfused form of the same scaling
    wild = torch.tensor([-3.0, -1.0, -1.0 - 2 ** -20, 1.0, 1.0 + 2 ** -20, 7.5, 0.0, -0.0], device=DEV).repeat(8).reshape(1, 1, 8, 8)
    assert torch.equal(eg.quality.to_u8(wild).cpu(), torch.from_numpy(R.to_u8(wild.cpu().numpy())))
    assert eg.quality.to_u8(wild).reshape(-1)[:6].tolist() == [0, 0, 0, 255, 255, 255]
    img = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(3)).mul(2.4).sub(1.2).to(DEV)
    hwc = eg.sampling.to_uint8_hwc(img * 0.5 + 0.5)                                         # save_image's bytes of the image in [0, 1]
    assert torch.equal(eg.quality.to_u8(img)[0].cpu(), torch.from_numpy(hwc).permute(2, 0, 1))
    assert torch.equal(eg.quality.to_u8(img).cpu(), torch.from_numpy(R.to_u8(img.cpu().numpy())))


# ---- 9. nearest_neighbours --------------------------------------------------------------------------------------------------------------
def test_nearest_neighbours_finds_planted_copies():
    data = torch.from_numpy(_rand((200, 1, 32, 32), 20)).to(DEV)
    planted = [150, 3, 199, 0, 77]
    q8 = torch.from_numpy(_rand((8, 1, 32, 32), 21)).to(DEV)
    q8[:5] = data[planted]
    qf = eg.quality.real_images("mnist", q8, 8)                    # the same images as the trainer sees them
    d8, i8 = eg.quality.nearest_neighbours(q8, data, k=3)
    df, i_f = eg.quality.nearest_neighbours(qf, data, k=3)
    assert torch.equal(d8, df) and torch.equal(i8, i_f)
    assert i8[:5, 0].tolist() == planted and not d8[:5, 0].any() and bool((d8[5:, 0] > 0).all())
    wd, wi = R.knn(q8.cpu().numpy(), data.cpu().numpy(), 3)
    assert torch.equal(d8.cpu().long(), torch.from_numpy(wd)) and torch.equal(i8.cpu().long(), torch.from_numpy(wi))

    class Sampler:                                                 # a sampler is anything with the dataset in .data
        pass
    s = Sampler()
    s.data = data
    d, i = eg.quality.nearest_neighbours(q8, s)                    # k = 8 by default
    assert tuple(d.shape) == (8, 8) and torch.equal(i[:, :3], i8)
    with pytest.raises(ValueError, match="against a dataset"):
        eg.quality.nearest_neighbours(q8[:, :, :16], data)


# ---- 10. nn_two_sample ------------------------------------------------------------------------------------------------------------------
def test_two_sample_test_on_separable_identical_and_random_sets():
    Tq, _ = _tiles()
    N = 2 * Tq + 3
    real, fake = _rand((N, 1, 8, 8), 22, 0, 64), _rand((N, 1, 8, 8), 23, 193, 256)
    got = eg.quality.nn_two_sample(torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV))
    assert got == {"accuracy": 1.0, "real": 1.0, "fake": 1.0} and all(type(v) is float for v in got.values())
    distinct = _rand((N, 1, 8, 8), 24)
    distinct[:, 0, 0, 0] = np.arange(N)                            # no two rows are equal
    t = torch.from_numpy(distinct).to(DEV)
    assert eg.quality.nn_two_sample(t, t.clone()) == {"accuracy": 0.0, "real": 0.0, "fake": 0.0}
    a, b = _rand((N, 1, 8, 8), 25, 0, 4), _rand((N, 1, 8, 8), 26, 0, 4)
    r, f, n = R.two_sample_counts(a, b)
    got = eg.quality.nn_two_sample(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert got == {"accuracy": 0.5 * (r / n + f / n), "real": r / n, "fake": f / n} and 0 < r < n and 0 < f < n
    fa = eg.quality.real_images("mnist", torch.from_numpy(a).to(DEV), N)
    assert eg.quality.nn_two_sample(fa, torch.from_numpy(b).to(DEV)) == got                 # float and uint8 sets mix
    with pytest.raises(ValueError, match="one shape"):
        eg.quality.nn_two_sample(t, t[:5])


# ---- 11. the figure ---------------------------------------------------------------------------------------------------------------------
def test_neighbour_grid_and_the_file_it_is_saved_to(tmp_path):
    data = torch.from_numpy(_rand((40, 3, 8, 8), 27)).to(DEV)
    q = torch.from_numpy(_rand((3, 3, 8, 8), 28)).to(DEV)
    dist, idx = eg.quality.nearest_neighbours(q, data, k=4)
    grid = eg.quality.neighbour_grid(q, data, idx)
    want = R.grid(q.cpu().numpy(), data.cpu().numpy(), idx.cpu().numpy())
    assert grid.dtype == torch.float32 and tuple(grid.shape) == (15, 3, 8, 8) and torch.equal(grid.cpu(), torch.from_numpy(want))
    fp, ref = str(tmp_path / "nn" / "grid.png"), str(tmp_path / "ref.png")
    eg.quality.save_neighbours(fp, q, data, idx)
    eg.sampling.save_image(torch.from_numpy(want).to(DEV), ref, nrow=5)
    assert open(fp, "rb").read() == open(ref, "rb").read()
    qf = q.float() * (2.0 / 255.0) - 1.0
    assert torch.equal(eg.quality.neighbour_grid(qf, data, idx), grid)                      # float queries go through to_u8


# ---- 12. a generator --------------------------------------------------------------------------------------------------------------------
def test_nearest_training_images_and_nn_generator_on_a_fresh_mnist_generator(tmp_path):
    torch.manual_seed(1)
    G = eg.mnist.Generator().to(DEV)
    data = torch.randint(0, 256, (64, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    before = {k: v.clone() for k, v in G.state_dict().items()}
    fp = str(tmp_path / "nearest.png")
    d1, i1 = eg.quality.nearest_training_images("mnist", G, data, n_images=16, k=4, batch=8, seed=2, out=fp)
    d2, i2 = eg.quality.nearest_training_images("mnist", G, data, n_images=16, k=4, batch=8, seed=2)
    assert tuple(d1.shape) == (16, 4) and torch.equal(d1, d2) and torch.equal(i1, i2)
    fake = eg.quality.to_u8(eg.quality.generate("mnist", G, 16, 8, seed=2))
    wd, wi = R.knn(fake.cpu().numpy(), data.cpu().numpy(), 4)
    assert torch.equal(d1.cpu().long(), torch.from_numpy(wd)) and torch.equal(i1.cpu().long(), torch.from_numpy(wi))
    assert open(fp, "rb").read()[:8] == b"\x89PNG\r\n\x1a\n"
    a = eg.quality.nn_generator("mnist", G, data, n_images=16, batch=8, seed=2)
    b = eg.quality.nn_generator("mnist", G, data, n_images=16, batch=8, seed=2)
    r, f, n = R.two_sample_counts(data[:16].cpu().numpy(), fake.cpu().numpy())
    assert a == b == {"accuracy": 0.5 * (r / n + f / n), "real": r / n, "fake": f / n}
    after = G.state_dict()
    assert G.training and list(after) == list(before) and all(torch.equal(before[k], after[k]) for k in before)
    for kind in ("dsprites", "colored_train"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.nearest_training_images(kind, G, data)
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.nn_generator(kind, G, data)

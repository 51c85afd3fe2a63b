"""The kernel MMD on the MI355X: ops.dist_select_u8, ops.kernel_sum_u8 and the functions of quality.py built on them against the
numpy restatement tests/mmd_refs.py.  The select returns an integer of a multiset of integers: every comparison of it is ==.  A kernel sum
is a float64 sum of n non-negative terms, each within a few ulp (the argument is the same rounded product on both sides): per row it holds
within the relative (n + 8) 2^-52 of ``mmd_refs.tolerance`` plus an absolute 1e-300 for the denormal tail -- a bound from the arithmetic,
not from what the device returned."""
import functools
import importlib

import numpy as np
import pytest
import torch

import knn_refs as R
import mmd_refs as MR
import prdc_refs as P

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


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def _kept(d, self0):
    return d[MR._kept(*d.shape, self0)]


def _select(q, x, rank, self0=-1):
    got = eg.ops.dist_select_u8(q if isinstance(q, torch.Tensor) else _dev(q), x if isinstance(x, torch.Tensor) else _dev(x), rank, self0)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2,)
    return tuple(got.tolist())


def _median_of(d, self0=-1):
    """(rank, element) of the lower median of the kept pairs of a distance matrix"""
    p = np.sort(_kept(d, self0))
    return (len(p) - 1) // 2, int(p[(len(p) - 1) // 2])


@functools.lru_cache(maxsize=None)
def _grid(K):
    """the lane-map data of the search's tests (tests/test_gpu_knn.py) at the largest size of the grid, and its distances: every case of the
    grid is a corner of this matrix"""
    Tq, Tr = _tiles()
    nq, n = 4 * Tq + 1, 3 * Tr + 5
    t = np.arange(K)
    q = ((7 * np.arange(nq)[:, None] + 3 * t) % 251).astype(np.uint8)
    x = ((5 * np.arange(n)[:, None] + 11 * t + 1) % 253).astype(np.uint8)
    for row, v in ((3, 0), (7, 255), (11, 127), (13, 128)):
        q[row] = v
    for row, v in ((2, 255), (17, 0), (30, 128), (41, 127), (47, 0), (130, 128), (n - 1, 127)):
        x[row] = v
    q[5::9] = x[(5 * np.arange(len(q[5::9]))) % n]                 # some queries are database rows: distance 0, kernel 1
    return q, x, R.distances(q, x)


def _grid_sizes():
    Tq, Tr = _tiles()
    return (1, 17, Tq - 1, Tq + 1, 4 * Tq - 1, 4 * Tq, 4 * Tq + 1), (1, Tr - 1, Tr, Tr + 1, 3 * Tr + 5)


def _first_split_n(nq):
    Tq, Tr = _tiles()
    for n in range(1, 64 * Tr):
        if eg.ops.knn_splits(nq, n) >= 2:
            return n
    raise AssertionError("the split policy does not cut a database of 64 tiles for so few queries")


def _slice_cases():
    """(nq, n): the smallest n that splits and that n + T_r + 3 on both sides of nothing special, and 41 slices"""
    Tq, Tr = _tiles()
    cases = []
    for nq in (5, 70):
        n0 = _first_split_n(nq)
        cases += [(nq, n0), (nq, n0 + Tr + 3)]
    assert eg.ops.knn_splits(3, 40 * Tr + 9) == 41
    return cases + [(3, 40 * Tr + 9)]


# ---- 1. the select ----------------------------------------------------------------------------------------------------------------------
def test_select_crosses_every_digit_boundary():
    rows, ds = MR.digit_boundary_rows()
    assert ds == sorted(ds) and len(ds) == 61 and ds[-1] == 2 ** 30
    order = np.random.RandomState(3).permutation(61)               # the rows are not stored in ascending order
    x = _dev(rows[order])
    q = torch.zeros(1, rows.shape[1], device=DEV, dtype=torch.uint8)
    assert R.distances(np.zeros((1, rows.shape[1]), np.uint8), rows)[0].tolist() == ds
    got = [_select(q, x, rank) for rank in range(61)]
    assert got == [(d, 0) for d in ds]


def test_select_on_heavy_ties():
    q, x = _rand((150, 192), 11, 0, 2), _rand((131, 192), 12, 0, 2)
    p = MR.pairs(q, x)
    assert p[-1] <= 192 and len(p) == 150 * 131
    values, counts = np.unique(p, return_counts=True)
    top = int(values[np.argmax(counts)])
    first, last = int(np.searchsorted(p, top, "left")), int(np.searchsorted(p, top, "right")) - 1
    assert last - first > 1000 and p[first - 1] < top < p[last + 1]
    qd, xd = _dev(q), _dev(x)
    for rank in (0, len(p) - 1, (len(p) - 1) // 2, first, last, first - 1, last + 1):
        assert _select(qd, xd, rank) == (int(p[rank]), 0), rank


@pytest.mark.parametrize("K", [64, 192])
def test_select_on_both_layouts_and_partial_tiles(K):
    q, x, d = _grid(K)
    nqs, ns = _grid_sizes()
    qd, xd = _dev(q), _dev(x)
    for nq in nqs:
        for n in ns:
            rank, want = _median_of(d[:nq, :n])
            assert _select(qd[:nq], xd[:n], rank) == (want, 0), (nq, n)


def test_select_over_database_slices():
    for nq, n in _slice_cases():
        assert eg.ops.knn_splits(nq, n) >= 2
        q, x = _rand((nq, 64), 7 + n, 0, 4), _rand((n, 64), 300 + n, 0, 4)      # few distinct distances: many ties
        p = MR.pairs(q, x)
        qd, xd = _dev(q), _dev(x)
        for rank in (0, (len(p) - 1) // 2, len(p) - 1, len(p) // 3):
            assert _select(qd, xd, rank) == (int(p[rank]), 0), (nq, n, rank)
        wide = _rand((n, 64), 500 + n)                             # and spread distances, where every pass narrows
        pw = MR.pairs(q, wide)
        assert _select(qd, _dev(wide), (len(pw) - 1) // 2) == (int(pw[(len(pw) - 1) // 2]), 0)


def _self0_cases():
    Tq, Tr = _tiles()
    n = 2 * Tr + 9
    x = _rand((n, 64), 15, 0, 3)
    x[n - 1] = x[0]
    tail = np.concatenate((x[n - 3:], _rand((5, 64), 16, 0, 3)))   # rows 3 .. 7 have self0 + i >= n and exclude nothing
    return x, [(x, -1), (x, 0), (x[37:37 + Tq + 6], 37), (tail, n - 3), (x[:9], n + 5)]


def test_select_with_self0_in_its_four_forms():
    x, cases = _self0_cases()
    xd = _dev(x)
    for q, self0 in cases:
        p = MR.pairs(q, x, self0)
        excluded = sum(1 for i in range(len(q)) if 0 <= self0 + i < len(x)) if self0 >= 0 else 0
        assert len(p) == len(q) * len(x) - excluded
        for rank in (0, (len(p) - 1) // 2, len(p) - 1):
            assert _select(_dev(q), xd, rank, self0) == (int(p[rank]), 0), (self0, rank)
        assert _select(_dev(q), xd, len(p), self0) == (int(p[-1]), 1), self0       # one beyond the pairs that are left
    # the zero distances of the diagonal are gone with self0 = 0 (row n - 1 copies row 0: two zeros remain)
    assert int((MR.pairs(x, x) == 0).sum()) - len(x) == int((MR.pairs(x, x, 0) == 0).sum()) >= 2
    assert eg.quality.median_distance(xd.reshape(len(x), 1, 8, 8)).item() == MR.median_distance(x)


def test_select_marks_a_rank_beyond_the_pairs():
    q, x = _rand((5, 64), 1), _rand((9, 64), 2)
    p = MR.pairs(q, x)
    assert _select(q, x, 44) == (int(p[44]), 0)
    for rank in (45, 46, 2 ** 40, 2 ** 64 - 1):
        assert _select(q, x, rank) == (int(p[-1]), 1), rank
    assert _select(q[:1], q[:1], 0, self0=0) == (0, 1)             # no pair at all


def test_select_at_the_largest_distance_an_int32_holds():
    K, top = 32768, 2130739200
    lo, hi = np.zeros(K, np.uint8), np.full(K, 255, np.uint8)
    assert _select(lo[None], hi[None], 0) == (top, 0)
    q, x = np.stack([lo, hi]), np.stack([hi, hi, lo, lo])
    assert MR.pairs(q, x).tolist() == [0] * 4 + [top] * 4
    assert [_select(q, x, r) for r in (0, 3, 4, 7, 8)] == [(0, 0), (0, 0), (top, 0), (top, 0), (top, 1)]


def test_select_gives_the_same_bits_twice_and_on_another_stream():
    q, x, d = _grid(192)
    qd, xd = _dev(q), _dev(x)
    rank, want = _median_of(d)
    a = eg.ops.dist_select_u8(qd, xd, rank)
    b = eg.ops.dist_select_u8(qd, xd, rank)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = eg.ops.dist_select_u8(qd, xd, rank)
    side.synchronize()
    assert a.tolist() == b.tolist() == c.tolist() == [want, 0]


# ---- 2. the kernel sums -----------------------------------------------------------------------------------------------------------------
def _close(got, want, n):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    err, bound = np.abs(got - want), MR.tolerance(n) * np.abs(want) + 1e-300
    assert got.shape == want.shape and np.isfinite(got).all() and (err <= bound).all(), (float((err / bound).max()), n)


def _inv_gammas(d, nb=4):
    """inverse bandwidths around the median distance: gamma_med / 8, gamma_med, 8 gamma_med, and one so small that most terms underflow"""
    med = float(np.sort(d.reshape(-1))[(d.size - 1) // 2]) or 1.0
    return (1.0 / np.array([med / 8.0, med, 8.0 * med, med / 2000.0]))[:nb] if nb > 1 else 1.0 / np.array([med])


def _check_sums(q, x, ig, self0=-1, want=None):
    got = eg.ops.kernel_sum_u8(q if isinstance(q, torch.Tensor) else _dev(q), x if isinstance(x, torch.Tensor) else _dev(x), _dev(ig), self0)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(q), len(ig))
    _close(got, MR.kernel_sums(q, x, ig, self0) if want is None else want, len(x))
    return got


@pytest.mark.parametrize("K", [64, 192])
def test_kernel_sums_on_both_layouts_and_partial_tiles(K):
    q, x, d = _grid(K)
    nqs, ns = _grid_sizes()
    qd, xd = _dev(q), _dev(x)
    ig4, ig1 = _inv_gammas(d), _inv_gammas(d, 1)
    with np.errstate(under="ignore"):
        terms = np.exp(-(d.astype(np.float64)[:, :, None] * ig4))                        # [nq, n, 4]: every case sums a corner of it
    assert (terms[:, :, 3] == 0).mean() > 0.5 and (terms[:, :, 3] > 0).any() and (terms[:, :, :3] > 0).all()
    for nq in nqs:
        for n in ns:
            got = eg.ops.kernel_sum_u8(qd[:nq], xd[:n], _dev(ig4))
            _close(got, terms[:nq, :n].sum(1), n)
            if n == ns[-1] or nq == nqs[0]:
                one = eg.ops.kernel_sum_u8(qd[:nq], xd[:n], _dev(ig1))
                assert tuple(one.shape) == (nq, 1)
                _close(one, terms[:nq, :n, 1:2].sum(1), n)


def test_kernel_sums_over_database_slices():
    for nq, n in _slice_cases():
        q, x = _rand((nq, 64), 7 + n), _rand((n, 64), 300 + n)
        q[1] = x[n - 1]                                            # the last row of the last slice counts 1
        d = R.distances(q, x)
        got = _check_sums(q, x, _inv_gammas(d))
        assert float(got[1, 3]) >= 1.0
        _check_sums(q, x, _inv_gammas(d, 1))


def test_kernel_sums_at_the_celeba_row_length():
    q, x = _rand((17, 3, 64, 64), 1, 100, 156), _rand((300, 3, 64, 64), 2, 100, 156)
    x[250] = q[4]
    d = R.distances(q, x)
    got = _check_sums(q, x, _inv_gammas(d))
    assert float(got[4, 3]) >= 1.0


def test_kernel_sums_with_self0_in_its_four_forms():
    x, cases = _self0_cases()
    ig = _inv_gammas(R.distances(x, x)[~np.eye(len(x), dtype=bool)][None])
    for q, self0 in cases:
        _check_sums(q, x, ig, self0)
    loo, full = _check_sums(x, x, ig, 0), _check_sums(x, x, ig)
    _close(full - loo, np.ones((len(x), 4)), len(x))               # the diagonal term is exp(0) = 1


def test_a_bad_inverse_bandwidth_sets_exactly_its_flag_bit():
    q, x, d = _grid(64)
    q, x, d = q[:70], x[:200], d[:70, :200]
    good = _inv_gammas(d)[[0, 1, 2, 1]]
    qd, xd = _dev(q), _dev(x)
    want = MR.kernel_sums(q, x, good)
    flag = torch.full((1,), -7, device=DEV, dtype=torch.int32)
    _close(eg.ops.kernel_sum_u8(qd, xd, _dev(good), flag=flag), want, 200)
    assert flag.item() == 0                                        # written, whatever it held
    for b, bad in enumerate((0.0, -1.0, float("inf"), float("nan"))):
        ig = good.copy()
        ig[b] = bad
        flag.fill_(-7)
        got = eg.ops.kernel_sum_u8(qd, xd, _dev(ig), flag=flag)
        assert flag.item() == 1 << b, (b, bad)
        keep = [c for c in range(4) if c != b]
        _close(got[:, keep], want[:, keep], 200)
    flag.fill_(0)
    eg.ops.kernel_sum_u8(qd, xd, _dev(np.array([0.0, good[1], float("nan")])), flag=flag)
    assert flag.item() == 0b101


def test_kernel_sums_write_only_their_result_and_give_the_same_bits_again():
    Tq, Tr = _tiles()
    q, x, d = _grid(192)
    nq, n, guard = Tq + 3, 2 * Tr + 1, 64
    qd, xd, ig = _dev(q[:nq]), _dev(x[:n]), _dev(_inv_gammas(d))
    buf = torch.full((nq + 2 * guard, 4), -7.0, device=DEV, dtype=torch.float64)
    out = buf[guard:guard + nq]
    got = eg.ops.kernel_sum_u8(qd, xd, ig, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == -7).all() and (buf[guard + nq:] == -7).all())
    _close(got, MR.kernel_sums(q[:nq], x[:n], ig.cpu().numpy()), n)
    again = eg.ops.kernel_sum_u8(qd, xd, ig)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = eg.ops.kernel_sum_u8(qd, xd, ig)
    side.synchronize()
    assert torch.equal(third.view(torch.int64), got.view(torch.int64))
    many_q, many_x = _dev(_rand((3, 64), 8)), _dev(_rand((40 * Tr + 9, 64), 9))          # 41 slices: the second kernel's tree
    a, b = eg.ops.kernel_sum_u8(many_q, many_x, ig), eg.ops.kernel_sum_u8(many_q, many_x, ig)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_shape_and_dtype_errors_of_the_front_ends():
    q = torch.zeros(4, 1, 8, 8, device=DEV, dtype=torch.uint8)
    ig = torch.ones(2, device=DEV, dtype=torch.float64)
    for call in (lambda a, b: eg.ops.kernel_sum_u8(a, b, ig), lambda a, b: eg.ops.dist_select_u8(a, b, 0)):
        with pytest.raises(ValueError, match="row length"):
            call(q[:, :, :, :7].contiguous(), q[:, :, :, :7].contiguous())
        with pytest.raises(ValueError, match="one length"):
            call(q, torch.zeros(4, 128, device=DEV, dtype=torch.uint8))
        with pytest.raises(ValueError, match="contiguous uint8"):
            call(q.float(), q)
        with pytest.raises(ValueError, match="contiguous uint8"):
            call(q[::2], q)
    for bad in (ig.float(), torch.ones(5, device=DEV, dtype=torch.float64), torch.ones(0, device=DEV, dtype=torch.float64), ig.cpu(),
                ig.reshape(2, 1), torch.ones(4, device=DEV, dtype=torch.float64)[::2]):
        with pytest.raises(ValueError, match="inv_gamma must be"):
            eg.ops.kernel_sum_u8(q, q, bad)
    for bad in (torch.zeros(4, 3, device=DEV, dtype=torch.float64), torch.zeros(4, 2, device=DEV, dtype=torch.float32)):
        with pytest.raises(ValueError, match="out must be"):
            eg.ops.kernel_sum_u8(q, q, ig, out=bad)
    with pytest.raises(ValueError, match="flag must be"):
        eg.ops.kernel_sum_u8(q, q, ig, flag=torch.zeros(1, device=DEV, dtype=torch.int64))
    with pytest.raises(ValueError, match="rank"):
        eg.ops.dist_select_u8(q, q, -1)
    assert eg.ops.kernel_sum_u8(q, q.reshape(4, 64), ig).tolist() == [[4.0, 4.0]] * 4     # trailing dimensions flatten; d = 0: every term is 1
    assert eg.ops.kernel_sum_u8(q, q, ig, self0=0).tolist() == [[3.0, 3.0]] * 4
    assert eg.ops.dist_select_u8(q, q, 5).tolist() == [0, 0]


# ---- 3. quality.mmd ---------------------------------------------------------------------------------------------------------------------
def _imgs(rows):
    return _dev(rows).reshape(len(rows), 1, 8, 8)


def _check_mmd(got, want, N, M):
    tol = 8 * MR.tolerance(max(N, M))
    assert sorted(got) == ["bandwidths", "gamma_median", "mean", "mmd2", "mmd2_biased"]
    assert got["gamma_median"] == want["gamma_median"] and got["bandwidths"] == want["bandwidths"]
    assert type(got["mean"]) is float and all(type(v) is float for v in got["mmd2"] + got["mmd2_biased"] + got["bandwidths"])
    for name in ("mmd2", "mmd2_biased"):
        assert len(got[name]) == len(want[name]) and all(abs(g - w) <= tol for g, w in zip(got[name], want[name])), (name, got[name], want[name])
    assert got["mean"] == sum(got["mmd2"]) / len(got["mmd2"])


def test_mmd_on_clustered_sets():
    a, b = P.clustered()
    want = MR.mmd(a, b)
    got = eg.quality.mmd(_imgs(a), _imgs(b))
    print(got)
    assert type(got["gamma_median"]) is int and got["gamma_median"] == MR.median_distance(np.concatenate((a, b)))
    _check_mmd(got, want, 150, 131)
    # the three sums behind it, with the very inverse bandwidths of the restatement
    ig = 1.0 / np.asarray(want["bandwidths"])
    sums, flags = eg.quality.mmd_sums(_imgs(a), _imgs(b), _dev(ig))
    assert flags.tolist() == [0, 0, 0] and tuple(sums.shape) == (3, 3)
    for got_s, want_s, n in zip(sums.cpu().numpy(), MR.sums(a, b, ig), (150, 131, 131)):
        _close(got_s, want_s, n)
    # a generator that misses one cluster and adds a foreign one is farther from the data than the data are from themselves
    halves = eg.quality.mmd(_imgs(a[0::2]), _imgs(a[1::2]))
    _check_mmd(halves, MR.mmd(a[0::2], a[1::2]), 75, 75)
    assert all(g > 5 * abs(h) for g, h in zip(got["mmd2"], halves["mmd2"])) and got["mean"] > 5 * abs(halves["mean"])
    _check_mmd(eg.quality.mmd(_imgs(b), _imgs(a)), MR.mmd(b, a), 131, 150)               # N != M both ways
    fa = eg.quality.real_images("mnist", _imgs(a), 150)                                    # float input goes through to_u8
    assert eg.quality.mmd(fa, _imgs(b)) == got
    one = eg.quality.mmd(_imgs(a), _imgs(b), scales=(1.0,))
    assert one["bandwidths"] == [float(got["gamma_median"])] and abs(one["mmd2"][0] - got["mmd2"][1]) <= 8 * MR.tolerance(150)
    fixed = eg.quality.mmd(_imgs(a), _imgs(b), bandwidths=[3000.0, 70000.0])             # no select
    assert fixed["gamma_median"] is None
    _check_mmd(fixed, MR.mmd(a, b, bandwidths=[3000.0, 70000.0]), 150, 131)


def test_mmd_refuses_what_it_cannot_score():
    a, _ = P.clustered()
    dup = np.concatenate((np.repeat(a[7:8], 40, 0), a[:6]))        # 40 of 46 rows are one row: the median distance is 0
    assert MR.median_distance(np.concatenate((dup, dup))) == 0
    with pytest.raises(ValueError, match="median distance .* is zero"):
        eg.quality.mmd(_imgs(dup), _imgs(dup))
    assert eg.quality.mmd(_imgs(dup), _imgs(dup), bandwidths=[1000.0])["gamma_median"] is None
    u = torch.zeros(6, 1, 8, 8, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one shape"):
        eg.quality.mmd(u, torch.zeros(6, 1, 16, 16, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least 2"):
        eg.quality.mmd(u, u[:1])
    for bad in ((), (1, 2, 3, 4, 5), (0.0,), (-1.0,), (float("inf"),), (float("nan"),)):
        with pytest.raises(ValueError, match="scales must be"):
            eg.quality.mmd(u, u, scales=bad)
        with pytest.raises(ValueError, match="bandwidths must be"):
            eg.quality.mmd(u, u, bandwidths=bad)


def test_witness_says_which_images_are_over_and_under_represented():
    a, b = P.clustered()
    gamma = float(MR.median_distance(np.concatenate((a, b))))
    z = np.concatenate((a, b))
    got = eg.quality.mmd_witness(_imgs(a), _imgs(b), _imgs(z), gamma)
    assert got.dtype == torch.float64 and tuple(got.shape) == (281,) and got.is_cuda
    want = MR.witness(a, b, z, gamma)
    assert np.abs(got.cpu().numpy() - want).max() <= 4 * MR.tolerance(150)                # two normalised sums <= 1 each, and their division
    w = got.cpu().numpy()
    assert (w[100:150] > 0).all()                                  # the real cluster that is never generated: data denser than samples
    assert (w[150 + 100:] < 0).all()                               # the generated rows around the foreign centre: over-produced
    assert abs(w[:100].mean()) < 0.2 * w[100:150].mean()           # the two shared clusters sit near zero


# ---- 4. a generator ---------------------------------------------------------------------------------------------------------------------
def test_mmd_generator_on_a_fresh_mnist_generator():
    torch.manual_seed(1)
    G = eg.mnist.Generator().to(DEV)
    data = torch.randint(112, 144, (20, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    before = {k: v.clone() for k, v in G.state_dict().items()}
    a = eg.quality.mmd_generator("mnist", G, data, n_images=16, batch=8, seed=2)
    b = eg.quality.mmd_generator("mnist", G, data, n_images=16, batch=8, seed=2)
    fake = eg.quality.to_u8(eg.quality.generate("mnist", G, 16, 8, seed=2))
    assert a == b
    _check_mmd(a, MR.mmd(data[:16].cpu().numpy(), fake.cpu().numpy()), 16, 16)
    after = G.state_dict()
    assert G.training and list(after) == list(before) and all(torch.equal(before[k], after[k]) for k in before)
    assert eg.quality.mmd_generator("mnist", G.eval(), data, n_images=16, batch=8, seed=2) != a      # the generator's current mode runs
    G.train()
    for kind in ("dsprites", "colored_train"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.mmd_generator(kind, G, data)

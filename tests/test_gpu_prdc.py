"""Precision, recall, density and coverage on the MI355X: ops.ball_count_u8 and the functions of quality.py built on it against
the int64 restatement tests/prdc_refs.py.  Counts are integers and the scores exact ratios of two, so every comparison is torch.equal / ==:
there is no tolerance anywhere in this file.  The balls are closed, and several cases sit on d == rad, where an open ball gives another
count."""
import importlib

import numpy as np
import pytest
import torch

import knn_refs as R
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


def _mid_radii(d, seed):
    """one radius per database row, uniform between the 5th and 95th percentile of the distances: counts are neither 0 nor n"""
    lo, hi = np.percentile(d, 5), np.percentile(d, 95)
    return np.random.RandomState(seed).randint(int(lo), int(hi) + 1, d.shape[1]).astype(np.int64)


def _check(q, x, rad, self0=-1, want=None):
    """one call against the restatement (or a prefix of one computed before); returns the device result"""
    got = eg.ops.ball_count_u8(_dev(q), _dev(x), _dev(rad, np.int32), self0)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(q),)
    want = P.ball_count(q, x, rad, self0) if want is None else want
    assert torch.equal(got.cpu().long(), torch.from_numpy(want)), (q.shape, x.shape, self0)
    return got


# ---- 1. lane map and sign handling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 192])
def test_lane_map_and_sign_handling_on_asymmetric_data(K):
    nq, n = 16, 48
    t = np.arange(K)
    q = ((7 * np.arange(nq)[:, None] + 3 * t) % 251).astype(np.uint8)
    x = ((5 * np.arange(n)[:, None] + 11 * t + 1) % 253).astype(np.uint8)
    for row, v in ((3, 0), (7, 255), (11, 127), (13, 128)):
        q[row] = v
    for row, v in ((2, 255), (17, 0), (30, 128), (41, 127), (47, 0)):
        x[row] = v
    d = R.distances(q, x)
    got = _check(q, x, _mid_radii(d, K))
    assert 0 < int(got.min()) and int(got.max()) < n and len(set(got.tolist())) > 4          # every query has a count of its own to get wrong
    _check(q, x, P.radii(x, 5))


# ---- 2. the <= edge ---------------------------------------------------------------------------------------------------------------------
def test_a_row_at_exactly_the_radius_is_inside():
    Tq, Tr = _tiles()
    n, i0 = 3 * Tr + 5, 9
    q, x = _rand((Tq + 1, 64), 31), _rand((n, 64), 32)
    x[5] = x[2 * Tr + 1] = q[2]                                    # two copies of query 2 in different tiles
    d = R.distances(q, x)
    rad = d[i0] + (np.arange(n) % 3 - 1)                           # d - 1, d, d + 1 of query i0: out, in (the edge), in
    rad[5] = rad[2 * Tr + 1] = 0                                   # a ball of radius 0 holds the copies of its centre
    rad[7::11] = -1                                                # empty balls
    got = _check(q, x, rad)
    mask = np.ones(n, bool)
    mask[[5, 2 * Tr + 1]] = False
    mask[7::11] = False
    assert int(got[i0]) == int(((np.arange(n) % 3 != 0) & mask).sum())
    assert int(got[i0]) != int((d[i0] < rad).sum())                # an open ball counts a third fewer
    assert (d[2, [5, 2 * Tr + 1]] == 0).all() and int(got[2]) == int((d[2] <= rad).sum()) >= 2
    assert not _check(q, x, np.full(n, -1)).any()
    assert _check(q[2:3], x, np.zeros(n, np.int64)).tolist() == [2]


def test_tie_rich_data_where_an_open_ball_cannot_pass():
    q, x = _rand((150, 64), 11, 0, 2), _rand((131, 64), 12, 0, 2)
    rad = P.radii(x, 5)
    d = R.distances(q, x)
    assert (int((d == rad[None, :]).sum()), int((d < rad[None, :]).sum())) == (403, 555)    # of the restatement, on the CPU
    got = _check(q, x, rad)
    assert not torch.equal(got.cpu().long(), torch.from_numpy((d < rad[None, :]).sum(1)))
    assert torch.equal(eg.quality.knn_radii(_dev(x).reshape(131, 1, 8, 8), 5).cpu().long(), torch.from_numpy(rad))


# ---- 3. the int32 edge ------------------------------------------------------------------------------------------------------------------
def test_the_largest_distance_an_int32_holds():
    K, top = 32768, 2130739200
    lo, hi = np.zeros(K, np.uint8), np.full(K, 255, np.uint8)
    q, x = np.stack([lo, hi]), np.stack([hi, hi, lo, lo])
    assert R.distances(q[:1], x[:1])[0, 0] == top == 255 * 255 * K
    got = _check(q, x, np.array([top, top - 1, top - 1, -1]))
    assert got.tolist() == [2, 2]                                  # query 0: rows 0 (d = top <= top) and 2; query 1: rows 0 and 1
    assert _check(q, x, np.array([top, top, top, top])).tolist() == [4, 4]
    assert _check(q, x, np.array([top - 1] * 4)).tolist() == [2, 2]
    assert _check(q, x, np.array([2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31])).tolist() == [2, 2]


# ---- 4. tile edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(5))
def test_tile_edges(which):
    """every query count around one and four query tiles (from 4 T_q queries on a workgroup owns two tiles: the other instantiation)
    against every row count around one and three row tiles"""
    Tq, Tr = _tiles()
    n = [1, Tr - 1, Tr, Tr + 1, 3 * Tr + 5][which]
    x = _rand((n, 64), 100 + which)
    q = _rand((4 * Tq + 1, 64), 200 + which)
    q[::3] = x[(5 * np.arange(len(q[::3]))) % n]                   # some queries are database rows: distance 0
    d = R.distances(q, x)
    rad = _mid_radii(d, 300 + which)
    want = P.ball_count(q, x, rad)                                 # no exclusion: the result of a prefix of the queries is a prefix
    if n > 1:
        assert 0 < want.min() or n < Tr
        assert want.max() < n and len(set(want.tolist())) > min(n, 8) // 2
    for nq in (1, 17, Tq - 1, Tq + 1, 4 * Tq - 1, 4 * Tq, 4 * Tq + 1):
        _check(q[:nq], x, rad, want=want[:nq])


# ---- 5. slices --------------------------------------------------------------------------------------------------------------------------
def _first_split_n(nq):
    Tq, Tr = _tiles()
    for n in range(1, 64 * Tr):
        if eg.ops.knn_splits(nq, n) >= 2:
            return n
    raise AssertionError("the split policy does not cut a database of 64 tiles for so few queries")


@pytest.mark.parametrize("nq", [5, 70])
def test_database_slices_and_their_sum(nq):
    Tq, Tr = _tiles()
    n0 = _first_split_n(nq)
    q = _rand((nq, 64), 7, 0, 4)
    for n in (n0, n0 + Tr + 3):                                    # the last slice is ragged
        assert eg.ops.knn_splits(nq, n) >= 2
        x = _rand((n, 64), 300 + n, 0, 4)                          # few distinct distances: many rows sit on the edge
        rad = _mid_radii(R.distances(q, x), n)
        rad[n - 1] = 2 ** 31 - 1                                   # the last row of the last slice counts for everybody
        _check(q, x, rad)


def test_many_slices():
    Tq, Tr = _tiles()
    n = 40 * Tr + 9
    assert eg.ops.knn_splits(3, n) == 41 and eg.ops.ball_count_ws_bytes(3, n) == 41 * 3 * 4
    q, x = _rand((3, 128), 8), _rand((n, 128), 9)
    _check(q, x, _mid_radii(R.distances(q, x), 10))


def test_celeba_row_length_across_tile_edges():
    q, x = _rand((17, 3, 64, 64), 1), _rand((300, 3, 64, 64), 2)
    x[250] = q[4]
    d = R.distances(q, x)
    rad = _mid_radii(d, 3)
    rad[250] = 0
    got = _check(q, x, rad)
    assert int(got[4]) == int((d[4] <= rad).sum()) >= 1


# ---- 6. exclusion -----------------------------------------------------------------------------------------------------------------------
def test_self0_in_its_four_forms():
    Tq, Tr = _tiles()
    n = 2 * Tr + 9
    x = _rand((n, 64), 15, 0, 3)
    x[n - 1] = x[0]
    rad = P.radii(x, 4)
    got = _check(x, x, rad, self0=0)                               # every row, leave-one-out
    plain = _check(x, x, rad)
    assert torch.equal(plain, got + 1)                             # without the exclusion every row also lies in its own ball
    nq = Tq + 6
    _check(x[37:37 + nq], x, rad, self0=37)                        # a window of the rows
    _check(x[n - 3:], x, rad, self0=n - 3)                         # the last three rows: each excludes itself
    q = np.concatenate((x[n - 3:], _rand((5, 64), 16, 0, 3)))      # nq = 8: rows 3 .. 7 have self0 + i >= n and exclude nothing
    _check(q, x, rad, self0=n - 3)
    _check(x[:nq], x, rad, self0=-1)


# ---- 7. output hygiene ------------------------------------------------------------------------------------------------------------------
def test_nothing_outside_the_result_is_written_and_two_calls_agree():
    Tq, Tr = _tiles()
    nq, n, guard = Tq + 3, 2 * Tr + 1, 64
    qn, xn = _rand((nq, 64), 17), _rand((n, 64), 18)
    radn = _mid_radii(R.distances(qn, xn), 19)
    q, x, rad = _dev(qn), _dev(xn), _dev(radn, np.int32)
    buf = torch.full((nq + 2 * guard,), -7, device=DEV, dtype=torch.int32)
    out = buf[guard:guard + nq]
    got = eg.ops.ball_count_u8(q, x, rad, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == -7).all() and (buf[guard + nq:] == -7).all())
    assert torch.equal(got.cpu().long(), torch.from_numpy(P.ball_count(qn, xn, radn)))
    again = eg.ops.ball_count_u8(q, x, rad)
    assert torch.equal(again, got)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = eg.ops.ball_count_u8(q, x, rad)
    side.synchronize()
    assert torch.equal(third, got)


def test_shape_and_dtype_errors_of_the_front_end():
    q = torch.zeros(4, 1, 8, 8, device=DEV, dtype=torch.uint8)
    rad = torch.zeros(4, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match="row length"):
        eg.ops.ball_count_u8(q[:, :, :, :7].contiguous(), q[:, :, :, :7].contiguous(), rad)
    with pytest.raises(ValueError, match="one length"):
        eg.ops.ball_count_u8(q, torch.zeros(4, 128, device=DEV, dtype=torch.uint8), rad)
    with pytest.raises(ValueError, match="contiguous uint8"):
        eg.ops.ball_count_u8(q.float(), q, rad)
    with pytest.raises(ValueError, match="contiguous uint8"):
        eg.ops.ball_count_u8(q[::2], q, rad)
    for bad in (rad.long(), rad[:3], torch.zeros(8, device=DEV, dtype=torch.int32)[::2], rad.cpu(), rad.reshape(4, 1)):
        with pytest.raises(ValueError, match="radii must be"):
            eg.ops.ball_count_u8(q, q, bad)
    for bad in (torch.zeros(3, device=DEV, dtype=torch.int32), torch.zeros(4, device=DEV, dtype=torch.int64)):
        with pytest.raises(ValueError, match="out must be"):
            eg.ops.ball_count_u8(q, q, rad, out=bad)
    assert eg.ops.ball_count_u8(q, q.reshape(4, 64), rad).tolist() == [4] * 4             # trailing dimensions flatten
    assert eg.ops.ball_count_u8(q, q, rad, self0=0).tolist() == [3] * 4


# ---- 8. quality.prdc --------------------------------------------------------------------------------------------------------------------
def _imgs(rows):
    return _dev(rows).reshape(len(rows), 1, 8, 8)


def _ratios(want):
    return {name: num / den for name, (num, den) in want.items()}


def test_prdc_on_clustered_sets():
    a, b = P.clustered()
    want = P.prdc(a, b, 5)
    # the restatement's own figures on the CPU: two of three real clusters are generated, a fifth of the generated rows are foreign
    assert want == {"precision": (91, 131), "recall": (93, 150), "density": (484, 655), "coverage": (97, 150)}
    got = eg.quality.prdc(_imgs(a), _imgs(b), 5)
    assert got == _ratios(want) and all(type(v) is float and 0 < v < 1 for v in got.values())
    assert eg.quality.prdc(_imgs(a), _imgs(b)) == got                                      # k = 5 by default
    got3 = eg.quality.prdc(_imgs(a), _imgs(b), 3)
    assert got3 == _ratios(P.prdc(a, b, 3)) and all(got3[name] != got[name] for name in got)
    assert eg.quality.prdc(_imgs(b), _imgs(a), 5) == _ratios(P.prdc(b, a, 5))              # N != M both ways
    fa = eg.quality.real_images("mnist", _imgs(a), 150)                                    # float input goes through to_u8
    assert eg.quality.prdc(fa, _imgs(b), 5) == got
    assert torch.equal(eg.quality.knn_radii(fa, 5), eg.quality.knn_radii(_imgs(a), 5))
    assert torch.equal(eg.quality.knn_radii(_imgs(a), 5).cpu().long(), torch.from_numpy(P.radii(a, 5)))


def test_prdc_on_identical_collapsed_and_far_apart_sets():
    a, b = P.clustered()
    got = eg.quality.prdc(_imgs(a), _imgs(a).clone(), 5)
    assert got == _ratios(P.prdc(a, a, 5)) and got["precision"] == got["recall"] == got["coverage"] == 1.0
    one = np.repeat(a[7:8], 131, 0)                                # mode collapse: 131 copies of one real row
    got = eg.quality.prdc(_imgs(a), _imgs(one), 5)
    assert got == _ratios(P.prdc(a, one, 5)) and got["precision"] == 1.0 and got["recall"] == 1 / 150
    lo, hi = (a // 4).astype(np.uint8), (192 + b // 4).astype(np.uint8)
    assert eg.quality.prdc(_imgs(lo), _imgs(hi), 5) == {"precision": 0.0, "recall": 0.0, "density": 0.0, "coverage": 0.0}
    small = _rand((17, 64), 40, 0, 3)                              # N = 17, M = 300, tie-rich, at the largest k
    big = _rand((300, 64), 41, 0, 3)
    assert eg.quality.prdc(_imgs(small), _imgs(big), 16) == _ratios(P.prdc(small, big, 16))


def test_prdc_refuses_what_it_cannot_score():
    a = torch.zeros(6, 1, 8, 8, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one shape"):
        eg.quality.prdc(a, torch.zeros(6, 1, 16, 16, device=DEV, dtype=torch.uint8))
    for k in (0, 6, 17):
        with pytest.raises(ValueError, match="k = "):
            eg.quality.prdc(a, a, k)
    with pytest.raises(ValueError, match="k = "):
        eg.quality.prdc(torch.zeros(40, 1, 8, 8, device=DEV, dtype=torch.uint8), a, 6)     # the smaller set bounds k
    with pytest.raises(ValueError, match="k = "):
        eg.quality.knn_radii(a, 6)
    assert eg.quality.prdc(a, a, 5) == {"precision": 1.0, "recall": 1.0, "density": 6 / 5, "coverage": 1.0}


# ---- 9. a generator ---------------------------------------------------------------------------------------------------------------------
def test_prdc_generator_on_a_fresh_mnist_generator():
    torch.manual_seed(1)
    G = eg.mnist.Generator().to(DEV)
    # 20 random images with the spread of a fresh generator's own train-mode output (bytes of standard deviation 9 around the middle
    # grey; in eval mode it draws a flatter image, of 3): real and generated rows are then neighbours and the scores see the generator.
    # Against uniform bytes every generated image lies inside every real ball in both modes and the four numbers say nothing.
    data = torch.randint(112, 144, (20, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    before = {k: v.clone() for k, v in G.state_dict().items()}
    a = eg.quality.prdc_generator("mnist", G, data, n_images=16, batch=8, seed=2)
    b = eg.quality.prdc_generator("mnist", G, data, n_images=16, batch=8, seed=2)
    fake = eg.quality.to_u8(eg.quality.generate("mnist", G, 16, 8, seed=2))
    assert a == b == _ratios(P.prdc(data[:16].cpu().numpy(), fake.cpu().numpy(), 5))
    after = G.state_dict()
    assert G.training and list(after) == list(before) and all(torch.equal(before[k], after[k]) for k in before)
    assert eg.quality.prdc_generator("mnist", G.eval(), data, n_images=16, batch=8, seed=2) != a      # the generator's current mode runs
    assert all(torch.equal(before[k], v) for k, v in G.state_dict().items())
    G.train()
    for kind in ("dsprites", "colored_train"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.prdc_generator(kind, G, data)

"""k-means over uint8 rows and the NDB score on the MI355X: ops.group_rows, ops.kmeans_update_u8, ops.kmeans_seed_u8,
ops.kmeans_u8 and quality.ndb against the numpy int64 restatement (tests/kmeans_refs.py) at the edges of their launches.  Every equality
is exact: integers throughout, and the score's floats are computed on the host from the exact counts by the same operations."""
import importlib

import numpy as np
import pytest
import torch

import kmeans_refs as KR

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None
BELOW_ONE = float(np.float32(1.0 - 2.0 ** -24))                   # the largest fp32 below 1


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _flag():
    return torch.full((1,), -7, device=DEV, dtype=torch.int32)


def _check_group(labels, bins, ws=None):
    flag = _flag()
    counts, offsets, order = eg.ops.group_rows(_t(labels, torch.int32), bins, ws=ws, flag=flag)
    wc, wo, wr, wf = KR.group(labels, bins)
    assert torch.equal(counts, _t(wc, torch.int32)) and torch.equal(offsets, _t(wo, torch.int32)) and torch.equal(order, _t(wr, torch.int32))
    assert int(flag) == wf
    o, off = order.cpu().numpy(), offsets.cpu().numpy()
    for c in range(bins):                                          # stability: ascending inside each cell
        cell = o[off[c]:off[c + 1]]
        assert (np.diff(cell) > 0).all() and (np.asarray(labels)[cell] == c).all()
    return counts, offsets, order


# ---- group_rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 2, 129, 1024])
@pytest.mark.parametrize("edge", [-1, 0, 1])
def test_group_rows_at_the_block_edge(edge, bins):
    n = eg.ops.group_rows_block() + edge
    _check_group(np.random.RandomState(bins + edge).randint(0, bins, n), bins)


def test_group_rows_over_several_blocks_with_empty_full_and_bad_cells():
    B = eg.ops.group_rows_block()
    n = 3 * B + 5
    rng = np.random.RandomState(4)
    labels = rng.randint(0, 129, n)
    labels[labels == 77] = 78                                      # a cell with no rows
    counts, _, _ = _check_group(labels, 129)
    assert int(counts[77]) == 0 and int(counts.sum()) == n
    counts, offsets, order = _check_group(np.full(n, 3), 5)        # all rows in one cell
    assert counts.tolist() == [0, 0, 0, n, 0] and torch.equal(order, torch.arange(n, device=DEV, dtype=torch.int32))
    bad = rng.randint(0, 10, n)
    bad[[0, B - 1, B, n - 1]] = [10, -1, 2 ** 31 - 1, -2 ** 31]    # outside [0, 10): flagged and left out
    counts, offsets, order = _check_group(bad, 10)
    assert int(offsets[10]) == n - 4 and order[n - 4:].tolist() == [-1] * 4 and int(counts.sum()) == n - 4
    # the workspace's earlier contents do not matter; two calls give the same bits
    ws = torch.full((eg.ops.group_rows_ws_bytes(n, 129) // 8 + 2,), -1, device=DEV, dtype=torch.int64)
    a = _check_group(labels, 129, ws=ws)
    b = _check_group(labels, 129, ws=ws)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_group_rows_argument_checks():
    lab = torch.zeros(8, device=DEV, dtype=torch.int32)
    for bins in (0, 1025):
        with pytest.raises(ValueError, match="bins"):
            eg.ops.group_rows(lab, bins)
    with pytest.raises(ValueError, match="int32"):
        eg.ops.group_rows(lab.long(), 4)
    with pytest.raises(ValueError, match="no CPU path"):
        eg.ops.group_rows(lab.cpu(), 4)


# ---- the centre update ------------------------------------------------------------------------------------------------------------------
def _update_case(K, seed):
    """cells of exactly one segment, one segment plus one row, three segments (the last partial), all-0 rows, all-255 rows, one row and none"""
    S = eg.ops.kmeans_segment_rows()
    sizes = [S, S + 1, 2 * S + 7, 40, 40, 1, 0]
    rng = np.random.RandomState(seed)
    labels = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    rows = rng.randint(0, 256, (len(labels), K)).astype(np.uint8)
    rows[labels == 3] = 0                                          # the sums at their extremes
    rows[labels == 4] = 255
    centres = rng.randint(0, 256, (len(sizes), K)).astype(np.uint8)
    return rows, labels, centres


@pytest.mark.parametrize("K", [64, 192, 1088])                    # 1088: one column chunk and 64 bytes of the next
def test_update_at_the_segment_edges(K):
    assert eg.ops.kmeans_column_chunk() == 1024 and eg.ops.kmeans_segment_rows() == 256, "the cases below sit on these edges"
    rows, labels, centres = _update_case(K, K)
    want = KR.update(rows, labels, centres)
    assert np.array_equal(want[6], centres[6]) and want[3].max() == 0 and want[4].min() == 255 and np.array_equal(want[5], rows[labels == 5][0])
    counts, offsets, order = eg.ops.group_rows(_t(labels, torch.int32), len(centres))
    d_rows = _t(rows)
    got = eg.ops.kmeans_update_u8(d_rows, order, offsets, counts, _t(centres))
    assert torch.equal(got, _t(want))
    # a workspace full of 0xFF gives the same result, and so does a second call
    n = len(rows)
    ws = torch.full((eg.ops.kmeans_update_ws_bytes(n, K, len(centres)) // 8 + 2,), -1, device=DEV, dtype=torch.int64)
    for _ in range(2):
        again = eg.ops.kmeans_update_u8(d_rows, order, offsets, counts, _t(centres), ws=ws)
        assert torch.equal(again, got)


def test_update_argument_checks():
    rows = torch.zeros(8, 64, device=DEV, dtype=torch.uint8)
    counts, offsets, order = eg.ops.group_rows(torch.zeros(8, device=DEV, dtype=torch.int32), 2)
    centres = torch.zeros(2, 64, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="multiple of 64"):
        eg.ops.kmeans_update_u8(torch.zeros(8, 96, device=DEV, dtype=torch.uint8), order, offsets, counts, centres)
    with pytest.raises(ValueError, match="centres"):
        eg.ops.kmeans_update_u8(rows, order, offsets, counts, centres[:1])
    with pytest.raises(ValueError, match="order"):
        eg.ops.kmeans_update_u8(rows, order[:4], offsets, counts, centres)
    with pytest.raises(ValueError, match="offsets"):
        eg.ops.kmeans_update_u8(rows, order, offsets[:2], counts, centres)


# ---- the seeding ------------------------------------------------------------------------------------------------------------------------
def _seed_rows(n, K, seed, distinct=None):
    """random rows, every third one a copy of an earlier row; ``distinct``: only that many different rows"""
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, 256, (n, K)).astype(np.uint8)
    if distinct is not None:
        rows = rows[:distinct][rng.permutation(np.arange(n) % distinct)]
    else:
        for i in range(3, n, 3):
            rows[i] = rows[rng.randint(0, i)]
    return rows


def _check_seed(rows, bins, u):
    flag = _flag()
    idx, centres = eg.ops.kmeans_seed_u8(_t(rows), bins, _t(np.asarray(u, np.float32)), flag=flag)
    want_idx, want_centres, want_flag = KR.seed(rows, bins, u)
    assert int(flag) == want_flag
    if not want_flag & KR.FLAG_DUPLICATES:
        assert torch.equal(idx, _t(want_idx, torch.int32)) and torch.equal(centres, _t(want_centres))
    return idx.cpu().numpy()


def test_seed_one_row():
    rows = _seed_rows(1, 64, 0)
    assert _check_seed(rows, 1, [0.7]).tolist() == [0]
    flag = _flag()
    eg.ops.kmeans_seed_u8(_t(rows), 2, _t(np.array([0.7, 0.2], np.float32)), flag=flag)
    assert int(flag) == eg.ops.SEED_FLAG_DUPLICATES


@pytest.mark.parametrize("K", [64, 192, 2112])                    # 2112: two full steps of a wave over a row and 64 bytes of a third
@pytest.mark.parametrize("shape", ["rows-1", "rows+1", "3 rows+5"])
def test_seed_at_the_workgroup_edges(shape, K):
    R = eg.ops.kmeans_seed_rows()
    n = {"rows-1": R - 1, "rows+1": R + 1, "3 rows+5": 3 * R + 5}[shape]
    rows = _seed_rows(n, K, n + K)
    u = [0.0, BELOW_ONE, 0.5, 0.0, BELOW_ONE, 0.123, 0.877]
    idx = _check_seed(rows, len(u), u)
    picked = {rows[i].tobytes() for i in idx}
    assert len(picked) == len(u), "a copy of a chosen centre was picked"
    assert _check_seed(rows, 1, [BELOW_ONE]).tolist() == [n - 1]


def test_seed_over_more_workgroups_than_the_pick_has_threads():
    """the one-workgroup pick gives each of its 1024 threads a run of consecutive partial sums: two a thread here, the last runs short"""
    R = eg.ops.kmeans_seed_rows()
    n = 1024 * R + R + 3
    rows = _seed_rows(n, 64, 11)
    idx = _check_seed(rows, 5, [0.3, BELOW_ONE, 0.0, 0.61, 0.5])
    assert idx[1] >= n - 3 * R and idx[2] <= 1 and len({rows[i].tobytes() for i in idx}) == 5


def test_seed_with_as_many_bins_as_distinct_rows_and_one_more():
    R = eg.ops.kmeans_seed_rows()
    rows = _seed_rows(2 * R + 9, 192, 5, distinct=6)
    u = np.random.RandomState(1).rand(7).astype(np.float32)
    idx = _check_seed(rows, 6, u[:6])
    assert len({rows[i].tobytes() for i in idx}) == 6
    flag = _flag()
    eg.ops.kmeans_seed_u8(_t(rows), 7, _t(u), flag=flag)
    assert int(flag) == eg.ops.SEED_FLAG_DUPLICATES
    flag = _flag()
    eg.ops.kmeans_seed_u8(_t(rows), 3, _t(np.array([0.5, 1.0, 0.5], np.float32)), flag=flag)
    assert int(flag) == eg.ops.SEED_FLAG_U
    with pytest.raises(ValueError, match="fp32"):
        eg.ops.kmeans_seed_u8(_t(rows), 3, _t(u[:3]).double())
    with pytest.raises(ValueError, match="bins"):
        eg.ops.kmeans_seed_u8(_t(rows), 0, _t(u[:0]))


# ---- Lloyd's loop -----------------------------------------------------------------------------------------------------------------------
N, K, MODES, ITERS = 600, 192, 30, 6


@pytest.fixture(scope="module")
def mixture():
    return KR.mixture(N, K, MODES, seed=1)


@pytest.mark.parametrize("bins", [7, 129])                        # 129 crosses the search's 128-row database tile
def test_kmeans_end_to_end(mixture, bins):
    u = eg.quality.bin_uniforms(3, bins)
    want_c, want_l, want_n, want_log, want_flag = KR.kmeans(mixture, bins, ITERS, u=u.cpu().numpy())
    assert want_flag == 0
    rows = _t(mixture)
    flag = _flag()
    centres, labels, counts, log = eg.ops.kmeans_u8(rows, bins, ITERS, u=u, flag=flag)
    print("inertia", log["inertia"].tolist(), "changed", log["changed"].tolist())
    assert int(flag) == 0
    assert torch.equal(centres, _t(want_c)) and torch.equal(labels, _t(want_l, torch.int32)) and torch.equal(counts, _t(want_n, torch.int32))
    assert log["inertia"].dtype == torch.int64 and torch.equal(log["inertia"], _t(want_log["inertia"]))
    assert log["changed"].dtype == torch.int32 and torch.equal(log["changed"], _t(want_log["changed"], torch.int32))
    again = eg.ops.kmeans_u8(rows, bins, ITERS, u=u)
    assert torch.equal(again[0], centres) and torch.equal(again[1], labels) and torch.equal(again[2], counts)
    assert torch.equal(again[3]["inertia"], log["inertia"]) and torch.equal(again[3]["changed"], log["changed"])
    # init= replaces the seeding: the seeding's rows, and the seeding's centres
    idx, seeded = eg.ops.kmeans_seed_u8(rows, bins, u)
    for init in (idx, idx.long(), seeded):
        other = eg.ops.kmeans_u8(rows, bins, ITERS, init=init)
        assert torch.equal(other[0], centres) and torch.equal(other[1], labels) and torch.equal(other[3]["inertia"], log["inertia"])


def test_an_empty_cell_keeps_its_bytes(mixture):
    rows = _t(mixture)
    init = np.concatenate((mixture[[0, 100, 200]], np.full((1, K), 255, np.uint8), np.zeros((1, K), np.uint8)))   # two centres far from every row
    centres, labels, counts, log = eg.ops.kmeans_u8(rows, 5, 3, init=_t(init))
    want = KR.kmeans(mixture, 5, 3, init=init)
    assert counts.tolist()[3:] == [0, 0] and torch.equal(centres[3:], _t(init[3:]))
    assert torch.equal(centres, _t(want[0])) and torch.equal(labels, _t(want[1], torch.int32)) and torch.equal(log["inertia"], _t(want[3]["inertia"]))
    zero = eg.ops.kmeans_u8(rows, 5, 0, init=_t(init))             # no iteration: the assignment to the initial centres
    assert torch.equal(zero[0], _t(init)) and zero[3]["changed"].numel() == 0 and zero[3]["inertia"].tolist() == [int(KR.assign(mixture, init)[1].sum())]
    with pytest.raises(ValueError, match="either u"):
        eg.ops.kmeans_u8(rows, 5, 3)
    with pytest.raises(ValueError, match="either u"):
        eg.ops.kmeans_u8(rows, 5, 3, u=eg.quality.bin_uniforms(0, 5), init=_t(init))
    with pytest.raises(ValueError, match="centres"):
        eg.ops.kmeans_u8(rows, 5, 3, init=_t(init[:4]))


# ---- the score --------------------------------------------------------------------------------------------------------------------------
BINS = 30


def _img(a):
    return _t(a).reshape(len(a), 3, 8, 8)


@pytest.fixture(scope="module")
def sets(mixture):
    dropped = KR.mixture(N, K, MODES, seed=2, keep=range(10, MODES))           # 10 modes removed
    same = KR.mixture(N, K, MODES, seed=3)
    return mixture, dropped, same


def test_ndb_equals_the_restatement_and_sees_dropped_modes(sets):
    real, dropped, same = sets
    u = eg.quality.bin_uniforms(0, BINS).cpu().numpy()
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    got = eg.quality.ndb(_img(real), _img(dropped), bins=BINS, iterations=ITERS, terms=True)
    want = KR.ndb(real, dropped, BINS, ITERS, u)
    print(got[0])
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2].tolist() and got[3] == want[3].tolist()
    assert sorted(got[0]) == ["bins", "changed_last", "empty_fake", "empty_real", "inertia", "js", "ndb", "ndb_over_bins"]
    base = eg.quality.ndb(_img(real), _img(same), bins=BINS, iterations=ITERS)
    assert base == KR.ndb(real, same, BINS, ITERS, u)[0]
    print(base)
    assert got[0]["ndb"] > base["ndb"] and got[0]["js"] > base["js"] and got[0]["empty_fake"] > base["empty_fake"]
    assert eg.quality.ndb(_img(real), _img(dropped), bins=BINS, iterations=ITERS) == got[0]            # two calls, the same numbers
    other = eg.quality.ndb(_img(real), _img(dropped), bins=BINS, iterations=ITERS, seed=1)
    assert other == KR.ndb(real, dropped, BINS, ITERS, eg.quality.bin_uniforms(1, BINS).cpu().numpy())[0]
    loose = eg.quality.ndb(_img(real), _img(dropped), bins=BINS, iterations=ITERS, z_threshold=1e9)
    assert loose["ndb"] == 0 and loose["js"] == got[0]["js"]


def test_ndb_of_a_set_with_itself_is_zero(sets):
    real = _img(sets[0])
    out = eg.quality.ndb(real, real, bins=BINS, iterations=ITERS)
    assert out["ndb"] == 0 and out["js"] == 0.0 and out["ndb_over_bins"] == 0.0 and out["empty_real"] == out["empty_fake"]


def test_ndb_honours_given_centres_and_image_bins(sets, tmp_path):
    real, dropped, _ = sets
    fit = eg.quality.image_bins(_img(real), BINS, ITERS, seed=0)
    want_c, want_l, want_n, want_log, _ = KR.kmeans(real, BINS, ITERS, u=eg.quality.bin_uniforms(0, BINS).cpu().numpy())
    assert fit.centres.shape == (BINS, 3, 8, 8) and torch.equal(fit.centres.reshape(BINS, K), _t(want_c))
    assert torch.equal(fit.counts, _t(want_n, torch.int32)) and torch.equal(fit.labels, _t(want_l, torch.int32))
    assert torch.equal(fit.inertia, _t(want_log["inertia"])) and torch.equal(fit.changed, _t(want_log["changed"], torch.int32))
    assert torch.equal(eg.quality.bin_counts(_img(dropped), fit.centres), _t(KR.bin_counts(dropped, want_c), torch.int32))
    fitted = eg.quality.ndb(_img(real), _img(dropped), bins=BINS, iterations=ITERS)
    given = eg.quality.ndb(_img(real), _img(dropped), centres=fit.centres)
    assert given["inertia"] is None and given["changed_last"] is None
    assert {k: v for k, v in given.items() if k not in ("inertia", "changed_last")} == {k: v for k, v in fitted.items() if k not in ("inertia", "changed_last")}
    elsewhere = real[:7].reshape(7, 3, 8, 8)                      # any centres: the first seven rows
    got = eg.quality.ndb(_img(real), _img(dropped), centres=_t(elsewhere), terms=True)
    want = KR.ndb(real, dropped, None, None, None, centres=real[:7])
    assert got[0] == want[0] and got[1] == want[1] and got[0]["bins"] == 7
    grid = eg.quality.bin_grid(_t(elsewhere), got[1])
    order = sorted(range(7), key=lambda c: (got[1][c], c))
    assert grid.shape == (7, 3, 8, 8) and torch.equal(grid, _t((elsewhere[order].astype(np.float32) / np.float32(255.0))))
    eg.quality.save_bins(str(tmp_path / "bins.png"), _t(elsewhere), got[1], nrow=4)
    want_png = eg.sampling.encode_png(eg.sampling.to_uint8_hwc(grid, nrow=4))
    assert open(tmp_path / "bins.png", "rb").read() == want_png and want_png[:8] == b"\x89PNG\r\n\x1a\n"


def test_ndb_takes_float_images_as_their_bytes(sets):
    real, dropped, _ = sets
    fr, ff = (_img(a).float() * (2.0 / 255.0) - 1.0 for a in (real, dropped))
    assert torch.equal(eg.quality.to_u8(fr), _img(real)) and torch.equal(eg.quality.to_u8(ff), _img(dropped))
    assert eg.quality.ndb(fr, ff, bins=BINS, iterations=ITERS) == eg.quality.ndb(_img(real), _img(dropped), bins=BINS, iterations=ITERS)


def test_ndb_value_errors(sets):
    real = _img(sets[0])
    with pytest.raises(ValueError, match="bins = 601"):
        eg.quality.ndb(real, real, bins=601)
    with pytest.raises(ValueError, match="bins = 0"):
        eg.quality.ndb(real, real, bins=0)
    with pytest.raises(ValueError, match="iterations = -1"):
        eg.quality.ndb(real, real, bins=4, iterations=-1)
    with pytest.raises(ValueError, match="one shape"):
        eg.quality.ndb(real, real.reshape(N, 3, 4, 16))
    with pytest.raises(ValueError, match="z_threshold"):
        eg.quality.ndb(real, real, bins=4, z_threshold=0.0)
    with pytest.raises(ValueError, match="centres"):
        eg.quality.ndb(real, real, centres=real[:4].float())
    copies = real[:3].repeat(50, 1, 1, 1)                          # three distinct images
    assert eg.quality.ndb(copies, copies, bins=3, iterations=2)["ndb"] == 0
    with pytest.raises(ValueError, match="fewer than bins = 4 distinct"):
        eg.quality.ndb(copies, copies, bins=4, iterations=2)
    with pytest.raises(ValueError, match="fewer than bins = 4 distinct"):
        eg.quality.image_bins(copies, 4, 2)
    with pytest.raises(ValueError, match="float or uint8 device tensor"):
        eg.quality.ndb(real.cpu(), real)
    with pytest.raises(ValueError, match="'mnist' or 'celeba'|sprite"):
        eg.quality.ndb_generator("dsprites", None, None)

"""k-means over uint8 rows and the NDB score without a GPU: the numpy int64 restatement (tests/kmeans_refs.py) against Python
integers, the rounding and seeding rules on hand-made numbers, the NDB / JS arithmetic on hand counts, the ABI and the plan's validation.
All equalities are exact."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import kmeans_refs as KR


def _pkg():
    return importlib.import_module("ead-gan_amd")


def test_restatement_against_python_integers_on_a_tiny_case():
    rng = np.random.RandomState(0)
    rows = rng.randint(0, 256, (23, 64)).astype(np.uint8)
    rows[5] = rows[2]                                              # a duplicate: never picked after its twin
    rows[11, :] = 255
    rows[12, :] = 0
    u = np.array([0.37, 0.0, 0.5, 0.999, 0.25], np.float32)
    idx, centres, flag = KR.seed(rows, 5, u)
    assert flag == 0 and idx.tolist() == KR.seed_brute(rows, 5, u) and len(set(idx.tolist())) == 5
    assert np.array_equal(centres, rows[idx])
    labels, dist = KR.assign(rows, centres)
    for i in range(len(rows)):
        ds = [sum((int(a) - int(b)) ** 2 for a, b in zip(rows[i], c)) for c in centres]
        assert dist[i] == min(ds) and labels[i] == ds.index(min(ds))
    new = KR.update(rows, labels, centres)
    assert np.array_equal(new, KR.update_brute(rows, labels, centres))
    # an empty cell keeps its bytes
    far = np.concatenate((centres[:4], np.full((1, 64), 7, np.uint8)))
    far_labels = np.minimum(labels, 3)
    assert np.array_equal(KR.update(rows, far_labels, far)[4], far[4]) and np.array_equal(KR.update(rows, far_labels, far), KR.update_brute(rows, far_labels, far))
    c2, l2, counts, log, flag = KR.kmeans(rows, 5, 3, u=u)
    assert flag == 0 and counts.sum() == 23 and len(log["inertia"]) == 4 and log["changed"][0] == 23
    assert np.array_equal(np.bincount(l2, minlength=5), counts) and log["inertia"][-1] == KR.assign(rows, c2)[1].sum()
    c3, l3, _, log3, _ = KR.kmeans(rows, 5, 3, init=idx)
    assert np.array_equal(c3, c2) and np.array_equal(l3, l2) and np.array_equal(log3["inertia"], log["inertia"])
    c4 = KR.kmeans(rows, 5, 3, init=centres)[0]
    assert np.array_equal(c4, c2)


def test_group_is_a_stable_counting_sort():
    labels = np.array([2, 0, 2, 5, 1, 2, -1, 0, 4, 0])
    counts, offsets, order, flag = KR.group(labels, 4)
    assert counts.tolist() == [3, 1, 3, 0] and offsets.tolist() == [0, 3, 4, 7, 7] and flag == 1
    assert order.tolist() == [1, 7, 9, 4, 0, 2, 5, -1, -1, -1]
    counts, offsets, order, flag = KR.group(np.array([0, 0, 0]), 1)
    assert counts.tolist() == [3] and offsets.tolist() == [0, 3] and order.tolist() == [0, 1, 2] and flag == 0


def test_half_up_rounding_on_hand_made_sums():
    assert KR.round_half_up([0, 1, 2, 3, 509, 510], 2).tolist() == [0, 1, 1, 2, 255, 255]        # .5 goes up
    assert KR.round_half_up([4, 5, 6, 7, 8], 3).tolist() == [1, 2, 2, 2, 3]                      # 1.33 1.67 2 2.33 2.67
    assert KR.round_half_up([0, 17, 255], 1).tolist() == [0, 17, 255]                            # count = 1 returns the row
    rows = np.array([[0] * 64, [1] * 64, [255] * 64, [254] * 64], np.uint8)
    out = KR.update(rows, np.array([0, 0, 1, 1]), np.zeros((3, 64), np.uint8) + 9)
    assert out[0].tolist() == [1] * 64 and out[1].tolist() == [255] * 64 and out[2].tolist() == [9] * 64
    top = 8421504                                                  # the largest n with n * 255 < 2^31: the extreme sum stays exact
    assert KR.round_half_up([top * 255], top).tolist() == [255] and top * 255 < 2 ** 31 <= (top + 1) * 255


def test_seeding_rule_on_hand_made_distances():
    mind = [0, 3, 0, 2, 5, 0]                                      # total 10, inclusive prefix 0 3 3 5 10 10
    u = lambda target: np.float32((target + 0.25) / 10)           # floor(u * 10) == target
    assert [KR.seed_pick(mind, u(t))[0] for t in range(10)] == [1, 1, 1, 3, 3, 4, 4, 4, 4, 4]
    assert KR.seed_pick(mind, np.float32(0.3))[0] == 3            # float32(0.3) > 0.3: the target is 3, ON the prefix boundary: 3 does not exceed 3
    assert KR.seed_pick(mind, np.float32(0.0)) == (1, 0)          # never row 0, whose distance is 0
    # the largest fp32 below 1: the target is total - 1 for small totals and stays below total for the largest one (the product of a
    # 24-bit u and a total <= 2^53 is one rounded multiplication, and u total <= total - total 2^-24 never rounds up to total)
    below_one = np.float32(1.0 - 2.0 ** -24)
    assert below_one < 1 and np.nextafter(below_one, np.float32(2)) == 1
    assert KR.seed_pick(mind, below_one) == (4, 0) and KR.seed_pick([1, 0, 1, 0], below_one) == (2, 0)
    for total in (1, 10, 2 ** 24 + 1, 2 ** 53 - 1, 2 ** 53, (2 ** 31 - 1) * 2 ** 22):
        assert math.floor(float(below_one) * float(total)) <= total - 1
    assert KR.seed_pick([2 ** 53 - 2, 1], below_one)[0] == 0 and KR.seed_pick([1, 2 ** 53 - 2], below_one)[0] == 1
    # a u that rounds to total -- only u = 1.0 itself, which is outside [0, 1) -- is clamped to total - 1: the last row with a distance
    assert math.floor(1.0 * 10.0) == 10 and KR.seed_pick(mind, np.float32(1.0))[0] == 4
    for t in range(10):                                            # rows at distance 0 are never picked
        assert mind[KR.seed_pick(mind, u(t))[0]] > 0
    assert KR.seed_pick([0, 0, 0], np.float32(0.5)) == (0, KR.FLAG_DUPLICATES)
    assert KR.first_pick(np.float32(0.0), 7) == 0 and KR.first_pick(below_one, 7) == 6 and KR.first_pick(np.float32(0.5), 7) == 3
    assert KR.first_pick(below_one, 2 ** 22) == 2 ** 22 - 1
    rows = np.zeros((4, 64), np.uint8)
    rows[2] = 1
    idx, _, flag = KR.seed(rows, 2, np.array([0.0, 0.9], np.float32))
    assert idx.tolist() == [0, 2] and flag == 0
    assert KR.seed(rows, 3, np.array([0.0, 0.9, 0.5], np.float32))[2] == KR.FLAG_DUPLICATES
    assert KR.seed(rows, 2, np.array([0.0, 1.0], np.float32))[2] == KR.FLAG_U


def test_ndb_and_js_arithmetic_on_hand_counts():
    eg = _pkg()
    stats = eg.quality.ndb_statistics
    a = [10, 20, 0, 30, 40]
    out, z = stats(a, a)
    assert out == {"bins": 5, "ndb": 0, "ndb_over_bins": 0.0, "js": 0.0, "empty_real": 1, "empty_fake": 1} and z == [0.0] * 5
    assert out == KR.ndb_stats(a, a) and z == KR.z_scores(a, a)
    assert stats([3, 1, 0, 0], [0, 0, 2, 2])[0]["js"] == 1.0      # disjoint supports; |z| = 2.19, 1.07, 1.63, 1.63 at four rows a set
    assert stats([3, 1, 0, 0], [0, 0, 2, 2])[0]["ndb"] == 1
    out, z = stats([30, 10, 0, 0], [0, 0, 20, 20])                 # the same shares at forty: |z| = 6.9, 3.4, 5.2, 5.2
    assert out["js"] == 1.0 and out["ndb"] == 4 and out["empty_real"] == 2 and out["empty_fake"] == 2
    assert z[0] < 0 < z[2]                                         # z < 0: under-produced
    out, z = stats([5, 0, 5], [4, 0, 6])
    assert z[1] == 0.0 and out["empty_real"] == 1                  # a = b = 0: SE = 0 and z = 0
    # one bin exactly on each side of the threshold
    a, b = [50, 30, 20], [40, 35, 25]
    _, z = stats(a, b)
    N = M = 100
    P = 90 / 200
    assert z[0] == (0.4 - 0.5) / math.sqrt(P * (1.0 - P) * (1.0 / N + 1.0 / M))
    mags = sorted(abs(v) for v in z)
    assert mags[0] < mags[1] < mags[2]
    assert stats(a, b, z_threshold=mags[2])[0]["ndb"] == 0                                     # |z| == threshold is not different
    assert stats(a, b, z_threshold=math.nextafter(mags[2], 0.0))[0]["ndb"] == 1
    assert stats(a, b, z_threshold=mags[1])[0]["ndb"] == 1 and stats(a, b, z_threshold=math.nextafter(mags[1], 0.0))[0]["ndb"] == 2
    got = stats([900, 100], [850, 150])[0]                         # z = 3.38: different at the default level
    assert got["ndb"] == 2 and got["ndb_over_bins"] == 1.0 and 0.0 < got["js"] < 0.01
    assert stats([900, 100], [890, 110])[0]["ndb"] == 0            # z = 0.73
    for a, b in (([7, 3, 9, 1], [5, 5, 5, 5]), ([1, 0, 0, 9], [0, 4, 6, 0]), ([12, 7], [100, 3])):
        assert stats(a, b)[0] == KR.ndb_stats(a, b) and stats(a, b)[1] == KR.z_scores(a, b)
        assert 0.0 <= stats(a, b)[0]["js"] <= 1.0
    assert eg.quality.Z_975 == KR.Z_975 == 1.959963984540054
    with pytest.raises(ValueError, match="ndb_statistics"):
        stats([0, 0], [1, 2])
    with pytest.raises(ValueError, match="ndb_statistics"):
        stats([1, 2, 3], [1, 2])


def test_abi_and_public_names():
    eg = _pkg()
    protos = eg._lib.parse_header()
    for name in ("eg_group_rows", "eg_group_rows_block", "eg_group_rows_ws_bytes", "eg_kmeans_update_u8", "eg_kmeans_update_ws_bytes",
                 "eg_kmeans_segment_rows", "eg_kmeans_column_chunk", "eg_kmeans_seed_u8", "eg_kmeans_seed_ws_bytes", "eg_kmeans_seed_rows"):
        assert name in protos, name
    assert len(protos["eg_group_rows"][1]) == 9 and len(protos["eg_kmeans_update_u8"][1]) == 10 and len(protos["eg_kmeans_seed_u8"][1]) == 10
    assert protos["eg_kmeans_update_ws_bytes"][0] is ctypes.c_size_t
    for fn in ("group_rows", "kmeans_update_u8", "kmeans_seed_u8", "kmeans_u8"):
        assert callable(getattr(eg.ops, fn)), fn
    for fn in ("image_bins", "bin_counts", "ndb", "ndb_statistics", "bin_grid", "save_bins", "ndb_generator", "NDBPlan", "Bins"):
        assert callable(getattr(eg.quality, fn)), fn
    assert eg.quality.NDBPlan(64) == (64, 100, 20, 0) and eg.quality.Bins._fields == ("centres", "counts", "labels", "inertia", "changed")
    assert "6r" in eg.quality.__doc__ and "ndb_generator" in eg.quality.__doc__ and "held-out" in eg.quality.__doc__
    assert eg.quality.SID_BINS >> 8 == 0x5D and eg.quality.SID_BINS not in (eg.quality.SID_POSITIONS, eg.quality.SID_DIRECTIONS, eg.quality.SID_NOISE,
                                                                             eg.quality.SID_LABELS, eg.quality.SID_CODE)
    lib = eg._lib.lib()
    assert lib.query("eg_group_rows_block") >= 64 and lib.query("eg_kmeans_segment_rows") >= 1 and lib.query("eg_kmeans_column_chunk") % 64 == 0
    assert lib.query("eg_group_rows_ws_bytes", 0, 4) == 0 and lib.query("eg_group_rows_ws_bytes", 1000, 4) > 0
    seg = lib.query("eg_kmeans_segment_rows")
    assert lib.query("eg_kmeans_update_ws_bytes", 10 * seg, 64, 3) >= (10 + 3) * 64 * 4
    # the argument checks of the entry points need no GPU: they come before any launch
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    for bins in (0, 1025):
        with pytest.raises(RuntimeError, match="1 <= bins <= 1024"):
            lib.call("eg_group_rows", p, 8, bins, p, p, p, p, p, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("eg_group_rows", p, 8, 3, p, p, p, p, None, None)
    with pytest.raises(RuntimeError, match=r"n \* 255 < 2\^31"):
        lib.call("eg_kmeans_update_u8", p, 8421505, 64, p, p, p, 2, p, p, None)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        lib.call("eg_kmeans_update_u8", p, 100, 96, p, p, p, 2, p, p, None)
    with pytest.raises(RuntimeError, match=r"n \* 2\^31 <= 2\^53"):
        lib.call("eg_kmeans_seed_u8", p, 2 ** 22 + 1, 64, 2, p, p, p, p, p, None)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        lib.call("eg_kmeans_seed_u8", p, 100, 32, 2, p, p, p, p, p, None)


def test_plan_validation_of_a_run_needs_no_gpu():
    eg = _pkg()
    Plan = eg.quality.NDBPlan

    def check(plan, kind="mnist", n_dataset=20, batch=8):
        return eg.train.check_plan("ndb", plan, Plan, kind, n_dataset, batch)

    assert check(Plan(16, 4)) == (16, 4, 20, 0) and check((16, 5, 3, 9)) == Plan(16, 5, 3, 9) and check(Plan(4, 2), batch=8) == Plan(4, 2)
    assert check(Plan(16, 16, 0)) == Plan(16, 16, 0)
    for kind in ("pxy", "dsprites", "colored"):
        with pytest.raises(ValueError, match="ndb: only 'mnist' and 'celeba'"):
            check(Plan(16, 4), kind=kind)
    with pytest.raises(ValueError, match="ndb: n_images = 64, the dataset has 20 images"):
        check(Plan(64))
    with pytest.raises(ValueError, match="ndb: n_images = 12 is no multiple of the trainer's batch size 8"):
        check(Plan(12, 4))
    with pytest.raises(ValueError, match=r"ndb: bins = 100 must be in 1 \.\. min\(1024, n_images = 16\)"):
        check(Plan(16))
    with pytest.raises(ValueError, match="ndb: bins = 0"):
        check(Plan(16, 0))
    with pytest.raises(ValueError, match="ndb: iterations = -1"):
        check(Plan(16, 4, -1))
    assert eg.train.ndb_seed(3, 10, 0) == (3 * 1000003 + 10 * 2909 + 86420) % 2 ** 32
    assert len({eg.train.ndb_seed(3, 10), eg.train.sinkhorn_seed(3, 10), eg.train.mmd_seed(3, 10), eg.train.nn_seed(3, 10), eg.train.swd_seed(3, 10)}) == 5

"""The radial power spectrum without a GPU: the integer ring tables, the closed forms the numpy restatement
(tests/spectrum_refs.py) must reproduce, the host statistics on hand-made vectors, the ABI and the plan's validation."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import spectrum_refs as SR


def _pkg():
    return importlib.import_module("ead-gan_amd")


@pytest.mark.parametrize("H, B", [(16, 12), (32, 24), (64, 46)])
def test_ring_tables(H, B):
    eg = _pkg()
    got, ref = eg.quality.radial_bins(H), SR.tables(H)
    KX = H // 2 + 1
    assert got["rings"] == ref["rings"] == B and sorted(got) == sorted(ref)
    for key in ("cell_ring", "ring_start", "ring_cells", "ring_count", "weight"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], ref[key]), key
    assert int(got["ring_count"].sum()) == H * H and got["ring_start"][0] == 0 and got["ring_start"][-1] == H * KX
    square = got["cell_ring"][:KX, :KX]
    assert np.array_equal(square, square.T)                                  # the rule is symmetric in (fy, fx)
    assert np.array_equal(got["cell_ring"][1:], got["cell_ring"][1:][::-1])  # ky and H - ky share a ring
    # (b - 1/2)^2 <= q < (b + 1/2)^2, in integers: 4 q against (2 b -+ 1)^2
    for ky in range(H):
        for kx in range(KX):
            q, b = min(ky, H - ky) ** 2 + kx ** 2, int(got["cell_ring"][ky, kx])
            assert (2 * b - 1) ** 2 <= 4 * q < (2 * b + 1) ** 2 or (b == 0 and q == 0)
    # every ring lists its own cells, ascending
    for b in range(B):
        cells = got["ring_cells"][got["ring_start"][b]:got["ring_start"][b + 1]]
        assert np.all(np.diff(cells) > 0) and np.all(got["cell_ring"].reshape(-1)[cells] == b)
        assert int(got["weight"][cells % KX].sum()) == int(got["ring_count"][b])
    tw = eg.ops.spectrum_host_tables(H)["cos_sin"]
    k = np.arange(H)
    assert tw.dtype == np.float64 and np.array_equal(tw, np.stack((np.cos(2 * np.pi * k / H), np.sin(2 * np.pi * k / H))))


def test_sides_outside_the_contract_are_refused():
    eg = _pkg()
    for H in (8, 48, 128, 0):
        with pytest.raises(ValueError, match="image side"):
            eg.quality.radial_bins(H)


@pytest.mark.parametrize("H", [16, 32, 64])
def test_closed_forms_of_the_restatement(H):
    rng = np.random.RandomState(H)
    KX = H // 2 + 1
    # one bright pixel: |X| = v everywhere, so every cell and every ring holds v^2 / H^2
    v = 201
    x = np.zeros((1, 1, H, H), np.uint8)
    x[0, 0, 5, 11] = v
    assert np.allclose(SR.profile(x), v * v / H ** 2, rtol=1e-12, atol=0)
    # vertical stripes 255 (x odd): X(0, 0) = 255 H^2 / 2, X(0, H/2) = -255 H^2 / 2, nothing else
    x = np.zeros((1, 1, H, H), np.uint8)
    x[..., 1::2] = 255
    P = SR.full(x)[0]
    want = np.zeros((H, KX))
    want[0, 0] = want[0, H // 2] = 255.0 ** 2 * H ** 2 / 4
    assert np.allclose(P, want, rtol=1e-12, atol=1e-6)
    tab = SR.tables(H)
    prof = np.zeros(tab["rings"])
    prof[0] = want[0, 0]
    prof[H // 2] = want[0, H // 2] / tab["ring_count"][H // 2]
    assert np.allclose(SR.profile(x)[0], prof, rtol=1e-12, atol=1e-6)
    # Parseval against the integer sum of squares, per image and through the ring counts
    x = rng.randint(0, 256, (3, 2, H, H)).astype(np.uint8)
    energy = (x.astype(np.int64) ** 2).sum((1, 2, 3))
    assert np.allclose((SR.power(x) * tab["weight"]).sum((1, 2, 3)), energy, rtol=1e-12)
    assert np.allclose((SR.profile(x) * tab["ring_count"]).sum(1) * 2, energy, rtol=1e-12)
    assert np.allclose(SR.mean_spectrum(x)[H // 2, H // 2], SR.log_db(SR.full(x).mean(0)[0, 0]), rtol=1e-12)


def test_statistics_on_hand_made_vectors():
    eg = _pkg()
    stat = eg.quality.spectrum_statistics
    H, B = 16, 12
    mr = [50.0, 40.0, 30.0, 20.0, 10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0]
    mf = [90.0, 40.0, 33.0, 20.0, 10.0, 9.0, 5.0, 7.0, 6.0, 5.0, 4.0, 4.0]      # gaps: 40 (ring 0), +3 (ring 2), -3 (ring 6), +1 (ring 11)
    vr = [1.0, 0.0, 2.0, 0.0, 1.0, 1.0, 4.0, 1.0, 1.0, 1.0, 1.0, 0.5]
    vf = [1.0, 0.0, 6.0, 0.0, 1.0, 1.0, 14.0, 1.0, 1.0, 1.0, 1.0, 1.5]
    got = stat(mr, vr, mf, vf, H)
    assert sorted(got) == ["distance_db", "effect", "fake_db", "gap_db", "high_db", "peak_db", "peak_ring", "real_db", "rings"]
    assert got["rings"] == B and got["real_db"] == mr and got["fake_db"] == mf
    assert got["gap_db"] == [40.0, 0.0, 3.0, 0.0, 0.0, 0.0, -3.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert got["distance_db"] == math.sqrt(19.0 / 11.0)                      # ring 0 is left out
    assert got["high_db"] == (-3.0 + 1.0) / 7.0                              # the rings 5 .. 11
    assert got["peak_ring"] == 2 and got["peak_db"] == 3.0                   # |+3| ties with |-3|: the lower ring
    assert got["effect"] == [40.0, 0.0, 1.5, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0]      # 0 / 0 -> 0
    mirrored = stat(mf, vf, mr, vr, H)
    assert mirrored["peak_ring"] == 2 and mirrored["peak_db"] == -3.0 and mirrored["gap_db"][6] == 3.0
    same = stat(mr, vr, mr, vr, H)
    assert same["gap_db"] == [0.0] * B and same["distance_db"] == 0.0 and same["high_db"] == 0.0 and same["effect"] == [0.0] * B
    assert same["peak_ring"] == 1 and same["peak_db"] == 0.0
    ref = SR.statistics(mr, vr, mf, vf, H)
    assert ref["peak_ring"] == 2 and ref["gap_db"] == got["gap_db"] and ref["effect"] == got["effect"]
    assert abs(ref["distance_db"] - got["distance_db"]) < 1e-15 and abs(ref["high_db"] - got["high_db"]) < 1e-15
    with pytest.raises(ValueError, match="four vectors"):
        stat(mr, vr[:-1], mf, vf, H)


def test_abi_declares_and_exports_the_entry_point():
    eg = _pkg()
    protos = eg._lib.parse_header()
    restype, argtypes = protos["eg_spectrum_u8"]
    assert restype is ctypes.c_int and len(argtypes) == 12
    assert argtypes[1:4] == [ctypes.c_int] * 3 and all(a is ctypes.c_void_p for a in argtypes[:1] + argtypes[4:])
    lib = eg._lib.lib()
    assert hasattr(lib.cdll, "eg_spectrum_u8")
    # the entry point repeats the Python layer's refusals before it touches a pointer
    for N, C, H in ((1, 1, 48), (1, 5, 64), (1, 0, 64), (0, 1, 16)):
        assert lib.query("eg_spectrum_u8", 8, N, C, H, 8, 8, 8, 8, 8, 8, None, None) == -1
        assert b"eg_spectrum_u8" in lib.cdll.eg_last_error()


def test_plan_validation():
    eg = _pkg()
    Plan, check = eg.quality.SpectrumPlan, eg.train.check_plan
    assert Plan(64) == (64, 0) and check("spectrum", Plan(64, 3), Plan, "mnist", 100, 32) == Plan(64, 3)
    with pytest.raises(ValueError, match="spectrum: n_images = 128, the dataset has 100 images"):
        check("spectrum", Plan(128), Plan, "mnist", 100, 32)
    with pytest.raises(ValueError, match="spectrum: n_images = 48 is no multiple of the trainer's batch size 32"):
        check("spectrum", Plan(48), Plan, "celeba", 100, 32)
    with pytest.raises(ValueError, match="spectrum: n_images = 1, the variance"):
        check("spectrum", Plan(1), Plan, "mnist", 100, 32)
    with pytest.raises(ValueError, match="only 'mnist' and 'celeba' runs"):
        check("spectrum", Plan(64), Plan, "dsprites", 100, 32)
    a, b = eg.train.spectrum_seed(3, 10, 0), eg.train.ndb_seed(3, 10, 0)
    assert a != b and 0 <= a < 2 ** 32 and eg.train.spectrum_seed(3, 10, 1) != a and eg.train.spectrum_seed(3, 11, 0) != a

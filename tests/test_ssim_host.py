"""SSIM, MS-SSIM and PSNR over image pairs without a GPU: the window table, the level count, the closed forms the numpy
restatement (tests/ssim_refs.py) must reproduce, its own rounding against a long-double run, the MS-SSIM combination on hand-made
statistics, the pair table, the ABI and the plan's validation."""
import ctypes
import importlib

import numpy as np
import pytest

import ssim_refs as SS

SHAPES = [(64, 3, 11), (32, 2, 11), (16, 1, 11), (16, 2, 7)]                 # (H, L, K)


def _pkg():
    return importlib.import_module("ead-gan_amd")


def test_window_table():
    eg = _pkg()
    for K, sigma in ((11, 1.5), (7, 1.5), (3, 0.5), (5, 2.0)):
        w = eg.ops.ssim_window(K, sigma)
        k = np.arange(K, dtype=np.float64) - K // 2
        f = np.exp(-(k * k) / (2.0 * sigma * sigma))
        assert w.dtype == np.float64 and w.shape == (K,) and abs(w.sum() - 1.0) <= 1e-15
        assert np.array_equal(w, w[::-1]) and np.array_equal(w, f / f.sum()) and np.array_equal(w, SS.window(K, sigma))
    assert np.array_equal(eg.ops.ssim_window(), eg.ops.ssim_window(11, 1.5))
    for K in (3, 5, 11):
        assert np.array_equal(eg.ops.ssim_window(K, None), np.full(K, 1.0 / K)) and np.array_equal(SS.window(K, None), np.full(K, 1.0 / K))
    for K in (1, 4, 13, 2.0):
        with pytest.raises(ValueError, match="odd number of taps"):
            eg.ops.ssim_window(K)
    with pytest.raises(ValueError, match="sigma"):
        eg.ops.ssim_window(11, 0.0)


def test_levels():
    eg = _pkg()
    for (H, K), L in {(64, 11): 3, (32, 11): 2, (16, 11): 1, (16, 7): 2, (64, 3): 5}.items():
        assert eg.ops.ssim_levels(H, K) == L == SS.levels(H, K)
    for H in (8, 48, 128, 0):
        with pytest.raises(ValueError, match="image side"):
            eg.ops.ssim_levels(H, 11)
    for K in (1, 4, 13):
        with pytest.raises(ValueError, match="odd number of taps"):
            eg.ops.ssim_levels(64, K)
    assert eg.ops.SSIM_SIDES == (16, 32, 64) and eg.ops.SSIM_MAX_C == 4 and eg.ops.SSIM_MAX_K == 11 and eg.ops.SSIM_FLAG_PAIR == 2


@pytest.mark.parametrize("H, L, K", SHAPES)
def test_closed_forms_of_the_restatement(H, L, K):
    rng = np.random.RandomState(H + K)
    C = 2
    a = SS.pink(rng, 3, C, H)
    idx = np.arange(3)
    same = np.stack((idx, idx), 1)
    # identical images: exactly 1.0 at every level
    st, sse = SS.stats(a, a, same, K, 1.5, L)
    assert st.shape == (3, L, 2) and np.all(st == 1.0) and np.all(sse == 0)
    # two flat images u, v: cs = 1, ssim = (2 u v + c1) / (u^2 + v^2 + c1), at every level
    c1 = (0.01 * 255.0) ** 2
    for u, v in ((0, 255), (77, 78), (200, 13)):
        fa, fb = np.full((1, C, H, H), u, np.uint8), np.full((1, C, H, H), v, np.uint8)
        st, sse = SS.stats(fa, fb, [[0, 0]], K, 1.5, L)
        assert np.allclose(st[0, :, 1], 1.0, rtol=0, atol=1e-12)
        assert np.allclose(st[0, :, 0], (2.0 * u * v + c1) / (u * u + v * v + c1), rtol=0, atol=1e-12)
        assert sse[0] == C * H * H * (u - v) ** 2
    # a against its negative: anticorrelated
    st, _ = SS.stats(a, 255 - a, same, K, 1.5, L)
    print("ssim of a 1/f image against 255 - a, level 0:", st[:, 0, 0])
    assert np.all(st[:, 0, 0] < 0.0) and np.all(st[:, 0, 1] < 0.0)
    # a against a + 1: every byte differs by one
    low = np.minimum(a, 254)
    assert np.all(SS.stats(low, low + 1, same, K, 1.5, L)[1] == C * H * H)
    assert np.array_equal(SS.psnr([0, C * H * H], C * H * H), [np.inf, 10.0 * np.log10(255.0 ** 2)])


@pytest.mark.parametrize("H, L, K", SHAPES)
def test_restatement_against_scipy(H, L, K):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(7 * H + K)
    sets = SS.image_sets(rng, 2, 2, H)
    w = SS.window(K, 1.5)
    r = K // 2
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    for name, (a, b) in sets.items():
        st, _ = SS.stats(a, b, [[0, 0], [1, 1], [0, 1]], K, 1.5, L)
        for p, (i, j) in enumerate(((0, 0), (1, 1), (0, 1))):
            for l in range(L):
                x, y = SS.pooled(a[i], l) / 4.0 ** l, SS.pooled(b[j], l) / 4.0 ** l

                def filt(z):
                    z = ndimage.correlate1d(ndimage.correlate1d(z, w, axis=-1, mode="constant"), w, axis=-2, mode="constant")
                    return z[..., r:z.shape[-2] - r, r:z.shape[-1] - r]
                ma, mb, eaa, ebb, eab = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
                cs = (2 * (eab - ma * mb) + c2) / (eaa - ma * ma + ebb - mb * mb + c2)
                lum = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
                assert abs((lum * cs).mean() - st[p, l, 0]) <= 1e-12 and abs(cs.mean() - st[p, l, 1]) <= 1e-12, (name, p, l)


@pytest.mark.parametrize("H, L, K", SHAPES)
def test_float64_restatement_against_long_double(H, L, K):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is float64 on this platform")
    rng = np.random.RandomState(3 * H + K)
    bound = SS.error_bound(K)
    worst = 0.0
    for name, (a, b) in SS.image_sets(rng, 3, 2, H).items():
        pairs = [[0, 0], [1, 1], [2, 2], [0, 2]]
        got, _ = SS.stats(a, b, pairs, K, 1.5, L)
        ref, _ = SS.stats(a, b, pairs, K, 1.5, L, dtype=np.longdouble)
        worst = max(worst, float(np.abs(got - ref).max()))
    print(f"H = {H}, L = {L}, K = {K}: float64 against long double, max error / bound = {worst / bound:.3e}")
    assert worst <= bound
    assert abs(SS.error_bound(11) - 2.5e-10) < 0.1e-10 and abs(SS.error_bound(7) - 1.7e-10) < 0.1e-10 and SS.tolerance(11) == 2 * SS.error_bound(11)


def test_ms_ssim_combination_on_hand_made_stats():
    eg = _pkg()
    W = np.array(eg.quality.MS_SSIM_WEIGHTS)
    assert eg.quality.MS_SSIM_WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) == SS.WEIGHTS
    for L in (1, 2, 3, 4):
        w = np.array(eg.quality.ms_ssim_weights(L))
        assert np.allclose(w, W[:L] / W[:L].sum(), rtol=1e-15) and abs(w.sum() - 1.0) < 1e-15
        assert np.allclose(SS.weights(L), w, rtol=1e-15)
    assert eg.quality.ms_ssim_weights(5) == eg.quality.MS_SSIM_WEIGHTS and np.array_equal(SS.weights(5), W)       # the full five, as published
    with pytest.raises(ValueError, match="levels"):
        eg.quality.ms_ssim_weights(6)
    with pytest.raises(ValueError, match="positive numbers"):
        eg.quality.ms_ssim_weights(2, (0.5, 0.0))
    # stats[p][l] = (ssim, cs): cs of the levels below the last, ssim of the last
    st = np.array([[[0.5, 0.81], [0.64, 0.3]],               # 0.81^w0 * 0.64^w1
                   [[0.9, -0.05], [0.7, 0.2]],               # a negative cs level: 0
                   [[-0.3, 1.0], [1.0, 0.9]],                # the ssim of a level below the last does not count
                   [[0.2, 0.5], [-0.1, 0.9]]])               # a negative last ssim: 0
    w = SS.weights(2)
    assert np.allclose(SS.ms_ssim(st), [0.81 ** w[0] * 0.64 ** w[1], 0.0, 1.0, 0.0], rtol=1e-15)
    torch = pytest.importorskip("torch")
    for L in (2, 3, 5):
        rng = np.random.RandomState(L)
        st = rng.uniform(0.05, 1.0, (6, L, 2))
        st[1, 0, 1] = -0.2
        want = np.prod(SS.bases(st) ** (W[:L] / W[:L].sum() if L < 5 else W), 1)
        assert want[1] == 0.0 and np.allclose(SS.ms_ssim(st), want, rtol=1e-15)
        got = eg.quality.ms_ssim_from_stats(torch.from_numpy(st)).numpy()
        assert got[1] == 0.0 and np.allclose(got, want, rtol=1e-14)
        own = eg.quality.ms_ssim_from_stats(torch.from_numpy(st), weights=[1.0] * L).numpy()
        assert np.allclose(own, np.prod(SS.bases(st), 1), rtol=1e-14)


def test_pair_table_from_draws():
    n = 4
    i, jp = np.meshgrid(np.arange(n), np.arange(n - 1), indexing="ij")
    table = SS.pair_table_from_draws(i.reshape(-1), jp.reshape(-1))
    assert table.dtype == np.int32 and table.shape == (n * (n - 1), 2)
    assert np.all(table[:, 0] != table[:, 1]) and table.min() == 0 and table.max() == n - 1
    assert sorted(map(tuple, table.tolist())) == [(a, b) for a in range(n) for b in range(n) if a != b]       # each ordered pair exactly once
    torch = pytest.importorskip("torch")
    eg = _pkg()
    got = eg.quality._pairs_from_draws(torch.from_numpy(i.reshape(-1)), torch.from_numpy(jp.reshape(-1)))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), table)


def test_abi_declares_and_exports_the_entry_point():
    eg = _pkg()
    restype, argtypes = eg._lib.parse_header()["eg_ssim_u8"]
    assert restype is ctypes.c_int and len(argtypes) == 17
    assert argtypes[11] is ctypes.c_double and argtypes[12] is ctypes.c_double                  # c1, c2
    assert [k for k, t in enumerate(argtypes) if t is ctypes.c_int] == [1, 3, 4, 5, 7, 9, 10]   # na, nb, C, H, P, K, L
    assert all(argtypes[k] is ctypes.c_void_p for k in (0, 2, 6, 8, 13, 14, 15, 16))            # the pointers (sse: long long*) and the stream
    header = open(eg._lib.HEADER).read()
    assert "long long* sse, int* flag, eg_stream_t s);" in header
    lib = eg._lib.lib()
    assert hasattr(lib.cdll, "eg_ssim_u8") and lib.query("eg_version") >= 116
    # the entry point repeats the Python layer's refusals before it touches a pointer: (na, nb, C, H, P, K, L, c1, c2)
    for na, nb, C, H, P, K, L, c1, c2 in ((1, 1, 1, 48, 1, 11, 1, 1.0, 1.0), (1, 1, 5, 64, 1, 11, 1, 1.0, 1.0), (1, 1, 0, 64, 1, 11, 1, 1.0, 1.0),
                                          (0, 1, 1, 16, 1, 11, 1, 1.0, 1.0), (1, 0, 1, 16, 1, 11, 1, 1.0, 1.0), (1, 1, 1, 16, 0, 11, 1, 1.0, 1.0),
                                          (1, 1, 1, 64, 1, 13, 1, 1.0, 1.0), (1, 1, 1, 64, 1, 4, 1, 1.0, 1.0), (1, 1, 1, 64, 1, 1, 1, 1.0, 1.0),
                                          (1, 1, 1, 64, 1, 11, 4, 1.0, 1.0), (1, 1, 1, 16, 1, 11, 2, 1.0, 1.0), (1, 1, 1, 64, 1, 11, 0, 1.0, 1.0),
                                          (1, 1, 1, 64, 1, 3, 6, 1.0, 1.0), (1, 1, 1, 64, 1, 11, 1, 0.0, 1.0), (1, 1, 1, 64, 1, 11, 1, 1.0, -1.0),
                                          (1, 1, 1, 64, 1, 11, 1, float("inf"), 1.0), (1, 1, 1, 64, 1, 11, 1, 1.0, float("nan"))):
        assert lib.query("eg_ssim_u8", 8, na, 8, nb, C, H, 8, P, 8, K, L, c1, c2, 8, 8, 8, None) == -1, (na, nb, C, H, P, K, L, c1, c2)
        assert b"eg_ssim_u8" in lib.cdll.eg_last_error()
    assert lib.query("eg_ssim_u8", None, 1, 8, 1, 1, 16, 8, 1, 8, 11, 1, 1.0, 1.0, 8, 8, 8, None) == -1


def test_cpu_tensors_are_refused():
    torch = pytest.importorskip("torch")
    eg = _pkg()
    x = torch.zeros(4, 1, 16, 16, dtype=torch.uint8)
    pairs = torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="there is no CPU path"):
        eg.ops.ssim_u8(x, x, pairs)
    with pytest.raises(ValueError, match="there is no CPU path"):
        eg.quality.ssim(x, x)
    with pytest.raises(ValueError, match="there is no CPU path"):
        eg.quality.diversity(x)
    with pytest.raises(ValueError, match="contiguous uint8 device tensor"):
        eg.ops.ssim_u8(x.float(), x, pairs)
    with pytest.raises(ValueError, match="contiguous uint8 device tensor"):
        eg.ops.ssim_u8(x.expand(4, 2, 16, 16), x, pairs)
    with pytest.raises(ValueError, match="there is no CPU path"):
        eg.ops.ssim_window_table(11, 1.5, "cpu")


def test_plan_validation():
    eg = _pkg()
    Plan, check = eg.quality.SSIMPlan, eg.train.check_plan
    assert Plan(64) == (64, 4096, 0) and check("ssim", (16, 8, 0), Plan, "mnist", 100, 8) == Plan(16, 8, 0)
    with pytest.raises(ValueError, match="ssim: n_images = 1, a pair needs at least 2 images"):
        check("ssim", Plan(1), Plan, "mnist", 100, 32)
    with pytest.raises(ValueError, match="ssim: n_pairs = 0 must be at least 1"):
        check("ssim", Plan(64, 0), Plan, "mnist", 100, 32)
    with pytest.raises(ValueError, match="only 'mnist' and 'celeba' runs"):
        check("ssim", Plan(64), Plan, "dsprites", 100, 32)
    with pytest.raises(ValueError, match="ssim: n_images = 48 is no multiple of the trainer's batch size 32"):
        check("ssim", Plan(48), Plan, "celeba", 100, 32)
    with pytest.raises(ValueError, match="ssim: n_images = 128, the dataset has 100 images"):
        check("ssim", Plan(128), Plan, "mnist", 100, 32)
    a, b = eg.train.ssim_seed(3, 10, 0), eg.train.spectrum_seed(3, 10, 0)
    assert a != b and 0 <= a < 2 ** 32 and eg.train.ssim_seed(3, 10, 1) != a and eg.train.ssim_seed(3, 11, 0) != a
    assert eg.quality.SID_PAIRS == 0x5D30

"""SSIM, MS-SSIM and PSNR over image pairs on the MI355X: ``ops.ssim_u8`` and what quality.py builds on it against the numpy
restatement (tests/ssim_refs.py: plain slicing) at the launch edges.

The tolerance on a stats entry is derived, not tuned: u = 2^-53; a moment is two K-term dot products with positive weights that sum to 1
over values <= 255^2, so |d moment| <= gamma 255^2 with gamma = (2 K + 2) u; through lum (denominator >= c1 = k1^2 255^2) that is
|d lum| <= 8 gamma / k1^2, through cs (denominator >= c2) |d cs| <= 12 gamma / k2^2, and with |lum|, |cs| <= 1
|d ssim| <= (8 / k1^2 + 12 / k2^2) (2 K + 2) 2^-53: 2.5e-10 at K = 11, 1.7e-10 at K = 7; the means inherit it.  The tests assert TWICE this
bound (``ssim_refs.tolerance``), the slack covering numpy's own error and the device's FMA contraction, and print max error / bound with
that asserted bound as the denominator: every printed figure must stay at or below 1.
MS-SSIM goes through a power: it is compared at the relative tolerance ``tolerance / max(clamped base over the levels)``; the inputs of
those comparisons keep every base away from 0.  ``sse``, ``duplicates``, pair tables and every device-to-device comparison are exact."""
import importlib

import numpy as np
import pytest
import torch

import ema_refs
import ssim_refs as SS

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None

SHAPES = [(1, 16, 11, 1.5, 1), (3, 16, 7, 1.5, 2), (1, 32, 11, 1.5, 2), (3, 64, 11, 1.5, 3), (4, 64, 3, 1.5, 5), (2, 32, 5, None, 3)]   # C, H, K, sigma, L
KINDS = ["uniform", "pink", "four", "flat", "negative"]
PAIRS = [[0, 0], [1, 1], [2, 2], [0, 2], [2, 1]]
_CACHE = {}


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _table(pairs):
    return _dev(np.asarray(pairs, np.int32).reshape(-1, 2))


def _sets(C, H):
    """the image kinds of one shape, drawn once"""
    if (C, H) not in _CACHE:
        _CACHE[C, H] = SS.image_sets(np.random.RandomState(100 * H + C), 3, C, H)
    return _CACHE[C, H]


def _call(a, b, pairs, K=11, sigma=1.5, L=None, flag=None):
    return eg.ops.ssim_u8(_dev(a), _dev(b), _table(pairs), window=eg.ops.ssim_window(K, sigma), levels=L, flag=flag)


def _ratio(got, ref, K):
    return float(np.abs(got.cpu().numpy() - ref).max() / SS.tolerance(K))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C, H, K, sigma, L", SHAPES)
def test_stats_and_sse_against_numpy(C, H, K, sigma, L, kind):
    a, b = _sets(C, H)[kind]
    assert eg.ops.ssim_levels(H, K) == L
    stats, sse = _call(a, b, PAIRS, K, sigma)
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (len(PAIRS), L, 2) and sse.dtype == torch.int64 and tuple(sse.shape) == (len(PAIRS),)
    ref, ref_sse = SS.stats(a, b, PAIRS, K, sigma, L)
    r = _ratio(stats, ref, K)
    print(f"ssim {kind} {(C, H, K, sigma, L)}: max error / bound = {r:.3e}")
    assert r <= 1.0
    assert np.array_equal(sse.cpu().numpy(), ref_sse)
    if kind == "negative":
        assert bool((stats[:3, 0, 0] < 0).all())
    # fewer levels: the same bits on the levels that remain
    if L > 1:
        assert torch.equal(_call(a, b, PAIRS, K, sigma, L - 1)[0], stats[:, :L - 1])


def test_pair_tables():
    C, H, K = 1, 32, 11
    rng = np.random.RandomState(5)
    a = np.concatenate((SS.pink(rng, 3, C, H), rng.randint(0, 256, (2, C, H, H)).astype(np.uint8)))            # 5 rows
    b = np.concatenate((SS.noisy(rng, a), rng.randint(0, 256, (4, C, H, H)).astype(np.uint8)))                # 9 rows
    pairs = np.stack((rng.randint(0, 5, 40), rng.randint(0, 9, 40)), 1)
    pairs[7] = pairs[19] = pairs[33] = (3, 8)                                # one pair at three places
    pairs[20:29, 0] = 2                                                      # one row used by many pairs
    pairs[20:29, 1] = np.arange(9)
    stats, sse = _call(a, b, pairs)
    ref, ref_sse = SS.stats(a, b, pairs)
    r = _ratio(stats, ref, K)
    print(f"ssim 5 rows against 9, 40 pairs: max error / bound = {r:.3e}")
    assert r <= 1.0 and np.array_equal(sse.cpu().numpy(), ref_sse)
    assert torch.equal(stats[7], stats[19]) and torch.equal(stats[7], stats[33]) and int(sse[7]) == int(sse[19]) == int(sse[33])
    sub = [3, 39, 11, 7]                                                     # a sub-table: the rows of the full table's result
    s2, e2 = _call(a, b, pairs[sub])
    assert torch.equal(s2, stats[sub]) and torch.equal(e2, sse[sub])
    s1, e1 = _call(a, b, pairs[5:6])                                         # P = 1
    assert tuple(s1.shape) == (1, 2, 2) and torch.equal(s1[0], stats[5]) and int(e1[0]) == int(sse[5])
    # self pairs, a is b
    x = _dev(a)
    idx = torch.arange(5, device=DEV, dtype=torch.int32)
    st, e = eg.ops.ssim_u8(x, x, torch.stack((idx, idx), 1).contiguous())
    assert bool((e == 0).all()) and float((st - 1.0).abs().max()) <= SS.tolerance(K)


def test_more_pairs_than_a_grid_dimension_of_65535():
    C, H, K, P = 1, 16, 11, 66000
    rng = np.random.RandomState(9)
    a = rng.randint(0, 256, (64, C, H, H)).astype(np.uint8)
    b = SS.noisy(rng, a, 60)
    pairs = rng.randint(0, 64, (P, 2))
    stats, sse = _call(a, b, pairs)
    ref, ref_sse = SS.stats(a, b, pairs)
    r = _ratio(stats, ref, K)
    print(f"ssim {P} pairs of {(C, H, H)}: max error / bound = {r:.3e}")
    assert r <= 1.0 and np.array_equal(sse.cpu().numpy(), ref_sse)
    s2, e2 = _call(a, b, pairs[P - 10:])
    assert torch.equal(s2, stats[P - 10:]) and torch.equal(e2, sse[P - 10:])


@pytest.mark.parametrize("bad", [(5, 0), (0, 9), (-1, 2), (2, -7), (2 ** 31 - 1, 0)])
def test_an_index_outside_its_set_is_flagged_and_nothing_else_moves(bad):
    C, H = 3, 16
    a, b = _sets(C, H)["uniform"]
    a, b = np.concatenate((a, a[:2])), np.concatenate((b, b, b))             # 5 and 9 rows
    pairs = np.array([[0, 0], [4, 8], [1, 3], [2, 2], [3, 7], [0, 5], [4, 4]])
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    good, good_sse = _call(a, b, pairs, 7, 1.5, None, flag)
    assert int(flag) == 0
    broken = pairs.copy()
    broken[3] = bad
    stats, sse = _call(a, b, broken, 7, 1.5, None, flag)
    assert int(flag) == eg.ops.SSIM_FLAG_PAIR == 2
    keep = [0, 1, 2, 4, 5, 6]
    assert bool(torch.isnan(stats[3]).all()) and int(sse[3]) == -1
    assert torch.equal(stats[keep], good[keep]) and torch.equal(sse[keep], good_sse[keep])


def test_wrapper_refusals():
    x = torch.zeros(4, 1, 16, 16, dtype=torch.uint8, device=DEV)
    pairs = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    for args, match in (((x, x, pairs.long()), "int32"), ((x, x, pairs[:, :1]), "int32"), ((x, torch.zeros(4, 1, 32, 32, dtype=torch.uint8, device=DEV), pairs), "one shape"),
                        ((torch.zeros(4, 5, 16, 16, dtype=torch.uint8, device=DEV),) * 2 + (pairs,), "channels"),
                        ((torch.zeros(4, 1, 24, 24, dtype=torch.uint8, device=DEV),) * 2 + (pairs,), "side")):
        with pytest.raises(ValueError, match=match):
            eg.ops.ssim_u8(*args)
    with pytest.raises(ValueError, match="levels"):
        eg.ops.ssim_u8(x, x, pairs, levels=2)
    with pytest.raises(ValueError, match="odd number of taps"):
        eg.ops.ssim_u8(x, x, pairs, window=np.full(4, 0.25))
    with pytest.raises(ValueError, match="positive and finite"):
        eg.ops.ssim_u8(x, x, pairs, k1=0.0)
    with pytest.raises(ValueError, match="one size"):
        eg.quality.ssim(x, x[:3])
    with pytest.raises(ValueError, match="n >= 2|2 <= n"):
        eg.quality.pair_table(1, 4)
    assert eg.ops.ssim_window_table(11, 1.5, DEV) is eg.ops.ssim_window_table(11, 1.5, DEV)                    # cached per (K, sigma, device)


@pytest.mark.parametrize("C, H, K", [(1, 32, 11), (3, 64, 11), (3, 16, 7)])
def test_quality_scores_against_numpy(C, H, K):
    rng = np.random.RandomState(H + C)
    a = SS.related(rng, 3, C, H)                                             # the cross pairs of PAIRS too keep their bases away from 0
    b = SS.noisy(rng, a)
    L = SS.levels(H, K)
    ref, ref_sse = SS.stats(a, b, PAIRS, K, 1.5, L)
    ua, ub, table = _dev(a), _dev(b), _table(PAIRS)
    fa, fb = eg.quality.real_images("celeba", ua, 3), eg.quality.real_images("celeba", ub, 3)               # floats in [-1, 1] of those bytes
    assert fa.dtype == torch.float32 and torch.equal(eg.quality.to_u8(fa), ua)
    tol = SS.tolerance(K)
    for x, y in ((ua, ub), (fa, fb)):
        s = eg.quality.ssim(x, y, table, window=K)
        m = eg.quality.ms_ssim(x, y, table, window=K)
        p = eg.quality.psnr(x, y, table)
        assert s.dtype == m.dtype == p.dtype == torch.float64 and tuple(s.shape) == tuple(m.shape) == tuple(p.shape) == (len(PAIRS),)
        if x is ua:
            first = (s, m, p)
        else:
            assert all(torch.equal(u, v) for u, v in zip(first, (s, m, p)))                                   # float and uint8 inputs: the same bits
    s, m, p = (t.cpu().numpy() for t in first)
    want = SS.ms_ssim(ref)
    assert SS.bases(ref).min() > 1e-6
    rs, rm = np.abs(s - ref[:, 0, 0]).max() / tol, (np.abs(m - want) / (want * SS.ms_ssim_rtol(ref, K))).max()
    print(f"quality {(C, H, K)}: ssim max error / bound = {rs:.3e}; ms_ssim max relative error / rtol = {rm:.3e}")
    assert rs <= 1.0 and rm <= 1.0
    assert np.allclose(p, SS.psnr(ref_sse, C * H * H), rtol=1e-14, atol=0)
    # without a table: row i against row i; explicit levels and weights
    assert torch.equal(eg.quality.ssim(ua, ub, window=K), eg.quality.ssim(ua, ub, _table([[0, 0], [1, 1], [2, 2]]), window=K))
    one = eg.quality.ms_ssim(ua, ub, table, levels=1, window=K)
    assert torch.equal(one, eg.quality.ssim(ua, ub, table, window=K).clamp_min(0.0))                          # L = 1: weight 1
    assert bool(torch.isinf(eg.quality.psnr(ua, ua)).all())
    if L >= 2:
        own = eg.quality.ms_ssim(ua, ub, table, levels=2, weights=(0.25, 0.75), window=K).cpu().numpy()
        want2 = SS.ms_ssim(ref[:, :2], (0.25, 0.75)) if L == 2 else SS.ms_ssim(SS.stats(a, b, PAIRS, K, 1.5, 2)[0], (0.25, 0.75))
        assert np.all(np.abs(own - want2) <= want2 * SS.ms_ssim_rtol(ref[:, :2], K))


def test_reconstruction():
    C, H, K = 3, 64, 11
    a, b = _sets(C, H)["pink"]
    ua, ub = _dev(a), _dev(b)
    tol = SS.tolerance(K)
    same = eg.quality.reconstruction(ua, ua)
    assert sorted(same) == ["levels", "ms_ssim", "mse", "psnr", "ssim"] and same["levels"] == 3
    assert same["psnr"] == float("inf") and same["mse"] == 0.0 and abs(same["ssim"] - 1.0) <= tol and abs(same["ms_ssim"] - 1.0) <= tol
    idx = np.stack((np.arange(3), np.arange(3)), 1)
    ref, ref_sse = SS.stats(a, b, idx)
    got, p, s, m = eg.quality.reconstruction(ua, ub, terms=True)
    mse = float(np.mean(ref_sse / (C * H * H)))
    want = SS.ms_ssim(ref)
    assert abs(got["mse"] - mse) <= 1e-12 * mse and abs(got["psnr"] - 10.0 * np.log10(255.0 ** 2 / mse)) <= 1e-12
    r = abs(got["ssim"] - ref[:, 0, 0].mean()) / tol
    print(f"reconstruction {(C, H)}: mean ssim error / bound = {r:.3e}; {got}")
    assert r <= 1.0 and abs(got["ms_ssim"] - want.mean()) <= float((want * SS.ms_ssim_rtol(ref, K)).max())
    assert torch.equal(s, eg.quality.ssim(ua, ub)) and torch.equal(m, eg.quality.ms_ssim(ua, ub)) and torch.equal(p, eg.quality.psnr(ua, ub))
    assert got == eg.quality.reconstruction(eg.quality.real_images("celeba", ua, 3), ub)


def test_diversity():
    C, H, K, N = 1, 32, 11, 64
    rng = np.random.RandomState(21)
    pink = SS.related(rng, N, C, H)                                          # 1/f images that share a half: every pair's cs stays above 0
    tol = SS.tolerance(K)
    copies = eg.quality.diversity(_dev(np.repeat(pink[:1], N, 0)), n_pairs=256, seed=3)
    assert sorted(copies) == ["duplicates", "levels", "ms_ssim", "pairs", "ssim"] and copies["levels"] == 2
    assert abs(copies["ms_ssim"] - 1.0) <= tol and abs(copies["ssim"] - 1.0) <= tol and copies["duplicates"] == copies["pairs"] == 256
    x = _dev(pink)
    got, pairs, m, s, sse = eg.quality.diversity(x, n_pairs=256, seed=3, terms=True)
    assert got["ms_ssim"] < copies["ms_ssim"] - 0.1 and got["duplicates"] == 0 and got["pairs"] == 256
    assert got == eg.quality.diversity(x, n_pairs=256, seed=3)                                                # the same seed: the same bits
    table = eg.quality.pair_table(N, 256, 3, DEV)
    assert torch.equal(pairs, table) and not torch.equal(table, eg.quality.pair_table(N, 256, 4, DEV))
    ri, rj = eg.quality.pair_draws(256, 3, N, N - 1, DEV)
    host = table.cpu().numpy()
    assert np.array_equal(host, SS.pair_table_from_draws(ri.cpu().numpy(), rj.cpu().numpy()))
    assert host.dtype == np.int32 and np.all(host[:, 0] != host[:, 1]) and host.min() >= 0 and host.max() < N and len(set(host[:, 0])) > N // 2
    ref, ref_sse = SS.stats(pink, pink, host)
    want = SS.ms_ssim(ref)
    assert SS.bases(ref).min() > 1e-6
    assert np.all(np.abs(m.cpu().numpy() - want) <= want * SS.ms_ssim_rtol(ref, K)) and np.array_equal(sse.cpu().numpy(), ref_sse)
    assert abs(got["ms_ssim"] - want.mean()) <= float((want * SS.ms_ssim_rtol(ref, K)).max()) and abs(got["ssim"] - ref[:, 0, 0].mean()) <= tol
    assert got == eg.quality.diversity(x, pairs=table)                                                        # an explicit table overrides the draw
    with pytest.raises(ValueError, match="outside its set"):
        eg.quality.diversity(x, pairs=_table([[0, 1], [2, N]]))
    # pairs inside classes: 4 classes of unequal size
    labels = np.array([0] * 30 + [1] * 2 + [2] * 21 + [3] * 11)
    labels = labels[rng.permutation(N)]
    lab = _dev(labels.astype(np.int64))
    got, pairs, m, s, sse = eg.quality.diversity(x, n_pairs=202, seed=8, labels=lab, n_classes=4, terms=True)
    host = pairs.cpu().numpy()
    k = np.arange(202) % 4
    assert np.array_equal(labels[host[:, 0]], k) and np.array_equal(labels[host[:, 1]], k) and np.all(host[:, 0] != host[:, 1])
    assert sorted(got) == ["by_class", "duplicates", "levels", "ms_ssim", "pairs", "ssim"] and len(got["by_class"]) == 4 and got["duplicates"] == 0
    assert all(len(set(host[k == c, 0])) > 1 for c in range(4))
    ref, _ = SS.stats(pink, pink, host)
    want = SS.ms_ssim(ref)
    rtol = float(SS.ms_ssim_rtol(ref, K).max())
    for c in range(4):
        assert abs(got["by_class"][c] - want[k == c].mean()) <= rtol * want[k == c].max()
    assert torch.equal(pairs, eg.quality.class_pair_table(lab, 4, 202, 8)[0])
    lonely = labels.copy()
    lonely[0] = 4                                                            # a fifth class with one row
    with pytest.raises(ValueError, match="fewer than 2 images"):
        eg.quality.diversity(x, n_pairs=64, seed=8, labels=_dev(lonely.astype(np.int64)), n_classes=5)


def test_diversity_generator_and_projection_quality():
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=1)
    got = eg.quality.diversity_generator("mnist", tr.G, inp, n_images=16, n_pairs=32, batch=8, seed=5)
    assert sorted(got) == ["fake", "gap", "real"]
    real = eg.quality.real_images("mnist", inp, 16)
    assert got["real"] == eg.quality.diversity(real, n_pairs=32, seed=5)                                      # bit for bit: one pair table
    fake = eg.quality.generate("mnist", tr.G, 16, 8, seed=5)
    assert got["fake"] == eg.quality.diversity(fake, n_pairs=32, seed=5) and got["gap"] == got["fake"]["ms_ssim"] - got["real"]["ms_ssim"]
    assert sorted(got["fake"]) == ["duplicates", "levels", "ms_ssim", "pairs", "ssim"] and got["fake"]["levels"] == 2 and got["fake"]["pairs"] == 32
    with pytest.raises(ValueError, match="sprite workloads"):
        eg.quality.diversity_generator("dsprites", tr.G, inp)
    G = tr.G.eval()
    target = real[:4]
    labels = torch.eye(int(G.n_classes), device=DEV)[:4].contiguous()
    out = eg.quality.projection_quality("mnist", G, target, labels, steps=2, lr=0.05)
    assert sorted(out) == ["levels", "loss", "ms_ssim", "mse", "psnr", "ssim"] and out["levels"] == 2
    assert all(np.isfinite(out[key]) for key in ("loss", "ms_ssim", "mse", "psnr", "ssim")) and out["mse"] > 0
    noise, onehot, code, losses = eg.sampling.project_images("mnist", G, target, labels, 2, 0.05)
    assert out["loss"] == float(losses[-1].double().mean())
    with torch.no_grad():
        image = G(noise, onehot, code)
    again = eg.quality.reconstruction(target, image)
    assert all(out[key] == again[key] for key in again)
    tr.G.train()

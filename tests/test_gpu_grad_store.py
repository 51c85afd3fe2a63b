"""Gradients are written once: every kernel that writes a parameter gradient has a store mode (out = x) beside the accumulate mode
(out += x), and CelebATrainer's backward passes store, so the iteration neither clears its gradient arenas nor reads the zeros.

1. kernel level: store into a NaN-filled slot == accumulate into a zero-filled slot (equal after adding 0.0, which folds -0.0), no NaN
   left in the written region, sentinels at both ends of it untouched;
2. trainer level: one eager iteration with both arenas poisoned with NaN in front of every backward pass is the iteration as shipped;
3. a captured graph replayed 3 times is 3 eager iterations."""
import importlib

import numpy as np
import pytest
import torch

from oracle import celeba_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None
ops = None
PAD = 64            # sentinel floats in front of and behind every gradient slot
SENT = 12345.0


def setup_module(module):
    global eg, ops
    eg = importlib.import_module("ead-gan_amd")
    ops = eg.ops
    torch.set_num_threads(16)


def rnd(*shape, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).to(dtype).contiguous()


def both_modes(sizes, launch):
    """launch(slots, accumulate) writes the gradient slots (views of ``sizes`` floats, each between two sentinel rows); run once accumulating
    into zeros and once storing into NaN -> the accumulate-mode results (the store-mode ones have been checked against them)"""
    res = {}
    for acc in (True, False):
        bufs = [torch.full((n + 2 * PAD,), SENT, device=DEV) for n in sizes]
        slots = [b[PAD:PAD + n] for b, n in zip(bufs, sizes)]
        for s in slots:
            s.fill_(0.0 if acc else float("nan"))
        launch(slots, acc)
        torch.cuda.synchronize()
        for b, n in zip(bufs, sizes):
            assert bool((b[:PAD] == SENT).all()) and bool((b[PAD + n:] == SENT).all()), "bytes outside the gradient slot were written"
        res[acc] = [s.clone() for s in slots]
    for a, b in zip(res[True], res[False]):
        assert not torch.isnan(b).any(), "the store mode left part of the slot unwritten (or read it)"
        assert torch.equal(a + 0.0, b + 0.0)
        assert float(a.abs().max()) > 0.0           # the launch did write something
    return res[True]


# Cout x Cin x taps, splits: the lean reduce (< 16 splits), the wide one, a ragged channel count (48) with many splits -- these three run the
# scalar loops (fewer than 64 channels per block); then full 64-channel blocks: the lean float4 loop, the wide kernel's split groups
# (1024 threads) and its float4 loop (a tile of 64 taps leaves no room for split groups)
REDUCE_CASES = [(32, 32, 16, 2), (32, 32, 16, 16), (128, 48, 16, 128), (64, 64, 16, 2), (64, 64, 16, 16), (4, 64, 64, 16)]


@pytest.mark.parametrize("N,C,T,ns", REDUCE_CASES)
def test_wgrad_reduce_store(N, C, T, ns):
    slab = rnd(ns, N, T, C, seed=1)
    got, = both_modes([N * C * T], lambda g, acc: ops.wgrad_reduce(slab, ns, N, N, C, T, g[0], accumulate=acc))
    want = slab.sum(0).permute(0, 2, 1).reshape(-1)            # [n][c][t]
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


@pytest.mark.parametrize("N,C,T,ns", REDUCE_CASES)
def test_wgrad_reduce_rank1_store_three_tapes(N, C, T, ns):
    slab = rnd(ns, N, T, C, seed=2)
    coef, u, v = rnd(4, seed=3), rnd(3, N, seed=4), rnd(3, C * T, seed=5)
    got, = both_modes([N * C * T], lambda g, acc: ops.wgrad_reduce_rank1(slab, ns, N, N, C, T, g[0], 3, coef, u, v, accumulate=acc))
    want = slab.sum(0).permute(0, 2, 1).reshape(N, C * T) - torch.einsum("q,qn,qk->nk", coef[:3], u, v)
    torch.testing.assert_close(got, want.reshape(-1), rtol=1e-4, atol=1e-5 * float(want.abs().max()))


@pytest.mark.parametrize("ns", [2, 16])
def test_wgrad_reduce_perm_store(ns):
    """slab row n -> gradient row (n % 4) * 8 + n // 4, destination rows of 24 of the slab's 32 (zero padded) channels"""
    N, C, T, crow = 32, 32, 16, 24
    slab = rnd(ns, N, T, C, seed=6)
    got, = both_modes([N * crow * T], lambda g, acc: ops.wgrad_reduce_perm(slab, ns, N, N, C, T, g[0], 4, 8, crow, accumulate=acc))
    rows = slab.sum(0)[:, :, :crow].permute(0, 2, 1)            # [n][c][t]
    want = torch.empty_like(rows)
    for n in range(N):
        want[(n % 4) * 8 + n // 4] = rows[n]
    torch.testing.assert_close(got, want.reshape(-1), rtol=1e-5, atol=1e-5 * float(want.abs().max()))


def test_wgrad_reduce_sn_store():
    Cout, Cin, k, ns = 32, 48, 4, 3
    c = ops.make_conv(2, 8, 8, Cin, Cout, k, 2, 1)
    slab = rnd(ns, Cout, k * k, Cin, seed=7)
    w, u, v = rnd(Cout * Cin * k * k, seed=8), rnd(Cout, seed=9), rnd(Cin * k * k, seed=10)
    sigma = torch.tensor([1.3], device=DEV)
    gtmp = torch.empty(Cout * Cin * k * k, device=DEV)
    part = torch.empty(ops.sn_partials(), device=DEV)
    both_modes([Cout * Cin * k * k], lambda g, acc: ops.wgrad_reduce_sn(c, slab, ns, w, sigma, u, v, gtmp, part, g[0], accumulate=acc))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bias_grad_store(dtype):
    dt = eg.engine.parse_dtype(dtype)
    rows, N = 300, 64
    dy = rnd(rows, N, seed=11, dtype=ops.torch_dtype(dt))
    part = torch.empty(ops.bias_grad_ws_floats(rows, N), device=DEV)
    got, = both_modes([N], lambda g, acc: ops.bias_grad(dt, dy, rows, N, part, g[0], accumulate=acc))
    torch.testing.assert_close(got, dy.float().sum(0), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bias_grad_sn_store(dtype):
    dt = eg.engine.parse_dtype(dtype)
    T, rpt, N = 3, 96, 64
    rows = T * rpt
    dzs, a = rnd(rows, N, seed=12, dtype=ops.torch_dtype(dt)), rnd(rows, N, seed=13, dtype=ops.torch_dtype(dt))
    bias, sigma = rnd(N, seed=14), torch.tensor([1.1, 0.9, 1.7], device=DEV)
    ws = torch.empty(ops.bias_grad_sn_ws_floats(rows, N, rpt), device=DEV)
    coef = torch.zeros(4, device=DEV)
    got, = both_modes([N], lambda g, acc: ops.bias_grad_sn(dt, dzs, a, bias, rows, N, rpt, sigma, 0.1, ws, g[0], coef, accumulate=acc))
    want = (dzs.float().reshape(T, rpt, N).sum(1) * sigma[:, None]).sum(0)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("N,nrb,tiles_m", [(128, 16, 4), (32, 1024, 256)])           # one wave per sum / one workgroup per sum (>= 1024 row blocks)
def test_bias_grad_sn_fused_store(N, nrb, tiles_m):
    T = 2
    stat = rnd(N * nrb + nrb * max(N // 128, 1), seed=15)
    sigma = torch.tensor([1.1, 0.9], device=DEV)
    coef = torch.zeros(4, device=DEV)
    got, = both_modes([N], lambda g, acc: ops.bias_grad_sn_fused(stat, nrb, N, tiles_m, tiles_m // T, T, sigma, g[0], coef, accumulate=acc))
    tape = (torch.arange(nrb, device=DEV) % tiles_m) // (tiles_m // T)
    want = (stat[:N * nrb].reshape(N, nrb) * sigma[tape][None, :]).sum(1)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))


def _bn_inputs(M, C, dt):
    tdt = ops.torch_dtype(dt)
    z, da = rnd(M, C, seed=16, dtype=tdt), rnd(M, C, seed=17, dtype=tdt)
    gamma, beta = rnd(C, seed=18), rnd(C, seed=19)
    mean, istd = rnd(C, seed=20) * 0.1, rnd(C, seed=21).abs() + 0.5
    return z, da, gamma, beta, mean, istd


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bn_bwd_store(dtype):
    dt = eg.engine.parse_dtype(dtype)
    M, C = 300, 32
    z, da, gamma, beta, mean, istd = _bn_inputs(M, C, dt)
    ws, sums, dz = torch.empty(ops.bn_ws_floats(M, C), device=DEV), torch.empty(2 * C, device=DEV), torch.empty_like(z)
    dg, db = both_modes([C, C], lambda g, acc: ops.bn_bwd(dt, z, da, dz, M, C, gamma, beta, mean, istd, ops.ACT_RELU, 0.0, g[0], g[1], sums, ws,
                                                          accumulate=acc))
    assert torch.equal(dg, sums[C:]) and torch.equal(db, sums[:C])
    both_modes([C, C], lambda g, acc: ops.bn_bwd_sums_local(dt, z, da, M, C, gamma, beta, mean, istd, ops.ACT_RELU, 0.0, g[0], g[1], sums, ws,
                                                            accumulate=acc))


@pytest.mark.parametrize("nrb", [8, 1024])                      # one wave per channel / one workgroup per channel
def test_bn_bwd_fused_store(nrb):
    dt = ops.EG_BF16
    M, C = 256, 32
    z, dy, gamma, beta, mean, istd = _bn_inputs(M, C, dt)
    stat = rnd(2 * C * nrb, seed=22)
    ws, sums, dz = torch.empty(ops.bn_ws_floats(M, C), device=DEV), torch.empty(2 * C, device=DEV), torch.empty_like(z)
    dg, db = both_modes([C, C], lambda g, acc: ops.bn_bwd_fused(dt, z, dy, dz, M, C, stat, nrb, gamma, beta, mean, istd, g[0], g[1], sums, ws,
                                                                accumulate=acc))
    want = stat.reshape(2, C, nrb).sum(2)
    torch.testing.assert_close(db, want[0], rtol=1e-4, atol=1e-4 * float(want.abs().max()))
    torch.testing.assert_close(dg, want[1], rtol=1e-4, atol=1e-4 * float(want.abs().max()))


def test_act_grad_mul_bias_nchw_store():
    B, C, HW = 5, 3, 4096
    a, gr = torch.tanh(rnd(B, C, HW, seed=23)), rnd(B, C, HW, seed=24)
    out, part = torch.empty(B, C, HW, device=DEV), torch.empty(B * C, device=DEV)
    got, = both_modes([C], lambda g, acc: ops.act_grad_mul_bias_nchw(gr, a, out, B, C, HW, ops.ACT_TANH, 0.0, part, g[0], accumulate=acc))
    torch.testing.assert_close(got, (gr * (1 - a * a)).sum((0, 2)), rtol=1e-4, atol=1e-3)


def test_dense_small_bgrad_store():
    B, N = 24, 19
    dy = rnd(B, N, seed=25)
    got, = both_modes([N], lambda g, acc: ops.dense_small_bgrad(dy, g[0], B, N, accumulate=acc))
    torch.testing.assert_close(got, dy.sum(0), rtol=1e-5, atol=1e-5)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------
B = 8               # the smallest batch of the CelebA trainer tests


def build_trainer(seed, dtype, **kw):
    orc = co.CelebAOracle(seed=seed)
    G = eg.celeba.Generator(dtype=dtype).to(DEV)
    D = eg.celeba.Discriminator(dtype=dtype).to(DEV)
    G.load_state_dict({k: v.detach() for k, v in orc.G.items()})
    D.load_state_dict({k: v.detach() for k, v in orc.D.items()})
    return G, D, eg.celeba.CelebATrainer(G, D, B, dtype=dtype, **kw)


def trainer_state(G, D, tr):
    ts = [G.arena.flat, D.arena.flat, tr.mG, tr.vG, tr.mD, tr.vD, tr.miG, tr.viG, tr.miD, tr.viD, G.arena.grad, D.arena.grad]
    return [t.clone() for t in ts] + [tr.steps.clone()]


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_iteration_with_poisoned_arenas_is_the_iteration(dtype, overlap):
    """Both gradient arenas are filled with NaN in front of each of the three backward passes: losses, parameters, Adam moments and the
    gradients left behind equal those of the plain iteration -> every slot an optimizer reads was stored by that pass."""
    def run(poison):
        G, D, tr = build_trainer(21, dtype, overlap=overlap)
        if poison:
            def hook(k):
                G.arena.grad.fill_(float("nan"))
                D.arena.grad.fill_(float("nan"))
                hook.calls.append(k)
            hook.calls = []
            tr.before_backward = hook
        rng = np.random.RandomState(4)
        z, code, labels = co.draw_step_inputs(rng, B)
        tr.load_inputs(co.synthetic_real(B, seed=9).to(DEV), z.to(DEV), code.to(DEV), labels.to(DEV))
        losses = tr.step_resident().clone()
        torch.cuda.synchronize()
        assert not poison or hook.calls == [1, 2, 3]
        return [losses] + trainer_state(G, D, tr)

    a, b = run(False), run(True)
    assert torch.isfinite(a[0][:3]).all()
    for x, y in zip(a, b):
        assert torch.equal(x + 0, y + 0)
    # D's gradients are those of the info step, G's too: nothing was left cleared
    assert float(a[-2].abs().max()) > 0 and float(a[-3].abs().max()) > 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_captured_replay_equals_eager(dtype):
    """one eager iteration, then 3 more / capture and 3 replays: the same losses and the same state, bit for bit"""
    def run(capture):
        G, D, tr = build_trainer(22, dtype)
        rng = np.random.RandomState(5)
        real = co.synthetic_real(B, seed=10).to(DEV)
        out = []
        for i in range(4):
            z, code, labels = co.draw_step_inputs(rng, B)
            tr.load_inputs(real, z.to(DEV), code.to(DEV), labels.to(DEV))
            if capture and i == 1:
                tr.capture()
            out.append(tr.step_resident().clone())
        torch.cuda.synchronize()
        return [torch.stack(out)] + trainer_state(G, D, tr)

    a, b = run(False), run(True)
    assert torch.isfinite(a[0][:, :3]).all()
    for x, y in zip(a, b):
        assert torch.equal(x, y)

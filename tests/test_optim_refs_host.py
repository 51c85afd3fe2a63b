"""Host side of tests/test_gpu_optim_lane.py: the float64 restatements of tests/optim_refs.py are what torch computes (torch.optim.Adam,
torch.nn.utils.spectral_norm, a naive gather for the panels); for every case the float32 yardstick is measured, and each mutant a case
declares misses float64 by at least ``MUTANT_FACTOR * K`` yardsticks -- so a kernel with that mistake cannot pass the GPU test's bound."""
import pytest
import torch

import optim_refs as R

F64 = torch.float64


# ---- the restatements are torch's semantics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [R.BETAS, R.BETAS_TORCH])
@pytest.mark.parametrize("t0", [0, 4])
def test_adam_restatement_equals_torch_optim_adam(t0, betas):
    c = R.adam_inputs(257, t0)
    lr, b1, b2, eps = (R.f32(x) for x in (R.LR, betas[0], betas[1], R.EPS))
    p = c["p"].to(F64).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    if t0:
        opt.state[p] = dict(step=torch.tensor(float(t0)), exp_avg=c["m"].to(F64).clone(), exp_avg_sq=c["v"].to(F64).clone())
    for k in range(c["g"].shape[0]):
        p.grad = c["g"][k].to(F64).clone()
        opt.step()
    got = R.adam(c["p"], c["g"], c["m"], c["v"], t0, c["g"].shape[0], R.LR, betas[0], betas[1], R.EPS)
    st = opt.state[p]
    assert int(st["step"]) == t0 + c["g"].shape[0]
    for a, b in zip(got, (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
        assert R.dist(a, b) < 1e-13


@pytest.mark.parametrize("case", [(7, 255), (17, 9), (1, 257)])
def test_power_iter_restatement_equals_torch_spectral_norm(case):
    Rr, Kd = case
    torch.manual_seed(3)
    m = torch.nn.utils.spectral_norm(torch.nn.Linear(Kd, Rr, bias=False).double(), eps=R.SN_EPS)
    W, u, v = m.weight_orig.detach().clone(), m.weight_u.clone(), m.weight_v.clone()
    x = torch.zeros(1, Kd, dtype=F64)
    for _ in range(2):
        m.train()
        m(x)                                           # one power iteration
        u, v, sigma = R.power_iter(W, u, v, R.SN_EPS, True)
        assert R.dist(u, m.weight_u) < 1e-13 and R.dist(v, m.weight_v) < 1e-13
        assert R.dist(W / sigma, m.weight.detach()) < 1e-13
    m.eval()
    m(x)
    ue, ve, sigma = R.power_iter(W, u, v, R.SN_EPS, False)
    assert torch.equal(ue, m.weight_u) and torch.equal(ve, m.weight_v)
    assert R.dist(W / sigma, m.weight.detach()) < 1e-13


def test_panel_closed_forms_equal_a_naive_gather():
    Cout, Cin, T = 3, 5, 4
    w = torch.arange(Cout * Cin * T, dtype=torch.float32)
    wp = R.fwd_panel(w, Cout, Cin, T)
    assert wp.shape == (Cout, T * Cin)
    for n in range(Cout):
        for c in range(Cin):
            for t in range(T):
                assert wp[n, t * Cin + c] == w[(n * Cin + c) * T + t]
    Kr, n_mod, n_mul, Kpad = 3, 4, 2, 8
    N = n_mod * n_mul
    w = 1 + torch.arange(Kr * N, dtype=torch.float32)
    wp = R.rows_panel(w, Kr, N, Kpad, n_mod, n_mul)
    assert wp.shape == (N, Kpad) and bool((wp[:, Kr:] == 0).all())
    for n in range(N):
        for k in range(Kr):
            assert wp[(n % n_mod) * n_mul + n // n_mod, k] == w[k * N + n]
    assert sorted(wp[:, :Kr].flatten().tolist()) == w.tolist()          # a permutation: every row of the panel is written


# ---- yardsticks and mutants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ADAM_HOST_CASES, ids=lambda c: f"t{c[0]}-{'x'.join(f'{s:g}' for s in c[1])}-b{c[2][0]}")
def test_adam_yardstick_and_mutants(case):
    t0, scales, betas = case
    c = R.adam_case(R.ADAM_HOST_N, t0, scales, betas)
    yard = c["yard"]
    print(f"adam t0={t0} scales={scales} betas={betas}: float32 yardstick {yard:.3g}")
    assert 0 < yard < 1e-6, yard
    for mut in R.adam_mutants(t0, scales, betas):
        got = R.adam(c["p"], c["g"], c["m"], c["v"], t0, len(scales), R.LR, betas[0], betas[1], R.EPS, mutant=mut)
        ratio = max(R.dist(a, b) for a, b in zip(got, c["want"])) / (R.K * yard)
        print(f"  mutant {mut}: error / bound = {ratio:.3g}")
        assert ratio >= R.MUTANT_FACTOR, (case, mut, ratio)


@pytest.mark.parametrize("t0", R.ADAM_T0)
def test_every_flat_adam_length_has_a_yardstick(t0):
    """the lengths of the GPU test, one element included: float32 misses float64 by something, and by little"""
    for n in R.ADAM_LENGTHS:
        for betas in (R.BETAS, R.BETAS_TORCH):
            yard = R.adam_case(n, t0, R.GRAD_SCALES, betas)["yard"]
            print(f"adam n={n} t0={t0} betas={betas}: float32 yardstick {yard:.3g}")
            assert 0 < yard < 1e-6, (n, t0, yard)


@pytest.mark.parametrize("case", R.SN_CASES + (R.SN_EXTRA,))
def test_power_iter_yardstick_and_mutants(case):
    Rr, Kd = case
    c = R.sn_case(Rr, Kd)
    for it, (_, yard) in enumerate(c["train"]):
        print(f"power_iter {case} iteration {it}: float32 yardstick {yard:.3g}")
        assert 0 <= yard < 1e-5, yard
        assert yard > 0 or case == (1, 1)              # one element: u = v = +-1 and sigma = |w| exactly, in any precision
    print(f"power_iter {case} eval: float32 yardstick {c['eval'][1]:.3g}")
    assert c["eval"][1] < 1e-5
    want, yard = c["train"][0]
    for mut in R.sn_mutants(Rr, Kd):
        got = R.power_iter(c["W"], c["u"], c["v"], R.SN_EPS, True, mutant=mut)
        ratio = R.sn_yardstick(got, want) / (R.K * yard)
        print(f"  mutant {mut}: error / bound = {ratio:.3g}")
        assert ratio >= R.MUTANT_FACTOR, (case, mut, ratio)


def test_power_iter_of_a_zero_matrix_is_zero():
    u, v, sigma = R.power_iter(torch.zeros(8, 16), *R.sn_inputs(8, 16)[1:], R.SN_EPS, True)
    assert not u.any() and not v.any() and sigma == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_fused_pack_yardsticks(dtype):
    """the fused kernels' cases: the masters' yardstick, and the panel's -- the float32 restatement rounded through the panel dtype"""
    tdt = R.TORCH_DTYPE[dtype]
    unit = {"f32": 2.0 ** -24, "bf16": 2.0 ** -9, "f16": 2.0 ** -11}[dtype]
    for seed, (Cout, Cin, k, _, _) in enumerate(R.CONV_LAYERS + (R.CONV_LAYER_MAYBE,)):
        c = R.pack_case(Cout * Cin * k * k, seed)
        p32 = R.adam(c["p"], c["g"], c["m"], c["v"], 0, 2, R.LR, *R.BETAS, R.EPS, dtype=torch.float32)[0]
        yard_p = R.dist(R.fwd_panel(p32, Cout, Cin, k * k).to(tdt).float(), R.fwd_panel(c["want"][0], Cout, Cin, k * k))
        print(f"adam_pack_conv {(Cout, Cin, k)} {dtype}: masters {c['yard']:.3g}, forward panel {yard_p:.3g}")
        assert 0 < c["yard"] < 1e-6 and 0 < yard_p <= 2 * unit + c["yard"]
    for seed, (Kr, Cout) in enumerate(R.ROWS_CASES):
        N = 16 * Cout
        c = R.pack_case(Kr * N, 100 + seed)
        p32 = R.adam(c["p"], c["g"], c["m"], c["v"], 0, 2, R.LR, *R.BETAS, R.EPS, dtype=torch.float32)[0]
        Kpad = (Kr + 63) // 64 * 64
        yard_p = R.dist(R.rows_panel(p32, Kr, N, Kpad, 16, Cout).to(tdt).float(), R.rows_panel(c["want"][0], Kr, N, Kpad, 16, Cout))
        print(f"adam_pack_rows {(Kr, Cout)} {dtype}: masters {c['yard']:.3g}, panel {yard_p:.3g}")
        assert 0 < c["yard"] < 1e-6 and 0 < yard_p <= 2 * unit + c["yard"]

"""Input gradients of the generators on the MI355X against float64 (tests/input_grad_refs.py): the two kernels (eg_linear_dinput,
eg_bn_bwd_eval) at their launch edges, the drop-in modules in train and eval mode, and sampling.project_images.

Kernel bounds follow the project's rule: a result may miss float64 (on operands pre-rounded to the compute dtype) by K = 8 times what
float32 torch on the CPU misses it by on the same operands; the figure and the bound are printed before they are compared."""
import importlib

import pytest
import torch

import input_grad_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")
    torch.set_num_threads(16)


def rel_err(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- eg_linear_dinput ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", R.LINEAR_CASES)
def test_linear_dinput_against_float64(case, dtype):
    B, NI, NJ, Kc = case
    c = R.linear_case(case, dtype)
    want = R.contraction(c["dH"], c["Wr"], NI, NJ, Kc, *c["strides"])
    yard = R.dist(R.contraction(c["dH"], c["Wr"], NI, NJ, Kc, *c["strides"], dtype=torch.float32), want)
    dt = eg.engine.parse_dtype(dtype)
    dH = c["dH"].to(R.TORCH_DTYPE[dtype]).to(DEV)
    W = c["W"].to(DEV)
    ws = torch.empty(max(1, eg.ops.linear_dinput_ws_floats(B, NI, NJ, Kc)), device=DEV)
    outs = []
    for _ in range(2):
        dX = torch.full((B, Kc), float("nan"), device=DEV)
        eg.ops.linear_dinput(dt, dH, NI * NJ, W, dX, B, NI, NJ, Kc, *c["strides"], ws)
        outs.append(dX)
    assert bool(torch.isfinite(outs[0]).all()), "an element of dX was not written"
    assert torch.equal(outs[0], outs[1])
    fig = R.dist(outs[0], want)
    print(f"linear_dinput {case} {dtype}: error {fig:.3g}, float32 yardstick {yard:.3g}, bound {R.K * yard:.3g}")
    assert fig <= R.K * yard, (case, dtype, fig, yard)


def test_linear_dinput_takes_a_row_stride():
    """dH rows inside a wider buffer (ldh > NI*NJ): the columns beyond the row are never read"""
    B, NI, NJ, Kc = 5, 3, 40, 9
    c = R.linear_case((B, NI, NJ, Kc), "f32")
    wide = torch.full((B, NI * NJ + 8), float("nan"), device=DEV)
    wide[:, :NI * NJ] = c["dH"].to(DEV)
    dX, ref = torch.empty(B, Kc, device=DEV), torch.empty(B, Kc, device=DEV)
    eg.ops.linear_dinput(0, wide, NI * NJ + 8, c["W"].to(DEV), dX, B, NI, NJ, Kc, *c["strides"], None)
    eg.ops.linear_dinput(0, c["dH"].to(DEV), NI * NJ, c["W"].to(DEV), ref, B, NI, NJ, Kc, *c["strides"], None)
    assert torch.equal(dX, ref)


# ---- eg_bn_bwd_eval -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", list(R.ACTS))
@pytest.mark.parametrize("case", R.BN_CASES)
def test_bn_bwd_eval_against_float64(case, name, dtype):
    M, C = case
    c = R.bn_case(case, dtype)
    tdt = R.TORCH_DTYPE[dtype]
    want, y64 = R.bn_eval_bwd(c, name)
    keep = R.bn_keep(y64, name)
    assert 1.0 - float(keep.float().mean()) <= R.EXCLUDE_CAP
    # the yardstick rounds its result to the dtype like the kernel's store does
    yard = R.dist(R.bn_eval_bwd(c, name, torch.float32)[0].to(tdt).float() * keep, want * keep)
    dev = lambda k: c[k].to(DEV)
    z, da = c["z"].to(tdt).to(DEV), c["da"].to(tdt).to(DEV)
    dz = torch.full((M, C), float("nan"), device=DEV, dtype=tdt)
    ws = torch.empty(2 * C, device=DEV)
    eg.ops.bn_bwd_eval(eg.engine.parse_dtype(dtype), z, da, dz, M, C, dev("gamma"), dev("beta"), c["eps"], dev("mean"), dev("var"), ws, R.ACTS[name], R.SLOPE)
    assert bool(torch.isfinite(dz).all())
    fig = R.dist(dz.float().cpu() * keep, want * keep)
    print(f"bn_bwd_eval {case} {name} {dtype}: error {fig:.3g}, yardstick {yard:.3g}, bound {R.K * yard:.3g}")
    assert fig <= R.K * yard, (case, name, dtype, fig, yard)


# ---- drop-in modules ----------------------------------------------------------------------------------------------------------------------
KINDS = ("celeba", "mnist", "dsprites", "colored")
PRE_BN_BIAS = {"celeba": ("conv_blocks.1.bias", "conv_blocks.4.bias", "conv_blocks.7.bias"),        # zero gradient up to rounding noise
               "mnist": ("l1.0.bias", "conv_blocks.2.bias", "conv_blocks.6.bias"),
               "dsprites": ("conv_block.0.bias", "conv_block.3.bias", "conv_block.6.bias"),
               "colored": ("conv_block.0.bias", "conv_block.3.bias", "conv_block.6.bias")}


def new_generator(kind, dtype="f32", seed=0):
    """a generator with default-initialised weights and running statistics moved off their initial (0, 1)"""
    torch.manual_seed(seed)
    G = {"celeba": lambda: eg.celeba.Generator(dtype=dtype), "mnist": lambda: eg.mnist.Generator(dtype=dtype),
         "dsprites": lambda: eg.dsprites.Generator(code_dim=4, n_classes=3, channels=1, dtype=dtype), "colored": lambda: eg.colored.Generator(dtype=dtype)}[kind]()
    g = torch.Generator().manual_seed(seed + 1)
    sd = G.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
    G.load_state_dict(sd)
    return G.to(DEV)


def state64(G, requires_grad=False):
    return {k: v.detach().double().cpu().clone().requires_grad_(requires_grad and v.is_floating_point() and "running" not in k)
            for k, v in G.state_dict().items()}


def engine_taps(kind, eng):
    """the engine's ReLU / LeakyReLU outputs in the layout of the float64 taps"""
    nchw = lambda t: t.permute(0, 3, 1, 2).float().cpu()
    if kind == "celeba":
        return [nchw(a) for a in eng.a]
    if kind == "mnist":
        return [nchw(eng.a1), nchw(eng.a2)]
    return [eng.a1.float().cpu(), nchw(eng.h).reshape(eng.B, -1)] + [nchw(a) for a in eng.a]


def count_flips(kind, eng, taps):
    return sum(int(((a > 0) != (t > 0)).sum()) for a, t in zip(engine_taps(kind, eng), taps))


def reference_pass(kind, G, inputs, dimg, training, params=False):
    """float64 autograd of the reference layer list -> (image, input gradients, {name: parameter gradient}, taps)"""
    sd = state64(G, params)
    leaves = [x.double().requires_grad_(True) for x in inputs]
    taps = []
    img = R.FORWARDS[kind](sd, leaves, training, taps)
    img.backward(dimg.double())
    return img.detach(), [x.grad for x in leaves], {k: v.grad for k, v in sd.items() if v.requires_grad}, taps


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("kind", KINDS)
def test_module_input_gradients_fp32(kind, mode):
    B = 8
    G = new_generator(kind)
    training = mode == "train"
    G.train(training)
    inputs = R.generator_case(kind, B, seed=3)
    leaves = [x.to(DEV).requires_grad_(True) for x in inputs]
    if not training:
        before = {k: v.clone() for k, v in G.state_dict().items()}
        plain = G(*[x.to(DEV) for x in inputs])
        assert plain.grad_fn is None and not plain.requires_grad            # without input leaves: today's no_grad path
        img = G(*leaves)
        with pytest.raises(NotImplementedError, match="requires_grad_"):     # parameters still require grad: refused, not a silent None
            img.backward(torch.ones_like(img))
        G.requires_grad_(False)
    img = G(*leaves)
    dimg = torch.randn(img.shape, generator=torch.Generator().manual_seed(1)) * 1e-3
    want_img, want_in, want_p, taps = reference_pass(kind, G, inputs, dimg, training, params=training)
    assert rel_err(img, want_img) < 2e-5
    img.backward(dimg.to(DEV))
    flips = count_flips(kind, G.engine(B), taps)
    assert flips <= 3, flips
    for x, w in zip(leaves, want_in):
        fig = rel_err(x.grad, w)
        print(f"{kind} {mode}: input gradient [{x.shape[1]}] rel_err {fig:.3g} (flips {flips})")
        assert fig < 1e-4 + 4e-3 * flips, (kind, mode, fig, flips)
    if training:
        # the parameter gradients of the same pass: those of a pass without input leaves, bit for bit
        first = {k: p.grad.clone() for k, p in G.named_parameters()}
        for k, p in G.named_parameters():
            if k not in PRE_BN_BIAS[kind]:
                assert rel_err(first[k], want_p[k]) < 1e-4 + 4e-3 * flips, k
            p.grad.zero_()
        G(*[x.to(DEV) for x in inputs]).backward(dimg.to(DEV))
        for k, p in G.named_parameters():
            assert torch.equal(p.grad, first[k]), k
    else:
        for k, v in G.state_dict().items():
            assert torch.equal(v, before[k]), k
        assert all(p.grad is None or not bool(p.grad.any()) for p in G.parameters())


@pytest.mark.parametrize("kind,dtype", [("celeba", "bf16"), ("mnist", "bf16"), ("dsprites", "bf16"), ("colored", "bf16"), ("colored", "f16")])
def test_module_input_gradients_16bit(kind, dtype):
    """train mode, one pass: the input gradient shares its chain with the parameter gradients and adds one fp32-accumulated GEMM, so its
    error against float64 stays within twice the largest error of the parameter gradients of the same pass (measured)"""
    B = 8
    G = new_generator(kind, dtype).train()
    inputs = R.generator_case(kind, B, seed=4)
    leaves = [x.to(DEV).requires_grad_(True) for x in inputs]
    img = G(*leaves)
    dimg = torch.randn(img.shape, generator=torch.Generator().manual_seed(2)) * 1e-3
    _, want_in, want_p, _ = reference_pass(kind, G, inputs, dimg, True, params=True)
    img.backward(dimg.to(DEV))
    a = max(rel_err(x.grad, w) for x, w in zip(leaves, want_in))
    errs = {k: rel_err(p.grad, want_p[k]) for k, p in G.named_parameters() if k not in PRE_BN_BIAS[kind]}
    b = max(errs.values())
    print(f"{kind} {dtype}: input gradient rel_err {a:.3g}; parameter gradients: largest rel_err {b:.3g} ({max(errs, key=errs.get)})")
    assert a <= 2 * b, (kind, dtype, a, b)


# ---- sampling.project_images --------------------------------------------------------------------------------------------------------------
PROJECT = {"celeba": dict(steps=6, lr=0.05), "mnist": dict(steps=10, lr=0.05), "dsprites": dict(steps=12, lr=0.05), "colored": dict(steps=12, lr=0.05)}


def project_case(kind, B=4):
    """an eval-mode generator, labels, the drawn (noise, code) and the target they generate"""
    G = new_generator(kind, seed=7).eval().requires_grad_(False)
    inputs = R.generator_case(kind, B, seed=11)
    if kind in ("dsprites", "colored"):
        ncls = R.WIDTHS[kind][0]
        labels, noise0, code0 = inputs[0][:, :ncls].contiguous(), None, inputs[0][:, ncls:].contiguous()
    else:
        noise0, labels, code0 = inputs
    with torch.no_grad():
        target = G(*[x.to(DEV) for x in inputs])
    return G, labels, noise0, code0, target


def module_loop(kind, G, labels, target, noise, code, steps, lr, code_range):
    """the plain loop a user writes over the drop-in module: leaves, torch.optim.Adam, clamp"""
    labels = labels.to(DEV)
    noise = None if noise is None else noise.clone().to(DEV).requires_grad_(True)
    code = code.clone().to(DEV).requires_grad_(True)
    opt = torch.optim.Adam([x for x in (noise, code) if x is not None], lr=lr)
    losses = []
    run = lambda: G(torch.cat((labels, code), 1)) if noise is None else G(noise, labels, code)
    for _ in range(steps):
        opt.zero_grad()
        per = ((run() - target) ** 2).flatten(1).mean(1)
        losses.append(per.detach())
        per.sum().backward()
        opt.step()
        with torch.no_grad():
            code.clamp_(*code_range)
    with torch.no_grad():
        losses.append(((run() - target) ** 2).flatten(1).mean(1))
    return noise, code, torch.stack(losses)


@pytest.mark.parametrize("kind", KINDS)
def test_project_images(kind):
    G, labels, noise0, code0, target = project_case(kind)
    B, cfg = target.shape[0], PROJECT[kind]
    start_noise = None if noise0 is None else torch.randn(noise0.shape, generator=torch.Generator().manual_seed(1))
    start_code = torch.zeros_like(code0)
    runs = [eg.sampling.project_images(kind, G, target, labels.to(DEV), cfg["steps"], cfg["lr"], seed=1) for _ in range(2)]
    noise, lab, code, losses = runs[0]
    assert losses.shape == (cfg["steps"] + 1, B) and bool(torch.isfinite(losses).all())
    ratios = (losses[-1] / losses[0]).cpu()
    print(f"project_images {kind}: loss after {cfg['steps']} steps / loss at the start, per sample: {[round(float(r), 3) for r in ratios]}")
    assert bool((losses[-1] < losses[0]).all()), ratios
    assert torch.equal(lab.cpu(), labels) and bool((code.abs() <= 1).all())
    for x, y in zip(runs[0], runs[1]):                                       # two runs: the same bits
        assert (x is None and y is None) or torch.equal(x, y)
    # the seeded start is the documented one
    again = eg.sampling.project_images(kind, G, target, labels.to(DEV), cfg["steps"], cfg["lr"], noise=start_noise, code=start_code)
    assert torch.equal(again[3], losses)
    # against the plain loop over the drop-in module, within K x what float32 torch on the CPU misses float64 by over the same loop
    m_noise, m_code, m_losses = module_loop(kind, G, labels, target, start_noise, start_code, cfg["steps"], cfg["lr"], (-1.0, 1.0))
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    fwd = lambda s, ins: R.FORWARDS[kind](s, ins, False)
    cpu = {}
    for dt in (torch.float32, torch.float64):
        sdt = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
        cpu[dt] = R.project_loop(fwd, sdt, labels, target.cpu(), start_noise, start_code, cfg["steps"], cfg["lr"], (-1.0, 1.0), dt)
    assert bool((cpu[torch.float64][2][-1] < cpu[torch.float64][2][0]).all())     # the float64 restatement meets the condition too
    for name, got, ref, i in (("noise", noise, m_noise, 0), ("code", code, m_code, 1), ("losses", losses, m_losses, 2)):
        if got is None:
            continue
        yard = R.dist(cpu[torch.float32][i], cpu[torch.float64][i])
        fig = R.dist(got, ref)
        print(f"project_images {kind} {name}: against the module loop {fig:.3g}, float32 yardstick {yard:.3g}, bound {R.K * yard:.3g}")
        assert fig <= R.K * yard, (kind, name, fig, yard)


def test_project_images_refuses_train_mode():
    G = new_generator("mnist").train()
    with pytest.raises(ValueError, match="eval"):
        eg.sampling.project_images("mnist", G, torch.zeros(2, 1, 32, 32, device=DEV), torch.zeros(2, 10, device=DEV), 1, 0.1)

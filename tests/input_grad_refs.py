"""float64 restatements for the input-gradient tests (tests/test_input_grad_host.py, tests/test_gpu_input_grad.py), written for that purpose
from the formulas of include/eadgan_hip.h and the layer lists of the reference scripts -- no code of the package is used:

* ``contraction``: dX[b][k] = sum_ij dH[b][i*NJ + j] * W[i*s_i + j*s_j + k*s_k]  (eg_linear_dinput), with the mutants of the host test;
* ``bn_eval_act`` / ``bn_eval_bwd``: eval-mode BatchNorm + activation and its input gradient (eg_bn_bwd_eval);
* ``FORWARDS``: the generator forwards of the CelebA, MNIST and dSprites scripts on a state_dict, returning the image and the outputs of
  their ReLU / LeakyReLU layers (``taps``), in train mode (batch statistics) or eval mode (running statistics)."""
import torch
import torch.nn.functional as F

K = 8.0                         # a result may miss float64 by K times what float32 torch on the CPU misses it by
MUTANT_FACTOR = 10.0
Y_EXCLUDE = 1e-4                # |y| below this: the sign that picks act'(y) is decided by rounding
EXCLUDE_CAP = 1e-3              # at most this share of a BatchNorm case may be left out
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# (B, NI, NJ, K): one row; the CelebA and MNIST layouts; B past one 128-row tile; a reduction shorter than one chunk with a ragged tail and a
# K that is no multiple of 8
LINEAR_CASES = ((1, 1, 128, 7), (3, 16, 1024, 218), (8, 64, 128, 79), (130, 1, 128, 5), (5, 3, 40, 9))
BN_CASES = ((128, 64), (130, 128), (8 * 64 * 64 // 16, 64))
ACTS = {"none": 0, "lrelu": 1, "relu": 2}          # EG_ACT_* codes
SLOPE = 0.2


def strides_of(NI, NJ, Kc):
    """(s_i, s_j, s_k, W elements) of a case: the real layouts where the case has their shape, else a [k][j][i] master"""
    if (NI, NJ) == (16, 1024):
        return 1, 16, 16 * 1024, Kc * 1024 * 16          # CelebA conv_blocks.0.weight [cin][1024][4][4]
    if (NI, NJ) == (64, 128):
        return Kc, 64 * Kc, 1, 8192 * Kc                 # MNIST l1.0.weight [8192][cin], row f = c*64 + hw
    if NI == 1:
        return 0, Kc, 1, NJ * Kc                         # dSprites fc1.0.weight [128][cin]
    return 1, NI, NI * NJ, NI * NJ * Kc


def linear_case(case, dtype, seed=0):
    """operands of one eg_linear_dinput case, pre-rounded to ``dtype``: dH [B, NI*NJ] (values of the dtype, as float32), W flat fp32
    master (NOT rounded: the kernel rounds it) and Wr, its values rounded to the dtype"""
    B, NI, NJ, Kc = case
    s_i, s_j, s_k, n = strides_of(NI, NJ, Kc)
    g = torch.Generator().manual_seed(1000 * seed + B + NI + NJ + Kc)
    tdt = TORCH_DTYPE[dtype]
    dH = torch.randn(B, NI * NJ, generator=g).to(tdt).float()
    W = torch.randn(n, generator=g) * 0.05
    return dict(dH=dH, W=W, Wr=W.to(tdt).float(), strides=(s_i, s_j, s_k))


def gather_w(W, NI, NJ, Kc, s_i, s_j, s_k):
    """Wv[i*NJ + j][k] = W[i*s_i + j*s_j + k*s_k]"""
    i = torch.arange(NI).view(NI, 1, 1)
    j = torch.arange(NJ).view(1, NJ, 1)
    k = torch.arange(Kc).view(1, 1, -1)
    return W.flatten()[(i * s_i + j * s_j + k * s_k).reshape(NI * NJ, Kc)]


def contraction(dH, W, NI, NJ, Kc, s_i, s_j, s_k, dtype=torch.float64, mutant=None, cpad=None):
    """the strided contraction in ``dtype``.  Mutants: ``swap_strides`` (s_i and s_j exchanged), ``padded_columns`` (the K columns are
    taken from a result that spans the padded row length ``cpad``, as if dX had the stride of the engines' ``inp``)"""
    if mutant == "swap_strides":
        s_i, s_j = s_j, s_i
    out = dH.to(dtype) @ gather_w(W, NI, NJ, Kc, s_i, s_j, s_k).to(dtype)
    if mutant == "padded_columns":
        return F.pad(out, (0, cpad - Kc)).flatten()[:dH.shape[0] * Kc].view(dH.shape[0], Kc)
    return out


def dist(got, want):
    """largest error against the float64 ``want``, in units of want's largest magnitude"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "non-finite value in a comparison"
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


# ---- eval-mode BatchNorm + activation -------------------------------------------------------------------------------------------------
def act(y, name):
    return y if name == "none" else (F.relu(y) if name == "relu" else F.leaky_relu(y, SLOPE))


def bn_case(case, dtype, seed=0):
    M, C = case
    g = torch.Generator().manual_seed(77 * seed + M + C)
    tdt = TORCH_DTYPE[dtype]
    return dict(z=torch.randn(M, C, generator=g).to(tdt).float(), da=torch.randn(M, C, generator=g).to(tdt).float(),
                gamma=1 + 0.1 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g), mean=0.2 * torch.randn(C, generator=g),
                var=0.5 + torch.rand(C, generator=g), eps=1e-5)


def bn_eval_act(z, c, name, dtype=torch.float64):
    """act(F.batch_norm(z, training=False)) on [M, C] rows"""
    t = lambda x: x.to(dtype)
    return act(F.batch_norm(t(z), t(c["mean"]), t(c["var"]), t(c["gamma"]), t(c["beta"]), False, 0.0, c["eps"]), name)


def bn_eval_bwd(c, name, dtype=torch.float64, mutant=None):
    """(dz, y) by autograd of bn_eval_act; mutant ``raw_var``: running_var used without eps and without the square root"""
    z = c["z"].detach().to(dtype).clone().requires_grad_(True)
    if mutant == "raw_var":
        t = lambda x: x.to(dtype)
        y = (z - t(c["mean"])) / t(c["var"]) * t(c["gamma"]) + t(c["beta"])
    else:
        y = F.batch_norm(z, c["mean"].to(dtype), c["var"].to(dtype), c["gamma"].to(dtype), c["beta"].to(dtype), False, 0.0, c["eps"])
    act(y, name).backward(c["da"].to(dtype))
    return z.grad, y.detach()


def bn_keep(y64, name):
    """elements whose act' does not hang on rounding (all of them without an activation)"""
    return torch.ones_like(y64, dtype=torch.bool) if name == "none" else y64.abs() >= Y_EXCLUDE


# ---- the generators (reference layer lists) on a state_dict ------------------------------------------------------------------------------
def _bn(x, sd, key, training, eps=1e-5):
    rm, rv = sd[key + ".running_mean"], sd[key + ".running_var"]
    if training:
        rm, rv = rm.clone(), rv.clone()
    return F.batch_norm(x, rm, rv, sd[key + ".weight"], sd[key + ".bias"], training, 0.1, eps)


def celeba_forward(sd, inputs, training, taps=None):
    """celebA/EAD-GAN_celebA.py:67-102; inputs = (noise, labels, code)"""
    x = torch.cat(inputs, -1).view(inputs[0].shape[0], -1, 1, 1)
    x = F.conv_transpose2d(x, sd["conv_blocks.0.weight"], sd["conv_blocks.0.bias"], 1, 0)
    for idx in (1, 4, 7):
        x = F.conv_transpose2d(x, sd[f"conv_blocks.{idx}.weight"], sd[f"conv_blocks.{idx}.bias"], 2, 1)
        x = F.relu(_bn(x, sd, f"conv_blocks.{idx + 1}", training))
        if taps is not None:
            taps.append(x.detach())
    return torch.tanh(F.conv_transpose2d(x, sd["conv_blocks.10.weight"], sd["conv_blocks.10.bias"], 2, 1))


def mnist_forward(sd, inputs, training, taps=None):
    """MNIST/EAD-GAN_rpqmnxy.py:71-98; inputs = (noise, labels, code)"""
    x = F.linear(torch.cat(inputs, -1), sd["l1.0.weight"], sd["l1.0.bias"]).view(inputs[0].shape[0], 128, 8, 8)
    x = _bn(x, sd, "conv_blocks.0", training)
    for conv, bn in ((2, 3), (6, 7)):
        x = F.interpolate(x, scale_factor=2)
        x = F.conv2d(x, sd[f"conv_blocks.{conv}.weight"], sd[f"conv_blocks.{conv}.bias"], 1, 1)
        x = F.leaky_relu(_bn(x, sd, f"conv_blocks.{bn}", training, 0.8), 0.2)
        if taps is not None:
            taps.append(x.detach())
    return torch.tanh(F.conv2d(x, sd["conv_blocks.9.weight"], sd["conv_blocks.9.bias"], 1, 1))


def dsprites_forward(sd, inputs, training, taps=None):
    """dSprites/rp.py:123-157 (colored_dSprites/rp_color.py with three channels); inputs = (z_c,)"""
    tap = (lambda t: taps.append(t.detach())) if taps is not None else (lambda t: None)
    x = F.relu(F.linear(inputs[0], sd["fc1.0.weight"], sd["fc1.0.bias"]))
    tap(x)
    x = F.relu(F.linear(x, sd["fc2.0.weight"], sd["fc2.0.bias"]))
    tap(x)
    x = x.view(-1, 64, 4, 4)
    for idx in (0, 3, 6):
        x = F.conv_transpose2d(x, sd[f"conv_block.{idx}.weight"], sd[f"conv_block.{idx}.bias"], 2, 1)
        x = F.relu(_bn(x, sd, f"conv_block.{idx + 1}", training))
        tap(x)
    return torch.sigmoid(F.conv_transpose2d(x, sd["conv_block.9.weight"], sd["conv_block.9.bias"], 2, 1))


FORWARDS = {"celeba": celeba_forward, "mnist": mnist_forward, "dsprites": dsprites_forward, "colored": dsprites_forward}
# input widths in the order the generators concatenate them
WIDTHS = {"celeba": (200, 10, 8), "mnist": (62, 10, 7), "dsprites": (3, 4), "colored": (3, 7)}


def first_layer(kind, cin, dtype=torch.float64, seed=0):
    """the reference-shaped first layer of a workload as (module output in the engines' dH order, weight, (NI, NJ, s_i, s_j, s_k)):
    x -> h with h flattened the way dh0 / dh / dz1 are stored"""
    g = torch.Generator().manual_seed(seed)
    if kind == "celeba":
        w = torch.randn(cin, 1024, 4, 4, generator=g).to(dtype)
        fn = lambda x: F.conv_transpose2d(x.view(x.shape[0], cin, 1, 1), w, None, 1, 0).permute(0, 2, 3, 1).reshape(x.shape[0], -1)      # NHWC: t*1024 + co
        return fn, w, (16, 1024, 1, 16, 16384)
    if kind == "mnist":
        lin = torch.nn.Linear(cin, 8192).to(dtype)
        fn = lambda x: lin(x).view(x.shape[0], 128, 8, 8).permute(0, 2, 3, 1).reshape(x.shape[0], -1)                                   # hw*128 + c
        return fn, lin.weight.detach(), (64, 128, cin, 64 * cin, 1)
    lin = torch.nn.Linear(cin, 128).to(dtype)
    return (lambda x: lin(x)), lin.weight.detach(), (1, 128, 0, cin, 1)


def generator_case(kind, B, seed):
    """float32 inputs of a module-level case: one tensor per generator input, one-hot labels"""
    g = torch.Generator().manual_seed(seed)
    w = WIDTHS[kind]
    if kind in ("dsprites", "colored"):
        lab = F.one_hot(torch.randint(0, w[0], (B,), generator=g), w[0]).float()
        return (torch.cat((lab, torch.rand(B, w[1], generator=g) * 2 - 1), 1),)
    lab = F.one_hot(torch.randint(0, w[1], (B,), generator=g), w[1]).float()
    return torch.randn(B, w[0], generator=g), lab, torch.rand(B, w[2], generator=g) * 2 - 1


def project_loop(forward, sd, labels, target, noise, code, steps, lr, code_range, dtype):
    """the projection loop restated with torch: eval forward, sum of per-sample mean squared errors, torch.optim.Adam on (noise, code),
    clamp of the code -> (noise, code, losses [steps + 1, B]).  ``forward(sd, inputs)``; ``noise`` None for the dSprites kinds"""
    t = lambda x: None if x is None else x.detach().to(dtype).clone()
    labels, target, noise, code = t(labels), t(target), t(noise), t(code)
    leaves = [x.requires_grad_(True) for x in (noise, code) if x is not None]
    opt = torch.optim.Adam(leaves, lr=lr)
    losses = []

    def loss_of():
        ins = (torch.cat((labels, code), 1),) if noise is None else (noise, labels, code)
        return ((forward(sd, ins) - target) ** 2).flatten(1).mean(1)
    for _ in range(steps):
        opt.zero_grad()
        per = loss_of()
        losses.append(per.detach())
        per.sum().backward()
        opt.step()
        if code_range is not None:
            with torch.no_grad():
                code.clamp_(*code_range)
    with torch.no_grad():
        losses.append(loss_of())
    return (None if noise is None else noise.detach()), code.detach(), torch.stack(losses)

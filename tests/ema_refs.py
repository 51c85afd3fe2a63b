"""float64 restatement of the weight average for tests/test_gpu_ema.py, written from the contract in include/eadgan_hip.h (no code of the
package is used): the decay of update t, the recurrence  e <- e + (1 - b_t) (w - e)  in a chosen precision with its mutants, the segment
table of the kernel test with its carved, canary-fenced operands, and the trainers the run tests build.

The bound is the project's: a result may miss float64 by K times what float32 torch on the CPU (``e + d * (w - e)``) misses
it by on the same operands, in units of the largest |result|; a mutant must miss it by MUTANT_FACTOR times that bound."""
import functools

import pytest
import torch

from input_grad_refs import K, MUTANT_FACTOR, dist           # noqa: F401  (the tests read them from here)

pytestmark = pytest.mark.gpu

SMALL_LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1026)            # below / around one and 64 16-byte groups, ragged ends
LARGE_LENGTH = (1 << 20) + 3
GRID_CHUNKS = 512 + 3                                        # chunks of the segment that outnumbers the launch's workgroups (ema.hip: 512)
DECAYS = ((0.999, 0.0, 0), (0.999, 10.0, 0), (0.999, 10.0, 5), (0.5, 10.0, 10 ** 6))      # (beta, ramp, t)
CANARY = 8


def decay(beta, ramp, t):
    """b_t as the float32 the kernel forms: three fp32 operations in the header's order -> Python float"""
    b = torch.tensor(beta, dtype=torch.float32)
    if ramp == 0:
        return float(b)
    tf = torch.tensor(int(t), dtype=torch.int64).to(torch.float32)
    r = torch.tensor(ramp, dtype=torch.float32)
    return float(torch.minimum(b, (torch.tensor(1.0, dtype=torch.float32) + tf) / (r + tf)))


def lerp(e, w, b, dtype=torch.float64, mutant=None, chunk=None):
    """one update of one segment in ``dtype``.  float64: d = 1 - b exactly (b is a float32 value); float32: d rounded, as the kernel has it.
    Mutants: ``swap`` (d = b), ``skip_ragged`` (the last, ragged chunk of the segment is left as it was)"""
    e, w = e.to(dtype), w.to(dtype)
    d = torch.tensor(b, dtype=dtype) if mutant == "swap" else torch.tensor(1.0, dtype=dtype) - torch.tensor(b, dtype=dtype)
    out = e + d * (w - e)
    if mutant == "skip_ragged" and e.numel() % chunk:
        keep = e.numel() // chunk * chunk
        out = out.clone()
        out.view(-1)[keep:] = e.view(-1)[keep:]
    return out


def recurrence(e0, ws, beta, ramp, t0=0, dtype=torch.float64):
    """the shadow after one update per entry of ``ws`` (the weights after each iteration), from ``e0``, the first update being number t0"""
    e = e0.to(dtype)
    for k, w in enumerate(ws):
        e = lerp(e, w, decay(beta, ramp, t0 + k), dtype)
    return e


def carve(n, off, dtype, gen):
    """-> (buffer, view): ``n`` elements that begin ``off`` elements behind a 16-byte boundary, CANARY elements of the buffer on both
    sides (and the alignment padding) holding a pattern of their own"""
    assert CANARY * 4 % 16 == 0
    total = CANARY + off + n + CANARY + 4
    if dtype == torch.float32:
        buf = torch.randn(total, generator=gen)
    else:
        buf = torch.randint(-2 ** 31, 2 ** 31 - 1, (total,), generator=gen, dtype=torch.int64).to(dtype)
    return buf, (CANARY + off, n)


@functools.lru_cache(maxsize=None)
def kernel_table(chunk, single=False):
    """host operands of the kernel test: [(kind, src buffer, src span, dst buffer, dst span)] -- kind 0 lerp (fp32), 1 copy.  The small
    lerp lengths at all 16 (src, dst) offsets from a 16-byte boundary; chunk - 1, chunk, chunk + 1 and the large length aligned, chunk + 1
    also at offsets (1, 2) (several chunks on the word path); an aligned segment of more chunks than the launch has workgroups; a copy segment of an odd word count; a copy segment over int64 elements.
    ``single``: one aligned lerp segment of chunk + 1 words.  Never modified."""
    g = torch.Generator().manual_seed(1234)
    segs = []

    def add(kind, n, so, do, dtype=torch.float32):
        sb, ss = carve(n, so, dtype, g)
        db, ds = carve(n, do, dtype, g)
        segs.append((kind, sb, ss, db, ds))

    if single:
        add(0, chunk + 1, 0, 0)
        return tuple(segs)
    for n in SMALL_LENGTHS:
        for so in range(4):
            for do in range(4):
                add(0, n, so, do)
    for n in (chunk - 1, chunk, chunk + 1, LARGE_LENGTH):
        add(0, n, 0, 0)
    add(0, chunk + 1, 1, 2)
    add(0, GRID_CHUNKS * chunk + 5, 0, 0)                    # more chunks than workgroups: every workgroup arrives, some walk two chunks
    add(1, 1001, 0, 0, torch.int32)                          # odd word count; every bit pattern, NaNs of fp32 among them
    add(1, 37, 0, 0, torch.int64)                            # two words per element
    return tuple(segs)


def lerp_operands(table):
    """(e, w) of the lerp segments of a table, concatenated (the bound is taken over the launch)"""
    es = [db[o:o + n] for kind, _, _, db, (o, n) in table if kind == 0]
    ws = [sb[o:o + n] for kind, sb, (o, n), _, _ in table if kind == 0]
    return es, ws


@functools.lru_cache(maxsize=None)
def kernel_reference(chunk, single, beta, ramp, t):
    """-> (float64 results of the lerp segments concatenated, yardstick, {mutant: its distance from the float64 results})"""
    es, ws = lerp_operands(kernel_table(chunk, single))
    b = decay(beta, ramp, t)
    want = torch.cat([lerp(e, w, b) for e, w in zip(es, ws)])
    yard = dist(torch.cat([lerp(e, w, b, torch.float32) for e, w in zip(es, ws)]), want)
    mutants = {m: dist(torch.cat([lerp(e, w, b, mutant=m, chunk=chunk) for e, w in zip(es, ws)]), want) for m in ("swap", "skip_ragged")}
    return want, yard, mutants


# ---- trainers ------------------------------------------------------------------------------------------------------------------------------
B = 8
N_IMAGES = 20


def sprites(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    s = torch.zeros(n, 64, 64, dtype=torch.uint8)
    for i in range(n):
        y, x, h, w = [int(v) for v in torch.randint(8, 40, (4,), generator=g)]
        s[i, y:y + 4 + h // 3, x:x + 4 + w // 3] = 1
    return s.to(dev)


def make(eg, kind, dtype, seed, dev="cuda", data_seed=4, input_seed=5):
    """modules with torch's default initialisation from ``seed``, a trainer at batch 8 and its device sampler (one seed) over 20 images"""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(data_seed)
    if kind == "celeba":
        mods = [eg.celeba.Generator(dtype=dtype).to(dev), eg.celeba.Discriminator(dtype=dtype).to(dev)]
        tr = eg.celeba.CelebATrainer(*mods, B, dtype=dtype)
        inp = eg.celeba.DeviceInputs(torch.randint(0, 256, (N_IMAGES, 3, 64, 64), dtype=torch.uint8, generator=g).to(dev), seed=input_seed)
    elif kind == "mnist":
        from oracle import mnist_oracle as mo
        eg.mnist.load_approximator(mo.make_approximator(123))
        mods = [eg.mnist.Generator(dtype=dtype).to(dev), eg.mnist.Discriminator(dtype=dtype).to(dev), eg.mnist.Encoder(dtype=dtype).to(dev)]
        tr = eg.mnist.MnistTrainer(*mods, B, dtype=dtype)
        inp = eg.mnist.DeviceInputs(torch.randint(0, 256, (N_IMAGES, 1, 32, 32), dtype=torch.uint8, generator=g).to(dev), seed=input_seed)
    elif kind in ("dsprites", "colored"):
        mod = eg.colored if kind == "colored" else eg.dsprites
        mods = [mod.Encoder_pxy(dtype=dtype).to(dev), mod.Generator(dtype=dtype).to(dev), mod.Discriminator(dtype=dtype).to(dev), mod.Encoder(dtype=dtype).to(dev)]
        tr = (mod.ColoredTrainer if kind == "colored" else mod.DspritesTrainer)(*mods, B, dtype=dtype)
        inp = mod.DeviceInputs(sprites(N_IMAGES, data_seed, dev), seed=input_seed)
    else:
        mod = eg.colored if kind == "pxy_color" else eg.dsprites
        mods = [mod.Encoder_pxy(dtype=dtype).to(dev)]
        tr = (eg.colored.PxyColorTrainer if kind == "pxy_color" else eg.dsprites.PxyTrainer)(mods[0], B, dtype=dtype)
        inp = mod.PxyDeviceInputs(sprites(N_IMAGES, data_seed, dev), seed=input_seed)
    return tr, inp


def segment_kind(module, key):
    """how the average treats the entry ``key`` of ``module.state_dict()``: 0 lerp (parameters, BatchNorm running statistics), 1 copy"""
    if key in dict(module.named_parameters()) or key.endswith(("running_mean", "running_var")):
        return 0
    return 1

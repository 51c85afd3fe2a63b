"""Sharded device draws on the MI355X: the ranks' draws, concatenated in rank order, are BIT FOR BIT the one-rank draw of the
global batch -- at the kernel (shards that begin inside a Philox quad or a Box-Muller pair, past one block, the fused launch with its
one-hot rows, the epoch permutation with an epoch end inside a shard), at the six samplers (every input slot of a trainer at B = 8 against
two trainers at B = 4), and the argument checks of ``train.TrainRun`` that need no process group.  Everything runs in one process: a
"rank" here is only the (rank, world) pair a draw is made with."""
import ctypes
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None
STEP = 7                               # a non-zero device step counter
SIZES = (1, 3, 4, 5, 1026)             # local sizes: rank 1 starts at lanes 1, 3, 0, 1 of a quad and past one block's 1024 elements
N_IMAGES = 20


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _step(v=STEP):
    return torch.tensor([v], device=DEV, dtype=torch.int32)


# (kind, a, b, dtype) of the four element-wise kinds
def _kinds():
    ops = eg.ops
    return ((ops.RNG_UNIFORM, -1.0, 1.0, torch.float32), (ops.RNG_NORMAL, 0.5, 2.0, torch.float32), (ops.RNG_RANDINT, 0, 10, torch.int64),
            (ops.RNG_BERNOULLI, 0.5, 0.0, torch.uint8))


# ---- the kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_concatenated_shards_are_the_one_rank_draw(n, world):
    ops = eg.ops
    st = _step()
    for kind, a, b, dtype in _kinds():
        whole = torch.empty(world * n, device=DEV, dtype=dtype)
        ops.rng_fill(kind, whole, a, b, 11, st, 3)
        parts = []
        for rank in range(world):
            out = torch.empty(n, device=DEV, dtype=dtype)
            ops.rng_fill(kind, out, a, b, 11, st, 3, rank=rank, world=world)
            parts.append(out)
        assert torch.equal(torch.cat(parts), whole), (kind, n, world)
        if world * n >= 8 and kind != ops.RNG_BERNOULLI:
            assert not torch.equal(parts[0], parts[1])                          # the shards are different draws
        # the keywords' defaults are the call without them
        again = torch.empty(world * n, device=DEV, dtype=dtype)
        ops.rng_fill(kind, again, a, b, 11, st, 3, rank=0, world=1)
        assert torch.equal(again, whole)


@pytest.mark.parametrize("world", [2, 3])
def test_fused_launch_shards_three_draws_of_different_sizes(world):
    """eg_rng_fill_multi: three draws of different local sizes in one launch (one of them label draws with fused one-hot rows, indexed
    locally), every kind, against the one-rank fused launch and against the single launches"""
    ops = eg.ops
    st = _step()
    for sizes in ((1, 3, 5), (1026, 4, 5), (5, 1026, 3)):
        for kind, a, b, dtype in _kinds():
            def draws(mult):
                outs = [torch.empty(mult * n, device=DEV, dtype=dtype) for n in sizes]
                oh = [torch.full((mult * n, 10), -1.0, device=DEV) if kind == ops.RNG_RANDINT else None for n in sizes]
                return outs, oh, [(kind, o, a, b, 2 + j) + ((h,) if h is not None else ()) for j, (o, h) in enumerate(zip(outs, oh))]

            w_out, w_oh, w_draws = draws(world)
            ops.rng_fill_multi(w_draws, 11, st)
            shard_out, shard_oh = [], []
            for rank in range(world):
                o, h, d = draws(1)
                ops.rng_fill_multi(d, 11, st, rank=rank, world=world)
                shard_out.append(o)
                shard_oh.append(h)
            for j, n in enumerate(sizes):
                assert torch.equal(torch.cat([s[j] for s in shard_out]), w_out[j]), (kind, sizes, j)
                single = torch.empty(world * n, device=DEV, dtype=dtype)
                ops.rng_fill(kind, single, a, b, 11, st, 2 + j)
                assert torch.equal(single, w_out[j])
                if kind == ops.RNG_RANDINT:
                    got = torch.cat([s[j] for s in shard_oh])
                    assert torch.equal(got, w_oh[j]) and torch.equal(got, torch.nn.functional.one_hot(w_out[j], 10).float())
            # defaults == no keywords
            d_out, _, d_draws = draws(world)
            ops.rng_fill_multi(d_draws, 11, st, rank=0, world=1)
            assert all(torch.equal(x, y) for x, y in zip(d_out, w_out))


def test_a_shard_past_its_total_is_refused_by_the_c_abi():
    out = torch.zeros(8, device=DEV)
    st = _step()
    L = eg._lib.lib()
    with pytest.raises(RuntimeError, match="exceeds total"):
        L.call("eg_rng_fill", 0, out.data_ptr(), 8, 0.0, 1.0, 1, st.data_ptr(), 1, 9, 16, None)              # 9 + 8 > 16
    with pytest.raises(RuntimeError, match="exceeds total"):
        L.call("eg_rng_fill", 0, out.data_ptr(), 8, 0.0, 1.0, 1, st.data_ptr(), 1, 17, 16, None)             # elem0 > total
    seg = (eg._lib.EgRngSeg * 1)(eg._lib.EgRngSeg(0, out.data_ptr(), 8, 0.0, 1.0, 1, None, 0, 1, 8))
    with pytest.raises(RuntimeError, match="exceeds total"):
        L.call("eg_rng_fill_multi", seg, 1, 1, st.data_ptr(), None)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                                                     # nothing was launched
    L.call("eg_rng_fill", 0, out.data_ptr(), 8, 0.0, 1.0, 1, st.data_ptr(), 1, 8, 16, None)                  # 8 + 8 == 16 is a shard
    assert float(out.abs().sum()) > 0.0


# ---- the epoch permutation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,world,steps", [(18, 2, 9), (20, 3, 10)])
def test_sharded_epoch_permutation_strides_by_the_global_batch(N, world, steps):
    """positions (step * world + rank) * n + i: at N = 18, n = 4, world = 2 the epoch ends after position 17, INSIDE rank 0's shard of step 2
    (positions 16 .. 19).  One epoch visits every image once over all ranks."""
    ops = eg.ops
    n = 4
    for fused in (False, True):
        step = torch.zeros(1, device=DEV, dtype=torch.int32)
        cat, whole = [], []
        for s in range(steps):
            parts = []
            for rank in range(world):
                out = torch.empty(n, device=DEV, dtype=torch.int64)
                if fused:
                    ops.rng_fill_multi([(ops.RNG_EPOCH_PERM, out, N, 0, 1)], 123, step, rank=rank, world=world)
                else:
                    ops.rng_fill(ops.RNG_EPOCH_PERM, out, N, 0, 123, step, 1, rank=rank, world=world)
                parts.append(out)
            w = torch.empty(world * n, device=DEV, dtype=torch.int64)
            ops.rng_fill(ops.RNG_EPOCH_PERM, w, N, 0, 123, step, 1)
            assert torch.equal(torch.cat(parts), w), (s, fused)
            cat += parts
            whole.append(w)
            ops.counter_add(step, 1)
        idx = torch.cat(cat).cpu()
        total = steps * world * n
        assert idx.numel() == total and total % N == 0
        assert torch.equal(torch.bincount(idx, minlength=N), torch.full((N,), total // N))              # 72 positions: every index 4 times
        for e in range(total // N):
            assert torch.equal(torch.sort(idx[e * N:(e + 1) * N]).values, torch.arange(N)), e           # once in each aligned block of N
        assert not torch.equal(idx[:N], idx[N:2 * N])


# ---- the samplers ------------------------------------------------------------------------------------------------------------
SLOTS = {"celeba": ("real", "z", "code", "labels", "onehot"), "mnist": ("real", "labels", "onehot", "z", "code"),
         "dsprites": ("img", "code1", "onehot1", "code2", "onehot2"), "colored": ("img", "code1", "onehot1", "code2", "onehot2", "gains"),
         "pxy": ("img_u8", "code"), "pxy_color": ("img_u8", "code", "gains")}
_trainers = {}


def _sprites(n, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.zeros(n, 64, 64, dtype=torch.uint8)
    for i in range(n):
        y, x, h, w = [int(v) for v in torch.randint(8, 40, (4,), generator=g)]
        s[i, y:y + 4 + h // 3, x:x + 4 + w // 3] = 1
    return s.to(DEV)


def _trainer(kind, B):
    """a real fp32 trainer of ``kind`` at batch ``B`` (built once per (kind, B): the samplers only write its input slots)"""
    if (kind, B) in _trainers:
        return _trainers[(kind, B)]
    torch.manual_seed(1)
    if kind == "celeba":
        tr = eg.celeba.CelebATrainer(eg.celeba.Generator(dtype="f32").to(DEV), eg.celeba.Discriminator(dtype="f32").to(DEV), B, dtype="f32")
    elif kind == "mnist":
        from oracle import mnist_oracle as mo
        eg.mnist.load_approximator(mo.make_approximator(123))
        tr = eg.mnist.MnistTrainer(eg.mnist.Generator(dtype="f32").to(DEV), eg.mnist.Discriminator(dtype="f32").to(DEV),
                                   eg.mnist.Encoder(dtype="f32").to(DEV), B, dtype="f32")
    elif kind in ("dsprites", "colored"):
        mod = eg.colored if kind == "colored" else eg.dsprites
        mods = [mod.Encoder_pxy(dtype="f32").to(DEV), mod.Generator(dtype="f32").to(DEV), mod.Discriminator(dtype="f32").to(DEV),
                mod.Encoder(dtype="f32").to(DEV)]
        tr = (mod.ColoredTrainer if kind == "colored" else mod.DspritesTrainer)(*mods, B, dtype="f32")
    else:
        mod = eg.colored if kind == "pxy_color" else eg.dsprites
        tr = (eg.colored.PxyColorTrainer if kind == "pxy_color" else eg.dsprites.PxyTrainer)(mod.Encoder_pxy(dtype="f32").to(DEV), B, dtype="f32")
    _trainers[(kind, B)] = tr
    return tr


def _sampler(kind, **kw):
    g = torch.Generator().manual_seed(4)
    if kind == "celeba":
        return eg.celeba.DeviceInputs(torch.randint(0, 256, (N_IMAGES, 3, 64, 64), dtype=torch.uint8, generator=g).to(DEV), seed=5, **kw)
    if kind == "mnist":
        return eg.mnist.DeviceInputs(torch.randint(0, 256, (N_IMAGES, 1, 32, 32), dtype=torch.uint8, generator=g).to(DEV), seed=5, **kw)
    if kind in ("dsprites", "colored"):
        return (eg.colored if kind == "colored" else eg.dsprites).DeviceInputs(_sprites(N_IMAGES, 4), seed=5, **kw)
    return (eg.colored if kind == "pxy_color" else eg.dsprites).PxyDeviceInputs(_sprites(N_IMAGES, 4), seed=5, **kw)


def _enqueue(inp, tr):
    """the sampler's launches of one iteration; the CelebA trainer's pipelined body would run the image gather (with the counter tick)
    on its preparation lane -- here it runs in place"""
    inp.enqueue(tr)
    tail = getattr(tr, "_inputs_tail", None)
    if tail is not None:
        tr._inputs_tail = None
        tail()


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "single-launches"])
@pytest.mark.parametrize("kind", sorted(SLOTS))
def test_two_sharded_samplers_fill_the_slots_of_one(kind, fuse, monkeypatch):
    """Real trainers of all six kinds at B = 8 and B = 4 (no stand-in was needed): for three consecutive ``enqueue`` calls every input
    slot of the whole trainer equals the concatenation of the two shards' slots, bit for bit.  20 images at a global batch of 8: the
    third call crosses the epoch end."""
    monkeypatch.setattr(eg.engine, "FUSE_DRAWS", fuse)
    whole_tr, whole_in = _trainer(kind, 8), _sampler(kind)
    assert (whole_in.rank, whole_in.world) == (0, 1)
    shard_in = [_sampler(kind, rank=r, world=2) for r in (0, 1)]
    assert [(s.rank, s.world) for s in shard_in] == [(0, 2), (1, 2)]
    shard_tr = _trainer(kind, 4)                     # one B = 4 trainer serves both ranks in turn: its slots are read out in between
    previous = None
    for it in range(3):
        _enqueue(whole_in, whole_tr)
        want = {s: getattr(whole_tr, s).clone() for s in SLOTS[kind]}
        got = []
        for r in (0, 1):
            _enqueue(shard_in[r], shard_tr)
            got.append({s: getattr(shard_tr, s).clone() for s in SLOTS[kind]})
        for s in SLOTS[kind]:
            cat = torch.cat((got[0][s], got[1][s]))
            assert cat.shape == want[s].shape and cat.dtype == want[s].dtype and torch.equal(cat, want[s]), (kind, it, s)
            assert not torch.equal(got[0][s], got[1][s]) or s.startswith("onehot") or s == "labels", (kind, it, s)
        if previous is not None:
            assert not torch.equal(previous["code" if "code" in want else "code1"], want["code" if "code" in want else "code1"])
        previous = want
    assert int(whole_in.step.item()) == 3 and all(int(s.step.item()) == 3 for s in shard_in)       # the counter counts global iterations


def test_sampler_constructors_validate_rank_and_world():
    data = torch.zeros(4, 3, 64, 64, dtype=torch.uint8, device=DEV)
    for rank, world in ((0, 0), (-1, 2), (2, 2)):
        with pytest.raises(ValueError, match="world"):
            eg.celeba.DeviceInputs(data, seed=1, rank=rank, world=world)
        with pytest.raises(ValueError, match="world"):
            eg.mnist.DeviceInputs(data, seed=1, rank=rank, world=world)


# ---- TrainRun's argument errors -------------------------------------------------------------------------------------------------
def test_train_run_admission_and_run_world(tmp_path):
    tr = _trainer("pxy", 4)
    with pytest.raises(ValueError, match=r"world = 2.*span 1"):
        eg.train.TrainRun("pxy", tr, _sampler("pxy", rank=0, world=2), str(tmp_path / "a"), n_epochs=1, graph=False)
    # a trainer with collectives over 2 ranks: a one-rank sampler is refused, and so is a captured run (before anything is captured)
    dp_tr = eg.dsprites.PxyTrainer(eg.dsprites.Encoder_pxy(dtype="f32").to(DEV), 4, dtype="f32", allreduce=eg.dp.GradAllReduce(2))
    with pytest.raises(ValueError, match=r"world = 1.*span 2"):
        eg.train.TrainRun("pxy", dp_tr, _sampler("pxy"), str(tmp_path / "b"), n_epochs=1, graph=False)
    with pytest.raises(ValueError, match="graph=False"):
        eg.train.TrainRun("pxy", dp_tr, _sampler("pxy", rank=1, world=2), str(tmp_path / "c"), n_epochs=1)
    assert dp_tr.graph is None
    # run.world in the state file
    run = eg.train.TrainRun("pxy", tr, _sampler("pxy"), str(tmp_path / "d"), n_epochs=1, sample_interval=1, graph=False)
    assert (run.rank, run.world, run.L) == (0, 1, 5)
    run.run(max_iters=1)
    path = run.files[-1]
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["run.world"] == 1 and sd["meta.format"] == 1
    two = str(tmp_path / "world2.pt")
    torch.save(dict(sd, **{"run.world": 2}), two)
    with pytest.raises(ValueError, match=r"run\.world"):
        eg.train.TrainRun.resume(two, "pxy", tr, _sampler("pxy"), str(tmp_path / "e"), n_epochs=1, sample_interval=1, graph=False)
    old = str(tmp_path / "old.pt")                   # a file from before run.world existed is a one-process run
    torch.save({k: v for k, v in sd.items() if k != "run.world"}, old)
    back = eg.train.TrainRun.resume(old, "pxy", tr, _sampler("pxy"), str(tmp_path / "f"), n_epochs=1, sample_interval=1, graph=False)
    assert back.batches_done == 1 and back.world == 1

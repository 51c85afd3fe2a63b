"""Weight averaging on the MI355X: the one-launch kernel against float64 at its launch edges (tests/ema_refs.py), its
determinism eagerly and inside a hipGraph, the trainers with an average attached (training undisturbed, the shadow bit-equal to the
launch applied by hand to the recorded weights and within the float64 bound), capture, state, and the run driver's files and resume."""
import gc
import importlib
import os

import numpy as np
import pytest
import torch

import ema_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None
BETA, RAMP = 0.9, 2.0
ITERS = 3


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


@pytest.fixture(autouse=True)
def _collect_trainers():
    """A trainer with a loss log is a reference cycle (trainer.log <-> log.trainer): only the cycle collector frees it, whenever it next
    runs -- possibly inside a later test's stream capture, where destroying this test's hipGraphs, streams and events is not allowed.
    Collect here, between tests, with the device idle."""
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


# ---- 1. the kernel against float64 ----------------------------------------------------------------------------------------------------------
def _device_table(single):
    """the host table of ema_refs on the device: -> (host table, [(src buffer, dst buffer)] on the device, segments for ops.ema_plan)"""
    table = R.kernel_table(eg.ops.ema_chunk_words(), single)
    bufs, segs = [], []
    for kind, sb, (so, n), db, (do, _) in table:
        s, d = sb.to(DEV), db.to(DEV)
        assert s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
        bufs.append((s, d))
        segs.append((s[so:so + n], d[do:do + n], kind))
    return table, bufs, segs


@pytest.mark.parametrize("single", [False, True], ids=["table", "nseg1"])
@pytest.mark.parametrize("beta,ramp,t", R.DECAYS)
def test_kernel_against_float64(beta, ramp, t, single):
    chunk = eg.ops.ema_chunk_words()
    table, bufs, segs = _device_table(single)
    if not single:
        pairs = {((s.data_ptr() // 4) % 4, (d.data_ptr() // 4) % 4) for s, d, _ in segs[:16 * len(R.SMALL_LENGTHS)]}
        assert len(pairs) == 16                                   # every (src, dst) offset from a 16-byte boundary occurs
    plan = eg.ops.ema_plan(segs)
    assert plan[2] == len(segs) == (1 if single else 16 * len(R.SMALL_LENGTHS) + 8)
    updates = torch.tensor([t, 0], dtype=torch.int32, device=DEV)
    eg.ops.ema_update(*plan, beta, ramp, updates)
    torch.cuda.synchronize()
    assert updates.tolist() == [t + 1, 0]
    got = []
    as_bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    for (kind, sb, (so, n), db, (do, _)), (s, d) in zip(table, bufs):
        s, d = s.cpu(), d.cpu()
        assert torch.equal(as_bits(s), as_bits(sb)), "src was written"
        assert torch.equal(as_bits(d[:do]), as_bits(db[:do])) and torch.equal(as_bits(d[do + n:]), as_bits(db[do + n:])), \
            f"written outside dst (n = {n}, offsets {so % R.CANARY}, {do % R.CANARY})"
        if kind == 1:
            assert torch.equal(as_bits(d[do:do + n]), as_bits(sb[so:so + n])), "copy segment differs from src"
        else:
            got.append(d[do:do + n])
    want, yard, mutants = R.kernel_reference(chunk, single, beta, ramp, t)
    err = R.dist(torch.cat(got), want)
    print(f"[ema-kernel] {'nseg1' if single else 'table'} beta {beta} ramp {ramp} t {t}: b_t = {R.decay(beta, ramp, t)!r}, error {err:.3e}, "
          f"yardstick {yard:.3e}, mutants {({k: float(f'{v:.3e}') for k, v in mutants.items()})}")
    assert float(eg.engine.ema_decay(beta, ramp, t)) == R.decay(beta, ramp, t)              # the host twin gives the reference's float32
    assert yard > 0
    assert err <= R.K * yard
    for name, miss in mutants.items():                            # the bound has teeth
        if name == "swap" and R.decay(beta, ramp, t) == 0.5:      # b = 1 - b: the swapped kernel IS the kernel, no bound can tell them apart
            assert miss == 0.0
            continue
        assert miss > R.MUTANT_FACTOR * R.K * yard, (name, miss, yard)


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_launches_and_a_replayed_graph_are_bit_equal():
    def fresh():
        table, bufs, segs = _device_table(False)
        return bufs, eg.ops.ema_plan(segs), torch.zeros(2, dtype=torch.int32, device=DEV)

    k = 3
    results = []
    for _ in range(2):                                            # two eager sequences of k launches from the same state
        bufs, plan, updates = fresh()
        for _ in range(k):
            eg.ops.ema_update(*plan, 0.999, 10.0, updates)
        torch.cuda.synchronize()
        results.append(([d.cpu() for _, d in bufs], updates.tolist()))
    bufs, plan, updates = fresh()                                 # a graph of the one launch, replayed k times
    start = [d.clone() for _, d in bufs]
    eg.ops.ema_update(*plan, 0.999, 10.0, updates)                # loads the kernel outside the capture
    for (_, d), d0 in zip(bufs, start):
        d.copy_(d0)
    updates.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eg.ops.ema_update(*plan, 0.999, 10.0, updates)
    for _ in range(k):
        graph.replay()
    torch.cuda.synchronize()
    results.append(([d.cpu() for _, d in bufs], updates.tolist()))
    assert results[0][1] == results[1][1] == results[2][1] == [k, 0]
    for a, b, c in zip(*(r[0] for r in results)):
        bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))


# ---- 3. training is undisturbed and the shadow is right ----------------------------------------------------------------------------------
def _weights(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items()}


@pytest.fixture(scope="module")
def eager_runs():
    """(kind, dtype) -> what tests 3 and 4 share: run A (no average: losses, recorded weights, final state) and run B (average attached)"""
    cache = {}

    def get(kind, dtype):
        if (kind, dtype) in cache:
            return cache[(kind, dtype)]
        names = ("G", "E") if kind == "dsprites" else ("G",)
        tr, inp = R.make(eg, kind, dtype, seed=1)
        tr.inputs = inp
        mods = tr._state_modules()
        rec = {n: [_weights(mods[n])] for n in names}
        lossA = []
        for _ in range(ITERS):
            lossA.append(tr.step_resident().clone())
            for n in names:
                rec[n].append(_weights(mods[n]))
        sdA = tr.state_dict()
        kinds = {n: {k: R.segment_kind(mods[n], k) for k in rec[n][0]} for n in names}
        del tr, inp, mods
        tr, inp = R.make(eg, kind, dtype, seed=1)
        tr.inputs = inp
        assert tr.ema is None
        ema = tr.attach_ema(BETA, ramp=RAMP, modules=names)
        assert ema is tr.ema and ema.names == names and ema.updates.tolist() == [0, 0]
        for n in names:                                            # at construction the shadow is the module's state
            for k, v in ema.state_dict(n).items():
                assert torch.equal(v, rec[n][0][k]), (n, k)
        lossB = [tr.step_resident().clone() for _ in range(ITERS)]
        sdB = tr.state_dict()
        shadow = {n: {k: v.detach().clone() for k, v in ema.state_dict(n).items()} for n in names}
        out = cache[(kind, dtype)] = dict(names=names, rec=rec, kinds=kinds, lossA=torch.stack(lossA).cpu(), lossB=torch.stack(lossB).cpu(), sdA=sdA,
                                          sdB=sdB, shadow=shadow, updates=ema.updates.tolist(), keys={n: list(ema.state_dict(n)) for n in names})
        return out

    return get


CASES = [("celeba", "f32"), ("mnist", "f32"), ("dsprites", "f32"), ("colored", "f32"), ("celeba", "bf16")]


@pytest.mark.parametrize("kind,dtype", CASES)
def test_training_is_undisturbed_and_the_shadow_is_right(kind, dtype, eager_runs):
    r = eager_runs(kind, dtype)
    assert torch.equal(r["lossA"], r["lossB"]) and bool(torch.isfinite(r["lossA"]).all())
    for k, v in r["sdA"].items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, r["sdB"][k]), k
        else:
            assert v == r["sdB"][k], k
    assert set(r["sdB"]) - set(r["sdA"]) == {f"ema.{n}.{k}" for n in r["names"] for k in r["keys"][n]} | {"ema.updates", "meta.ema"}
    assert r["updates"] == [ITERS, 0]
    for n in r["names"]:
        rec, kinds = r["rec"][n], r["kinds"][n]
        assert r["keys"][n] == list(rec[0])                        # the module's own keys in the module's own order
        # the one launch applied by hand to the weights recorded after each of A's iterations, from A's initial state
        hand = {k: v.clone() for k, v in rec[0].items()}
        updates = torch.zeros(2, dtype=torch.int32, device=DEV)
        for i in range(1, ITERS + 1):
            plan = eg.ops.ema_plan([(rec[i][k].reshape(-1), hand[k].reshape(-1), kinds[k]) for k in hand])
            eg.ops.ema_update(*plan, BETA, RAMP, updates)
        torch.cuda.synchronize()
        assert updates.tolist() == [ITERS, 0]
        for k in hand:
            assert torch.equal(hand[k], r["shadow"][n][k]), f"{kind}/{dtype} {n}.{k}: the trainer's shadow differs from the launch by hand"
            if kinds[k] == 1:
                assert torch.equal(hand[k], rec[ITERS][k]), (n, k)             # a copy segment holds the last weights
        # and the float64 recurrence over the recorded weights, under the kernel test's rule
        lerped = [k for k in hand if kinds[k] == 0]
        cat = lambda sd: torch.cat([sd[k].reshape(-1).cpu() for k in lerped])
        e0, ws = cat(rec[0]), [cat(rec[i]) for i in range(1, ITERS + 1)]
        want = R.recurrence(e0, ws, BETA, RAMP)
        yard = R.dist(R.recurrence(e0, ws, BETA, RAMP, dtype=torch.float32), want)
        err = R.dist(cat(r["shadow"][n]), want)
        moved = R.dist(e0, want)
        print(f"[ema-shadow] {kind}/{dtype} {n}: {len(lerped)} lerp + {len(hand) - len(lerped)} copy tensors, error {err:.3e}, yardstick {yard:.3e}, "
              f"shadow moved {moved:.3e}")
        assert yard > 0 and err <= R.K * yard
        assert moved > R.MUTANT_FACTOR * R.K * yard                 # the weights moved: a shadow that never updated would miss the bound


def test_attach_rejects_unknown_modules():
    tr, _ = R.make(eg, "pxy", "f32", seed=1)
    with pytest.raises(ValueError, match="'G'"):
        tr.attach_ema()                                            # the pxy trainers have only "P"
    with pytest.raises(ValueError, match="'X'"):
        tr.attach_ema(modules=("X",))
    assert tr.ema is None
    assert tr.attach_ema(modules=("P",)).names == ("P",)


# ---- 4. capture -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["celeba", "dsprites"])
def test_captured_iteration_carries_the_average(kind, eager_runs):
    r = eager_runs(kind, "bf16")
    tr, inp = R.make(eg, kind, "bf16", seed=1)
    tr.inputs = inp
    ema = tr.attach_ema(BETA, ramp=RAMP, modules=r["names"])
    sd0 = tr.state_dict()
    tr.step_resident()                                             # an eager iteration moves the average ...
    assert ema.updates.tolist() == [1, 0]
    inp.enqueue(tr)
    tr.capture(warmup=True, inputs=inp)                            # ... the warm-up is a real step too: the saved state puts everything back,
    tr.load_state_dict(sd0)                                        # as train.TrainRun does before its first replay
    assert ema.updates.tolist() == [0, 0]
    for n in r["names"]:
        for k, v in ema.state_dict(n).items():
            assert torch.equal(v.cpu(), sd0[f"modules.{n}.{k}"]), (n, k)
    with pytest.raises(RuntimeError, match="already captured"):
        tr.attach_ema(BETA, ramp=RAMP)
    losses = torch.stack([tr.step_resident().clone() for _ in range(ITERS)]).cpu()
    assert tr.graph is not None and torch.equal(losses, r["lossB"])
    assert ema.updates.tolist() == r["updates"] == [ITERS, 0]
    for n in r["names"]:
        for k, v in ema.state_dict(n).items():
            assert torch.equal(v, r["shadow"][n][k]), f"{kind} {n}.{k}: captured and eager shadows differ"


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------------------
def test_state_carries_the_average():
    kind = "dsprites"
    plain, _ = R.make(eg, kind, "f32", seed=1)
    # a trainer without an average: exactly the keys it had before there was one (a literal set, not the code under test)
    expect = {f"modules.{n}.{k}" for n, m in plain._state_modules().items() for k in m.state_dict()}
    expect |= {f"adam.{n}.{s}" for n in plain._state_moments() for s in ("m", "v")}
    expect |= {"adam.steps", "meta.kind", "meta.dtype", "meta.lr", "meta.betas", "meta.format"}
    sd_plain = plain.state_dict()
    assert set(sd_plain) == expect

    tr, inp = R.make(eg, kind, "f32", seed=1)
    tr.inputs = inp
    tr.attach_ema(BETA, ramp=RAMP)
    for _ in range(2):
        tr.step_resident()
    sd = tr.state_dict()
    gkeys = list(tr.G.state_dict())
    assert all(f"ema.G.{k}" in sd for k in gkeys) and sd["ema.updates"].tolist() == [2, 0] and sd["ema.updates"].dtype == torch.int32
    assert sd["meta.ema"] == [BETA, RAMP, ["G"]] and sd["meta.format"] == 1
    assert set(sd) == expect | {f"ema.G.{k}" for k in gkeys} | {"ema.updates", "meta.ema", "inputs.seed", "inputs.step", "inputs.sampling", "inputs.flip"}
    assert any(not torch.equal(sd[f"ema.G.{k}"], sd[f"modules.G.{k}"]) for k in gkeys)

    tr2, inp2 = R.make(eg, kind, "f32", seed=77)                  # a fresh trainer from another seed, with the same average attached
    tr2.inputs = inp2
    tr2.attach_ema(BETA, ramp=RAMP)
    tr2.ema.updates[1] = 5                                         # a stale arrival counter must not survive a load
    tr2.load_state_dict(sd)
    sd2 = tr2.state_dict()
    assert set(sd2) == set(sd)
    for k, v in sd.items():
        assert (torch.equal(v, sd2[k]) if isinstance(v, torch.Tensor) else v == sd2[k]), k
    for a, b in zip(tr.step_resident().tolist(), tr2.step_resident().tolist()):           # and both go on alike
        assert a == b
    for k, v in tr.ema.state_tensors().items():
        assert torch.equal(v, tr2.ema.state_tensors()[k]), k

    first = f"ema.G.{gkeys[0]}"
    with pytest.raises(ValueError, match=first.replace(".", r"\.")):
        tr2.load_state_dict({k: v for k, v in sd.items() if k != first})
    for bad in (["x", None, ["G"]], 3, [BETA, RAMP]):              # not [number, number, [names]]: the same error, no TypeError
        with pytest.raises(ValueError, match=r"meta\.ema"):
            tr2.load_state_dict(dict(sd, **{"meta.ema": bad}))
    with pytest.raises(ValueError, match=r"ema\.updates"):
        tr2.load_state_dict({k: v for k, v in sd.items() if k != "ema.updates"})
    with pytest.raises(ValueError, match=r"ema\.G\."):
        tr2.load_state_dict(dict(sd_plain, **{k: sd[k] for k in sd if k.startswith("inputs.")}))      # a state without an average
    tr3, inp3 = R.make(eg, kind, "f32", seed=77)
    tr3.inputs = inp3
    with pytest.raises(ValueError, match=r"meta\.ema"):
        tr3.load_state_dict(sd)                                    # dropping an average silently would be data loss
    for beta, ramp, names in ((0.8, RAMP, ("G",)), (BETA, 3.0, ("G",)), (BETA, RAMP, ("G", "E"))):
        tr3.ema = None
        tr3.attach_ema(beta, ramp=ramp, modules=names)
        full = dict(sd, **{f"ema.E.{k}": v for k, v in tr3.E.state_dict().items()}) if "E" in names else sd
        with pytest.raises(ValueError, match=r"meta\.ema"):
            tr3.load_state_dict(full)


# ---- 6. runs ----------------------------------------------------------------------------------------------------------------------------------
def _pngs(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".png"):
                out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def _run(kind, out_dir, seed, ema=True, resume=None, **kw):
    tr, inp = R.make(eg, kind, "f32", seed=seed)
    if ema:
        tr.attach_ema(BETA, ramp=RAMP)
    args = dict(n_epochs=100, sample_interval=2, seed=3, graph=True, log_capacity=16, **kw)
    if resume is None:
        run = eg.train.TrainRun(kind, tr, inp, out_dir, **args)
    else:
        run = eg.train.TrainRun.resume(resume, kind, tr, inp, out_dir, **args)
    return tr, run


def test_run_writes_the_average_and_its_grids(tmp_path):
    od = str(tmp_path / "A")
    tr, run = _run("celeba", od, 1, ema_samples=True)
    run.run(max_iters=1)                                           # iteration 0 samples and saves
    path = os.path.join(od, "generator_ema_0.pt")
    assert os.path.exists(path) and os.path.exists(os.path.join(od, "checkpoint_0.tar"))
    assert run.files.index(path) == run.files.index(os.path.join(od, "checkpoint_0.tar")) + 1      # behind the script's own file
    assert tr.graph is not None and tr.ema.updates.tolist() == [1, 0]
    G = eg.sampling.load_generator("celeba", path)
    want = tr.ema.state_dict("G")
    got = G.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert any(not torch.equal(want[k], v) for k, v in tr.G.state_dict().items())
    run.run(max_iters=3)
    assert run.batches_done == 4 and tr.ema.updates.tolist() == [4, 0]
    live, avg = _pngs(os.path.join(od, "images")), _pngs(os.path.join(od, "ema", "images"))
    assert set(live) == set(avg) and len(live) == 2 * 11          # iterations 0 and 2: static, original, scaled, varying_c1..8
    for name in live:
        if name.startswith(("original", "scaled")):
            assert live[name] == avg[name], name                   # the two image batches are the run's own
        else:
            assert live[name] != avg[name], name                   # the averaged generator draws something else
    assert all(os.path.join(od, "ema", "images", n) in run.files for n in avg)
    # host discipline: no wait that the run without an average lacks
    tr0, run0 = _run("celeba", str(tmp_path / "plain"), 1, ema=False)
    run0.run(max_iters=1)
    run0.run(max_iters=3)
    assert run.waits == run0.waits
    assert not os.path.exists(str(tmp_path / "plain" / "ema")) and not os.path.exists(str(tmp_path / "plain" / "generator_ema_0.pt"))
    assert live == _pngs(str(tmp_path / "plain" / "images"))       # and the live grids are those of the run without one
    sd, sd0 = tr.state_dict(), tr0.state_dict()
    for k, v in sd0.items():
        assert (torch.equal(v, sd[k]) if isinstance(v, torch.Tensor) else v == sd[k]), k
    with pytest.raises(ValueError, match="ema_samples"):
        _run("celeba", str(tmp_path / "none"), 1, ema=False, ema_samples=True)


def test_run_rejects_average_grids_without_a_grid(tmp_path):
    tr, inp = R.make(eg, "pxy", "f32", seed=1)
    tr.attach_ema(modules=("P",))
    with pytest.raises(ValueError, match="no sample_image"):
        eg.train.TrainRun("pxy", tr, inp, str(tmp_path), n_epochs=1, graph=False, ema_samples=True)


@pytest.mark.parametrize("kind", ["celeba", "dsprites"])
def test_resume_carries_the_average(kind, tmp_path):
    trA, runA = _run(kind, str(tmp_path / "A"), 1)
    runA.run(max_iters=4)
    trB, runB = _run(kind, str(tmp_path / "B"), 1)
    runB.run(max_iters=2)
    path = runB.save()
    del trB, runB
    trB, runB = _run(kind, str(tmp_path / "B"), 77, resume=path)         # fresh modules from another seed
    assert runB.batches_done == 2
    runB.run(max_iters=2)
    sdA, sdB = trA.state_dict(), trB.state_dict()
    assert set(sdA) == set(sdB) and sdA["ema.updates"].tolist() == [4, 0] and any(k.startswith("ema.G.") for k in sdA)
    for k, v in sdA.items():
        assert (torch.equal(v, sdB[k]) if isinstance(v, torch.Tensor) else v == sdB[k]), k
    assert np.array_equal(np.load(str(tmp_path / "A" / "losses.npy")).view(np.uint32), np.load(str(tmp_path / "B" / "losses.npy")).view(np.uint32))
    a = torch.load(str(tmp_path / "A" / "generator_ema_0.pt"), map_location="cpu", weights_only=True)
    b = torch.load(str(tmp_path / "B" / "generator_ema_0.pt"), map_location="cpu", weights_only=True)
    assert list(a) == list(trA.G.state_dict()) and all(torch.equal(a[k], b[k]) for k in a)

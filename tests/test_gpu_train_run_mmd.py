"""The kernel MMD inside a training run on the MI355X: ``TrainRun(..., mmd=quality.MMDPlan(...))`` writes one line of
``mmd.jsonl`` per checkpoint iteration and changes nothing else of the run -- not its waits, lines, losses, checkpoints, trainer state or,
beside the other plans, their ``swd.jsonl`` and ``nn.jsonl``.  The run's own comparisons are bit for bit; the recomputed line holds within
the float64 bound of tests/mmd_refs.py."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import ema_refs
import mmd_refs as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None

RUN = dict(n_epochs=100, sample_interval=1, seed=3, graph=True, log_capacity=16)       # MNIST saves every 10 sample intervals: iterations 0 and 10
SWD = (16, 0, 8, 1, 16)
KEYS = ["bandwidths", "gamma_median", "mean", "mmd2", "mmd2_biased"]


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _run(tmp, name, iters, ema=True, mmd=True, nn=False, swd=False, resume=None, seed=1):
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=seed)
    # the 20 dataset images get the spread of a fresh generator's output (see test_gpu_prdc.py): real and generated rows are then
    # neighbours, and the live and the averaged generator, iteration 0 and iteration 10, score differently
    band = torch.randint(112, 144, tuple(inp.data.shape), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    inp.data.copy_(band.to(inp.data.device))
    if ema:
        tr.attach_ema(0.9, ramp=0.0, modules=("G",))
    kw = dict(RUN, mmd=eg.quality.MMDPlan(16) if mmd else None, nn=eg.quality.NNPlan(16) if nn else None,
              swd=eg.quality.SWDPlan(*SWD) if swd else None)
    od = str(tmp / name)
    if resume is None:
        run = eg.train.TrainRun("mnist", tr, inp, od, **kw)
    else:
        run = eg.train.TrainRun.resume(resume, "mnist", tr, inp, od, **kw)
    run.run(max_iters=iters)
    return tr, run


def _lines(run, name="mmd.jsonl"):
    return open(os.path.join(run.out_dir, name)).read().splitlines()


@pytest.fixture(scope="module")
def scored(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mmd_runs")
    return tmp, _run(tmp, "scored", 11)


def test_run_scores_checkpoint_iterations_and_changes_nothing_else(scored):
    tmp, (tr, run) = scored
    tr0, run0 = _run(tmp, "plain", 11, mmd=False)
    lines = [json.loads(s) for s in _lines(run)]
    print("\n".join(_lines(run)))
    assert [ln["batches_done"] for ln in lines] == [0, 10] and run.files.count(os.path.join(run.out_dir, "mmd.jsonl")) == 1
    for ln in lines:
        assert sorted(ln) == ["G", "G_ema", "batches_done"]
        for key in ("G", "G_ema"):
            got = ln[key]
            assert sorted(got) == KEYS and type(got["gamma_median"]) is int and got["gamma_median"] > 0
            assert got["bandwidths"] == [s * got["gamma_median"] for s in (0.5, 1.0, 2.0)]
            assert len(got["mmd2"]) == len(got["mmd2_biased"]) == 3 and got["mean"] == sum(got["mmd2"]) / 3
            assert all(-1e-12 <= b <= 2 and u <= b for u, b in zip(got["mmd2"], got["mmd2_biased"]))
    assert lines[1]["G"] != lines[1]["G_ema"] and lines[0]["G"] != lines[1]["G"]
    # the live generator's line of iteration 10, from the trainer's weights as the run left them at its end (iteration 10 is its last)
    fake = eg.quality.to_u8(eg.quality.generate("mnist", tr.G, 16, 8, seed=eg.train.mmd_seed(3, 10, 0)))
    real = run.inputs.data[:16]
    assert eg.quality.mmd(real, fake) == lines[1]["G"]
    want = MR.mmd(real.cpu().numpy(), fake.cpu().numpy())
    tol = 8 * MR.tolerance(16)
    assert lines[1]["G"]["gamma_median"] == want["gamma_median"] and lines[1]["G"]["bandwidths"] == want["bandwidths"]
    for name in ("mmd2", "mmd2_biased"):
        assert all(abs(g - w) <= tol for g, w in zip(lines[1]["G"][name], want[name])), name
    assert not os.path.exists(os.path.join(run0.out_dir, "mmd.jsonl"))
    assert run.waits == run0.waits and run.lines == run0.lines
    assert np.array_equal(run.history.view(np.uint32), run0.history.view(np.uint32))
    names = sorted(f for f in os.listdir(run.out_dir) if f.endswith(".pt") and not f.startswith("run_state_"))
    assert names and names == sorted(f for f in os.listdir(run0.out_dir) if f.endswith(".pt") and not f.startswith("run_state_"))
    for f in names:
        a = torch.load(os.path.join(run.out_dir, f), map_location="cpu", weights_only=True)
        b = torch.load(os.path.join(run0.out_dir, f), map_location="cpu", weights_only=True)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), f
    sd, sd0 = tr.state_dict(), tr0.state_dict()
    assert set(sd) == set(sd0)
    for k, v in sd0.items():
        assert (torch.equal(v, sd[k]) if isinstance(v, torch.Tensor) else v == sd[k]), k


def test_all_plans_write_the_lines_each_writes_alone(scored):
    tmp, (_, run) = scored
    _, every = _run(tmp, "every", 11, nn=True, swd=True)
    _, others = _run(tmp, "others", 11, mmd=False, nn=True, swd=True)
    for name in ("swd.jsonl", "nn.jsonl"):
        assert _lines(every, name) == _lines(others, name) and len(_lines(every, name)) == 2
    assert _lines(every) == _lines(run)                            # and the mmd lines of the mmd plan alone
    assert not os.path.exists(os.path.join(others.out_dir, "mmd.jsonl"))
    order = [every.files.index(os.path.join(every.out_dir, n)) for n in ("swd.jsonl", "nn.jsonl", "mmd.jsonl")]
    assert order == sorted(order)


def test_run_without_an_average_scores_the_live_generator_only(tmp_path):
    _, run = _run(tmp_path, "live", 1, ema=False)
    lines = [json.loads(s) for s in _lines(run)]
    assert len(lines) == 1 and sorted(lines[0]) == ["G", "batches_done"]
    tr, inp = ema_refs.make(eg, "pxy", "f32", seed=1)
    with pytest.raises(ValueError, match="mmd: only 'mnist' and 'celeba'"):
        eg.train.TrainRun("pxy", tr, inp, str(tmp_path / "pxy"), n_epochs=1, graph=False, mmd=eg.quality.MMDPlan(16))
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=1)
    with pytest.raises(ValueError, match="mmd: n_images = 64, the dataset has 20 images"):
        eg.train.TrainRun("mnist", tr, inp, str(tmp_path / "big"), n_epochs=1, graph=False, mmd=eg.quality.MMDPlan(64))
    with pytest.raises(ValueError, match="mmd: n_images = 12 is no multiple of the trainer's batch size 8"):
        eg.train.TrainRun("mnist", tr, inp, str(tmp_path / "odd"), n_epochs=1, graph=False, mmd=eg.quality.MMDPlan(12))
    with pytest.raises(ValueError, match="mmd: n_images = 1, the estimate needs"):
        eg.train.TrainRun("mnist", tr, inp, str(tmp_path / "one"), n_epochs=1, graph=False, mmd=eg.quality.MMDPlan(1))
    with pytest.raises(ValueError, match="mmd: .*scales must be"):
        eg.train.TrainRun("mnist", tr, inp, str(tmp_path / "scales"), n_epochs=1, graph=False, mmd=eg.quality.MMDPlan(16, scales=(1.0, 0.0)))


def test_resumed_run_appends_the_line_of_the_uninterrupted_one(scored):
    tmp, (_, run) = scored
    _, part = _run(tmp, "resumed", 5)
    path = part.save()
    assert len(_lines(part)) == 1
    del part
    _, rest = _run(tmp, "resumed", 6, resume=path, seed=77)                    # fresh modules from another seed
    assert rest.batches_done == 11
    assert _lines(rest) == _lines(run)

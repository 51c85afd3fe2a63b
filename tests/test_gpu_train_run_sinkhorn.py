"""The Sinkhorn divergence inside a training run on the MI355X: ``TrainRun(..., sinkhorn=quality.SinkhornPlan(...))`` writes one
line of ``sinkhorn.jsonl`` per checkpoint iteration, after the ``mmd.jsonl`` line, and a resumed run appends the lines of the uninterrupted
one.  The run's own comparisons are bit for bit; the recomputed line holds within the bound of tests/sinkhorn_refs.py."""
import importlib
import json
import os

import pytest
import torch

import ema_refs
import sinkhorn_refs as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None

RUN = dict(n_epochs=100, sample_interval=1, seed=3, graph=True, log_capacity=16)       # MNIST saves every 10 sample intervals: iterations 0 and 10
KEYS = ["divergence", "epsilon", "gamma_median", "iterations", "marginal_error", "ot_xx", "ot_xy", "ot_yy", "relative"]
PLAN = (16, 0.1, 20, 0)


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _run(tmp, name, iters, ema=True, mmd=False, resume=None, seed=1):
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=seed)
    # the 20 dataset images get the spread of a fresh generator's output (see test_gpu_prdc.py): real and generated rows are then neighbours
    band = torch.randint(112, 144, tuple(inp.data.shape), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    inp.data.copy_(band.to(inp.data.device))
    if ema:
        tr.attach_ema(0.9, ramp=0.0, modules=("G",))
    kw = dict(RUN, sinkhorn=eg.quality.SinkhornPlan(*PLAN), mmd=eg.quality.MMDPlan(16) if mmd else None)
    od = str(tmp / name)
    if resume is None:
        run = eg.train.TrainRun("mnist", tr, inp, od, **kw)
    else:
        run = eg.train.TrainRun.resume(resume, "mnist", tr, inp, od, **kw)
    run.run(max_iters=iters)
    return tr, run


def _lines(run, name="sinkhorn.jsonl"):
    return open(os.path.join(run.out_dir, name)).read().splitlines()


@pytest.fixture(scope="module")
def scored(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sinkhorn_runs")
    return tmp, _run(tmp, "scored", 11, mmd=True)


def test_run_scores_checkpoint_iterations_after_the_mmd_line(scored):
    tmp, (tr, run) = scored
    lines = [json.loads(s) for s in _lines(run)]
    print("\n".join(_lines(run)))
    assert [ln["batches_done"] for ln in lines] == [0, 10] and run.files.count(os.path.join(run.out_dir, "sinkhorn.jsonl")) == 1
    for ln in lines:
        assert sorted(ln) == ["G", "G_ema", "batches_done"]
        for key in ("G", "G_ema"):
            got = ln[key]
            assert sorted(got) == KEYS and type(got["gamma_median"]) is int and got["gamma_median"] > 0
            assert got["epsilon"] == 0.1 * got["gamma_median"] and got["iterations"] == 20
            assert got["divergence"] > 0 and got["relative"] == got["divergence"] / got["gamma_median"] and 0 <= got["marginal_error"] < float("inf")
    assert lines[1]["G"] != lines[1]["G_ema"] and lines[0]["G"] != lines[1]["G"]
    order = [run.files.index(os.path.join(run.out_dir, n)) for n in ("mmd.jsonl", "sinkhorn.jsonl")]
    assert order == sorted(order) and len(_lines(run, "mmd.jsonl")) == 2
    # the live generator's line of iteration 10, from the trainer's weights as the run left them at its end (iteration 10 is its last)
    fake = eg.quality.to_u8(eg.quality.generate("mnist", tr.G, 16, 8, seed=eg.train.sinkhorn_seed(3, 10, 0)))
    real = run.inputs.data[:16]
    assert eg.quality.sinkhorn(real, fake, iterations=20) == lines[1]["G"]
    det = {}
    want = SR.sinkhorn(real.cpu().numpy(), fake.cpu().numpy(), iterations=20, detail=det)
    assert lines[1]["G"]["gamma_median"] == want["gamma_median"] and lines[1]["G"]["epsilon"] == want["epsilon"]
    size = max(abs(det[k]).max() for k in "fgpr")
    for name, pots in (("ot_xy", 2), ("ot_xx", 2), ("ot_yy", 2), ("divergence", 4)):
        assert abs(lines[1]["G"][name] - want[name]) <= pots * (det["bound"] + 16 * 2.0 ** -53 * size), name
    tr2, inp2 = ema_refs.make(eg, "mnist", "f32", seed=1)
    with pytest.raises(ValueError, match="sinkhorn: n_images = 64, the dataset has 20 images"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, sinkhorn=eg.quality.SinkhornPlan(64))


def test_run_without_an_average_scores_the_live_generator_only(tmp_path):
    _, run = _run(tmp_path, "live", 1, ema=False)
    lines = [json.loads(s) for s in _lines(run)]
    assert len(lines) == 1 and sorted(lines[0]) == ["G", "batches_done"] and not os.path.exists(os.path.join(run.out_dir, "mmd.jsonl"))


def test_resumed_run_appends_the_lines_of_the_uninterrupted_one(scored):
    tmp, (_, run) = scored
    _, part = _run(tmp, "resumed", 5)
    path = part.save()
    assert len(_lines(part)) == 1
    del part
    _, rest = _run(tmp, "resumed", 6, resume=path, seed=77)                    # fresh modules from another seed
    assert rest.batches_done == 11
    assert _lines(rest) == _lines(run)

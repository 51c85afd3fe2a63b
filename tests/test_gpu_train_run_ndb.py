"""The NDB score inside a training run on the MI355X: ``TrainRun(..., ndb=quality.NDBPlan(...))`` writes one line of
``ndb.jsonl`` per checkpoint iteration, after the ``sinkhorn.jsonl`` line, from bins of the real images that are fitted once; a resumed
run refits them and appends the lines of the uninterrupted one.  Every comparison is exact."""
import importlib
import json
import os

import pytest
import torch

import ema_refs
import kmeans_refs as KR

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None

RUN = dict(n_epochs=100, sample_interval=1, seed=3, graph=True, log_capacity=16)       # MNIST saves every 10 sample intervals: iterations 0 and 10
KEYS = ["bins", "changed_last", "empty_fake", "empty_real", "inertia", "js", "ndb", "ndb_over_bins"]
PLAN = (16, 4, 3, 0)                                               # 16 images, 4 bins, 3 Lloyd iterations


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _run(tmp, name, iters, ema=True, sinkhorn=False, resume=None, seed=1):
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=seed)
    # the 20 dataset images get the spread of a fresh generator's output (see test_gpu_prdc.py): real and generated rows are then neighbours
    band = torch.randint(112, 144, tuple(inp.data.shape), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    inp.data.copy_(band.to(inp.data.device))
    if ema:
        tr.attach_ema(0.9, ramp=0.0, modules=("G",))
    kw = dict(RUN, ndb=eg.quality.NDBPlan(*PLAN), sinkhorn=eg.quality.SinkhornPlan(16, 0.1, 4) if sinkhorn else None)
    od = str(tmp / name)
    if resume is None:
        run = eg.train.TrainRun("mnist", tr, inp, od, **kw)
    else:
        run = eg.train.TrainRun.resume(resume, "mnist", tr, inp, od, **kw)
    run.run(max_iters=iters)
    return tr, run


def _lines(run, name="ndb.jsonl"):
    return open(os.path.join(run.out_dir, name)).read().splitlines()


@pytest.fixture(scope="module")
def scored(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ndb_runs")
    return tmp, _run(tmp, "scored", 11, sinkhorn=True)


def test_run_scores_checkpoint_iterations_after_the_sinkhorn_line(scored):
    tmp, (tr, run) = scored
    lines = [json.loads(s) for s in _lines(run)]
    print("\n".join(_lines(run)))
    assert [ln["batches_done"] for ln in lines] == [0, 10] and run.files.count(os.path.join(run.out_dir, "ndb.jsonl")) == 1
    for ln in lines:
        assert sorted(ln) == ["G", "G_ema", "batches_done"]
        for key in ("G", "G_ema"):
            got = ln[key]
            assert sorted(got) == KEYS and got["bins"] == 4 and 0 <= got["ndb"] <= 4 and got["ndb_over_bins"] == got["ndb"] / 4
            assert 0.0 <= got["js"] <= 1.0 and type(got["inertia"]) is int and got["inertia"] > 0 and type(got["changed_last"]) is int
            assert 0 <= got["empty_real"] < 4 and 0 <= got["empty_fake"] < 4
    assert lines[0]["G"]["inertia"] == lines[1]["G"]["inertia"] == lines[1]["G_ema"]["inertia"]       # ONE fit serves every line
    order = [run.files.index(os.path.join(run.out_dir, n)) for n in ("sinkhorn.jsonl", "ndb.jsonl")]
    assert order == sorted(order) and len(_lines(run, "sinkhorn.jsonl")) == 2
    # the live generator's line of iteration 10, from the trainer's weights as the run left them at its end (iteration 10 is its last)
    fake = eg.quality.to_u8(eg.quality.generate("mnist", tr.G, 16, 8, seed=eg.train.ndb_seed(3, 10, 0)))
    real = run.inputs.data[:16]
    assert eg.quality.ndb(real, fake, bins=4, iterations=3, seed=0) == lines[1]["G"]
    u = eg.quality.bin_uniforms(0, 4).cpu().numpy()
    assert KR.ndb(real.cpu().numpy(), fake.cpu().numpy(), 4, 3, u)[0] == lines[1]["G"]
    assert torch.equal(run.ndb_bins.centres, eg.quality.image_bins(real, 4, 3, seed=0).centres)
    # quality.ndb_generator: one seed for the generated images and for the bins
    fake5 = eg.quality.generate("mnist", tr.G, 16, 8, seed=5)
    got = eg.quality.ndb_generator("mnist", tr.G, run.inputs, n_images=16, batch=8, seed=5, bins=4, iterations=3)
    assert got == eg.quality.ndb(real, fake5, bins=4, iterations=3, seed=5)
    assert got == KR.ndb(real.cpu().numpy(), eg.quality.to_u8(fake5).cpu().numpy(), 4, 3, eg.quality.bin_uniforms(5, 4).cpu().numpy())[0]
    tr2, inp2 = ema_refs.make(eg, "mnist", "f32", seed=1)
    with pytest.raises(ValueError, match="ndb: n_images = 64, the dataset has 20 images"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, ndb=eg.quality.NDBPlan(64))
    with pytest.raises(ValueError, match="ndb: bins = 100"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, ndb=eg.quality.NDBPlan(16))


def test_run_without_an_average_scores_the_live_generator_only(tmp_path):
    _, run = _run(tmp_path, "live", 1, ema=False)
    lines = [json.loads(s) for s in _lines(run)]
    assert len(lines) == 1 and sorted(lines[0]) == ["G", "batches_done"] and not os.path.exists(os.path.join(run.out_dir, "sinkhorn.jsonl"))


def test_resumed_run_appends_the_lines_of_the_uninterrupted_one(scored):
    tmp, (_, run) = scored
    _, part = _run(tmp, "resumed", 5)
    path = part.save()
    assert len(_lines(part)) == 1
    del part
    _, rest = _run(tmp, "resumed", 6, resume=path, seed=77)                    # fresh modules from another seed; the bins are refitted
    assert rest.batches_done == 11
    assert _lines(rest) == _lines(run)

"""The radial power-spectrum score inside a training run on the MI355X: ``TrainRun(..., spectrum=quality.SpectrumPlan(...))``
writes one line of ``spectrum.jsonl`` per checkpoint iteration, after the ``ndb.jsonl`` line, against moments of the real images that are
computed once; a resumed run recomputes them and appends the lines of the uninterrupted one.  Every comparison between device results is
exact; the comparison with numpy takes the dB tolerance of tests/test_gpu_spectrum.py."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import ema_refs
import spectrum_refs as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None

RUN = dict(n_epochs=100, sample_interval=1, seed=3, graph=True, log_capacity=16)       # MNIST saves every 10 sample intervals: iterations 0 and 10
KEYS = ["distance_db", "effect", "fake_db", "gap_db", "high_db", "peak_db", "peak_ring", "real_db", "rings"]
PLAN = (16, 0)                                                     # 16 images


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _run(tmp, name, iters, ema=True, ndb=False, resume=None, seed=1):
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=seed)
    if ema:
        tr.attach_ema(0.9, ramp=0.0, modules=("G",))
    kw = dict(RUN, spectrum=eg.quality.SpectrumPlan(*PLAN), ndb=eg.quality.NDBPlan(16, 4, 3, 0) if ndb else None)
    od = str(tmp / name)
    if resume is None:
        run = eg.train.TrainRun("mnist", tr, inp, od, **kw)
    else:
        run = eg.train.TrainRun.resume(resume, "mnist", tr, inp, od, **kw)
    run.run(max_iters=iters)
    return tr, run


def _lines(run, name="spectrum.jsonl"):
    return open(os.path.join(run.out_dir, name)).read().splitlines()


@pytest.fixture(scope="module")
def scored(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("spectrum_runs")
    return tmp, _run(tmp, "scored", 11, ndb=True)


def test_run_scores_checkpoint_iterations_after_the_ndb_line(scored):
    tmp, (tr, run) = scored
    lines = [json.loads(s) for s in _lines(run)]
    assert [ln["batches_done"] for ln in lines] == [0, 10] and run.files.count(os.path.join(run.out_dir, "spectrum.jsonl")) == 1
    for ln in lines:
        assert sorted(ln) == ["G", "G_ema", "batches_done"]
        for key in ("G", "G_ema"):
            got = ln[key]
            assert sorted(got) == KEYS and got["rings"] == 24 and 1 <= got["peak_ring"] <= 23
            assert all(len(got[k]) == 24 for k in ("real_db", "fake_db", "gap_db", "effect")) and got["distance_db"] >= 0.0
            assert all(np.isfinite(got[k]).all() for k in ("real_db", "fake_db", "gap_db", "effect"))
    assert lines[0]["G"]["real_db"] == lines[1]["G"]["real_db"] == lines[1]["G_ema"]["real_db"]      # ONE set of real moments serves every line
    order = [run.files.index(os.path.join(run.out_dir, n)) for n in ("ndb.jsonl", "spectrum.jsonl")]
    assert order == sorted(order) and len(_lines(run, "ndb.jsonl")) == 2
    # the live generator's line of iteration 10, from the trainer's weights as the run left them at its end (iteration 10 is its last)
    fake = eg.quality.to_u8(eg.quality.generate("mnist", tr.G, 16, 8, seed=eg.train.spectrum_seed(3, 10, 0)))
    real = run.inputs.data[:16]
    assert eg.quality.spectrum(real, fake) == lines[1]["G"]
    assert torch.equal(run.spectrum_real, eg.quality.spectrum_moments(real)[0])
    ref = SR.spectrum(real.cpu().numpy(), fake.cpu().numpy())
    tol = SR.db_tolerance(real.cpu().numpy()) + SR.db_tolerance(fake.cpu().numpy())
    assert np.all(np.abs(np.array(lines[1]["G"]["gap_db"]) - np.array(ref["gap_db"])) <= tol) and ref["peak_ring"] == lines[1]["G"]["peak_ring"]
    # quality.spectrum_generator
    fake5 = eg.quality.generate("mnist", tr.G, 16, 8, seed=5)
    assert eg.quality.spectrum_generator("mnist", tr.G, run.inputs, n_images=16, batch=8, seed=5) == eg.quality.spectrum(real, fake5)
    tr2, inp2 = ema_refs.make(eg, "mnist", "f32", seed=1)
    with pytest.raises(ValueError, match="spectrum: n_images = 64, the dataset has 20 images"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, spectrum=eg.quality.SpectrumPlan(64))
    with pytest.raises(ValueError, match="spectrum: n_images = 12 is no multiple of the trainer's batch size 8"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, spectrum=eg.quality.SpectrumPlan(12))


def test_run_without_an_average_scores_the_live_generator_only(tmp_path):
    _, run = _run(tmp_path, "live", 1, ema=False)
    lines = [json.loads(s) for s in _lines(run)]
    assert len(lines) == 1 and sorted(lines[0]) == ["G", "batches_done"] and not os.path.exists(os.path.join(run.out_dir, "ndb.jsonl"))


def test_resumed_run_appends_the_lines_of_the_uninterrupted_one(scored):
    tmp, (_, run) = scored
    _, part = _run(tmp, "resumed", 5)
    path = part.save()
    assert len(_lines(part)) == 1
    del part
    _, rest = _run(tmp, "resumed", 6, resume=path, seed=77)                    # fresh modules from another seed; the moments are recomputed
    assert rest.batches_done == 11
    assert _lines(rest) == _lines(run)

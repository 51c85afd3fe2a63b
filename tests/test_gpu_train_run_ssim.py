"""The pair diversity (MS-SSIM) inside a training run on the MI355X: ``TrainRun(..., ssim=quality.SSIMPlan(...))`` writes one
line of ``ssim.jsonl`` per checkpoint iteration, after the ``spectrum.jsonl`` line, beside the diversity of the real images, which is
computed once over one pair table; a resumed run recomputes it and appends the lines of the uninterrupted one.  Every comparison between
device results is exact."""
import importlib
import json
import os

import pytest
import torch

import ema_refs

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None

RUN = dict(n_epochs=100, sample_interval=1, seed=3, graph=True, log_capacity=16)       # MNIST saves every 10 sample intervals: iterations 0 and 10
KEYS = ["duplicates", "levels", "ms_ssim", "pairs", "ssim"]
PLAN = (16, 8, 2)                                                  # 16 images, 8 pairs, plan seed 2


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _run(tmp, name, iters, ema=True, spectrum=False, resume=None, seed=1):
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=seed)
    if ema:
        tr.attach_ema(0.9, ramp=0.0, modules=("G",))
    kw = dict(RUN, ssim=eg.quality.SSIMPlan(*PLAN), spectrum=eg.quality.SpectrumPlan(16, 0) if spectrum else None)
    od = str(tmp / name)
    if resume is None:
        run = eg.train.TrainRun("mnist", tr, inp, od, **kw)
    else:
        run = eg.train.TrainRun.resume(resume, "mnist", tr, inp, od, **kw)
    run.run(max_iters=iters)
    return tr, run


def _lines(run, name="ssim.jsonl"):
    return open(os.path.join(run.out_dir, name)).read().splitlines()


@pytest.fixture(scope="module")
def scored(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ssim_runs")
    return tmp, _run(tmp, "scored", 11, spectrum=True)


def test_run_scores_checkpoint_iterations_after_the_spectrum_line(scored):
    tmp, (tr, run) = scored
    lines = [json.loads(s) for s in _lines(run)]
    assert [ln["batches_done"] for ln in lines] == [0, 10] and run.files.count(os.path.join(run.out_dir, "ssim.jsonl")) == 1
    for ln in lines:
        assert sorted(ln) == ["G", "G_ema", "batches_done"]
        for key in ("G", "G_ema"):
            got = ln[key]
            assert sorted(got) == sorted(KEYS + ["gap", "real"]) and sorted(got["real"]) == KEYS
            assert got["levels"] == got["real"]["levels"] == 2 and got["pairs"] == got["real"]["pairs"] == 8
            assert 0.0 <= got["ms_ssim"] <= 1.0 and -1.0 <= got["ssim"] <= 1.0 and got["gap"] == got["ms_ssim"] - got["real"]["ms_ssim"]
    assert lines[0]["G"]["real"] == lines[1]["G"]["real"] == lines[1]["G_ema"]["real"] == run.ssim_real          # ONE real entry serves every line
    order = [run.files.index(os.path.join(run.out_dir, n)) for n in ("spectrum.jsonl", "ssim.jsonl")]
    assert order == sorted(order) and len(_lines(run, "spectrum.jsonl")) == 2
    # the live generator's line of iteration 10, from the trainer's weights as the run left them at its end (iteration 10 is its last)
    fake = eg.quality.generate("mnist", tr.G, 16, 8, seed=eg.train.ssim_seed(3, 10, 2))
    real = eg.quality.real_images("mnist", run.inputs, 16)
    table = eg.quality.pair_table(16, 8, 2, DEV)
    want = eg.quality.diversity(fake, pairs=table)
    want["real"] = eg.quality.diversity(real, n_pairs=8, seed=2)
    want["gap"] = want["ms_ssim"] - want["real"]["ms_ssim"]
    assert want == lines[1]["G"] and want["real"] == eg.quality.diversity(run.inputs.data[:16], pairs=table)
    tr2, inp2 = ema_refs.make(eg, "mnist", "f32", seed=1)
    with pytest.raises(ValueError, match="ssim: n_images = 64, the dataset has 20 images"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, ssim=eg.quality.SSIMPlan(64))
    with pytest.raises(ValueError, match="ssim: n_images = 12 is no multiple of the trainer's batch size 8"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, ssim=eg.quality.SSIMPlan(12))
    with pytest.raises(ValueError, match="ssim: n_pairs = 0 must be at least 1"):
        eg.train.TrainRun("mnist", tr2, inp2, str(tmp / "big"), n_epochs=1, graph=False, ssim=eg.quality.SSIMPlan(16, 0))


def test_run_without_an_average_scores_the_live_generator_only(tmp_path):
    _, run = _run(tmp_path, "live", 1, ema=False)
    lines = [json.loads(s) for s in _lines(run)]
    assert len(lines) == 1 and sorted(lines[0]) == ["G", "batches_done"] and not os.path.exists(os.path.join(run.out_dir, "spectrum.jsonl"))


def test_resumed_run_appends_the_lines_of_the_uninterrupted_one(scored):
    tmp, (_, run) = scored
    _, part = _run(tmp, "resumed", 5)
    path = part.save()
    assert len(_lines(part)) == 1
    del part
    _, rest = _run(tmp, "resumed", 6, resume=path, seed=77)                    # fresh modules from another seed; the real set is scored again
    assert rest.batches_done == 11
    assert _lines(rest) == _lines(run)

"""Data-parallel training runs: ``train.TrainRun`` around the CelebA trainer on two gloo ranks that share the one GPU of the
test box (B = 4 each, ``GradAllReduce(2)``, ``SyncBN(2, rank)``, device inputs sharded by (rank, world)) against one process at B = 8 with
the same seeds.  20 images at a global batch of 8: 3 iterations per epoch, the 4 iterations cross an epoch end.  With all learning rates 0
every iteration is one step of tests/test_gpu_dp.py on a fresh sharded batch, so its loss bound (2e-5) holds per iteration.  The ranks
run once (one spawn of two processes, one of one process: with this process at most three hold the GPU) and every test reads the files
they left."""
import os
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_run_worker  # noqa: E402

pytestmark = pytest.mark.gpu
PORT = 29561
TIME_LIMIT = 420.0


def _spawn(world, port, outdir):
    """the children are joined under a time limit and killed when it runs out; no retry"""
    ctx = mp.spawn(dp_run_worker.run_rank, args=(world, port, outdir), nprocs=world, join=False)
    deadline = time.monotonic() + TIME_LIMIT
    try:
        while not ctx.join(timeout=5.0):
            if time.monotonic() > deadline:
                raise TimeoutError(f"{world} rank(s) did not finish within {TIME_LIMIT:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
        for p in ctx.processes:
            p.join(10)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dp_run"))
    _spawn(2, PORT, d)
    _spawn(1, PORT + 1, d)
    load = lambda name, r, w: torch.load(os.path.join(d, f"{name}_rank{r}_of{w}.pt"), weights_only=True)
    out = {"single": load("lr0", 0, 1)}
    for name in ("lr0", "A", "A2", "B"):
        out[name] = [load(name, r, 2) for r in (0, 1)]
    return out


def _state(res):
    return {k: v for k, v in res.items() if k.startswith("state/modules.") or k.startswith("state/adam.")}


def test_replicas_end_bit_equal(runs):
    for name in ("lr0", "A", "B"):
        r0, r1 = (_state(r) for r in runs[name])
        assert set(r0) == set(r1) and len(r0) > 20
        for k in r0:
            assert torch.equal(r0[k], r1[k]), (name, k)           # BatchNorm running statistics included: every rank runs the sample forward


def test_only_rank_0_writes_and_writes_what_one_process_writes(runs):
    r0, r1 = runs["lr0"]
    single = runs["single"]
    assert r1["files"] == [] and r1["lines"] != [] and r1["waits"] == r0["waits"] == single["waits"]
    assert r0["files"] == single["files"] and r0["present"] == single["present"]
    assert "checkpoint_0.tar" in r0["present"] and "run_state_4.pt" in r0["present"] and "losses.npy" in r0["present"]
    assert any(p.endswith("2.png") for p in r0["present"])
    for k in single:
        if k.startswith("png/images/static") or k.startswith("png/images/varying"):      # the sample grids: seeded draws through equal weights
            assert torch.equal(r0[k], single[k]), k
    assert torch.equal(r0["losses.npy"], r0["history"])                                   # rank 0's shard losses, as documented


def test_progress_line_prefixes_are_those_of_the_global_batch(runs):
    head = lambda ln: ln[:ln.index("[D loss")]
    got, want = [head(ln) for ln in runs["lr0"][0]["lines"]], [head(ln) for ln in runs["single"]["lines"]]
    assert got == want == ["[Epoch 0/2] [Batch 0/3] "]                                    # CelebA prints every 10th iteration
    assert [head(ln) for ln in runs["lr0"][1]["lines"]] == want                           # kept, not printed


def test_mean_of_the_rank_losses_is_the_one_process_loss(runs):
    h0, h1, w = runs["lr0"][0]["history"], runs["lr0"][1]["history"], runs["single"]["history"]
    assert h0.shape == h1.shape == w.shape == (4, 4) and torch.isfinite(w).all()
    mean = (h0.double() + h1.double()) * 0.5
    err = (mean - w.double()).abs()
    print(f"[dp-run] max |mean over ranks - one process| per column: {err.max(0).values.tolist()}")
    assert float(err.max()) <= 2e-5, err
    assert not torch.equal(h0, h1)                                                        # the ranks saw different shards
    assert not torch.equal(w[0], w[1])                                                    # and every iteration a fresh batch


def _diff(a, b):
    if torch.equal(a, b):
        return 0.0
    if a.shape != b.shape:
        return float("inf")
    d = (a.double() - b.double()).abs().max().item()
    return d if d > 0 else float("nan")


def test_resumed_two_rank_run_reproduces_the_uninterrupted_one(runs):
    """the rule of tests/test_gpu_train_run.py::_compare: B equals A bitwise wherever the control A' equals A bitwise, otherwise per tensor
    max |B - A| <= 4 max |A' - A|.  A rank > 0 resumes from rank 0's file, so its loss rows of the iterations before the file are rank
    0's: its history is compared from the resume point on."""
    bitwise, worst = True, (0.0, 0.0)
    for rank in (0, 1):
        A, A2, Bv = runs["A"][rank], runs["A2"][rank], runs["B"][rank]
        assert A["lines"] == Bv["lines"] or A["lines"] != A2["lines"]
        assert Bv["present"] == sorted(set(A["present"]) | {"run_state_2.pt"})          # the directory rank 0 wrote, listed by every rank
        assert set(A) == set(A2) == set(Bv)
        for k in sorted(A):
            if not isinstance(A[k], torch.Tensor):
                continue
            a, c, b = A[k], A2[k], Bv[k]
            if k == "history" and rank > 0:
                a, c, b = a[2:], c[2:], b[2:]
            dc, db = _diff(a, c), _diff(a, b)
            if dc == 0.0:
                assert db == 0.0, f"rank {rank}: {k} resumed differs from uninterrupted by {db}, control is bit-equal"
            else:
                bitwise = False
                assert db <= 4 * dc, f"rank {rank}: {k} resumed differs by {db}, control by {dc}"
                worst = max(worst, (dc, db))
    print(f"[dp-run exact-resume] branch = {'bitwise' if bitwise else 'tolerance'}; max |A' - A| = {worst[0]:.3e}, max |B - A| = {worst[1]:.3e}")
    assert runs["A"][0]["history"].shape == (4, 4) and not torch.equal(runs["A"][0]["history"][2], runs["lr0"][0]["history"][2])

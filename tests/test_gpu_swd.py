"""The sliced Wasserstein distance on the MI355X: every kernel of csrc/swd.hip against the float64 restatement
tests/swd_refs.py under the rounding bound that restatement derives for the stage, the column sort against torch.sort bit for bit, and the
host layer quality.py end to end, alone and inside a training run.  Every bounded comparison prints its largest error / bound ratio."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import ema_refs
import swd_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _ratio(label, got, want, bound):
    """largest |got - want| / bound; the comparison itself is elementwise"""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.all(err <= bound), f"{label}: error {err.max():.3e} above its bound at {int((err > bound).sum())} elements"
    r = float((err / np.maximum(bound, 1e-300)).max())
    print(f"[swd-bound] {label}: max error / bound = {r:.3f}")
    return r


# ---- sort -------------------------------------------------------------------------------------------------------------------------------
def _sort_data(cols, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-50, 50, (cols, n), generator=g).float() * 0.5           # duplicates
    special = torch.tensor([float("inf"), float("-inf"), 0.0, -0.0, float("inf"), -0.0])
    for c in range(cols):
        k = min(n, len(special))
        idx = torch.randperm(n, generator=g)[:k]
        x[c, idx] = special[torch.randperm(len(special), generator=g)[:k]]
    return x


def _sort_sizes():
    T = importlib.import_module("ead-gan_amd").ops.sort_tile_elems()
    return [1, 2, 3, T - 1, T, T + 1, 2 * T, 4 * T + 5]


@pytest.mark.parametrize("cols", [1, 3, 128])
@pytest.mark.parametrize("which", range(8))
def test_sort_columns_equals_torch_sort(which, cols):
    n = _sort_sizes()[which]
    x = _sort_data(cols, n, 1000 * which + cols).to(DEV)
    want = torch.sort(x, dim=1).values
    got = eg.ops.sort_columns(x.clone())
    assert torch.equal(got, want), (n, cols)


def test_sort_columns_with_a_row_stride_and_twice_the_same_bits():
    T = eg.ops.sort_tile_elems()
    n, cols, pad = 2 * T + 3, 5, 7
    x = _sort_data(cols, n + pad, 7).to(DEV)
    buf = x.clone()
    eg.ops.sort_columns(buf, n)                                          # ld = n + 7 > n
    assert torch.equal(buf[:, :n], torch.sort(x[:, :n], dim=1).values)
    assert torch.equal(buf[:, n:].view(torch.int32), x[:, n:].view(torch.int32))          # nothing past n is touched
    again = x.clone()
    eg.ops.sort_columns(again, n)
    assert torch.equal(again.view(torch.int32), buf.view(torch.int32))                     # bitwise, the zeros' signs included
    with pytest.raises(ValueError):
        eg.ops.sort_columns(x.t())
    with pytest.raises(ValueError):
        eg.ops.sort_columns(x, 0)


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H", [(1, 1, 32), (2, 3, 32), (2, 1, 64)])
def test_pyramid_kernels_against_float64(N, C, H):
    x = torch.randn(N, C, H, H, generator=torch.Generator().manual_seed(H + N)) * 0.7 + 0.2
    xd = x.to(DEV)
    coarse = torch.empty(N, C, H // 2, H // 2, device=DEV)
    eg.ops.pyr_down(xd, coarse, N * C, H)
    x64 = x.double().numpy()
    _ratio(f"pyr_down {N}x{C}x{H}", coarse.cpu().numpy(), R.down(x64), R.down_bound(x64))
    fine = xd.clone()
    eg.ops.pyr_up_sub(fine, coarse, N * C, H)
    c64 = coarse.double().cpu().numpy()
    _ratio(f"pyr_up_sub {N}x{C}x{H}", fine.cpu().numpy(), x64 - R.up(c64), R.up_sub_bound(x64, c64))
    pyr = eg.quality.laplacian_pyramid(xd)
    assert [p.shape[-1] for p in pyr] == R.level_sides(H) and torch.equal(pyr[0], fine) and torch.equal(xd, x.to(DEV))
    if H == 32:
        assert torch.equal(pyr[1], coarse)
    # The whole pyramid against the float64 one.  With M = max |x| (the taps are non-negative and sum to 1, so no Gaussian level exceeds M):
    # a down costs 26 u M, an up_sub 11 u (M + M); errors pass through down and up without growing.  Gaussian level 1 is off by <= 26 u M,
    # level 2 by <= 52 u M; a Laplacian level adds its own Gaussian error, the coarser one's and the subtraction: at most 26 + 52 + 22 = 100 u M.
    for got, want in zip(pyr, R.laplacian_pyramid(x64)):
        assert np.abs(got.double().cpu().numpy() - want).max() <= 100 * R.U * np.abs(x64).max()


# ---- patch statistics ---------------------------------------------------------------------------------------------------------------------
def _level(N, C, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, H, H, generator=g) * torch.tensor([0.3, 1.0, 2.5][:C]).view(1, C, 1, 1) + torch.tensor([0.5, -1.0, 4.0][:C]).view(1, C, 1, 1)


def _positions(N, P, H, seed):
    """random legal centres, the first four pinned to the four legal corners"""
    pos = torch.randint(3, H - 3, (N * P, 2), generator=torch.Generator().manual_seed(seed)).int()
    pos[:4] = torch.tensor([[3, 3], [3, H - 4], [H - 4, 3], [H - 4, H - 4]]).int()
    return pos


def _stats(level, pos, P):
    N, C, H, _ = level.shape
    out = torch.empty(C, 2, device=DEV, dtype=torch.float64)
    ws = torch.empty(eg.ops.swd_patch_stats_ws_doubles(C), device=DEV, dtype=torch.float64)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    eg.ops.swd_patch_stats(level.to(DEV).contiguous(), pos.to(DEV).contiguous(), pos.shape[0], P, C, H, ws, out, flag)
    return out.cpu().numpy(), int(flag.item())


@pytest.mark.parametrize("N,P,C,H", [(3, 5, 1, 16), (16, 8, 3, 32), (40, 50, 3, 64)])
def test_patch_stats_against_float64(N, P, C, H):
    level, pos = _level(N, C, H, 11), _positions(N, P, H, 12)
    got, flag = _stats(level, pos, P)
    mean, std = R.stats(R.descriptors(level.double().numpy(), pos.numpy(), P))
    assert flag == 0
    assert np.all(np.abs(got[:, 0] - mean) <= 1e-10 * np.abs(mean)) and np.all(np.abs(got[:, 1] - std) <= 1e-10 * std), (got, mean, std)
    print(f"[swd-bound] patch_stats {N}x{P}x{C}x{H}: max relative error = {max(np.abs(got[:, 0] / mean - 1).max(), np.abs(got[:, 1] / std - 1).max()):.3e}")


def test_patch_stats_flag():
    N, P, C, H = 3, 5, 3, 32
    level, pos = _level(N, C, H, 13), _positions(N, P, H, 14)
    flat = level.clone()
    flat[:, 1] = 0.25
    got, flag = _stats(flat, pos, P)
    assert flag == eg.ops.SWD_FLAG_ZERO_STD and got[1, 1] == 0.0 and got[1, 0] == 0.25 and got[0, 1] > 0
    bad = level.clone()
    y, x = pos[7].tolist()
    bad[7 // P, 2, y + 3, x - 3] = float("inf")                              # a corner pixel of one gathered patch
    assert _stats(bad, pos, P)[1] == eg.ops.SWD_FLAG_NONFINITE
    bad[7 // P, 2, y + 3, x - 3] = float("nan")
    assert _stats(bad, pos, P)[1] == eg.ops.SWD_FLAG_NONFINITE
    out = pos.clone()
    out[9, 1] = H - 3                                                         # one column too far: read clamped, and flagged
    assert _stats(level, out, P)[1] == eg.ops.SWD_FLAG_POSITION


# ---- projection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 128])
@pytest.mark.parametrize("N,P", [(3, 5), (16, 8)])
@pytest.mark.parametrize("C", [1, 3])
def test_projection_against_float64(C, N, P, D):
    H = 32
    level, pos = _level(N, C, H, 21 + C), _positions(N, P, H, 22 + N)
    n_desc = N * P
    W = torch.randn(49 * C, D, generator=torch.Generator().manual_seed(D)).to(DEV)
    eg.ops.swd_unit_columns(W, 49 * C, D)
    W64 = W.double().cpu().numpy()
    assert np.abs(np.sqrt((W64 ** 2).sum(0)) - 1).max() <= 4 * R.U
    desc = R.descriptors(level.double().numpy(), pos.numpy(), P)
    mean, std = R.stats(desc)
    stats = torch.from_numpy(np.stack([mean, std], 1)).to(DEV)
    ws = torch.empty(eg.ops.swd_project_ws_floats(C), device=DEV)
    for ld in (n_desc, n_desc + 4 - n_desc % 4):                                # the scalar and the 16-byte stores
        out = torch.full((D, ld), float("nan"), device=DEV)
        eg.ops.swd_project(level.to(DEV), pos.to(DEV), n_desc, P, C, H, W, D, stats, ws, out, ld)
        want, bound = R.project(desc, W64, mean, std)
        _ratio(f"project C={C} n_desc={n_desc} D={D} ld={ld}", out[:, :n_desc].t().cpu().numpy(), want, bound)
        assert torch.isnan(out[:, n_desc:]).all()                              # nothing past n_desc is written
        # the corners: the first four descriptors are exactly the patches at the image's legal corners
        corner = R.project(R.descriptors(level.double().numpy()[:1], pos.numpy()[:P], P), W64, mean, std)[0][:4]
        assert np.abs(out[:, :4].t().cpu().numpy() - corner).max() <= bound[:4].max()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _two_sets(N, C, H, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(N, C, H, H, generator=g)
    Bt = torch.rand(N, C, H, H, generator=g) * 2 - 1
    Bt = (Bt + torch.roll(Bt, 1, 3)) * 0.5                                    # another patch distribution: neighbours correlate
    return A.to(DEV), Bt.to(DEV)


def _plan_to_numpy(plan):
    return [p.cpu().numpy() for p in plan[0]], [[W.double().cpu().numpy() for W in level] for level in plan[1]]


@pytest.mark.parametrize("N,C,H,P,Rp,D", [(4, 3, 64, 16, 2, 128), (5, 1, 32, 7, 2, 32)])
def test_swd_against_float64_with_explicit_draws(N, C, H, P, Rp, D):
    """The reference takes the draws ``draw_plan`` returns and the Laplacian levels the device formed (each kernel of the pyramid is
    bounded on its own above), so what differs is the statistics (1e-10) and the projections: sorting and the mean absolute difference
    are 1-Lipschitz in the sup norm of the projections, hence |device - reference| <= the sum of the two sets' largest projection
    bounds, which the reference computes."""
    A, Bs = _two_sets(N, C, H, 31)
    plan = eg.quality.draw_plan(5, A.shape, P, Rp, D)
    got = eg.quality.swd(A, Bs, positions=plan[0], directions=plan[1])
    pos, dirs = _plan_to_numpy(plan)
    for l, side in enumerate(R.level_sides(H)):
        assert pos[l].shape == (N * P, 2) and pos[l].dtype == np.int32 and pos[l].min() >= 3 and pos[l].max() < side - 3
        assert len(dirs[l]) == Rp and all(np.abs(np.sqrt((W ** 2).sum(0)) - 1).max() <= 4 * R.U for W in dirs[l])
    la = [p.double().cpu().numpy() for p in eg.quality.laplacian_pyramid(A)]
    lb = [p.double().cpu().numpy() for p in eg.quality.laplacian_pyramid(Bs)]
    want, mean, slack = R.swd_levels(la, lb, pos, dirs, P)
    assert sorted(got["levels"]) == sorted(want) and all(isinstance(v, float) for v in got["levels"].values())
    worst = 0.0
    for side, v in want.items():
        assert v > 100 * slack                                                 # two different distributions: far from zero on the bound's scale
        assert abs(got["levels"][side] - v) <= slack, (side, got["levels"][side], v, slack)
        worst = max(worst, abs(got["levels"][side] - v) / slack)
    assert abs(got["mean"] - mean) <= slack
    print(f"[swd-bound] swd end to end {N}x{C}x{H}: max |device - reference| / slack = {worst:.4f} (slack {slack:.3e}, mean {mean:.3f})")
    # seeds
    kw = dict(patches_per_image=P, repeats=Rp, dirs=D)
    s5 = eg.quality.swd(A, Bs, seed=5, **kw)
    assert s5 == got == eg.quality.swd(A, Bs, seed=5, **kw)                  # draw_plan returned the tensors swd draws; two calls, the same bits
    assert eg.quality.swd(A, Bs, seed=6, **kw)["mean"] != got["mean"]
    again = eg.quality.draw_plan(5, A.shape, P, Rp, D)
    assert all(torch.equal(a, b) for a, b in zip(plan[0], again[0])) and all(torch.equal(a, b) for x, y in zip(plan[1], again[1]) for a, b in zip(x, y))
    assert eg.quality.swd(A, A, seed=5, **kw)["mean"] == 0.0


def test_swd_refuses_what_it_cannot_score():
    A, Bs = _two_sets(2, 3, 32, 41)
    flat = Bs.clone()
    flat[:, 2] = -1.0
    with pytest.raises(ValueError, match="fake set at level 32: a channel without variance"):
        eg.quality.swd(A, flat, patches_per_image=4, repeats=1, dirs=8)
    nan = A.clone()
    nan[1, 0] = float("nan")
    with pytest.raises(ValueError, match="real set"):
        eg.quality.swd(nan, Bs, patches_per_image=4, repeats=1, dirs=8)
    with pytest.raises(ValueError, match="one shape"):
        eg.quality.swd(A, Bs[:1])
    with pytest.raises(ValueError, match="C = 1 or 3"):
        eg.quality.swd(A[:, :2], Bs[:, :2])
    plan = eg.quality.draw_plan(0, A.shape, 4, 1, 8)
    with pytest.raises(ValueError, match="together"):
        eg.quality.swd(A, Bs, positions=plan[0])
    bad = [p.clone() for p in plan[0]]
    bad[1][3, 0] = 1
    with pytest.raises(ValueError, match="level 16: a patch centre outside"):
        eg.quality.swd(A, Bs, positions=bad, directions=plan[1])
    sprites = torch.rand(2, 1, 64, 64, device=DEV)                              # the sprite shapes are scored by swd itself
    assert eg.quality.swd(sprites, sprites.flip(0) ** 2, patches_per_image=4, repeats=1, dirs=8)["mean"] > 0


# ---- generators and runs ------------------------------------------------------------------------------------------------------------------
def _mnist_data(n=20, seed=4):
    return torch.randint(0, 256, (n, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_swd_generator_on_a_fresh_mnist_generator():
    torch.manual_seed(1)
    G = eg.mnist.Generator().to(DEV)
    data = _mnist_data()
    before = {k: v.clone() for k, v in G.state_dict().items()}
    kw = dict(n_images=16, batch=8, seed=2, patches_per_image=16, repeats=2, dirs=32)
    a = eg.quality.swd_generator("mnist", G, data, **kw)
    b = eg.quality.swd_generator("mnist", G, data, **kw)
    assert a == b and sorted(a["levels"]) == [16, 32] and all(np.isfinite(v) and v > 0 for v in a["levels"].values()) and np.isfinite(a["mean"])
    after = G.state_dict()
    assert G.training and list(after) == list(before) and all(torch.equal(before[k], after[k]) for k in before)
    assert eg.quality.swd_generator("mnist", G.eval(), data, **kw) != a           # the generator's current mode is the one that runs
    assert all(torch.equal(before[k], v) for k, v in G.state_dict().items())
    G.train()
    with pytest.raises(ValueError, match="multiple of batch"):
        eg.quality.swd_generator("mnist", G, data, **dict(kw, n_images=12))
    real = eg.quality.real_images("mnist", data, 16)
    assert (real - (data[:16].float() * (2.0 / 255.0) - 1.0)).abs().max() <= 2 ** -23          # one rounding apart at most (fused or not), |v| <= 1
    imgs = eg.quality.generate("mnist", G, 16, 8, seed=2)
    assert imgs.shape == (16, 1, 32, 32) and torch.equal(imgs, eg.quality.generate("mnist", G, 16, 8, seed=2))
    assert not torch.equal(imgs, eg.quality.generate("mnist", G, 16, 8, seed=3)) and not torch.equal(imgs[:8], imgs[8:])


RUN = dict(n_epochs=100, sample_interval=1, seed=3, graph=True, log_capacity=16)       # MNIST saves every 10 sample intervals: iterations 0 and 10
PLAN = (16, 0, 8, 1, 16)
_runs = {}


def _run(tmp, name, iters, ema=True, swd=PLAN, resume=None, seed=1):
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=seed)
    if ema:
        tr.attach_ema(0.9, ramp=0.0, modules=("G",))
    od = str(tmp / name)
    if resume is None:
        run = eg.train.TrainRun("mnist", tr, inp, od, swd=None if swd is None else eg.quality.SWDPlan(*swd), **RUN)
    else:
        run = eg.train.TrainRun.resume(resume, "mnist", tr, inp, od, swd=None if swd is None else eg.quality.SWDPlan(*swd), **RUN)
    run.run(max_iters=iters)
    return tr, run


def _lines(run):
    return open(os.path.join(run.out_dir, "swd.jsonl")).read().splitlines()


@pytest.fixture(scope="module")
def scored(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("swd_runs")
    return tmp, _run(tmp, "scored", 11)


def test_run_scores_checkpoint_iterations_and_changes_nothing_else(scored):
    tmp, (tr, run) = scored
    tr0, run0 = _run(tmp, "plain", 11, swd=None)
    lines = [json.loads(s) for s in _lines(run)]
    assert [ln["batches_done"] for ln in lines] == [0, 10] and run.files.count(os.path.join(run.out_dir, "swd.jsonl")) == 1
    for ln in lines:
        assert sorted(ln) == ["G", "G_ema", "batches_done"]
        for key in ("G", "G_ema"):
            assert sorted(ln[key]["levels"]) == ["16", "32"] and np.isfinite(ln[key]["mean"]) and ln[key]["mean"] > 0
    assert lines[1]["G"] != lines[1]["G_ema"] and lines[0]["G"] != lines[1]["G"]
    assert not os.path.exists(os.path.join(run0.out_dir, "swd.jsonl"))
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


def test_run_without_an_average_scores_the_live_generator_only(tmp_path):
    _, run = _run(tmp_path, "live", 1, ema=False)
    lines = [json.loads(s) for s in _lines(run)]
    assert len(lines) == 1 and sorted(lines[0]) == ["G", "batches_done"]
    tr, inp = ema_refs.make(eg, "pxy", "f32", seed=1)
    with pytest.raises(ValueError, match="only 'mnist' and 'celeba'"):
        eg.train.TrainRun("pxy", tr, inp, str(tmp_path / "pxy"), n_epochs=1, graph=False, swd=eg.quality.SWDPlan(16))
    tr, inp = ema_refs.make(eg, "mnist", "f32", seed=1)
    with pytest.raises(ValueError, match="the dataset has 20 images"):
        eg.train.TrainRun("mnist", tr, inp, str(tmp_path / "big"), n_epochs=1, graph=False, swd=eg.quality.SWDPlan(64))
    with pytest.raises(ValueError, match="no multiple of the trainer's batch size 8"):
        eg.train.TrainRun("mnist", tr, inp, str(tmp_path / "odd"), n_epochs=1, graph=False, swd=eg.quality.SWDPlan(12))


def test_resumed_run_appends_the_line_of_the_uninterrupted_one(scored):
    tmp, (_, run) = scored
    _, part = _run(tmp, "resumed", 5)
    path = part.save()
    assert len(_lines(part)) == 1
    del part
    _, rest = _run(tmp, "resumed", 6, resume=path, seed=77)                    # fresh modules from another seed
    assert rest.batches_done == 11
    assert _lines(rest) == _lines(run)

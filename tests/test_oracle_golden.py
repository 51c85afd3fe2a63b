"""Oracle (CPU restatement) vs golden vectors produced by the reference itself (oracle/make_golden.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from oracle import celeba_oracle as co
from oracle import mnist_oracle as mo


def check_probes(prefix, tensors, gold, rtol, atol, noise_floor=0.0, noise_grads=None, init=None, max_step=0.0):
    """tensors: name -> tensor; compares head/sum/abs fingerprints.  Scale-aware: tolerances are relative
    to the mean |value| of the tensor so that near-zero entries do not dominate.

    Post-Adam state (noise_grads = prefix of the gradient probes): where the golden gradient is rounding noise (mean |g| below 1e-8,
    the floor of the gradient check: conv biases in front of a BatchNorm), a first Adam step moves every entry by up to its learning
    rate in a direction that rounding picks, so the sum and |sum| fingerprints depend on the host's BLAS kernels.  For those tensors
    they are replaced by what holds on every host: each entry lies within max_step (the summed learning rates) of its seeded value in
    init (the head check, sized for such moves, stays)."""
    for k, v in tensors.items():
        t = v.detach().double().flatten().cpu()
        ab = float(gold[f"{prefix}/{k}/abs"])
        scale = ab / max(t.numel(), 1)
        if scale < noise_floor:      # e.g. gradients of conv biases in front of a BatchNorm: pure rounding noise
            continue
        tol = rtol * scale + atol
        np.testing.assert_allclose(t[:8].numpy(), gold[f"{prefix}/{k}/head"], rtol=0, atol=8 * tol, err_msg=f"{prefix}/{k}")
        g_abs = f"{noise_grads}/{k}/abs"
        if noise_grads is not None and g_abs in gold and float(gold[g_abs]) / max(t.numel(), 1) < 1e-8:
            moved = (t - init[k].detach().double().flatten()).abs().max().item()
            assert moved <= max_step * (1 + 1e-3), f"{prefix}/{k} moved {moved} > {max_step}"
            continue
        assert abs(t.abs().sum().item() - ab) <= rtol * ab + atol * t.numel() ** 0.5, f"{prefix}/{k} abs"
        assert abs(t.sum().item() - float(gold[f"{prefix}/{k}/sum"])) <= rtol * ab + atol * t.numel() ** 0.5, f"{prefix}/{k} sum"


def test_celeba_step_matches_reference():
    gold = np.load(os.path.join(GOLDEN, "celeba_b4_s3.npz"))
    B, steps, seed = int(gold["B"]), int(gold["steps"]), int(gold["seed"])
    torch.set_num_threads(8)
    orc = co.CelebAOracle(seed=seed)
    init_G, init_D = ({k: v.detach().clone() for k, v in m.items()} for m in (orc.G, orc.D))
    lr = lambda opt: opt.param_groups[0]["lr"]
    rng = np.random.RandomState(seed)
    real = co.synthetic_real(B * steps, seed=int(gold["real_seed"])).view(steps, B, 3, 64, 64)
    for i in range(steps):
        z, code, labels = co.draw_step_inputs(rng, B)
        out = orc.train_step(real[i], z, code, labels)
        # step 0 is a pure function of the seeded init; later steps pass through Adam's first-step
        # sign amplification of rounding noise, hence the looser bound.  Its size depends on the host's BLAS kernels: step 1 moved
        # by up to 2e-5 where the golden file was made and by 0.8e-3 - 1.2e-3 on hosts whose MKL takes other kernels (AMD, AVX2 path).
        tol = (2e-6, 2e-3, 5e-3)[i]
        for k in ("g_loss", "d_loss", "info_loss"):
            assert abs(out[k] - gold[k][i]) < tol, (i, k, out[k], gold[k][i])
        if i == 0:
            # gradients left by the info step: smooth quantities -> tight
            check_probes("gG1", {k: v.grad for k, v in orc.G.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("gD1", {k: v.grad for k, v in orc.D.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            # post-Adam state: entries with ~0 gradient move by +-lr on rounding noise -> atol 2.5e-3 on heads
            check_probes("G1", orc.G, gold, 2e-3, 3e-4, noise_grads="gG1", init=init_G, max_step=lr(orc.opt_G) + lr(orc.opt_info))
            check_probes("D1", orc.D, gold, 2e-3, 3e-4, noise_grads="gD1", init=init_D, max_step=lr(orc.opt_D) + lr(orc.opt_info))


def grid_rounding_slack(img, theta):
    """How far a bilinear warp may move when only the float32 rounding of its sampling grid differs.  affine_grid forms each grid
    coordinate as a three-term dot product (base point x, y, 1 against a row of theta) in a BLAS batched matmul whose kernel, and so
    whose rounding, depends on the host CPU: two hosts may differ by 2 * gamma_3 ~ 6 units of rounding (2**-24) of the sum of |terms|,
    and grid_sample rounds g + 1 on its way to pixels: 8 units of |terms| + 1 in all.  An output element moves by its slope along its
    own grid point times that: per channel, d out / d grid by autograd."""
    N, C, H, W = img.shape
    grid = F.affine_grid(theta, [N, C, H, W], align_corners=False).detach()
    xs, ys = (torch.arange(W) * 2 + 1) / W - 1, (torch.arange(H) * 2 + 1) / H - 1
    base = torch.stack((xs.view(1, W).expand(H, W), ys.view(H, 1).expand(H, W), torch.ones(H, W)), -1).abs()    # |x|, |y|, 1
    terms = torch.einsum("hwi,ndi->nhwd", base.double(), theta.abs().double())
    dgrid = 8 * 2.0 ** -24 * (terms + 1)
    slack = torch.empty(N, C, H, W, dtype=torch.float64)
    for c in range(C):
        g = grid.clone().requires_grad_()
        F.grid_sample(img[:, c:c + 1], g, mode="bilinear", padding_mode="border", align_corners=False).sum().backward()
        slack[:, c] = (g.grad.abs().double() * dgrid).sum(-1)
    return slack.numpy()


def test_celeba_affine_functions_match_reference():
    gold = np.load(os.path.join(GOLDEN, "celeba_affine.npz"))
    code = torch.tensor(gold["code"])
    A = co.get_matrix(code[:, :5])
    np.testing.assert_allclose(A.numpy(), gold["A"], rtol=1e-6, atol=1e-7)
    img = co.synthetic_real(4, seed=int(gold["img_seed"]))
    warped = co.warp(img, A[:4, 0:2])
    err = np.abs(warped.numpy() - gold["warped"])
    tol = 1e-6 + 1e-5 * np.abs(gold["warped"]) + grid_rounding_slack(img, A[:4, 0:2])
    assert (err <= tol).all(), f"{(err > tol).sum()} of {err.size} elements off, worst {err.max():.3g}"
    rc = torch.tensor(gold["real_code"], requires_grad=True)
    tc = torch.tensor(gold["trans_code"], requires_grad=True)
    pred = co.affine_regularzier(rc, tc)
    np.testing.assert_allclose(pred.detach().numpy(), gold["pred"], rtol=1e-4, atol=1e-5)
    (pred * torch.tensor(gold["w"])).sum().backward()
    np.testing.assert_allclose(rc.grad.numpy(), gold["d_real"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(tc.grad.numpy(), gold["d_trans"], rtol=1e-3, atol=1e-4)


def test_mnist_step_matches_reference():
    gold = np.load(os.path.join(GOLDEN, "mnist_b8_s3.npz"))
    B, steps, seed = int(gold["B"]), int(gold["steps"]), int(gold["seed"])
    torch.set_num_threads(8)
    orc = mo.MnistOracle(seed=seed, mlp=mo.make_approximator(int(gold["mlp_seed"])))
    rng = np.random.RandomState(seed)
    real = mo.synthetic_real(B * steps, seed=int(gold["real_seed"])).view(steps, B, 1, 32, 32)
    for i in range(steps):
        z, code, labels = mo.draw_step_inputs(rng, B)
        out = orc.train_step(real[i], z, code, labels)
        tol = (2e-6, 1e-3, 1e-2)[i]
        for k in ("g_loss", "d_loss", "info_loss"):
            assert abs(out[k] - gold[k][i]) < tol, (i, k, out[k], gold[k][i])
        if i == 0:
            check_probes("gG1", {k: v.grad for k, v in orc.G.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("gE1", {k: v.grad for k, v in orc.E.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("G1", orc.G, gold, 2e-3, 3e-4)
            check_probes("D1", orc.D, gold, 2e-3, 3e-4)
            check_probes("E1", orc.E, gold, 2e-3, 3e-4)


def test_mnist_affine_functions_match_reference():
    gold = np.load(os.path.join(GOLDEN, "mnist_affine.npz"))
    mlp = mo.make_approximator(int(gold["mlp_seed"]))
    A = mo.get_matrix(torch.tensor(gold["code"]))
    np.testing.assert_allclose(A.numpy(), gold["A"], rtol=1e-6, atol=1e-7)
    rc = torch.tensor(gold["real_code"], requires_grad=True)
    tc = torch.tensor(gold["trans_code"], requires_grad=True)
    pred = mo.affine_regularizer(mlp, rc, tc)
    np.testing.assert_allclose(pred.detach().numpy(), gold["pred"], rtol=1e-4, atol=1e-5)
    (pred * torch.tensor(gold["w"])).sum().backward()
    np.testing.assert_allclose(rc.grad.numpy(), gold["d_real"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(tc.grad.numpy(), gold["d_trans"], rtol=1e-3, atol=1e-4)


def test_dsprites_step_matches_reference():
    from oracle import dsprites_oracle as do
    gold = np.load(os.path.join(GOLDEN, "dsprites_b8_s3.npz"))
    B, steps, seed = int(gold["B"]), int(gold["steps"]), int(gold["seed"])
    torch.set_num_threads(8)
    orc = do.DspritesOracle(seed=seed, pxy=do.make_encoder_pxy(int(gold["pxy_seed"])))
    rng = np.random.RandomState(seed)
    sprites = do.synthetic_sprites(B * steps, seed=int(gold["sprite_seed"])).view(steps, B, 64, 64)
    names = ("d_loss", "g_loss", "info_loss", "affine_loss", "relative_cat_loss")
    for i in range(steps):
        out = orc.train_step(sprites[i], *do.draw_step_inputs(rng, B))
        tol = (3e-6, 1e-3, 1e-2)[i]
        for k in names:
            assert abs(out[k] - gold[k][i]) < tol, (i, k, out[k], gold[k][i])
        if i == 0:
            check_probes("gG1", {k: v.grad for k, v in orc.G.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("gE1", {k: v.grad for k, v in orc.E.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("G1", orc.G, gold, 2e-3, 3e-4)
            check_probes("D1", orc.D, gold, 2e-3, 3e-4)
            check_probes("E1", orc.E, gold, 2e-3, 3e-4)


def test_colored_dsprites_step_matches_reference():
    from oracle import dsprites_oracle as do
    gold = np.load(os.path.join(GOLDEN, "colored_b8_s3.npz"))
    B, steps, seed = int(gold["B"]), int(gold["steps"]), int(gold["seed"])
    torch.set_num_threads(8)
    orc = do.ColoredOracle(seed=seed, pxy=do.make_encoder_pxy(int(gold["pxy_seed"]), ch=3, pxy_out=6))
    rng = np.random.RandomState(seed)
    sprites = do.synthetic_sprites(B * steps, seed=int(gold["sprite_seed"])).view(steps, B, 64, 64)
    for i in range(steps):
        out = orc.train_step(sprites[i], *do.draw_colored_inputs(rng, B))
        tol = (3e-6, 1e-3, 1e-2)[i]
        assert abs(out["d_loss"] - gold["d_loss"][i]) < tol and abs(out["g_loss"] - gold["g_loss"][i]) < tol
        assert abs(out["info_loss"] - (gold["cat_loss"][i] + gold["cont_loss"][i])) < tol
        assert abs(out["affine_loss"] - gold["affine_color_loss"][i]) < tol
        assert abs(out["relative_cat_loss"] - gold["relative_cat_loss"][i]) < tol
        if i == 0:
            check_probes("gG1", {k: v.grad for k, v in orc.G.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("gE1", {k: v.grad for k, v in orc.E.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)


def test_pxy_stage1_step_matches_reference():
    """dSprites/pxy.py (stage-1 trainer of Encoder_pxy): oracle vs the loop body run through the harness"""
    from oracle import dsprites_oracle as do
    gold = np.load(os.path.join(GOLDEN, "pxy_b8_s3.npz"))
    B, steps, seed = int(gold["B"]), int(gold["steps"]), int(gold["seed"])
    torch.set_num_threads(8)
    orc = do.PxyOracle(seed=seed)
    rng = np.random.RandomState(seed)
    sprites = do.synthetic_sprites(B * steps, seed=int(gold["sprite_seed"])).view(steps, B, 64, 64)
    for i in range(steps):
        out = orc.train_step(sprites[i], do.draw_pxy_inputs(rng, B))
        assert abs(out["affine_loss"] - gold["affine_loss"][i]) < (2e-6, 3e-4, 2e-3)[i], (i, out, gold["affine_loss"][i])
        if i == 0:
            check_probes("gP1", {k: v.grad for k, v in orc.P.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("P1", orc.P, gold, 2e-3, 3e-4)


def test_pxy_color_stage1_step_matches_reference():
    """colored_dSprites/pxy_color.py (stage-1 trainer of the colored Encoder_pxy): oracle vs the loop body run through the harness"""
    from oracle import dsprites_oracle as do
    gold = np.load(os.path.join(GOLDEN, "pxy_color_b8_s3.npz"))
    B, steps, seed = int(gold["B"]), int(gold["steps"]), int(gold["seed"])
    torch.set_num_threads(8)
    orc = do.PxyColorOracle(seed=seed)
    rng = np.random.RandomState(seed)
    sprites = do.synthetic_sprites(B * steps, seed=int(gold["sprite_seed"])).view(steps, B, 64, 64)
    for i in range(steps):
        out = orc.train_step(sprites[i], *do.draw_pxy_color_inputs(rng, B))
        assert abs(out["affine_loss"] - gold["affine_loss"][i]) < (2e-6, 3e-4, 2e-3)[i], (i, out, gold["affine_loss"][i])
        if i == 0:
            check_probes("gP1", {k: v.grad for k, v in orc.P.items() if getattr(v, "grad", None) is not None}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("P1", orc.P, gold, 2e-3, 3e-4)


def test_approximator_fit_matches_reference():
    """MNIST/approximate_rpqmnxy.py (fit of the affine-inverse MLP): oracle vs the script's __main__ loop run through the harness"""
    gold = np.load(os.path.join(GOLDEN, "approximator_fit_s5.npz"))
    steps, seed, B = int(gold["steps"]), int(gold["seed"]), int(gold["B"])
    torch.set_num_threads(8)
    orc = mo.ApproximatorOracle(seed=seed)
    rng = np.random.RandomState(seed)
    for i in range(steps):
        out = orc.train_step(mo.draw_approximator_inputs(rng, B))
        assert abs(out["affine_loss"] - gold["affine_loss"][i]) < (2e-6, 1e-4, 3e-4, 1e-3, 2e-3)[i], (i, out, gold["affine_loss"][i])
        if i == 0:
            check_probes("gM1", {k: v.grad for k, v in orc.mlp.items()}, gold, 1e-2, 1e-9, noise_floor=1e-8)
            check_probes("M1", {k: v.detach() for k, v in orc.mlp.items()}, gold, 2e-3, 3e-4)


def _plan_matches_golden(plan_of, gold, kind):
    import json
    n = int(gold["n"])
    plan = plan_of(kind, n)
    saves = json.loads(str(gold[f"{kind}/saves"]))
    assert [p[0] for p in plan] == [s[0].rsplit("/", 1)[0] for s in saves]
    assert [p[2] for p in plan] == [s[3] for s in saves]
    assert all(s[1] == n and s[2] is True for s in saves)           # every file: nrow = n, normalize=True
    calls = [p[1] for p in plan if p[1] is not None]
    assert len(calls) == len([k for k in gold.files if k.startswith(kind + "/call") and k.endswith("/in0")])
    for i, inputs in enumerate(calls):
        for j, a in enumerate(inputs):
            g = gold[f"{kind}/call{i}/in{j}"]
            assert tuple(a.shape) == g.shape and np.array_equal(np.asarray(a, dtype=np.float32), g), (kind, i, j)
        assert f"{kind}/call{i}/in{len(inputs)}" not in gold.files


@pytest.mark.parametrize("kind", ["mnist_train", "mnist_tool", "celeba_train", "celeba_tool", "dsprites_train", "colored_train"])
def test_sample_plans_match_reference(kind):
    """sample_image of the six scripts: the oracle's plan AND the product's host-side plan equal what the reference functions
    fed their generator / writer (recorded by oracle/ref_harness.record_sample_image into tests/golden/sample_plans.npz)"""
    import importlib
    from oracle import sampling_oracle as so
    gold = np.load(os.path.join(GOLDEN, "sample_plans.npz"))
    _plan_matches_golden(lambda k, n: [(p["path"], p["inputs"], p["gridded"]) for p in so.sample_plan(k, n, np.random.RandomState(0))], gold, kind)
    sampling = importlib.import_module("ead-gan_amd.sampling")
    _plan_matches_golden(lambda k, n: sampling.sample_inputs(k, n, np.random.RandomState(0)), gold, kind)


def test_grid_oracle_hand_checked():
    """make_grid / save_image restatement (torchvision 0.8.2, parity unpinned: see oracle/sampling_oracle.py) on cases small enough to
    verify by hand: geometry, single-channel replication, where normalisation applies, rounding of the quantiser"""
    from oracle import sampling_oracle as so
    t = torch.arange(5 * 1 * 2 * 3, dtype=torch.float32).view(5, 1, 2, 3)
    g = so.make_grid(t, nrow=3, padding=2)
    assert g.shape == (3, 2 * 4 + 2, 3 * 5 + 2)
    assert torch.equal(g[0], g[1]) and torch.equal(g[1], g[2])
    assert torch.equal(g[0, 2:4, 2:5], t[0, 0]) and torch.equal(g[0, 6:8, 7:10], t[4, 0])
    assert float(g[0, :2].abs().sum()) == 0 and float(g[0, 6:8, 12:15].abs().sum()) == 0      # border and the unused sixth cell
    assert so.make_grid(t[:1], nrow=3).shape == (3, 2, 3)                                           # one image: no border
    # 4-D + normalize: images span [0, 1), gaps stay 0 -> black; value k/29 -> floor(k/(29+1e-5)*255 + .5)
    b = so.to_uint8_hwc(t, nrow=3, normalize=True)
    assert b.shape == (10, 17, 3) and b[0, 0, 0] == 0 and b[2, 2, 0] == 0 and b[7, 9, 0] == 255 and b[7, 8, 0] == int(28 / (29 + 1e-5) * 255 + 0.5) and b[2, 4, 1] == int(2 / (29 + 1e-5) * 255 + 0.5)
    # grid first, then normalize=True: the gaps take part -> with images in [1, 2] the gaps (0) are the minimum, images start at 127/128
    b2 = so.to_uint8_hwc(so.make_grid(t / 29 + 1, nrow=3), nrow=3, normalize=True)
    assert b2[0, 0, 0] == 0 and b2[2, 2, 0] == int(np.float32(1) / np.float32(2 + 1e-5) * 255 + 0.5) and b2[7, 9, 0] == 255


def test_png_encoder_roundtrip():
    """host logic: the PNG container written for the grids decodes (PIL, independent decoder) to the same bytes"""
    import importlib
    import io
    PIL = pytest.importorskip("PIL.Image")
    sampling = importlib.import_module("ead-gan_amd.sampling")
    rng = np.random.RandomState(0)
    for shape in ((7, 5, 3), (64, 33, 3), (9, 4, 1)):
        a = rng.randint(0, 256, shape).astype(np.uint8)
        im = np.asarray(PIL.open(io.BytesIO(sampling.encode_png(a))))
        assert np.array_equal(im.reshape(shape), a)

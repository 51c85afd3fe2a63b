"""MIG and FactorVAE of dSprites / colored-dSprites encoders on the MI355X (ead-gan_amd/score.py, csrc/score.hip) against the reference's
own score/ scripts, recorded in tests/golden/score_{dsprites,colored}.npz by tests/make_score_golden.py."""
import importlib
import os
import time

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import score_data as sd

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("dsprites", "colored")
eg = None


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_{kind}.npz"))


def sprites(g):
    n = int(np.prod(g["sizes"]))
    return np.unpackbits(g["sprites_bits"], axis=1)[:, :4096].reshape(n, 64, 64)


def ref_rows(cat, cols):
    return np.concatenate([cat.astype(np.float64)[:, None], cols.astype(np.float64)], 1)


def encoders(kind, g):
    mod = eg.colored if kind == "colored" else eg.dsprites
    P, E = mod.Encoder_pxy(), mod.Encoder()
    s_pxy, s_enc = (int(s) for s in g["weight_seeds"])
    psd = sd.make_weights(P.state_dict(), s_pxy, float(g["cat_scale"]))
    esd = sd.make_weights(E.state_dict(), s_enc, float(g["cat_scale"]))
    assert np.array_equal(sd.checksums(psd), g["pxy_checksums"]) and np.array_equal(sd.checksums(esd), g["enc_checksums"])
    P.load_state_dict(psd)
    E.load_state_dict(esd)
    return P.to(DEV), E.to(DEV), psd, esd


def close(got, want, rel, ab):
    return np.all(np.abs(got - want) <= np.maximum(rel * np.abs(want), ab))


# ---- 1. metric kernels on the reference's own codes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_mig_kernels_on_reference_codes(kind):
    g = gold(kind)
    codes = torch.from_numpy(g["mig_mus"]).to(DEV)
    bins = eg.score.discretize(codes).cpu().numpy()
    assert np.array_equal(bins.T, g["mig_disc"].astype(np.int32))
    factors = g["latents_values"][g["mig_idx"].astype(np.int64)][:, 1:6]
    score, m, H = eg.score.mig(codes, factors)
    assert close(m, g["mig_m"], 1e-12, 1e-15), np.abs(m - g["mig_m"]).max()
    assert close(H, g["mig_H"], 1e-12, 1e-15)
    assert abs(score - float(g["mig_score"])) <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_factor_vae_kernels_on_reference_codes(kind):
    g = gold(kind)
    ev = torch.from_numpy(ref_rows(g["fv_eval_cat"], g["fv_eval_cols"])).to(DEV)
    gr = torch.from_numpy(ref_rows(g["fv_group_cat"], g["fv_group_cols"])).to(DEV)
    labels = g["fv_labels"][:int(g["fv_groups"])].astype(np.int64)
    eval_std, predict, votes = eg.score.factor_vae_votes(ev, gr, labels, 5)
    assert np.array_equal(eval_std.cpu().numpy(), g["fv_eval_std"])              # numpy's np.std, bit for bit
    assert np.array_equal(predict.cpu().numpy(), g["fv_predict"].astype(np.int32))
    assert np.array_equal(votes.cpu().numpy(), g["fv_votes"])
    res = eg.score.factor_vae(ev, gr, labels, 5)
    assert res["factorVAE_metric"] == float(g["fv_metric"])
    assert res["factorVAE_metric_revised"] == float(g["fv_metric_revised"])
    assert np.array_equal(res["factorVAE_metric_detail"], g["fv_votes"].astype(np.float64))


@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_constant_code_column(kind):
    """one constant code: numpy's +-0.5 range widening, sklearn's single-cluster MI = 0, numpy's first-NaN argmin (0/0 column)"""
    g = gold(kind)
    col = int(g["deg_col"])
    mus = g["mig_mus"].copy()
    mus[:, col] = 0.0
    codes = torch.from_numpy(mus).to(DEV)
    bins = eg.score.discretize(codes).cpu().numpy()
    assert np.array_equal(bins.T, g["deg_disc"].astype(np.int32))
    assert len(np.unique(bins[col])) == 1
    score, m, H = eg.score.mig(codes, g["latents_values"][g["mig_idx"].astype(np.int64)][:, 1:6])
    assert np.all(m[col] == 0.0)
    assert close(m, g["deg_m"], 1e-12, 1e-15)
    assert abs(score - float(g["deg_score"])) <= 1e-12
    ev = ref_rows(g["fv_eval_cat"], g["fv_eval_cols"])
    gr = ref_rows(g["fv_group_cat"], g["fv_group_cols"])
    ev[:, col] = 0.0
    gr[:, col] = 0.0
    labels = g["fv_labels"][:int(g["fv_groups"])].astype(np.int64)
    eval_std, predict, votes = eg.score.factor_vae_votes(torch.from_numpy(ev).to(DEV), torch.from_numpy(gr).to(DEV), labels, 5)
    assert eval_std.cpu().numpy()[col] == 0.0
    assert np.array_equal(predict.cpu().numpy(), g["deg_predict"].astype(np.int32))
    assert votes.cpu().numpy()[col].sum() == labels.size


# ---- 2. representation vs the reference (fp32) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_representation_matches_reference(kind):
    g = gold(kind)
    P, E, _, _ = encoders(kind, g)
    data = torch.from_numpy(sprites(g)).to(DEV)
    P.train()
    E.eval()
    rep = eg.score.Representation(P, E, kind, batch=256)
    got = rep.codes(data, g["mig_idx"].astype(np.int64), g["mig_gains"] if kind == "colored" else None).cpu().numpy()
    assert P.training and not E.training                                          # each module's mode restored
    want = g["mig_mus"]
    tol = 1e-4 if kind == "colored" else 1e-5
    err = np.abs(got[:, 1:] - want[:, 1:]).max()
    assert err <= tol, err
    p = np.sort(g["mig_probs"].astype(np.float64), axis=1)
    tie = (p[:, -1] - p[:, -2]) <= 1e-6
    bad = (got[:, 0] != want[:, 0]) & ~tie
    assert not bad.any(), np.flatnonzero(bad)
    assert len(np.unique(got[:, 0])) > 1


# ---- 3. end to end through run_score ----------------------------------------------------------------------------------------------
def write_inputs(kind, g, tmp_path, psd, esd):
    imgs, lv, lc, meta = sd.dataset(tuple(g["sizes"]))
    npz = os.path.join(tmp_path, sd.NPZ_NAME)
    sd.write_npz(npz, imgs, lv, lc, meta)
    pp, ep = os.path.join(tmp_path, "pxy.pt"), os.path.join(tmp_path, "enc.pt")
    torch.save(psd, pp)
    torch.save(esd, ep)
    return npz, pp, ep


@pytest.mark.parametrize("kind", KINDS)
def test_run_score_end_to_end(kind, tmp_path, capsys):
    g = gold(kind)
    P, E, psd, esd = encoders(kind, g)
    npz, pp, ep = write_inputs(kind, g, str(tmp_path), psd, esd)
    score = eg.score.run_score(kind, "mig", npz, pp, ep, seed=int(g["seed"]))
    assert "MIG score" in capsys.readouterr().out
    assert abs(score - float(g["mig_score"])) <= 0.02
    # every discretised entry that differs from the reference sits within 1e-5 of a bin edge
    np.random.seed(int(g["seed"]))
    plan = eg.score.mig_plan(int(np.prod(g["sizes"])), kind == "colored")
    codes = eg.score.Representation(P, E, kind).codes(torch.from_numpy(sprites(g)).to(DEV), plan["idx"], plan["gains"])
    bins = eg.score.discretize(codes).cpu().numpy().T
    c = codes.cpu().numpy()
    for i, j in zip(*np.nonzero(bins != g["mig_disc"])):
        x = c[:, j]
        lo, hi = x.min(), x.max()
        edges = np.arange(20) * ((hi - lo) / 20) + lo
        assert np.abs(edges - c[i, j]).min() <= 1e-5, (i, j)
    res = eg.score.run_score(kind, "factor_vae", npz, pp, ep, seed=int(g["seed"]), groups=int(g["fv_groups"]))
    assert set(res) == {"factorVAE_metric", "factorVAE_metric_revised", "factorVAE_metric_detail"}
    moved = np.abs(res["factorVAE_metric_detail"] - g["fv_votes"]).sum() / 2
    assert moved <= 0.01 * int(g["fv_groups"]), moved


# ---- 4. scale ---------------------------------------------------------------------------------------------------------------------
def big_table(g, n=16384):
    """>= 16 k synthetic sprites on the device: the fixture's sprites rolled by (dy, dx) offsets"""
    base = torch.from_numpy(sprites(g)).to(DEV)
    reps = []
    k = 0
    while sum(r.shape[0] for r in reps) < n:
        reps.append(torch.roll(base, shifts=(k % 7 - 3, k // 7 % 7 - 3), dims=(1, 2)))
        k += 1
    return torch.cat(reps)[:n].contiguous()


def test_factor_vae_at_reference_sizes():
    g = gold("dsprites")
    P, E, _, _ = encoders("dsprites", g)
    table = big_table(g)
    plan = eg.score.factor_vae_plan(sd.FULL_SIZES, int(np.prod(sd.FULL_SIZES)), False, rng=np.random.RandomState(0))
    rep = eg.score.Representation(P, E, "dsprites", batch=4096)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = rep.codes(table, plan["eval_idx"] % table.shape[0])
    gr = rep.codes(table, plan["group_idx"].reshape(-1) % table.shape[0])
    res = eg.score.factor_vae(ev, gr, plan["labels"], 5)
    dt = time.perf_counter() - t0
    assert ev.shape == (73728, 5) and gr.shape == (50000, 5)
    assert res["factorVAE_metric_detail"].sum() == 500
    assert 0.0 < res["factorVAE_metric"] <= 1.0
    assert dt < 60.0, dt


@pytest.mark.parametrize("kind", KINDS)
def test_codes_equal_module_forward(kind):
    """2048 rows: the chunked path == Encoder_pxy.forward + eg_warp_affine_zeros (+ gain division) + Encoder.forward in eval mode"""
    g = gold(kind)
    P, E, _, _ = encoders(kind, g)
    table = big_table(g)
    rng = np.random.RandomState(1)
    idx = rng.randint(table.shape[0], size=2048)
    gains = rng.uniform(0.5, 1, (2048, 3)) if kind == "colored" else None
    got = eg.score.Representation(P, E, kind, batch=2048).codes(table, idx, gains)
    img = table[torch.from_numpy(idx).to(DEV)].unsqueeze(1).float()
    if gains is not None:
        img = (img * torch.from_numpy(gains.astype(np.float32)).to(DEV)[:, :, None, None]).contiguous()
    E.eval()
    P.eval()
    code = P(img)
    theta = torch.empty(2048, 2, 3, device=DEV)
    eg.ops.theta_pxy_align_inv(code, code.shape[1], 2048, theta)
    al = torch.empty_like(img)
    eg.ops.warp_affine_zeros(img, theta, al, 2048, img.shape[1], 64, 64)
    if gains is not None:
        al = al / (code[:, 3:] * 0.1 + 1)[:, :, None, None]
    cat, cont = E(al.contiguous())
    want = torch.cat([cat.argmax(1, keepdim=True).double(), cont[:, 0:2].double(), code[:, 1:3].double()], 1)
    assert torch.equal(got[:, 1:], want[:, 1:]), (got - want)[:, 1:].abs().max().item()
    assert torch.equal(got[:, 0], want[:, 0])


@pytest.mark.parametrize("kind", KINDS)
def test_codes_independent_of_chunk_size(kind):
    g = gold(kind)
    P, E, _, _ = encoders(kind, g)
    table = big_table(g)
    rng = np.random.RandomState(2)
    idx = rng.randint(table.shape[0], size=5000)
    gains = rng.uniform(0.5, 1, (5000, 3)) if kind == "colored" else None
    a = eg.score.Representation(P, E, kind, batch=512).codes(table, idx, gains)
    b = eg.score.Representation(P, E, kind, batch=4096).codes(table, idx, gains)
    assert torch.equal(a, b), (a - b).abs().max().item()

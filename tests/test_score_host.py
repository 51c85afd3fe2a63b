"""Host side of the disentanglement scores (ead-gan_amd/score.py): the sampling plans are the reference's numpy draws bit for bit
(tests/golden/score_*.npz, recorded from dSprites|colored_dSprites/score/{MIG,FactorVAE}.py), the synthetic weights reproduce their
checksums, and the generator reproduces the fixtures where the reference tree is present."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN
import score_data as sd

eg = importlib.import_module("ead-gan_amd")
KINDS = ("dsprites", "colored")


def gold(kind):
    return np.load(os.path.join(GOLDEN, f"score_{kind}.npz"))


@pytest.mark.parametrize("kind", KINDS)
def test_mig_plan_matches_reference_draws(kind):
    g = gold(kind)
    N = int(np.prod(g["sizes"]))
    np.random.seed(int(g["seed"]))
    plan = eg.score.mig_plan(N, kind == "colored")
    assert np.array_equal(plan["idx"], g["mig_idx"].astype(np.int64))
    if kind == "colored":
        assert np.array_equal(plan["gains"], g["mig_gains"])          # randint then uniform per batch of 16, float64 bits
    else:
        assert plan["gains"] is None
    # an explicit RandomState gives the same stream as the seeded global one
    again = eg.score.mig_plan(N, kind == "colored", rng=np.random.RandomState(int(g["seed"])))
    assert np.array_equal(again["idx"], plan["idx"])


@pytest.mark.parametrize("kind", KINDS)
def test_factor_vae_plan_matches_reference_draws(kind):
    g = gold(kind)
    N = int(np.prod(g["sizes"]))
    np.random.seed(int(g["seed"]))
    plan = eg.score.factor_vae_plan(g["sizes"], N, kind == "colored")
    assert plan["group_idx"].shape == (500, 100)
    assert np.array_equal(plan["group_idx"], g["fv_group_idx"].astype(np.int64))
    assert np.array_equal(plan["labels"], g["fv_labels"].astype(np.int64))
    assert np.array_equal(plan["eval_idx"], g["fv_eval_idx"].astype(np.int64))
    if kind == "colored":                                             # evaluate(): eval-set gains first, then each group's
        assert np.array_equal(plan["eval_gains"], g["fv_eval_gains"])
        assert sd.digest(plan["group_gains"][:int(g["fv_groups"])]) == str(g["fv_group_gains_sha256"])     # the groups evaluate() ran


def test_factor_vae_plan_at_archive_sizes():
    g = gold("dsprites")
    N = int(np.prod(sd.FULL_SIZES))
    np.random.seed(int(g["full_seed"]))
    plan = eg.score.factor_vae_plan(sd.FULL_SIZES, N, False)
    assert plan["eval_idx"].size == int(g["full_eval_n"]) == 73728
    assert np.array_equal(plan["labels"], g["full_labels"].astype(np.int64))
    assert np.array_equal(plan["group_idx"][:4], g["full_group_idx_head"].astype(np.int64))
    assert np.array_equal(plan["eval_idx"][:64], g["full_eval_idx_head"].astype(np.int64))
    assert sd.digest(plan["group_idx"]) == str(g["full_group_idx_sha256"])
    assert sd.digest(plan["eval_idx"]) == str(g["full_eval_idx_sha256"])


@pytest.mark.parametrize("kind", KINDS)
def test_weight_helper_reproduces_checksums(kind):
    g = gold(kind)
    mod = eg.colored if kind == "colored" else eg.dsprites
    s_pxy, s_enc = (int(s) for s in g["weight_seeds"])
    pxy = sd.make_weights(mod.Encoder_pxy().state_dict(), s_pxy, float(g["cat_scale"]))
    enc = sd.make_weights(mod.Encoder().state_dict(), s_enc, float(g["cat_scale"]))
    assert np.array_equal(sd.checksums(pxy), g["pxy_checksums"])
    assert np.array_equal(sd.checksums(enc), g["enc_checksums"])


def test_synthetic_dataset_matches_fixture():
    g = gold("dsprites")
    imgs, lv, _, meta = sd.dataset(tuple(g["sizes"]))
    assert np.array_equal(np.packbits(imgs.reshape(imgs.shape[0], -1), axis=1), g["sprites_bits"])
    assert np.array_equal(lv, g["latents_values"])
    assert tuple(meta["latents_sizes"]) == sd.SMALL_SIZES


def test_latents_bases_and_entry_checks():
    assert list(eg.score.latents_bases(sd.FULL_SIZES)) == [737280, 245760, 40960, 1024, 32, 1]
    with pytest.raises(ValueError):
        eg.score.run_score("mnist", "mig", "x.npz", "a.pt", "b.pt")
    with pytest.raises(ValueError):
        eg.score.run_score("dsprites", "dci", "x.npz", "a.pt", "b.pt")


@pytest.mark.parametrize("kind", KINDS)
def test_generator_regenerates_fixture(kind):
    from oracle import ref_harness as rh
    if not rh.available():
        pytest.skip("the reference tree is not on this host")
    import make_score_golden as msg
    got = msg.make(kind)
    want = gold(kind)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(np.asarray(got[k]), want[k]), k

"""Training runs, the parts that need no GPU: the loss-log entry point of the C ABI, the cadence table against the reference scripts'
three ``%`` tests, the progress lines against literals, ``LossLog.rows()`` on a host-filled mirror, and the checks of
``load_state_dict`` on a state file that loads with ``weights_only=True``."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch


def _pkg():
    return importlib.import_module("ead-gan_amd")


def test_runlog_append_is_declared_exported_and_checks_arguments():
    eg = _pkg()
    protos = eg._lib.parse_header()
    assert "eg_runlog_append" in protos
    restype, argtypes = protos["eg_runlog_append"]
    assert restype is ctypes.c_int and len(argtypes) == 7 and argtypes[1] is ctypes.c_int and argtypes[3] is ctypes.c_int
    assert hasattr(ctypes.CDLL(eg._lib.LIB_PATH), "eg_runlog_append")
    # argument errors return a code and launch nothing (no GPU is touched: the checks come first)
    with pytest.raises(RuntimeError, match="null pointer"):
        eg._lib.lib().call("eg_runlog_append", None, 4, None, 8, None, None, None)
    buf = (ctypes.c_float * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for n, cap in ((0, 8), (65, 8), (4, 0)):
        with pytest.raises(RuntimeError, match="capacity"):
            eg._lib.lib().call("eg_runlog_append", ptr, n, ptr, cap, ptr, ptr, None)


# the reference's conditions, written out: (print, sample, checkpoint) of the iteration ``b`` with --sample_interval ``si``
REFERENCE_TESTS = {
    "celeba": lambda b, si: (b % 10 == 0, b % si == 0, b % (si * 15) == 0),                 # celebA/EAD-GAN_celebA.py:404,411,414
    "mnist": lambda b, si: (b % 100 == 0, b % si == 0, b % (si * 10) == 0),                 # MNIST/EAD-GAN_rpqmnxy.py:453,459,462
    "dsprites": lambda b, si: (b % 100 == 0, b % (si * 2) == 0, b % (si * 500) == 0),       # dSprites/rp.py:491,504,507
    "colored": lambda b, si: (b % 100 == 0, b % (si * 2) == 0, b % (si * 50) == 0),         # colored_dSprites/rp_color.py:523,536,539
    "pxy": lambda b, si: (b % 100 == 0, False, b % (si * 50) == 0),                         # dSprites/pxy.py:194,204 (sample grids out of scope)
    "pxy_color": lambda b, si: (b % 100 == 0, False, b % (si * 10) == 0),                   # colored_dSprites/pxy_color.py:223,233
}


@pytest.mark.parametrize("kind", sorted(REFERENCE_TESTS))
def test_cadence_table_matches_the_scripts(kind):
    tr = _pkg().train
    assert set(tr.KINDS) == set(REFERENCE_TESTS)
    si = 3
    mults = {"celeba": (10, si, si * 15), "mnist": (100, si, si * 10), "dsprites": (100, si * 2, si * 500), "colored": (100, si * 2, si * 50),
             "pxy": (100, si * 50), "pxy_color": (100, si * 10)}[kind]
    lcm = 1
    for m in mults:
        lcm = lcm * m // math.gcd(lcm, m)
    want = [set(), set(), set()]
    got = [set(), set(), set()]
    for b in range(0, 3 * lcm):
        for j, (w, g) in enumerate(zip(REFERENCE_TESTS[kind](b, si), tr.cadence(kind, b, si))):
            if w:
                want[j].add(b)
            if g:
                got[j].add(b)
    assert got == want
    assert 0 in got[0] and 0 in got[2]                      # iteration 0 prints and saves, as the scripts do
    # the scripts' --sample_interval defaults when none is given
    default = {"celeba": 4000, "mnist": 4000}.get(kind, 1000)
    assert tr.cadence(kind, default * 1000, None) == REFERENCE_TESTS[kind](default * 1000, default)
    assert tr.cadence(kind, default * 1000 + default, None) == REFERENCE_TESTS[kind](default * 1000 + default, default)


def test_progress_lines_are_the_scripts_literals():
    tr = _pkg().train
    # N = 20 images at B = 8: DataLoader's length is 3; iteration 7 is epoch 2, batch 1
    assert tr.loader_len(20, 8) == 3 and tr.loader_len(16, 8) == 2 and tr.loader_len(1, 8) == 1
    row = np.float32([0.12345678, 1.9999996, 3.5, 0.25, 7.0000005, 0.0625, 10.125, 0.0])
    assert tr.progress_line("celeba", 7, 50, 20, 8, row) == "[Epoch 2/50] [Batch 1/3] [D loss: 2.000000] [G loss: 0.123457]"
    assert tr.progress_line("mnist", 7, 200, 20, 8, row) == "[Epoch 2/200] [Batch 1/3] [D loss: 2.000000] [G loss: 0.123457] [info loss: 3.500000]"
    assert tr.progress_line("dsprites", 300, 100, 20, 8, row) == ("[Epoch 100/100] [Batch 0/3] [D loss: 0.123457] [G loss: 2.000000] [info cat loss: 0.062500] "
                                                                   "[info cont loss: 10.125000] [affine loss: 0.250000] [relative_cat_loss: 7.000000] ")
    assert tr.progress_line("colored", 2, 100, 20, 8, row) == ("[Epoch 0/100] [Batch 2/3] [D loss: 0.123457] [G loss: 2.000000] [info cat loss: 0.062500] "
                                                                "[info cont loss: 10.125000] [affine_color loss: 0.250000] [relative_cat_loss: 7.000000] ")
    assert tr.progress_line("pxy", 5, 10, 20, 8, row) == "[Epoch 1/10] [Batch 2/3] [D loss: 0.123457]"
    assert tr.progress_line("pxy_color", 0, 10, 24, 8, row) == "[Epoch 0/10] [Batch 0/3] [D loss: 0.123457]"
    assert tr.minmax_lines("dsprites", (0.0, 1.0, 0.25, 0.5)) == ["trans_img_affine max tensor(1., device='cuda:0')", "gen_imgs max tensor(0.5000, device='cuda:0')",
                                                                "trans_img_affine min tensor(0., device='cuda:0')", "gen_imgs min tensor(0.2500, device='cuda:0')"]
    assert tr.minmax_lines("colored", (0.0, 1.0, 0.25, 0.5))[0].startswith("trans_img_affine_color max ")
    assert tr.checkpoint_files("celeba", 60000) == ["checkpoint_60000.tar"]
    assert tr.checkpoint_files("mnist", 40000) == ["generator_40000.pt", "encoder_40000.pt"]
    assert tr.checkpoint_files("dsprites", 5) == ["encoder_5.pt", "generator_5.pt"] == tr.checkpoint_files("colored", 5)
    assert tr.checkpoint_files("pxy", 50000) == ["encoder_pxy_50000.pt"] and tr.checkpoint_files("pxy_color", 7) == ["encoder_pxy_color_7.pt"]
    with pytest.raises(ValueError, match="kind"):
        tr.cadence("imagenet", 0)


@pytest.mark.parametrize("appends", [5, 8, 8 * 2 + 3])
def test_losslog_rows_unwraps_a_host_filled_mirror(appends):
    eng = _pkg().engine
    cap, n = 8, 3
    log = eng.LossLog.host_mirror(n, cap)
    for h in range(appends):                                   # what eg_runlog_append does, on the host
        log.mirror[h % cap] = np.float32([h, h + 0.5, -h])
    log.mirror_head = appends
    rows = log.rows()
    first = max(0, appends - cap)
    assert rows.shape == (min(appends, cap), n) and rows.dtype == np.float32
    np.testing.assert_array_equal(rows[:, 0], np.arange(first, appends, dtype=np.float32))
    np.testing.assert_array_equal(rows[:, 2], -np.arange(first, appends, dtype=np.float32))
    assert log.first_row() == first
    since = appends - 2
    np.testing.assert_array_equal(log.rows(since=since)[:, 0], np.float32([since, since + 1]))
    f, r = eng.unwrap_ring(log.mirror, appends, cap, since=0)
    assert f == first and len(r) == min(appends, cap)


def _hand_made_state():
    return {"modules.P.fc1.weight": torch.zeros(3, 4), "modules.P.fc1.bias": torch.zeros(3), "modules.P.bn.num_batches_tracked": torch.tensor(7),
            "adam.P.m": torch.zeros(15), "adam.P.v": torch.ones(15), "adam.steps": torch.tensor([6], dtype=torch.int32),
            "inputs.seed": 5, "inputs.step": 6, "inputs.sampling": "permutation", "inputs.flip": 0, "log.head": 6, "log.first_nonfinite": 0,
            "meta.kind": "pxy", "meta.dtype": "bf16", "meta.lr": [2e-4], "meta.betas": [0.5, 0.999], "meta.format": 1}


def test_state_file_loads_with_weights_only_and_is_validated(tmp_path):
    eng = _pkg().engine
    sd = _hand_made_state()
    path = tmp_path / "run_state_6.pt"
    torch.save(sd, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert set(back) == set(sd) and back["meta.kind"] == "pxy" and back["inputs.sampling"] == "permutation" and back["meta.lr"] == [2e-4]
    assert torch.equal(back["adam.steps"], sd["adam.steps"]) and back["adam.steps"].dtype == torch.int32
    spec = {k: (tuple(v.shape) if isinstance(v, torch.Tensor) else None) for k, v in sd.items() if not k.startswith("meta.")}
    eng.validate_state(back, "pxy", spec)                                          # a matching state passes
    with pytest.raises(ValueError, match="meta.kind"):
        eng.validate_state(back, "dsprites", spec)
    for key in ("adam.P.v", "inputs.step", "modules.P.fc1.bias", "log.head"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            eng.validate_state({k: v for k, v in back.items() if k != key}, "pxy", spec)
    with pytest.raises(ValueError, match=r"modules\.P\.fc1\.weight"):
        eng.validate_state(dict(back, **{"modules.P.fc1.weight": torch.zeros(4, 3)}), "pxy", spec)
    with pytest.raises(ValueError, match=r"adam\.P\.m"):
        eng.validate_state(dict(back, **{"adam.P.m": torch.zeros(16)}), "pxy", spec)
    with pytest.raises(ValueError, match=r"adam\.steps"):
        eng.validate_state(dict(back, **{"adam.steps": 6}), "pxy", spec)
    with pytest.raises(ValueError, match=r"meta\.format"):
        eng.validate_state(dict(back, **{"meta.format": 2}), "pxy", spec)


def test_trainers_expose_the_state_interface():
    eg = _pkg()
    kinds = {eg.celeba.CelebATrainer: "celeba", eg.mnist.MnistTrainer: "mnist", eg.dsprites.DspritesTrainer: "dsprites",
             eg.colored.ColoredTrainer: "colored", eg.dsprites.PxyTrainer: "pxy", eg.colored.PxyColorTrainer: "pxy_color"}
    for cls, kind in kinds.items():
        assert cls.STATE_KIND == kind and callable(cls.state_dict) and callable(cls.load_state_dict), cls
    assert set(kinds.values()) == set(eg.train.KINDS)
    import eadgan
    assert eadgan.train is eg.train

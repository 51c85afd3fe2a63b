"""Weight averaging, the checks that need no GPU: the C ABI of eg_ema_plan / eg_ema_update, eg_ema_plan itself (host code: chunk
prefixes and every argument error, through fake non-null pointers that are never dereferenced), the host twin of the decay, and the
names of the averaged checkpoint files."""
import ctypes
import importlib

import numpy as np
import pytest


def _pkg():
    return importlib.import_module("ead-gan_amd")


def _plan(segs, nseg=None, first=True):
    """eg_ema_plan over [(src address, dst address, n words, kind)] -> the chunk prefix as a list"""
    eg = _pkg()
    arr = (eg._lib.EgEmaSeg * max(len(segs), 1))()
    for i, (src, dst, n, kind) in enumerate(segs):
        arr[i] = eg._lib.EgEmaSeg(src, dst, n, kind)
    n = len(segs) if nseg is None else nseg
    out = (ctypes.c_uint * (max(n, 0) + 1))()
    eg._lib.lib().call("eg_ema_plan", arr, n, out if first else None)
    return list(out)


def test_abi_declares_and_exports_the_ema_entry_points():
    eg = _pkg()
    protos = eg._lib.parse_header()
    assert len(protos["eg_ema_plan"][1]) == 3
    assert len(protos["eg_ema_update"][1]) == 7
    assert protos["eg_ema_chunk_words"][1] == []
    cdll = ctypes.CDLL(eg._lib.LIB_PATH)
    for name in ("eg_ema_plan", "eg_ema_update", "eg_ema_chunk_words"):
        assert hasattr(cdll, name), name
    assert eg._lib.lib().query("eg_version") >= 110
    # the ctypes mirror has the header's fields in the header's order
    import re
    src = open(eg._lib.HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct eg_ema_seg \{(.*?)\} eg_ema_seg;", src, re.S).group(1), flags=re.S)
    fields = [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == [n for n, _ in eg._lib.EgEmaSeg._fields_] == ["src", "dst", "n", "kind"]
    assert ctypes.sizeof(eg._lib.EgEmaSeg) == 32


def test_plan_chunk_prefixes():
    eg = _pkg()
    chunk = eg.ops.ema_chunk_words()
    assert chunk > 0 and chunk % 4 == 0                  # a chunk is a whole number of 16-byte groups: it starts as aligned as its segment
    ns = [1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
    segs = [(0x1000 + 64 * i, 0x100000 + 64 * i, n, i % 2) for i, n in enumerate(ns)]
    got = _plan(segs)
    want = np.concatenate(([0], np.cumsum([-(-n // chunk) for n in ns]))).tolist()
    assert want == [0, 1, 2, 3, 5, 9]
    assert got == want
    for n in ns:                                          # and each alone
        assert _plan([(0x1000, 0x2000, n, 0)]) == [0, -(-n // chunk)]
    # 2^31 chunks are the most a table may hold
    assert _plan([(0x1000, 0x2000, (2 ** 31) * chunk, 1)]) == [0, 2 ** 31]


def test_plan_argument_errors_do_not_abort():
    eg = _pkg()
    chunk = eg.ops.ema_chunk_words()
    ok = (0x1000, 0x2000, 8, 0)
    import re
    max_segs = int(re.search(r"^#define EG_EMA_MAX_SEGS (\d+)", open(eg._lib.HEADER).read(), re.M).group(1))
    with pytest.raises(RuntimeError, match="null pointer"):
        eg._lib.lib().call("eg_ema_plan", None, 1, (ctypes.c_uint * 2)())
    with pytest.raises(RuntimeError, match="null pointer"):
        _plan([ok], first=False)
    for nseg in (0, -1, max_segs + 1):
        with pytest.raises(RuntimeError, match="nseg must be in 1.."):
            _plan([ok] * max(nseg, 1), nseg=nseg)
    assert len(_plan([(0x1000 + 32 * i, 0x100000 + 32 * i, 8, 0) for i in range(max_segs)])) == max_segs + 1
    assert max_segs >= 64
    with pytest.raises(RuntimeError, match="segment 1: null src or dst"):
        _plan([ok, (None, 0x2000, 8, 0)])
    with pytest.raises(RuntimeError, match="segment 0: null src or dst"):
        _plan([(0x1000, None, 8, 0)])
    with pytest.raises(RuntimeError, match="segment 2: n == 0"):
        _plan([ok, ok, (0x1000, 0x2000, 0, 0)])
    for kind in (2, -1):
        with pytest.raises(RuntimeError, match="kind must be 0 .lerp. or 1 .copy."):
            _plan([(0x1000, 0x2000, 8, kind)])
    for src, dst in ((0x1002, 0x2000), (0x1000, 0x2001), (0x1003, 0x2003)):
        with pytest.raises(RuntimeError, match="4-byte aligned"):
            _plan([(src, dst, 8, 0)])
    with pytest.raises(RuntimeError, match="src == dst"):
        _plan([(0x1000, 0x1000, 8, 1)])
    with pytest.raises(RuntimeError, match="more than 2.31 chunks"):
        _plan([(0x1000, 0x2000, (2 ** 31) * chunk + 1, 0)])
    with pytest.raises(RuntimeError, match="more than 2.31 chunks .through segment 1."):
        _plan([(0x1000, 0x2000, (2 ** 31) * chunk, 0), (0x3000, 0x4000, 1, 0)])
    assert _plan([ok]) == [0, 1]                           # the process is alive and the library still answers


def test_update_argument_errors_do_not_abort():
    """eg_ema_update checks its arguments before it launches: these calls never reach a device"""
    eg = _pkg()
    call = eg._lib.lib().call
    p = 0x1000
    with pytest.raises(RuntimeError, match="null pointer"):
        call("eg_ema_update", None, p, 1, 0.5, 0.0, p, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        call("eg_ema_update", p, None, 1, 0.5, 0.0, p, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        call("eg_ema_update", p, p, 1, 0.5, 0.0, None, None)
    for beta in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"beta must be in \[0, 1\)"):
            call("eg_ema_update", p, p, 1, beta, 0.0, p, None)
    for ramp in (-1.0, float("nan")):
        with pytest.raises(RuntimeError, match="ramp must be >= 0"):
            call("eg_ema_update", p, p, 1, 0.5, ramp, p, None)
    with pytest.raises(RuntimeError, match="nseg must be in 1.."):
        call("eg_ema_update", p, p, 0, 0.5, 0.0, p, None)


def test_ema_decay_is_the_kernels_float32():
    eg = _pkg()
    d = eg.engine.ema_decay
    for beta in (0.0, 0.5, 0.999, 0.9999):
        for t in (0, 1, 10 ** 6):
            v = d(beta, 0, t)
            assert isinstance(v, np.float32) and v == np.float32(beta)
    assert d(0.999, 10, 0) == np.float32(0.1) and isinstance(d(0.999, 10, 0), np.float32)
    vals = [d(0.999, 10, t) for t in range(20000)]
    assert all(isinstance(v, np.float32) for v in vals)
    assert all(b >= a for a, b in zip(vals, vals[1:]))                   # monotone non-decreasing in t
    first = next(t for t, v in enumerate(vals) if v == np.float32(0.999))
    assert 0 < first < 20000 and all(v == np.float32(0.999) for v in vals[first:])      # beta exactly, from some t on
    # the three fp32 operations, in the kernel's order
    for t in (0, 5, 123, 8990, 8991, 10 ** 6):
        want = min(np.float32(0.999), (np.float32(1) + np.float32(t)) / (np.float32(10) + np.float32(t)))
        assert d(0.999, 10, t) == want
    assert d(0.5, 10, 10 ** 6) == np.float32(0.5)


def test_ema_checkpoint_file_names():
    eg = _pkg()
    f = eg.train.ema_checkpoint_files
    assert f("celeba", 7, ("G",)) == ["generator_ema_7.pt"]
    assert f("mnist", 40000, ("G", "E")) == ["generator_ema_40000.pt", "encoder_ema_40000.pt"]
    assert f("dsprites", 0, ("G", "E")) == ["generator_ema_0.pt", "encoder_ema_0.pt"]
    assert f("colored", 50, ("E",)) == ["encoder_ema_50.pt"]
    assert f("pxy", 3, ("P",)) == ["encoder_pxy_ema_3.pt"]
    assert f("pxy_color", 3, ("P",)) == ["encoder_pxy_color_ema_3.pt"]
    assert f("celeba", 1, ()) == []
    with pytest.raises(ValueError, match="'G'"):
        f("pxy", 0, ("G",))
    with pytest.raises(ValueError, match="kind must be one of"):
        f("nope", 0, ("G",))
    # the scripts' own files keep their names
    c = eg.train.checkpoint_files
    assert c("celeba", 7) == ["checkpoint_7.tar"] and c("mnist", 7) == ["generator_7.pt", "encoder_7.pt"]
    assert c("dsprites", 7) == ["encoder_7.pt", "generator_7.pt"] == c("colored", 7)
    assert c("pxy", 7) == ["encoder_pxy_7.pt"] and c("pxy_color", 7) == ["encoder_pxy_color_7.pt"]


def test_trainers_have_no_average_by_default():
    eg = _pkg()
    assert eg.engine.TrainerState.ema is None and eg.engine.ResidentStep.ema is None
    for cls in (eg.celeba.CelebATrainer, eg.mnist.MnistTrainer, eg.dsprites.DspritesTrainer, eg.dsprites.PxyTrainer):
        assert cls.ema is None and callable(cls.attach_ema)

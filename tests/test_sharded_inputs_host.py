"""Sharded device draws, the parts that need no GPU: the C ABI declares the shard arguments (``elem0``, ``total``) on the existing entry
points, ``engine.shard_span`` is the one rule that maps (rank, world) to them, and the Python surface defaults to the unsharded draw."""
import ctypes
import importlib
import inspect
import re

import pytest


def _pkg():
    return importlib.import_module("ead-gan_amd")


def test_header_declares_the_shard_arguments():
    eg = _pkg()
    protos = eg._lib.parse_header()
    restype, argtypes = protos["eg_rng_fill"]
    assert restype is ctypes.c_int and len(argtypes) == 11
    assert argtypes[8] is ctypes.c_size_t and argtypes[9] is ctypes.c_size_t and argtypes[10] is ctypes.c_void_p      # elem0, total, stream
    assert len(protos["eg_rng_fill_multi"][1]) == 5                                      # the segments carry the shard
    src = open(eg._lib.HEADER).read()
    seg = re.search(r"typedef struct eg_rng_seg \{(.*?)\} eg_rng_seg;", src, re.S).group(1)
    assert re.search(r"\bsize_t\s+elem0\s*,\s*total\s*;", seg)
    fields = [n for n, _ in eg._lib.EgRngSeg._fields_]
    assert fields[-2:] == ["elem0", "total"] and fields[:3] == ["kind", "out", "n"]
    assert dict(eg._lib.EgRngSeg._fields_)["elem0"] is ctypes.c_size_t and dict(eg._lib.EgRngSeg._fields_)["total"] is ctypes.c_size_t
    assert eg._lib.lib().query("eg_version") >= 108


def test_shard_span_is_rank_major_and_validates():
    eng = _pkg().engine
    assert eng.shard_span(5, 1, 3) == (5, 15)
    assert eng.shard_span(7, 0, 1) == (0, 7)
    assert eng.shard_span(4, 2, 3) == (8, 12)
    for rank, world in ((0, 0), (-1, 2), (2, 2), (3, 2)):
        with pytest.raises(ValueError, match="world"):
            eng.shard_span(4, rank, world)


def test_python_surface_defaults_to_the_unsharded_draw():
    eg = _pkg()
    for fn in (eg.ops.rng_fill, eg.ops.rng_fill_multi, eg.engine.DeviceSampler.__init__, eg.celeba.DeviceInputs.__init__):
        p = inspect.signature(fn).parameters
        assert p["rank"].default == 0 and p["world"].default == 1, fn
    # the seven-positional call of the existing tests keeps its meaning
    assert list(inspect.signature(eg.ops.rng_fill).parameters)[:7] == ["kind", "out", "a", "b", "seed", "step", "stream_id"]
    assert list(inspect.signature(eg.ops.rng_fill_multi).parameters)[:3] == ["draws", "seed", "step"]
    # the samplers of the small networks inherit the constructor
    for cls in (eg.mnist.DeviceInputs, eg.dsprites.DeviceInputs, eg.colored.DeviceInputs, eg.dsprites.PxyDeviceInputs, eg.colored.PxyDeviceInputs):
        assert issubclass(cls, eg.engine.DeviceSampler) and cls.__init__ is eg.engine.DeviceSampler.__init__

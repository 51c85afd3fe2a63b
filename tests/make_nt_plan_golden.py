"""Record what the NT convolution planner answers, over a grid of problems, in tests/golden/nt_plan_table.npz (host only: the four query
functions of the library are pure host code and need no GPU).

    python tests/make_nt_plan_golden.py [path/to/libeadgan_hip.so]

Run it with the library of the commit whose decisions are to be kept (default: the one built in this tree); tests/test_nt_plan_host.py
imports the enumeration below, recomputes every case with the library under test and compares array for array.  Only the answers are
stored: the inputs are this enumeration.

  automatic hints   every geometry of AUTO_* below in three dtypes, forward and backward-data: eg_conv_splitk_ws_bytes, then
                    eg_igemm_nt_tile_ep and eg_conv_stat_blocks with no scratch, 1 MiB of scratch and exactly the scratch the first answer
                    asks for
  hints cross       HINT_GEOMS x every nt_variant in -6..6 x nt_splitk in {0, 1, 2, 4, 8}: eg_igemm_nt_tile (bare hints, unlimited
                    scratch), and the two per-call queries with the same three scratch sizes

The scratch is never allocated: the queries read eg_epilogue.splitk_ws for null / non-null only.
"""
from __future__ import annotations

import ctypes
import importlib
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "golden", "nt_plan_table.npz")

AUTO_B = (1, 8, 128, 384)
AUTO_HW = (4, 8, 16, 32, 64)
AUTO_KSPU = ((4, 2, 1, 0), (3, 1, 1, 0), (3, 1, 1, 1), (1, 1, 0, 0), (3, 2, 1, 0))          # (k, stride, pad, up)
AUTO_C = (8, 16, 32, 64, 128, 256, 512, 1024)
DTYPES = (0, 1, 2)                                                                       # EG_F32, EG_BF16, EG_F16
DTYPE_NAMES = ("f32", "bf16", "f16")
AUTO_MAX_ELEMS = 1 << 28                                                                 # B * H * W * max(Cin, Cout)

HINT_GEOMS = ((8, 16, 16, 128, 128, 4, 2, 1), (8, 16, 16, 128, 64, 4, 2, 1), (128, 32, 32, 128, 256, 4, 2, 1),
              (128, 8, 8, 512, 1024, 4, 2, 1), (128, 64, 64, 64, 128, 4, 2, 1), (512, 8, 8, 64, 64, 4, 2, 1))   # (B, H, W, Cin, Cout, k, s, p)
HINT_VARIANTS = tuple(range(-6, 7))
HINT_SPLITK = (0, 1, 2, 4, 8)

MIB = 1 << 20
SCRATCH_NAMES = ("none", "1 MiB", "exact")
# label = BM * 1000 + code (eg_igemm_nt_tile in the header); every code the planner can answer must occur in the fixture
CODES = (-1, 16, 32, 64, 128, 131, 132, 135, 147, 148, 149, 150, 151, 152)


def auto_cases():
    """[(B, H, W, Cin, Cout, k, stride, pad, up, dtype, bwd)]"""
    out = []
    for B, hw, (k, s, p, up), cin, cout in itertools.product(AUTO_B, AUTO_HW, AUTO_KSPU, AUTO_C, AUTO_C):
        if B * hw * hw * max(cin, cout) > AUTO_MAX_ELEMS:
            continue
        out += [(B, hw, hw, cin, cout, k, s, p, up, dt, bwd) for dt in DTYPES for bwd in (0, 1)]
    return out


def hint_cases():
    """[(B, H, W, Cin, Cout, k, stride, pad, up, dtype, bwd, nt_variant, nt_splitk)]"""
    return [g + (0, dt, bwd, v, sk) for g in HINT_GEOMS for dt in DTYPES for bwd in (0, 1) for v in HINT_VARIANTS for sk in HINT_SPLITK]


def codes_of(labels):
    labels = np.asarray(labels).ravel()
    return set(np.unique(np.where(labels < 0, labels, labels % 1000)).tolist())


def describe(case, scratch=None):
    B, H, W, cin, cout, k, s, p, up, dt, bwd = case[:11]
    hints = f"nt_variant={case[11]} nt_splitk={case[12]}" if len(case) > 11 else "automatic"
    where = "unlimited scratch" if scratch is None else f"scratch {SCRATCH_NAMES[scratch]}"
    return f"(B={B} H={H} W={W} {cin}->{cout} k={k} s={s} p={p} up={up}, {DTYPE_NAMES[dt]}, bwd={bwd}, {hints}, {where})"


def load(lib_path=None):
    """the bound library of this tree, or another build of it (same header) at ``lib_path``"""
    eg = importlib.import_module("ead-gan_amd")
    if lib_path is None:
        return eg, eg._lib.lib().cdll
    cdll = ctypes.CDLL(os.path.abspath(lib_path))
    for name, (restype, argtypes) in eg._lib.parse_header().items():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    return eg, cdll


def _per_call(cdll, ep, c, dt, bwd, exact, tile, stat):
    """the two per-call queries under the three scratch sizes -> tile[3], stat[3]"""
    for j, size in enumerate((0, MIB, exact)):
        ep.splitk_ws, ep.splitk_ws_bytes = 64, size             # any non-null address: the queries never dereference it
        tile[j] = cdll.eg_igemm_nt_tile_ep(c, dt, bwd, ctypes.byref(ep))
        stat[j] = cdll.eg_conv_stat_blocks(c, dt, bwd, ctypes.byref(ep))


def compute(lib_path=None):
    eg, cdll = load(lib_path)
    auto, hint = auto_cases(), hint_cases()
    out = {"auto_ws": np.zeros(len(auto), np.int64), "auto_tile": np.zeros((len(auto), 3), np.int32), "auto_stat": np.zeros((len(auto), 3), np.int32),
           "hint_tile": np.zeros(len(hint), np.int32), "hint_tile_ep": np.zeros((len(hint), 3), np.int32), "hint_stat": np.zeros((len(hint), 3), np.int32)}
    ep = eg.ops.epilogue(splitk_ws=None)
    for i, case in enumerate(auto):
        dt, bwd = case[9], case[10]
        c = ctypes.byref(eg.ops.make_conv(*case[:9]))
        out["auto_ws"][i] = cdll.eg_conv_splitk_ws_bytes(c, dt, bwd)
        _per_call(cdll, ep, c, dt, bwd, int(out["auto_ws"][i]), out["auto_tile"][i], out["auto_stat"][i])
    for i, case in enumerate(hint):
        dt, bwd, variant, splitk = case[9:]
        c = ctypes.byref(eg.ops.make_conv(*case[:9]))
        out["hint_tile"][i] = cdll.eg_igemm_nt_tile(c, dt, bwd, variant, splitk)
        hep = eg.ops.epilogue(splitk_ws=None, nt_variant=variant, nt_splitk=splitk)
        _per_call(cdll, hep, c, dt, bwd, cdll.eg_conv_splitk_ws_bytes(c, dt, bwd), out["hint_tile_ep"][i], out["hint_stat"][i])
    return out


def main(argv):
    out = compute(argv[0] if argv else None)
    np.savez_compressed(PATH, **out)
    labels = np.concatenate([out[k].ravel() for k in ("auto_tile", "hint_tile", "hint_tile_ep")])
    print(PATH, os.path.getsize(PATH), "bytes;", len(out["auto_ws"]), "automatic cases,", len(out["hint_tile"]), "hinted cases; codes",
          sorted(codes_of(labels)), "; scratch zero / positive", int((out["auto_ws"] == 0).sum()), int((out["auto_ws"] > 0).sum()),
          "; statistics zero / positive", int((out["auto_stat"] == 0).sum()), int((out["auto_stat"] > 0).sum()))


if __name__ == "__main__":
    main(sys.argv[1:])

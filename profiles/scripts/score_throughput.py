"""Throughput of the disentanglement-score path (ead-gan_amd/score.py): one JSON line with
  - images/s of Representation.codes at B = 4096 for dSprites and colored dSprites,
  - wall time of a FactorVAE run at the reference's sizes (73 728 eval + 500 x 100 group images) and of a MIG run (1000 points),
  - the kernel split of one ``rocprofv3 --kernel-trace --stats`` run of the FactorVAE workload (``--no-prof``: skipped).
Synthetic weights and a 16 k-image synthetic sprite table (tests/score_data.py).

    python profiles/scripts/score_throughput.py [--no-prof] [--out DIR]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import score_data as sd          # noqa: E402

eg = importlib.import_module("ead-gan_amd")


def setup(kind, n=16384):
    mod = eg.colored if kind == "colored" else eg.dsprites
    P, E = mod.Encoder_pxy(), mod.Encoder()
    P.load_state_dict(sd.make_weights(P.state_dict(), sd.WEIGHT_SEEDS[kind]))
    E.load_state_dict(sd.make_weights(E.state_dict(), sd.WEIGHT_SEEDS[kind] + 100))
    imgs = torch.from_numpy(sd.dataset()[0]).cuda()
    table = torch.cat([torch.roll(imgs, shifts=(k % 7 - 3, k // 7 % 7 - 3), dims=(1, 2)) for k in range(-(-n // imgs.shape[0]))])[:n].contiguous()
    return P.cuda(), E.cuda(), table


def factor_vae_full(kind, P, E, table):
    rng = np.random.RandomState(0)
    t0 = time.perf_counter()
    plan = eg.score.factor_vae_plan(sd.FULL_SIZES, int(np.prod(sd.FULL_SIZES)), kind == "colored", rng=rng)
    t1 = time.perf_counter()
    rep = eg.score.Representation(P, E, kind, 4096)
    ev = rep.codes(table, plan["eval_idx"] % table.shape[0], plan.get("eval_gains"))
    gg = plan["group_gains"].reshape(-1, 3) if kind == "colored" else None
    gr = rep.codes(table, plan["group_idx"].reshape(-1) % table.shape[0], gg)
    res = eg.score.factor_vae(ev, gr, plan["labels"], 5)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, res["factorVAE_metric"]


def measure():
    out = {}
    for kind in ("dsprites", "colored"):
        P, E, table = setup(kind)
        rep = eg.score.Representation(P, E, kind, 4096)
        rng = np.random.RandomState(1)
        n = 65536
        idx = rng.randint(table.shape[0], size=n)
        gains = rng.uniform(0.5, 1, (n, 3)) if kind == "colored" else None
        codes = torch.empty(n, 5, dtype=torch.float64, device="cuda")
        rep.codes(table, idx, gains, out=codes)                  # warm-up: engines, panels
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            rep.codes(table, idx, gains, out=codes)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[f"{kind}_codes_img_per_s_b4096"] = round(n / min(ts))
        factor_vae_full(kind, P, E, table)                       # warm-up
        plan_s, dev_s, metric = factor_vae_full(kind, P, E, table)
        out[f"{kind}_factor_vae_full_plan_s"] = round(plan_s, 3)
        out[f"{kind}_factor_vae_full_device_s"] = round(dev_s, 3)
        np.random.seed(0)
        t0 = time.perf_counter()
        plan = eg.score.mig_plan(table.shape[0], kind == "colored")
        c = rep.codes(table, plan["idx"], plan["gains"])
        score, _, _ = eg.score.mig(c, np.stack([plan["idx"] % 3, plan["idx"] % 6, plan["idx"] % 40, plan["idx"] % 32, plan["idx"] // 32 % 32], 1))
        out[f"{kind}_mig_1000_s"] = round(time.perf_counter() - t0, 4)
    return out


def kernel_split(outdir):
    d = os.path.join(outdir, "score_prof")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "score", "-f", "csv", "--", sys.executable, os.path.abspath(__file__), "--inner"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        return {}
    rows = list(csv.DictReader(open(stats[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    split = {}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]:
        split[r["Name"][:60]] = round(100.0 * float(r["TotalDurationNs"]) / tot, 1)
    return {"factor_vae_kernel_ms": round(tot / 1e6, 2), "factor_vae_kernel_pct": split}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true", help="(child of the profiled run) one dSprites FactorVAE run at full size")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default=None, help="directory for the rocprofv3 output (default: a fresh temporary directory)")
    a = ap.parse_args()
    if a.inner:
        P, E, table = setup("dsprites")
        factor_vae_full("dsprites", P, E, table)
        torch.cuda.synchronize()
        sys.exit(0)
    res = {"metric": "score_throughput", **measure()}
    if not a.no_prof:
        res.update(kernel_split(a.out or tempfile.mkdtemp(prefix="score_prof_")))
    print(json.dumps(res))

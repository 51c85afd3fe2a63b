"""Cost of the device loss log: the same captured trainer with and without ``log=`` -- CelebA bf16 B = 128 and dSprites bf16
B = 128 -- as alternating A/B blocks in one process on one GPU.  Two trainers per workload (identical modules and sampler seed), each
captured once; every round times a block of replays of A (no log) and then of B (log attached: one eg_runlog_append node at the tail
of the graph; for dSprites also the two loss-only launches of the separate info terms).  Prints one table; pipe it into
profiles/train_run_overhead.txt.

    python profiles/scripts/train_run_overhead.py [--rounds 8] [--steps 200]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
DEV = torch.device("cuda:0")


def sprites(n, g):
    return (torch.rand((n, 64, 64), device=DEV, generator=g) < 0.1).to(torch.uint8)


def build(workload, B, with_log):
    torch.manual_seed(0)
    g = torch.Generator(device=DEV).manual_seed(1000)
    if workload == "celeba":
        G, D = eg.celeba.Generator(dtype="bf16").to(DEV), eg.celeba.Discriminator(dtype="bf16").to(DEV)
        tr = eg.celeba.CelebATrainer(G, D, B, dtype="bf16")
        inp = eg.celeba.DeviceInputs(torch.randint(0, 256, (4096, 3, 64, 64), device=DEV, dtype=torch.uint8, generator=g), seed=1000)
    else:
        m = eg.dsprites
        mods = [m.Encoder_pxy(dtype="bf16").to(DEV), m.Generator(dtype="bf16").to(DEV), m.Discriminator(dtype="bf16").to(DEV), m.Encoder(dtype="bf16").to(DEV)]
        tr = m.DspritesTrainer(*mods, B, dtype="bf16")
        inp = m.DeviceInputs(sprites(8192, g), seed=1000)
    tr.inputs = inp
    log = eg.engine.LossLog(tr, 1024) if with_log else None
    if log is not None:
        tr.log = log
    tr.step_resident()
    tr.capture(inputs=inp, log=log)
    return tr, log


def block(tr, log, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step_resident()
        if log is not None and i % 100 == 99:
            log.flush_async()                            # what the driver does at print cadence
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    print(f"# ms per captured iteration, B = {a.batch}, bf16, {a.rounds} alternating rounds of {a.steps} replays; A = no log, B = log attached")
    for workload in ("celeba", "dsprites"):
        ta, _ = build(workload, a.batch, False)
        tb, log = build(workload, a.batch, True)
        for tr, lg in ((ta, None), (tb, log)):
            block(tr, lg, 50)                            # warm-up
        A, Bm = [], []
        for r in range(a.rounds):
            A.append(block(ta, None, a.steps))
            Bm.append(block(tb, log, a.steps))
            print(f"{workload:9s} round {r}: A {A[-1]:.4f}  B {Bm[-1]:.4f}  B-A {Bm[-1] - A[-1]:+.4f}", flush=True)
        ma, mb = statistics.median(A), statistics.median(Bm)
        print(f"{workload:9s} median A {ma:.4f} ms (spread {min(A):.4f} .. {max(A):.4f}), median B {mb:.4f} ms (spread {min(Bm):.4f} .. {max(Bm):.4f}), "
              f"B-A {mb - ma:+.4f} ms = {100 * (mb - ma) / ma:+.2f} %; inside the spread of A: {abs(mb - ma) <= max(A) - min(A)}", flush=True)
        del ta, tb, log


if __name__ == "__main__":
    main()

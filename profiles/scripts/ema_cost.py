"""Cost of weight averaging, two measurements in one process on one GPU.  Prints one table; pipe it into profiles/ema_cost.txt.

1. In the step: the same captured trainer with and without ``attach_ema()`` -- CelebA bf16 and dSprites bf16 at B = 128 -- as alternating
   A/B blocks (the method of train_run_overhead.py): two trainers per workload (identical modules and sampler seed), each captured once;
   every round times a block of replays of A (no average) and then of B (one eg_ema_update node at the tail of the graph).
2. The kernel alone: a hipGraph of 10 eg_ema_update launches over the table of CelebA's generator, timed with device events, next to
   (a) torch: ``lerp_`` on the flat fp32 tensors plus one ``lerp_`` / ``copy_`` per buffer, eagerly and as a graph of 10 such passes, and
   (b) a device-to-device copy of the bytes the launch moves (12 per averaged word, 8 per copied word), the rate ceiling.

    python profiles/scripts/ema_cost.py [--rounds 8] [--steps 200]"""
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


def build(workload, B, with_ema, capture=True):
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
    if with_ema:
        tr.attach_ema(0.999, ramp=10.0)
    if capture:
        tr.step_resident()
        tr.capture(inputs=inp)
    return tr


def block(tr, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step_resident()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def in_the_step(a):
    print(f"# ms per captured iteration, B = {a.batch}, bf16, {a.rounds} alternating rounds of {a.steps} replays; A = no average, B = attach_ema()")
    for workload in ("celeba", "dsprites"):
        ta, tb = build(workload, a.batch, False), build(workload, a.batch, True)
        words = sum(int(s[0].numel() * s[0].element_size() // 4) for s in tb.ema._segments)
        for tr in (ta, tb):
            block(tr, 50)                                # warm-up
        A, Bm = [], []
        for r in range(a.rounds):
            A.append(block(ta, a.steps))
            Bm.append(block(tb, a.steps))
            print(f"{workload:9s} round {r}: A {A[-1]:.4f}  B {Bm[-1]:.4f}  B-A {Bm[-1] - A[-1]:+.4f}", flush=True)
        ma, mb = statistics.median(A), statistics.median(Bm)
        print(f"{workload:9s} {tb.ema.nseg} segments, {words} words; median A {ma:.4f} ms (spread {min(A):.4f} .. {max(A):.4f}), median B {mb:.4f} ms "
              f"(spread {min(Bm):.4f} .. {max(Bm):.4f}), B-A {mb - ma:+.4f} ms = {100 * (mb - ma) / ma:+.2f} %; inside the spread of A: "
              f"{abs(mb - ma) <= max(A) - min(A)}", flush=True)
        del ta, tb


def timed(fn, reps):
    """median / min / max ms of ``reps`` calls of fn, each between two device events"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def graph_of(fn, n):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g


def kernel_alone(a):
    tr = build("celeba", 8, True, capture=False)
    ema = tr.ema
    segs = ema._segments
    lerp_words = sum(s.numel() for s, d, k in segs if k == 0)
    copy_words = sum(s.numel() * s.element_size() // 4 for s, d, k in segs if k == 1)
    moved = 12 * lerp_words + 8 * copy_words
    N = 10
    print(f"# the kernel alone: CelebA generator table, {ema.nseg} segments, {lerp_words} averaged + {copy_words} copied words, {moved / 1e6:.1f} MB moved "
          f"per launch; {N} launches per timing, {a.reps} timings each (median, min .. max), per launch")

    def torch_pass():
        for s, d, k in segs:
            if k == 0:
                d.lerp_(s, 0.001)
            else:
                d.copy_(s)

    src = torch.empty(moved // 8, device=DEV, dtype=torch.float32)
    dst = torch.empty_like(src)
    rows = [("eg_ema_update, graph of 10", graph_of(ema.update, N).replay),
            ("eg_ema_update, 10 eager launches", lambda: [ema.update() for _ in range(N)]),
            (f"torch lerp_/copy_ ({len(segs)} launches per pass), graph of 10", graph_of(torch_pass, N).replay),
            (f"torch lerp_/copy_ ({len(segs)} launches per pass), 10 eager passes", lambda: [torch_pass() for _ in range(N)]),
            ("device-to-device copy of the same bytes, graph of 10", graph_of(lambda: dst.copy_(src), N).replay)]
    for name, fn in rows:
        fn()
        torch.cuda.synchronize()
        med, lo, hi = timed(fn, a.reps)
        print(f"{name:70s} {med / N * 1e3:8.1f} us ({lo / N * 1e3:.1f} .. {hi / N * 1e3:.1f})  {moved / (med / N * 1e-3) / 1e9:8.0f} GB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("step", "kernel"), default=None)
    a = ap.parse_args()
    if a.only != "step":
        kernel_alone(a)
    if a.only != "kernel":
        in_the_step(a)


if __name__ == "__main__":
    main()

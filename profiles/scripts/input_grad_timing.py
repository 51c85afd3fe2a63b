"""Time of eg_linear_dinput at the production shapes (B = 128; the three layout rows of DESIGN 6k) next to torch.matmul on the same fp32
operands, and of one sampling.project_images step next to one eval forward, on one MI355X; run from the repo root.
Kernel rows: each variant is captured into a hipGraph of CHAIN back-to-back launches and replayed REPLAYS times between two device events
(after WARM replays); five windows, median / min / max per launch.  Bytes: the fp32 master once, dH once, the split partials written and
read once, dX.  Projection rows: eager launches, wall clock around a synchronise, (time of STEPS_B steps - time of STEPS_A steps) per step."""
import importlib, os, statistics, sys, time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops = eg.ops

B = 128
CHAIN, WARM, REPLAYS, WINDOWS = 10, 20, 100, 5
ROWS = {"celeba   NI,NJ = 16,1024  K = 218": (16, 1024, 218, (1, 16, 16384), 218 * 16384),
        "mnist    NI,NJ = 64,128   K = 79": (64, 128, 79, (79, 64 * 79, 1), 8192 * 79),
        "dsprites NI,NJ = 1,128    K = 7": (1, 128, 7, (0, 7, 1), 128 * 7),
        "colored  NI,NJ = 1,128    K = 10": (1, 128, 10, (0, 10, 1), 128 * 10)}
DTYPES = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}


def graph_time(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CHAIN):
            fn()
    for _ in range(WARM):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (REPLAYS * CHAIN))
    return statistics.median(times), min(times), max(times)


torch.manual_seed(0)
print(f"B = {B}; graph of {CHAIN} launches, {REPLAYS} replays a window, {WINDOWS} windows; us per launch (median min max), MB moved, GB/s at the median", flush=True)
for name, (NI, NJ, K, strides, wn) in ROWS.items():
    W = torch.randn(wn, device="cuda") * 0.05
    dX = torch.empty(B, K, device="cuda")
    nws = ops.linear_dinput_ws_floats(B, NI, NJ, K)
    ws = torch.empty(max(1, nws), device="cuda")
    for dname, (dt, tdt) in DTYPES.items():
        dH = torch.randn(B, NI * NJ, device="cuda").to(tdt)
        med, lo, hi = graph_time(lambda: ops.linear_dinput(dt, dH, NI * NJ, W, dX, B, NI, NJ, K, *strides, ws))
        mb = (NI * NJ * K * 4 + dH.numel() * dH.element_size() + 2 * nws * 4 + dX.numel() * 4) / 1e6
        print(f"eg_linear_dinput {name} {dname:4s} {med:8.2f} {lo:8.2f} {hi:8.2f}   {mb:7.2f} MB  {mb / med * 1e3:8.1f} GB/s", flush=True)
    i, j, k = torch.arange(NI).view(NI, 1, 1), torch.arange(NJ).view(1, NJ, 1), torch.arange(K).view(1, 1, K)
    Wv = W[(i * strides[0] + j * strides[1] + k * strides[2]).reshape(NI * NJ, K).cuda()].contiguous()      # [NI*NJ][K] fp32, gathered once
    dH32 = torch.randn(B, NI * NJ, device="cuda")
    out = torch.empty(B, K, device="cuda")
    med, lo, hi = graph_time(lambda: torch.matmul(dH32, Wv, out=out))
    print(f"torch.matmul     {name} f32  {med:8.2f} {lo:8.2f} {hi:8.2f}   (contiguous [NI*NJ][K] copy of the master, fp32 operands)", flush=True)

STEPS_A, STEPS_B, PB = 10, 60, 4
GENS = {"celeba": lambda: eg.celeba.Generator(), "mnist": lambda: eg.mnist.Generator(),
        "dsprites": lambda: eg.dsprites.Generator(code_dim=4, n_classes=3, channels=1), "colored": lambda: eg.colored.Generator()}
print(f"\nsampling.project_images, fp32, B = {PB}: us per step (eager, wall clock) next to one eval forward of the same engine", flush=True)
for kind, make in GENS.items():
    G = make().cuda().eval().requires_grad_(False)
    sprite = kind in ("dsprites", "colored")
    labels = torch.nn.functional.one_hot(torch.arange(PB) % G.n_classes, G.n_classes).float().cuda()
    code = torch.rand(PB, G.code_dim, device="cuda") * 2 - 1
    noise = None if sprite else torch.randn(PB, G.latent_dim, device="cuda")
    with torch.no_grad():
        target = G(torch.cat((labels, code), 1)) if sprite else G(noise, labels, code)

    def wall(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eg.sampling.project_images(kind, G, target, labels, steps, 0.05)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    wall(STEPS_A)
    per = statistics.median((wall(STEPS_B) - wall(STEPS_A)) / (STEPS_B - STEPS_A) for _ in range(5)) * 1e6
    eng = G.engine(PB)
    fwd = (lambda: eng.forward(labels, code, training=False)) if sprite else (lambda: eng.forward(noise, labels, code, training=False))
    fwd()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        fwd()
    torch.cuda.synchronize()
    print(f"{kind:9s} project_images step {per:8.1f}   eval forward {(time.perf_counter() - t0) / 200 * 1e6:8.1f}", flush=True)

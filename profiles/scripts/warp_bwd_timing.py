"""Time of eg_warp_affine_bwd next to the forward warp at the CelebA shape (128, 3, 64, 64) on one MI355X; run from the repo root.
Each variant is captured into a hipGraph of CHAIN back-to-back launches and replayed REPLAYS times between two device events (after
WARM replays); five windows, the median and the spread are printed, per launch."""
import importlib, os, statistics, sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
eg = importlib.import_module("ead-gan_amd")
ops = eg.ops

B, C, H, W = 128, 3, 64, 64
CHAIN, WARM, REPLAYS, WINDOWS = 10, 20, 200, 5
torch.manual_seed(0)
img = torch.rand(B, C, H, W, device="cuda")
code = torch.rand(B, 5, device="cuda") * 2 - 1
theta = torch.empty(B, 2, 3, device="cuda")
ops.theta_rpqxy(code, 5, B, theta)
dout = torch.randn(B, C, H, W, device="cuda")
out, dimg, dtheta = torch.empty_like(img), torch.empty_like(img), torch.empty(B, 6, device="cuda")
far = torch.tensor([[1.0, 0, 4], [0, 1.0, 4]], device="cuda").repeat(B, 1, 1)          # every tap outside: 'zeros' adds nothing to the plane

VARIANTS = {
    "forward  eg_warp_affine (border)": lambda: ops.warp_affine(img, theta, out, B, C, H, W),
    "forward  eg_warp_affine_zeros": lambda: ops.warp_affine_zeros(img, theta, out, B, C, H, W),
    "backward border dimg + dtheta": lambda: ops.warp_affine_bwd(img, theta, dout, dimg, dtheta, B, C, H, W),
    "backward border dimg only": lambda: ops.warp_affine_bwd(img, theta, dout, dimg, None, B, C, H, W),
    "backward border dtheta only": lambda: ops.warp_affine_bwd(img, theta, dout, None, dtheta, B, C, H, W),
    "backward zeros  dimg + dtheta": lambda: ops.warp_affine_bwd(img, theta, dout, dimg, dtheta, B, C, H, W, zeros=True),
    "backward zeros  dimg only, no tap inside": lambda: ops.warp_affine_bwd(img, far, dout, dimg, None, B, C, H, W, zeros=True),
}

print(f"shape ({B}, {C}, {H}, {W}); graph of {CHAIN} launches, {REPLAYS} replays a window, {WINDOWS} windows; us per launch", flush=True)
for name, fn in VARIANTS.items():
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
    print(f"{name:42s} median {statistics.median(times):7.2f}  min {min(times):7.2f}  max {max(times):7.2f}", flush=True)

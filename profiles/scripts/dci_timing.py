"""Wall time of the DCI moments + Lasso fits at n = 73 728 on the device, next to sklearn's five default fits on this host's CPU."""
import importlib, os, sys, time, warnings
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
eg = importlib.import_module("ead-gan_amd")
import make_dci_golden as gen
codes, fv = gen.production_set()
n, k = codes.shape; nf = fv.shape[1]; m = k + nf
dev = "cuda"
cd, fd = torch.from_numpy(codes).to(dev), torch.from_numpy(fv).to(dev)
ws = torch.empty(eg.ops.score_norm_gram_ws_bytes(n, k, nf), device=dev, dtype=torch.uint8)
mean, std = torch.empty(m, device=dev, dtype=torch.float64), torch.empty(m, device=dev, dtype=torch.float64)
G = torch.empty(m, m, device=dev, dtype=torch.float64); status = torch.zeros(2, device=dev, dtype=torch.int32)
W = torch.empty(nf, k, device=dev, dtype=torch.float64); info = torch.empty(nf, 4, device=dev, dtype=torch.float64)
tol = eg.score.DCI_KKT_TOL
def moments(): eg.ops.score_norm_gram(cd, fd, n, k, nf, ws, mean, std, G, status)
def fit(): eg.ops.score_lasso_gram_fit(G, k, nf, 0.02, 10000, tol, W, info)
def both(): moments(); fit()
def timed(fn, reps):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): fn()
        b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return out
for name, fn in (("moments", moments), ("fit", fit), ("moments+fit", both)):
    t = timed(fn, 500)
    print(f"{name}: device-event time per call, 5 windows of 500 calls, us: " + " ".join(f"{v:.1f}" for v in t), flush=True)
print("sweeps", info.cpu().numpy()[:, 0], "status", info.cpu().numpy()[:, 3], "bytes read per moments call", 2 * n * m * 8)
ts = []
for _ in range(5):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = eg.score.lasso_fit(cd, fd)
    ts.append((time.perf_counter() - t0) * 1e3)
print("lasso_fit wall (allocations, two entry points, one host read), ms:", " ".join(f"{v:.3f}" for v in ts))
from sklearn.linear_model import Lasso
Z, Y = gen.normalize(codes), gen.normalize(fv)
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        coefs = [Lasso(alpha=0.02).fit(Z, Y[:, j]).coef_ for j in range(nf)]
    ts.append((time.perf_counter() - t0) * 1e3)
print("sklearn", __import__("sklearn").__version__, "normalize + five default Lasso fits on the CPU (", os.cpu_count(), "logical CPUs, threads limited to", os.environ.get("OMP_NUM_THREADS"), "), ms:", " ".join(f"{v:.2f}" for v in ts))
t0 = time.perf_counter(); gen.normalize(codes); gen.normalize(fv); print("of which numpy normalize, ms: %.2f" % ((time.perf_counter() - t0) * 1e3))
print("max|device W - sklearn default coef|", np.abs(res["W"].cpu().numpy() - np.stack(coefs)).max())

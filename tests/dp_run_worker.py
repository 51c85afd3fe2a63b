"""Worker of tests/test_gpu_dp_run.py: one rank of a data-parallel ``train.TrainRun`` of the CelebA trainer on the (shared) GPU, gloo
backend, or the one-process run at the same global batch.  Kept free of pytest imports so that torch.multiprocessing can spawn it."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_IMAGES = 20
B_GLOBAL = 8


def _dataset():
    g = torch.Generator().manual_seed(4)
    return torch.randint(0, 256, (N_IMAGES, 3, 64, 64), dtype=torch.uint8, generator=g).to("cuda")


def _trainer(eg, rank, world, lr0, seed):
    """fp32 modules, ``lr0``: the seeded weights of the test infrastructure and all learning rates 0; else torch's default initialisation
    from ``seed`` and the trainer's default learning rates"""
    torch.manual_seed(seed)
    G, D = eg.celeba.Generator(dtype="f32").to("cuda"), eg.celeba.Discriminator(dtype="f32").to("cuda")
    if lr0:
        from oracle import celeba_oracle as co
        orc = co.CelebAOracle(seed=3, lrs=(0.0, 0.0, 0.0))
        G.load_state_dict({k: v.detach() for k, v in orc.G.items()})
        D.load_state_dict({k: v.detach() for k, v in orc.D.items()})
    kw = dict(lr_g=0.0, lr_d=0.0, lr_info=0.0) if lr0 else {}
    if world > 1:
        kw.update(allreduce=eg.dp.GradAllReduce(world), sync_bn=eg.dp.SyncBN(world, rank))
    tr = eg.celeba.CelebATrainer(G, D, B_GLOBAL // world, dtype="f32", **kw)
    inp = eg.celeba.DeviceInputs(_dataset(), seed=5, rank=rank, world=world)
    return tr, inp


def _result(run, tr, out_dir):
    """what two runs are compared on, as plain tensors / lists (loads with weights_only=True)"""
    out = {f"state/{k}": v for k, v in tr.state_dict().items() if isinstance(v, torch.Tensor)}
    out["history"] = torch.from_numpy(run.history.copy())
    out["lines"] = list(run.lines)
    out["files"] = sorted(os.path.relpath(f, out_dir) for f in run.files)
    out["waits"] = list(run.waits)
    present = []
    if os.path.isdir(out_dir):
        for root, _, files in os.walk(out_dir):
            for f in sorted(files):
                p = os.path.join(root, f)
                rel = os.path.relpath(p, out_dir)
                present.append(rel)
                if f.endswith(".png"):
                    out[f"png/{rel}"] = torch.frombuffer(bytearray(open(p, "rb").read()), dtype=torch.uint8).clone()
                elif f == "losses.npy":
                    import numpy as np
                    out["losses.npy"] = torch.from_numpy(np.load(p))
    out["present"] = sorted(present)
    return out


def _run(eg, rank, world, out_dir, lr0, iters, seed=1):
    tr, inp = _trainer(eg, rank, world, lr0, seed)
    run = eg.train.TrainRun("celeba", tr, inp, out_dir, n_epochs=2, sample_interval=2, seed=3, graph=False, log_capacity=16)
    run.run(max_iters=iters)
    return run, tr


def run_rank(rank, world, port, outdir):
    """world 1: the one-process run at B = 8, learning rates 0.  world 2: that run on two ranks at B = 4 each, then with the default
    learning rates two uninterrupted runs of 4 iterations (A and the control A') and the run interrupted after 2 and resumed on fresh
    modules (B).  Every rank writes ``<outdir>/<name>_rank<r>_of<w>.pt``; run directories are ``<outdir>/<name>_of<w>`` (rank 0 writes)."""
    eg = importlib.import_module("ead-gan_amd")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if world > 1:
        eg.dp.init_from_env(backend="gloo")
    torch.cuda.set_device(0)

    def save(name, run, tr):
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()              # rank 0's files are complete before anybody lists the directory
        torch.save(_result(run, tr, os.path.join(outdir, f"{name}_of{world}")), os.path.join(outdir, f"{name}_rank{rank}_of{world}.pt"))

    run, tr = _run(eg, rank, world, os.path.join(outdir, f"lr0_of{world}"), True, 4)
    save("lr0", run, tr)
    if world > 1:
        for name in ("A", "A2"):
            run, tr = _run(eg, rank, world, os.path.join(outdir, f"{name}_of{world}"), False, 4)
            save(name, run, tr)
        bdir = os.path.join(outdir, f"B_of{world}")
        run, tr = _run(eg, rank, world, bdir, False, 2)
        lines, files = list(run.lines), list(run.files)
        torch.cuda.synchronize()
        torch.distributed.barrier()                  # run_state_2.pt of rank 0 is on disk
        tr2, inp2 = _trainer(eg, rank, world, False, 77)             # fresh modules from another seed, fresh collectives, fresh sampler
        run2 = eg.train.TrainRun.resume(os.path.join(bdir, "run_state_2.pt"), "celeba", tr2, inp2, bdir, n_epochs=2, sample_interval=2, seed=3,
                                        graph=False, log_capacity=16)
        assert run2.batches_done == 2
        run2.run(max_iters=2)
        run2.lines = lines + run2.lines
        run2.files = files + run2.files
        save("B", run2, tr2)
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()

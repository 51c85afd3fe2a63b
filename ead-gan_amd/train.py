"""Training runs: the part of the reference's scripts below the loop body -- progress lines, sample grids, checkpoint files
(celebA/EAD-GAN_celebA.py:403-423, MNIST/EAD-GAN_rpqmnxy.py:451-466, dSprites/rp.py:486-509, colored_dSprites/rp_color.py:518-541,
dSprites/pxy.py:189-205, colored_dSprites/pxy_color.py:218-234) -- around the fused trainers' ``step_resident()``, with a loss log that
lives on the device (engine.LossLog, written inside the captured iteration) and a full-state checkpoint from which a run continues bit
for bit (``trainer.state_dict()``).  The loop only enqueues; every blocking wait goes through ``TrainRun._wait`` and is recorded.
Data parallel: one TrainRun per rank around a trainer with ``allreduce`` / ``sync_bn`` and a sampler sharded by (rank, world); eager
launches only, rank 0 alone prints and writes, and the run adds no collective of its own."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import ops, quality, sampling
from .engine import LossLog

# One row per script.  print: the progress line's cadence; fmt: its format string, character for character; cols: which entries of the
# trainer's loss row fill it; sample / ckpt: multiples of ``sample_interval`` (None: the script's sample_image is not restated);
# minmax: labels of the four extra print lines of the dSprites scripts; interval: the script's --sample_interval default.
_HEAD = "[Epoch %d/%d] [Batch %d/%d] "
_RUNS = {
    "celeba": dict(print=10, fmt=_HEAD + "[D loss: %f] [G loss: %f]", cols=(1, 0), sample=1, ckpt=15, grid="celeba_train", interval=4000,
                   minmax=None),                                                                    # celebA/EAD-GAN_celebA.py:404-414
    "mnist": dict(print=100, fmt=_HEAD + "[D loss: %f] [G loss: %f] [info loss: %f]", cols=(1, 0, 2), sample=1, ckpt=10, grid="mnist_train",
                  interval=4000, minmax=None),                                                      # MNIST/EAD-GAN_rpqmnxy.py:453-462
    "dsprites": dict(print=100, fmt=_HEAD + "[D loss: %f] [G loss: %f] [info cat loss: %f] [info cont loss: %f] [affine loss: %f] "
                                            "[relative_cat_loss: %f] ", cols=(0, 1, 5, 6, 3, 4), sample=2, ckpt=500, grid="dsprites_train",
                     interval=1000, minmax="trans_img_affine"),                                     # dSprites/rp.py:491-507
    "colored": dict(print=100, fmt=_HEAD + "[D loss: %f] [G loss: %f] [info cat loss: %f] [info cont loss: %f] [affine_color loss: %f] "
                                           "[relative_cat_loss: %f] ", cols=(0, 1, 5, 6, 3, 4), sample=2, ckpt=50, grid="colored_train",
                    interval=1000, minmax="trans_img_affine_color"),                                # colored_dSprites/rp_color.py:523-539
    "pxy": dict(print=100, fmt=_HEAD + "[D loss: %f]", cols=(0,), sample=None, ckpt=50, grid=None, interval=1000, minmax=None),   # dSprites/pxy.py:194-204
    "pxy_color": dict(print=100, fmt=_HEAD + "[D loss: %f]", cols=(0,), sample=None, ckpt=10, grid=None, interval=1000,
                      minmax=None),                                                                 # colored_dSprites/pxy_color.py:223-233
}
KINDS = tuple(_RUNS)
WAIT_REASONS = ("ring-full", "sample", "checkpoint", "end")


class NonFiniteLoss(RuntimeError):
    """a loss of iteration ``iteration`` (1-based, as the device log latches it) was NaN or infinite; nothing was saved afterwards"""

    def __init__(self, iteration):
        super().__init__(f"non-finite loss first seen at iteration {iteration}")
        self.iteration = int(iteration)


def _plan(kind):
    if kind not in _RUNS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    return _RUNS[kind]


def cadence(kind, batches_done, sample_interval=None):
    """-> (print?, sample?, checkpoint?) for the iteration that has just run: the scripts' ``batches_done % k == 0`` tests, so iteration
    0 prints, samples and saves"""
    p = _plan(kind)
    si = p["interval"] if sample_interval is None else int(sample_interval)
    return (batches_done % p["print"] == 0,
            p["sample"] is not None and batches_done % (si * p["sample"]) == 0,
            batches_done % (si * p["ckpt"]) == 0)


def loader_len(n_images, batch_size):
    """len(DataLoader(dataset, batch_size)) with drop_last=False"""
    return -(-int(n_images) // int(batch_size))


def progress_line(kind, batches_done, n_epochs, n_images, batch_size, row):
    """the script's progress line for the iteration ``batches_done`` with the loss row the trainer wrote in it"""
    p = _plan(kind)
    L = loader_len(n_images, batch_size)
    return p["fmt"] % ((batches_done // L, n_epochs, batches_done % L, L) + tuple(float(row[c]) for c in p["cols"]))


def minmax_lines(kind, vals):
    """the four extra lines of the dSprites scripts (rp.py:498-501): ``vals`` = (trans min, trans max, gen min, gen max).  The values
    print as torch prints a 0-dim device tensor (the reference's gen_imgs lines also carry a grad_fn, which is not restated)."""
    name = _plan(kind)["minmax"]
    t = lambda v: str(torch.tensor(float(v), dtype=torch.float32))[:-1] + ", device='cuda:0')"
    return [f"{name} max {t(vals[1])}", f"gen_imgs max {t(vals[3])}", f"{name} min {t(vals[0])}", f"gen_imgs min {t(vals[2])}"]


_FILES = {"celeba": ("checkpoint_%d.tar",), "mnist": ("generator_%d.pt", "encoder_%d.pt"), "dsprites": ("encoder_%d.pt", "generator_%d.pt"),
          "colored": ("encoder_%d.pt", "generator_%d.pt"), "pxy": ("encoder_pxy_%d.pt",), "pxy_color": ("encoder_pxy_color_%d.pt",)}


def checkpoint_files(kind, batches_done):
    """names of the reference-format files one checkpoint iteration writes (celebA.py:415, rpqmnxy.py:465-466, rp.py:508-509,
    rp_color.py:540-541, pxy.py:205, pxy_color.py:234)"""
    _plan(kind)
    return [n % batches_done for n in _FILES[kind]]


# the file stem each script gives a module's checkpoint; the averaged copy of a module carries ``_ema`` before the number.  CelebA's script
# writes one .tar dictionary: its averaged generator is a bare state dict, what sampling.load_generator also reads
_EMA_STEMS = {"celeba": {"G": "generator", "D": "discriminator"}, "mnist": {"G": "generator", "E": "encoder", "D": "discriminator"},
              "dsprites": {"E": "encoder", "G": "generator", "D": "discriminator", "P": "encoder_pxy"},
              "colored": {"E": "encoder", "G": "generator", "D": "discriminator", "P": "encoder_pxy_color"},
              "pxy": {"P": "encoder_pxy"}, "pxy_color": {"P": "encoder_pxy_color"}}


def ema_checkpoint_files(kind, batches_done, names):
    """names of the files a checkpoint iteration adds for the averaged weights of the tracked modules ``names``, in their
    order: the script's own name of that module's file with ``_ema`` before the number (``generator_ema_%d.pt``, ``encoder_ema_%d.pt``,
    ``encoder_pxy_ema_%d.pt``, ...), each a bare state dict"""
    _plan(kind)
    stems = _EMA_STEMS[kind]
    for n in names:
        if n not in stems:
            raise ValueError(f"ema_checkpoint_files: a {kind!r} trainer has no module {n!r} (it has {', '.join(stems)})")
    return [f"{stems[n]}_ema_{int(batches_done)}.pt" for n in names]


def _module_like(module):
    """a fresh module of ``module``'s class and dimensions, on the CPU: the drop-in classes keep every constructor argument as an attribute
    of the same name (``dtype`` as ``compute_dtype``)"""
    import inspect
    kw = {}
    for name in inspect.signature(type(module).__init__).parameters:
        if name == "dtype":
            kw[name] = module.compute_dtype
        elif name != "self":
            kw[name] = getattr(module, name)
    return type(module)(**kw)


def sample_seed(seed, batches_done):
    """seed of the sample grids' numpy draws: a function of (run seed, iteration), so a resumed run writes the same PNG bytes"""
    return (int(seed) * 1000003 + int(batches_done) * 7919 + 12345) % (2 ** 32)


def swd_seed(seed, batches_done, plan_seed=0):
    """seed of a checkpoint iteration's SWD draws: a function of (run seed, iteration, the plan's own seed) like ``sample_seed``, so a
    resumed run writes the same line"""
    return (int(seed) * 1000003 + int(batches_done) * 6151 + int(plan_seed) * 104729 + 54321) % (2 ** 32)


def nn_seed(seed, batches_done, plan_seed=0):
    """seed of a checkpoint iteration's generated images for the nearest-neighbour scores: ``swd_seed``'s form with constants of its own"""
    return (int(seed) * 1000003 + int(batches_done) * 4447 + int(plan_seed) * 130003 + 98765) % (2 ** 32)


def mmd_seed(seed, batches_done, plan_seed=0):
    """seed of a checkpoint iteration's generated images for the kernel MMD: ``swd_seed``'s form with constants of its own"""
    return (int(seed) * 1000003 + int(batches_done) * 5381 + int(plan_seed) * 115249 + 24680) % (2 ** 32)


def sinkhorn_seed(seed, batches_done, plan_seed=0):
    """seed of a checkpoint iteration's generated images for the Sinkhorn divergence: ``swd_seed``'s form with constants of its own"""
    return (int(seed) * 1000003 + int(batches_done) * 3571 + int(plan_seed) * 122949 + 13579) % (2 ** 32)


def ndb_seed(seed, batches_done, plan_seed=0):
    """seed of a checkpoint iteration's generated images for the NDB score: ``swd_seed``'s form with constants of its own.  (The bins of
    the real images are fitted once, from the plan's own seed.)"""
    return (int(seed) * 1000003 + int(batches_done) * 2909 + int(plan_seed) * 137911 + 86420) % (2 ** 32)


def spectrum_seed(seed, batches_done, plan_seed=0):
    """seed of a checkpoint iteration's generated images for the radial power-spectrum score: ``swd_seed``'s form with constants of its
    own"""
    return (int(seed) * 1000003 + int(batches_done) * 4099 + int(plan_seed) * 150989 + 24680) % (2 ** 32)


def ssim_seed(seed, batches_done, plan_seed=0):
    """seed of a checkpoint iteration's generated images for the pair diversity (MS-SSIM): ``swd_seed``'s form with constants of its own.
    (The pair table is drawn once, from the plan's own seed.)"""
    return (int(seed) * 1000003 + int(batches_done) * 4597 + int(plan_seed) * 163841 + 97531) % (2 ** 32)


def check_plan(what, plan, cls, kind, n_dataset, batch):
    """-> ``plan`` as a ``cls`` (quality.SWDPlan, NNPlan, MMDPlan, SinkhornPlan, NDBPlan, SpectrumPlan or SSIMPlan) after the checks every
    score plan of a run passes: the kind of the run, ``n_images`` against the dataset and against the trainer's batch size; an MMD plan
    also needs two images a set and 1 .. 4 positive scales, a Sinkhorn plan two images a set, a positive scale and at least one iteration,
    an NDB plan 1 .. min(1024, n_images) bins and no negative iteration count, a spectrum plan two images a set, an SSIM plan two images
    a set and at least one pair"""
    if kind not in ("mnist", "celeba"):
        raise ValueError(f"{what}: only 'mnist' and 'celeba' runs are scored (quality.generate), not {kind!r}")
    plan = cls(*plan)
    if not 1 <= int(plan.n_images) <= int(n_dataset):
        raise ValueError(f"{what}: n_images = {plan.n_images}, the dataset has {n_dataset} images")
    if int(plan.n_images) % min(int(batch), int(plan.n_images)):                # the generator runs at the trainer's batch size
        raise ValueError(f"{what}: n_images = {plan.n_images} is no multiple of the trainer's batch size {batch}")
    if cls is quality.MMDPlan:
        if int(plan.n_images) < 2:
            raise ValueError(f"{what}: n_images = {plan.n_images}, the estimate needs at least 2 images a set")
        try:
            quality._positive(plan.scales, "MMDPlan", "scales")
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
    if cls is quality.SinkhornPlan:
        if int(plan.n_images) < 2:
            raise ValueError(f"{what}: n_images = {plan.n_images}, the divergence needs at least 2 images a set")
        try:
            quality._positive((plan.scale,), "SinkhornPlan", "scale")
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
        if int(plan.iterations) < 1:
            raise ValueError(f"{what}: iterations = {plan.iterations} must be at least 1")
    if cls is quality.NDBPlan:
        if not 1 <= int(plan.bins) <= min(ops.KMEANS_MAX_BINS, int(plan.n_images)):
            raise ValueError(f"{what}: bins = {plan.bins} must be in 1 .. min({ops.KMEANS_MAX_BINS}, n_images = {plan.n_images})")
        if int(plan.iterations) < 0:
            raise ValueError(f"{what}: iterations = {plan.iterations} must not be negative")
    if cls is quality.SpectrumPlan:
        if int(plan.n_images) < 2:
            raise ValueError(f"{what}: n_images = {plan.n_images}, the variance over a set needs at least 2 images")
    if cls is quality.SSIMPlan:
        if int(plan.n_images) < 2:
            raise ValueError(f"{what}: n_images = {plan.n_images}, a pair needs at least 2 images a set")
        if int(plan.n_pairs) < 1:
            raise ValueError(f"{what}: n_pairs = {plan.n_pairs} must be at least 1")
    return plan


class TrainRun:
    """``run(max_iters=None)`` continues from ``batches_done`` until ``n_epochs`` epochs of ``ceil(N / B)`` iterations are done or
    ``max_iters`` more iterations ran; ``save()`` writes ``run_state_<batches_done>.pt``; ``TrainRun.resume(path, ...)`` continues such a
    file on a fresh trainer.  ``graph=True``: the iteration (input draws, step, log append) is captured into one hipGraph;
    engine.CaptureFailed propagates (no in-process fallback).  ``log_in_graph=False``: the trainer runs without the log (its
    graph is node for node the one ``capture(inputs=...)`` alone gives) and the loop enqueues the append after every iteration -- the
    trade for the small-network steps, where the log's launches are measurable; the dSprites lines then print 0 for the two
    separate info terms, which only a trainer with a log computes.

    A trainer with averaged weights (``trainer.attach_ema(...)`` before the run): checkpoint iterations also write one bare
    state dict per tracked module (``ema_checkpoint_files``), after the script's own files.  ``ema_samples=True``: sample iterations
    also write the same grids from the averaged generator into ``out_dir/ema/`` -- a scratch generator, built once and filled by
    ``WeightEMA.copy_to``, in the live generator's mode on the same seeded inputs; nothing of it is state.

    ``swd=quality.SWDPlan(n_images, ...)`` ('mnist' and 'celeba' runs): on checkpoint iterations, after the checkpoint files,
    rank 0 scores a scratch copy of the live generator -- and, if the trainer averages ``G``, one filled by ``WeightEMA.copy_to`` --
    in the live generator's mode against the first ``n_images`` dataset images, and appends one JSON line ``{"batches_done", "G"[,
    "G_ema"]}`` to ``out_dir/swd.jsonl``.  The draws are seeded by ``swd_seed``; trainer, sampler and their counters are not touched, the
    other ranks do nothing and no collective is added.  The score's one host read follows the checkpoint's ``_wait``: the device is
    already drained, it waits for the score's own launches only.

    ``nn=quality.NNPlan(n_images, k=5, seed=0)`` (the same runs): on checkpoint iterations, after the SWD line if there
    is one, rank 0 appends ``{"batches_done", "G": {"two_sample": ..., "prdc": ...}[, "G_ema": ...]}`` to ``out_dir/nn.jsonl`` --
    ``quality.nn_two_sample`` and ``quality.prdc`` at ``k`` of ONE set of generated images per generator (seeded by ``nn_seed``) against
    the first ``n_images`` dataset images.  The scratch generator is the SWD plan's; nothing else of the run is touched.

    ``mmd=quality.MMDPlan(n_images, scales=(0.5, 1.0, 2.0), seed=0)`` (the same runs): on checkpoint iterations, after the
    ``nn.jsonl`` line if there is one, rank 0 appends ``{"batches_done", "G": quality.mmd(...)[, "G_ema": ...]}`` to ``out_dir/mmd.jsonl``
    -- the kernel MMD at ``scales`` times the median bandwidth of one set of generated images per generator (seeded by ``mmd_seed``)
    against the first ``n_images`` dataset images.  The same scratch generator; nothing else of the run is touched.

    ``sinkhorn=quality.SinkhornPlan(n_images, scale=0.1, iterations=60, seed=0)`` (the same runs): on checkpoint iterations,
    after the ``mmd.jsonl`` line if there is one, rank 0 appends ``{"batches_done", "G": quality.sinkhorn(...)[, "G_ema": ...]}`` to
    ``out_dir/sinkhorn.jsonl`` -- the debiased Sinkhorn divergence of one set of generated images per generator (seeded by
    ``sinkhorn_seed``) against the first ``n_images`` dataset images.  The same scratch generator; nothing else of the run is touched.

    ``ndb=quality.NDBPlan(n_images, bins=100, iterations=20, seed=0)`` (the same runs): on checkpoint iterations, after the
    ``sinkhorn.jsonl`` line if there is one, rank 0 appends ``{"batches_done", "G": quality.ndb(...)[, "G_ema": ...]}`` to
    ``out_dir/ndb.jsonl`` -- the number of statistically different bins of one set of generated images per generator (seeded by
    ``ndb_seed``) against the first ``n_images`` dataset images.  The real set does not change during a run: its bins are fitted once,
    at the first scored checkpoint, from the plan's seed, and kept on the run object (``ndb_bins``).  They are no part of
    ``run_state_%d.pt``: a resumed run refits them, and the fit is deterministic, so it gets the same bits.

    ``spectrum=quality.SpectrumPlan(n_images, seed=0)`` (the same runs): on checkpoint iterations, after the ``ndb.jsonl`` line
    if there is one, rank 0 appends ``{"batches_done", "G": quality.spectrum(...)[, "G_ema": ...]}`` to ``out_dir/spectrum.jsonl`` -- the
    radial power spectrum of one set of generated images per generator (seeded by ``spectrum_seed``) against that of the first
    ``n_images`` dataset images.  The real set's per-ring mean and variance are computed once, at the first scored checkpoint, and kept
    on the run object (``spectrum_real``); they are no part of ``run_state_%d.pt``: a resumed run recomputes the same bits.

    ``ssim=quality.SSIMPlan(n_images, n_pairs=4096, seed=0)`` (the same runs): on checkpoint iterations, after the
    ``spectrum.jsonl`` line if there is one, rank 0 appends ``{"batches_done", "G": {...}[, "G_ema": {...}]}`` to ``out_dir/ssim.jsonl``;
    every entry is ``quality.diversity`` (the mean MS-SSIM and SSIM over random pairs) of one set of generated images per generator
    (seeded by ``ssim_seed``) plus ``"real"``, the same dictionary of the first ``n_images`` dataset images, and ``"gap"``, the generated
    set's ms_ssim minus the real set's.  One pair table, drawn from the plan's seed, serves every set and every line.  The real set's
    diversity is computed once, at the first scored checkpoint, and kept on the run object (``ssim_real``); it is no part of
    ``run_state_%d.pt``: a resumed run recomputes the same bits.

    Data parallel (``inputs.world`` > 1, the world of the trainer's ``allreduce`` / ``sync_bn``): ``graph=False`` is required; the
    iteration count, cadence, sample seeds and file names are those of one process at the global batch ``B * world``; rank 0 prints and
    writes every file, the other ranks write none (``files == []``) and print nothing but execute every ``_wait`` and keep ``history``
    / ``lines`` of their own shard.  The run adds no collective: rank 0's lines and ``losses.npy`` carry rank 0's shard losses."""

    def __init__(self, kind, trainer, inputs, out_dir, n_epochs, sample_interval=None, seed=0, graph=True, log_capacity=1024, log_in_graph=True,
                 ema_samples=False, swd=None, nn=None, mmd=None, sinkhorn=None, ndb=None, spectrum=None, ssim=None):
        self.plan = _plan(kind)
        if getattr(trainer, "STATE_KIND", None) != kind:
            raise ValueError(f"a {kind!r} run needs a {kind!r} trainer, got {type(trainer).__name__}")
        self.rank, self.world = int(getattr(inputs, "rank", 0)), int(getattr(inputs, "world", 1))
        trainer_world = 1                                           # a trainer without collectives is one process
        for coll in (getattr(trainer, "allreduce", None), getattr(trainer, "sync_bn", None)):
            if coll is not None:
                trainer_world = int(getattr(coll, "world", 1))
                break
        if self.world != trainer_world:
            raise ValueError(f"the sampler shards the batch over world = {self.world} ranks, the trainer's collectives span {trainer_world}: "
                             "build the sampler with the rank / world of the trainer's allreduce / sync_bn")
        if graph and self.world > 1:
            raise ValueError(f"a data-parallel run (world = {self.world}) launches eagerly: pass graph=False (a captured multi-rank "
                             "iteration is not supported, DESIGN 6i)")
        self.kind, self.trainer, self.inputs, self.out_dir = kind, trainer, inputs, str(out_dir)
        self.n_epochs = int(n_epochs)
        self.sample_interval = self.plan["interval"] if sample_interval is None else int(sample_interval)
        self.seed, self.graph, self.log_in_graph = int(seed), bool(graph), bool(log_in_graph)
        self.log = LossLog(trainer, log_capacity)
        self.n_images = int(inputs.data.shape[0])
        self.global_batch = int(trainer.B) * self.world
        self.L = loader_len(self.n_images, self.global_batch)
        self.batches_done = 0
        self.history = np.zeros((0, self.log.n), np.float32)       # loss rows of the iterations [0, len)
        self.lines = []                                             # every line printed so far
        self.waits = []
        self.files = []                                             # reference-format files and run states written by this object
        self._prints = []                                           # (iteration, slot of its min / max values or None) not printed yet
        self._prepared = False
        self._enqueued = 0
        if self.rank == 0:
            os.makedirs(self.out_dir, exist_ok=True)
        trainer.inputs, trainer.log = inputs, (self.log if self.log_in_graph else None)
        self.ema_samples, self._ema_G = bool(ema_samples), None
        if self.ema_samples:
            if self.plan["grid"] is None:
                raise ValueError(f"ema_samples: the {kind!r} script has no sample_image, there is no grid to write")
            ema = getattr(trainer, "ema", None)
            if ema is None or "G" not in ema.names:
                raise ValueError("ema_samples: the trainer keeps no average of its generator -- call trainer.attach_ema(modules=('G', ...)) first")
            if self.rank == 0:
                self._ema_G = _module_like(trainer.G).to(trainer.losses.device)
        self.swd, self.nn, self.mmd, self.sinkhorn, self._score_G = swd, nn, mmd, sinkhorn, None       # one scratch generator serves every plan
        self.ndb, self.ndb_bins = ndb, None                         # ndb_bins: quality.Bins of the real images, fitted at the first scored checkpoint
        self.spectrum, self.spectrum_real = spectrum, None          # spectrum_real: quality.spectrum_moments of the real images [2, B], computed once
        self.ssim, self.ssim_real, self._ssim_pairs = ssim, None, None     # ssim_real: quality.diversity of the real images, computed once
        for what, plan, cls in (("swd", swd, quality.SWDPlan), ("nn", nn, quality.NNPlan), ("mmd", mmd, quality.MMDPlan),
                                ("sinkhorn", sinkhorn, quality.SinkhornPlan), ("ndb", ndb, quality.NDBPlan),
                                ("spectrum", spectrum, quality.SpectrumPlan), ("ssim", ssim, quality.SSIMPlan)):
            if plan is None:
                continue
            setattr(self, what, check_plan(what, plan, cls, kind, self.n_images, trainer.B))
            if self.rank == 0 and self._score_G is None:
                self._score_G = _module_like(trainer.G).to(trainer.losses.device)
        if self.nn is not None and not 1 <= int(self.nn.k) <= min(16, int(self.nn.n_images) - 1):
            raise ValueError(f"nn: k = {self.nn.k} must be in 1 .. min(16, n_images - 1) for n_images = {self.nn.n_images}")
        if self.plan["minmax"]:
            dev = trainer.losses.device
            self._mm_dev = torch.zeros(4, device=dev, dtype=torch.float32)
            self._mm_ws = torch.empty(ops.minmax_ws_floats(), device=dev, dtype=torch.float32)
            self._mm_host = torch.zeros(256, 4, dtype=torch.float32).pin_memory()
            self._mm_n = 0

    # -- host discipline ----------------------------------------------------------------------------
    def _wait(self, reason):
        """THE blocking wait of a run: drains the device, brings the loss log up to date, prints what is due"""
        assert reason in WAIT_REASONS, reason
        self.waits.append(reason)
        torch.cuda.synchronize()
        self.log.flush_async()
        self.log.wait()
        self._collect()

    def _collect(self):
        """take the rows of a landed copy (never blocks), print the lines whose rows are there, end the run on a non-finite loss"""
        if not self.log.landed():
            return
        head = self.log.mirror_head
        have = len(self.history)
        if head > have:
            if head - have > self.log.capacity:
                raise RuntimeError(f"loss log overrun: {head - have} rows since the last flush, capacity {self.log.capacity}")
            self.history = np.concatenate((self.history, self.log.rows(since=have)), 0)
        while self._prints and self._prints[0][0] < len(self.history):
            it, slot = self._prints.pop(0)
            out = [progress_line(self.kind, it, self.n_epochs, self.n_images, self.global_batch, self.history[it])]
            if slot is not None:
                out += minmax_lines(self.kind, self._mm_host[slot].tolist())
            if self.rank == 0:
                for ln in out:
                    print(ln, flush=True)
            self.lines += out
        if self.log.mirror_flag:
            raise NonFiniteLoss(self.log.mirror_flag)

    # -- pieces of an iteration's tail ----------------------------------------------------------------
    def _queue_print(self, it):
        slot = None
        if self.plan["minmax"]:
            tr = self.trainer
            slot = self._mm_n % self._mm_host.shape[0]
            self._mm_n += 1
            ops.minmax_f32(tr.trans2, tr.trans2.numel(), self._mm_ws, self._mm_dev[0:2])
            ops.minmax_f32(tr.ge2.img, tr.ge2.img.numel(), self._mm_ws, self._mm_dev[2:4])
            self._mm_host[slot].copy_(self._mm_dev, non_blocking=True)        # lands before the flush that brings this iteration's row
        self._prints.append((it, slot))

    def _sample(self, it):
        # Every rank runs the generator on the (seeded, identical) sample inputs: in train mode that moves its BatchNorm running
        # statistics, and the replicas stay bit-equal without a broadcast.  Rank 0 alone writes the grids.
        tr = self.trainer
        real, trans = {"celeba": lambda: (tr.real, tr.scaled), "mnist": lambda: (tr.real, tr.scaled),
                       "dsprites": lambda: (tr.align, tr.trans2), "colored": lambda: (tr.align, tr.trans2)}[self.kind]()
        rng = np.random.RandomState(sample_seed(self.seed, it))
        self.files += sampling.sample_image(self.plan["grid"], tr.G, n=10, batches_done=it, real=real[:100], trans=trans[:100],
                                            out_dir=self.out_dir, rng=rng, device=tr.losses.device, write=self.rank == 0)
        if self._ema_G is not None:
            # the same grids from the averaged weights: the scratch generator's own BatchNorm statistics move in train mode and are
            # overwritten by the next copy_to -- the trainer's state is not touched
            G = tr.ema.copy_to("G", self._ema_G).train(tr.G.training)
            rng = np.random.RandomState(sample_seed(self.seed, it))
            self.files += sampling.sample_image(self.plan["grid"], G, n=10, batches_done=it, real=real[:100], trans=trans[:100],
                                                out_dir=os.path.join(self.out_dir, "ema"), rng=rng, device=tr.losses.device)

    def _checkpoint(self, it):
        if self.rank != 0:
            return
        tr, od = self.trainer, self.out_dir
        names = [os.path.join(od, n) for n in checkpoint_files(self.kind, it)]
        if self.kind == "celeba":
            sampling.save_checkpoint(names[0], tr.G, tr.D, it // self.L, it)
        elif self.kind == "mnist":
            torch.save(tr.G.state_dict(), names[0])
            torch.save(tr.E.state_dict(), names[1])
        elif self.kind in ("dsprites", "colored"):
            torch.save(tr.E.state_dict(), names[0])
            torch.save(tr.G.state_dict(), names[1])
        else:
            torch.save(tr.P.state_dict(), names[0])
        self.files += names
        ema = getattr(tr, "ema", None)
        if ema is not None:
            for name, fn in zip(ema.names, ema_checkpoint_files(self.kind, it, ema.names)):
                torch.save({k: v.detach().to("cpu", copy=True) for k, v in ema.state_dict(name).items()}, os.path.join(od, fn))
                self.files.append(os.path.join(od, fn))

    def _score(self, it):
        """one line of ``swd.jsonl``: the live generator and, where the trainer averages it, the averaged one, as scratch copies"""
        if self._score_G is None or self.swd is None:
            return
        tr, plan = self.trainer, self.swd
        seed = swd_seed(self.seed, it, plan.seed)
        kw = dict(n_images=plan.n_images, batch=min(int(tr.B), int(plan.n_images)), seed=seed, patches_per_image=plan.patches_per_image,
                  repeats=plan.repeats, dirs=plan.dirs)
        self._score_line("swd.jsonl", it, lambda G: quality.swd_generator(self.kind, G, self.inputs, **kw))

    def _score_nn(self, it):
        """one line of ``nn.jsonl``: the leave-one-out 1-NN two-sample test and precision / recall / density / coverage
        of ONE set of generated images per generator against the first ``n_images`` dataset images"""
        if self._score_G is None or self.nn is None:
            return
        tr, plan = self.trainer, self.nn
        n, seed = int(plan.n_images), nn_seed(self.seed, it, plan.seed)
        real = quality.to_u8(quality.real_images(self.kind, self.inputs, n))

        def score(G):
            fake = quality.to_u8(quality.generate(self.kind, G, n, min(int(tr.B), n), seed))
            return {"two_sample": quality.nn_two_sample(real, fake), "prdc": quality.prdc(real, fake, plan.k)}
        self._score_line("nn.jsonl", it, score)

    def _score_mmd(self, it):
        """one line of ``mmd.jsonl``: ``quality.mmd`` of one set of generated images per generator against the first
        ``n_images`` dataset images"""
        if self._score_G is None or self.mmd is None:
            return
        tr, plan = self.trainer, self.mmd
        n, seed = int(plan.n_images), mmd_seed(self.seed, it, plan.seed)
        real = quality.to_u8(quality.real_images(self.kind, self.inputs, n))
        self._score_line("mmd.jsonl", it, lambda G: quality.mmd(real, quality.generate(self.kind, G, n, min(int(tr.B), n), seed), scales=plan.scales))

    def _score_sinkhorn(self, it):
        """one line of ``sinkhorn.jsonl``: ``quality.sinkhorn`` of one set of generated images per generator against the first
        ``n_images`` dataset images"""
        if self._score_G is None or self.sinkhorn is None:
            return
        tr, plan = self.trainer, self.sinkhorn
        n, seed = int(plan.n_images), sinkhorn_seed(self.seed, it, plan.seed)
        real = quality.to_u8(quality.real_images(self.kind, self.inputs, n))
        self._score_line("sinkhorn.jsonl", it, lambda G: quality.sinkhorn(real, quality.generate(self.kind, G, n, min(int(tr.B), n), seed),
                                                                          scale=plan.scale, iterations=plan.iterations))

    def _score_ndb(self, it):
        """one line of ``ndb.jsonl``: ``quality.ndb`` of one set of generated images per generator against the bins of the
        first ``n_images`` dataset images, which are fitted here once"""
        if self._score_G is None or self.ndb is None:
            return
        tr, plan = self.trainer, self.ndb
        n, seed = int(plan.n_images), ndb_seed(self.seed, it, plan.seed)
        real = quality.to_u8(quality.real_images(self.kind, self.inputs, n))
        if self.ndb_bins is None:
            self.ndb_bins = quality.image_bins(real, plan.bins, plan.iterations, plan.seed)
        fit = self.ndb_bins
        inertia, changed = int(fit.inertia[-1]), (int(fit.changed[-1]) if int(plan.iterations) else None)

        def score(G):
            out = quality.ndb(real, quality.generate(self.kind, G, n, min(int(tr.B), n), seed), centres=fit.centres)
            out["inertia"], out["changed_last"] = inertia, changed      # the line of quality.ndb(real, fake, bins, iterations, plan.seed)
            return out
        self._score_line("ndb.jsonl", it, score)

    def _score_spectrum(self, it):
        """one line of ``spectrum.jsonl``: ``quality.spectrum`` of one set of generated images per generator against the
        first ``n_images`` dataset images, whose per-ring moments are computed here once"""
        if self._score_G is None or self.spectrum is None:
            return
        tr, plan = self.trainer, self.spectrum
        n, seed = int(plan.n_images), spectrum_seed(self.seed, it, plan.seed)
        if self.spectrum_real is None:
            self.spectrum_real = quality.spectrum_moments(quality.real_images(self.kind, self.inputs, n))[0]
        H = int(self.inputs.data.shape[2])
        self._score_line("spectrum.jsonl", it, lambda G: quality.spectrum_from_moments(
            self.spectrum_real, quality.spectrum_moments(quality.generate(self.kind, G, n, min(int(tr.B), n), seed))[0], H))

    def _score_ssim(self, it):
        """one line of ``ssim.jsonl``: ``quality.diversity`` of one set of generated images per generator, beside that of the
        first ``n_images`` dataset images, which is computed here once; one pair table for all"""
        if self._score_G is None or self.ssim is None:
            return
        tr, plan = self.trainer, self.ssim
        n, seed = int(plan.n_images), ssim_seed(self.seed, it, plan.seed)
        if self.ssim_real is None:
            real = quality.real_images(self.kind, self.inputs, n)
            self._ssim_pairs = quality.pair_table(n, int(plan.n_pairs), plan.seed, real.device)
            self.ssim_real = quality.diversity(real, pairs=self._ssim_pairs)

        def score(G):
            out = quality.diversity(quality.generate(self.kind, G, n, min(int(tr.B), n), seed), pairs=self._ssim_pairs)
            out["real"] = dict(self.ssim_real)
            out["gap"] = out["ms_ssim"] - self.ssim_real["ms_ssim"]
            return out
        self._score_line("ssim.jsonl", it, score)

    def _score_line(self, name, it, score):
        """``{"batches_done", "G": score(live generator)[, "G_ema": score(averaged generator)]}`` appended to ``out_dir/name``"""
        tr, G = self.trainer, self._score_G
        G.load_state_dict(tr.G.state_dict())
        line = {"batches_done": int(it), "G": score(G.train(tr.G.training))}
        ema = getattr(tr, "ema", None)
        if ema is not None and "G" in ema.names:
            line["G_ema"] = score(ema.copy_to("G", G).train(tr.G.training))
        path = os.path.join(self.out_dir, name)
        with open(path, "a") as f:
            f.write(json.dumps(line, sort_keys=True) + "\n")
        if path not in self.files:
            self.files.append(path)

    def _prepare(self):
        tr = self.trainer
        tr.inputs, tr.log = self.inputs, (self.log if self.log_in_graph else None)
        if self.graph and tr.graph is None:
            # capture(warmup=True) is a real training step on the current slots: run it on a saved state and put that state back
            sd = tr.state_dict()
            self.inputs.enqueue(tr)                      # a real batch in the slots for the warm-up iteration
            tr.capture(warmup=True, inputs=self.inputs, log=tr.log)
            tr.load_state_dict(sd)
        # the log numbers its rows like the run numbers its iterations
        if len(self.history) < self.batches_done:
            self.history = np.concatenate((self.history, np.zeros((self.batches_done - len(self.history), self.log.n), np.float32)), 0)
        self.log.load(self.batches_done, int(self.log.first_nonfinite.item()))
        self._enqueued = self.batches_done
        self._prepared = True

    # -- public ---------------------------------------------------------------------------------------
    def run(self, max_iters=None):
        if not self._prepared or self._enqueued != self.batches_done or len(self.history) > self.batches_done:
            self.history = self.history[:self.batches_done]
            self._prepare()
        tr, log = self.trainer, self.log
        total = self.n_epochs * self.L
        done = 0
        while self.batches_done < total and (max_iters is None or done < max_iters):
            it = self.batches_done
            if self._enqueued - len(self.history) >= log.capacity:       # the next append would overwrite a row not yet taken
                self._wait("ring-full")
            tr.step_resident()
            if not self.log_in_graph:
                log.append()
            self._enqueued += 1
            do_print, do_sample, do_ckpt = cadence(self.kind, it, self.sample_interval)
            if do_print:
                self._queue_print(it)
            if log.landed() and (do_print or self._enqueued - log.mirror_head >= log.capacity // 2):
                log.flush_async()
            self._collect()
            if do_sample:
                self._wait("sample")
                self._sample(it)
            if do_ckpt:
                self._wait("checkpoint")
                self._checkpoint(it)
                self._score(it)
                self._score_nn(it)
                self._score_mmd(it)
                self._score_sinkhorn(it)
                self._score_ndb(it)
                self._score_spectrum(it)
                self._score_ssim(it)
            self.batches_done = it + 1
            done += 1
            if do_ckpt:
                self._write_state()
        self._wait("end")
        self.save()
        return self

    def _write_state(self):
        if self.rank != 0:                                          # the replicas are identical: every rank resumes from rank 0's file
            return None
        sd = self.trainer.state_dict()
        sd["run.kind"] = self.kind
        sd["run.world"] = int(self.world)
        sd["run.batches_done"] = int(self.batches_done)
        sd["run.losses"] = torch.from_numpy(self.history[:self.batches_done].copy())
        path = os.path.join(self.out_dir, f"run_state_{self.batches_done}.pt")
        torch.save(sd, path)
        np.save(os.path.join(self.out_dir, "losses.npy"), self.history[:self.batches_done])
        self.files.append(path)
        return path

    def save(self):
        """``out_dir/run_state_<batches_done>.pt``: the trainer's full state, ``batches_done`` and the loss rows so far; and
        ``out_dir/losses.npy``.  Rank 0 only: the other ranks of a data-parallel run write nothing and return None."""
        if len(self.history) < self.batches_done:
            self._wait("end")
        return self._write_state()

    @classmethod
    def resume(cls, path, kind, trainer, inputs, out_dir, n_epochs, **kw):
        """continue the run saved in ``path`` on a (fresh or used) trainer of the same kind with a sampler of the same seed.  Data
        parallel: every rank loads rank 0's file (the replicas are identical; without SyncBN each rank takes rank 0's BatchNorm running
        statistics, as DDP broadcasts buffers); the loss rows of the iterations before the file are rank 0's on every rank."""
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if sd.get("run.kind") != kind:
            raise ValueError(f"run.kind: {sd.get('run.kind')!r} in the file, {kind!r} asked for")
        file_world, have_world = int(sd.get("run.world", 1)), int(getattr(inputs, "world", 1))
        if file_world != have_world:
            raise ValueError(f"run.world: {file_world} in the file, {have_world} in the attached sampler")
        run = cls(kind, trainer, inputs, out_dir, n_epochs, **kw)
        trainer.load_state_dict(sd)
        run.batches_done = int(sd["run.batches_done"])
        run.history = sd["run.losses"].numpy().astype(np.float32).reshape(-1, run.log.n)
        return run

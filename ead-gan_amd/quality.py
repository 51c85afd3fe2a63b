"""Image quality of a generator as a number: the sliced Wasserstein distance of Karras et al., "Progressive Growing of GANs"
(2018), between real and generated images -- the distribution of local 7 x 7 patches of a Laplacian pyramid, compared at every scale from
full resolution down to 16 px.  It needs no pretrained network (FID and its relatives need Inception weights) and is deterministic once
the random draws are fixed.  Not in the reference, whose scripts only write sample grids.

* ``laplacian_pyramid(images)``                  the levels H, H/2 ... 16 (ops.pyr_down / ops.pyr_up_sub)
* ``swd(real, fake, ...)``                       per-level distances and their mean, times 1e3 as the paper reports them
* ``draw_plan(seed, shape, ...)``                the patch centres and unit directions ``swd`` draws for that seed
* ``generate`` / ``real_images``                 the two image sets of an MNIST or CelebA run
* ``swd_generator(kind, generator, inputs)``     the three together
* ``SWDPlan``                                    what ``train.TrainRun(..., swd=...)`` scores on checkpoint iterations

Memorisation: SWD cannot see a generator that copies training images -- it scores perfectly.  The exact nearest-neighbour search
over the uint8 datasets (ops.knn_u8: integer squared L2 distances on the int8 MFMA, ties to the lower index) answers that twice:

* ``to_u8(images)``                              [-1, 1] fp32 -> the dataset's bytes (the inverse of the trainers' 2/255 u - 1)
* ``nearest_neighbours(images, database, k)``    distances and indices of the k nearest dataset images
* ``nn_two_sample(real, fake)``                  the leave-one-out 1-NN two-sample test (Lopez-Paz & Oquab 2017; Xu et al. 2018)
* ``neighbour_grid`` / ``save_neighbours``       the figure: every query beside its nearest dataset images
* ``nearest_training_images`` / ``nn_generator`` the two for a generator of an MNIST or CelebA run

Fidelity and diversity apart: the k-NN-ball scores over the same exact distances (ops.ball_count_u8 counts, per row, the closed
balls of the other set that contain it):

* ``knn_radii(images, k)``                       the distance from every image to its k-th nearest other image of the set
* ``prdc(real, fake, k)``                        precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020)
* ``prdc_generator(kind, generator, inputs)``    the same for a generator of an MNIST or CelebA run
* ``NNPlan``                                     what ``train.TrainRun(..., nn=...)`` scores on checkpoint iterations

A distance between the two distributions: the kernel maximum mean discrepancy (Gretton et al. 2012), the second score Xu et
al. (2018) found to behave well, with k(a, b) = exp(-d(a, b) / gamma) over the same exact distances and gamma a multiple of their exact
median (ops.dist_select_u8: a radix select over histogram passes of the search's tile loop; ops.kernel_sum_u8: the row sums in double):

* ``median_distance(images)``                    the lower median distance between different images of a set, an integer
* ``mmd(real, fake, scales)``                    the unbiased and the biased MMD^2 per bandwidth and the mean over the bandwidths
* ``mmd_sums(real, fake, inv_gamma)``            the three kernel sums behind them, on the device
* ``mmd_witness(real, fake, queries, gamma)``    the witness function: which images are over- or under-represented
* ``mmd_generator(kind, generator, inputs)``     ``mmd`` for a generator of an MNIST or CelebA run
* ``MMDPlan``                                    what ``train.TrainRun(..., mmd=...)`` scores on checkpoint iterations

A transport cost between the two image sets themselves: the debiased Sinkhorn divergence (Genevay et al. 2018; Feydy et al.
2019) over the same exact distances, its temperature a multiple of their exact median (ops.softmin_u8: a streaming log-sum-exp over the
search's tile loop, one call per half-iteration; the distance matrix is never stored):

* ``sinkhorn(real, fake, scale)``                the divergence, its three transport terms and the marginal error left by the fixed loop;
                                                 with ``terms=True`` the per-image shares as well
* ``sinkhorn_generator(kind, generator, inputs)`` the same for a generator of an MNIST or CelebA run
* ``SinkhornPlan``                               what ``train.TrainRun(..., sinkhorn=...)`` scores on checkpoint iterations

Which modes of the data the generator drops or over-produces: the Number of statistically Different Bins of Richardson &
Weiss, "On GANs and GMMs" (2018).  The real images are cut into Voronoi cells by k-means over their bytes (ops.kmeans_u8: centres are
bytes, i.e. images; k-means++ seeding and the centre update are streaming passes on the device, the assignment is ops.knn_u8), real and
generated images are counted per cell and every cell takes a two-proportion z-test:

* ``image_bins(images, bins)``                   the fitted cells: ``Bins(centres, counts, labels, inertia, changed)``
* ``bin_counts(images, centres)``                how many images fall into every cell
* ``ndb(real, fake, bins)``                      the number of cells whose share differs at the 5 % level, the Jensen-Shannon divergence of
                                                 the two histograms; with ``terms=True`` the per-cell z, real and generated counts as well
* ``bin_grid`` / ``save_bins``                   the figure: the cell centres ordered by z, most under-produced first
* ``ndb_generator(kind, generator, inputs)``     ``ndb`` for a generator of an MNIST or CelebA run
* ``NDBPlan``                                    what ``train.TrainRun(..., ndb=...)`` scores on checkpoint iterations

Bins fitted on ``real`` itself are biased towards ``real`` (the cells are where its rows are dense): two samples of one distribution do
NOT give 0.05 x bins.  In a numpy trial of this contract two samples of one 30-mode mixture (4000 rows, 50 bins) gave NDB 2 .. 8 against
the nominal 2.5, so read a number against the NDB of a held-out real split, or fit the bins elsewhere (``centres=``).

What up-convolutions do to the high frequencies: the azimuthally averaged power spectrum of Durall et al., "Watch your
Up-Convolution" (2020).  Every score above but the SWD rests on the L2 distance between the bytes, which the low frequencies dominate;
this one reads the other end.  P = |DFT of the bytes|^2 / H^2 per image (ops.spectrum_u8: a direct fp64 matrix DFT, one workgroup per
image), averaged over integer rings of the frequency plane, in dB, real against generated:

* ``radial_bins(H)``                             the integer ring tables, numpy arrays on the host
* ``power_profile(images)``                      float64 [N, B] on the device: every image's ring means
* ``mean_spectrum(images)``                      float64 [H, H] on the device: the set's mean 2-D spectrum in dB, zero frequency at the centre
* ``spectrum(real, fake)``                       per ring the two mean log-profiles, their gap and effect size; the rms gap, the mean gap
                                                 of the high rings, the ring of the largest gap
* ``spectrum_grid`` / ``save_spectra``           the figure: the two mean spectra side by side (checkerboard peaks are dots on the axes
                                                 and in the corners)
* ``spectrum_generator(kind, generator, inputs)`` ``spectrum`` for a generator of an MNIST or CelebA run
* ``SpectrumPlan``                               what ``train.TrainRun(..., spectrum=...)`` scores on checkpoint iterations

Image against image: every score above is a statement about two SETS.  Two daily questions are about PAIRS: how good is a
reconstruction (PSNR and SSIM of an output against its target: ``sampling.project_images`` reports only its own loss), and has the
generator collapsed (the mean MS-SSIM over random pairs of generated images beside the same figure for real images, Odena et al. 2017: a
value close to 1, or well above the real images', means mode collapse; per class for the class-conditional generators, where collapse
inside one class hides in every set-level score).  Both rest on ops.ssim_u8: the windowed five-moment filter of Wang et al. (2004) over the
levels of a 2 x 2 mean pyramid, in float64, one workgroup per pair, thousands of pairs per launch:

* ``pair_table(n, n_pairs, seed)``               int32 [n_pairs, 2] on the device: ordered pairs of different rows of one set
* ``ssim`` / ``ms_ssim`` / ``psnr(a, b, pairs)``   float64 [P] on the device, no host read
* ``reconstruction(target, output)``             PSNR, mean squared error, mean SSIM and MS-SSIM of a set of outputs against their targets
* ``projection_quality(kind, generator, ...)``   ``reconstruction`` of what ``sampling.project_images`` found
* ``diversity(images, n_pairs, seed, labels)``   mean MS-SSIM and SSIM over random pairs, the number of identical pairs; per class with labels
* ``diversity_generator(kind, generator, inputs)`` ``diversity`` of real and generated images of an MNIST or CelebA run over ONE pair table
* ``SSIMPlan``                                   what ``train.TrainRun(..., ssim=...)`` scores on checkpoint iterations

With the 11-tap window a level needs a side of 11 px, so MNIST's 32 px give L = 2 levels and CelebA's 64 px L = 3, weighted by the first L
of Wang's five weights divided by their sum.  The numbers are therefore comparable within a workload, not across workloads or with papers
that use 5 levels on larger images.

Per level and set: patch statistics (ops.swd_patch_stats), then per repeat one fused gather-and-project launch (ops.swd_project: the
descriptors, 0.6 GB per set and level at full size, never exist), one column sort per set (ops.sort_columns) and one reduction
(ops.l1_mean).  Everything is enqueued on the current stream; ``swd`` reads the device once, at its end.  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import ops, sampling

PATCH, MIN_SIDE = 7, 16
# Philox stream ids of this module's draws (ops.rng_fill): a block no sampler uses (the samplers' ids are 1 .. 8).  The device counter of
# a draw holds the level (centres), level * repeats + repeat (directions) or the batch index (generator inputs).
SID_POSITIONS, SID_DIRECTIONS, SID_NOISE, SID_LABELS, SID_CODE = 0x5D00, 0x5D01, 0x5D10, 0x5D11, 0x5D12
SID_BINS = 0x5D20                # the k-means seeding's uniforms (image_bins); the device counter holds 0
SID_PAIRS = 0x5D30               # the pair tables (pair_table, class_pair_table); the device counter holds 0 for the first row of a pair, 1 for the second
# how the trainers see a dataset image: eg_gather_u8_images' scale and shift (celebA/EAD-GAN_celebA.py:194-201, MNIST/EAD-GAN_rpqmnxy.py:235-243)
_REAL_SCALE = {"mnist": (2.0 / 255.0, -1.0), "celeba": (2.0 / 255.0, -1.0)}
_SPRITES = ("dsprites", "colored", "pxy")


class SWDPlan(NamedTuple):
    """what a training run scores on its checkpoint iterations: ``n_images`` generated against the first ``n_images`` dataset images"""
    n_images: int
    seed: int = 0
    patches_per_image: int = 128
    repeats: int = 4
    dirs: int = 128


class NNPlan(NamedTuple):
    """the nearest-neighbour scores a training run writes on its checkpoint iterations (``nn_two_sample`` and ``prdc`` at ``k``):
    ``n_images`` generated against the first ``n_images`` dataset images"""
    n_images: int
    k: int = 5
    seed: int = 0


class MMDPlan(NamedTuple):
    """the kernel MMD a training run writes on its checkpoint iterations (``mmd`` at ``scales`` times the median bandwidth): ``n_images``
    generated against the first ``n_images`` dataset images"""
    n_images: int
    scales: tuple = (0.5, 1.0, 2.0)
    seed: int = 0


class SinkhornPlan(NamedTuple):
    """the Sinkhorn divergence a training run writes on its checkpoint iterations (``sinkhorn`` at ``scale`` times the median distance,
    ``iterations`` updates): ``n_images`` generated against the first ``n_images`` dataset images"""
    n_images: int
    scale: float = 0.1
    iterations: int = 60
    seed: int = 0


class NDBPlan(NamedTuple):
    """the NDB score a training run writes on its checkpoint iterations (``ndb`` over ``bins`` k-means cells of the real images, fitted
    once with ``iterations`` Lloyd iterations): ``n_images`` generated against the first ``n_images`` dataset images"""
    n_images: int
    bins: int = 100
    iterations: int = 20
    seed: int = 0


class SpectrumPlan(NamedTuple):
    """the radial power-spectrum score a training run writes on its checkpoint iterations (``spectrum``): ``n_images`` generated against
    the first ``n_images`` dataset images"""
    n_images: int
    seed: int = 0


class SSIMPlan(NamedTuple):
    """the pair diversity a training run writes on its checkpoint iterations (``diversity``): the mean MS-SSIM over ``n_pairs`` random
    pairs of ``n_images`` generated images beside that of the first ``n_images`` dataset images, one pair table (from ``seed``) for all"""
    n_images: int
    n_pairs: int = 4096
    seed: int = 0


class Bins(NamedTuple):
    """k-means cells of an image set (``image_bins``), on the device: ``centres`` uint8 [bins, C, H, W]; ``counts`` int32 [bins] and
    ``labels`` int32 [N] of the fitted images; ``inertia`` int64 [iterations + 1]; ``changed`` int32 [iterations]"""
    centres: torch.Tensor
    counts: torch.Tensor
    labels: torch.Tensor
    inertia: torch.Tensor
    changed: torch.Tensor


def level_sides(H):
    """sides of the pyramid levels of an H x H image, finest first: H, H/2 ... 16"""
    H = int(H)
    if H < MIN_SIDE or H & (H - 1):
        raise ValueError(f"swd: the image side must be a power of two >= {MIN_SIDE}, got {H}")
    sides = []
    while H >= MIN_SIDE:
        sides.append(H)
        H //= 2
    return sides


def _images(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"quality: {name} must be a tensor on the GPU (there is no CPU fallback)")
    if t.dim() != 4 or t.shape[1] not in (1, 3) or t.shape[2] != t.shape[3]:
        raise ValueError(f"quality: {name} must be [N, C, H, H] with C = 1 or 3, got {tuple(t.shape)}")
    level_sides(t.shape[2])
    return t.detach().float().contiguous()


def laplacian_pyramid(images):
    """[N, C, H, H] on the device -> the Laplacian levels H, H/2 ... 16 as new fp32 tensors, finest first; the coarsest stays Gaussian"""
    x = _images(images, "images")
    N, C, H, _ = x.shape
    pyr = [x.clone()]
    for side in level_sides(H)[1:]:
        coarse = torch.empty(N, C, side, side, device=x.device, dtype=torch.float32)
        ops.pyr_down(pyr[-1], coarse, N * C, 2 * side)
        ops.pyr_up_sub(pyr[-1], coarse, N * C, 2 * side)
        pyr.append(coarse)
    return pyr


def draw_plan(seed, shape, patches_per_image=128, repeats=4, dirs=128, device="cuda"):
    """-> (positions, directions) exactly as ``swd(..., seed=seed)`` draws them for image sets of ``shape`` = (N, C, H, H):
    positions[l]: int32 [N * P, 2] = (y, x) patch centres of level l, uniform in [3, H_l - 3); directions[l][r]: fp32 [49 C, dirs] with
    unit columns.  Feed them back through ``swd(positions=..., directions=...)`` or to any other implementation."""
    N, C, H, W = (int(v) for v in shape)
    P, R, D = int(patches_per_image), int(repeats), int(dirs)
    if C not in (1, 3) or H != W or N < 1 or P < 1 or R < 1 or not 1 <= D <= 128:
        raise ValueError("draw_plan: shape (N, C, H, H) with C = 1 or 3; patches_per_image, repeats >= 1; 1 <= dirs <= 128")
    dev = torch.device(device)
    step = torch.zeros(1, device=dev, dtype=torch.int32)
    positions, directions = [], []
    for l, side in enumerate(level_sides(H)):
        draw = torch.empty(N * P, 2, device=dev, dtype=torch.int64)
        step.fill_(l)
        ops.rng_fill(ops.RNG_RANDINT, draw, 3, side - 3, seed, step, SID_POSITIONS)
        positions.append(draw.to(torch.int32))
        level = []
        for r in range(R):
            W_ = torch.empty(PATCH * PATCH * C, D, device=dev, dtype=torch.float32)
            step.fill_(l * R + r)
            ops.rng_fill(ops.RNG_NORMAL, W_, 0.0, 1.0, seed, step, SID_DIRECTIONS)
            ops.swd_unit_columns(W_, W_.shape[0], D)
            level.append(W_)
        directions.append(level)
    return positions, directions


def _check_plan(positions, directions, N, C, sides, dev):
    if len(positions) != len(sides) or len(directions) != len(sides):
        raise ValueError(f"swd: positions and directions need one entry per level {sides}")
    n_desc = int(positions[0].shape[0])
    if n_desc < N or n_desc % N:
        raise ValueError(f"swd: positions[l] must be [N * P, 2]: {n_desc} rows for N = {N} images")
    R, D = len(directions[0]), int(directions[0][0].shape[1])
    for pos, level in zip(positions, directions):
        if not (pos.is_cuda and pos.dtype == torch.int32 and tuple(pos.shape) == (n_desc, 2) and pos.is_contiguous()):
            raise ValueError("swd: every positions[l] must be a contiguous int32 device tensor [N * P, 2]")
        if len(level) != R or R < 1:
            raise ValueError("swd: every level needs the same number (>= 1) of direction matrices")
        for W in level:
            if not (W.is_cuda and W.dtype == torch.float32 and tuple(W.shape) == (PATCH * PATCH * C, D) and W.is_contiguous() and 1 <= D <= 128):
                raise ValueError(f"swd: every direction matrix must be a contiguous fp32 device tensor [{PATCH * PATCH * C}, D <= 128]")
    return n_desc, n_desc // N, R, D


_FLAG_TEXT = ((ops.SWD_FLAG_ZERO_STD, "a channel without variance"), (ops.SWD_FLAG_NONFINITE, "a NaN or an infinity among the patch pixels"),
              (ops.SWD_FLAG_POSITION, "a patch centre outside [3, H - 3)"))


def swd(real, fake, patches_per_image=128, repeats=4, dirs=128, seed=0, positions=None, directions=None):
    """Sliced Wasserstein distance between two image sets [N, C, H, H] (C = 1 or 3, H a power of two >= 16) on the device
    -> {"levels": {H: v, H/2: v, ... 16: v}, "mean": v}, Python floats times 1e3.  ``positions`` / ``directions``: explicit draws in
    ``draw_plan``'s form (both or neither; the counts then come from their shapes); otherwise drawn from ``seed``.  The same positions
    serve both sets; each set is normalised per level and channel by its own statistics, so the result does not change under a
    per-channel rescale a x + b (a > 0) of either set.  A channel with zero variance at some level (or a non-finite pixel) raises
    ValueError.  One host read, at the end."""
    A, B = _images(real, "real"), _images(fake, "fake")
    if A.shape != B.shape or A.device != B.device:
        raise ValueError(f"swd: the two sets must have one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    N, C, H, _ = A.shape
    sides = level_sides(H)
    dev = A.device
    if (positions is None) != (directions is None):
        raise ValueError("swd: pass positions and directions together (draw_plan returns both)")
    if positions is None:
        positions, directions = draw_plan(seed, A.shape, patches_per_image, repeats, dirs, dev)
    n_desc, P, R, D = _check_plan(positions, directions, N, C, sides, dev)
    ld = ops.round_up(n_desc, 4)
    proj = torch.empty(2, D, ld, device=dev, dtype=torch.float32)
    stats = torch.empty(2, C, 2, device=dev, dtype=torch.float64)
    stats_ws = torch.empty(ops.swd_patch_stats_ws_doubles(C), device=dev, dtype=torch.float64)
    proj_ws = torch.empty(ops.swd_project_ws_floats(C), device=dev, dtype=torch.float32)
    l1_ws = torch.empty(ops.l1_mean_ws_doubles(), device=dev, dtype=torch.float64)
    flags = torch.zeros(2, len(sides), device=dev, dtype=torch.int32)
    dist = torch.zeros(len(sides), R, device=dev, dtype=torch.float64)
    pyrs = (laplacian_pyramid(A), laplacian_pyramid(B))
    for l, side in enumerate(sides):
        for s in range(2):
            ops.swd_patch_stats(pyrs[s][l], positions[l], n_desc, P, C, side, stats_ws, stats[s], flags[s, l:l + 1])
        for r in range(R):
            for s in range(2):
                ops.swd_project(pyrs[s][l], positions[l], n_desc, P, C, side, directions[l][r], D, stats[s], proj_ws, proj[s], ld)
                ops.sort_columns(proj[s], n_desc)
            ops.l1_mean(proj[0], proj[1], n_desc, D, ld, l1_ws, dist[l, r:r + 1])
    host = torch.cat((dist.reshape(-1), flags.reshape(-1).double())).cpu()          # THE host read
    got, bad = host[:len(sides) * R].reshape(len(sides), R), host[len(sides) * R:].to(torch.int64).reshape(2, len(sides))
    for s, name in enumerate(("real", "fake")):
        for l, side in enumerate(sides):
            why = [text for bit, text in _FLAG_TEXT if int(bad[s, l]) & bit]
            if why:
                raise ValueError(f"swd: the {name} set at level {side}: {'; '.join(why)}")
    levels = {side: 1e3 * float(got[l].mean()) for l, side in enumerate(sides)}
    return {"levels": levels, "mean": sum(levels.values()) / len(levels)}


def _family(kind, what):
    family = str(kind).split("_")[0]
    if family in _SPRITES:
        raise ValueError(f"quality.{what}: the sprite workloads ({kind!r}) are not scored this way -- their `real' distribution is the aligned "
                         "and warped image and they have disentanglement scores (score.py); quality.swd itself accepts their 64 px images")
    if family not in _REAL_SCALE:
        raise ValueError(f"quality.{what}: kind must be of the 'mnist' or 'celeba' family, got {kind!r}")
    return family


def generate(kind, generator, n_images, batch, seed=0):
    """``n_images`` outputs [n_images, C, H, H] of a generator of the 'mnist' or 'celeba' family in its current mode, in batches of ``batch``:
    z ~ N(0, 1), uniform class labels and code ~ U(-1, 1) as the training scripts draw them, on the device, keyed by ``seed``.
    ``n_images % batch != 0`` raises: in train mode BatchNorm makes the composition of a batch part of the result.  The generator's
    state is left as it was (train-mode BatchNorm moves the running statistics; they are put back)."""
    _family(kind, "generate")
    n_images, batch = int(n_images), int(batch)
    if batch < 1 or n_images < 1 or n_images % batch:
        raise ValueError(f"quality.generate: n_images = {n_images} is no positive multiple of batch = {batch}")
    dev = next(generator.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("quality.generate: the generator must be on the GPU (there is no CPU fallback)")
    ncls = int(generator.n_classes)
    z = torch.empty(batch, int(generator.latent_dim), device=dev, dtype=torch.float32)
    code = torch.empty(batch, int(generator.code_dim), device=dev, dtype=torch.float32)
    lab = torch.empty(batch, device=dev, dtype=torch.int64)
    onehot = torch.empty(batch, ncls, device=dev, dtype=torch.float32)
    out = torch.empty(n_images, int(generator.channels), int(generator.img_size), int(generator.img_size), device=dev, dtype=torch.float32)
    step = torch.zeros(1, device=dev, dtype=torch.int32)
    keep = {name: b.detach().clone() for name, b in generator.named_buffers()}
    with torch.no_grad():
        for i in range(n_images // batch):
            step.fill_(i)
            ops.rng_fill_multi([(ops.RNG_NORMAL, z, 0.0, 1.0, SID_NOISE), (ops.RNG_RANDINT, lab, 0, ncls, SID_LABELS, onehot),
                                (ops.RNG_UNIFORM, code, -1.0, 1.0, SID_CODE)], seed, step)
            out[i * batch:(i + 1) * batch].copy_(generator(z, onehot, code))
        for name, b in generator.named_buffers():
            b.copy_(keep[name])
    return out


def real_images(kind, inputs, n_images):
    """the first ``n_images`` dataset images as the trainer sees them (scaled to [-1, 1], no flip): ``inputs`` is the run's sampler or its
    uint8 device dataset [N, C, H, H]"""
    scale, shift = _REAL_SCALE[_family(kind, "real_images")]
    data = getattr(inputs, "data", inputs)
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.uint8 and data.dim() == 4):
        raise ValueError("quality.real_images: inputs must be a sampler or a uint8 device dataset [N, C, H, W]")
    n = int(n_images)
    if not 1 <= n <= data.shape[0]:
        raise ValueError(f"quality.real_images: n_images = {n}, the dataset has {data.shape[0]} images")
    _, C, H, W = data.shape
    idx = torch.arange(n, device=data.device, dtype=torch.int64)
    out = torch.empty(n, C, H, W, device=data.device, dtype=torch.float32)
    ops.gather_u8_images(data.contiguous(), idx, None, out, n, C, H, W, scale, shift)
    return out


def swd_generator(kind, generator, inputs, n_images=8192, batch=None, seed=0, **swd_kw):
    """SWD of ``generate(kind, generator, n_images, batch, seed)`` against ``real_images(kind, inputs, n_images)``; ``batch`` defaults to
    64 (the scripts' batch size) or ``n_images`` if that is smaller; ``swd_kw``: patches_per_image, repeats, dirs"""
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    return swd(real_images(kind, inputs, n_images), fake, seed=seed, **swd_kw)


# ---- nearest neighbours over the uint8 datasets -----------------------------------------------------------------------------
def to_u8(images):
    """fp32 [N, C, H, W] in [-1, 1] on the device -> uint8 [N, C, H, W]: the inverse of the trainers' 2/255 u - 1.  The byte is
    eg_quantize_u8 of v' = 0.5 v + 0.5 (clamp(v' * 255 + 0.5, 0, 255) truncated), every step a separately rounded fp32 operation, so
    ``to_u8(real_images(...))`` gives back the dataset's bytes for all 256 values; values outside [-1, 1] clamp."""
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.is_floating_point() and images.dim() == 4):
        raise ValueError("quality.to_u8: images must be a floating-point device tensor [N, C, H, W]")
    v = images.detach().float().mul(0.5).add_(0.5).contiguous()              # two roundings, as stated
    out = torch.empty(v.shape, device=v.device, dtype=torch.uint8)
    per = v[0].numel()
    step = max(1, (2 ** 31 - 1) // per)                                      # the kernel's extents are ints
    for i in range(0, v.shape[0], step):
        part = v[i:i + step]
        ops.quantize_u8(part, 1, 1, part.numel(), None, out[i:i + step])     # C = H = 1: the flat order
    return out


def _u8_rows(t, name):
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.is_floating_point():
        return to_u8(t)
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.dtype == torch.uint8:
        return t.contiguous()
    raise ValueError(f"quality: {name} must be a float or uint8 device tensor [N, C, H, W]")


def _dataset(inputs, what):
    data = getattr(inputs, "data", inputs)
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.uint8 and data.dim() == 4):
        raise ValueError(f"quality.{what}: the database must be a sampler or a uint8 device dataset [N, C, H, W]")
    return data.contiguous()


def nearest_neighbours(images, database, k=8):
    """-> (dist, idx), int32 [N, k] on the device: the ``k`` nearest images of ``database`` (a sampler or its uint8 device dataset) to
    every image of ``images`` (float in [-1, 1], turned into bytes by ``to_u8``, or uint8), by exact squared L2 distance between the
    bytes, nearest first; equal distances go to the lower index."""
    data = _dataset(database, "nearest_neighbours")
    q = _u8_rows(images, "images")
    if q.shape[1:] != data.shape[1:]:
        raise ValueError(f"quality.nearest_neighbours: images {tuple(q.shape[1:])} against a dataset of {tuple(data.shape[1:])}")
    return ops.knn_u8(q, data, k)


def nn_two_sample(real, fake):
    """Leave-one-out 1-NN two-sample test between two image sets [N, C, H, W] (float in [-1, 1] or uint8):
    -> {"accuracy", "real", "fake"}, Python floats.  The sets are pooled, real rows first, and every row takes its nearest OTHER row
    (one ops.knn_u8 call with self0 = 0).  ``real`` = the share of real rows whose neighbour is real, ``fake`` = the share of fake rows
    whose neighbour is fake, each exactly count / N; ``accuracy`` = their mean.  0.5 says the sets cannot be told apart, 1 that they are
    trivially separable; ``fake`` well under 0.5 says the generated images sit on top of real ones (memorisation).  Tie rule: of equally
    distant rows the lower index in the pool wins, so a real row wins a tie against a fake one.  One host read, at the end."""
    A, B = _u8_rows(real, "real"), _u8_rows(fake, "fake")
    if A.shape != B.shape or A.device != B.device:
        raise ValueError(f"nn_two_sample: the two sets must have one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    N = int(A.shape[0])
    pool = torch.cat((A, B))
    _, idx = ops.knn_u8(pool, pool, 1, self0=0)
    is_real = idx[:, 0] < N
    counts = torch.stack((is_real[:N].sum(), (~is_real[N:]).sum())).cpu()     # THE host read
    r, f = int(counts[0]) / N, int(counts[1]) / N
    return {"accuracy": 0.5 * (r + f), "real": r, "fake": f}


def neighbour_grid(queries, database, idx):
    """-> fp32 [nq (1 + k), C, H, W] in [0, 1] on the device: row r of the figure is query r followed by the ``k`` dataset images
    ``idx[r]`` (``nearest_neighbours``' second result)"""
    data = _dataset(database, "neighbour_grid")
    q = _u8_rows(queries, "queries")
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dim() == 2 and idx.shape[0] == q.shape[0] and q.shape[1:] == data.shape[1:]):
        raise ValueError("quality.neighbour_grid: idx must be a device tensor [nq, k] for queries [nq, C, H, W] shaped like the dataset")
    nq, k = idx.shape
    rows = torch.cat((q.unsqueeze(1), data[idx.long().reshape(-1)].reshape(nq, k, *data.shape[1:])), 1)
    # u / 255 correctly rounded, from a table: a device division by a scalar multiplies by the rounded reciprocal and differs in the last bit
    table = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(data.device)
    return table[rows.reshape(nq * (1 + k), *data.shape[1:]).long()]


def save_neighbours(fp, queries, database, idx):
    """writes ``neighbour_grid`` as a PNG with one query and its neighbours per row"""
    sampling.save_image(neighbour_grid(queries, database, idx), fp, nrow=1 + int(idx.shape[1]))


def nearest_training_images(kind, generator, inputs, n_images=64, k=8, batch=None, seed=0, out=None):
    """``n_images`` outputs of a generator of the 'mnist' or 'celeba' family (``generate``) against the WHOLE dataset of ``inputs``
    -> (dist, idx) as ``nearest_neighbours`` returns them; ``out``: a path for the figure (``save_neighbours``)"""
    _family(kind, "nearest_training_images")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = to_u8(generate(kind, generator, n_images, batch, seed))
    dist, idx = nearest_neighbours(fake, inputs, k)
    if out is not None:
        save_neighbours(out, fake, inputs, idx)
    return dist, idx


def nn_generator(kind, generator, inputs, n_images=8192, batch=None, seed=0):
    """``nn_two_sample`` of ``real_images(kind, inputs, n_images)`` against ``generate(kind, generator, n_images, batch, seed)``;
    ``batch`` as in ``swd_generator``"""
    _family(kind, "nn_generator")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    return nn_two_sample(real_images(kind, inputs, n_images), fake)


# ---- precision, recall, density and coverage -------------------------------------------------------------------------------
def _check_k(k, what, *sizes):
    k, top = int(k), min(16, *(int(s) - 1 for s in sizes))
    if not 1 <= k <= top:
        raise ValueError(f"quality.{what}: k = {k} must be in 1 .. min(16, rows - 1) = {top} (sets of {', '.join(str(int(s)) for s in sizes)} rows)")
    return k


def knn_radii(images, k=5):
    """-> int32 [N] on the device: the exact squared L2 distance from every image (float in [-1, 1] through ``to_u8``, or uint8) to its
    ``k``-th nearest OTHER image of the set -- ``knn_u8(S, S, k, self0=0)[0][:, k - 1]``, the radius of its k-NN ball"""
    rows = _u8_rows(images, "images")
    k = _check_k(k, "knn_radii", rows.shape[0])
    return ops.knn_u8(rows, rows, k, self0=0)[0][:, k - 1].contiguous()


def prdc(real, fake, k=5):
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) between ``real`` [N, C, H, W]
    and ``fake`` [M, C, H, W] (float in [-1, 1] or uint8; N != M is allowed) over the exact integer distances d between their bytes
    -> {"precision", "recall", "density", "coverage"}, Python floats, each exactly count / denominator.  With rad_k(S)[j] = the distance
    from S[j] to its k-th nearest other row of S (``knn_radii``):

        precision = #{ i : fake[i] lies in the ball of some real row } / M
        density   = sum_i #{ j : fake[i] lies in the ball of real[j] } / (k M)               (can exceed 1)
        recall    = #{ j : real[j] lies in the ball of some fake row } / N
        coverage  = #{ j : the nearest fake row of real[j] lies in the ball of real[j] } / N

    The balls are CLOSED, as in both papers: a lies in the ball of S[j] iff d(a, S[j]) <= rad_k(S)[j].  (Naeem et al.'s published code
    compares with <; on continuous features the two agree, on integer distances they do not.)  Five device calls -- two radii searches,
    two ball counts (ops.ball_count_u8) and one ``knn_u8(real, fake, 1)`` -- and one host read, of the four integer sums."""
    A, B = _u8_rows(real, "real"), _u8_rows(fake, "fake")
    if A.shape[1:] != B.shape[1:] or A.device != B.device:
        raise ValueError(f"prdc: the two sets must hold images of one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    N, M = int(A.shape[0]), int(B.shape[0])
    k = _check_k(k, "prdc", N, M)
    rad_real = ops.knn_u8(A, A, k, self0=0)[0][:, k - 1].contiguous()
    rad_fake = ops.knn_u8(B, B, k, self0=0)[0][:, k - 1].contiguous()
    in_real = ops.ball_count_u8(B, A, rad_real)                               # [M]: real balls around every fake row
    in_fake = ops.ball_count_u8(A, B, rad_fake)                               # [N]: fake balls around every real row
    nearest = ops.knn_u8(A, B, 1)[0][:, 0]
    sums = torch.stack(((in_real > 0).sum(), in_real.sum(dtype=torch.int64), (in_fake > 0).sum(), (nearest <= rad_real).sum())).cpu()   # THE host read
    p, d, r, c = (int(v) for v in sums)
    return {"precision": p / M, "recall": r / N, "density": d / (k * M), "coverage": c / N}


def prdc_generator(kind, generator, inputs, n_images=8192, k=5, batch=None, seed=0):
    """``prdc`` of ``real_images(kind, inputs, n_images)`` against ``generate(kind, generator, n_images, batch, seed)``; ``batch`` as in
    ``swd_generator``"""
    _family(kind, "prdc_generator")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    return prdc(real_images(kind, inputs, n_images), fake, k)


# ---- kernel MMD with an exact median bandwidth -----------------------------------------------------------------------------
def median_distance(images):
    """-> int32 device scalar: the lower median of the exact squared L2 distances between the bytes of all pairs of DIFFERENT images of the
    set (float in [-1, 1] through ``to_u8``, or uint8) -- the element of 0-based rank (P - 1) // 2 among the P = T (T - 1) ordered pairs,
    which is the lower median over the unordered pairs as well.  One ``ops.dist_select_u8`` call, no host read."""
    rows = _u8_rows(images, "images")
    T = int(rows.shape[0])
    if T < 2:
        raise ValueError(f"quality.median_distance: a median over pairs needs at least 2 images, got {T}")
    return ops.dist_select_u8(rows, rows, (T * (T - 1) - 1) // 2, self0=0)[0]


def _positive(values, what, name):
    try:
        vals = [float(v) for v in values]
    except TypeError:
        raise ValueError(f"quality.{what}: {name} must be a sequence of 1 .. 4 positive finite numbers") from None
    if not 1 <= len(vals) <= 4 or not all(0.0 < v < float("inf") for v in vals):
        raise ValueError(f"quality.{what}: {name} must be a sequence of 1 .. 4 positive finite numbers, got {vals}")
    return vals


def mmd_sums(real, fake, inv_gamma):
    """-> (sums, flags) on the device: sums float64 [3, nb] = (S_xx, S_yy, S_xy) of ``mmd`` for the kernels exp(-d * inv_gamma[b]) over two
    uint8 image sets, flags int32 [3] = the three calls' marks of an ``inv_gamma`` that is no finite positive number.  Three
    ``ops.kernel_sum_u8`` calls -- (X, X) and (Y, Y) without the diagonal, and (X, Y) -- and one column sum each; no host read."""
    dev = real.device
    flags = torch.empty(3, device=dev, dtype=torch.int32)
    rows = (ops.kernel_sum_u8(real, real, inv_gamma, self0=0, flag=flags[0:1]), ops.kernel_sum_u8(fake, fake, inv_gamma, self0=0, flag=flags[1:2]),
            ops.kernel_sum_u8(real, fake, inv_gamma, flag=flags[2:3]))
    return torch.stack([r.sum(0) for r in rows]), flags


def mmd(real, fake, scales=(0.5, 1.0, 2.0), bandwidths=None):
    """Kernel maximum mean discrepancy (Gretton et al. 2012) between ``real`` [N, C, H, W] and ``fake`` [M, C, H, W] (float in [-1, 1] or
    uint8; N != M is allowed, N, M >= 2) with the kernels k(a, b) = exp(-d(a, b) / gamma) over the exact integer distances d between
    their bytes -> {"gamma_median", "bandwidths", "mmd2", "mmd2_biased", "mean"}.  gamma = s * gamma_median for every s of ``scales`` (at
    most 4), gamma_median the lower median distance of the pooled sets (``median_distance``: no hand-tuned constant); or ``bandwidths``:
    absolute gamma > 0, then no median is taken and "gamma_median" is None.  Per bandwidth, with S_xx / S_yy the kernel sums over ordered
    pairs of different rows and S_xy over all pairs:

        mmd2        = S_xx / (N (N - 1)) + S_yy / (M (M - 1)) - 2 S_xy / (N M)         unbiased, may be slightly negative
        mmd2_biased = (S_xx + N) / N^2 + (S_yy + M) / M^2 - 2 S_xy / (N M)

    "mean" = the mean of "mmd2": the MMD^2 of the mean of the kernels.  One select on the pool and three kernel-sum calls (``mmd_sums``);
    the inverse bandwidths are formed on the device from the select's result.  A median of 0 (more than half of the pairs are
    duplicates) raises ValueError.  One host read, at the end: the median, the sums and the flags."""
    A, B = _u8_rows(real, "real"), _u8_rows(fake, "fake")
    if A.shape[1:] != B.shape[1:] or A.device != B.device:
        raise ValueError(f"mmd: the two sets must hold images of one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    N, M = int(A.shape[0]), int(B.shape[0])
    if N < 2 or M < 2:
        raise ValueError(f"mmd: both sets need at least 2 images, got {N} and {M}")
    dev = A.device
    if bandwidths is None:
        factors = _positive(scales, "mmd", "scales")
        pool = torch.cat((A, B))
        T = N + M
        sel = ops.dist_select_u8(pool, pool, (T * (T - 1) - 1) // 2, self0=0)
        gamma = sel[0].double() * torch.tensor(factors, device=dev, dtype=torch.float64)
    else:
        factors = _positive(bandwidths, "mmd", "bandwidths")
        sel = torch.zeros(2, device=dev, dtype=torch.int32)
        gamma = torch.tensor(factors, device=dev, dtype=torch.float64)
    nb = len(factors)
    sums, flags = mmd_sums(A, B, gamma.reciprocal())
    host = torch.cat((sel.double(), flags.double(), sums.reshape(-1))).cpu()       # THE host read
    med = None if bandwidths is not None else int(host[0])
    if med == 0:
        raise ValueError(f"mmd: the median distance of the pooled {N} + {M} images is zero -- more than half of the pairs are duplicates, "
                         "there is no median bandwidth (pass bandwidths=)")
    if int(host[1]) or any(int(v) for v in host[2:5]):
        raise ValueError(f"mmd: the select or a kernel sum refused its arguments (rank mark {int(host[1])}, bandwidth flags {[int(v) for v in host[2:5]]})")
    S = host[5:].reshape(3, nb).tolist()
    unbiased = [S[0][b] / (N * (N - 1)) + S[1][b] / (M * (M - 1)) - 2.0 * S[2][b] / (N * M) for b in range(nb)]
    biased = [(S[0][b] + N) / (N * N) + (S[1][b] + M) / (M * M) - 2.0 * S[2][b] / (N * M) for b in range(nb)]
    return {"gamma_median": med, "bandwidths": [f * med for f in factors] if med is not None else factors, "mmd2": unbiased, "mmd2_biased": biased,
            "mean": sum(unbiased) / nb}


def mmd_witness(real, fake, queries, bandwidth):
    """-> float64 [nq] on the device: the witness function of the MMD at ``bandwidth`` (an absolute gamma > 0, e.g. one of ``mmd``'s
    "bandwidths"), w(z) = (1/N) sum_i k(z, real[i]) - (1/M) sum_j k(z, fake[j]) for every image z of ``queries``: positive where the data
    are denser than the samples, negative where the generator over-produces.  Two ``ops.kernel_sum_u8`` calls, no host read."""
    A, B, Z = _u8_rows(real, "real"), _u8_rows(fake, "fake"), _u8_rows(queries, "queries")
    if A.shape[1:] != B.shape[1:] or A.shape[1:] != Z.shape[1:] or A.device != B.device or A.device != Z.device:
        raise ValueError(f"mmd_witness: the three sets must hold images of one shape on one device, got {tuple(A.shape)}, {tuple(B.shape)} "
                         f"and {tuple(Z.shape)}")
    gamma = _positive((bandwidth,), "mmd_witness", "bandwidth")
    ig = torch.tensor(gamma, device=A.device, dtype=torch.float64).reciprocal()
    return ops.kernel_sum_u8(Z, A, ig)[:, 0] / A.shape[0] - ops.kernel_sum_u8(Z, B, ig)[:, 0] / B.shape[0]


def mmd_generator(kind, generator, inputs, n_images=8192, batch=None, seed=0, **kw):
    """``mmd`` of ``real_images(kind, inputs, n_images)`` against ``generate(kind, generator, n_images, batch, seed)``; ``batch`` as in
    ``swd_generator``; ``kw``: scales, bandwidths"""
    _family(kind, "mmd_generator")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    return mmd(real_images(kind, inputs, n_images), fake, **kw)


# ---- debiased Sinkhorn divergence ------------------------------------------------------------------------------------------
def sinkhorn(real, fake, scale=0.1, epsilon=None, iterations=60, rho=0.5, terms=False):
    """Debiased Sinkhorn divergence (Genevay et al. 2018; Feydy et al. 2019) between ``real`` [N, C, H, W] and ``fake`` [M, C, H, W] (float
    in [-1, 1] or uint8; N != M is allowed, N, M >= 2) with uniform weights and the exact integer squared distance between their bytes as
    the cost: S = OT_eps(X, Y) - OT_eps(X, X) / 2 - OT_eps(Y, Y) / 2, zero for equal sets, the Wasserstein cost as eps -> 0
    -> {"gamma_median", "epsilon", "iterations", "divergence", "relative", "ot_xy", "ot_xx", "ot_yy", "marginal_error"}.

    eps = ``scale`` x gamma_median, the lower median distance of the pooled sets (one ``ops.dist_select_u8``, as in ``mmd``); or
    ``epsilon``: an absolute eps > 0, then no median is taken and "gamma_median" and "relative" are None.  Iteration t runs at
    eps_t = max(eps, eps_0 rho^t), eps_0 the largest pooled distance (a second select, at the last rank); the inverse values are formed
    on the device.  Three problems, each a fixed number of symmetric (Jacobi) averaged updates by ``ops.softmin_u8`` from potentials 0:

        XY:  f' = (f + softmin(X, Y, g)) / 2 and g' = (g + softmin(Y, X, f)) / 2, both from the OLD potentials
        XX:  p' = (p + softmin(X, X, p)) / 2, in place, the diagonal included;   YY:  r likewise

    ot_xy = mean f + mean g, ot_xx = 2 mean p, ot_yy = 2 mean r, divergence = mean(f - p) + mean(g - r), relative = divergence /
    gamma_median.  "marginal_error" = mean_i |exp((f_i - softmin(X, Y, g)_i) / eps) - 1|, the row-marginal error of the XY plan after
    the loop: how far the fixed iteration count is from convergence.  ``terms=True``: -> (that dictionary, f - p [N], g - r [M]),
    float64 on the device: the per-image shares, whose means add up to "divergence" -- large for a real image the generator does not
    reach, and for a sample far from the data.  A median of 0, an eps that is no finite positive number and non-finite potentials raise
    ValueError.  Every launch is enqueued up front; one host read, at the end."""
    A, B = _u8_rows(real, "real"), _u8_rows(fake, "fake")
    if A.shape[1:] != B.shape[1:] or A.device != B.device:
        raise ValueError(f"sinkhorn: the two sets must hold images of one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    N, M = int(A.shape[0]), int(B.shape[0])
    if N < 2 or M < 2:
        raise ValueError(f"sinkhorn: both sets need at least 2 images, got {N} and {M}")
    iterations, rho = int(iterations), float(rho)
    if iterations < 1 or not 0.0 < rho < 1.0:
        raise ValueError(f"sinkhorn: iterations = {iterations} must be >= 1 and rho = {rho} in (0, 1)")
    value, what = (scale, "scale") if epsilon is None else (epsilon, "epsilon")
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"sinkhorn: {what} must be a positive finite number") from None
    if not 0.0 < value < float("inf"):
        raise ValueError(f"sinkhorn: {what} must be a positive finite number, got {value}")
    dev = A.device
    pool = torch.cat((A, B))
    P = (N + M) * (N + M - 1)
    top = ops.dist_select_u8(pool, pool, P - 1, self0=0)                           # eps_0: the largest pooled distance
    if epsilon is None:
        sel = ops.dist_select_u8(pool, pool, (P - 1) // 2, self0=0)
        eps = sel[0].double() * value
    else:
        sel = torch.zeros(2, device=dev, dtype=torch.int32)
        eps = torch.tensor(value, device=dev, dtype=torch.float64)
    decay = torch.tensor([rho ** t for t in range(iterations)], dtype=torch.float64).to(dev)
    sched = torch.maximum(eps, top[0].double() * decay)                            # [iterations]
    inv = sched.reciprocal()
    flags = torch.empty(iterations + 1, device=dev, dtype=torch.int32)
    f, g = torch.zeros(N, device=dev, dtype=torch.float64), torch.zeros(M, device=dev, dtype=torch.float64)
    f2, g2, p, r = torch.empty_like(f), torch.empty_like(g), torch.zeros_like(f), torch.zeros_like(g)
    for t in range(iterations):
        ie, fl = inv[t:t + 1], flags[t:t + 1]
        ops.softmin_u8(A, B, g, ie, prev=f, out=f2, flag=fl)
        ops.softmin_u8(B, A, f, ie, prev=g, out=g2, flag=fl)
        ops.softmin_u8(A, A, p, ie, prev=p, out=p, flag=fl)
        ops.softmin_u8(B, B, r, ie, prev=r, out=r, flag=fl)
        f, f2, g, g2 = f2, f, g2, g
    last = ops.softmin_u8(A, B, g, inv[-1:], flag=flags[iterations:])
    marginal = ((f - last) * inv[-1]).exp().sub(1.0).abs().mean()
    share_x, share_y = f - p, g - r
    finite = torch.stack([v.isfinite().all() for v in (f, g, p, r, last)]).all()
    host = torch.stack((sel[0].double(), sel[1].double(), top[1].double(), flags.max().double(), finite.double(), sched[-1], f.mean(), g.mean(), p.mean(),
                        r.mean(), share_x.mean(), share_y.mean(), marginal)).cpu().tolist()       # THE host read
    med = None if epsilon is not None else int(host[0])
    if med == 0:
        raise ValueError(f"sinkhorn: the median distance of the pooled {N} + {M} images is zero -- more than half of the pairs are duplicates, "
                         "there is no median temperature (pass epsilon=)")
    if host[1] or host[2] or host[3]:
        raise ValueError(f"sinkhorn: a select or a soft minimum refused its arguments (rank marks {int(host[1])}, {int(host[2])}; epsilon flag "
                         f"{int(host[3])})")
    if not host[4]:
        raise ValueError("sinkhorn: the potentials are not finite")
    mf, mg, mp, mr, sx, sy = host[6:12]
    div = sx + sy
    out = {"gamma_median": med, "epsilon": host[5], "iterations": iterations, "divergence": div, "relative": None if med is None else div / med,
           "ot_xy": mf + mg, "ot_xx": 2.0 * mp, "ot_yy": 2.0 * mr, "marginal_error": host[12]}
    return (out, share_x, share_y) if terms else out


def sinkhorn_generator(kind, generator, inputs, n_images=8192, batch=None, seed=0, **kw):
    """``sinkhorn`` of ``real_images(kind, inputs, n_images)`` against ``generate(kind, generator, n_images, batch, seed)``; ``batch`` as in
    ``swd_generator``; ``kw``: scale, epsilon, iterations, rho, terms"""
    _family(kind, "sinkhorn_generator")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    return sinkhorn(real_images(kind, inputs, n_images), fake, **kw)


# ---- k-means bins and the NDB score ------------------------------------------------------------------------------------------
Z_975 = 1.959963984540054                                                    # the 0.975 quantile of the normal distribution: a two-sided 5 % test


def bin_uniforms(seed, bins, device="cuda"):
    """-> fp32 [bins] in [0, 1) on the device: the uniforms ``image_bins(..., seed=seed)`` seeds its k-means with (one ops.rng_fill draw
    on this module's stream SID_BINS; the generator's largest value rounds to 1.0 in fp32 and is clamped to the largest fp32 below 1)"""
    u = torch.empty(int(bins), device=torch.device(device), dtype=torch.float32)
    step = torch.zeros(1, device=u.device, dtype=torch.int32)
    ops.rng_fill(ops.RNG_UNIFORM, u, 0.0, 1.0, seed, step, SID_BINS)
    return u.clamp_(0.0, 1.0 - 2.0 ** -24)


def _check_fit(what, bins, iterations, n):
    bins, iterations = int(bins), int(iterations)
    if not 1 <= bins <= min(ops.KMEANS_MAX_BINS, int(n)):
        raise ValueError(f"quality.{what}: bins = {bins} must be in 1 .. min({ops.KMEANS_MAX_BINS}, images = {int(n)})")
    if iterations < 0:
        raise ValueError(f"quality.{what}: iterations = {iterations} must be >= 0")
    return bins, iterations


def _fit_bins(rows, bins, iterations, seed):
    """-> (Bins, the seeding's flag word on the device) for uint8 rows: no host read"""
    flag = torch.empty(1, device=rows.device, dtype=torch.int32)
    centres, labels, counts, log = ops.kmeans_u8(rows, bins, iterations, u=bin_uniforms(seed, bins, rows.device), flag=flag)
    return Bins(centres, counts, labels, log["inertia"], log["changed"]), flag


def _raise_seed_flag(what, flag, bins):
    if flag & ops.SEED_FLAG_DUPLICATES:
        raise ValueError(f"quality.{what}: the images hold fewer than bins = {bins} distinct ones: there is nothing left to seed a cell with")
    if flag:
        raise ValueError(f"quality.{what}: the seeding refused its uniforms (flag {flag})")


def image_bins(images, bins=100, iterations=20, seed=0):
    """k-means cells of an image set [N, C, H, W] (float in [-1, 1] through ``to_u8``, or uint8) over the exact squared L2 distance between
    the bytes -> ``Bins(centres, counts, labels, inertia, changed)`` on the device (``ops.kmeans_u8``: k-means++ seeding from ``seed``, a
    fixed number of Lloyd ``iterations``, centres rounded to bytes -- they are images --, ties to the lower cell, empty cells keep their
    centre).  Deterministic: the same images and seed give the same bits.  Fewer than ``bins`` distinct images raise ValueError (the one
    host read, of the seeding's flag)."""
    rows = _u8_rows(images, "images")
    bins, iterations = _check_fit("image_bins", bins, iterations, rows.shape[0])
    fit, flag = _fit_bins(rows, bins, iterations, seed)
    _raise_seed_flag("image_bins", int(flag.cpu()), bins)                    # THE host read
    return fit


def _check_centres(what, centres, rows):
    if not (isinstance(centres, torch.Tensor) and centres.dtype == torch.uint8 and centres.dim() == 4 and centres.shape[1:] == rows.shape[1:]
            and centres.device == rows.device and 1 <= centres.shape[0] <= ops.KMEANS_MAX_BINS):
        raise ValueError(f"quality.{what}: centres must be a uint8 device tensor [bins <= {ops.KMEANS_MAX_BINS}, ...] of images shaped like the "
                         f"others, {tuple(rows.shape[1:])}")
    return centres.contiguous()


def bin_counts(images, centres):
    """-> int32 [bins] on the device: how many of ``images`` (float in [-1, 1] or uint8) have ``centres[c]`` (uint8 [bins, C, H, W], e.g.
    ``image_bins(...).centres``) as their nearest centre, ties to the lower cell: one ``ops.knn_u8`` and a count, no host read"""
    rows = _u8_rows(images, "images")
    centres = _check_centres("bin_counts", centres, rows)
    labels = ops.knn_u8(rows, centres, 1)[1].reshape(-1)
    return ops.group_rows(labels, int(centres.shape[0]))[0]


def ndb_statistics(a, b, z_threshold=Z_975):
    """the host half of ``ndb``: from the real and generated counts per bin (sequences of ints) -> (dictionary, z) over Python floats.
    p = a / N, q = b / M, P = (a + b) / (N + M), SE = sqrt(P (1 - P) (1 / N + 1 / M)), z = (q - p) / SE and 0 where SE = 0; "ndb" = the
    bins with |z| > z_threshold; "js" = the Jensen-Shannon divergence of p and q in bits, with 0 log 0 = 0, in [0, 1]"""
    import math
    a, b = [int(v) for v in a], [int(v) for v in b]
    N, M = sum(a), sum(b)
    if len(a) != len(b) or not a or N < 1 or M < 1:
        raise ValueError("quality.ndb_statistics: two count vectors of one length >= 1, each with a positive sum")
    z, js = [], 0.0
    for x, y in zip(a, b):
        p, q, P = x / N, y / M, (x + y) / (N + M)
        se = math.sqrt(P * (1.0 - P) * (1.0 / N + 1.0 / M))
        z.append((q - p) / se if se > 0.0 else 0.0)
        m = 0.5 * (p + q)
        if p > 0.0:
            js += 0.5 * (p * math.log2(p / m))
        if q > 0.0:
            js += 0.5 * (q * math.log2(q / m))
    different = sum(1 for v in z if abs(v) > z_threshold)
    return {"bins": len(z), "ndb": different, "ndb_over_bins": different / len(z), "js": min(1.0, max(0.0, js)),
            "empty_real": sum(1 for v in a if v == 0), "empty_fake": sum(1 for v in b if v == 0)}, z


def ndb(real, fake, bins=100, iterations=20, seed=0, centres=None, z_threshold=Z_975, terms=False):
    """Number of statistically Different Bins (Richardson & Weiss 2018) between ``real`` [N, C, H, W] and ``fake`` [M, C, H, W] (float in
    [-1, 1] or uint8; N != M is allowed): ``real`` is cut into ``bins`` k-means cells (``image_bins(real, bins, iterations, seed)``), both
    sets are counted per cell (a, b) and every cell takes the two-proportion z-test of ``ndb_statistics``
    -> {"bins", "ndb", "ndb_over_bins", "js", "empty_real", "empty_fake", "inertia", "changed_last"}: "ndb" = the cells with
    |z| > ``z_threshold`` (default: the two-sided 5 % level), "js" the Jensen-Shannon divergence of the two histograms in bits,
    "empty_*" the cells without a real / generated image, "inertia" the fit's final sum of squared distances and "changed_last" the rows
    that changed cell in its last iteration (0: the fit is at a fixed point).  ``centres=``: uint8 [bins, C, H, W] fitted elsewhere, e.g.
    on the whole dataset; nothing is fitted then, and "inertia" and "changed_last" are None.  ``terms=True``: -> (that dictionary, z, a,
    b), Python lists per cell; z < 0 marks a cell the generator under-produces.

    Cells fitted on ``real`` itself are biased towards ``real``: two samples of one distribution give more than 0.05 x bins (2 .. 8
    instead of 2.5 for 50 bins in a numpy trial), so compare with the NDB of a held-out real split.  All numbers are Python numbers
    computed on the host from the exact integer counts.  Every launch is enqueued up front; one host read."""
    A, B = _u8_rows(real, "real"), _u8_rows(fake, "fake")
    if A.shape[1:] != B.shape[1:] or A.device != B.device:
        raise ValueError(f"ndb: the two sets must hold images of one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    try:
        z_threshold = float(z_threshold)
    except (TypeError, ValueError):
        raise ValueError("ndb: z_threshold must be a positive finite number") from None
    if not 0.0 < z_threshold < float("inf"):
        raise ValueError(f"ndb: z_threshold must be a positive finite number, got {z_threshold}")
    dev = A.device
    if centres is None:
        nb, iterations = _check_fit("ndb", bins, iterations, A.shape[0])
        fit, flag = _fit_bins(A, nb, iterations, seed)
        centres, a = fit.centres, fit.counts
        last = fit.changed[-1:].long() if iterations else torch.zeros(1, device=dev, dtype=torch.int64)
        head = torch.cat((flag.long(), fit.inertia[-1:], last))
    else:
        centres = _check_centres("ndb", centres, A)
        nb, iterations = int(centres.shape[0]), None
        a = bin_counts(A, centres)
        head = torch.zeros(3, device=dev, dtype=torch.int64)
    b = bin_counts(B, centres)
    host = torch.cat((head, a.long(), b.long())).cpu().tolist()               # THE host read
    _raise_seed_flag("ndb", host[0], nb)
    out, z = ndb_statistics(host[3:3 + nb], host[3 + nb:], z_threshold)
    out["inertia"] = None if iterations is None else host[1]
    out["changed_last"] = host[2] if iterations else None
    return (out, z, host[3:3 + nb], host[3 + nb:]) if terms else out


def bin_grid(centres, z):
    """-> fp32 [bins, C, H, W] in [0, 1] on the device: the cell centres ordered by ``z`` ascending (``ndb(..., terms=True)``'s second
    result), the most under-produced cell first; equal z keep the cell order"""
    if not (isinstance(centres, torch.Tensor) and centres.is_cuda and centres.dtype == torch.uint8 and centres.dim() == 4 and len(z) == centres.shape[0]):
        raise ValueError("quality.bin_grid: centres must be a uint8 device tensor [bins, C, H, W] and z one number per cell")
    order = sorted(range(len(z)), key=lambda c: (float(z[c]), c))
    table = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(centres.device)      # u / 255 correctly rounded
    return table[centres[torch.tensor(order, device=centres.device)].long()]


def save_bins(fp, centres, z, nrow=10):
    """writes ``bin_grid`` as a PNG, ``nrow`` centres a row, reading order = ascending z"""
    sampling.save_image(bin_grid(centres, z), fp, nrow=int(nrow))


def ndb_generator(kind, generator, inputs, n_images=8192, batch=None, seed=0, **kw):
    """``ndb`` of ``real_images(kind, inputs, n_images)`` against ``generate(kind, generator, n_images, batch, seed)``, the bins seeded by
    ``seed`` as well; ``batch`` as in ``swd_generator``; ``kw``: bins, iterations, centres, z_threshold, terms"""
    _family(kind, "ndb_generator")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    return ndb(real_images(kind, inputs, n_images), fake, seed=seed, **kw)


# ---- the radial power spectrum -----------------------------------------------------------------------------------------------
SPECTRUM_FLOOR = 1.0 / 12.0      # the power per cell of the byte rounding itself (uniform noise of variance 1/12): keeps log10 of a flat image finite
_DB = 10.0


def radial_bins(H):
    """the integer ring tables of an H x H spectrum (H = 16, 32 or 64) as numpy arrays on the host -> {"rings": B, "cell_ring": int32
    [H, H/2 + 1], "ring_start": int32 [B + 1], "ring_cells": int32 [H (H/2 + 1)], "ring_count": int32 [B], "weight": int32 [H/2 + 1]}
    (``ops.spectrum_host_tables`` without the twiddles): cell (ky, kx) of the half spectrum lies in ring b with
    (b - 1/2)^2 <= min(ky, H - ky)^2 + kx^2 < (b + 1/2)^2; ``ring_count`` sums the column weights and adds up to H^2"""
    tab = ops.spectrum_host_tables(H)
    return {k: (v if k == "rings" else v.copy()) for k, v in tab.items() if k != "cos_sin"}


def power_profile(images):
    """-> float64 [N, B] on the device: the ring means of P = |DFT of the bytes|^2 / H^2 of every image of ``images`` [N, C, H, H] (float in
    [-1, 1] through ``to_u8``, or uint8; H = 16, 32 or 64, C = 1 .. 4), averaged over the channels; ring 0 is the zero frequency.  No
    host read."""
    return ops.spectrum_u8(_u8_rows(images, "images"))


def mean_spectrum(images):
    """-> float64 [H, H] on the device: 10 log10(the mean over the images of the channel-mean P + 1/12), the half spectrum mirrored to
    the full plane (P[ky, kx] = P[-ky, -kx]) and shifted so that the zero frequency sits at [H/2, H/2].  No host read."""
    half = ops.spectrum_u8(_u8_rows(images, "images"), full=True)[1].mean(0)
    H, KX = int(half.shape[0]), int(half.shape[1])
    db = _DB * torch.log10(half + SPECTRUM_FLOOR)
    ky = (-torch.arange(H, device=db.device)) % H
    kx = H - torch.arange(KX, H, device=db.device)
    plane = torch.cat((db, db[ky][:, kx]), 1)
    return torch.roll(plane, (H // 2, H // 2), (0, 1))


def spectrum_grid(real, fake):
    """-> fp32 [2, 1, H, H] in [0, 1] on the device: ``mean_spectrum(real)`` and ``mean_spectrum(fake)``, scaled jointly (one minimum, one
    maximum for both; all zeros if they are equal)"""
    both = torch.stack((mean_spectrum(real), mean_spectrum(fake)))
    lo, hi = both.min(), both.max()
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    return ((both - lo) / span).float().unsqueeze(1)


def save_spectra(fp, real, fake):
    """writes ``spectrum_grid`` as a PNG: the real set's mean spectrum on the left, the generated set's on the right"""
    sampling.save_image(spectrum_grid(real, fake), fp, nrow=2)


def spectrum_statistics(mean_real, var_real, mean_fake, var_fake, H):
    """the host half of ``spectrum``: from the per-ring mean and unbiased variance of the log-profiles in dB of the two sets (sequences of
    B numbers, ring 0 first) -> the dictionary of ``spectrum`` over Python floats.  gap = fake - real; "distance_db" = sqrt(mean of gap^2
    over the rings 1 .. B - 1) (ring 0 is brightness, not texture); "high_db" = the mean gap over the rings b > H / 4; "peak_ring" = the
    ring b >= 1 of largest |gap|, ties to the lower ring, "peak_db" its gap; effect = gap / sqrt((var_real + var_fake) / 2), 0 where
    that is 0."""
    import math
    mr, vr, mf, vf = ([float(v) for v in seq] for seq in (mean_real, var_real, mean_fake, var_fake))
    B, H = len(mr), int(H)
    if not (len(vr) == len(mf) == len(vf) == B and B >= 2 and 0 < H // 4 < B - 1):
        raise ValueError("quality.spectrum_statistics: four vectors of one length B >= 2 and a side H with H / 4 < B - 1")
    gap = [f - r for r, f in zip(mr, mf)]
    high = gap[H // 4 + 1:]
    peak = 1
    for b in range(2, B):
        if abs(gap[b]) > abs(gap[peak]):
            peak = b
    effect = []
    for g, a, b in zip(gap, vr, vf):
        pooled = math.sqrt(0.5 * (a + b))
        effect.append(g / pooled if pooled > 0.0 else 0.0)
    return {"rings": B, "real_db": mr, "fake_db": mf, "gap_db": gap, "distance_db": math.sqrt(sum(g * g for g in gap[1:]) / (B - 1)),
            "high_db": sum(high) / len(high), "peak_db": gap[peak], "peak_ring": peak, "effect": effect}


def spectrum_moments(images):
    """-> (moments float64 [2, B], profile float64 [N, B]) on the device: the per-ring mean and unbiased variance over the images of
    L = 10 log10(``power_profile`` + 1/12) in dB; N >= 2.  No host read."""
    rows = _u8_rows(images, "images")
    if rows.shape[0] < 2:
        raise ValueError(f"quality.spectrum: a set needs at least 2 images (the variance over the set), got {int(rows.shape[0])}")
    profile = ops.spectrum_u8(rows)
    L = _DB * torch.log10(profile + SPECTRUM_FLOOR)
    return torch.stack((L.mean(0), L.var(0, unbiased=True))), profile


def spectrum_from_moments(real_moments, fake_moments, H):
    """``spectrum``'s dictionary from two ``spectrum_moments`` results [2, B] on one device: THE host read, then ``spectrum_statistics``"""
    host = torch.cat((real_moments, fake_moments)).cpu().tolist()
    return spectrum_statistics(host[0], host[1], host[2], host[3], H)


def spectrum(real, fake, terms=False):
    """The azimuthally averaged power spectrum (Durall et al. 2020) of ``real`` [N, C, H, H] against ``fake`` [M, C, H, H] (float in
    [-1, 1] or uint8; H = 16, 32 or 64, C = 1 .. 4, N, M >= 2, N != M is allowed) -> {"rings", "real_db", "fake_db", "gap_db",
    "distance_db", "high_db", "peak_db", "peak_ring", "effect"}: per ring the mean over each set of L = 10 log10(profile + 1/12) in dB
    and their gap fake - real; the rms gap over the rings >= 1, the mean gap over the rings above H / 4 (where an up-convolution's
    spectrum bends), the ring >= 1 of the largest |gap| and its gap, and per ring the gap in pooled standard deviations of L over the
    images (Cohen's d).  A generator that stamps a lattice on its images shows as a peak of tens of dB in the top rings while every
    distance between the bytes barely moves.  ``terms=True``: -> (that dictionary, profile_real [N, B], profile_fake [M, B]), the
    float64 device tensors of ``power_profile``.  One host read."""
    A, B = _u8_rows(real, "real"), _u8_rows(fake, "fake")
    if A.shape[1:] != B.shape[1:] or A.device != B.device:
        raise ValueError(f"spectrum: the two sets must hold images of one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    ma, pa = spectrum_moments(A)
    mb, pb = spectrum_moments(B)
    out = spectrum_from_moments(ma, mb, A.shape[2])
    return (out, pa, pb) if terms else out


def spectrum_generator(kind, generator, inputs, n_images=8192, batch=None, seed=0, **kw):
    """``spectrum`` of ``real_images(kind, inputs, n_images)`` against ``generate(kind, generator, n_images, batch, seed)``; ``batch`` as in
    ``swd_generator``; ``kw``: terms"""
    _family(kind, "spectrum_generator")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    return spectrum(real_images(kind, inputs, n_images), fake, **kw)


# ---- SSIM, MS-SSIM and PSNR over image pairs -----------------------------------------------------------------------------------
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli & Bovik (2003), finest level first
PAIR_DRAW_BITS = 24              # a draw inside a class is (r m) >> 24 with r uniform in [0, 2^24): the draws are fp32-ranged integers
_FLAG_CLASS = 1 << 8             # diversity's own bit beside ops.SSIM_FLAG_PAIR: a class with fewer than 2 rows


def _pairs_from_draws(i, jp):
    j = jp + (jp >= i).to(jp.dtype)
    return torch.stack((i, j), 1).to(torch.int32).contiguous()


def pair_draws(n_pairs, seed, high_i, high_j, device="cuda"):
    """-> (r_i, r_j), int64 [n_pairs] on the device: the two draws behind a pair table, uniform integers in [0, high_i) and [0, high_j)
    (two ops.rng_fill(RNG_RANDINT) draws on this module's stream SID_PAIRS, device counters 0 and 1)"""
    dev = torch.device(device)
    ri = torch.empty(int(n_pairs), device=dev, dtype=torch.int64)
    rj = torch.empty(int(n_pairs), device=dev, dtype=torch.int64)
    step = torch.zeros(1, device=dev, dtype=torch.int32)
    ops.rng_fill(ops.RNG_RANDINT, ri, 0, int(high_i), seed, step, SID_PAIRS)
    step.fill_(1)
    ops.rng_fill(ops.RNG_RANDINT, rj, 0, int(high_j), seed, step, SID_PAIRS)
    return ri, rj


def pair_table(n, n_pairs, seed=0, device="cuda"):
    """-> int32 [n_pairs, 2] on the device: ordered pairs (i, j) of DIFFERENT rows of one set of ``n`` >= 2 images, i ~ U{0 .. n - 1},
    j' ~ U{0 .. n - 2}, j = j' + (j' >= i) (``pair_draws(n_pairs, seed, n, n - 1)``): every ordered pair is equally likely.  The same
    ``seed`` gives the same table.  n <= 2^24 (the draw's bounds are fp32).  No host read."""
    n, P = int(n), int(n_pairs)
    if not (2 <= n <= 2 ** PAIR_DRAW_BITS and P >= 1):
        raise ValueError(f"quality.pair_table: need 2 <= n <= 2^{PAIR_DRAW_BITS} rows and n_pairs >= 1, got n = {n}, n_pairs = {P}")
    return _pairs_from_draws(*pair_draws(P, seed, n, n - 1, device))


def class_pair_table(labels, n_classes, n_pairs, seed=0):
    """-> (pairs int32 [n_pairs, 2], flag int32 [1]) on the device of ``labels`` (int64 [N], values in [0, n_classes)): pairs of different
    rows of ONE class.  The rows are ordered by a stable sort of the labels; pair p belongs to class k = p % n_classes, whose segment
    holds m rows; with r_i, r_j = ``pair_draws(n_pairs, seed, 2^24, 2^24)`` the places inside the segment are i = (r_i m) >> 24,
    j' = (r_j (m - 1)) >> 24, j = j' + (j' >= i) (integers; a place's probability differs from 1 / m by less than 2^-24).  A class with
    fewer than 2 rows, or a label outside [0, n_classes), raises bit 8 of ``flag`` (its pairs hold row 0 twice).  No host read."""
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int64 and labels.dim() == 1 and labels.shape[0] >= 2):
        raise ValueError("quality.class_pair_table: labels must be an int64 device tensor [N], N >= 2")
    K, P, N = int(n_classes), int(n_pairs), int(labels.shape[0])
    if not (K >= 1 and P >= 1 and N <= 2 ** PAIR_DRAW_BITS):
        raise ValueError(f"quality.class_pair_table: need n_classes >= 1, n_pairs >= 1 and N <= 2^{PAIR_DRAW_BITS}, got {K}, {P}, {N}")
    inside = (labels >= 0) & (labels < K)
    order = torch.sort(labels.clamp(0, K - 1), stable=True).indices
    counts = torch.bincount(labels.clamp(0, K - 1), minlength=K)
    start = torch.cumsum(counts, 0) - counts
    k = torch.arange(P, device=labels.device, dtype=torch.int64) % K
    m = counts[k]
    ri, rj = pair_draws(P, seed, 2 ** PAIR_DRAW_BITS, 2 ** PAIR_DRAW_BITS, labels.device)
    i = (ri * m) >> PAIR_DRAW_BITS
    jp = (rj * (m - 1).clamp_min(0)) >> PAIR_DRAW_BITS
    j = jp + (jp >= i).to(torch.int64)
    ok = m >= 2
    rows_i = torch.where(ok, order[(start[k] + i).clamp(0, N - 1)], torch.zeros_like(i))
    rows_j = torch.where(ok, order[(start[k] + j).clamp(0, N - 1)], torch.zeros_like(j))
    flag = ((~ok).any() | (~inside).any()).to(torch.int32).mul(_FLAG_CLASS).reshape(1)
    return torch.stack((rows_i, rows_j), 1).to(torch.int32).contiguous(), flag


def ms_ssim_weights(L, weights=None):
    """-> the L per-level exponents of ``ms_ssim`` as a tuple of floats: ``weights`` as given (L positive numbers), or the first L of
    ``MS_SSIM_WEIGHTS`` divided by their sum (all five, L = 5, as they are)"""
    L = int(L)
    if weights is None:
        if not 1 <= L <= len(MS_SSIM_WEIGHTS):
            raise ValueError(f"quality.ms_ssim: levels = {L} must be in 1 .. {len(MS_SSIM_WEIGHTS)}")
        total = sum(MS_SSIM_WEIGHTS[:L]) if L < len(MS_SSIM_WEIGHTS) else 1.0     # the full five are Wang's own, as published
        return tuple(w / total for w in MS_SSIM_WEIGHTS[:L])
    w = tuple(float(v) for v in weights)
    if len(w) != L or not all(0.0 < v < float("inf") for v in w):
        raise ValueError(f"quality.ms_ssim: weights must be {L} positive numbers, one per level")
    return w


def ms_ssim_from_stats(stats, weights=None):
    """-> float64 [P] on the device from ``ops.ssim_u8``'s stats [P, L, 2]: prod_{l < L - 1} max(cs_l, 0)^w_l * max(ssim_{L-1}, 0)^w_{L-1}
    in torch float64; the clamp at 0 is the TensorFlow implementation's (unrelated images do give a negative cs)"""
    L = int(stats.shape[1])
    w = torch.tensor(ms_ssim_weights(L, weights), device=stats.device, dtype=torch.float64)
    base = torch.cat((stats[:, :L - 1, 1], stats[:, L - 1:, 0]), 1).clamp_min(0.0)
    return torch.pow(base, w).prod(1)


def _pair_sets(a, b, pairs, what):
    """-> (A, B, pairs): the two sets as uint8 rows and the pair table (None: row i against row i)"""
    for name, t in (("a", a), ("b", b)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"quality.{what}: {name} must be a float or uint8 device tensor [N, C, H, W] (there is no CPU path)")
    A = _u8_rows(a, "a")
    B = A if b is a else _u8_rows(b, "b")
    if A.shape[1:] != B.shape[1:] or A.device != B.device:
        raise ValueError(f"quality.{what}: the two sets must hold images of one shape on one device, got {tuple(A.shape)} and {tuple(B.shape)}")
    if pairs is None:
        if A.shape[0] != B.shape[0]:
            raise ValueError(f"quality.{what}: without a pair table row i meets row i: the sets need one size, got {A.shape[0]} and {B.shape[0]}")
        idx = torch.arange(A.shape[0], device=A.device, dtype=torch.int32)
        pairs = torch.stack((idx, idx), 1).contiguous()
    elif not (isinstance(pairs, torch.Tensor) and pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2 and pairs.device == A.device):
        raise ValueError(f"quality.{what}: pairs must be an int32 device tensor [P, 2] beside the images")
    return A, B, pairs.contiguous()


def _window(window, sigma, device):
    return ops.ssim_window_table(int(window), sigma, device) if isinstance(window, int) else window


def ssim(a, b, pairs=None, window=11, sigma=1.5):
    """-> float64 [P] on the device: the mean SSIM (Wang et al. 2004, "valid" windows, k1 = 0.01, k2 = 0.03 on the bytes) of a[i] against
    b[j] for every row (i, j) of ``pairs`` (int32 [P, 2] on the device; None: row i against row i of two sets of one size).  Images
    [N, C, H, H], float in [-1, 1] through ``to_u8`` or uint8, H = 16, 32 or 64, C = 1 .. 4.  ``window``: the number of taps of the
    Gaussian of width ``sigma`` (``sigma=None``: uniform), or a [K] table.  No host read; a row index outside its set gives NaN."""
    A, B, pairs = _pair_sets(a, b, pairs, "ssim")
    return ops.ssim_u8(A, B, pairs, _window(window, sigma, A.device), levels=1)[0][:, 0, 0].contiguous()


def ms_ssim(a, b, pairs=None, levels=None, weights=None, window=11, sigma=1.5):
    """-> float64 [P] on the device: the multi-scale SSIM (Wang et al. 2003) of the pairs of ``ssim`` over ``levels`` levels of a 2 x 2
    mean pyramid (None: as many as the side allows, ``ops.ssim_levels``: 3 at 64 px, 2 at 32 px, 1 at 16 px with 11 taps):
    prod_{l < L - 1} max(cs_l, 0)^w_l * max(ssim_{L-1}, 0)^w_{L-1}.  ``weights``: L positive exponents; None: for L < 5 levels the first
    L of ``MS_SSIM_WEIGHTS`` divided by their sum, so the value is comparable within a workload, not with 5-level figures.  No host read."""
    A, B, pairs = _pair_sets(a, b, pairs, "ms_ssim")
    stats = ops.ssim_u8(A, B, pairs, _window(window, sigma, A.device), levels=levels)[0]
    return ms_ssim_from_stats(stats, weights)


def _psnr_from_sse(sse, numel):
    mse = sse.double() / float(numel)
    return torch.where(sse == 0, torch.full_like(mse, float("inf")), 10.0 * torch.log10(255.0 ** 2 / mse.clamp_min(2.0 ** -60)))


def psnr(a, b, pairs=None):
    """-> float64 [P] on the device: 10 log10(255^2 C H W / sse) of the pairs of ``ssim`` from the exact integer squared error of the bytes,
    +inf where the two images are equal.  No host read."""
    A, B, pairs = _pair_sets(a, b, pairs, "psnr")
    sse = ops.ssim_u8(A, B, pairs, ops.ssim_window_table(3, None, A.device), levels=1)[1]
    return _psnr_from_sse(sse, A[0].numel())


def _pair_scores(A, B, pairs, levels, weights, window, sigma):
    """one launch -> (ssim [P], ms_ssim [P], sse [P], flag [1], L) on the device"""
    flag = torch.zeros(1, device=A.device, dtype=torch.int32)
    stats, sse = ops.ssim_u8(A, B, pairs, _window(window, sigma, A.device), levels=levels, flag=flag)
    return stats[:, 0, 0].contiguous(), ms_ssim_from_stats(stats, weights), sse, flag, int(stats.shape[1])


def _raise_pair_flag(what, flag):
    if flag & _FLAG_CLASS:
        raise ValueError(f"quality.{what}: a class holds fewer than 2 images (or a label lies outside [0, n_classes)): there is no pair inside it")
    if flag & ops.SSIM_FLAG_PAIR:
        raise ValueError(f"quality.{what}: the pair table names a row outside its set")


def _reconstruction_device(target, output, levels, weights, window, sigma):
    A, B, pairs = _pair_sets(target, output, None, "reconstruction")
    ss, ms, sse, flag, L = _pair_scores(A, B, pairs, levels, weights, window, sigma)
    numel = A[0].numel()
    vec = torch.stack((sse.double().mean() / float(numel), ss.mean(), ms.mean(), flag[0].double()))
    return vec, (_psnr_from_sse(sse, numel), ss, ms), L


def _reconstruction_dict(host, L):
    import math
    mse = float(host[0])
    _raise_pair_flag("reconstruction", int(host[3]))
    return {"psnr": 10.0 * math.log10(255.0 ** 2 / mse) if mse > 0.0 else float("inf"), "mse": mse, "ssim": float(host[1]),
            "ms_ssim": float(host[2]), "levels": L}


def reconstruction(target, output, terms=False, levels=None, weights=None, window=11, sigma=1.5):
    """How good is a reconstruction: ``output`` [N, C, H, H] against ``target`` [N, C, H, H], image i against image i (float in [-1, 1] or
    uint8) -> {"psnr", "mse", "ssim", "ms_ssim", "levels"}: "mse" = the mean over the set of sse / (C H W) in squared byte units, "psnr" =
    10 log10(255^2 / mse) (inf when it is 0), "ssim" and "ms_ssim" the means of ``ssim`` and ``ms_ssim`` over the set.  ``terms=True``:
    -> (that dictionary, psnr [N], ssim [N], ms_ssim [N]), the per-image float64 device tensors.  One launch, one host read."""
    vec, per, L = _reconstruction_device(target, output, levels, weights, window, sigma)
    out = _reconstruction_dict(vec.cpu().tolist(), L)                       # THE host read
    return (out,) + per if terms else out


def projection_quality(kind, generator, target, labels, steps, lr, **kw):
    """``reconstruction(target, G(inputs))`` for the inputs ``sampling.project_images(kind, generator, target, labels, steps, lr, **kw)``
    finds, plus "loss": the mean of the last row of its ``losses`` (the mean squared error in [-1, 1] units it minimised).  The eval-mode
    generator is called as there: the sprite generators take (labels, code), the others (noise, labels, code).  One host read."""
    noise, onehot, code, losses = sampling.project_images(kind, generator, target, labels, steps, lr, **kw)
    with torch.no_grad():
        image = generator(onehot, code) if noise is None else generator(noise, onehot, code)
    vec, _, L = _reconstruction_device(sampling._dev(target), image, None, None, 11, 1.5)
    host = torch.cat((vec, losses[-1].double().mean().reshape(1))).cpu().tolist()        # THE host read
    out = _reconstruction_dict(host, L)
    out["loss"] = float(host[4])
    return out


def _diversity_device(images, n_pairs, seed, labels, n_classes, pairs, levels, weights, window, sigma):
    """-> (vec float64 on the device: [mean ms_ssim, mean ssim, duplicates, flags, by_class ...], (pairs, ms_ssim, ssim, sse), meta)"""
    if not (isinstance(images, torch.Tensor) and images.is_cuda):
        raise ValueError("quality.diversity: images must be a float or uint8 device tensor [N, C, H, W] (there is no CPU path)")
    rows = _u8_rows(images, "images")
    N = int(rows.shape[0])
    if N < 2:
        raise ValueError(f"quality.diversity: a set needs at least 2 images, got {N}")
    flags = torch.zeros(1, device=rows.device, dtype=torch.int32)
    K = 0
    if labels is not None:
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.int64 and tuple(labels.shape) == (N,)):
            raise ValueError(f"quality.diversity: labels must be an int64 device tensor [{N}], one per image")
        if n_classes is None or int(n_classes) < 1:
            raise ValueError("quality.diversity: labels need n_classes >= 1 (reading it off the labels would be a host read)")
        K = int(n_classes)
    if pairs is None:
        if labels is None:
            pairs = pair_table(N, n_pairs, seed, rows.device)
        else:
            pairs, flags = class_pair_table(labels, K, n_pairs, seed)
    A, B, pairs = _pair_sets(rows, rows, pairs, "diversity")
    ss, ms, sse, flag, L = _pair_scores(A, B, pairs, levels, weights, window, sigma)
    P = int(pairs.shape[0])
    parts = [ms.mean().reshape(1), ss.mean().reshape(1), (sse == 0).sum().double().reshape(1), (flag | flags).double()]
    if K:
        if P < K:
            raise ValueError(f"quality.diversity: n_pairs = {P} leaves a class of {K} without a pair")
        k = torch.arange(P, device=rows.device, dtype=torch.int64) % K
        sums = torch.zeros(K, device=rows.device, dtype=torch.float64).index_add_(0, k, ms)
        parts.append(sums / torch.bincount(k, minlength=K).double())
    return torch.cat(parts), (pairs, ms, ss, sse), {"pairs": P, "levels": L, "classes": K}


def _diversity_dict(host, meta):
    _raise_pair_flag("diversity", int(host[3]))
    out = {"ms_ssim": float(host[0]), "ssim": float(host[1]), "pairs": meta["pairs"], "duplicates": int(host[2]), "levels": meta["levels"]}
    if meta["classes"]:
        out["by_class"] = [float(v) for v in host[4:4 + meta["classes"]]]
    return out


def diversity(images, n_pairs=16384, seed=0, labels=None, n_classes=None, pairs=None, terms=False, levels=None, weights=None, window=11,
              sigma=1.5):
    """Has the generator collapsed: the mean MS-SSIM over random pairs of different images of ONE set [N, C, H, H] (float in [-1, 1] or
    uint8; Odena et al. 2017) -> {"ms_ssim", "ssim", "pairs", "duplicates", "levels"}: the means of ``ms_ssim`` and ``ssim`` over
    ``pair_table(N, n_pairs, seed)``, the number of pairs of identical images (sse == 0) and the number of levels.  Read it beside the same
    figure of the real images: a value close to 1, or well above theirs, means mode collapse.  With ``labels`` (int64 [N] on the device)
    and ``n_classes`` the pairs are drawn inside classes (``class_pair_table``: pair p belongs to class p % n_classes) and the result
    gains "by_class": the mean MS-SSIM of every class's pairs -- collapse inside one class hides in every set-level score; a class with
    fewer than 2 images raises ValueError.  ``pairs`` (int32 [P, 2] on the device) overrides the draw; with labels, pair p still counts
    for class p % n_classes.  ``terms=True``: -> (that dictionary, pairs, ms_ssim [P], ssim [P], sse [P]) with the device tensors.
    Deterministic: the same images and seed give the same bits.  One launch, one host read (which carries the flags)."""
    vec, per, meta = _diversity_device(images, n_pairs, seed, labels, n_classes, pairs, levels, weights, window, sigma)
    out = _diversity_dict(vec.cpu().tolist(), meta)                          # THE host read
    return (out,) + per if terms else out


def diversity_generator(kind, generator, inputs, n_images=8192, n_pairs=16384, batch=None, seed=0):
    """-> {"real": ``diversity`` of ``real_images(kind, inputs, n_images)``, "fake": ``diversity`` of ``generate(kind, generator, n_images,
    batch, seed)``, "gap": fake's ms_ssim - real's}: ONE pair table, ``pair_table(n_images, n_pairs, seed)``, serves both sets.  A gap
    well above 0 means that the generated images resemble each other more than the data do.  ``batch`` as in ``swd_generator``.  One
    host read."""
    _family(kind, "diversity_generator")
    batch = min(64, int(n_images)) if batch is None else int(batch)
    fake = generate(kind, generator, n_images, batch, seed)
    real = real_images(kind, inputs, n_images)
    table = pair_table(int(n_images), n_pairs, seed, real.device)
    rv, _, rmeta = _diversity_device(real, n_pairs, seed, None, None, table, None, None, 11, 1.5)
    fv, _, fmeta = _diversity_device(fake, n_pairs, seed, None, None, table, None, None, 11, 1.5)
    host = torch.cat((rv, fv)).cpu().tolist()                                # THE host read
    out = {"real": _diversity_dict(host[:len(rv)], rmeta), "fake": _diversity_dict(host[len(rv):], fmeta)}
    out["gap"] = out["fake"]["ms_ssim"] - out["real"]["ms_ssim"]
    return out

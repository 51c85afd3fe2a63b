"""Synthetic dSprites data and encoder weights shared by tests/make_score_golden.py and the score tests (imported by both; not a test).

The sprites are rendered from a small latents grid with float64 elementwise numpy (the same bits on every host); the weights come from
``np.random.RandomState`` (a stream numpy keeps fixed) so the fixtures store only a seed plus per-tensor checksums."""
from __future__ import annotations

import numpy as np
import torch

SMALL_SIZES = (1, 3, 2, 4, 4, 4)            # color, shape, scale, orientation, posX, posY
FULL_SIZES = (1, 3, 6, 40, 32, 32)          # the real dSprites archive
NPZ_NAME = "dsprites_ndarray_co1sh3sc6or40x32y32_64x64.npz"
WEIGHT_SEEDS = {"dsprites": 11, "colored": 12}
CAT_SCALE = 400.0
CONT_SCALE = 100.0


def latents_grid(sizes=SMALL_SIZES):
    """-> (latents_classes int64 [N,6], latents_values float64 [N,6]) in the archive's C order (dSprites value conventions)."""
    cls = np.stack(np.meshgrid(*[np.arange(s) for s in sizes], indexing="ij"), -1).reshape(-1, len(sizes)).astype(np.int64)
    lin = lambda a, b, n: np.linspace(a, b, n) if n > 1 else np.array([a])
    tables = [np.ones(sizes[0]), np.arange(1, sizes[1] + 1, dtype=np.float64), lin(0.5, 1.0, sizes[2]),
              lin(0.0, 2 * np.pi, sizes[3] + 1)[:-1], lin(0.0, 1.0, sizes[4]), lin(0.0, 1.0, sizes[5])]
    vals = np.stack([tables[j][cls[:, j]] for j in range(len(sizes))], 1)
    return cls, vals


def render(latents_values):
    """{0,1} uint8 sprites [N,64,64]: square / ellipse / triangle, scaled, rotated, placed."""
    yy, xx = np.meshgrid(np.arange(64) + 0.5, np.arange(64) + 0.5, indexing="ij")
    out = np.zeros((latents_values.shape[0], 64, 64), dtype=np.uint8)
    for i, (_, shape, scale, ori, px, py) in enumerate(latents_values):
        cx, cy, r = 18.0 + px * 28.0, 18.0 + py * 28.0, 11.0 * scale
        dx, dy = xx - cx, yy - cy
        c, s = np.cos(ori), np.sin(ori)
        u, v = (c * dx + s * dy) / r, (-s * dx + c * dy) / r
        if shape == 1:
            m = (np.abs(u) <= 0.8) & (np.abs(v) <= 0.8)
        elif shape == 2:
            m = u * u / 1.0 + v * v / 0.45 <= 1.0
        else:
            m = (v >= -0.7) & (v <= 0.9 - 1.6 * np.abs(u))
        out[i] = m
    return out


def dataset(sizes=SMALL_SIZES):
    """-> (imgs uint8 [N,64,64], latents_values, latents_classes, metadata dict as the archive stores it)"""
    cls, vals = latents_grid(sizes)
    return render(vals), vals, cls, {"latents_sizes": np.array(sizes, dtype=np.int64)}


def write_npz(path, imgs, latents_values, latents_classes, metadata):
    np.savez(path, imgs=imgs, latents_values=latents_values, latents_classes=latents_classes, metadata=np.array(metadata, dtype=object))


def _unit(x):
    return x / np.sqrt((x * x).sum())


def make_weights(template, seed, cat_scale=CAT_SCALE):
    """float32 state dict in ``template``'s key order and layout (a reference or product Encoder / Encoder_pxy state dict).  Weights
    U(-sqrt(6/fan_in), sqrt(6/fan_in)), biases U(-.001, .001); spectral-norm vectors from ten float64 power iterations on the drawn
    weight.  Random spectrally normalised trunks shrink the sparse sprites' features, so the heads' ``u`` are divided by ``cat_scale`` /
    CONT_SCALE: eval-mode SN divides by u.W.v with the stored vectors, so the logits grow by that factor and argmax takes more than one
    value."""
    rng = np.random.RandomState(seed)
    out = {}
    for k, t in template.items():
        if k.endswith("weight_u") or k.endswith("weight_v"):
            continue
        shape = tuple(t.shape)
        if k.endswith("bias"):
            out[k] = rng.uniform(-0.001, 0.001, shape)
        else:
            a = np.sqrt(6.0 / np.prod(shape[1:]))
            out[k] = rng.uniform(-a, a, shape)
    for k in template:
        if not k.endswith("weight_u"):
            continue
        base = k[: -len("weight_u")]
        W = out[base + "weight_orig"].reshape(out[base + "weight_orig"].shape[0], -1)
        v = _unit(rng.normal(size=W.shape[1]))
        for _ in range(10):
            u = _unit((W * v[None, :]).sum(axis=1))
            v = _unit((W * u[:, None]).sum(axis=0))
        if base.startswith("cat_layer"):
            u = u / cat_scale
        elif base.startswith("cont_layer"):
            u = u / CONT_SCALE
        out[base + "weight_u"], out[base + "weight_v"] = u, v
    return {k: torch.from_numpy(np.asarray(out[k], dtype=np.float32).reshape(tuple(template[k].shape))) for k in template}


def digest(a):
    """sha256 of an index / gain array as little-endian int64 (integers) or float64 values: large recorded plans are pinned by digest"""
    import hashlib
    a = np.asarray(a)
    a = a.astype("<i8") if np.issubdtype(a.dtype, np.integer) else a.astype("<f8")
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def checksums(sd):
    """[n_tensors, 2] float64: sum and abs-sum of each float32 tensor, in key order."""
    return np.array([[v.double().sum().item(), v.double().abs().sum().item()] for v in sd.values()])

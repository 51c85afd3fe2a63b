"""Generate tests/golden/score_{dsprites,colored}.npz from the reference's own score/ scripts (needs the reference tree; host only).

    python tests/make_score_golden.py [dsprites] [colored]

The reference's MIG.py / FactorVAE.py functions and classes are loaded with oracle.ref_harness.load_defs and run unchanged on torch-CPU
against a synthetic archive and checkpoints written to a temporary directory (they read ``../dsprites_ndarray_...npz`` and
``encoder_*.pt`` relative to the working directory).  Only numbers are written out.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import ref_harness as rh        # noqa: E402
import score_data as sd                     # noqa: E402

GOLD = os.path.join(HERE, "golden")
SEED = {"dsprites": 5, "colored": 6}
FULL_SEED = 7
FV_GROUPS = 60
DEGENERATE_COL = 2
DIRS = {"dsprites": "dSprites/score", "colored": "colored_dSprites/score"}
PXY_CKPT = {"dsprites": "encoder_pxy_50000.pt", "colored": "encoder_pxy_color_50000.pt"}
NAMES = ("load_data", "Encoder", "Encoder_pxy", "transformation_2D", "load_encoder", "add_color_2_img", "generate_batch_factor_code",
         "make_discretizer", "discrete_mutual_info", "discrete_entropy", "FactorVAEMetric")


def ref_globals(kind, script):
    from sklearn import metrics
    u = rh.load_defs(f"{DIRS[kind]}/utils_pxy.py", ("from_latent_vector_2_affine_para_pxy", "from_latent_vector_2_color_para_pxy",
                                                   "get_matrix_pxy_align"))
    extra = {k: u[k] for k in ("from_latent_vector_2_affine_para_pxy", "from_latent_vector_2_color_para_pxy", "get_matrix_pxy_align")
             if k in u}
    extra.update(metrics=metrics, code_dim=7 if kind == "colored" else 4, n_classes=3, img_shape=(64, 64, 1))
    g = rh.load_defs(f"{DIRS[kind]}/{script}.py", NAMES, extra=extra)
    g["trans_2D"] = g["transformation_2D"]()
    return g


def weights(kind):
    g = ref_globals(kind, "MIG")
    pxy = sd.make_weights(g["Encoder_pxy"]().state_dict(), sd.WEIGHT_SEEDS[kind])
    enc = sd.make_weights(g["Encoder"]().state_dict(), sd.WEIGHT_SEEDS[kind] + 100)
    return pxy, enc


@contextlib.contextmanager
def workdir(imgs, lv, lc, meta, pxy, enc, kind):
    """tmp/<archive>.npz and tmp/work/<checkpoints>; cwd = tmp/work for the duration"""
    tmp = tempfile.mkdtemp(prefix="eadgan_score_")
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    sd.write_npz(os.path.join(tmp, sd.NPZ_NAME), imgs, lv, lc, meta)
    torch.save(pxy, os.path.join(work, PXY_CKPT[kind]))
    torch.save(enc, os.path.join(work, "encoder_500000.pt"))
    cwd = os.getcwd()
    os.chdir(work)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield tmp
    finally:
        os.chdir(cwd)


def recording(g, colors):
    """load_encoder with output-recording hooks on both encoders, add_color_2_img that records its gains (the script's functions otherwise)"""
    outs = {"pxy": [], "enc": []}

    load = g["load_encoder"]

    def load_encoder():
        P, E = load()
        P.register_forward_hook(lambda m, i, y: outs["pxy"].append(y.detach().clone()))
        E.register_forward_hook(lambda m, i, y: outs["enc"].append((y[0].detach().clone(), y[1].detach().clone())))
        return P, E

    orig = g.get("add_color_2_img")

    def add_color(img):
        img, code = orig(img)
        colors.append(code.reshape(-1, 3).copy())
        return img, code

    g["load_encoder"] = load_encoder
    if orig is not None:
        g["add_color_2_img"] = add_color
    return outs


def rows(outs, i):
    """the reference's representation rows of recorded call i + the cat probabilities"""
    cat, cont = outs["enc"][i]
    pxy = outs["pxy"][i]
    return np.concatenate((np.argmax(cat.numpy(), axis=1).reshape(-1, 1), cont.numpy()[:, 0:2], pxy.numpy()[:, 1:3]), axis=1), cat.numpy()


def split(codes):
    """float64 rows -> (int8 cat, float32 [n,4]); lossless: the rows are float32 values and small integers"""
    cat, cols = codes[:, 0].astype(np.int8), codes[:, 1:].astype(np.float32)
    assert np.array_equal(np.concatenate([cat[:, None].astype(np.float64), cols.astype(np.float64)], 1), codes)
    return cat, cols


def fv_plan_indices(kind, sizes, seed):
    """FactorVAE load_data's plan read back through an archive whose images are their own indices"""
    g = ref_globals(kind, "FactorVAE")
    cls, lv = sd.latents_grid(sizes)
    N = lv.shape[0]
    with workdir(np.arange(N, dtype=np.int64), lv, cls, {"latents_sizes": np.array(sizes, dtype=np.int64)}, {}, {}, kind):
        np.random.seed(seed)
        _, md, _, _ = g["load_data"]()
    return np.stack([d["img"] for d in md["groups"]]), np.array([d["label"] for d in md["groups"]]), md["img_eval_std"]


def make(kind):
    torch.set_num_threads(8)
    colored = kind == "colored"
    imgs, lv, lc, meta = sd.dataset()
    N = imgs.shape[0]
    pxy, enc = weights(kind)
    out = {"sizes": np.array(sd.SMALL_SIZES), "sprites_bits": np.packbits(imgs.reshape(N, -1), axis=1), "latents_values": lv,
           "weight_seeds": np.array([sd.WEIGHT_SEEDS[kind], sd.WEIGHT_SEEDS[kind] + 100]), "pxy_checksums": sd.checksums(pxy),
           "enc_checksums": sd.checksums(enc), "cat_scale": np.array(sd.CAT_SCALE), "seed": np.array(SEED[kind])}

    # ---- MIG (module-level code of MIG.py) ----
    g = ref_globals(kind, "MIG")
    colors = []
    outs = recording(g, colors)
    with workdir(imgs, lv, lc, meta, pxy, enc, kind):
        np.random.seed(SEED[kind])
        img, latents_values = g["load_data"]()
        refined = np.concatenate([latents_values[:, 1:6], np.arange(N)[:, None]], axis=1)      # + the row index, read back below
        g["encoder_pxy"], g["encoder_r_cat"] = g["load_encoder"]()
        mus, ys = g["generate_batch_factor_code"](img, refined, g["encoder_pxy"], g["encoder_r_cat"], 1000, 16)
        idx, ys = ys[5].astype(np.int64), ys[:5]
        disc = g["make_discretizer"](mus, 20)
        m = g["discrete_mutual_info"](disc, ys)
        H = g["discrete_entropy"](ys)
        sorted_m = np.sort(m, axis=0)[::-1]
        score = np.mean(np.divide(sorted_m[0, :] - sorted_m[1, :], H[:]))
    probs = np.concatenate([o[0].numpy() for o in outs["enc"]])
    out.update(mig_idx=idx.astype(np.uint16), mig_mus=mus.T.copy(), mig_disc=disc.T.astype(np.int8), mig_m=m, mig_H=H, mig_score=np.array(score),
               mig_probs=probs.astype(np.float32))
    if colored:
        out["mig_gains"] = np.concatenate(colors)
    assert len(np.unique(mus[0])) > 1, "cat code is constant: raise CAT_SCALE"

    # ---- FactorVAE (module-level code of FactorVAE.py on the first FV_GROUPS groups) ----
    gidx, labels, eidx = fv_plan_indices(kind, sd.SMALL_SIZES, SEED[kind])
    g = ref_globals(kind, "FactorVAE")
    colors = []
    outs = recording(g, colors)
    with workdir(imgs, lv, lc, meta, pxy, enc, kind):
        np.random.seed(SEED[kind])
        _, md, _, _ = g["load_data"]()
        md["groups"] = md["groups"][:FV_GROUPS]
        res = g["FactorVAEMetric"](md).evaluate()
    ev, ev_probs = rows(outs, 0)
    grp = np.stack([rows(outs, i + 1)[0] for i in range(FV_GROUPS)])
    eval_std = np.std(ev, axis=0, keepdims=True)
    pred = np.array([np.argmin(np.std(grp[i] / eval_std, axis=0)) for i in range(FV_GROUPS)])
    votes = res["factorVAE_metric_detail"]
    assert np.array_equal(np.bincount(pred * 5 + labels[:FV_GROUPS], minlength=25).reshape(5, 5), votes)
    ec, ecols = split(ev)
    gcat, gcols = split(grp.reshape(-1, 5))
    out.update(fv_group_idx=gidx.astype(np.uint16), fv_labels=labels.astype(np.int8), fv_eval_idx=eidx.astype(np.uint16),
               fv_eval_cat=ec, fv_eval_cols=ecols, fv_eval_probs=ev_probs.astype(np.float32), fv_group_cat=gcat, fv_group_cols=gcols,
               fv_eval_std=eval_std[0], fv_predict=pred.astype(np.int8), fv_votes=votes.astype(np.int64),
               fv_metric=np.array(res["factorVAE_metric"]), fv_metric_revised=np.array(res["factorVAE_metric_revised"]),
               fv_groups=np.array(FV_GROUPS))
    if colored:
        out["fv_eval_gains"] = colors[0]
        out["fv_group_gains_sha256"] = np.array(sd.digest(np.stack(colors[1:])))

    # ---- degenerate: one constant code column (numpy / sklearn through the reference's functions) ----
    g = ref_globals(kind, "MIG")
    dmus = mus.copy()
    dmus[DEGENERATE_COL] = 0.0
    ddisc = g["make_discretizer"](dmus, 20)
    dm = g["discrete_mutual_info"](ddisc, ys)
    dsm = np.sort(dm, axis=0)[::-1]
    dev_codes, dgrp = ev.copy(), grp.copy()
    dev_codes[:, DEGENERATE_COL] = 0.0
    dgrp[:, :, DEGENERATE_COL] = 0.0
    dstd = np.std(dev_codes, axis=0, keepdims=True)
    with np.errstate(all="ignore"):
        dpred = np.array([np.argmin(np.std(dgrp[i] / dstd, axis=0)) for i in range(FV_GROUPS)])
    assert (dpred == DEGENERATE_COL).all()
    out.update(deg_col=np.array(DEGENERATE_COL), deg_disc=ddisc.T.astype(np.int8), deg_m=dm, deg_score=np.array(np.mean((dsm[0] - dsm[1]) / H)),
               deg_predict=dpred.astype(np.int8))

    if kind == "dsprites":     # the plan at the archive's sizes (indices only)
        fg, fl, fe = fv_plan_indices(kind, sd.FULL_SIZES, FULL_SEED)
        out.update(full_seed=np.array(FULL_SEED), full_labels=fl.astype(np.int8), full_group_idx_head=fg[:4].astype(np.uint32),
                   full_group_idx_sha256=np.array(sd.digest(fg)), full_eval_idx_head=fe[:64].astype(np.uint32),
                   full_eval_idx_sha256=np.array(sd.digest(fe)), full_eval_n=np.array(fe.size))
    return out


def main(kinds):
    for kind in kinds:
        out = make(kind)
        path = os.path.join(GOLD, f"score_{kind}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes; MIG", float(out["mig_score"]), "FactorVAE", float(out["fv_metric"]))


if __name__ == "__main__":
    main(sys.argv[1:] or ["dsprites", "colored"])

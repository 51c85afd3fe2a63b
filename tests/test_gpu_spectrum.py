"""The radial power spectrum on the MI355X: ``ops.spectrum_u8`` and ``quality.spectrum`` against the numpy restatement
(tests/spectrum_refs.py: np.fft.rfft2, the integer ring rule) at the launch edges.

The tolerance on a profile or full-spectrum entry is derived, not tuned: u = 2^-53, S = the image's largest per-channel byte sum,
gamma = H u bounds a fp64 dot product of H terms; two stages give |dX| <= 2 gamma S, with |X| <= S that is |dP| <= 4 gamma S^2 / H^2 per
cell and per ring average.  The tests assert 2^-50 S^2 / H = 8 H u S^2 / H^2, twice that, the slack covering numpy's own error.  In dB
the same tolerance goes through the logarithm: (10 / ln 10) tol / (ref + 1/12) + 1e-9 per entry, averaged over the set."""
import importlib
import math
import struct

import numpy as np
import pytest
import torch

import spectrum_refs as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None

SHAPES = [(3, 3, 16), (70, 1, 32), (5, 3, 64), (2, 4, 64)]
KINDS = ["uniform", "low", "pink", "constant"]


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _images(kind, N, C, H, seed=0):
    rng = np.random.RandomState(1000 * H + 10 * N + C + seed)
    if kind == "low":
        return rng.randint(0, 4, (N, C, H, H)).astype(np.uint8)
    if kind == "pink":
        return SR.pink(rng, N, C, H)
    x = rng.randint(0, 256, (N, C, H, H)).astype(np.uint8)
    if kind == "constant":
        x[1] = 137                                                           # one flat image inside the batch
    return x


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ratio(got, ref, tol):
    return float((np.abs(got.cpu().numpy() - ref) / tol).max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N, C, H", SHAPES)
def test_profile_and_full_against_numpy(N, C, H, kind):
    x = _images(kind, N, C, H)
    tol = SR.profile_tolerance(x)
    profile, full = eg.ops.spectrum_u8(_dev(x), full=True)
    assert profile.dtype == torch.float64 and tuple(profile.shape) == (N, SR.tables(H)["rings"]) and tuple(full.shape) == (N, H, H // 2 + 1)
    rp, rf = _ratio(profile, SR.profile(x), tol), _ratio(full, SR.full(x), tol[:, :, None])
    print(f"spectrum {kind} {(N, C, H)}: max error / bound = {rp:.3e} (profile) {rf:.3e} (full)")
    assert rp <= 1.0 and rf <= 1.0
    assert torch.equal(eg.ops.spectrum_u8(_dev(x)), profile)                 # the same bits with and without `full`


def test_more_images_than_a_grid_dimension_of_65535():
    N, C, H = 66000, 1, 16
    x = _images("uniform", N, C, H)
    profile = eg.ops.spectrum_u8(_dev(x))
    r = _ratio(profile, SR.profile(x), SR.profile_tolerance(x))
    print(f"spectrum uniform {(N, C, H)}: max error / bound = {r:.3e} (profile)")
    assert r <= 1.0
    assert torch.equal(eg.ops.spectrum_u8(_dev(x[65990:])), profile[65990:])


@pytest.mark.parametrize("H", [16, 32, 64])
def test_bright_pixel_and_stripes(H):
    tab = SR.tables(H)
    v = 201
    x = np.zeros((2, 1, H, H), np.uint8)
    x[0, 0, 5, 11] = v                                                       # |X| = v in every cell: v^2 / H^2 in every ring
    x[1, 0, :, 1::2] = 255                                                   # 255^2 H^2 / 4 in the cells (0, 0) and (0, H/2), nothing elsewhere
    profile, full = eg.ops.spectrum_u8(_dev(x), full=True)
    profile, full = profile.cpu().numpy(), full.cpu().numpy()
    tol = SR.profile_tolerance(x)
    assert np.all(np.abs(profile[0] - v * v / H ** 2) <= tol[0]) and np.all(np.abs(full[0] - v * v / H ** 2) <= tol[0])
    want = np.zeros((H, H // 2 + 1))
    want[0, 0] = want[0, H // 2] = 255.0 ** 2 * H ** 2 / 4
    assert np.all(np.abs(full[1] - want) <= tol[1])
    ring = np.zeros(tab["rings"])
    ring[0], ring[H // 2] = want[0, 0], want[0, H // 2] / tab["ring_count"][H // 2]        # a wrong Nyquist weight or ring count shows here
    assert np.all(np.abs(profile[1] - ring) <= tol[1])


@pytest.mark.parametrize("C, H", [(3, 16), (1, 32), (3, 64)])
def test_shift_transpose_ring_sums_and_parseval(C, H):
    x = _images("pink", 4, C, H, seed=3)
    tol = SR.profile_tolerance(x)
    base, full = eg.ops.spectrum_u8(_dev(x), full=True)
    for other in (np.roll(x, (5, H - 3), (2, 3)), x.transpose(0, 1, 3, 2)):  # |X| is invariant under a circular shift; a transpose swaps the axes, not the rings
        assert _ratio(eg.ops.spectrum_u8(_dev(other)), base.cpu().numpy(), tol) <= 1.0
    tab = SR.tables(H)
    w = torch.from_numpy(tab["weight"]).to(DEV).double()
    member = torch.from_numpy((tab["cell_ring"].reshape(-1, 1) == np.arange(tab["rings"])).astype(np.float64)).to(DEV)
    sums = ((full * w).reshape(4, -1) @ member) / torch.from_numpy(tab["ring_count"]).to(DEV).double()
    assert _ratio(sums, base.cpu().numpy(), tol) <= 1.0                      # weighted ring sums of `full` reproduce `profile`
    energy = (x.astype(np.int64) ** 2).sum((1, 2, 3)).astype(np.float64)
    assert np.all(np.abs((full * w).sum((1, 2)).cpu().numpy() * C - energy) <= 1e-9 * energy)


def test_bits_do_not_depend_on_the_call_the_batch_or_the_position():
    x = _images("pink", 70, 1, 32)
    x[69] = x[0]
    d = _dev(x)
    first, ffull = eg.ops.spectrum_u8(d, full=True)
    again, afull = eg.ops.spectrum_u8(d, full=True)
    assert torch.equal(first, again) and torch.equal(ffull, afull)
    for n in (0, 17, 69):
        alone, alone_full = eg.ops.spectrum_u8(d[n:n + 1], full=True)
        assert torch.equal(alone[0], first[n]) and torch.equal(alone_full[0], ffull[n])
    assert torch.equal(first[0], first[69]) and torch.equal(ffull[0], ffull[69])
    y = _images("uniform", 5, 3, 64)
    whole = eg.ops.spectrum_u8(_dev(y))
    assert torch.equal(eg.ops.spectrum_u8(_dev(y[3:4]))[0], whole[3]) and torch.equal(eg.ops.spectrum_u8(_dev(y)), whole)


@pytest.fixture(scope="module")
def sets():
    rng = np.random.RandomState(7)
    real, fake = SR.pink(rng, 70, 3, 64, std=10.0), SR.pink(rng, 33, 3, 64, std=10.0)
    return real, fake, SR.profile(real), SR.profile(fake)


KEYS = ["distance_db", "effect", "fake_db", "gap_db", "high_db", "peak_db", "peak_ring", "real_db", "rings"]


def test_quality_spectrum_against_numpy(sets):
    real, fake, pr, pf = sets
    got, gr, gf = eg.quality.spectrum(_dev(real), _dev(fake), terms=True)
    ref = SR.spectrum(real, fake)
    assert sorted(got) == KEYS and got["rings"] == 46 == ref["rings"] and tuple(gr.shape) == (70, 46) and tuple(gf.shape) == (33, 46)
    assert _ratio(gr, pr, SR.profile_tolerance(real)) <= 1.0 and _ratio(gf, pf, SR.profile_tolerance(fake)) <= 1.0
    tr, tf = SR.db_tolerance(real, pr), SR.db_tolerance(fake, pf)
    tg = tr + tf
    worst = max(float(np.max(np.abs(np.array(got[k]) - np.array(ref[k])) / t)) for k, t in (("real_db", tr), ("fake_db", tf), ("gap_db", tg)))
    print(f"quality.spectrum: max dB error / tolerance = {worst:.3e}; distance {got['distance_db']:.4f} dB, peak ring {got['peak_ring']}")
    assert worst <= 1.0
    assert got["peak_ring"] == ref["peak_ring"] and abs(got["peak_db"] - ref["peak_db"]) <= tg[ref["peak_ring"]]
    assert abs(got["high_db"] - ref["high_db"]) <= tg[17:].mean()            # a mean of gaps
    assert abs(got["distance_db"] - ref["distance_db"]) <= math.sqrt(np.mean(tg[1:] ** 2))      # the rms is 1-Lipschitz in the rms norm
    # effect = gap / pooled: d(effect) <= (d(gap) + |effect| d(pooled)) / pooled; a standard deviation moves by at most
    # sqrt(N / (N - 1)) max_n |dL|, and pooled = |(sd_real, sd_fake)| / sqrt(2) by no more than the larger of the two
    per_image = lambda x, p: ((10.0 / math.log(10.0)) * SR.profile_tolerance(x) / (p + SR.FLOOR) + 1e-9).max(0)
    t_sd = np.maximum(per_image(real, pr) * math.sqrt(70 / 69), per_image(fake, pf) * math.sqrt(33 / 32))
    pooled = np.sqrt(0.5 * (SR.moments(real)[1] + SR.moments(fake)[1]))
    t_eff = 1.01 * (tg + np.abs(ref["effect"]) * t_sd) / pooled
    assert np.all(np.abs(np.array(got["effect"]) - np.array(ref["effect"])) <= t_eff)
    assert eg.quality.spectrum(_dev(real), _dev(fake)) == got and torch.equal(eg.quality.power_profile(_dev(real)), gr)


def test_equal_sets_give_exact_zeros_and_floats_take_the_byte_route(sets):
    real, fake, _, _ = sets
    same = eg.quality.spectrum(_dev(real), _dev(real.copy()))
    assert same["gap_db"] == [0.0] * 46 and same["distance_db"] == 0.0 and same["high_db"] == 0.0 and same["peak_db"] == 0.0
    assert same["peak_ring"] == 1 and same["effect"] == [0.0] * 46 and same["real_db"] == same["fake_db"]
    as_float = lambda x: _dev(x).float().mul(2.0 / 255.0).sub(1.0)           # how the trainers see a byte
    assert torch.equal(eg.quality.to_u8(as_float(real)), _dev(real))
    assert eg.quality.spectrum(as_float(real), as_float(fake)) == eg.quality.spectrum(_dev(real), _dev(fake))
    assert eg.quality.spectrum(as_float(real), _dev(fake)) == eg.quality.spectrum(_dev(real), _dev(fake))


def test_a_lattice_of_six_grey_levels_shows_in_the_top_rings(sets):
    """the up-convolution artefact in its plainest form; a numpy trial of the contract gave +23.8 dB at ring 45, +7.8 dB at ring 32 and
    at most 0.1 dB elsewhere for 1/f images with a ring-32 floor of about 40 per cell (a standard deviation of about 10 grey levels)"""
    real = sets[0]
    got = eg.quality.spectrum(_dev(real), _dev(SR.lattice(real)))
    print(f"lattice: peak ring {got['peak_ring']} {got['peak_db']:.2f} dB, ring 32 {got['gap_db'][32]:.2f} dB, "
          f"rings 1 .. 30 at most {max(abs(g) for g in got['gap_db'][1:31]):.4f} dB, distance {got['distance_db']:.3f} dB")
    assert got["peak_ring"] == 45 and got["peak_db"] > 10.0 and got["gap_db"][32] > 3.0
    assert all(abs(g) < 1.0 for g in got["gap_db"][1:31])


def test_mean_spectrum_and_the_figure(sets, tmp_path):
    real, fake, _, _ = sets
    got = eg.quality.mean_spectrum(_dev(real))
    assert got.dtype == torch.float64 and tuple(got.shape) == (64, 64)
    ref = SR.mean_spectrum(real)
    mean_power = 10.0 ** (ref / 10.0)                                        # = mean_n full + 1/12
    tol = (10.0 / math.log(10.0)) * SR.profile_tolerance(real).mean() / mean_power + 1e-9
    assert float((np.abs(got.cpu().numpy() - ref) / tol).max()) <= 1.0
    assert int(got.argmax()) == 32 * 64 + 32                                 # the zero frequency sits at [H/2, H/2]
    grid = eg.quality.spectrum_grid(_dev(real), _dev(SR.lattice(fake)))
    assert tuple(grid.shape) == (2, 1, 64, 64) and float(grid.min()) == 0.0 and float(grid.max()) == 1.0
    path = str(tmp_path / "spectra.png")
    eg.quality.save_spectra(path, _dev(real), _dev(SR.lattice(fake)))
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", data[16:24]) == (2 * 64 + 6, 64 + 4)


def test_refusals():
    ok = torch.zeros(4, 3, 64, 64, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="device tensor"):
        eg.quality.spectrum(ok.cpu(), ok)
    with pytest.raises(ValueError, match="no CPU path"):
        eg.ops.spectrum_u8(ok.cpu())
    for bad, text in ((torch.zeros(4, 3, 48, 48, dtype=torch.uint8, device=DEV), "side in"),
                      (torch.zeros(4, 3, 64, 32, dtype=torch.uint8, device=DEV), "square"),
                      (torch.zeros(4, 5, 64, 64, dtype=torch.uint8, device=DEV), "C = 5")):
        with pytest.raises(ValueError, match=text):
            eg.quality.spectrum(bad, bad)
        with pytest.raises(ValueError, match=text):
            eg.ops.spectrum_u8(bad)
    with pytest.raises(ValueError, match="at least 2 images"):
        eg.quality.spectrum(ok[:1], ok)
    with pytest.raises(ValueError, match="at least 2 images"):
        eg.quality.spectrum(ok, ok[:1])
    with pytest.raises(ValueError, match="one shape on one device"):
        eg.quality.spectrum(ok, ok[:, :1])
    with pytest.raises(ValueError, match="one shape on one device"):
        eg.quality.spectrum(ok, torch.zeros(4, 3, 32, 32, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="uint8"):
        eg.ops.spectrum_u8(ok.float())
    with pytest.raises(ValueError, match="sprite workloads"):
        eg.quality.spectrum_generator("dsprites", None, ok)
    flat = eg.quality.spectrum(ok, ok)                                       # all-zero images: finite through the 1/12 floor
    assert all(abs(v - 10.0 * math.log10(1.0 / 12.0)) < 1e-9 for v in flat["real_db"])
    assert flat["distance_db"] == 0.0 and flat["effect"] == [0.0] * 46

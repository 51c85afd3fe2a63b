"""The Sinkhorn divergence on the MI355X: ops.softmin_u8 and quality.sinkhorn against the numpy restatement
tests/sinkhorn_refs.py.  Every comparison of a soft minimum holds within ``sinkhorn_refs.tolerance(n, eps, tmax)``, a bound from the
arithmetic of the two sides (its docstring), with tmax taken from the reference's own arguments; a whole ``sinkhorn`` within iterations x
the largest such bound of its calls.  The potentials g are drawn so that the arguments t = (g - d) / eps span several hundred units: the
running maximum of the streaming log-sum-exp moves, and most terms underflow against it."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import knn_refs as R
import sinkhorn_refs as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
eg = None
EPS = 1000.0            # distances between random rows of 64 bytes spread over some 1e5: t spans hundreds of units


def setup_module(module):
    global eg
    eg = importlib.import_module("ead-gan_amd")


def _tiles():
    ops = importlib.import_module("ead-gan_amd").ops
    return ops.knn_tile_queries(), ops.knn_tile_rows()


def _rand(shape, seed, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, shape).astype(np.uint8)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(DEV)


def _pot(n, seed, span=2e5):
    return np.random.RandomState(seed).uniform(-span, span, n)


def _ie(eps):
    return torch.tensor([1.0 / eps], device=DEV, dtype=torch.float64)


def _close(got, want, tol, what=None):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    err = np.abs(got - want)
    print(what, "largest error", float(err.max()), "bound", tol)
    assert got.shape == want.shape and np.isfinite(got).all() and (err <= tol).all(), (what, float(err.max()), tol)


def _check(q, x, g, eps, self0=-1, prev=None, d=None, what=None):
    """one device call against the reference; -> the device's result"""
    st = {}
    d = R.distances(q, x) if d is None else d
    want = SR.softmin_d(d, g, 1.0 / eps, self0, prev, st)
    got = eg.ops.softmin_u8(q if isinstance(q, torch.Tensor) else _dev(q), x if isinstance(x, torch.Tensor) else _dev(x), _dev(g), _ie(eps), self0,
                            None if prev is None else _dev(prev))
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(d),)
    _close(got, want, SR.tolerance(d.shape[1], eps, st["tmax"]), what)
    return got, st


@functools.lru_cache(maxsize=None)
def _grid(K):
    q, x = _rand((300, K), 1 + K), _rand((333, K), 2 + K)
    return q, x, R.distances(q, x)


# ---- 1. the soft minimum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 192])
def test_softmin_on_both_layouts_and_partial_tiles(K):
    Tq, Tr = _tiles()
    assert 70 > Tq and 70 % Tq and 300 >= 4 * Tq and (128, 129) == (Tr, Tr + 1)       # a partial narrow tile, the wide layout, a full tile and one more row
    q, x, d = _grid(K)
    qd, xd = _dev(q), _dev(x)
    g, prev = _pot(333, 3), _pot(300, 4, 1e5)
    eps = EPS * K / 64
    for nq in (70, 300):
        for n in (1, 5, 128, 129, 333):                            # n = 1 and 5: most parts of the tile get no offer and hold (-inf, 0)
            _, st = _check(qd[:nq], xd[:n], g[:n], eps, d=d[:nq, :n], what=(K, nq, n))
            assert n == 1 or st["tmax"] > 300
            if n in (5, 333):
                _check(qd[:nq], xd[:n], g[:n], eps, prev=prev[:nq], d=d[:nq, :n], what=(K, nq, n, "prev"))


def _first_split_n(nq):
    Tq, Tr = _tiles()
    for n in range(1, 64 * Tr):
        if eg.ops.knn_splits(nq, n) >= 2:
            return n
    raise AssertionError("the split policy does not cut a database of 64 tiles for so few queries")


def test_softmin_over_database_slices():
    Tq, Tr = _tiles()
    cases = []
    for nq in (5, 70):
        n0 = _first_split_n(nq)
        assert eg.ops.knn_splits(nq, n0 - 1) == 1
        cases += [(nq, n0), (nq, n0 + Tr + 3)]
    assert eg.ops.knn_splits(3, 40 * Tr + 9) == 41
    for nq, n in cases + [(3, 40 * Tr + 9)]:
        assert eg.ops.knn_splits(nq, n) >= 2
        q, x = _rand((nq, 64), 7 + n), _rand((n, 64), 300 + n)
        g = _pot(n, n)
        g[n - 1] += 4e5                                            # the last row of the last slice holds the maximum of most queries
        _check(q, x, g, EPS, what=(nq, n))
        _check(q, x, g, 50 * EPS, prev=_pot(nq, 5), what=(nq, n, "warm"))       # every slice contributes


def test_softmin_at_the_celeba_row_length():
    q, x = _rand((64, 3, 64, 64), 1, 100, 156), _rand((200, 3, 64, 64), 2, 100, 156)
    x[150] = q[4]
    d = R.distances(q, x)
    g = _pot(200, 6, 3e5)
    got, st = _check(q, x, g, 2000.0, d=d, what="K = 12288")
    assert st["tmax"] > 300


def test_softmin_with_self0_in_its_four_forms():
    Tq, Tr = _tiles()
    n = 2 * Tr + 9
    x = _rand((n, 64), 15)
    tail = np.concatenate((x[n - 3:], _rand((5, 64), 16)))         # rows 3 .. 7 have self0 + i >= n and exclude nothing
    g = _pot(n, 17)
    xd = _dev(x)
    for q, self0 in ((x, -1), (x, 0), (x[37:37 + Tq + 6], 37), (tail, n - 3), (x[:9], n + 5)):
        _check(q, xd, g, EPS, self0, d=R.distances(q, x), what=("self0", self0))
    # with the diagonal, a row's own term (d = 0) is the maximum where g is large; without it the result is another
    big = np.full(n, 5e5)
    with_diag, _ = _check(x, xd, big, EPS, -1, d=R.distances(x, x))
    without, _ = _check(x, xd, big, EPS, 0, d=R.distances(x, x))
    assert bool((with_diag < without).all())
    two = x[:2]
    _check(two, two, g[:2], EPS, 0, what="n - 1 = 1")             # one candidate a query: soft = d - g of the other row


def test_softmin_with_a_maximum_far_above_and_with_every_term_far_below():
    q, x, d = _grid(64)
    nq, n = 70, 333
    g = _pot(n, 8)
    g[200] += 1e6 * EPS                                            # t of row 200 is 1e6 above the rest: every other term underflows
    got, st = _check(q[:nq], x[:n], g, EPS, d=d[:nq, :n], what="one term")
    assert st["tmax"] > 9e5
    alone = d[:nq, 200] - g[200] + EPS * math.log(n)               # that term alone
    assert np.abs(got.cpu().numpy() - alone).max() <= SR.tolerance(n, EPS, st["tmax"]) + 4 * 2.0 ** -53 * np.abs(alone).max()
    low = _pot(n, 9) - 2e6                                         # all t below -800: exp(t) is 0 in double, the sum is not
    got, st = _check(q[:nq], x[:n], low, EPS, d=d[:nq, :n], what="all below")
    assert (low[None, :] - d[:nq, :n]).max() / EPS < -800 and bool(torch.isfinite(got).all())
    high = _pot(n, 10) + 3e6                                       # and all above +800: exp(t) overflows, the pair does not
    got, _ = _check(q[:nq], x[:n], high, EPS, d=d[:nq, :n], what="all above")
    assert (high[None, :] - d[:nq, :n]).min() / EPS > 800 and bool(torch.isfinite(got).all())


def test_softmin_with_prev_given_absent_and_aliased():
    x = _rand((200, 64), 21)
    d = R.distances(x, x)
    xd = _dev(x)
    p = _pot(200, 22, 1e5)
    st = {}
    soft = SR.softmin_d(d, p, 1.0 / EPS, -1, None, st)
    tol = SR.tolerance(200, EPS, st["tmax"])
    ie = _ie(EPS)
    _close(eg.ops.softmin_u8(xd, xd, _dev(p), ie), soft, tol, "absent")
    _close(eg.ops.softmin_u8(xd, xd, _dev(p), ie, prev=_dev(p)), 0.5 * p + 0.5 * soft, tol, "given")
    buf = _dev(p)
    out = eg.ops.softmin_u8(xd, xd, buf, ie, prev=buf, out=buf)    # the in-place update of the symmetric problem
    assert out.data_ptr() == buf.data_ptr()
    _close(buf, 0.5 * p + 0.5 * soft, tol, "prev is g is out")
    separate = eg.ops.softmin_u8(xd, xd, _dev(p), ie, prev=_dev(p))
    assert torch.equal(separate.view(torch.int64), buf.view(torch.int64))
    gout = _dev(p)                                                 # g is out, without prev
    eg.ops.softmin_u8(xd, xd, gout, ie, out=gout)
    _close(gout, soft, tol, "g is out")


def test_softmin_writes_only_its_result_and_gives_the_same_bits_again():
    Tq, Tr = _tiles()
    q, x, d = _grid(192)
    nq, n, guard = Tq + 3, 2 * Tr + 1, 64
    qd, xd, g, ie = _dev(q[:nq]), _dev(x[:n]), _dev(_pot(n, 30)), _ie(3 * EPS)
    buf = torch.full((nq + 2 * guard,), -7.0, device=DEV, dtype=torch.float64)
    out = buf[guard:guard + nq]
    got = eg.ops.softmin_u8(qd, xd, g, ie, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == -7).all() and (buf[guard + nq:] == -7).all())
    st = {}
    want = SR.softmin_d(d[:nq, :n], g.cpu().numpy(), 1.0 / (3 * EPS), stats=st)
    _close(got, want, SR.tolerance(n, 3 * EPS, st["tmax"]))
    again = eg.ops.softmin_u8(qd, xd, g, ie)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = eg.ops.softmin_u8(qd, xd, g, ie)
    side.synchronize()
    assert torch.equal(third.view(torch.int64), got.view(torch.int64))
    # the workspace, through the library itself: splits * nq pairs are written, the bytes on both sides of them are not
    words = eg.ops.softmin_ws_bytes(nq, n) // 8
    assert words == eg.ops.knn_splits(nq, n) * nq * 2 and eg.ops.knn_splits(nq, n) == 3
    wsbuf = torch.full((words + 2 * guard,), -7.0, device=DEV, dtype=torch.float64)
    ws, res, flag = wsbuf[guard:guard + words], torch.empty(nq, device=DEV, dtype=torch.float64), torch.full((3,), -7, device=DEV, dtype=torch.int32)
    eg.ops.lib().call("eg_softmin_u8", qd.data_ptr(), nq, xd.data_ptr(), n, 192, g.data_ptr(), ie.data_ptr(), -1, None, ws.data_ptr(), res.data_ptr(),
                      flag[1:2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert torch.equal(res.view(torch.int64), got.view(torch.int64)) and flag.tolist() == [-7, 0, -7]
    assert bool((wsbuf[:guard] == -7).all() and (wsbuf[guard + words:] == -7).all())
    pairs = ws.reshape(-1, 2)
    assert bool(torch.isfinite(pairs).all() and (pairs[:, 1] >= 1).all())          # every slice of every query received an offer
    many_q, many_x = _dev(_rand((3, 64), 8)), _dev(_rand((40 * Tr + 9, 64), 9))    # 41 slices: the second kernel's tree
    gm = _dev(_pot(40 * Tr + 9, 31))
    a, b = eg.ops.softmin_u8(many_q, many_x, gm, _ie(EPS)), eg.ops.softmin_u8(many_q, many_x, gm, _ie(EPS))
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_a_bad_inverse_epsilon_sets_the_flag_and_nothing_else():
    q, x, d = _grid(64)
    nq, n, guard = 70, 200, 64
    qd, xd, g = _dev(q[:nq]), _dev(x[:n]), _dev(_pot(n, 40))
    flag = torch.full((3,), -7, device=DEV, dtype=torch.int32)
    buf = torch.full((nq + 2 * guard,), -7.0, device=DEV, dtype=torch.float64)
    out = buf[guard:guard + nq]
    eg.ops.softmin_u8(qd, xd, g, _ie(EPS), out=out, flag=flag[1:2])
    assert flag.tolist() == [-7, 0, -7]                            # written, whatever it held
    st = {}
    _close(out, SR.softmin_d(d[:nq, :n], g.cpu().numpy(), 1.0 / EPS, stats=st), SR.tolerance(n, EPS, st["tmax"]))
    for bad in (0.0, -1.0 / EPS, float("nan"), float("inf"), -float("inf")):
        flag.fill_(-7)
        eg.ops.softmin_u8(qd, xd, g, torch.tensor([bad], device=DEV, dtype=torch.float64), out=out, flag=flag[1:2])
        assert flag.tolist() == [-7, 1, -7], bad
        assert bool((buf[:guard] == -7).all() and (buf[guard + nq:] == -7).all()), bad


# ---- 2. quality.sinkhorn ----------------------------------------------------------------------------------------------------------------
KEYS = ["divergence", "epsilon", "gamma_median", "iterations", "marginal_error", "ot_xx", "ot_xy", "ot_yy", "relative"]


def _imgs(rows):
    return _dev(rows).reshape(len(rows), 3, 8, 8)


@functools.lru_cache(maxsize=None)
def _clustered():
    a, b = SR.clustered()
    det = {}
    return a, b, SR.sinkhorn(a, b, detail=det), det


def _check_sinkhorn(got, want, det, N, M):
    """the dictionary within iterations x tolerance per potential that enters a figure, plus the rounding of a mean of N or M numbers"""
    assert sorted(got) == KEYS and all(type(got[k]) is float for k in KEYS if k not in ("gamma_median", "iterations", "relative"))
    assert got["gamma_median"] == want["gamma_median"] and got["epsilon"] == want["epsilon"] and got["iterations"] == want["iterations"]
    size = max(np.abs(det[k]).max() for k in "fgpr")
    mean = max(N, M) * 2.0 ** -53 * size                            # a sum of n numbers in any order, and its division
    bound = det["bound"]
    print({k: (got[k], want[k]) for k in KEYS}, "bound", bound)
    for key, pots in (("ot_xy", 2), ("ot_xx", 2), ("ot_yy", 2), ("divergence", 4)):
        assert abs(got[key] - want[key]) <= pots * (bound + mean), key
    if want["relative"] is None:
        assert got["relative"] is None
    else:
        assert got["relative"] == got["divergence"] / got["gamma_median"]
    # exp is 1-Lipschitz about 0 up to the factor exp(|a|): both potentials of the exponent move by the bound
    assert abs(got["marginal_error"] - want["marginal_error"]) <= 4 * bound / want["epsilon"] * (1 + want["marginal_error"]) + 2.0 ** -50


def test_sinkhorn_on_clustered_sets():
    a, b, want, det = _clustered()
    assert a.shape == (200, 192) and b.shape == (130, 192)
    A, B = _imgs(a), _imgs(b)
    got, sx, sy = eg.quality.sinkhorn(A, B, terms=True)
    assert type(got["gamma_median"]) is int and got["iterations"] == 60 and got["epsilon"] == 0.1 * got["gamma_median"]
    _check_sinkhorn(got, want, det, 200, 130)
    assert got["marginal_error"] < 1e-2 and got["divergence"] > 0
    assert sx.dtype == torch.float64 and tuple(sx.shape) == (200,) and tuple(sy.shape) == (130,) and sx.is_cuda
    _close(sx, det["f"] - det["p"], 2 * det["bound"], "f - p")
    _close(sy, det["g"] - det["r"], 2 * det["bound"], "g - r")
    assert got["divergence"] == float(sx.mean()) + float(sy.mean())
    share = sy.cpu().numpy()                                       # the samples around the foreign centre are the ones far from the data
    assert share[100:].min() > 3 * np.abs(share[:100]).max()
    assert eg.quality.sinkhorn(A, B) == got                        # without the terms, and to the bit again
    fa = eg.quality.real_images("mnist", A, 200)                   # float input goes through to_u8
    assert eg.quality.sinkhorn(fa, B) == got
    back = eg.quality.sinkhorn(B, A)                               # N != M both ways
    assert abs(back["divergence"] - got["divergence"]) <= 8 * det["bound"] + 1e-12 * got["divergence"]
    det2 = {}
    fixed = eg.quality.sinkhorn(A, B, epsilon=20000.0, iterations=20, rho=0.7)
    assert fixed["gamma_median"] is None and fixed["relative"] is None and fixed["epsilon"] == 20000.0
    _check_sinkhorn(fixed, SR.sinkhorn(a, b, epsilon=20000.0, iterations=20, rho=0.7, detail=det2), det2, 200, 130)


def test_sinkhorn_is_zero_on_equal_sets_and_grows_with_the_distance():
    a, b, _, _ = _clustered()
    A = _imgs(a)
    same = eg.quality.sinkhorn(A, A.clone())
    assert same["divergence"] == 0.0 and same["relative"] == 0.0 and same["ot_xy"] == same["ot_xx"] == same["ot_yy"]
    near, far = (eg.quality.sinkhorn(A, _imgs((a.astype(np.int64) + s).astype(np.uint8)), iterations=30) for s in (6, 25))
    assert 0 < near["divergence"] < far["divergence"] and 0 < near["relative"] < far["relative"]
    for got, s in ((near, 6), (far, 25)):                          # a set moved by s in each of its 192 bytes: the transport cost is 192 s^2
        assert abs(got["divergence"] - 192 * s * s) < 0.01 * 192 * s * s and got["marginal_error"] < 1e-3
    dup = np.concatenate((np.repeat(a[7:8], 40, 0), a[:6]))        # 40 of 46 rows are one row: the median distance is 0
    with pytest.raises(ValueError, match="median distance .* is zero"):
        eg.quality.sinkhorn(_imgs(dup), _imgs(dup))
    assert eg.quality.sinkhorn(_imgs(dup), _imgs(dup), epsilon=1000.0)["divergence"] == 0.0
    u = torch.zeros(6, 1, 8, 8, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one shape"):
        eg.quality.sinkhorn(u, torch.zeros(6, 1, 16, 16, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at least 2"):
        eg.quality.sinkhorn(u, u[:1])
    for kw in (dict(scale=0.0), dict(scale=float("nan")), dict(epsilon=-1.0), dict(epsilon=float("inf")), dict(iterations=0), dict(rho=1.0), dict(rho=0.0)):
        with pytest.raises(ValueError, match="sinkhorn: "):
            eg.quality.sinkhorn(u, u, **kw)


# ---- 3. a generator ---------------------------------------------------------------------------------------------------------------------
def test_sinkhorn_generator_on_a_fresh_mnist_generator():
    torch.manual_seed(1)
    G = eg.mnist.Generator().to(DEV)
    data = torch.randint(112, 144, (64, 1, 32, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    before = {k: v.clone() for k, v in G.state_dict().items()}
    a = eg.quality.sinkhorn_generator("mnist", G, data, n_images=64, batch=8, seed=2)
    b = eg.quality.sinkhorn_generator("mnist", G, data, n_images=64, batch=8, seed=2)
    print(a)
    assert a == b and sorted(a) == KEYS
    assert all(math.isfinite(a[k]) for k in KEYS) and a["divergence"] > 0 and a["relative"] > 0 and a["gamma_median"] > 0
    fake = eg.quality.to_u8(eg.quality.generate("mnist", G, 64, 8, seed=2))
    assert eg.quality.sinkhorn(data, fake) == a
    after = G.state_dict()
    assert G.training and list(after) == list(before) and all(torch.equal(before[k], after[k]) for k in before)
    for kind in ("dsprites", "colored_train"):
        with pytest.raises(ValueError, match="disentanglement scores"):
            eg.quality.sinkhorn_generator(kind, G, data)

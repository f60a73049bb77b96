"""The float64 IEnKS weight update with tau = 1 on tiles (csrc/lienks_tile64.hip, mia_lienks_update_matfun_f64,
LetkfEngine.ienks_update(method="tile64")): what LocalizedIEnKSTransform / LocalizedIEnKSBundle.inner_loop run per grid point in
the reference's default working precision (core/ienks.py:108-141, interface/lienks.py:75-118).  The contract is the project's
float64 tile one: relative Frobenius error <= 1e-10 on W as a whole against O.lienks_weights and <= 1e-10 on the WORST
SINGLE GRID POINT.  Every test asserts that lienks_update64_kernel ran; where a test says so no point may carry MIA_FLAG_RETRY,
so that the general kernel cannot supply the parity."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_fro
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
LOG_TOL, MARGIN, CAP = 26.0, 2, 127            # the float64 table's truncation target, margin and degree cap
KERNEL = "lienks_update64_kernel"
GENERAL = "ienks_update_kernel<double, 256>"
EPS = 1e-3
RETRY, NONFINITE, OVERFLOW = 8, 4, 1


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def last_kernel():
    from torch_assimilate_amd import _cabi
    return _cabi.last_analysis_kernel()


def check(got, ref, what, tol=TOL64):
    """W [G][k][k] against the reference: the whole and the worst single grid point"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    pp = np.sqrt(((got - ref) ** 2).sum(axis=(1, 2))) / np.maximum(np.sqrt((ref ** 2).sum(axis=(1, 2))), 1e-300)
    fro = rel_fro(got, ref)
    worst = float(pp.max()) if pp.size else 0.0
    print("\n[ienks64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, worst, int(pp.argmax()) if pp.size else -1))
    assert fro <= tol, what
    assert worst <= tol, what
    return fro, worst


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel() and "ienks_update_kernel" not in last_kernel()


def upd(eng, w_in, yb, d, nb, eps, method="tile64", **kw):
    """engine.ienks_update with its flags: (W, flags as numpy, kernel name)"""
    f32_first(eng)
    res = eng.ienks_update(dev(w_in), dev(yb), dev(d), nb, 1.0, eps, return_flags=True, method=method, **kw)
    torch.cuda.synchronize()
    return res[0], res[1].cpu().numpy(), last_kernel()


def expected_degrees64(yb, nb, inf=1.0):
    """Chebyshev degree per grid point as the float64 tile kernels choose it (tests/test_gpu_weights64.py), restated in float64
    numpy from the per-point lists: Gershgorin bound L of S = D G D, T = L / reg rounded up to the table's geometric grid (32 per
    octave, 2^-24 .. 2^8), degree = ceil(26 / log rho) + 2, rho = (sqrt(1 + T) + 1) / (sqrt(1 + T) - 1).  For the bundle variant
    ``yb`` is Yb / eps: the bound is that of the scaled S."""
    cnt, idx, w = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy(), nb.w.cpu().numpy()
    k = yb.shape[0]
    reg = (k - 1) / inf
    out = []
    for g in range(len(cnt)):
        D, Y = w[g, :cnt[g]], yb[:, idx[g, :cnt[g]]]
        L = max(float(np.max(D * (np.abs(Y.T @ Y) @ D), initial=0.0)), 1e-300 * reg) * (1.0 + 1e-12)
        ti = int(np.clip(np.ceil(32 * np.log2(L / reg)) + 24 * 32, 0, 32 * 32 - 1))
        sq = np.sqrt(1 + 2.0 ** ((ti - 24 * 32) / 32))
        out.append(max(3, int(np.ceil(LOG_TOL / np.log((sq + 1) / max(sq - 1, 1e-12))) + MARGIN)))
    return np.array(out)


def weights_in(G, k, seed, bundle):
    """per-point incoming weights.  Bundle: I + 0.3 A / sqrt(k) + 0.1 m 1^T with a random row-centred A -- Wp far from I, which
    the bundle variant never looks at; transform: I + 0.1 m 1^T -- Wp = I, another mean at every point."""
    rs = np.random.RandomState(1000 + seed)
    m = rs.normal(size=(G, k, 1))
    W = np.eye(k)[None] + 0.1 * m * np.ones((1, 1, k))
    if bundle:
        A = rs.normal(size=(G, k, k))
        W = W + 0.3 * (A - A.mean(axis=2, keepdims=True)) / np.sqrt(k)
    return W


@functools.lru_cache(maxsize=None)
def case1d(G, k, stride, seed):
    return O.synthetic_case(G, k, stride, seed=seed)


# ---- 1. shape sweep against the oracle, both variants, nothing declined ---------------------------------------------------------
SWEEP = [(8, 1, 2.0), (20, 2, 9.0), (27, 1, 6.0), (40, 2, 18.0), (40, 4, 36.0), (64, 1, 15.0), (64, 2, 28.0)]


@pytest.mark.parametrize("k,stride,c", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, stride, c):
    """UT 1 .. 4, KT 1 .. 4, k no multiple of 4, a ragged last tile; per-point incoming weights.  The degrees are the restated
    rule's, none above the cap, and no point is declined: the parity is the tile kernel's own."""
    G = 67 if k == 64 else 203
    case = case1d(G, k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert 0 < nb.p_max <= k
    for vname, eps, scale in (("bundle", EPS, EPS), ("transform", None, 1.0)):
        yb = case["yb"] * scale
        w_in = weights_in(G, k, k, eps is not None)
        want = expected_degrees64(yb / scale, nb)
        assert int(want.max()) <= CAP
        W, fl, kern = upd(eng, w_in, yb, case["d"], nb, eps)
        assert KERNEL in kern, kern
        assert int((fl & 0xff).max()) == 0, vname                           # nothing declined, nothing non-finite
        assert np.array_equal((fl >> 8) & 0xff, want), vname
        ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], yb, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s k %d stride %d c %g p_max %d (%s)" % (vname, k, stride, c, nb.p_max, kern))


def test_shared_prior_and_a_tiny_ensemble(eng):
    """ONE (k, k) matrix for all points (w_stride = 0: the prior of the first iteration), both variants; and k = 3 with lists of
    at most three observations."""
    G, k, stride, c = 203, 20, 2, 9.0
    case = case1d(G, k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    for vname, eps, scale in (("bundle", EPS, EPS), ("transform", None, 1.0)):
        W, fl, kern = upd(eng, np.eye(k), case["yb"] * scale, case["d"], nb, eps)
        assert KERNEL in kern and int((fl & 0xff).max()) == 0
        ref = O.lienks_weights(np.eye(k), case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, shared prior" % vname)
    # a shared matrix with another mean (bundle: any Wp)
    w1 = weights_in(1, k, 5, True)[0]
    W, fl, kern = upd(eng, w1, case["yb"] * EPS, case["d"], nb, EPS)
    assert KERNEL in kern and int((fl & 0xff).max()) == 0
    check(W.cpu().numpy(), O.lienks_weights(w1, case["grid_x"], case["obs_x"], case["yb"] * EPS, case["d"], c, 1.0, EPS),
          "bundle, one shared non-prior matrix")
    G, k, stride, c = 203, 3, 4, 2.0
    case = case1d(G, k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert 0 < nb.p_max <= k
    for vname, eps, scale in (("bundle", EPS, EPS), ("transform", None, 1.0)):
        w_in = weights_in(G, k, k, eps is not None)
        W, fl, kern = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
        assert KERNEL + "<1, 1>" in kern and int((fl & 0xff).max()) == 0
        assert np.array_equal((fl >> 8) & 0xff, expected_degrees64(case["yb"], nb))
        ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s k 3 p_max %d" % (vname, nb.p_max))


# ---- 2. chain --------------------------------------------------------------------------------------------------------------------
def test_three_bundle_iterations_vs_three_oracle_iterations(eng):
    """The map from the incoming w_mean to W' is a contraction (|| D psi(S) D^T || < 1): errors do not grow along the chain, the
    bar stays 1e-10."""
    G, k, stride, c = 96, 20, 2, 6.0
    case = case1d(G, k, stride, 77)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    yb = case["yb"] * EPS
    w, ref = np.eye(k), np.eye(k)
    for it in range(3):
        W, fl, kern = upd(eng, w, yb, case["d"], nb, EPS)
        assert KERNEL in kern and int((fl & 0xff).max()) == 0
        w = W.cpu().numpy()
        ref = O.lienks_weights(ref, case["grid_x"], case["obs_x"], yb, case["d"], c, 1.0, EPS)
        check(w, ref, "bundle chain, iteration %d" % it)


# ---- 3. the transform variant past the prior ---------------------------------------------------------------------------------------
def test_transform_past_the_prior_is_the_general_kernels(eng):
    G, k, stride, c = 203, 20, 2, 9.0
    case = case1d(G, k, stride, 78)
    keep = case["obs_x"] < 150                       # (points beyond 168 see no observation)
    yb, d, ox = case["yb"][:, keep], case["d"][keep], case["obs_x"][keep]
    nb = eng.localize(case["grid_x"], ox, [c])
    has = nb.cnt.cpu().numpy() > 0
    assert 0 < int(has.sum()) < G
    w1, fl, kern = upd(eng, np.eye(k), yb, d, nb, None)
    assert KERNEL in kern and int((fl & 0xff).max()) == 0
    ref1 = O.lienks_weights(np.eye(k), case["grid_x"], ox, yb, d, c, 1.0, None)
    check(w1.cpu().numpy(), ref1, "transform, first iteration")
    # second iteration: Wp != I wherever the first one saw an observation
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.ienks_update(w1, dev(yb), dev(d), nb, 1.0, None, return_flags=True, method="tile64", defer_retry=True,
                                     out=out)
    torch.cuda.synchronize()
    assert W is out and KERNEL in last_kernel()
    fln = fl.cpu().numpy()
    assert np.array_equal((fln & RETRY) != 0, has)
    sel = torch.as_tensor(has, device=DEV)
    assert bool((out[sel] == -7.0).all())
    assert torch.equal(out[~sel], w1[~sel]) and int(fln[~has].max()) == 0         # no observation: W_in bit for bit, flag 0
    assert finish() == int(has.sum())
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & RETRY).max()) == 0                  # the redo rewrote the flags
    ref2 = O.lienks_weights(ref1, case["grid_x"], ox, yb, d, c, 1.0, None)
    check(out.cpu().numpy(), ref2, "transform, second iteration after the retry (the general kernel's bar)", tol=1e-9)
    # auto does not spend a launch that would be declined whole
    W2, fl2, kern = upd(eng, w1.cpu().numpy(), yb, d, nb, None, method="auto")
    assert KERNEL not in kern and GENERAL in kern, kern
    assert rel_fro(W2.cpu().numpy(), ref2) <= 1e-9


# ---- 4. points without observations ---------------------------------------------------------------------------------------------
def test_points_without_observations_return_their_weights_bit_for_bit(eng):
    G, k, c = 203, 20, 5.0
    case = O.synthetic_case(G, k, 2, seed=31)
    keep = (case["obs_x"] < 60) | (case["obs_x"] > 140)                     # a gap much wider than the radius
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    empty = nb.cnt.cpu().numpy() == 0
    assert empty[80:120].all() and 0 < int(empty.sum()) < G                # whole tiles and parts of tiles without any observation
    for vname, eps, scale in (("bundle", EPS, EPS), ("transform", None, 1.0)):
        w_in = weights_in(G, k, 4, eps is not None)
        W, fl, kern = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
        assert KERNEL in kern and int((fl & 0xff).max()) == 0
        sel = torch.as_tensor(empty, device=DEV)
        assert torch.equal(W[sel], dev(w_in)[sel]) and int(fl[empty].max()) == 0
        ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, observations in two parts of the domain" % vname)
    # no observation at all, a single ragged tile
    from torch_assimilate_amd.engine import NeighbourLists
    nb0 = NeighbourLists(torch.zeros(5, dtype=torch.int32, device=DEV), torch.full((5, 8), -1, dtype=torch.int32, device=DEV),
                         torch.zeros((5, 8), dtype=torch.float64, device=DEV), 8, 0, 0, 5)
    w_in = weights_in(5, k, 6, True)
    W, fl, kern = upd(eng, w_in, np.zeros((k, 0)), np.zeros(0), nb0, EPS)
    assert KERNEL in kern and torch.equal(W, dev(w_in)) and int(fl.max()) == 0


# ---- 5. declined points --------------------------------------------------------------------------------------------------------
def test_a_strong_cluster_declines_exactly_the_points_above_the_cap(eng):
    """The strong-cluster input of tests/test_gpu_weights64.py at inflation 1: before the retry exactly the points whose restated
    degree exceeds the cap carry MIA_FLAG_RETRY and are untouched; after it every point is the oracle's, and the points that were
    not declined keep their bits."""
    G, k, c = 203, 40, 10.0
    case = O.synthetic_case(G, k, 2, seed=6)
    case["yb"][:, 40:46] *= 14.0
    case["d"][40:46] *= 14.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    want = expected_degrees64(case["yb"], nb) > CAP
    assert 0 < int(want.sum()) < G
    w_in = weights_in(G, k, 8, True)
    yb = case["yb"] * EPS
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.ienks_update(dev(w_in), dev(yb), dev(case["d"]), nb, 1.0, EPS, return_flags=True, method="tile64",
                                     defer_retry=True, out=out)
    torch.cuda.synchronize()
    assert W is out and KERNEL in last_kernel()
    assert np.array_equal((fl.cpu().numpy() & RETRY) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())
    before = out.clone()
    assert finish() == int(want.sum())
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & RETRY).max()) == 0
    assert torch.equal(out[~sel], before[~sel])
    ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], yb, case["d"], c, 1.0, EPS)
    check(out.cpu().numpy(), ref, "strong cluster, %d points redone" % int(want.sum()))


# ---- 6. tile independence, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c", [(40, 2, 10.0), (64, 1, 15.0)])
def test_a_points_bits_do_not_depend_on_its_tile(eng, k, stride, c):
    G = 331
    case = case1d(G, k, stride, 21)
    w_in = weights_in(G, k, 9, True)
    yb = case["yb"] * EPS

    def run(g0, g1, w, eps, y):
        nb = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
        W, fl, kern = upd(eng, w, y, case["d"], nb, eps)
        assert KERNEL in kern and int((fl & 0xff).max()) == 0
        return W
    full = run(0, G, w_in, EPS, yb)
    assert torch.equal(full, run(0, G, w_in, EPS, yb))
    prior = run(0, G, np.eye(k), None, case["yb"])
    for g0, g1 in ((5, 200), (21, G), (103, 119), (1, 2)):
        part = run(g0, g1, w_in[g0:g1], EPS, yb)
        assert part.shape[0] == g1 - g0
        assert torch.equal(part, full[g0:g1]), (g0, g1)
        assert torch.equal(run(g0, g1, np.eye(k), None, case["yb"]), prior[g0:g1]), (g0, g1)


# ---- 7. a NaN record, an understated p_max ----------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it_and_overflow_is_loud(mia, eng):
    G, k, c = 203, 40, 10.0
    case = O.synthetic_case(G, k, 2, seed=32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    w_in = weights_in(G, k, 10, True)
    clean = upd(eng, w_in, case["yb"] * EPS, case["d"], nb, EPS)[0]
    j = 37
    bad = case["yb"] * EPS
    bad[3, j] = np.nan
    W, fl, kern = upd(eng, w_in, bad, case["d"], nb, EPS)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G and KERNEL in kern
    assert np.array_equal((fl & NONFINITE) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(W[keep], clean[keep])
    # a NeighbourLists that understates p_max: flag 1 and NaN weights on the overflowing points, the others as before
    small = mia.NeighbourLists(nb.cnt, nb.idx, nb.w, nb.p_cap, 15, nb.g0, nb.g1)
    W, fl, kern = upd(eng, w_in, case["yb"] * EPS, case["d"], small, EPS)
    over = cnt > 15
    assert 0 < over.sum() < G and KERNEL in kern
    assert np.all((fl & 0xff)[over] == OVERFLOW) and np.all((fl & 0xff)[~over] == 0)
    assert torch.isnan(W[torch.as_tensor(over, device=DEV)]).all()
    assert torch.equal(W[torch.as_tensor(~over, device=DEV)], clean[torch.as_tensor(~over, device=DEV)])


# ---- 8. through the classes --------------------------------------------------------------------------------------------------------
def test_update_state_loop_through_the_classes(mia, eng):
    """The toy loop of tests/test_gpu_ienks.py::test_update_state_loop_vs_oracle at k = 40, tau = 1, float64 end to end.  ``auto``
    takes the tile kernel from LetkfEngine.IENKS64_AUTO_MIN_K members on (bundle: every iteration; transform: the first, from
    the prior) and the general kernel below it."""
    G, k, s, c = 96, 40, 2, 6.0
    takes = k >= mia.LetkfEngine.IENKS64_AUTO_MIN_K
    rs = np.random.RandomState(21)
    state = rs.normal(size=(1, k, G))
    ox = np.arange(0, G, s, dtype=np.float64)
    y = rs.normal(size=ox.shape[0])
    var = np.full(ox.shape[0], 0.5)
    gx = np.arange(G, dtype=np.float64)

    def model_np(x):
        return 0.9 * x + 0.1 * np.roll(x, 1, axis=-1)

    def forward_model(x, it):
        nxt = 0.9 * x + 0.1 * torch.roll(x, 1, dims=-1)
        return nxt, nxt

    def observe(pseudo):
        return [pseudo[0][:, ::s]], [torch.tensor(y)], [torch.tensor(var)], None

    for vname, eps in (("bundle", EPS), ("transform", None)):
        w = np.eye(k)
        for it in range(3):
            if eps is None:
                mw = np.broadcast_to(w, (G, k, k)) if w.ndim == 2 else w
            else:
                mw = eps * np.eye(k) + (np.broadcast_to(w, (G, k, k)) if w.ndim == 2 else w).mean(axis=-1, keepdims=True)
            pseudo = model_np(O.apply_weights(state, mw))
            yb, d = O.obs_space_uncorr(pseudo[0][:, ::s], y, var)
            w = O.lienks_weights(w, gx, ox, yb, d, c, 1.0, eps)
        ref = O.apply_weights(state, w)
        cls = mia.LocalizedIEnKSTransform if eps is None else mia.LocalizedIEnKSBundle
        kw = dict(tau=1.0, dtype=torch.float64)
        if eps is not None:
            kw["epsilon"] = eps
        for max_iter in (1, 3):
            f32_first(eng)
            a = cls(forward_model, mia.GaspariCohn(c, mia.AbsoluteDistance()), max_iter=max_iter, **kw)
            xa = a.update_state_arrays(state, observe, grid_coords=gx, obs_coords=ox)
            torch.cuda.synchronize()
            on_tiles = takes and (eps is not None or max_iter == 1)
            assert (KERNEL in last_kernel()) == on_tiles, (vname, max_iter, last_kernel())
            assert on_tiles or GENERAL in last_kernel(), (vname, max_iter, last_kernel())
        assert rel_fro(xa.cpu().numpy(), ref) < 1e-8, vname
    # by name the route is there whatever the gate says
    nb = eng.localize(gx, ox, [c])
    assert upd(eng, np.eye(k), yb, d, nb, None)[2].startswith(KERNEL)


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------
def test_tile64_by_name_refuses_what_it_does_not_cover(eng):
    case = O.synthetic_case(96, 20, 2, seed=33)
    nb = eng.localize(case["grid_x"], case["obs_x"], [6.0])
    yb, d = dev(case["yb"]), dev(case["d"])
    eye = torch.eye(20, dtype=torch.float64)
    with pytest.raises(ValueError, match="float64"):
        eng.ienks_update(torch.eye(20, dtype=torch.float32), yb.float(), d.float(), nb, method="tile64")
    with pytest.raises(ValueError, match="tau"):
        eng.ienks_update(eye, yb, d, nb, tau=0.9, method="tile64")
    dense = O.synthetic_case(96, 20, 1, seed=33)
    nbd = eng.localize(dense["grid_x"], dense["obs_x"], [8.0])
    assert nbd.p_max > 20
    with pytest.raises(ValueError, match="p_max"):
        eng.ienks_update(eye, dev(dense["yb"]), dev(dense["d"]), nbd, method="tile64")
    c65 = O.synthetic_case(96, 65, 2, seed=34)
    nb65 = eng.localize(c65["grid_x"], c65["obs_x"], [10.0])
    assert 0 < nb65.p_max <= 64
    with pytest.raises(ValueError, match="k <= 64"):
        eng.ienks_update(torch.eye(65, dtype=torch.float64), dev(c65["yb"]), dev(c65["d"]), nb65, method="tile64")
    with pytest.raises(ValueError):
        eng.ienks_update(eye, yb, d, nb, method="cheb")
    # the same shapes under "auto" and "eig" are the general kernel's, as before
    f32_first(eng)
    W = eng.ienks_update(eye, dev(dense["yb"]), dev(dense["d"]), nbd)
    torch.cuda.synchronize()
    assert GENERAL in last_kernel()
    assert rel_fro(W.cpu().numpy(), O.lienks_weights(np.eye(20), dense["grid_x"], dense["obs_x"], dense["yb"], dense["d"], 8.0)) <= 1e-9
    W = eng.ienks_update(eye, yb, d, nb, method="eig")
    torch.cuda.synchronize()
    assert GENERAL in last_kernel()
    assert rel_fro(W.cpu().numpy(), O.lienks_weights(np.eye(20), case["grid_x"], case["obs_x"], case["yb"], case["d"], 6.0)) <= 1e-9

"""The float64 weights on tiles (csrc/letkf_tile64w.hip, mia_letkf_weights_matfun_f64, LetkfEngine.weights64): what
LETKF.estimate_weights_arrays and analyse_arrays(weight_save_path=...) run in the default working precision.  The contract is the
project's float64 one: relative Frobenius error <= 1e-10 on W as a whole against the golden vectors and the float64
oracle, and <= 1e-10 on the WORST SINGLE GRID POINT, || W_g - ref_g ||_F / || ref_g ||_F.  Where a test says so no point may be
declined, so that the Jacobi kernel cannot supply the parity."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
LOG_TOL, MARGIN, CAP = 26.0, 2, 127            # the float64 table's truncation target, margin and degree cap
KERNEL = "letkf_weights64_kernel"
NEW_SYMBOLS = ("mia_letkf_weights_matfun_f64", "mia_letkf_weights_retry_f64", "mia_letkf_weights_f64_cover")


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


def check(got, ref, what):
    """W [G][k][k] against the reference: the whole and the worst single grid point"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    pp = np.sqrt(((got - ref) ** 2).sum(axis=(1, 2))) / np.maximum(np.sqrt((ref ** 2).sum(axis=(1, 2))), 1e-300)
    fro = rel_fro(got, ref)
    worst = float(pp.max()) if pp.size else 0.0
    print("\n[weights64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, worst, int(pp.argmax()) if pp.size else -1))
    assert fro <= TOL64, what
    assert worst <= TOL64, what
    return fro, worst


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh (letkf_wave.hip never reports one)"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel() and "letkf_tile64" not in last_kernel()


def w64(eng, case, nb, inf, **kw):
    """engine.weights64 with its flags: (W, flags as numpy, kernel name); fails when the route refuses"""
    f32_first(eng)
    res = eng.weights64(dev(case["yb"]), dev(case["d"]), nb, inf, return_flags=True, **kw)
    assert res is not None, "weights64 refused the shape"
    torch.cuda.synchronize()
    return res[0], res[1].cpu().numpy(), last_kernel()


def expected_degrees64(yb, nb, inf):
    """Chebyshev degree per grid point as the float64 tile kernels choose it, restated in float64 numpy from the per-point
    lists: Gershgorin bound L of S = D G D, T = L / reg rounded up to the table's geometric grid (32 per octave,
    2^-24 .. 2^8), degree = ceil(26 / log rho) + 2, rho = (sqrt(1 + T) + 1) / (sqrt(1 + T) - 1)"""
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


@functools.lru_cache(maxsize=None)
def case1d(G, k, stride, seed):
    return O.synthetic_case(G, k, stride, seed=seed)


@functools.lru_cache(maxsize=None)
def oracle1d(G, k, stride, seed, c, inf):
    """the oracle's weights of a 1-D case, computed once and shared (treat as read-only)"""
    case = case1d(G, k, stride, seed)
    W = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, inf)[1]
    W.setflags(write=False)
    return W


# ---- 1. symbols ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve(mia):
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS
    assert lib.mia_letkf_weights_f64_cover(40, 20, 100000, 50000) == 1
    assert lib.mia_letkf_weights_f64_cover(65, 20, 1000, 10) == 0
    assert lib.mia_letkf_weights_f64_cover(20, 21, 1000, 10) == 0
    # argument validation precedes any device work, in the order of mia_letkf_analysis_matfun_f64
    call = lib.mia_letkf_weights_matfun_f64
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, -1.0, 0.0, None, 10, 0, None, None, None, None) == -2
    assert call(None, 10, 1, 4, 0, 0, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0, None, None, None, None) == 0
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.5, None, 10, 0, None, None, None, None) == -3
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0, None, None, None, None) == -1
    assert lib.mia_letkf_weights_retry_f64(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0, None,
                                           None, None) == -1


# ---- 2. golden vectors -----------------------------------------------------------------------------------------------------------
def test_config2_golden_weights_and_the_analysis_they_give(eng, golden):
    """g7 config 2, all 256 points, both inflations: the reference-generated weights at c2_widx, every point against the oracle,
    computed by the new kernel; applied to the state they give the matfun64 analysis."""
    g = golden("g7_synthetic_configs.npz")
    case = dict(state=g["c2_state"], grid_x=g["c2_grid_x"], obs_x=g["c2_obs_x"], yb=g["c2_yb"], d=g["c2_d"])
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    for inf, tag in ((1.0, "1p0"), (1.1, "1p1")):
        W, fl, kern = w64(eng, case, nb, inf)
        assert KERNEL + "<2, 3>" in kern, kern
        assert int((fl & 0xff).max()) == 0
        check(W.cpu().numpy()[g["c2_widx"]], g["c2_%s_weights" % tag], "golden c2 weights inf %s" % inf)
        ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, inf)[1]
        check(W.cpu().numpy(), ref, "c2 every point vs oracle inf %s" % inf)
        xw = eng.apply_local_weights(dev(case["state"]), W)
        xm = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, inf, method="matfun64")
        torch.cuda.synchronize()
        assert "letkf_tile64" in last_kernel()
        assert rel_fro(xw.cpu().numpy(), xm.cpu().numpy()) <= TOL64
        assert rel_fro(xw.cpu().numpy(), g["c2_%s_analysis" % tag]) <= TOL64


# ---- 3. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
SWEEP = [(8, 4, 7.0), (8, 2, 4.0), (8, 1, 2.0), (20, 4, 18.0), (20, 2, 9.0), (20, 1, 4.5), (27, 4, 24.0), (27, 2, 12.0),
         (27, 1, 6.0), (40, 4, 36.0), (40, 2, 18.0), (40, 1, 9.0), (64, 4, 50.0), (64, 2, 28.0), (64, 1, 15.0)]


@pytest.mark.parametrize("k,stride,c", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, stride, c):
    """k x network density with p_max <= k (UT 1 .. 4, KT 1 .. 4, k no multiple of 4, tiles in halves), ragged last tile
    (G = 203), both inflations.  The degrees are the restated rule's, none above the cap: no point is declined."""
    G = 203
    case = case1d(G, k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert 0 < nb.p_max <= k
    for inf in (1.0, 1.1):
        want = expected_degrees64(case["yb"], nb, inf)
        assert int(want.max()) <= CAP
        W, fl, kern = w64(eng, case, nb, inf)
        assert KERNEL in kern, kern
        assert int((fl & 0xff).max()) == 0                                  # nothing declined, nothing non-finite
        assert np.array_equal((fl >> 8) & 0xff, want)
        check(W.cpu().numpy(), oracle1d(G, k, stride, k + 1, c, inf), "k %d stride %d c %g inf %g p_max %d (%s)" % (k, stride, c, inf, nb.p_max, kern))


# ---- 4. 2-D mesh: unions beyond the instantiation's slots -------------------------------------------------------------------------
def mesh_case(nx, ny, k, stride, seed):
    rnd = np.random.RandomState(seed)
    gy, gx = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    sel = ((grid[:, 0] % stride) == 0) & ((grid[:, 1] % stride) == 0)
    state = rnd.normal(size=(1, k, grid.shape[0]))
    y = rnd.normal(size=int(sel.sum()))
    yb, d = O.obs_space_uncorr(state[0][:, sel], y, np.ones_like(y))
    return dict(state=state, grid=grid, obs=grid[sel], yb=yb, d=d)


def test_mesh_2d_tiles_in_halves(eng):
    case = mesh_case(26, 18, 40, 2, seed=7)
    nb = eng.localize(case["grid"], case["obs"], [2.5])
    assert 8 <= nb.p_max <= 40
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    unions = [len(set(np.concatenate([idx[g, :cnt[g]] for g in range(t, min(t + 16, len(cnt)))]))) for t in range(0, len(cnt), 16)]
    slots = 16 * min(4, max(1, (nb.p_max + 8 + 15) // 16))
    assert max(unions) > slots
    f32_first(eng)
    W, fl, kern = w64(eng, case, nb, 1.1)
    assert KERNEL in kern and int((fl & 0xff).max()) == 0
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], 2.5, 1.1)[1]
    check(W.cpu().numpy(), ref, "2-D mesh, p_max %d, largest union %d of %d slots (%s)" % (nb.p_max, max(unions), slots, kern))


# ---- 5. through the classes in the default dtype: every localisation ---------------------------------------------------------------
def test_classes_take_the_kernel_with_every_localisation(mia, eng):
    """Two radius groups, GaspariCohnInf, PeriodicMetric and a Python dist_func through LETKF(...).estimate_weights_arrays
    without a dtype: the route works from the per-point lists, whatever made them.  k = 40: the classes hand over from
    LetkfEngine.WEIGHTS64_AUTO_MIN_K members on (the measured factor 2); smaller ensembles are the sweep's, by weights64."""
    case = mesh_case(20, 6, 40, 2, seed=9)
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn((3.0, 1.5), mia.EuclideanMetric([0, 1])), inf_factor=1.1)
    W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid"], obs_coords=case["obs"])
    assert W.dtype == torch.float64 and KERNEL in last_kernel(), last_kernel()
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], [3.0, 1.5], 1.1, coord_group=[0, 1])[1]
    check(W.cpu().numpy(), ref, "two radius groups")

    c1 = O.synthetic_case(150, 40, 2, seed=11)
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohnInf(9.0, mia.AbsoluteDistance()), inf_factor=1.0)
    W = f.estimate_weights_arrays(c1["yb"], c1["d"], grid_coords=c1["grid_x"], obs_coords=c1["obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    ref = O.letkf_analysis(c1["state"], c1["grid_x"], c1["obs_x"], c1["yb"], c1["d"], 9.0, 1.0, taper="gc_inf")[1]
    check(W.cpu().numpy(), ref, "GaspariCohnInf")

    G, L, c = 203, 203.0, 6.0                      # (G is not a multiple of 16: the last tile ends at the seam)
    case = O.synthetic_case(G, 40, 2, seed=41)

    def ring(g, o):
        dd = np.abs(np.asarray(o, dtype=np.float64).reshape(-1) - float(np.asarray(g).reshape(-1)[0]))
        return np.minimum(dd, L - dd)
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.1, dist_func=ring)[1]
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(c, dist_func=mia.PeriodicMetric(L)), inf_factor=1.1)
    W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    check(W.cpu().numpy(), ref, "PeriodicMetric ring")
    f32_first(eng)
    user = mia.GaspariCohn(c, lambda grid, obs: ring(grid, obs))
    W = mia.LETKF(localization=user, inf_factor=1.1).estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid_x"],
                                                                             obs_coords=case["obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    check(W.cpu().numpy(), ref, "python dist_func")


# ---- 6. declined points --------------------------------------------------------------------------------------------------------
def test_a_strong_cluster_declines_exactly_the_points_above_the_cap(eng):
    """One strong cluster in an otherwise unit-variance network: before the retry exactly the points whose restated degree
    exceeds the cap carry MIA_FLAG_RETRY and are untouched in W; after it every point is the oracle's, and the points that were
    not declined keep their bits."""
    G = 203
    case = O.synthetic_case(G, 40, 2, seed=6)
    case["yb"][:, 40:46] *= 14.0
    case["d"][40:46] *= 14.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    want = expected_degrees64(case["yb"], nb, 1.1) > CAP
    assert 0 < int(want.sum()) < G
    out = torch.full((G, 40, 40), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.weights64(dev(case["yb"]), dev(case["d"]), nb, 1.1, out=out, return_flags=True, defer_retry=True)
    torch.cuda.synchronize()
    assert W is out and KERNEL in last_kernel()
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())
    before = out.clone()
    assert finish() == int(want.sum())
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & 8).max()) == 0                      # the redo rewrote the flags
    assert torch.equal(out[~sel], before[~sel])
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, 1.1)[1]
    check(out.cpu().numpy(), ref, "strong cluster, %d points redone" % int(want.sum()))


# ---- 7. tile independence, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c", [(40, 2, 10.0), (20, 1, 4.5), (64, 1, 15.0)])
def test_a_points_bits_do_not_depend_on_its_tile(eng, k, stride, c):
    G = 331
    case = case1d(G, k, stride, 21)
    full, fl, kern = w64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c]), 1.1)
    assert int((fl & 0xff).max()) == 0 and KERNEL in kern
    again = w64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c]), 1.1)[0]
    assert torch.equal(full, again)
    for g0, g1 in ((5, 200), (21, G), (37, 150), (103, 119), (1, 2)):
        part = w64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1), 1.1)[0]
        assert part.shape[0] == g1 - g0
        assert torch.equal(part, full[g0:g1]), (g0, g1)


# ---- 8. points without observations --------------------------------------------------------------------------------------------
def test_points_without_observations_get_sqrt_inf_identity(eng):
    case = O.synthetic_case(203, 20, 2, seed=31)
    keep = case["obs_x"] < 60
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    W, fl, kern = w64(eng, case, nb, 1.1)
    assert KERNEL in kern and int((fl & 0xff).max()) == 0
    far = W.cpu().numpy()[80:]                                          # (whole tiles and parts of tiles without any observation)
    assert np.abs(far - np.sqrt(1.1) * np.eye(20)).max() <= 1e-14
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 5.0, 1.1)[1]
    check(W.cpu().numpy(), ref, "observations in a part of the domain")
    # no observation at all, a single ragged tile
    from torch_assimilate_amd.engine import NeighbourLists
    none = dict(yb=np.zeros((20, 0)), d=np.zeros(0))
    nb = NeighbourLists(torch.zeros(5, dtype=torch.int32, device=DEV), torch.full((5, 8), -1, dtype=torch.int32, device=DEV),
                        torch.zeros((5, 8), dtype=torch.float64, device=DEV), 8, 0, 0, 5)
    W, fl, kern = w64(eng, none, nb, 1.1)
    assert KERNEL in kern and W.shape == (5, 20, 20) and int((fl & 0xff).max()) == 0
    assert np.abs(W.cpu().numpy() - np.sqrt(1.1) * np.eye(20)).max() <= 1e-14


# ---- 9. a NaN record ------------------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    case = O.synthetic_case(203, 40, 2, seed=32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    clean = w64(eng, case, nb, 1.1)[0]
    j = 37
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][3, j] = np.nan
    W, fl, kern = w64(eng, bad, nb, 1.1)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(203)])
    assert 0 < uses.sum() < 203 and KERNEL in kern
    assert np.array_equal((fl & 4) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(W[keep], clean[keep])


# ---- 10. outside the route ------------------------------------------------------------------------------------------------------
def entry_rc(eng, case, nb, k, inf=1.1, gamma=0.0):
    """mia_letkf_weights_matfun_f64 itself on float64 copies of the case: its return code"""
    from torch_assimilate_amd import _cabi
    n = nb.g1 - nb.g0
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    W = torch.empty((n, k, k), dtype=torch.float64, device=DEV)
    fl = torch.zeros(n, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_letkf_weights_matfun_f64(None, nb.g1, 1, k, nb.g0, nb.g1, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                                  nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, inf, gamma, None, n, 0,
                                                  W.data_ptr(), fl.data_ptr(), retry.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


def test_shapes_outside_the_route_take_the_jacobi_kernel(mia, eng):
    """p_max > k, k = 65, float32 input, the RBF core and option tile = 0: the entry answers MIA_ERR_UNSUPPORTED (-3) and
    weights64 returns None -- float32 input is refused by weights64 itself, a C entry cannot see a dtype -- and the class
    still returns the oracle's weights, from the Jacobi kernel."""
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    loc = lambda c: mia.GaspariCohn(c, mia.AbsoluteDistance())      # noqa: E731

    def by_class(case, c, filt=None):
        f32_first(eng)
        f = filt or mia.LETKF(localization=loc(c), inf_factor=1.1)
        W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
        assert W.dtype == torch.float64 and KERNEL not in last_kernel() and "letkf_tile64" not in last_kernel()
        return W.cpu().numpy()
    # p_max > k
    case = O.synthetic_case(100, 20, 1, seed=33)
    nb = eng.localize(case["grid_x"], case["obs_x"], [8.0])
    assert nb.p_max > 20 and lib.mia_letkf_weights_f64_cover(20, nb.p_max, 100, 100) == 0
    assert entry_rc(eng, case, nb, 20) == -3
    assert eng.weights64(dev(case["yb"]), dev(case["d"]), nb, 1.1) is None
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 8.0, 1.1)[1]
    check(by_class(case, 8.0), ref, "p_max > k through the class")
    # k = 65
    c65 = O.synthetic_case(96, 65, 2, seed=34)
    nb65 = eng.localize(c65["grid_x"], c65["obs_x"], [10.0])
    assert 0 < nb65.p_max <= 64
    assert entry_rc(eng, c65, nb65, 65) == -3
    assert eng.weights64(dev(c65["yb"]), dev(c65["d"]), nb65, 1.1) is None
    ref = O.letkf_analysis(c65["state"], c65["grid_x"], c65["obs_x"], c65["yb"], c65["d"], 10.0, 1.1)[1]
    check(by_class(c65, 10.0), ref, "k = 65 through the class")
    # inside the route from here on: config 2's shape
    c2 = O.synthetic_case(203, 40, 2, seed=35)
    nb2 = eng.localize(c2["grid_x"], c2["obs_x"], [10.0])
    ref2 = O.letkf_analysis(c2["state"], c2["grid_x"], c2["obs_x"], c2["yb"], c2["d"], 10.0, 1.1)[1]
    assert entry_rc(eng, c2, nb2, 40) == 0
    # float32 input
    assert eng.weights64(dev(c2["yb"], torch.float32), dev(c2["d"], torch.float32), nb2, 1.1) is None
    # the RBF core
    assert entry_rc(eng, c2, nb2, 40, gamma=0.5) == -3
    assert eng.weights64(dev(c2["yb"]), dev(c2["d"]), nb2, 1.1, rbf_gamma=0.5) is None
    core = lambda a, b, i: O.ketkf_weights(a, b, lambda x, y: O.rbf_kernel(x, y, 0.5), i)      # noqa: E731
    refk = O.letkf_analysis(c2["state"], c2["grid_x"], c2["obs_x"], c2["yb"], c2["d"], 10.0, 1.1, core=core)[1]
    check(by_class(c2, 10.0, mia.LKETKF(mia.RBFKernel(0.5), localization=loc(10.0), inf_factor=1.1)), refk, "RBF core through the class")
    # engine.analysis keeps the weights on the Jacobi kernel
    f32_first(eng)
    _, We = eng.analysis(dev(c2["state"]), dev(c2["yb"]), dev(c2["d"]), nb2, 1.1, return_weights=True)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel() and "letkf_tile64" not in last_kernel()
    check(We.cpu().numpy(), ref2, "engine.analysis(return_weights=True)")
    # option tile = 0
    set_option("tile", 0)
    assert entry_rc(eng, c2, nb2, 40) == -3
    assert eng.weights64(dev(c2["yb"]), dev(c2["d"]), nb2, 1.1) is None
    check(by_class(c2, 10.0), ref2, "tile = 0 through the class")


# ---- 11. weight_save_path ---------------------------------------------------------------------------------------------------------
def test_weight_save_path_in_the_default_dtype(mia, eng, golden, tmp_path):
    """filter.py:157-164 with a weight_save_path at config 2's golden size, no dtype argument: the file holds the golden weights,
    the analysis is the golden analysis, and the weights came from the new kernel."""
    from torch_assimilate_amd import weights_io as io
    g = golden("g7_synthetic_configs.npz")
    path = str(tmp_path / "w.nc")
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(10.0, mia.AbsoluteDistance()), inf_factor=1.1, weight_save_path=path)
    xa = f.analyse_arrays(g["c2_state"], g["c2_yb"], g["c2_d"], grid_coords=g["c2_grid_x"], obs_coords=g["c2_obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    assert xa.dtype == torch.float64 and rel_fro(xa.cpu().numpy(), g["c2_1p1_analysis"]) <= TOL64
    W, coords = io.load_weights(path)
    assert tuple(W.shape) == (256, 40, 40) and coords["grid"].tolist() == list(range(256))
    check(W.numpy()[g["c2_widx"]], g["c2_1p1_weights"], "weights file vs golden")


# ---- 12. the classes' hand-over rule, and a refused shape at a size the classes do hand over ---------------------------------------
def test_the_class_hands_over_from_the_gate_on_and_falls_through_where_the_entry_refuses(mia, eng):
    """LETKF(...).estimate_weights_arrays in the default dtype takes the kernel at k = WEIGHTS64_AUTO_MIN_K and not one member
    below (the measured factor 2); at that size a list longer than the ensemble makes weights64 answer None and the
    class falls through to the Jacobi kernel.  The oracle's weights in every case."""
    kmin = mia.LetkfEngine.WEIGHTS64_AUTO_MIN_K
    assert kmin == 40
    for k, takes in ((kmin, True), (kmin - 1, False)):
        case = O.synthetic_case(203, k, 2, seed=51)
        f32_first(eng)
        f = mia.LETKF(localization=mia.GaspariCohn(10.0, mia.AbsoluteDistance()), inf_factor=1.1)
        W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
        assert (KERNEL in last_kernel()) == takes, (k, last_kernel())
        ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, 1.1)[1]
        check(W.cpu().numpy(), ref, "class at k = %d (%s)" % (k, "weights64" if takes else "Jacobi kernel"))
        nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
        assert w64(eng, case, nb, 1.1)[2].startswith(KERNEL)              # the engine method itself has no gate
    case = O.synthetic_case(120, kmin, 1, seed=52)
    nb = eng.localize(case["grid_x"], case["obs_x"], [12.0])
    assert nb.p_max > kmin
    assert eng.weights64(dev(case["yb"]), dev(case["d"]), nb, 1.1) is None
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(12.0, mia.AbsoluteDistance()), inf_factor=1.1)
    W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    assert KERNEL not in last_kernel() and "letkf_tile64" not in last_kernel()
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 12.0, 1.1)[1]
    check(W.cpu().numpy(), ref, "k = %d, p_max %d > k through the class" % (kmin, nb.p_max))


# ---- 13. the redo of declined points on a sub-range ----------------------------------------------------------------------------------
def test_retry_on_a_sub_range(eng):
    """The strong cluster of test 6 on grid points [21, 150): the lists, the flags and W count from g0, the one-row zero state of
    the redo from 0.  The undeferred call: declined points are redone inside weights64."""
    G, g0, g1 = 203, 21, 150
    case = O.synthetic_case(G, 40, 2, seed=6)
    case["yb"][:, 40:46] *= 14.0
    case["d"][40:46] *= 14.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0], g0=g0, g1=g1)
    want = expected_degrees64(case["yb"], nb, 1.1) > CAP
    assert 0 < int(want.sum()) < g1 - g0
    W, fl, kern = w64(eng, case, nb, 1.1)
    assert KERNEL in kern and W.shape[0] == g1 - g0 and int((fl & 8).max()) == 0
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, 1.1)[1]
    check(W.cpu().numpy(), ref[g0:g1], "sub-range [%d, %d), %d points redone" % (g0, g1, int(want.sum())))

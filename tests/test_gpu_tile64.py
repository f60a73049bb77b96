"""The float64 tile route (csrc/letkf_tile64.hip, mia_letkf_analysis_matfun_f64): what LETKF(...) runs in its default working
precision.  The contract is the project's float64 one: relative Frobenius error <= 1e-10 against the golden vectors and
the float64 oracle -- and here also the WORST SINGLE GRID POINT <= 1e-10.  In the shape sweep no point may be declined, so that the
Jacobi kernel cannot supply the parity."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
LOG_TOL, MARGIN, CAP = 26.0, 2, 127            # the float64 table's truncation target, margin and degree cap


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


def per_point(got, ref):
    """relative error of every grid point's (m, k) block, and the relative Frobenius error of the whole"""
    from oracle_pool import per_point_errors
    return per_point_errors(got, ref)


def check(got, ref, what):
    pp, fro = per_point(got, ref)
    print("\n[tile64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= TOL64, what
    assert pp.max() <= TOL64, what
    return fro, float(pp.max())


def run64(eng, case, nb, inf, method="auto", **kw):
    """engine.analysis in float64 with a caller-owned decline counter: (Xa, flags, declined, kernel name)"""
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xa, fl = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, inf, return_flags=True, method=method,
                          retry=retry, **kw)
    torch.cuda.synchronize()
    return xa, fl, int(retry.item()), last_kernel()


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh (letkf_wave.hip never reports one)"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert "letkf_tile64" not in last_kernel()


def expected_degrees64(yb, nb, inf):
    """Chebyshev degree per grid point as letkf_tile64_kernel chooses it, restated in float64 numpy from the per-point lists:
    Gershgorin bound L of S = D G D, T = L / reg rounded up to the table's geometric grid (32 per octave, 2^-24 .. 2^8),
    degree = ceil(26 / log rho) + 2, rho = (sqrt(1 + T) + 1) / (sqrt(1 + T) - 1)"""
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


# ---- 1. the default call ------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve(mia):
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    for name in ("mia_letkf_analysis_matfun_f64", "mia_letkf_analysis_retry_f64", "mia_letkf_matfun_f64_cover"):
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS
    assert lib.mia_letkf_matfun_f64_cover(1, 40, 20, 100000, 100000, 100000, 50000) == 1
    assert lib.mia_letkf_matfun_f64_cover(3, 64, 64, 1000, 1000, 1000, 10) == 1
    assert lib.mia_letkf_matfun_f64_cover(1, 65, 20, 1000, 1000, 1000, 10) == 0        # ensemble size
    assert lib.mia_letkf_matfun_f64_cover(1, 20, 21, 1000, 1000, 1000, 10) == 0        # primal route
    # argument validation precedes any device work
    assert lib.mia_letkf_analysis_matfun_f64(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, -1.0, 0.0, None, 10, 0,
                                             None, None, None) == -2
    assert lib.mia_letkf_analysis_matfun_f64(None, 10, 1, 4, 0, 0, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0,
                                             None, None, None) == 0
    assert lib.mia_letkf_analysis_matfun_f64(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.5, None, 10, 0,
                                             None, None, None) == -3                    # gamma > 0
    assert lib.mia_letkf_analysis_matfun_f64(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0,
                                             None, None, None) == -1
    assert lib.mia_letkf_analysis_retry_f64(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0,
                                            None, None) == -1


@pytest.mark.parametrize("name", ["c2", "c2m3"])
def test_default_dtype_runs_the_tile64_kernel_vs_golden(mia, eng, golden, name):
    """LETKF(localization, inf_factor) exactly as with the reference -- no dtype argument -- on the reference-generated g7
    configurations: the golden analysis to 1e-10 (whole and worst grid point), computed by letkf_tile64_kernel."""
    g = golden("g7_synthetic_configs.npz")
    for inf, tag in ((1.0, "1p0"), (1.1, "1p1")):
        f32_first(eng)
        f = mia.LETKF(localization=mia.GaspariCohn(10.0, mia.AbsoluteDistance()), inf_factor=inf)
        xa = f.analyse_arrays(g[name + "_state"], g[name + "_yb"], g[name + "_d"], grid_coords=g[name + "_grid_x"],
                              obs_coords=g[name + "_obs_x"])
        assert xa.dtype == torch.float64
        assert "letkf_tile64" in last_kernel(), last_kernel()
        check(xa.cpu().numpy(), g["%s_%s_analysis" % (name, tag)], "golden %s inf %s" % (name, inf))


# ---- 2. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
SWEEP = [(8, 4, 7.0), (8, 2, 4.0), (8, 1, 2.0), (20, 4, 18.0), (20, 2, 9.0), (20, 1, 4.5), (27, 4, 24.0), (27, 2, 12.0),
         (27, 1, 6.0), (40, 4, 36.0), (40, 2, 18.0), (40, 1, 9.0), (64, 4, 50.0), (64, 2, 28.0), (64, 1, 15.0)]


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k,stride,c", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, stride, c, m):
    """k x network density with the radius chosen so that p_max <= k (unions of 1 .. 4 sixteen-slot blocks, tiles in halves
    where sixteen points of a dense network see more than the instantiation holds), ragged last tile (G = 203), one and
    several state rows, both inflations.  random points: the UT = 1 instantiations are among them."""
    case = O.synthetic_case(203, k, stride, seed=k + m, m=m)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert 0 < nb.p_max <= k
    for inf in (1.0, 1.1):
        f32_first(eng)
        xa, fl, declined, kern = run64(eng, case, nb, inf)
        assert "letkf_tile64" in kern, kern
        assert declined == 0
        fl = fl.cpu().numpy()
        assert int((fl & 0xff).max()) == 0
        assert np.array_equal((fl >> 8) & 0xff, expected_degrees64(case["yb"], nb, inf))
        ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, inf)[0]
        check(xa.cpu().numpy(), ref, "k %d stride %d c %g m %d inf %g p_max %d (%s)" % (k, stride, c, m, inf, nb.p_max, kern))


def mesh_case(nx, ny, k, stride, seed, m=1):
    rnd = np.random.RandomState(seed)
    gy, gx = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    sel = ((grid[:, 0] % stride) == 0) & ((grid[:, 1] % stride) == 0)
    state = rnd.normal(size=(m, k, grid.shape[0]))
    y = rnd.normal(size=int(sel.sum()))
    yb, d = O.obs_space_uncorr(state[0][:, sel], y, np.ones_like(y))
    return dict(state=state, grid=grid, obs=grid[sel], yb=yb, d=d)


def test_mesh_2d_unions_above_32_slots(eng):
    """A 2-D mesh in row-major order, Euclidean distance: sixteen consecutive points see far more observations than one does,
    the unions exceed the slots of the instantiation and the tiles are analysed in parts."""
    case = mesh_case(26, 18, 40, 2, seed=7)
    nb = eng.localize(case["grid"], case["obs"], [2.5])
    assert 8 <= nb.p_max <= 40
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    unions = [len(set(np.concatenate([idx[g, :cnt[g]] for g in range(t, min(t + 16, len(cnt)))]))) for t in range(0, len(cnt), 16)]
    assert max(unions) > 32
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert "letkf_tile64" in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], 2.5, 1.1)[0]
    check(xa.cpu().numpy(), ref, "2-D mesh, p_max %d, largest union %d (%s)" % (nb.p_max, max(unions), kern))


def test_two_radius_groups_gc_inf_and_small_grids(eng):
    """Two radius groups (horizontal x vertical), GaspariCohnInf, and G < 16 (one ragged tile)."""
    case = mesh_case(20, 6, 27, 2, seed=9, m=2)
    nb = eng.localize(case["grid"], case["obs"], [3.0, 1.5], coord_group=[0, 1])
    assert 0 < nb.p_max <= 27
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert "letkf_tile64" in kern and declined == 0
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], [3.0, 1.5], 1.1, coord_group=[0, 1])[0]
    check(xa.cpu().numpy(), ref, "two radius groups")
    c1 = O.synthetic_case(150, 20, 2, seed=11)
    nb = eng.localize(c1["grid_x"], c1["obs_x"], [9.0], taper=1)
    assert 0 < nb.p_max <= 20
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, c1, nb, 1.0)
    assert "letkf_tile64" in kern and declined == 0
    ref = O.letkf_analysis(c1["state"], c1["grid_x"], c1["obs_x"], c1["yb"], c1["d"], 9.0, 1.0, taper="gc_inf")[0]
    check(xa.cpu().numpy(), ref, "GaspariCohnInf")
    c2 = O.synthetic_case(11, 20, 1, seed=12, m=2)
    nb = eng.localize(c2["grid_x"], c2["obs_x"], [3.0])
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, c2, nb, 1.1)
    assert "letkf_tile64" in kern and declined == 0
    ref = O.letkf_analysis(c2["state"], c2["grid_x"], c2["obs_x"], c2["yb"], c2["d"], 3.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "G = 11")


# ---- 3. declined points are redone ---------------------------------------------------------------------------------------------
def test_strong_observations_are_declined_and_redone(eng):
    """The C2 recipe with yb, d scaled x10 (spectra x100: a-priori degree far above the cap): EVERY point is flagged and
    counted, and the Jacobi kernel's redo gives the oracle's analysis of the scaled inputs."""
    G = 203
    case = O.synthetic_case(G, 40, 2, seed=5)
    case["yb"], case["d"] = case["yb"] * 10.0, case["d"] * 10.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    assert int(expected_degrees64(case["yb"], nb, 1.1).min()) > CAP
    # the C entry alone: flags and count, Xa untouched
    from torch_assimilate_amd import _cabi
    X = dev(case["state"])
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    out = torch.full((1, 40, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_letkf_analysis_matfun_f64(X.data_ptr(), G, 1, 40, 0, G, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                                   nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, 1.1, 0.0, out.data_ptr(),
                                                   G, 0, fl.data_ptr(), retry.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(retry.item()) == G
    assert bool((fl == 8).all()) and bool((out == -7.0).all())
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert declined == G and "letkf_tile64" in kern           # (the redo does not overwrite the reported kernel)
    assert int((fl.cpu().numpy() & 8).max()) == 0             # the redo rewrote the flags
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "x10 observations, all %d points redone" % G)


def test_a_strong_cluster_declines_exactly_the_points_above_the_cap(eng):
    """One strong cluster in an otherwise unit-variance network: the flagged set equals "degree from the table for this point's
    Gershgorin bound > cap", restated in float64 numpy."""
    G = 203
    case = O.synthetic_case(G, 40, 2, seed=6)
    case["yb"][:, 40:46] *= 14.0
    case["d"][40:46] *= 14.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    want = expected_degrees64(case["yb"], nb, 1.1) > CAP
    assert 0 < int(want.sum()) < G
    X = dev(case["state"])
    out = torch.full((1, 40, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = eng.analysis(X, dev(case["yb"]), dev(case["d"]), nb, 1.1, out=out, flags=fl, retry=retry, defer_retry=True)
    torch.cuda.synchronize()
    got = (fl.cpu().numpy() & 8) != 0
    assert np.array_equal(got, want)
    assert int(retry.item()) == int(want.sum())
    assert bool((out[:, :, torch.as_tensor(want, device=DEV)] == -7.0).all())       # declined points are left untouched
    assert res[-1]() == int(want.sum())                                            # the deferred redo
    torch.cuda.synchronize()
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, 1.1)[0]
    check(out.cpu().numpy(), ref, "strong cluster, %d points redone" % int(want.sum()))


# ---- 4. tile independence, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c", [(40, 2, 10.0), (20, 1, 4.5), (64, 1, 15.0)])
def test_a_points_bits_do_not_depend_on_its_tile(eng, k, stride, c):
    G = 331
    case = O.synthetic_case(G, k, stride, seed=21, m=2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    full, _, declined, kern = run64(eng, case, nb, 1.1)
    assert declined == 0 and "letkf_tile64" in kern
    again = run64(eng, case, nb, 1.1)[0]
    assert torch.equal(full, again)
    for g0, g1 in ((5, 200), (21, G), (37, 150), (103, 119), (1, 2)):
        part = run64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1), 1.1)[0]
        assert part.shape[-1] == g1 - g0
        assert torch.equal(part, full[:, :, g0:g1]), (g0, g1)


def test_observation_order(eng):
    """A permutation of the observations changes the ranks inside a union, i.e. the summation order -- rounding only.  Observed
    figures are printed for both kernels; the bound is float64 rounding through a recurrence of at most 127 steps over at most
    64 terms (1e-16 x 64 x 127 < 1e-12), two orders below the contract."""
    case = O.synthetic_case(331, 40, 2, seed=22)
    perm = np.random.RandomState(1).permutation(case["obs_x"].shape[0])
    pc = dict(case, obs_x=case["obs_x"][perm], yb=case["yb"][:, perm], d=case["d"][perm])
    out = {}
    for method in ("auto", "eig"):
        a = run64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [10.0]), 1.1, method=method)[0]
        b = run64(eng, pc, eng.localize(pc["grid_x"], pc["obs_x"], [10.0]), 1.1, method=method)[0]
        out[method] = float(torch.linalg.norm(a - b) / torch.linalg.norm(a))
    print("\n[tile64] permuted observations: rel. change %.3e (tile64), %.3e (Jacobi kernel)" % (out["auto"], out["eig"]))
    assert out["auto"] <= 1e-12


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------
def test_points_without_observations_get_the_inflated_prior(eng):
    case = O.synthetic_case(203, 20, 2, seed=31, m=2)
    keep = case["obs_x"] < 60
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert "letkf_tile64" in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
    far = slice(80, 203)                                             # (whole tiles and parts of tiles without any observation)
    st = case["state"][:, :, far]
    mean = st.mean(axis=1, keepdims=True)
    assert rel_fro(xa.cpu().numpy()[:, :, far], mean + np.sqrt(1.1) * (st - mean)) <= 1e-14
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 5.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "observations in a part of the domain")


def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    case = O.synthetic_case(203, 40, 2, seed=32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    clean = run64(eng, case, nb, 1.1)[0]
    j = 37
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][3, j] = np.nan
    xa, fl, declined, kern = run64(eng, bad, nb, 1.1)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(203)])
    assert 0 < uses.sum() < 203
    assert np.array_equal((fl.cpu().numpy() & 4) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(xa[:, :, keep], clean[:, :, keep])


def test_shapes_outside_the_route_take_the_jacobi_kernel(eng):
    """p_max > k (primal route): MIA_ERR_UNSUPPORTED from the C entry before any launch, the right answer from engine.analysis."""
    from torch_assimilate_amd import _cabi
    G = 100
    case = O.synthetic_case(G, 20, 1, seed=33)
    nb = eng.localize(case["grid_x"], case["obs_x"], [8.0])
    assert nb.p_max > 20
    lib = _cabi.lib()
    assert lib.mia_letkf_matfun_f64_cover(1, 20, nb.p_max, G, G, G, G) == 0
    X = dev(case["state"])
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    out = torch.empty((1, 20, G), dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    f32_first(eng)
    rc = lib.mia_letkf_analysis_matfun_f64(X.data_ptr(), G, 1, 20, 0, G, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                           nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, 1.1, 0.0, out.data_ptr(), G, 0,
                                           fl.data_ptr(), retry.data_ptr(), None)
    assert rc == -3
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert "letkf_tile64" not in kern and declined == 0
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 8.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "primal route through engine.analysis")
    with pytest.raises(Exception):
        run64(eng, case, nb, 1.1, method="matfun64")


def test_tile_option_eig_method_and_output_offset(eng):
    case = O.synthetic_case(203, 40, 2, seed=34, m=2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, 1.1)[0]
    xa, _, declined, kern = run64(eng, case, nb, 1.1)
    assert "letkf_tile64" in kern and declined == 0
    check(xa.cpu().numpy(), ref, "auto")
    x64, _, _, kern = run64(eng, case, nb, 1.1, method="matfun64")
    assert "letkf_tile64" in kern and torch.equal(x64, xa)
    # method="eig" stays the Jacobi kernel
    f32_first(eng)
    xe, _, _, kern = run64(eng, case, nb, 1.1, method="eig")
    assert "letkf_tile64" not in kern
    check(xe.cpu().numpy(), ref, "eig")
    # tile = 0 turns the route off, as it turns the float32 tile route off
    set_option("tile", 0)
    f32_first(eng)
    xo, _, _, kern = run64(eng, case, nb, 1.1)
    assert "letkf_tile64" not in kern
    check(xo.cpu().numpy(), ref, "tile = 0")
    assert torch.equal(xo, xe)
    set_option("tile", 1)
    # out= with a column offset, a sub-range of the grid
    g0, g1 = 21, 150
    nbs = eng.localize(case["grid_x"], case["obs_x"], [10.0], g0=g0, g1=g1)
    out = torch.full((2, 40, g1 - g0 + 9), -7.0, dtype=torch.float64, device=DEV)
    res = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nbs, 1.1, out=out, out_offset=5)
    torch.cuda.synchronize()
    assert res is out and "letkf_tile64" in last_kernel()
    assert torch.equal(out[:, :, 5:5 + g1 - g0], xa[:, :, g0:g1])
    assert bool((out[:, :, :5] == -7.0).all()) and bool((out[:, :, 5 + g1 - g0:] == -7.0).all())
    # float64 weights stay on the eigensolver; method="matfun" keeps refusing float64
    f32_first(eng)
    eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, 1.1, return_weights=True)
    assert "letkf_tile64" not in last_kernel()
    with pytest.raises(ValueError):
        eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, 1.1, method="matfun")


# ---- 6. metric independence ----------------------------------------------------------------------------------------------------
def test_periodic_metric_and_python_distance_in_the_default_dtype(mia, eng):
    """The route works from per-point lists, whatever made them: a ring with tiles at the seam (PeriodicMetric) and a host
    ``dist_func`` (lists from localize_from_dist), both through LETKF(...) without a dtype."""
    G, L, c = 203, 203.0, 6.0                      # (G is not a multiple of 16: the last tile ends at the seam)
    case = O.synthetic_case(G, 27, 2, seed=41, m=2)

    def ring(g, o):
        dd = np.abs(np.asarray(o, dtype=np.float64).reshape(-1) - float(np.asarray(g).reshape(-1)[0]))
        return np.minimum(dd, L - dd)
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.1, dist_func=ring)[0]
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(c, dist_func=mia.PeriodicMetric(L)), inf_factor=1.1)
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"], case["obs_x"])
    assert "letkf_tile64" in last_kernel(), last_kernel()
    check(xa.cpu().numpy(), ref, "PeriodicMetric ring")
    f32_first(eng)
    user = mia.GaspariCohn(c, lambda grid, obs: ring(grid, obs))
    xu = mia.LETKF(localization=user, inf_factor=1.1).analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"],
                                                                     case["obs_x"])
    assert "letkf_tile64" in last_kernel(), last_kernel()
    check(xu.cpu().numpy(), ref, "python dist_func")


# ---- 7. full size --------------------------------------------------------------------------------------------------------------
def test_config2_at_full_size_every_point(mia):
    """Config 2 at 1e5 grid points (k = 40, 5e4 observations) through LETKF(...).analyse_arrays in the default dtype, EVERY grid
    point against the float64 oracle.  Measured on one MI355X: see DESIGN 9."""
    import bench
    import oracle_pool
    if not oracle_pool.started():
        pytest.skip("oracle worker pool not running (it is forked at session start for -m gpu runs)")
    G = 100000
    X, gx, ox, Yb, d = bench.make_case(G, 40, 2, torch.device(DEV), seed=42)
    X, Yb, d = X.double(), Yb.double(), d.double()
    f = mia.LETKF(localization=mia.GaspariCohn(10.0, mia.AbsoluteDistance()), inf_factor=1.1)
    xa = f.analyse_arrays(X, Yb, d, grid_coords=gx.cpu().numpy(), obs_coords=ox.cpu().numpy())
    assert "letkf_tile64_kernel<2, 3>" in last_kernel(), last_kernel()
    assert xa.dtype == torch.float64 and bool(torch.isfinite(xa).all())
    ref = oracle_pool.oracle_analysis(X.cpu().numpy(), gx.cpu().numpy(), ox.cpu().numpy(), Yb.cpu().numpy(), d.cpu().numpy(),
                                      10.0, 1.1, np.arange(G))
    check(xa.cpu().numpy(), ref, "config 2, 1e5 grid points, every point")

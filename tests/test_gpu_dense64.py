"""The float64 tile route for dense local networks, p_max > k (csrc/letkf_dense64.hip, mia_letkf_analysis_dense_f64): what
LETKF(...) runs in its default working precision when a grid point sees more observations than there are members.  Contract as
tests/test_gpu_tile64.py: relative Frobenius error AND the worst single grid point <= 1e-10 against the float64 oracle.  In the
shape sweep no point may be declined, so that the Jacobi kernel cannot supply the parity."""
import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O
from torch_assimilate_amd._cabi import MiaError

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
LOG_TOL, MARGIN, CAP = 26.0, 2, 127            # the float64 tables' truncation target, margin and degree cap
KERNEL = "letkf_dense64_kernel"


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
    from oracle_pool import per_point_errors
    pp, fro = per_point_errors(got, ref)
    print("\n[dense64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= TOL64, what
    assert pp.max() <= TOL64, what
    return fro, float(pp.max())


def run64(eng, case, nb, inf, method="dense64", **kw):
    """engine.analysis in float64 with a caller-owned decline counter: (Xa, flags, declined, kernel name).  The route is named:
    method="auto" takes it only up to p_max = 2.4 k (LetkfEngine.DENSE64_AUTO_NUM; test_methods_... checks that hand-over)"""
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
    assert KERNEL not in last_kernel()


def expected_degrees64(yb, nb, inf):
    """Chebyshev degree per grid point as the kernel chooses it, restated in float64 numpy from the per-point lists (the formula
    of tests/test_gpu_tile64.py: C_g and S = D G D share the non-zero spectrum, so the bound is the same): Gershgorin bound L of
    S, T = L / reg rounded up to the table's geometric grid (32 per octave, 2^-24 .. 2^8), degree = ceil(26 / log rho) + 2,
    rho = (sqrt(1 + T) + 1) / (sqrt(1 + T) - 1)"""
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


def mesh_case(nx, ny, k, stride, seed, m=1):
    rnd = np.random.RandomState(seed)
    gy, gx = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    sel = ((grid[:, 0] % stride) == 0) & ((grid[:, 1] % stride) == 0)
    state = rnd.normal(size=(m, k, grid.shape[0]))
    y = rnd.normal(size=int(sel.sum()))
    yb, d = O.obs_space_uncorr(state[0][:, sel], y, np.ones_like(y))
    return dict(state=state, grid=grid, obs=grid[sel], yb=yb, d=d)


def largest_union(nb):
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    return max(len(set(np.concatenate([idx[g, :cnt[g]] for g in range(t, min(t + 16, len(cnt)))]))) for t in range(0, len(cnt), 16))


def entry_args(X, G, m, k, rec, nb, inf, out, fl, retry):
    return (X.data_ptr(), G, m, k, 0, G, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(), nb.idx.data_ptr(), nb.w.data_ptr(),
            nb.p_cap, nb.p_max, inf, 0.0, out.data_ptr(), G, 0, fl.data_ptr(), retry.data_ptr(), None)


# ---- 1. symbols -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve(mia):
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    for name in ("mia_letkf_analysis_dense_f64", "mia_letkf_dense_f64_cover"):
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS
    assert lib.mia_letkf_dense_f64_cover(1, 40, 77, 100000, 100000, 100000, 100000) == 1
    assert lib.mia_letkf_dense_f64_cover(3, 64, 153, 1000, 1000, 1000, 1000) == 1
    assert lib.mia_letkf_dense_f64_cover(1, 65, 153, 1000, 1000, 1000, 1000) == 0       # ensemble size
    assert lib.mia_letkf_dense_f64_cover(1, 40, 40, 1000, 1000, 1000, 1000) == 0        # p_max <= k: the dual route's
    assert lib.mia_letkf_dense_f64_cover(1, 40, 20, 1000, 1000, 1000, 1000) == 0
    assert lib.mia_letkf_dense_f64_cover(1, 24, 3000, 1000, 1000, 1000, 3000) == 0      # stays on the Jacobi kernel
    # argument validation precedes any device work
    call = lib.mia_letkf_analysis_dense_f64
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, -1.0, 0.0, None, 10, 0, None, None, None) == -2
    assert call(None, 10, 1, 1, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None) == -2
    assert call(None, 10, 1, 4, 0, 0, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None) == 0
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.5, None, 10, 0, None, None, None) == -3   # gamma > 0
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None) == -1


# ---- 2. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
# (k, obs stride, radius) of the 1-D rows; p_max and the largest union of sixteen points as the CPU emulation of the route had them
SWEEP = [(20, 1, 8.0, 31, 46), (8, 1, 10.0, 39, 54), (27, 1, 16.0, 61, 76), (40, 1, 20.0, 77, 92), (40, 1, 45.0, 173, 188),
         (64, 1, 40.0, 153, 168), (5, 2, 30.0, 58, 65)]


def sweep_checks(eng, case, nb, loc, m, what, **okw):
    for inf in (1.0, 1.1):
        f32_first(eng)
        xa, fl, declined, kern = run64(eng, case, nb, inf)
        assert KERNEL in kern and "letkf_tile64" not in kern, kern
        assert declined == 0
        fl = fl.cpu().numpy()
        assert int((fl & 0xff).max()) == 0
        assert np.array_equal((fl >> 8) & 0xff, expected_degrees64(case["yb"], nb, inf))
        ref = O.letkf_analysis(case["state"], loc[0], loc[1], case["yb"], case["d"], loc[2], inf, **okw)[0]
        check(xa.cpu().numpy(), ref, "%s m %d inf %g p_max %d (%s)" % (what, m, inf, nb.p_max, kern))


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k,stride,c,p_max,union", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, stride, c, p_max, union, m):
    """k x dense networks with p_max > k: KT = 1 .. 4 (k = 5 and 8 are the KT = 1 instantiations with random points,
    DESIGN 4.2), unions of 46 .. 188 slots, ragged last tile (G = 203), one and several state rows, both inflations."""
    case = O.synthetic_case(203, k, stride, seed=k + m, m=m)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == p_max and p_max > k and largest_union(nb) == union
    sweep_checks(eng, case, nb, (case["grid_x"], case["obs_x"], c), m, "k %d stride %d c %g" % (k, stride, c))


@pytest.mark.parametrize("m", [1, 3])
def test_mesh_2d_with_observations_everywhere(eng, m):
    """An 18 x 18 mesh in row-major order with an observation at every point, radius 3: p_max 101, sixteen consecutive points
    see about 200 observations -- more than the slots of the launch, so the tiles are analysed in parts."""
    case = mesh_case(18, 18, 40, 1, seed=7 + m, m=m)
    nb = eng.localize(case["grid"], case["obs"], [3.0])
    assert nb.p_max == 101 and largest_union(nb) == 200
    sweep_checks(eng, case, nb, (case["grid"], case["obs"], 3.0), m, "18 x 18 mesh, k 40, c 3")


# ---- 3. other inputs -------------------------------------------------------------------------------------------------------------
def test_one_ragged_tile_and_more_tiles_than_xcd_classes(eng):
    case = O.synthetic_case(2500, 20, 1, seed=13, m=2)          # 157 tiles: more than the 8 XCD classes of the tile map
    nb = eng.localize(case["grid_x"], case["obs_x"], [8.0])
    assert nb.p_max > 20
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 8.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "G = 2500")
    # one ragged tile of eleven points that see MORE observations than members: k = 5
    case = O.synthetic_case(11, 5, 1, seed=12, m=2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [8.0])
    assert nb.p_max > 5
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 8.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "G = 11")


def test_two_radius_groups_and_gc_inf(eng):
    case = mesh_case(20, 6, 27, 1, seed=9, m=2)
    nb = eng.localize(case["grid"], case["obs"], [4.0, 2.0], coord_group=[0, 1])
    assert nb.p_max > 27
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern and declined == 0
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], [4.0, 2.0], 1.1, coord_group=[0, 1])[0]
    check(xa.cpu().numpy(), ref, "two radius groups, p_max %d" % nb.p_max)
    c1 = O.synthetic_case(150, 20, 1, seed=11)
    nb = eng.localize(c1["grid_x"], c1["obs_x"], [9.0], taper=1)
    assert nb.p_max > 20
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, c1, nb, 1.0)
    assert KERNEL in kern and declined == 0
    ref = O.letkf_analysis(c1["state"], c1["grid_x"], c1["obs_x"], c1["yb"], c1["d"], 9.0, 1.0, taper="gc_inf")[0]
    check(xa.cpu().numpy(), ref, "GaspariCohnInf, p_max %d" % nb.p_max)


def test_periodic_metric_and_python_distance_in_the_default_dtype(mia, eng):
    """The route works from per-point lists, whatever made them: a ring with tiles at the seam (PeriodicMetric) and a host
    ``dist_func`` (lists from localize_from_dist), both through LETKF(...) without a dtype."""
    G, L, c = 203, 203.0, 12.0                     # (G is not a multiple of 16: the last tile ends at the seam)
    case = O.synthetic_case(G, 27, 1, seed=41, m=2)

    def ring(g, o):
        dd = np.abs(np.asarray(o, dtype=np.float64).reshape(-1) - float(np.asarray(g).reshape(-1)[0]))
        return np.minimum(dd, L - dd)
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.1, dist_func=ring)[0]
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(c, dist_func=mia.PeriodicMetric(L)), inf_factor=1.1)
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"], case["obs_x"])
    assert xa.dtype == torch.float64 and KERNEL in last_kernel(), last_kernel()
    check(xa.cpu().numpy(), ref, "PeriodicMetric ring")
    f32_first(eng)
    user = mia.GaspariCohn(c, lambda grid, obs: ring(grid, obs))
    xu = mia.LETKF(localization=user, inf_factor=1.1).analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"],
                                                                     case["obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    check(xu.cpu().numpy(), ref, "python dist_func")


# ---- 4. declined points are redone -----------------------------------------------------------------------------------------------
def test_strong_observations_are_declined_and_redone(eng):
    """k 40, c 20 with yb, d scaled x10 (a-priori degree 208, far above the cap): EVERY point is flagged and counted, Xa is
    untouched by the C entry, and the Jacobi kernel's redo gives the oracle's analysis of the scaled inputs."""
    G = 203
    case = O.synthetic_case(G, 40, 1, seed=5)
    case["yb"], case["d"] = case["yb"] * 10.0, case["d"] * 10.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    assert int(expected_degrees64(case["yb"], nb, 1.1).min()) > CAP
    from torch_assimilate_amd import _cabi
    X = dev(case["state"])
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    out = torch.full((1, 40, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_letkf_analysis_dense_f64(*entry_args(X, G, 1, 40, rec, nb, 1.1, out, fl, retry))
    torch.cuda.synchronize()
    assert rc == 0 and int(retry.item()) == G
    assert bool((fl == 8).all()) and bool((out == -7.0).all())
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert declined == G and KERNEL in kern                   # (the redo does not overwrite the reported kernel)
    assert int((fl.cpu().numpy() & 8).max()) == 0             # the redo rewrote the flags
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 20.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "x10 observations, all %d points redone" % G)


def test_a_strong_cluster_declines_exactly_the_points_above_the_cap(eng):
    """Observations 80 .. 85 ten times as strong: the flagged set equals "degree from the table for this point's Gershgorin
    bound > cap", restated in float64 numpy -- 39 of 203 points."""
    G = 203
    case = O.synthetic_case(G, 40, 1, seed=6)
    case["yb"][:, 80:86] *= 10.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    want = expected_degrees64(case["yb"], nb, 1.1) > CAP
    assert int(want.sum()) == 39
    X = dev(case["state"])
    out = torch.full((1, 40, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    f32_first(eng)
    res = eng.analysis(X, dev(case["yb"]), dev(case["d"]), nb, 1.1, out=out, flags=fl, retry=retry, defer_retry=True)
    torch.cuda.synchronize()
    assert KERNEL in last_kernel()
    got = (fl.cpu().numpy() & 8) != 0
    assert np.array_equal(got, want)
    assert int(retry.item()) == 39
    assert bool((out[:, :, torch.as_tensor(want, device=DEV)] == -7.0).all())       # declined points are left untouched
    assert res[-1]() == 39                                                          # the deferred redo
    torch.cuda.synchronize()
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 20.0, 1.1)[0]
    check(out.cpu().numpy(), ref, "strong cluster, 39 points redone")


# ---- 5. bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c", [(40, 45.0), (20, 16.0), (8, 10.0)])
def test_a_points_bits_do_not_depend_on_its_tile(eng, k, c):
    """Sub-ranges against the full run, bit for bit.  The route is chosen from the shard's own p_max, and a shard whose longest
    list has at most k entries belongs to letkf_tile64_kernel, another summation altogether: the radii are such that the
    single edge point of the (1, 2) shard still sees more observations than there are members, and every part is checked to
    have run on this kernel."""
    G = 331
    case = O.synthetic_case(G, k, 1, seed=21, m=2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max > k
    full, _, declined, kern = run64(eng, case, nb, 1.1)
    assert declined == 0 and KERNEL in kern
    again = run64(eng, case, nb, 1.1)[0]
    assert torch.equal(full, again)
    for g0, g1 in ((5, 200), (21, G), (103, 119), (1, 2)):
        nbp = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
        assert nbp.p_max > k, (g0, g1)
        f32_first(eng)
        part, _, _, kern = run64(eng, case, nbp, 1.1)
        assert KERNEL in kern, (g0, g1, kern)
        assert part.shape[-1] == g1 - g0
        assert torch.equal(part, full[:, :, g0:g1]), (g0, g1)


def test_observation_order(eng):
    """A permutation of the observations changes the ranks inside a union, i.e. the summation order -- rounding only.  The
    bound is float64 rounding through a recurrence of at most 127 steps over at most 256 terms (1.1e-16 x 256 x 127 < 4e-12
    if every rounding error lined up; as a random walk sqrt(256 x 127) x 1.1e-16 = 2e-14): 1e-11, one order below the contract."""
    case = O.synthetic_case(331, 40, 1, seed=22)
    perm = np.random.RandomState(1).permutation(case["obs_x"].shape[0])
    pc = dict(case, obs_x=case["obs_x"][perm], yb=case["yb"][:, perm], d=case["d"][perm])
    out = {}
    for method in ("auto", "eig"):
        f32_first(eng)
        a, _, _, ka = run64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [20.0]), 1.1, method=method)
        b = run64(eng, pc, eng.localize(pc["grid_x"], pc["obs_x"], [20.0]), 1.1, method=method)[0]
        out[method] = float(torch.linalg.norm(a - b) / torch.linalg.norm(a))
        assert method == "eig" or KERNEL in ka           # (the Jacobi kernel reports no name of its own)
    print("\n[dense64] permuted observations: rel. change %.3e (dense64), %.3e (Jacobi kernel)" % (out["auto"], out["eig"]))
    assert out["auto"] <= 1e-11


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------
def test_points_without_observations_get_the_inflated_prior(eng):
    case = O.synthetic_case(203, 20, 1, seed=31, m=2)
    keep = case["obs_x"] < 60
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [8.0])
    assert nb.p_max > 20
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
    far = slice(90, 203)                                             # (whole tiles and parts of tiles without any observation)
    assert int(nb.cnt[far].max().item()) == 0
    st = case["state"][:, :, far]
    mean = st.mean(axis=1, keepdims=True)
    assert rel_fro(xa.cpu().numpy()[:, :, far], mean + np.sqrt(1.1) * (st - mean)) <= 1e-14
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 8.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "observations in a part of the domain")


def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    case = O.synthetic_case(203, 40, 1, seed=32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    clean, _, _, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern
    j = 77
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][3, j] = np.nan
    xa, fl, declined, kern = run64(eng, bad, nb, 1.1)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(203)])
    assert 0 < uses.sum() < 203
    assert np.array_equal((fl.cpu().numpy() & 4) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(xa[:, :, keep], clean[:, :, keep])


# ---- 7. routing ----------------------------------------------------------------------------------------------------------------
def test_methods_tile_option_and_output_offset(eng):
    case = O.synthetic_case(203, 40, 1, seed=34, m=2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 20.0, 1.1)[0]
    f32_first(eng)
    assert 5 * nb.p_max <= 12 * 40
    xa, _, declined, kern = run64(eng, case, nb, 1.1, method="auto")
    assert KERNEL in kern and declined == 0
    check(xa.cpu().numpy(), ref, "auto")
    f32_first(eng)
    xd, _, _, kern = run64(eng, case, nb, 1.1, method="dense64")
    assert KERNEL in kern and torch.equal(xd, xa)
    # "dense64" names the route and raises outside it: p_max <= k, float32, weights, the RBF core
    sparse = O.synthetic_case(203, 40, 2, seed=34)
    nbs = eng.localize(sparse["grid_x"], sparse["obs_x"], [10.0])
    assert nbs.p_max <= 40
    with pytest.raises(MiaError, match="status -3"):
        run64(eng, sparse, nbs, 1.1, method="dense64")
    X, Yb, d = dev(case["state"]), dev(case["yb"]), dev(case["d"])
    with pytest.raises(ValueError):
        eng.analysis(X.float(), Yb.float(), d.float(), nb, 1.1, method="dense64")
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, nb, 1.1, method="dense64", return_weights=True)
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, nb, 1.1, method="dense64", rbf_gamma=0.5)
    with pytest.raises(MiaError, match="status -3"):
        run64(eng, case, nb, 1.1, method="matfun64")           # the dual route keeps refusing p_max > k
    # method="eig" and tile = 0 stay on the Jacobi kernel and agree bit for bit
    f32_first(eng)
    xe, _, _, kern = run64(eng, case, nb, 1.1, method="eig")
    assert KERNEL not in kern and "letkf_tile64" not in kern
    check(xe.cpu().numpy(), ref, "eig")
    set_option("tile", 0)
    try:
        f32_first(eng)
        xo, _, _, kern = run64(eng, case, nb, 1.1, method="auto")
        assert KERNEL not in kern and "letkf_tile64" not in kern
        with pytest.raises(MiaError, match="status -3"):
            run64(eng, case, nb, 1.1, method="dense64")
    finally:
        set_option("tile", 1)
    assert torch.equal(xo, xe)
    # above p_max = 2.4 k "auto" stays on the Jacobi kernel (the gain there is not a function of the shape alone);
    # "dense64" still names the route
    nbw = eng.localize(case["grid_x"], case["obs_x"], [45.0])
    assert 5 * nbw.p_max > 12 * 40
    f32_first(eng)
    xw, _, _, kern = run64(eng, case, nbw, 1.1, method="auto")
    assert KERNEL not in kern and "letkf_tile64" not in kern
    assert torch.equal(xw, run64(eng, case, nbw, 1.1, method="eig")[0])
    f32_first(eng)
    assert KERNEL in run64(eng, case, nbw, 1.1)[3]
    # ... and so it does above 8 state rows (a further row costs the dense route three times what it costs the Jacobi kernel)
    rows = dict(case, state=np.concatenate([case["state"]] * 5, axis=0)[:9])
    f32_first(eng)
    x9, _, _, kern = run64(eng, rows, nb, 1.1, method="auto")
    assert KERNEL not in kern and "letkf_tile64" not in kern
    assert torch.equal(x9, run64(eng, rows, nb, 1.1, method="eig")[0])
    # out= with a column offset, a sub-range of the grid
    g0, g1 = 21, 150
    nbr = eng.localize(case["grid_x"], case["obs_x"], [20.0], g0=g0, g1=g1)
    out = torch.full((2, 40, g1 - g0 + 9), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    res = eng.analysis(X, Yb, d, nbr, 1.1, out=out, out_offset=5)
    torch.cuda.synchronize()
    assert res is out and KERNEL in last_kernel()
    assert torch.equal(out[:, :, 5:5 + g1 - g0], xa[:, :, g0:g1])
    assert bool((out[:, :, :5] == -7.0).all()) and bool((out[:, :, 5 + g1 - g0:] == -7.0).all())

"""The streamed float64 tile route for dense local networks of up to 128 members (csrc/letkf_stream64.hip,
mia_letkf_analysis_stream_f64): what LETKF(...) runs in its default working precision at 97 .. 128 members when a grid point sees
more observations than there are members -- shapes that raised MiaError before (the Jacobi kernel's LDS).  Contract as
tests/test_gpu_dense64.py: relative Frobenius error AND the worst single grid point <= 1e-10 against the float64 oracle.  In the
shape sweep no point may be declined, so that the Jacobi kernel cannot supply the parity."""
import numpy as np
import pytest
import torch

from conftest import rel_fro
from oracle import letkf_oracle as O
from torch_assimilate_amd._cabi import MiaError

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
LOG_TOL, MARGIN, CAP = 26.0, 2, 127            # the float64 tables' truncation target, margin and degree cap
KERNEL = "letkf_stream64_kernel"
G = 203


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
    print("\n[stream64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= TOL64, what
    assert pp.max() <= TOL64, what
    return fro, float(pp.max())


def run64(eng, case, nb, inf, method="stream64", **kw):
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
    assert KERNEL not in last_kernel()


def expected_degrees64(yb, nb, inf):
    """Chebyshev degree per grid point as the kernel chooses it, restated in float64 numpy from the per-point lists (the formula
    of tests/test_gpu_dense64.py): Gershgorin bound L of S = D G D, T = L / reg rounded up to the table's geometric grid (32 per
    octave, 2^-24 .. 2^8), degree = ceil(26 / log rho) + 2, rho = (sqrt(1 + T) + 1) / (sqrt(1 + T) - 1)"""
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


def entry_args(X, n, m, k, rec, nb, inf, out, fl, retry, p_max=None):
    return (X.data_ptr(), n, m, k, 0, n, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(), nb.idx.data_ptr(), nb.w.data_ptr(),
            nb.p_cap, nb.p_max if p_max is None else p_max, inf, 0.0, out.data_ptr(), n, 0, fl.data_ptr(), retry.data_ptr(), None)


_CASE80 = {}


def case80(eng):
    """the k = 80 / c = 24 case of tests 4 and 6, its lists and its full analysis by name (computed once, never changed)"""
    if not _CASE80:
        case = O.synthetic_case(G, 80, 1, seed=21, m=2)
        nb = eng.localize(case["grid_x"], case["obs_x"], [24.0])
        assert nb.p_max == 93
        full, _, declined, kern = run64(eng, case, nb, 1.1)
        assert declined == 0 and KERNEL in kern
        _CASE80.update(case=case, nb=nb, full=full)
    return _CASE80["case"], _CASE80["nb"], _CASE80["full"]


# ---- 1. symbols and validation codes ---------------------------------------------------------------------------------------------
def test_new_symbols_resolve(mia):
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    for name in ("mia_letkf_analysis_stream_f64", "mia_letkf_stream_f64_cover"):
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS
    cover = lib.mia_letkf_stream_f64_cover
    assert cover(1, 128, 139, 100000, 100000, 100000, 100000) == 1
    assert cover(3, 80, 256, 1000, 1000, 1000, 1000) == 1
    assert cover(1, 40, 77, 1000, 1000, 1000, 1000) == 1           # k <= 64 by name
    assert cover(1, 129, 203, 1000, 1000, 1000, 1000) == 0         # ensemble size
    assert cover(1, 80, 80, 1000, 1000, 1000, 1000) == 0           # p_max <= k: the dual routes'
    assert cover(1, 80, 257, 1000, 1000, 1000, 1000) == 0          # more than 256 slots: stays on the Jacobi kernel
    # argument validation precedes any device work
    call = lib.mia_letkf_analysis_stream_f64
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, -1.0, 0.0, None, 10, 0, None, None, None) == -2
    assert call(None, 10, 1, 1, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None) == -2
    assert call(None, 10, 1, 4, 0, 0, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None) == 0
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.5, None, 10, 0, None, None, None) == -3   # gamma > 0
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None) == -1


# ---- 2. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
# (k, radius, p_max, largest union of sixteen points): KT = 5 with one member in the last block .. KT = 8 ragged and full, one
# list that holds every observation, and k <= 64 by name
SWEEP = [(65, 20.0, 77, 92), (80, 24.0, 93, 108), (80, 45.0, 173, 188), (96, 28.0, 107, 122), (113, 32.0, 123, 138),
         (128, 36.0, 139, 154), (128, 62.0, 203, 203), (40, 20.0, 77, 92)]


def sweep_checks(eng, case, nb, loc, m, what):
    xs = None
    for inf in (1.0, 1.1):
        f32_first(eng)
        xa, fl, declined, kern = run64(eng, case, nb, inf)
        assert KERNEL in kern, kern
        assert declined == 0
        fl = fl.cpu().numpy()
        assert int((fl & 0xff).max()) == 0
        assert np.array_equal((fl >> 8) & 0xff, expected_degrees64(case["yb"], nb, inf))
        ref = O.letkf_analysis(case["state"], loc[0], loc[1], case["yb"], case["d"], loc[2], inf)[0]
        check(xa.cpu().numpy(), ref, "%s m %d inf %g p_max %d (%s)" % (what, m, inf, nb.p_max, kern))
        xs = xa
    return xs


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k,c,p_max,union", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, c, p_max, union, m):
    case = O.synthetic_case(G, k, 1, seed=k + m, m=m)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == p_max and p_max > k and largest_union(nb) == union
    xs = sweep_checks(eng, case, nb, (case["grid_x"], case["obs_x"], c), m, "k %d c %g" % (k, c))
    if k == 40:
        # the resident image against the streamed one: the same chains over the union, but the recurrence's other terms enter
        # the accumulator first here -- rounding only; printed, not asserted
        xd = run64(eng, case, nb, 1.1, method="dense64")[0]
        print("\n[stream64] k 40: largest difference to method='dense64' %.3e (largest |xa| %.3e)"
              % (float((xs - xd).abs().max()), float(xd.abs().max())))


# ---- 3. tiles in parts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
def test_mesh_2d_with_observations_everywhere(eng, m):
    """An 18 x 18 mesh in row-major order with an observation at every point, radius 3, 80 members: p_max 101, sixteen
    consecutive points see 200 observations -- the launch takes ceil((101 + 16) / 16) = 8 blocks = 128 slots, so the tiles are
    analysed in halves."""
    case = mesh_case(18, 18, 80, 1, seed=7 + m, m=m)
    nb = eng.localize(case["grid"], case["obs"], [3.0])
    assert nb.p_max == 101 and largest_union(nb) == 200
    assert 16 * ((nb.p_max + 31) >> 4) < 200
    sweep_checks(eng, case, nb, (case["grid"], case["obs"], 3.0), m, "18 x 18 mesh, k 80, c 3")


# ---- 4. bits -------------------------------------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile_or_shard(eng):
    """Sub-ranges that start at 0, 5, 16 and 37, two shards, and a second call, against the full call, bit for bit.  Every range
    holds interior points (93 observations > 80 members), so every part runs on this kernel."""
    case, nb, full = case80(eng)
    again = run64(eng, case, nb, 1.1)[0]
    assert torch.equal(full, again)
    for g0, g1 in ((0, 120), (5, 200), (16, 64), (37, G), (0, 101), (101, G)):
        nbp = eng.localize(case["grid_x"], case["obs_x"], [24.0], g0=g0, g1=g1)
        assert nbp.p_max > 80, (g0, g1)
        f32_first(eng)
        part, _, declined, kern = run64(eng, case, nbp, 1.1)
        assert KERNEL in kern and declined == 0, (g0, g1, kern)
        assert part.shape[-1] == g1 - g0
        assert torch.equal(part, full[:, :, g0:g1]), (g0, g1)


# ---- 5. non-finite and loud failures ---------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    case = O.synthetic_case(G, 65, 1, seed=32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    clean, _, declined, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern and declined == 0
    j = 77
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][3, j] = np.nan
    xa, fl, declined, kern = run64(eng, bad, nb, 1.1)
    assert KERNEL in kern
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G
    assert np.array_equal((fl.cpu().numpy() & 4) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(xa[:, :, keep], clean[:, :, keep])


def test_an_understated_p_max_fails_loudly_for_those_points_only(eng):
    from torch_assimilate_amd import _cabi
    k = 65
    case = O.synthetic_case(G, k, 1, seed=33)
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    clean, _, _, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern
    short = nb.p_max - 3
    cnt = nb.cnt.cpu().numpy()
    over = cnt > short
    assert short > k and 0 < over.sum() < G
    X = dev(case["state"])
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    out = torch.full((1, k, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_letkf_analysis_stream_f64(*entry_args(X, G, 1, k, rec, nb, 1.1, out, fl, retry, p_max=short))
    torch.cuda.synchronize()
    assert rc == 0 and int(retry.item()) == 0
    assert np.array_equal((fl.cpu().numpy() & 0xff) == 1, over)                    # MIA_FLAG_OVERFLOW
    sel = torch.as_tensor(over, device=DEV)
    assert bool(torch.isnan(out[:, :, sel]).all())
    assert torch.equal(out[:, :, ~sel], clean[:, :, ~sel])


def test_points_without_observations_get_the_inflated_prior(eng):
    case = O.synthetic_case(G, 65, 1, seed=31, m=2)
    keep = case["obs_x"] < 100
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    assert nb.p_max > 65
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert KERNEL in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
    cnt = nb.cnt.cpu().numpy()
    far = cnt == 0
    assert far.sum() >= 17 and cnt[far.argmax() - 1] > 0            # whole tiles and a part of a tile without any observation
    st = case["state"][:, :, far]
    mean = st.mean(axis=1, keepdims=True)
    assert rel_fro(xa.cpu().numpy()[:, :, far], mean + np.sqrt(1.1) * (st - mean)) <= 1e-14
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 20.0, 1.1)[0]
    check(xa.cpu().numpy(), ref, "observations in a part of the domain")


# ---- 6. declines -----------------------------------------------------------------------------------------------------------------
def strong_cluster(case, nb, inf):
    """Observations 80 .. 85 scaled by the smallest power of sqrt(2) at which the numpy degree exceeds the cap at SOME points:
    (scaled case, declined mask)"""
    for e in range(1, 40):
        s = 2.0 ** (0.5 * e)
        yb, d = case["yb"].copy(), case["d"].copy()
        yb[:, 80:86] *= s
        d[80:86] *= s
        want = expected_degrees64(yb, nb, inf) > CAP
        if want.any():
            assert not want.all()
            return dict(case, yb=yb, d=d), want
    raise AssertionError("no scale declines a point")


def test_a_strong_cluster_is_declined_and_redone_at_80_members(eng):
    case, nb, full = case80(eng)
    strong, want = strong_cluster(case, nb, 1.1)
    X = dev(strong["state"])
    out = torch.full((2, 80, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    f32_first(eng)
    res = eng.analysis(X, dev(strong["yb"]), dev(strong["d"]), nb, 1.1, out=out, flags=fl, retry=retry, defer_retry=True,
                       method="stream64")
    torch.cuda.synchronize()
    assert KERNEL in last_kernel()
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    assert int(retry.item()) == int(want.sum()) > 0
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[:, :, sel] == -7.0).all())                                    # declined points are left untouched
    before = out.clone()
    assert res[-1]() == int(want.sum())                                            # the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & 8).max()) == 0                                  # the redo rewrote the flags
    assert torch.equal(out[:, :, ~sel], before[:, :, ~sel])                        # ... and nothing else
    ref = O.letkf_analysis(strong["state"], strong["grid_x"], strong["obs_x"], strong["yb"], strong["d"], 24.0, 1.1)[0]
    check(out.cpu().numpy(), ref, "strong cluster, %d points redone" % int(want.sum()))


def test_a_declined_point_raises_at_128_members_after_the_others_are_written(eng):
    """The redo is the Jacobi kernel's, which cannot hold 128 members: MiaError, data-dependent, AFTER every other point has been
    written (as 2.11)."""
    case = O.synthetic_case(G, 128, 1, seed=23)
    nb = eng.localize(case["grid_x"], case["obs_x"], [36.0])
    strong, want = strong_cluster(case, nb, 1.1)
    out = torch.full((1, 128, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    f32_first(eng)
    with pytest.raises(MiaError, match="status -3"):
        eng.analysis(dev(strong["state"]), dev(strong["yb"]), dev(strong["d"]), nb, 1.1, out=out, flags=fl)
    torch.cuda.synchronize()
    assert KERNEL in last_kernel()
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[:, :, sel] == -7.0).all())
    ref = O.letkf_analysis(strong["state"], strong["grid_x"], strong["obs_x"], strong["yb"], strong["d"], 36.0, 1.1)[0]
    check(out.cpu().numpy()[:, :, ~want], ref[:, :, ~want], "k 128: the %d points that were not declined" % int((~want).sum()))


# ---- 7. hand-over ----------------------------------------------------------------------------------------------------------------
def test_auto_hands_over_where_the_rule_says(eng):
    for k, c, kernel in ((128, 36.0, KERNEL), (40, 20.0, "letkf_dense64_kernel"), (80, 16.5, "letkf_wide64_kernel")):
        case = O.synthetic_case(G, k, 1, seed=50 + k)
        nb = eng.localize(case["grid_x"], case["obs_x"], [c])
        assert (nb.p_max > k) == (kernel != "letkf_wide64_kernel")
        f32_first(eng)
        xa, _, declined, kern = run64(eng, case, nb, 1.1, method="auto")
        assert kernel in kern and declined == 0, (k, kern)
        check(xa.cpu().numpy(), O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.1)[0],
              "auto, k %d" % k)
    # "stream64" names the route and raises outside it: p_max <= k (the case above), float32, weights, the RBF core
    with pytest.raises(MiaError, match="status -3"):
        run64(eng, case, nb, 1.1, method="stream64")
    X, Yb, d = dev(case["state"]), dev(case["yb"]), dev(case["d"])
    with pytest.raises(ValueError):
        eng.analysis(X.float(), Yb.float(), d.float(), nb, 1.1, method="stream64")
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, nb, 1.1, method="stream64", return_weights=True)
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, nb, 1.1, method="stream64", rbf_gamma=0.5)
    # where the Jacobi kernel runs (65 .. 96 members) "auto" hands over inside the measured range only: p_max / k up
    # to 173 / 80, up to 8 state rows
    assert (eng.STREAM64_AUTO_MIN_K, eng.STREAM64_AUTO_NUM, eng.STREAM64_AUTO_DEN, eng.STREAM64_AUTO_MAX_ROWS) == (65, 173, 80, 8)
    for k, c, m, stream in ((80, 45.0, 1, True), (80, 24.0, 8, True), (80, 24.0, 9, False), (65, 45.0, 1, False)):
        case = O.synthetic_case(G, k, 1, seed=70 + m, m=m)
        nb = eng.localize(case["grid_x"], case["obs_x"], [c])
        assert nb.p_max == (173 if c == 45.0 else 93)
        f32_first(eng)
        kern = run64(eng, case, nb, 1.1, method="auto")[3]
        assert (KERNEL in kern) == stream and "letkf_wide64" not in kern and "letkf_tile64" not in kern, (k, c, m, kern)
    # "auto" never takes the route at k <= 64, whatever the lists
    case = O.synthetic_case(G, 64, 1, seed=64)
    nb = eng.localize(case["grid_x"], case["obs_x"], [45.0])
    assert 5 * nb.p_max > 12 * 64
    f32_first(eng)
    assert KERNEL not in run64(eng, case, nb, 1.1, method="auto")[3]


# ---- 8. the class ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c", [(128, 36.0), (113, 32.0)])
def test_the_class_in_the_default_dtype(mia, eng, k, c):
    """LETKF(localization, inf_factor) exactly as with the reference -- no dtype argument.  Before this route these calls raised
    MiaError (status -3): the Jacobi kernel's two k x (k + 1) float64 matrices are 264 KB at k = 128 and 206 KB at k = 113."""
    case = O.synthetic_case(G, k, 1, seed=90 + k, m=2)
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(c, mia.AbsoluteDistance()), inf_factor=1.1)
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    assert xa.dtype == torch.float64 and KERNEL in last_kernel(), last_kernel()
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.1)[0]
    check(xa.cpu().numpy(), ref, "LETKF(...) default dtype, k %d" % k)

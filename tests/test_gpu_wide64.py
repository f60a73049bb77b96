"""The wide float64 tile route (csrc/letkf_wide64.hip, mia_letkf_analysis_wide_f64): what LETKF(...) runs in its default working
precision for ensembles of 65 .. 128 members with p_max <= k.  The contract is the project's float64 one: relative
Frobenius error <= 1e-10 against the float64 oracle -- and also the WORST SINGLE GRID POINT <= 1e-10.  In the shape sweep no point
may be declined, so that the Jacobi kernel cannot supply the parity."""
import re

import numpy as np
import pytest
import torch

from conftest import set_option
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
G = 203                                        # thirteen tiles, the last one ragged
LOG_TOL, MARGIN, CAP = 26.0, 2, 127            # the float64 table's truncation target, margin and degree cap
KERNEL = "letkf_wide64_kernel<"


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
    print("\n[wide64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= TOL64, what
    assert pp.max() <= TOL64, what
    return fro, float(pp.max())


_REF = {}


def oracle(case, key, c, inf):
    """the oracle's analysis of a case, computed once per (case key, radius, inflation) and shared, never modified"""
    full = key + (c, inf)
    if full not in _REF:
        ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, inf)[0]
        ref.setflags(write=False)
        _REF[full] = ref
    return _REF[full]


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
    assert KERNEL not in last_kernel() and "letkf_tile64" not in last_kernel()


def template_args(kern):
    """(UT, KT, NW) of a reported letkf_wide64_kernel<UT, KT, NW>"""
    m = re.match(r"letkf_wide64_kernel<(\d+), (\d+), (\d+)>$", kern)
    assert m, kern
    return tuple(int(v) for v in m.groups())


def expected_degrees64(yb, nb, inf):
    """Chebyshev degree per grid point as the float64 tile kernels choose it, restated in float64 numpy from the per-point
    lists: Gershgorin bound L of S = D G D, T = L / reg rounded up to the table's geometric grid (32 per octave, 2^-24 .. 2^8),
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


def largest_union(nb):
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    return max(len(set(np.concatenate([idx[g, :cnt[g]] for g in range(t, min(t + 16, len(cnt)))]))) for t in range(0, len(cnt), 16))


# ---- 1. the default call ------------------------------------------------------------------------------------------------------
def test_default_dtype_runs_the_wide64_kernel_at_80_members(mia, eng):
    """LETKF(localization, inf_factor) exactly as with the reference -- no dtype argument -- on the shape of BASELINE config 4
    (k = 80, an observation at every grid point, GaspariCohn(16.5)): float64, letkf_wide64_kernel<5, 5, 2>, the oracle's
    analysis to 1e-10.  "auto" takes k = 80 because the measured case is more than twice as fast as the Jacobi kernel
    (LetkfEngine.WIDE64_AUTO_*)."""
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    for name in ("mia_letkf_analysis_wide_f64", "mia_letkf_wide_f64_cover"):
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS
    case = O.synthetic_case(G, 80, 1, seed=81)
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(16.5, mia.AbsoluteDistance()), inf_factor=1.1)
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    assert xa.dtype == torch.float64
    assert last_kernel().startswith("letkf_wide64_kernel<5, 5, 2"), last_kernel()
    check(xa.cpu().numpy(), oracle(case, (80, 1, 81, 1), 16.5, 1.1), "LETKF(...) default dtype, k 80")


# ---- 2. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
# (k, stride, c, p_max, largest union of a tile)
SWEEP = [(80, 1, 16.5, 63, 78),        # config 4's shape: UT 5, three + two row blocks
         (80, 2, 30.0, 58, 65),
         (72, 1, 18.0, 69, 84),        # 84 > 80 slots: a tile in parts
         (96, 1, 21.0, 81, 96),        # exactly the 96 slots of UT 6: the boundary
         (128, 1, 25.0, 97, 112),      # UT 7, four wavefronts, KT 8
         (128, 2, 32.0, 62, 69),
         (65, 1, 14.0, 53, 68),        # ragged last member block
         (65, 4, 20.0, 20, 23)]        # UT 2 under KT 5


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k,stride,c,p_max,union", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, stride, c, p_max, union, m):
    case = O.synthetic_case(G, k, stride, seed=k + m, m=m)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == p_max and largest_union(nb) == union
    for inf in (1.0, 1.1):
        f32_first(eng)
        xa, fl, declined, kern = run64(eng, case, nb, inf, method="wide64")
        ut, kt, nw = template_args(kern)
        assert ut == min((p_max + 8 + 15) // 16, 8) and kt == (k + 15) // 16 and nw == (2 if ut <= 6 else 4), kern
        if k == 72:
            assert (ut, 16 * ut, union) == (5, 80, 84)      # the largest union does not fit the instantiation: a tile in parts
        if k == 96:
            assert (ut, 16 * ut, union) == (6, 96, 96)      # ... and here it fits exactly
        assert declined == 0
        fl = fl.cpu().numpy()
        assert int((fl & 0xff).max()) == 0
        want = expected_degrees64(case["yb"], nb, inf)
        assert int(want.max()) <= 37           # (checked on the CPU beforehand: nothing near the cap)
        assert np.array_equal((fl >> 8) & 0xff, want)
        check(xa.cpu().numpy(), oracle(case, (k, stride, k + m, m), c, inf),
              "k %d stride %d c %g m %d inf %g p_max %d union %d (%s)" % (k, stride, c, m, inf, nb.p_max, union, kern))


# ---- 3. the mathematics of letkf_tile64_kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c", [(40, 2, 18.0), (64, 1, 15.0)])
def test_same_mathematics_as_the_one_wavefront_kernel(eng, k, stride, c):
    """k <= 64: the named method against letkf_tile64_kernel.  Both within 1e-10 of the oracle and of each other, point by point.
    The chains of matrix instructions are the same, so the difference should be zero; it is printed, not asserted, because
    the compiler's contraction of the element-wise updates is not under this test's control."""
    case = O.synthetic_case(G, k, stride, seed=k, m=2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert 32 < nb.p_max <= k
    ref = oracle(case, (k, stride, k, 2), c, 1.1)
    xw, _, dw, kw = run64(eng, case, nb, 1.1, method="wide64")
    xt, _, dt, kt = run64(eng, case, nb, 1.1, method="matfun64")
    assert kw.startswith(KERNEL) and "letkf_tile64_kernel" in kt and dw == 0 and dt == 0
    check(xw.cpu().numpy(), ref, "wide64 k %d (%s)" % (k, kw))
    check(xt.cpu().numpy(), ref, "matfun64 k %d (%s)" % (k, kt))
    pp, fro = per_point(xw.cpu().numpy(), xt.cpu().numpy())
    print("[wide64] k %d: wide64 against matfun64: largest absolute difference %.3e, worst grid point %.3e"
          % (k, float((xw - xt).abs().max()), pp.max()))
    assert pp.max() <= TOL64
    # "auto" never takes the wide route here: the one-wavefront kernel has the shape
    assert "letkf_tile64_kernel" in run64(eng, case, nb, 1.1)[3]


# ---- 4. tile independence, bit for bit -----------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile(eng):
    case = O.synthetic_case(G, 80, 1, seed=21, m=2)
    c = 16.5
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    full, _, declined, kern = run64(eng, case, nb, 1.1)
    assert declined == 0 and kern.startswith(KERNEL)
    assert torch.equal(full, run64(eng, case, nb, 1.1)[0])
    assert torch.equal(full, run64(eng, case, nb, 1.1, method="wide64")[0])
    g0, g1 = 21, 150
    nbs = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
    part = run64(eng, case, nbs, 1.1)[0]
    assert part.shape[-1] == g1 - g0 and torch.equal(part, full[:, :, g0:g1])
    out = torch.full((2, 80, g1 - g0 + 9), -7.0, dtype=torch.float64, device=DEV)
    res = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nbs, 1.1, out=out, out_offset=5)
    torch.cuda.synchronize()
    assert res is out and last_kernel().startswith(KERNEL)
    assert torch.equal(out[:, :, 5:5 + g1 - g0], full[:, :, g0:g1])
    assert bool((out[:, :, :5] == -7.0).all()) and bool((out[:, :, 5 + g1 - g0:] == -7.0).all())


# ---- 5. declined points ----------------------------------------------------------------------------------------------------------
def test_a_strong_cluster_declines_exactly_the_points_above_the_cap(eng):
    """Observations 80 .. 85 scaled by 10 in config 4's network: the flagged set equals "degree from the table for this point's
    Gershgorin bound > cap", restated in float64 numpy (30 of the 203 points); the other columns of their tiles are written,
    the declined ones untouched until the Jacobi kernel's redo."""
    case = O.synthetic_case(G, 80, 1, seed=5)
    case["yb"][:, 80:86] *= 10.0
    case["d"][80:86] *= 10.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    want = expected_degrees64(case["yb"], nb, 1.1) > CAP
    assert int(want.sum()) == 30
    X = dev(case["state"])
    out = torch.full((1, 80, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = eng.analysis(X, dev(case["yb"]), dev(case["d"]), nb, 1.1, out=out, flags=fl, retry=retry, defer_retry=True,
                       method="wide64")
    torch.cuda.synchronize()
    assert last_kernel().startswith(KERNEL)
    got = (fl.cpu().numpy() & 8) != 0
    assert np.array_equal(got, want)
    assert int(retry.item()) == int(want.sum())
    wt = torch.as_tensor(want, device=DEV)
    assert bool((out[:, :, wt] == -7.0).all())                                     # declined points are left untouched
    assert bool((out[:, :, ~wt] != -7.0).all())
    assert res[-1]() == int(want.sum())                                            # the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & 8).max()) == 0                                  # the redo rewrote the flags
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 16.5, 1.1)[0]
    check(out.cpu().numpy(), ref, "strong cluster, %d points redone" % int(want.sum()))


# ---- 6. a non-finite record ------------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    case = O.synthetic_case(G, 80, 1, seed=32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    clean, _, declined, kern = run64(eng, case, nb, 1.1, method="wide64")
    assert declined == 0 and kern.startswith(KERNEL)
    j = 37
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][3, j] = np.nan
    xa, fl, declined, kern = run64(eng, bad, nb, 1.1, method="wide64")
    assert kern.startswith(KERNEL)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G
    assert np.array_equal((fl.cpu().numpy() & 4) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(xa[:, :, keep], clean[:, :, keep])


# ---- 7. the edges of the route ---------------------------------------------------------------------------------------------------
def test_shapes_outside_the_route_take_what_ran_before(eng):
    """p_max > k at k = 80, k = 129, float32, the RBF core, weights output and tile = 0: "auto" runs what it ran before this
    route existed, with the right answer; method="wide64" raises."""
    inputs = lambda case, dtype=torch.float64: (dev(case["state"], dtype), dev(case["yb"], dtype), dev(case["d"], dtype))
    # p_max > k
    case = O.synthetic_case(G, 80, 1, seed=33)
    nb = eng.localize(case["grid_x"], case["obs_x"], [25.0])
    assert nb.p_max > 80
    f32_first(eng)
    xa, _, declined, kern = run64(eng, case, nb, 1.1)
    assert KERNEL not in kern and "letkf_tile64" not in kern and declined == 0
    check(xa.cpu().numpy(), oracle(case, (80, 1, 33, 1), 25.0, 1.1), "p_max > k at k 80")
    with pytest.raises(Exception):
        run64(eng, case, nb, 1.1, method="wide64")
    # k = 129
    c129 = O.synthetic_case(G, 129, 4, seed=34)
    nb129 = eng.localize(c129["grid_x"], c129["obs_x"], [20.0])
    assert 0 < nb129.p_max <= 129
    f32_first(eng)
    xa, _, declined, kern = run64(eng, c129, nb129, 1.1)
    assert KERNEL not in kern and declined == 0
    check(xa.cpu().numpy(), oracle(c129, (129, 4, 34, 1), 20.0, 1.1), "k 129")
    with pytest.raises(Exception):
        run64(eng, c129, nb129, 1.1, method="wide64")
    # inside the cover, but not this route's: float32, the RBF core, the weights, tile = 0
    case = O.synthetic_case(G, 80, 1, seed=35)
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    ref = oracle(case, (80, 1, 35, 1), 16.5, 1.1)
    x32 = eng.analysis(*inputs(case, torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert x32.dtype == torch.float32 and KERNEL not in last_kernel()
    assert per_point(x32.double().cpu().numpy(), ref)[1] <= 1e-4              # (the float32 contract)
    with pytest.raises(ValueError):
        eng.analysis(*inputs(case, torch.float32), nb, 1.1, method="wide64")
    f32_first(eng)
    xr = eng.analysis(*inputs(case), nb, 1.1, rbf_gamma=0.5)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel()
    assert torch.equal(xr, eng.analysis(*inputs(case), nb, 1.1, rbf_gamma=0.5, method="eig"))
    with pytest.raises(ValueError):
        eng.analysis(*inputs(case), nb, 1.1, rbf_gamma=0.5, method="wide64")
    f32_first(eng)
    xw, W = eng.analysis(*inputs(case), nb, 1.1, return_weights=True)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel() and W.shape == (G, 80, 80)
    check(xw.cpu().numpy(), ref, "return_weights=True")
    with pytest.raises(ValueError):
        eng.analysis(*inputs(case), nb, 1.1, return_weights=True, method="wide64")
    xe = run64(eng, case, nb, 1.1, method="eig")[0]
    set_option("tile", 0)
    f32_first(eng)
    xo, _, _, kern = run64(eng, case, nb, 1.1)
    assert KERNEL not in kern
    assert torch.equal(xo, xe)
    check(xo.cpu().numpy(), ref, "tile = 0")
    with pytest.raises(Exception):
        run64(eng, case, nb, 1.1, method="wide64")
    set_option("tile", 1)
    xa, _, _, kern = run64(eng, case, nb, 1.1)
    assert kern.startswith(KERNEL)
    check(xa.cpu().numpy(), ref, "tile = 1 again")
    with pytest.raises(ValueError):
        run64(eng, case, nb, 1.1, method="wide")


def test_points_without_observations_get_the_inflated_prior(eng):
    case = O.synthetic_case(G, 80, 1, seed=31, m=2)
    keep = case["obs_x"] < 60
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    xa, fl, declined, kern = run64(eng, case, nb, 1.1)
    assert kern.startswith(KERNEL) and declined == 0 and int((fl & 0xff).max().item()) == 0
    far = slice(100, G)                                              # (whole tiles and parts of tiles without any observation)
    assert int(nb.cnt.cpu().numpy()[far].max()) == 0
    st = case["state"][:, :, far]
    mean = st.mean(axis=1, keepdims=True)
    check(xa.cpu().numpy()[:, :, far], mean + np.sqrt(1.1) * (st - mean), "no observations: the inflated prior")
    check(xa.cpu().numpy(), O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 16.5, 1.1)[0],
          "observations in a part of the domain")


def test_the_auto_rule_at_its_edge(eng):
    """LetkfEngine.WIDE64_AUTO_*: "auto" hands k >= 65 with up to eight state rows to the wide route and nothing else
    (k = 64 is the one-wavefront kernel's; nine rows were not measured and stay on the Jacobi kernel)."""
    assert (eng.WIDE64_AUTO_MIN_K, eng.WIDE64_AUTO_MAX_ROWS) == (65, 8)
    for k, m, wide in ((65, 1, True), (64, 1, False), (65, eng.WIDE64_AUTO_MAX_ROWS, True), (65, eng.WIDE64_AUTO_MAX_ROWS + 1, False)):
        case = O.synthetic_case(48, k, 4, seed=40 + m, m=m)
        nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
        assert 0 < nb.p_max <= k
        f32_first(eng)
        xa, _, declined, kern = run64(eng, case, nb, 1.1)
        assert kern.startswith(KERNEL) == wide, (k, m, kern)
        assert ("letkf_tile64_kernel" in kern) == (k == 64)
        xn = run64(eng, case, nb, 1.1, method="wide64")[0]                    # the named method runs it everywhere
        assert last_kernel().startswith(KERNEL)
        check(xa.cpu().numpy(), O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 20.0, 1.1)[0],
              "auto at k %d, %d rows (%s)" % (k, m, kern))
        assert per_point(xn.cpu().numpy(), xa.cpu().numpy())[0].max() <= TOL64

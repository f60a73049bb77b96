"""The float64 RBF tile route (csrc/lketkf_tile64.hip, mia_lketkf_rbf_analysis_matfun_f64): what LKETKF(RBFKernel(gamma), localization)
and LETKF-type filters with a GaussKernel run in the default working precision.  The contract is the project's float64 one
(DESIGN 8): relative Frobenius error <= 1e-10 against the golden vectors and the float64 oracle AND the worst single grid point
<= 1e-10; the reference's single KETKF blocks to the 1e-9 that test_gpu_parity.py::test_ketkf_blocks_vs_reference applies to them.
In every parity test nothing may be declined and the reported kernel is the new one, so that the Jacobi kernel cannot supply the
parity."""
import dataclasses

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
KERNEL = "lketkf_tile64"
LOG_TOL, MARGIN = 26.0, 2            # the float64 table's truncation target and margin


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
    from oracle_pool import per_point_errors
    pp, fro = per_point_errors(got, ref)
    print("\n[rbf64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= tol, what
    assert pp.max() <= tol, what


def run64(eng, case, nb, inf, gamma, method="rbf64", **kw):
    """engine.analysis in float64 with a caller-owned decline counter: (Xa, flags, declined, kernel name)"""
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xa, fl = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, inf, return_flags=True, method=method,
                          retry=retry, rbf_gamma=gamma, **kw)
    torch.cuda.synchronize()
    return xa, fl, int(retry.item()), last_kernel()


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh (letkf_wave.hip never reports one)"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel()


def rbf_core(gamma, lam=None):
    """O.ketkf_weights with O.rbf_kernel as the per-point core; ``lam`` (a list) collects the largest eigenvalue of Kc = C K C"""
    def core(a, b, inf):
        if lam is not None:
            k = a.shape[-2]
            if a.shape[-1] == 0:
                lam.append(0.0)
            else:
                K = O.rbf_kernel(a, a, gamma).numpy()
                C_ = np.eye(k) - 1.0 / k
                lam.append(float(np.linalg.eigvalsh(C_ @ K @ C_).max()))
        return O.ketkf_weights(a, b, lambda x, y: O.rbf_kernel(x, y, gamma), inf)
    return core


def oracle_weights(case, c, inf, gamma, lam=None, **kw):
    return O.letkf_weights(case.get("grid_x", case.get("grid")), case.get("obs_x", case.get("obs")), case["yb"], case["d"], c, inf,
                           core=rbf_core(gamma, lam), **kw)


def degree64(T):
    """The float64 table's degree for T = L / reg, restated: T rounded up to the geometric grid (32 per octave, 2^-24 .. 2^8),
    degree = ceil(26 / log rho) + 2, rho = (sqrt(1 + T) + 1) / (sqrt(1 + T) - 1), at least 3"""
    ti = int(np.clip(np.ceil(32 * np.log2(max(T, 1e-300))) + 24 * 32, 0, 32 * 32 - 1))
    sq = np.sqrt(1 + 2.0 ** ((ti - 24 * 32) / 32))
    return max(3, int(np.ceil(LOG_TOL / np.log((sq + 1) / max(sq - 1, 1e-12))) + MARGIN))


# ---- 1. golden ------------------------------------------------------------------------------------------------------------------
def test_core_blocks_vs_reference(eng, golden):
    """The reference's own KETKF weights (golden g4: RBF gamma 0.5 / 10, Gauss lengthscale 2 = gamma 0.125; inflation 1.0 / 1.1)
    applied to a random ensemble = the kernel's analysis of ONE grid point that sees every observation with weight 1."""
    from torch_assimilate_amd import _cabi
    g = golden("g3_g4_core_blocks.npz")
    seen = 0
    for ci, (k, p) in enumerate(g["cases"]):
        k, p = int(k), int(p)
        if not _cabi.lib().mia_lketkf_rbf_f64_cover(3, k, p, 1, 1, 1, p):
            assert k > 40 or p > 64, (k, p)
            continue
        case = dict(state=np.random.RandomState(100 + ci).normal(size=(3, k, 1)), yb=g[f"yb_{ci}"], d=g[f"d_{ci}"])
        nb = eng.localize(np.zeros(1), np.zeros(p), [5.0])
        assert nb.p_max == p
        for gname, gamma in (("rbf0p5", 0.5), ("rbf10", 10.0), ("gauss2", 0.125)):
            for inf, tag in ((1.0, "1p0"), (1.1, "1p1")):
                f32_first(eng)
                xa, fl, declined, kern = run64(eng, case, nb, inf, gamma)
                assert KERNEL in kern and declined == 0 and int((fl & 0xff).max().item()) == 0, (k, p, kern)
                ref = O.apply_weights(case["state"], g[f"ketkf_{gname}_{ci}_{tag}"][None])
                err = rel_fro(xa.cpu().numpy(), ref)
                print("\n[rbf64] golden block k %d p %d %s inf %s: %.3e" % (k, p, gname, inf, err))
                assert err <= 1e-9, (k, p, gname, tag)
                seen += 1
    assert seen == 36         # (k, p) = (10, 40), (20, 40), (40, 20), (40, 19), (40, 1), (7, 5) x 3 kernels x 2 inflations


def test_default_dtype_runs_the_rbf64_kernel_vs_golden(mia, eng, golden):
    """LKETKF(RBFKernel(0.5), localization, inf_factor) exactly as with the reference -- no dtype argument -- on the
    reference-generated config 5 (G = 256, k = 40)."""
    g = golden("g7_synthetic_configs.npz")
    for inf, tag in ((1.0, "1p0"), (1.1, "1p1")):
        f32_first(eng)
        f = mia.LKETKF(mia.RBFKernel(0.5), localization=mia.GaspariCohn(10.0, mia.AbsoluteDistance()), inf_factor=inf)
        xa = f.analyse_arrays(g["c5_state"], g["c5_yb"], g["c5_d"], grid_coords=g["c5_grid_x"], obs_coords=g["c5_obs_x"])
        assert xa.dtype == torch.float64
        assert KERNEL in last_kernel(), last_kernel()
        check(xa.cpu().numpy(), g["c5_%s_analysis" % tag], "golden config 5 inf %s" % inf)


# ---- 2. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
SWEEP = [(2, 1, 3.0), (3, 1, 3.0), (5, 1, 3.0), (8, 2, 6.0), (8, 1, 9.0), (16, 2, 6.0), (17, 1, 4.0), (20, 3, 25.0), (32, 1, 4.0),
         (37, 2, 10.0), (40, 2, 10.0), (40, 1, 15.0)]
_REF = {}


def sweep_case(k, stride, c):
    """The G = 203 case of a sweep entry (three state rows; one row = its first) and, computed once per (gamma, inf), the
    oracle's weights with the largest eigenvalue of every point's Kc."""
    key = (k, stride, c)
    if key not in _REF:
        _REF[key] = dict(case=O.synthetic_case(203, k, stride, seed=k + 3, m=3), w={})
    return _REF[key]


def sweep_ref(k, stride, c, gamma, inf):
    ent = sweep_case(k, stride, c)
    if (gamma, inf) not in ent["w"]:
        lam = []
        ent["w"][(gamma, inf)] = (oracle_weights(ent["case"], c, inf, gamma, lam), np.array(lam))
    return ent["w"][(gamma, inf)]


@pytest.mark.parametrize("k,stride,c", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, stride, c):
    """fewer pairs than one row block (k = 2, 3, 5), pair counts just across a block boundary (16, 17), p_max > k (8, 1, 9),
    unions of 74 slots that run in parts (40, 1, 15); ragged last tile (G = 203, 13 tiles), one and three state rows, three
    kernel widths, both inflations; the reported degree between the table's degree for the largest eigenvalue of Kc and for
    the row-sum bound's ceiling k."""
    case3 = sweep_case(k, stride, c)["case"]
    nb = eng.localize(case3["grid_x"], case3["obs_x"], [c])
    assert 0 < nb.p_max <= 64
    for m in (1, 3):
        case = dict(case3, state=case3["state"][:m])
        for gamma in (0.02, 0.5, 10.0):
            for inf in (1.0, 1.1):
                f32_first(eng)
                xa, fl, declined, kern = run64(eng, case, nb, inf, gamma)
                assert KERNEL in kern, kern
                assert declined == 0
                fl = fl.cpu().numpy()
                assert int((fl & 0xff).max()) == 0
                W, lam = sweep_ref(k, stride, c, gamma, inf)
                reg = (k - 1) / inf
                got = (fl >> 8) & 0xff
                lo = np.array([degree64(l / reg) for l in lam])
                hi = degree64(k * (1.0 + 1e-9) / reg)
                assert (lo <= got).all() and (got <= hi).all(), (got.min(), got.max(), lo.max(), hi)
                check(xa.cpu().numpy(), O.apply_weights(case["state"], W),
                      "k %d stride %d c %g m %d gamma %g inf %g p_max %d degrees %d..%d (%s)" % (k, stride, c, m, gamma, inf, nb.p_max,
                                                                                          got.min(), got.max(), kern))


# ---- 3. small and odd grids -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [11, 129])
def test_small_grids(eng, G):
    """G = 11: one ragged tile; G = 129: nine tiles, one point in the last"""
    case = O.synthetic_case(G, 20, 1, seed=12, m=2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [3.0])
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1, 0.5)
    assert KERNEL in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
    check(xa.cpu().numpy(), O.apply_weights(case["state"], oracle_weights(case, 3.0, 1.1, 0.5)), "G = %d" % G)


def test_two_radius_groups_and_gc_inf(eng):
    from test_gpu_tile64 import mesh_case
    case = mesh_case(20, 6, 27, 2, seed=9, m=2)
    nb = eng.localize(case["grid"], case["obs"], [3.0, 1.5], coord_group=[0, 1])
    assert 0 < nb.p_max <= 64
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, case, nb, 1.1, 0.5)
    assert KERNEL in kern and declined == 0
    check(xa.cpu().numpy(), O.apply_weights(case["state"], oracle_weights(case, [3.0, 1.5], 1.1, 0.5, coord_group=[0, 1])),
          "two radius groups")
    c1 = O.synthetic_case(150, 20, 2, seed=11)
    nb = eng.localize(c1["grid_x"], c1["obs_x"], [9.0], taper=1)
    f32_first(eng)
    xa, fl, declined, kern = run64(eng, c1, nb, 1.0, 0.5)
    assert KERNEL in kern and declined == 0
    check(xa.cpu().numpy(), O.apply_weights(c1["state"], oracle_weights(c1, 9.0, 1.0, 0.5, taper="gc_inf")), "GaspariCohnInf")


def test_periodic_metric_python_distance_and_gauss_kernel_in_the_default_dtype(mia, eng):
    """The route works from per-point lists, whatever made them: a ring with tiles at the seam (PeriodicMetric) and a host
    ``dist_func``, both through LKETKF(...) without a dtype; GaussKernel(lengthscale=2) is gamma 0.125.  (Where the issue
    speaks of "LETKF with a GaussKernel", LKETKF(GaussKernel(2.0), ...) is meant: LETKF.__init__ takes no kernel, as in the
    reference, so the kernelised class is the only way to hand one over.)"""
    G, L, c = 203, 203.0, 6.0
    case = O.synthetic_case(G, 27, 2, seed=41, m=2)

    def ring(g, o):
        dd = np.abs(np.asarray(o, dtype=np.float64).reshape(-1) - float(np.asarray(g).reshape(-1)[0]))
        return np.minimum(dd, L - dd)
    ref = O.apply_weights(case["state"], oracle_weights(case, c, 1.1, 0.5, dist_func=ring))
    f32_first(eng)
    f = mia.LKETKF(mia.RBFKernel(0.5), localization=mia.GaspariCohn(c, dist_func=mia.PeriodicMetric(L)), inf_factor=1.1)
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"], case["obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    check(xa.cpu().numpy(), ref, "PeriodicMetric ring")
    f32_first(eng)
    user = mia.GaspariCohn(c, lambda grid, obs: ring(grid, obs))
    xu = mia.LKETKF(mia.RBFKernel(0.5), localization=user, inf_factor=1.1).analyse_arrays(case["state"], case["yb"], case["d"],
                                                                                      case["grid_x"], case["obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    check(xu.cpu().numpy(), ref, "python dist_func")
    f32_first(eng)
    fg = mia.LKETKF(mia.GaussKernel(2.0), localization=mia.GaspariCohn(c, mia.AbsoluteDistance()), inf_factor=1.1)
    xg = fg.analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"], case["obs_x"])
    assert KERNEL in last_kernel(), last_kernel()
    check(xg.cpu().numpy(), O.apply_weights(case["state"], oracle_weights(case, c, 1.1, 0.125)), "GaussKernel(2)")


# ---- 4. independence, bit for bit -------------------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile(eng):
    case = dict(sweep_case(40, 2, 10.0)["case"])
    c = 10.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    full, _, declined, kern = run64(eng, case, nb, 1.1, 0.5)
    assert declined == 0 and KERNEL in kern
    assert torch.equal(full, run64(eng, case, nb, 1.1, 0.5)[0])
    g0, g1 = 37, 150
    nbs = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
    part = run64(eng, case, nbs, 1.1, 0.5)[0]
    assert part.shape[-1] == g1 - g0 and torch.equal(part, full[:, :, g0:g1])
    # the dense case: its tiles run in parts, the shard cuts them elsewhere
    cd = dict(sweep_case(40, 1, 15.0)["case"])
    fulld = run64(eng, cd, eng.localize(cd["grid_x"], cd["obs_x"], [15.0]), 1.1, 0.5)[0]
    partd = run64(eng, cd, eng.localize(cd["grid_x"], cd["obs_x"], [15.0], g0=g0, g1=g1), 1.1, 0.5)[0]
    assert torch.equal(partd, fulld[:, :, g0:g1])
    # out= with a column offset into a wider buffer
    out = torch.full((3, 40, g1 - g0 + 9), -7.0, dtype=torch.float64, device=DEV)
    res = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nbs, 1.1, rbf_gamma=0.5, method="rbf64", out=out,
                       out_offset=5)
    torch.cuda.synchronize()
    assert res is out and KERNEL in last_kernel()
    assert torch.equal(out[:, :, 5:5 + g1 - g0], full[:, :, g0:g1])
    assert bool((out[:, :, :5] == -7.0).all()) and bool((out[:, :, 5 + g1 - g0:] == -7.0).all())


# ---- 5. against the Jacobi kernel -------------------------------------------------------------------------------------------------
def test_agrees_with_the_jacobi_kernel(eng):
    case = dict(sweep_case(40, 2, 10.0)["case"])
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    xa, _, declined, kern = run64(eng, case, nb, 1.1, 0.5)
    assert KERNEL in kern and declined == 0
    f32_first(eng)
    xe, _, _, kern = run64(eng, case, nb, 1.1, 0.5, method="eig")
    assert KERNEL not in kern
    check(xa.cpu().numpy(), xe.cpu().numpy(), "rbf64 against eig")


# ---- 6. no local observations -----------------------------------------------------------------------------------------------------
def test_points_without_local_observations(eng):
    """Observations on one third of the domain only: points that see none get the prior branch of ETKFModule.forward
    (core/etkf.py:91-95: weights sqrt(inf) I, i.e. mean + sqrt(inf) x') from the same kernel, tiles that mix both kinds included.
    The branch is one multiply-add per entry: 1e-14."""
    G, k = 400, 40
    case = O.synthetic_case(G, k, 2, seed=17, m=2)
    keep = case["obs_x"] < 130.0
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    cnt = nb.cnt.cpu().numpy()
    assert any(0 < (cnt[t:t + 16] == 0).sum() < 16 for t in range(0, G, 16))          # a tile that mixes both kinds
    for inf in (1.0, 1.3):
        f32_first(eng)
        xa, fl, declined, kern = run64(eng, case, nb, inf, 0.5)
        assert KERNEL in kern and declined == 0 and int((fl & 0xff).max().item()) == 0
        check(xa.cpu().numpy(), O.apply_weights(case["state"], oracle_weights(case, 10.0, inf, 0.5)), "observations on a third, inf %g" % inf)
        far = cnt == 0
        assert far.sum() > 200
        st = case["state"][:, :, far]
        mean = st.mean(axis=1, keepdims=True)
        assert rel_fro(xa.cpu().numpy()[:, :, far], mean + np.sqrt(inf) * (st - mean)) <= 1e-14


def test_points_without_local_observations_at_a_very_large_inflation(eng):
    """inf = 200: the degree the table gives for K = 1 (T = k inf / (k - 1) = 205) is above the cap of 127.  A point without
    local observations takes the prior branch all the same -- not declined, not counted -- and does not lengthen its tile's
    recurrence; the points the kernel analyses itself match the oracle, whatever IS declined is redone by the Jacobi kernel."""
    G, k, inf = 200, 40, 200.0
    case = O.synthetic_case(G, k, 2, seed=18)
    keep = case["obs_x"] < 70.0
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    far = nb.cnt.cpu().numpy() == 0
    assert far.sum() > 90 and degree64(k * inf / (k - 1)) > 127
    out = torch.full((1, k, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, inf, rbf_gamma=0.5, method="rbf64", out=out, flags=fl,
                       retry=retry, defer_retry=True)
    torch.cuda.synchronize()
    assert KERNEL in last_kernel()
    f = fl.cpu().numpy()
    assert not (f[far] & 0xff).any()
    assert int(retry.item()) == int(((f & 0xff) == 8).sum())
    st = case["state"][:, :, far]
    mean = st.mean(axis=1, keepdims=True)
    assert rel_fro(out.cpu().numpy()[:, :, far], mean + np.sqrt(inf) * (st - mean)) <= 1e-14
    own = (f & 0xff) != 8                                   # what the kernel analysed itself, prior branch included
    assert own.sum() > far.sum()
    ref = O.apply_weights(case["state"], oracle_weights(case, 10.0, inf, 0.5))
    check(out.cpu().numpy()[:, :, own], ref[:, :, own], "inflation 200, the points the kernel analysed")
    assert res[-1]() == int((~own).sum())                   # the declined ones are the Jacobi kernel's
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not (fl.cpu().numpy() & 8).any()


# ---- 7. non-finite record and overflow ----------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    """One NaN in yb: the flagged points are EXACTLY those whose list holds the observation (the tile is analysed point by
    point), they number the decline counter and are left untouched; every other point -- those of the same tiles included --
    is finite and equals the clean run; the engine's redo hands the flagged points to the Jacobi kernel."""
    G, k, j = 640, 40, 100
    case = O.synthetic_case(G, k, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    clean = run64(eng, case, nb, 1.1, 0.5)[0]
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][5, j] = np.nan
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G and len(set(np.nonzero(uses)[0] // 16)) >= 2
    out = torch.full((1, k, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = eng.analysis(dev(bad["state"]), dev(bad["yb"]), dev(bad["d"]), nb, 1.1, rbf_gamma=0.5, method="rbf64", out=out, flags=fl,
                       retry=retry, defer_retry=True)
    torch.cuda.synchronize()
    assert KERNEL in last_kernel()
    flagged = (fl.cpu().numpy() & 0xff) == 8                 # MIA_FLAG_RETRY
    assert np.array_equal(flagged, uses)
    assert int(retry.item()) == int(uses.sum())
    keep = torch.as_tensor(~uses, device=DEV)
    assert bool((out[:, :, ~keep] == -7.0).all())            # declined points are left untouched
    assert bool(torch.isfinite(out[:, :, keep]).all())
    check(out[:, :, keep].cpu().numpy(), clean[:, :, keep].cpu().numpy(), "points that do not see the NaN record")
    assert torch.equal(out[:, :, keep], clean[:, :, keep])   # (canonical summation order: the very bits)
    assert res[-1]() == int(uses.sum())                      # the deferred redo
    torch.cuda.synchronize()
    after = fl.cpu().numpy() & 0xff
    assert int(after[~uses].max()) == 0 and not (after & 8).any()
    assert torch.equal(out[:, :, keep], clean[:, :, keep])


def test_a_list_that_does_not_fit_is_flagged_never_truncated(eng):
    case = O.synthetic_case(203, 40, 2, seed=5)
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    cnt = nb.cnt.cpu().numpy()
    small = dataclasses.replace(nb, p_max=int(cnt.max()) - 2)
    over = cnt > small.p_max
    assert 0 < over.sum() < 203
    xa, fl, declined, kern = run64(eng, case, small, 1.1, 0.5)
    assert KERNEL in kern and declined == 0
    assert np.array_equal((fl.cpu().numpy() & 0xff) == 1, over)          # MIA_FLAG_OVERFLOW
    assert bool(torch.isnan(xa[:, :, torch.as_tensor(over, device=DEV)]).all())
    full = run64(eng, case, nb, 1.1, 0.5)[0]
    ok = torch.as_tensor(~over, device=DEV)
    assert torch.equal(xa[:, :, ok], full[:, :, ok])


# ---- 8. routes ----------------------------------------------------------------------------------------------------------------------
def test_named_route_requirements_and_shapes_outside_the_cover(eng):
    from torch_assimilate_amd import _cabi
    case = dict(sweep_case(40, 2, 10.0)["case"])
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    args = (dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, 1.1)
    with pytest.raises(ValueError):
        eng.analysis(*(a.float() if torch.is_tensor(a) else a for a in args), rbf_gamma=0.5, method="rbf64")
    with pytest.raises(ValueError):
        eng.analysis(*args, rbf_gamma=0.5, method="rbf64", return_weights=True)
    with pytest.raises(ValueError):
        eng.analysis(*args, method="rbf64")
    with pytest.raises(ValueError):
        eng.analysis(*args, method="rbf64", kernel_program=[(0, 0.0)])
    # an ensemble above the cover: the named route raises, "auto" returns the oracle's answer from the Jacobi kernel
    big = O.synthetic_case(100, 48, 2, seed=8)
    nbb = eng.localize(big["grid_x"], big["obs_x"], [10.0])
    assert _cabi.lib().mia_lketkf_rbf_f64_cover(1, 48, nbb.p_max, 100, 100, 100, 50) == 0
    with pytest.raises(_cabi.MiaError):
        run64(eng, big, nbb, 1.1, 0.5)
    f32_first(eng)
    xa, _, declined, kern = run64(eng, big, nbb, 1.1, 0.5, method="auto")
    assert KERNEL not in kern and declined == 0
    check(xa.cpu().numpy(), O.apply_weights(big["state"], oracle_weights(big, 10.0, 1.1, 0.5)), "k = 48 through auto")


def test_auto_rule_and_tile_option(eng):
    """method="auto" takes the route from RBF64_AUTO_MIN_K members on, with ONE state row while p_max <= RBF64_AUTO_MAX_P and with
    up to RBF64_AUTO_MAX_ROWS state rows while p_max <= RBF64_AUTO_MAX_P_ROWS: each gate pinned on both sides, with the values
    the measurements of DESIGN 9 justify (method="rbf64" stays available on the other side).  ``p_max`` is the bound the lists
    carry: a larger one than the longest list is a valid bound, and it is what the rule looks at.  Option tile = 0 sends
    "auto" to the Jacobi kernel."""
    kmin, rows, pone, prows = eng.RBF64_AUTO_MIN_K, eng.RBF64_AUTO_MAX_ROWS, eng.RBF64_AUTO_MAX_P, eng.RBF64_AUTO_MAX_P_ROWS
    assert (kmin, rows, pone, prows) == (8, 8, 21, 20)

    def auto_kernel(k, m, p_bound=None):
        case = O.synthetic_case(96, k, 2, seed=50 + k, m=m)
        nb = eng.localize(case["grid_x"], case["obs_x"], [6.0], p_cap=72)
        assert nb.p_max <= prows
        if p_bound is not None:
            nb = dataclasses.replace(nb, p_max=p_bound)
        f32_first(eng)
        xa, _, declined, kern = run64(eng, case, nb, 1.1, 0.5, method="auto")
        assert declined == 0
        xn, _, _, named = run64(eng, case, nb, 1.1, 0.5)
        assert KERNEL in named
        check(xa.cpu().numpy(), xn.cpu().numpy(), "auto against rbf64, k %d m %d p_max %s" % (k, m, p_bound))
        return kern
    assert KERNEL in auto_kernel(kmin, 1) and KERNEL not in auto_kernel(kmin - 1, 1)
    assert KERNEL in auto_kernel(40, rows, prows) and KERNEL not in auto_kernel(40, rows + 1, prows)
    assert KERNEL in auto_kernel(40, 2, prows) and KERNEL not in auto_kernel(40, 2, prows + 1)
    assert KERNEL in auto_kernel(40, 1, pone) and KERNEL not in auto_kernel(40, 1, pone + 1)
    case = O.synthetic_case(96, 40, 2, seed=90)
    nb = eng.localize(case["grid_x"], case["obs_x"], [6.0])
    set_option("tile", 0)
    f32_first(eng)
    xo, _, _, kern = run64(eng, case, nb, 1.1, 0.5, method="auto")
    assert KERNEL not in kern
    set_option("tile", 1)
    xa, _, _, kern = run64(eng, case, nb, 1.1, 0.5, method="auto")
    assert KERNEL in kern
    check(xa.cpu().numpy(), xo.cpu().numpy(), "tile = 1 against tile = 0")


def test_weights_stay_on_the_jacobi_kernel(mia, eng, tmp_path):
    case = O.synthetic_case(96, 40, 2, seed=91)
    loc = mia.GaspariCohn(6.0, mia.AbsoluteDistance())
    ref = O.apply_weights(case["state"], oracle_weights(case, 6.0, 1.1, 0.5))
    f32_first(eng)
    f = mia.LKETKF(mia.RBFKernel(0.5), localization=loc, inf_factor=1.1, weight_save_path=str(tmp_path / "w.nc"))
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"], case["obs_x"])
    assert KERNEL not in last_kernel()
    check(xa.cpu().numpy(), ref, "weight_save_path")
    f32_first(eng)
    W = mia.LKETKF(mia.RBFKernel(0.5), localization=loc, inf_factor=1.1).estimate_weights_arrays(case["yb"], case["d"], case["grid_x"],
                                                                                              case["obs_x"])
    assert KERNEL not in last_kernel() and W.shape == (96, 40, 40)
    check(O.apply_weights(case["state"], W.cpu().numpy()), ref, "estimate_weights_arrays")

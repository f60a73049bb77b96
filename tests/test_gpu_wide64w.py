"""The float64 weights on tiles for ensembles of 65 .. 128 members (csrc/letkf_wide64w.hip, mia_letkf_weights_wide_f64,
LetkfEngine.weights_wide64): what LETKF.estimate_weights_arrays and analyse_arrays(weight_save_path=...) run in the default
working precision above 64 members.  The contract is the project's float64 one: relative Frobenius error <= 1e-10 on W
as a whole against the float64 oracle, and <= 1e-10 on the WORST SINGLE GRID POINT, || W_g - ref_g ||_F / || ref_g ||_F.  In the
shape sweep no point may be declined, so that the Jacobi kernel cannot supply the parity.

Run against a build of the commit before this route, test_the_class_takes_the_kernel fails (LetkfEngine has no
WEIGHTS_WIDE64_AUTO_MIN_K), and the calls it makes do this there: at k = 96 (p_max 81) and k = 128 (p_max 97)
estimate_weights_arrays raises MiaError (mia_letkf_analysis_packed_f64 failed with status -3: the Jacobi kernel cannot hold the
local observations); at k = 80 and 65 it returns the oracle's weights from the Jacobi kernel, which reports no kernel name."""
import functools
import re

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O
from test_gpu_wide64 import SWEEP, expected_degrees64, largest_union

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
G = 203                                        # thirteen tiles, the last one ragged
CAP = 127                                      # the float64 table's degree cap
KERNEL = "letkf_wide64w_kernel<"
# the largest degree of every SWEEP case at inflation (1.0, 1.1), from the restated rule on the CPU: nothing near the cap
SWEEP_DEGREES = [(33, 34), (32, 33), (34, 35), (35, 37), (35, 36), (30, 31), (33, 35), (24, 25)]


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


def per_point_w(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    return np.sqrt(((got - ref) ** 2).sum(axis=(1, 2))) / np.maximum(np.sqrt((ref ** 2).sum(axis=(1, 2))), 1e-300)


def check(got, ref, what):
    """W [G][k][k] against the reference: the whole and the worst single grid point"""
    pp = per_point_w(got, ref)
    fro = rel_fro(got, ref)
    worst = float(pp.max()) if pp.size else 0.0
    print("\n[wide64w] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, worst, int(pp.argmax()) if pp.size else -1))
    assert fro <= TOL64, what
    assert worst <= TOL64, what
    return fro, worst


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh (letkf_wave.hip never reports one)"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert "letkf_wide64" not in last_kernel() and "letkf_weights64" not in last_kernel()


def ww64(eng, case, nb, inf, **kw):
    """engine.weights_wide64 with its flags: (W, flags as numpy, kernel name); fails when the route refuses"""
    f32_first(eng)
    res = eng.weights_wide64(dev(case["yb"]), dev(case["d"]), nb, inf, return_flags=True, **kw)
    assert res is not None, "weights_wide64 refused the shape"
    torch.cuda.synchronize()
    return res[0], res[1].cpu().numpy(), last_kernel()


def template_args(kern):
    """(UT, KT, NW) of a reported letkf_wide64w_kernel<UT, KT, NW>"""
    m = re.match(r"letkf_wide64w_kernel<(\d+), (\d+), (\d+)>$", kern)
    assert m, kern
    return tuple(int(v) for v in m.groups())


@functools.lru_cache(maxsize=None)
def case1d(k, stride, seed, m=1):
    return O.synthetic_case(G, k, stride, seed=seed, m=m)


@functools.lru_cache(maxsize=None)
def oracle1d(k, stride, seed, c, inf, m=1):
    """the oracle's (analysis, weights) of a 1-D case, computed once and shared, never modified"""
    case = case1d(k, stride, seed, m)
    xa, W = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, inf)[:2]
    xa.setflags(write=False)
    W.setflags(write=False)
    return xa, W


def by_class(mia, eng, case, c, inf=1.1, filt=None):
    f32_first(eng)
    f = filt or mia.LETKF(localization=mia.GaspariCohn(c, mia.AbsoluteDistance()), inf_factor=inf)
    W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    torch.cuda.synchronize()
    assert W.dtype == torch.float64
    return W.cpu().numpy(), last_kernel()


# ---- 1. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c,p_max,union,degs", [s + (dg,) for s, dg in zip(SWEEP, SWEEP_DEGREES)])
def test_shape_sweep_vs_oracle(eng, k, stride, c, p_max, union, degs):
    case = case1d(k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == p_max and largest_union(nb) == union
    for inf, dmax in zip((1.0, 1.1), degs):
        W, fl, kern = ww64(eng, case, nb, inf)
        ut, kt, nw = template_args(kern)
        assert ut == min((p_max + 8 + 15) // 16, 8) and kt == (k + 15) // 16 and nw == (2 if ut <= 6 else 4), kern
        want = expected_degrees64(case["yb"], nb, inf)
        assert int(want.max()) == dmax <= CAP          # (checked on the CPU beforehand: nothing near the cap)
        assert int((fl & 0xff).max()) == 0             # nothing declined, nothing non-finite
        assert np.array_equal((fl >> 8) & 0xff, want)
        check(W.cpu().numpy(), oracle1d(k, stride, k + 1, c, inf)[1],
              "k %d stride %d c %g inf %g p_max %d union %d (%s)" % (k, stride, c, inf, p_max, union, kern))


# ---- 2. through the class in the default dtype -------------------------------------------------------------------------------------
def test_the_class_takes_the_kernel(mia, eng):
    """LETKF(...).estimate_weights_arrays without a dtype at k = 96 (p_max 81) and k = 128 (p_max 97), which the Jacobi kernel
    cannot hold, at k = 80 and at the gate: float64 weights of the oracle from letkf_wide64w_kernel.  If the gate is above 65,
    one member below it runs the Jacobi kernel with the oracle's weights."""
    kmin = mia.LetkfEngine.WEIGHTS_WIDE64_AUTO_MIN_K
    assert 65 <= kmin <= 128
    cases = [(96, 1, 21.0), (128, 1, 25.0), (80, 1, 16.5)]
    if kmin == 65:
        cases.append((65, 1, 14.0))
    for k, stride, c in cases:
        assert k >= kmin
        W, kern = by_class(mia, eng, case1d(k, stride, k + 1), c)
        assert kern.startswith(KERNEL), (k, kern)
        check(W, oracle1d(k, stride, k + 1, c, 1.1)[1], "class at k = %d (%s)" % (k, kern))
    if kmin > 65:
        for k, takes in ((kmin, True), (kmin - 1, False)):
            case = O.synthetic_case(G, k, 2, seed=51)
            W, kern = by_class(mia, eng, case, 20.0)
            assert kern.startswith(KERNEL) == takes, (k, kern)
            assert "letkf_wide64" not in kern or takes
            ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 20.0, 1.1)[1]
            check(W, ref, "class at k = %d (%s)" % (k, kern))


# ---- 3. weight_save_path -----------------------------------------------------------------------------------------------------------
def test_weight_save_path_in_the_default_dtype(mia, eng, tmp_path):
    """config 4's shape (k = 80, an observation at every grid point, GaspariCohn(16.5)) with a weight_save_path and no dtype
    argument: the file holds the oracle's weights, the analysis is the oracle's."""
    from torch_assimilate_amd import weights_io as io
    case = case1d(80, 1, 81)
    xref, wref = oracle1d(80, 1, 81, 16.5, 1.1)
    path = str(tmp_path / "w.nc")
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(16.5, mia.AbsoluteDistance()), inf_factor=1.1, weight_save_path=path)
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    torch.cuda.synchronize()
    assert last_kernel().startswith(KERNEL), last_kernel()
    assert xa.dtype == torch.float64
    from oracle_pool import per_point_errors
    pp, fro = per_point_errors(xa.cpu().numpy(), xref)
    assert fro <= TOL64 and pp.max() <= TOL64
    W, coords = io.load_weights(path)
    assert tuple(W.shape) == (G, 80, 80) and coords["grid"].tolist() == list(range(G))
    check(W.numpy(), wref, "weights file vs oracle")


# ---- 4. the weights give the wide analysis ---------------------------------------------------------------------------------------
def test_the_weights_applied_to_a_state_give_the_wide64_analysis(eng):
    from oracle_pool import per_point_errors
    case = case1d(80, 1, 21, 2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    W, fl, kern = ww64(eng, case, nb, 1.1)
    assert kern.startswith(KERNEL) and int((fl & 0xff).max()) == 0
    X = dev(case["state"])
    xw = eng.apply_local_weights(X, W)
    xm = eng.analysis(X, dev(case["yb"]), dev(case["d"]), nb, 1.1, method="wide64")
    torch.cuda.synchronize()
    assert last_kernel().startswith("letkf_wide64_kernel<")
    pp, fro = per_point_errors(xw.cpu().numpy(), xm.cpu().numpy())
    print("\n[wide64w] W applied against analysis(method='wide64'): rel. Frobenius %.3e, worst grid point %.3e" % (fro, pp.max()))
    assert fro <= TOL64 and pp.max() <= TOL64


# ---- 5. bits -----------------------------------------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile(eng):
    case = case1d(80, 1, 21)
    c = 16.5
    full, fl, kern = ww64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c]), 1.1)
    assert int((fl & 0xff).max()) == 0 and kern.startswith(KERNEL)
    again = ww64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c]), 1.1)[0]
    assert torch.equal(full, again)
    g0, g1 = 21, 150
    part = ww64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1), 1.1)[0]
    assert part.shape[0] == g1 - g0
    assert torch.equal(part, full[g0:g1])


@pytest.mark.parametrize("k,stride,c", [(40, 2, 18.0), (64, 1, 15.0)])
def test_same_mathematics_as_the_one_wavefront_kernel(eng, k, stride, c):
    """k <= 64: the named method against letkf_weights64_kernel.  Both within 1e-10 of the oracle and of each other, point by
    point; the largest difference is printed, not asserted (the compiler's contraction of the element-wise updates is not under
    this test's control)."""
    case = case1d(k, stride, k)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert 32 < nb.p_max <= k
    ref = oracle1d(k, stride, k, c, 1.1)[1]
    Ww, flw, kw = ww64(eng, case, nb, 1.1)
    f32_first(eng)
    Wt, flt = eng.weights64(dev(case["yb"]), dev(case["d"]), nb, 1.1, return_flags=True)
    torch.cuda.synchronize()
    kt = last_kernel()
    assert kw.startswith(KERNEL) and "letkf_weights64_kernel" in kt
    assert int((flw & 0xff).max()) == 0 and int((flt.cpu().numpy() & 0xff).max()) == 0
    check(Ww.cpu().numpy(), ref, "weights_wide64 k %d (%s)" % (k, kw))
    check(Wt.cpu().numpy(), ref, "weights64 k %d (%s)" % (k, kt))
    pp = per_point_w(Ww.cpu().numpy(), Wt.cpu().numpy())
    print("[wide64w] k %d: weights_wide64 against weights64: largest absolute difference %.3e, worst grid point %.3e"
          % (k, float((Ww - Wt).abs().max()), pp.max()))
    assert pp.max() <= TOL64


# ---- 6. declined points ----------------------------------------------------------------------------------------------------------
def test_a_strong_cluster_declines_exactly_the_points_above_the_cap(eng):
    """Observations 80 .. 85 scaled by 10 in config 4's network: the flagged set equals "degree from the table for this point's
    Gershgorin bound > cap", restated in float64 numpy (30 of the 203 points); the other rows of a prefilled W are written, the
    declined ones untouched until the Jacobi kernel's redo, after which W is the oracle's."""
    case = O.synthetic_case(G, 80, 1, seed=5)
    case["yb"][:, 80:86] *= 10.0
    case["d"][80:86] *= 10.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    want = expected_degrees64(case["yb"], nb, 1.1) > CAP
    assert int(want.sum()) == 30
    out = torch.full((G, 80, 80), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.weights_wide64(dev(case["yb"]), dev(case["d"]), nb, 1.1, out=out, return_flags=True, defer_retry=True)
    torch.cuda.synchronize()
    assert W is out and last_kernel().startswith(KERNEL)
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())
    before = out.clone()
    assert finish() == 30                                              # the counter, then the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & 8).max()) == 0                      # the redo rewrote the flags
    assert torch.equal(out[~sel], before[~sel])
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 16.5, 1.1)[1]
    check(out.cpu().numpy(), ref, "strong cluster, 30 points redone")


# ---- 7. the edges of the route ---------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    case = case1d(80, 1, 32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    clean = ww64(eng, case, nb, 1.1)[0]
    j = 37
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][3, j] = np.nan
    W, fl, kern = ww64(eng, bad, nb, 1.1)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G and kern.startswith(KERNEL)
    assert np.array_equal((fl & 4) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(W[keep], clean[keep])


def test_points_without_observations_get_sqrt_inf_identity(eng):
    case = O.synthetic_case(G, 80, 1, seed=31)
    keep = case["obs_x"] < 60
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    W, fl, kern = ww64(eng, case, nb, 1.1)
    assert kern.startswith(KERNEL) and int((fl & 0xff).max()) == 0
    assert int(nb.cnt.cpu().numpy()[100:].max()) == 0
    far = W.cpu().numpy()[100:]                                         # (whole tiles and parts of tiles without any observation)
    assert np.abs(far - np.sqrt(1.1) * np.eye(80)).max() <= 1e-14
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 16.5, 1.1)[1]
    check(W.cpu().numpy(), ref, "observations in a part of the domain")
    # a shard without any observation, a single ragged tile
    from torch_assimilate_amd.engine import NeighbourLists
    none = dict(yb=np.zeros((80, 0)), d=np.zeros(0))
    nb = NeighbourLists(torch.zeros(5, dtype=torch.int32, device=DEV), torch.full((5, 8), -1, dtype=torch.int32, device=DEV),
                        torch.zeros((5, 8), dtype=torch.float64, device=DEV), 8, 0, 0, 5)
    W, fl, kern = ww64(eng, none, nb, 1.1)
    assert kern.startswith(KERNEL) and W.shape == (5, 80, 80) and int((fl & 0xff).max()) == 0
    assert np.abs(W.cpu().numpy() - np.sqrt(1.1) * np.eye(80)).max() <= 1e-14


def entry_rc(eng, case, nb, k, inf=1.1, gamma=0.0):
    """mia_letkf_weights_wide_f64 itself on float64 copies of the case: its return code"""
    from torch_assimilate_amd import _cabi
    n = nb.g1 - nb.g0
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    W = torch.empty((n, k, k), dtype=torch.float64, device=DEV)
    fl = torch.zeros(n, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_letkf_weights_wide_f64(None, nb.g1, 1, k, nb.g0, nb.g1, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                                nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, inf, gamma, None, n, 0,
                                                W.data_ptr(), fl.data_ptr(), retry.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


def test_shapes_outside_the_route(mia, eng):
    """p_max > k, k = 129, float32 input, the RBF core and option tile = 0: the entry answers MIA_ERR_UNSUPPORTED (-3) and
    weights_wide64 returns None -- float32 input is refused by weights_wide64 itself, a C entry cannot see a dtype -- and the
    class still returns the oracle's weights where the Jacobi kernel can hold the shape.  out= of the wrong shape or dtype
    raises ValueError."""
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    oracle_w = lambda case, c, **kw: O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.1, **kw)[1]   # noqa: E731
    # p_max > k at k = 80: refused; through the class at a size the Jacobi kernel holds (k = 20)
    case = O.synthetic_case(G, 80, 1, seed=33)
    nb = eng.localize(case["grid_x"], case["obs_x"], [25.0])
    assert nb.p_max > 80 and lib.mia_letkf_weights_wide_f64_cover(80, nb.p_max, G, G) == 0
    assert entry_rc(eng, case, nb, 80) == -3
    assert eng.weights_wide64(dev(case["yb"]), dev(case["d"]), nb, 1.1) is None
    c20 = O.synthetic_case(100, 20, 1, seed=33)
    nb20 = eng.localize(c20["grid_x"], c20["obs_x"], [8.0])
    assert nb20.p_max > 20 and eng.weights_wide64(dev(c20["yb"]), dev(c20["d"]), nb20, 1.1) is None
    W, kern = by_class(mia, eng, c20, 8.0)
    assert "letkf_wide64" not in kern and "letkf_weights64" not in kern
    check(W, oracle_w(c20, 8.0), "p_max > k through the class")
    # k = 129
    c129 = O.synthetic_case(G, 129, 4, seed=34)
    nb129 = eng.localize(c129["grid_x"], c129["obs_x"], [20.0])
    assert 0 < nb129.p_max <= 64 and lib.mia_letkf_weights_wide_f64_cover(129, nb129.p_max, G, G) == 0
    assert entry_rc(eng, c129, nb129, 129) == -3
    assert eng.weights_wide64(dev(c129["yb"]), dev(c129["d"]), nb129, 1.1) is None
    W, kern = by_class(mia, eng, c129, 20.0)
    assert "letkf_wide64" not in kern
    check(W, oracle_w(c129, 20.0), "k = 129 through the class")
    # inside the route from here on: k = 80 on a sparse network, which the Jacobi kernel holds as well
    c80 = O.synthetic_case(G, 80, 4, seed=35)
    nb80 = eng.localize(c80["grid_x"], c80["obs_x"], [20.0])
    assert 0 < nb80.p_max <= 64
    ref80 = oracle_w(c80, 20.0)
    assert entry_rc(eng, c80, nb80, 80) == 0
    # float32 input
    assert eng.weights_wide64(dev(c80["yb"], torch.float32), dev(c80["d"], torch.float32), nb80, 1.1) is None
    # the RBF core
    assert entry_rc(eng, c80, nb80, 80, gamma=0.5) == -3
    assert eng.weights_wide64(dev(c80["yb"]), dev(c80["d"]), nb80, 1.1, rbf_gamma=0.5) is None
    core = lambda a, b, i: O.ketkf_weights(a, b, lambda x, y: O.rbf_kernel(x, y, 0.5), i)      # noqa: E731
    filt = mia.LKETKF(mia.RBFKernel(0.5), localization=mia.GaspariCohn(20.0, mia.AbsoluteDistance()), inf_factor=1.1)
    W, kern = by_class(mia, eng, c80, 20.0, filt=filt)
    assert "letkf_wide64" not in kern
    check(W, oracle_w(c80, 20.0, core=core), "RBF core through the class")
    # out= of the wrong shape or dtype
    for bad in (torch.empty((G, 80, 79), dtype=torch.float64, device=DEV), torch.empty((G - 1, 80, 80), dtype=torch.float64, device=DEV),
                torch.empty((G, 80, 80), dtype=torch.float32, device=DEV)):
        with pytest.raises(ValueError):
            eng.weights_wide64(dev(c80["yb"]), dev(c80["d"]), nb80, 1.1, out=bad)
    # the class takes the route here ...
    W, kern = by_class(mia, eng, c80, 20.0)
    assert kern.startswith(KERNEL) == (80 >= mia.LetkfEngine.WEIGHTS_WIDE64_AUTO_MIN_K)
    check(W, ref80, "k = 80 stride 4 through the class")
    # ... and not with the option tile = 0
    set_option("tile", 0)
    assert entry_rc(eng, c80, nb80, 80) == -3
    assert eng.weights_wide64(dev(c80["yb"]), dev(c80["d"]), nb80, 1.1) is None
    W, kern = by_class(mia, eng, c80, 20.0)
    assert "letkf_wide64" not in kern
    check(W, ref80, "tile = 0 through the class")

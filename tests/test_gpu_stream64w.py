"""The float64 weights on tiles for dense local networks of up to 128 members (csrc/letkf_stream64w.hip,
mia_letkf_weights_stream_f64, LetkfEngine.weights_stream64): what LETKF.estimate_weights_arrays and
analyse_arrays(weight_save_path=...) run in the default working precision where a grid point sees more observations than there are
members and the Jacobi kernel cannot hold the shape (97 .. 128 members).  The contract is the project's float64 one:
relative Frobenius error <= 1e-10 on W as a whole against the float64 oracle, and <= 1e-10 on the WORST SINGLE GRID POINT,
|| W_g - ref_g ||_F / || ref_g ||_F.  In the shape sweep no point may be declined (degrees of 54 at most against the cap 127,
restated on the CPU), so that the Jacobi kernel cannot supply the parity.

Run against a build of the commit before this route, test_the_class_takes_the_kernel fails: at k = 128 (p_max 139) and k = 113
(p_max 123) estimate_weights_arrays raises MiaError (mia_letkf_analysis_packed_f64 failed with status -3: the Jacobi kernel
cannot hold a point's two k x (k + 1) matrices from 97 members on)."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O
from torch_assimilate_amd._cabi import MiaError
from test_gpu_stream64 import SWEEP, expected_degrees64, largest_union, mesh_case, strong_cluster

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
G = 203                                        # thirteen tiles, the last one ragged
CAP = 127                                      # the float64 tables' degree cap
KERNEL = "letkf_stream64w_kernel<"


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
    print("\n[stream64w] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)"
          % (what, fro, worst, int(pp.argmax()) if pp.size else -1))
    assert fro <= TOL64, what
    assert worst <= TOL64, what
    return fro, worst


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh (letkf_wave.hip never reports one)"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert "letkf_stream64" not in last_kernel()


def ws64(eng, case, nb, inf, **kw):
    """engine.weights_stream64 with its flags: (W, flags as numpy, kernel name); fails when the route refuses"""
    f32_first(eng)
    res = eng.weights_stream64(dev(case["yb"]), dev(case["d"]), nb, inf, return_flags=True, **kw)
    assert res is not None, "weights_stream64 refused the shape"
    torch.cuda.synchronize()
    return res[0], res[1].cpu().numpy(), last_kernel()


@functools.lru_cache(maxsize=None)
def case1d(k, seed, m=1):
    return O.synthetic_case(G, k, 1, seed=seed, m=m)


@functools.lru_cache(maxsize=None)
def oracle1d(k, seed, c, inf, m=1):
    """the oracle's (analysis, weights) of a 1-D case, computed once and shared, never modified"""
    case = case1d(k, seed, m)
    xa, W = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, inf)[:2]
    xa.setflags(write=False)
    W.setflags(write=False)
    return xa, W


def by_class(mia, eng, case, c, inf=1.1, **kw):
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(c, mia.AbsoluteDistance()), inf_factor=inf, **kw)
    W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    torch.cuda.synchronize()
    return W, last_kernel()


# ---- 1. shape sweep against the oracle, every point, nothing declined ------------------------------------------------------------
@pytest.mark.parametrize("k,c,p_max,union", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, c, p_max, union):
    case = case1d(k, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == p_max and p_max > k and largest_union(nb) == union
    for inf in (1.0, 1.1):
        want = expected_degrees64(case["yb"], nb, inf)
        assert int(want.max()) <= 54 < CAP              # (on the CPU beforehand: nothing near the cap)
        W, fl, kern = ws64(eng, case, nb, inf)
        assert kern == "letkf_stream64w_kernel<%d>" % ((k + 15) // 16), kern
        assert int((fl & 0xff).max()) == 0              # nothing declined, nothing non-finite
        assert np.array_equal((fl >> 8) & 0xff, want)
        check(W.cpu().numpy(), oracle1d(k, k + 1, c, inf)[1], "k %d c %g inf %g p_max %d union %d (%s)" % (k, c, inf, p_max, union, kern))


# ---- 2. through the class in the default dtype -------------------------------------------------------------------------------------
def test_the_class_takes_the_kernel(mia, eng):
    """LETKF(...).estimate_weights_arrays without a dtype at k = 128 (p_max 139) and k = 113 (p_max 123), which the Jacobi
    kernel cannot hold: float64 weights of the oracle from letkf_stream64w_kernel.  At k = 80 (p_max 93) the weights are the
    oracle's whichever kernel the rule chose; at k = 20 a dense network stays on the Jacobi kernel."""
    for k, c in ((128, 36.0), (113, 32.0)):
        W, kern = by_class(mia, eng, case1d(k, k + 1), c)
        assert W.dtype == torch.float64 and kern == "letkf_stream64w_kernel<8>", (k, kern)
        check(W.cpu().numpy(), oracle1d(k, k + 1, c, 1.1)[1], "class at k = %d (%s)" % (k, kern))
    W, kern = by_class(mia, eng, case1d(80, 81), 24.0)
    assert kern.startswith(KERNEL) == eng._weights_stream64_auto(80, 93), kern
    check(W.cpu().numpy(), oracle1d(80, 81, 24.0, 1.1)[1], "class at k = 80 (%s)" % kern)
    case = O.synthetic_case(G, 20, 1, seed=20)
    assert eng.localize(case["grid_x"], case["obs_x"], [8.0]).p_max > 20
    W, kern = by_class(mia, eng, case, 8.0)
    assert not eng._weights_stream64_auto(20, 29) and "letkf_stream64" not in kern, kern
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], 8.0, 1.1)[1]
    assert ref.shape == (G, 20, 20)
    check(W.cpu().numpy(), ref, "class at k = 20, dense (%s)" % kern)


# ---- 3. weight_save_path -----------------------------------------------------------------------------------------------------------
def test_weight_save_path_in_the_default_dtype(mia, eng, tmp_path):
    """k = 128, p_max 139 with a weight_save_path and no dtype argument: the file holds the oracle's weights, the analysis is
    the oracle's (MiaError before this route)."""
    from oracle_pool import per_point_errors
    from torch_assimilate_amd import weights_io as io
    case = case1d(128, 129)
    xref, wref = oracle1d(128, 129, 36.0, 1.1)
    path = str(tmp_path / "w.nc")
    f32_first(eng)
    f = mia.LETKF(localization=mia.GaspariCohn(36.0, mia.AbsoluteDistance()), inf_factor=1.1, weight_save_path=path)
    xa = f.analyse_arrays(case["state"], case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    torch.cuda.synchronize()
    assert last_kernel() == "letkf_stream64w_kernel<8>", last_kernel()
    assert xa.dtype == torch.float64
    pp, fro = per_point_errors(xa.cpu().numpy(), xref)
    print("\n[stream64w] analysis through the weights file: rel. Frobenius %.3e, worst grid point %.3e" % (fro, pp.max()))
    assert fro <= TOL64 and pp.max() <= TOL64
    W, coords = io.load_weights(path)
    assert tuple(W.shape) == (G, 128, 128) and coords["grid"].tolist() == list(range(G))
    check(W.numpy(), wref, "weights file vs oracle")


# ---- 4. the weights give the analysis --------------------------------------------------------------------------------------------
def test_the_weights_applied_to_a_state_give_the_stream64_analysis(eng):
    from oracle_pool import per_point_errors
    case = case1d(80, 21, 2)
    nb = eng.localize(case["grid_x"], case["obs_x"], [24.0])
    assert nb.p_max == 93
    W, fl, kern = ws64(eng, case, nb, 1.1)
    assert kern == "letkf_stream64w_kernel<5>" and int((fl & 0xff).max()) == 0
    X, Yb, d = dev(case["state"]), dev(case["yb"]), dev(case["d"])
    xw = eng.apply_local_weights(X, W)
    xm = eng.analysis(X, Yb, d, nb, 1.1, method="stream64")
    torch.cuda.synchronize()
    assert last_kernel().startswith("letkf_stream64_kernel<")
    pp, fro = per_point_errors(xw.cpu().numpy(), xm.cpu().numpy())
    print("\n[stream64w] W applied against analysis(method='stream64'): rel. Frobenius %.3e, worst grid point %.3e" % (fro, pp.max()))
    assert fro <= TOL64 and pp.max() <= TOL64
    We = eng.analysis(X, Yb, d, nb, 1.1, method="eig", return_weights=True)[1]
    torch.cuda.synchronize()
    check(W.cpu().numpy(), We.cpu().numpy(), "against the Jacobi kernel's weights at k = 80")


# ---- 5. bits -----------------------------------------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile_or_shard(eng):
    """Sub-ranges that start at 0, 5, 16 and 37, two shards, and a second call, against the full call, bit for bit.  Every range
    holds interior points (93 observations > 80 members), so every part runs on this kernel."""
    case = case1d(80, 21)
    c = 24.0
    full, fl, kern = ws64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c]), 1.1)
    assert int((fl & 0xff).max()) == 0 and kern.startswith(KERNEL)
    again = ws64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c]), 1.1)[0]
    assert torch.equal(full, again)
    for g0, g1 in ((0, 120), (5, 200), (16, 64), (37, G), (0, 101), (101, G)):
        nbp = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
        assert nbp.p_max > 80, (g0, g1)
        part, flp, kern = ws64(eng, case, nbp, 1.1)
        assert kern.startswith(KERNEL) and int((flp & 0xff).max()) == 0, (g0, g1, kern)
        assert part.shape[0] == g1 - g0
        assert torch.equal(part, full[g0:g1]), (g0, g1)


# ---- 6. tiles in parts -------------------------------------------------------------------------------------------------------------
def test_mesh_2d_with_observations_everywhere(eng):
    """An 18 x 18 mesh in row-major order with an observation at every point, radius 3, 80 members: p_max 101, sixteen
    consecutive points see 200 observations -- the launch takes ceil((101 + 16) / 16) = 8 blocks = 128 slots, so the tiles are
    done in halves."""
    case = mesh_case(18, 18, 80, 1, seed=8)
    nb = eng.localize(case["grid"], case["obs"], [3.0])
    assert nb.p_max == 101 and largest_union(nb) == 200
    assert 16 * ((nb.p_max + 31) >> 4) < 200
    want = expected_degrees64(case["yb"], nb, 1.1)
    assert int(want.max()) <= CAP
    W, fl, kern = ws64(eng, case, nb, 1.1)
    assert kern == "letkf_stream64w_kernel<5>" and int((fl & 0xff).max()) == 0
    assert np.array_equal((fl >> 8) & 0xff, want)
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], 3.0, 1.1)[1]
    check(W.cpu().numpy(), ref, "18 x 18 mesh, k 80, c 3")


# ---- 7. declined points ----------------------------------------------------------------------------------------------------------
def test_a_strong_cluster_is_declined_and_redone_at_80_members(eng):
    case = case1d(80, 21)
    nb = eng.localize(case["grid_x"], case["obs_x"], [24.0])
    strong, want = strong_cluster(case, nb, 1.1)
    n_decl = int(want.sum())
    assert 0 < n_decl < G                          # (the CPU restatement first: the cluster's points and no others)
    out = torch.full((G, 80, 80), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.weights_stream64(dev(strong["yb"]), dev(strong["d"]), nb, 1.1, out=out, return_flags=True, defer_retry=True)
    torch.cuda.synchronize()
    assert W is out and last_kernel().startswith(KERNEL)
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())     # declined blocks are left untouched
    before = out.clone()
    assert finish() == n_decl                                                         # the counter, then the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & 8).max()) == 0                                     # the redo rewrote the flags
    assert torch.equal(out[~sel], before[~sel])                                       # ... and nothing else
    ref = O.letkf_analysis(strong["state"], strong["grid_x"], strong["obs_x"], strong["yb"], strong["d"], 24.0, 1.1)[1]
    check(out.cpu().numpy(), ref, "strong cluster, %d points redone" % n_decl)


def test_a_declined_point_raises_at_128_members_after_the_others_are_written(eng):
    """The redo is the Jacobi kernel's, which cannot hold 128 members: MiaError, data-dependent, AFTER every other point has been
    written (as 2.17)."""
    case = case1d(128, 23)
    nb = eng.localize(case["grid_x"], case["obs_x"], [36.0])
    strong, want = strong_cluster(case, nb, 1.1)
    n_decl = int(want.sum())
    assert 0 < n_decl < G
    out = torch.full((G, 128, 128), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.weights_stream64(dev(strong["yb"]), dev(strong["d"]), nb, 1.1, out=out, return_flags=True, defer_retry=True)
    torch.cuda.synchronize()
    assert last_kernel() == "letkf_stream64w_kernel<8>"
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    with pytest.raises(MiaError, match="status -3"):
        finish()
    torch.cuda.synchronize()
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all())
    ref = O.letkf_analysis(strong["state"], strong["grid_x"], strong["obs_x"], strong["yb"], strong["d"], 36.0, 1.1)[1]
    check(out.cpu().numpy()[~want], ref[~want], "k 128: the %d points that were not declined" % int((~want).sum()))


# ---- 8. the edges of the route ---------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    case = case1d(65, 32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    clean, flc, kern = ws64(eng, case, nb, 1.1)
    assert kern.startswith(KERNEL) and int((flc & 0xff).max()) == 0
    j = 77
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][3, j] = np.nan
    W, fl, kern = ws64(eng, bad, nb, 1.1)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G and kern.startswith(KERNEL)
    assert np.array_equal((fl & 4) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(W[keep], clean[keep])


def test_points_without_observations_get_sqrt_inf_identity(eng):
    """The observations around a stretch of the grid removed (65 members, c = 18: a list holds up to 69 observations, the
    points 106 .. 135 none): whole tiles and parts of tiles without any observation get sqrt(inf) I exactly and flag 0; their
    neighbours have the oracle's weights and, in a shard that ends before the stretch, the same bits."""
    k, c, inf = 65, 18.0, 1.1
    case = case1d(k, 31)
    keep = (case["obs_x"] < 72) | (case["obs_x"] >= 170)
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 69 > k
    cnt = nb.cnt.cpu().numpy()
    far = cnt == 0
    first, n_far = int(far.argmax()), int(far.sum())
    assert n_far >= 17 and first % 16 != 0 and cnt[first - 1] > 0 and cnt[first + n_far] > 0 and far[first:first + n_far].all()
    W, fl, kern = ws64(eng, case, nb, inf)
    assert kern == "letkf_stream64w_kernel<5>" and int((fl & 0xff).max()) == 0
    eye = (math.sqrt(inf) * torch.eye(k, dtype=torch.float64, device=DEV)).expand(n_far, k, k)
    assert torch.equal(W[first:first + n_far], eye)
    assert int(np.abs(fl[far]).max()) == 0 and int(fl[~far].min()) > 0
    assert np.array_equal((fl[~far] >> 8) & 0xff, expected_degrees64(case["yb"], nb, inf)[~far])
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, inf)[1]
    check(W.cpu().numpy(), ref, "observations removed around a stretch of the grid")
    # the neighbours: a shard that ends with the last point that has observations holds the same bits
    nbp = eng.localize(case["grid_x"], case["obs_x"], [c], g0=5, g1=first)
    assert nbp.p_max == 69
    part = ws64(eng, case, nbp, inf)[0]
    assert torch.equal(part, W[5:first])


def entry_rc(eng, yb, d, nb, k, inf=1.1, gamma=0.0):
    """mia_letkf_weights_stream_f64 itself on float64 copies: its return code"""
    from torch_assimilate_amd import _cabi
    n = nb.g1 - nb.g0
    rec = eng.pack_obs(dev(yb), dev(d), torch.float64)
    W = torch.zeros((n, k, k), dtype=torch.float64, device=DEV)
    fl = torch.zeros(n, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_letkf_weights_stream_f64(None, nb.g1, 1, k, nb.g0, nb.g1, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                                   nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, inf, gamma, None, n, 0,
                                                   W.data_ptr(), fl.data_ptr(), retry.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


# ---- 9. outside the route --------------------------------------------------------------------------------------------------------
def test_outside_the_route(mia, eng):
    # p_max <= k: the dual routes'; through the class it is letkf_wide64w_kernel's, as before
    case = case1d(80, 81)
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    assert nb.p_max <= 80
    Yb, d = dev(case["yb"]), dev(case["d"])
    assert eng.weights_stream64(Yb, d, nb, 1.1) is None and entry_rc(eng, case["yb"], case["d"], nb, 80) == -3
    W, kern = by_class(mia, eng, case, 16.5)
    assert kern.startswith("letkf_wide64w_kernel<"), kern
    check(W.cpu().numpy(), oracle1d(80, 81, 16.5, 1.1)[1], "class at k = 80, p_max <= k (%s)" % kern)
    # inside the route: float32 input, rbf_gamma and the option tile = 0
    nb = eng.localize(case["grid_x"], case["obs_x"], [24.0])
    assert nb.p_max == 93
    assert eng.weights_stream64(Yb.float(), d.float(), nb, 1.1) is None
    assert eng.weights_stream64(Yb, d, nb, 1.1, rbf_gamma=0.5) is None and entry_rc(eng, case["yb"], case["d"], nb, 80, gamma=0.5) == -3
    assert entry_rc(eng, case["yb"], case["d"], nb, 80) == 0
    set_option("tile", 0)
    assert eng.weights_stream64(Yb, d, nb, 1.1) is None and entry_rc(eng, case["yb"], case["d"], nb, 80) == -3
    W, kern = by_class(mia, eng, case, 24.0)           # the class with tile = 0: the Jacobi kernel, as before
    assert "letkf_stream64" not in kern
    check(W.cpu().numpy(), oracle1d(80, 81, 24.0, 1.1)[1], "class at k = 80 with tile = 0 (%s)" % kern)
    set_option("tile", -1)
    # float32 through the class: float32 weights from the float32 kernels, as before
    W, kern = by_class(mia, eng, case, 24.0, dtype=torch.float32)
    assert W.dtype == torch.float32 and "letkf_stream64" not in kern
    # k = 129
    case = O.synthetic_case(G, 129, 1, seed=129)
    nb = eng.localize(case["grid_x"], case["obs_x"], [36.0])
    assert nb.p_max == 139
    assert eng.weights_stream64(dev(case["yb"]), dev(case["d"]), nb, 1.1) is None
    assert entry_rc(eng, case["yb"], case["d"], nb, 129) == -3
    with pytest.raises(MiaError, match="status -3"):   # ... and the class raises, as before
        by_class(mia, eng, case, 36.0)

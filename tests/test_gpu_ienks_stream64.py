"""The float64 IEnKS weight update with tau = 1 on tiles for DENSE local networks of up to 128 members
(csrc/lienks_stream64.hip, mia_lienks_update_stream_f64, LetkfEngine.ienks_update(method="stream64")): what
LocalizedIEnKSTransform / LocalizedIEnKSBundle.inner_loop run per grid point in the reference's default working precision where
a grid point sees more observations than there are members.  The contract is the project's float64 one: relative
Frobenius error <= 1e-10 on W as a whole against O.lienks_weights and <= 1e-10 on the WORST SINGLE GRID POINT.  Every test
asserts that lienks_stream64_kernel ran; in the shape sweep no point may carry a flag byte, so that the general kernel -- which
cannot hold most of these shapes anyway -- cannot supply the parity.

The general kernel's limits (LDS by the formula of csrc/ienks.hip against 162 816 bytes, tau = 1):

    k    p_max   bundle             transform
    65   77      117 648 ok         159 536 ok
    72   77      136 384 ok         183 200 -3
    80   93      172 496 -3         234 992 -3
    96   107     242 480 -3         328 080 -3
    128  139     422 432 -3         569 216 -3
    128  203     490 784 -3         705 152 -3

On a build of the commit before this route the class tests fail: LocalizedIEnKSBundle(dtype=torch.float64) raises MiaError
(mia_lienks_update_f64 failed with status -3) in its first inner loop at k = 96 / p_max 107 and k = 128 / p_max 139,
LocalizedIEnKSTransform does at k = 80 / p_max 93 and IEnKSBundleModule at k = 96 with 120 observations; ienks_update knows no
method "stream64"."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O
from test_gpu_ienks64 import weights_in
from test_gpu_ienks_wide64 import toy_loop
from test_gpu_stream64 import SWEEP, expected_degrees64, largest_union, strong_cluster

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
G = 203                                        # thirteen tiles, the last one ragged
CAP = 127                                      # the float64 tables' degree cap
KERNEL = "lienks_stream64_kernel<"
GENERAL = "ienks_update_kernel<double, 256>"
EPS = 1e-3
RETRY, NONFINITE, OVERFLOW = 8, 4, 1
VARIANTS = (("bundle", EPS, EPS), ("transform", None, 1.0))


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.require(a, requirements="CW"), dtype=dtype, device=DEV)      # (a copy of a read-only array)


def last_kernel():
    from torch_assimilate_amd import _cabi
    return _cabi.last_analysis_kernel()


def kname(k):
    return "lienks_stream64_kernel<%d>" % ((k + 15) // 16)


def per_point_w(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    return np.sqrt(((got - ref) ** 2).sum(axis=(1, 2))) / np.maximum(np.sqrt((ref ** 2).sum(axis=(1, 2))), 1e-300)


def check(got, ref, what, tol=TOL64):
    """W [G][k][k] against the reference: the whole and the worst single grid point"""
    pp = per_point_w(got, ref)
    fro = rel_fro(got, ref)
    worst = float(pp.max()) if pp.size else 0.0
    print("\n[ienks_stream64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)"
          % (what, fro, worst, int(pp.argmax()) if pp.size else -1))
    assert fro <= tol, what
    assert worst <= tol, what
    return fro, worst


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert "lienks" not in last_kernel() and "ienks_update_kernel" not in last_kernel()


def upd(eng, w_in, yb, d, nb, eps, method="stream64", **kw):
    """engine.ienks_update with its flags: (W, flags as numpy, kernel name)"""
    f32_first(eng)
    res = eng.ienks_update(dev(w_in), dev(yb), dev(d), nb, 1.0, eps, return_flags=True, method=method, **kw)
    torch.cuda.synchronize()
    return res[0], res[1].cpu().numpy(), last_kernel()


@functools.lru_cache(maxsize=None)
def case1d(k, seed):
    return O.synthetic_case(G, k, 1, seed=seed)           # (shared: the tests copy before they change a record)


@functools.lru_cache(maxsize=None)
def w_in1d(k, seed, bundle):
    return weights_in(G, k, seed, bundle)                  # (shared: a test that changes an element copies first)


@functools.lru_cache(maxsize=None)
def oracle1d(k, seed, c, variant, wseed):
    """the oracle's update of a 1-D case from the per-point weights w_in1d(k, wseed, .), computed once and shared, never modified.
    Bundle: the records are Yb eps, so that D = Yl / eps is the case's own Yb."""
    case = case1d(k, seed)
    eps, scale = (EPS, EPS) if variant == "bundle" else (None, 1.0)
    W = O.lienks_weights(w_in1d(k, wseed, eps is not None), case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
    W.setflags(write=False)
    return W


# ---- 1. shape sweep against the oracle, both variants, nothing flagged ----------------------------------------------------------
@pytest.mark.parametrize("k,c,p_max,union", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, c, p_max, union):
    """k 40 .. 128, p_max 77 .. 203, KT 3 .. 8, a ragged last member block at 65 and 113, tiles in halves at p_max 173 and 203;
    per-point incoming weights.  The degrees are the restated rule's at inflation 1 (the bundle variant's bound is that of
    D = Yl / eps, the case's own Yb) and no point carries a flag byte: the parity is the tile kernel's own."""
    case = case1d(k, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == p_max and p_max > k and largest_union(nb) == union
    want = expected_degrees64(case["yb"], nb, 1.0)
    assert int(want.max()) <= 54 < CAP                  # (on the CPU beforehand: nothing near the cap)
    for vname, eps, scale in VARIANTS:
        W, fl, kern = upd(eng, w_in1d(k, k, eps is not None), case["yb"] * scale, case["d"], nb, eps)
        assert kern == kname(k), kern
        assert int((fl & 0xff).max()) == 0, vname       # nothing declined, nothing non-finite
        assert np.array_equal((fl >> 8) & 0xff, want), vname
        check(W.cpu().numpy(), oracle1d(k, k + 1, c, vname, k),
              "%s k %d c %g p_max %d union %d (%s)" % (vname, k, c, p_max, union, kern))


# ---- 2. one shared matrix --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c", [(80, 24.0), (128, 36.0)])
def test_one_shared_matrix(eng, k, c):
    """ONE (k, k) matrix for all points (w_stride = 0): the prior of the first iteration in both variants, and a matrix with
    another mean and another Wp in the bundle variant."""
    case = case1d(k, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max > k
    for vname, eps, scale in VARIANTS:
        W, fl, kern = upd(eng, np.eye(k), case["yb"] * scale, case["d"], nb, eps)
        assert kern == kname(k) and int((fl & 0xff).max()) == 0
        ref = O.lienks_weights(np.eye(k), case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, shared prior, k %d (%s)" % (vname, k, kern))
    w1 = weights_in(1, k, 5, True)[0]
    W, fl, kern = upd(eng, w1, case["yb"] * EPS, case["d"], nb, EPS)
    assert kern == kname(k) and int((fl & 0xff).max()) == 0
    check(W.cpu().numpy(), O.lienks_weights(w1, case["grid_x"], case["obs_x"], case["yb"] * EPS, case["d"], c, 1.0, EPS),
          "bundle, one shared non-prior matrix, k %d" % k)


# ---- 3. chain --------------------------------------------------------------------------------------------------------------------
def test_three_bundle_iterations_vs_three_oracle_iterations(eng):
    """k = 128 with 139 local observations, which the general kernel cannot hold.  The map from the incoming w_mean to W' is a
    contraction (|| psi(C) C || < 1): errors do not grow along the chain, the bar stays 1e-10."""
    k, c = 128, 36.0
    case = case1d(k, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 139
    yb = case["yb"] * EPS
    w, ref = np.eye(k), np.eye(k)
    for it in range(3):
        W, fl, kern = upd(eng, w, yb, case["d"], nb, EPS)
        assert kern == kname(k) and int((fl & 0xff).max()) == 0
        w = W.cpu().numpy()
        ref = O.lienks_weights(ref, case["grid_x"], case["obs_x"], yb, case["d"], c, 1.0, EPS)
        check(w, ref, "bundle chain at k = 128, iteration %d" % it)


# ---- 4. through the classes, no method named ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c,p_max", [(96, 28.0, 107), (128, 36.0, 139)])
def test_the_bundle_class_on_dense_networks(mia, eng, k, c, p_max):
    """LocalizedIEnKSBundle(dtype=torch.float64) with no method named, at shapes the general kernel cannot hold: inner_loop_arrays
    and a three-iteration update_state_arrays return the oracle's result from lienks_stream64_kernel (MiaError before this route)."""
    assert not eng._ienks_general_fits(k, p_max, 1.0, True) and eng._ienks_stream64_auto(k, p_max, True, False)
    state, gx, ox, forward_model, observe, reference = toy_loop(k)
    a = mia.LocalizedIEnKSBundle(forward_model, mia.GaspariCohn(c, mia.AbsoluteDistance()), max_iter=3, tau=1.0, epsilon=EPS,
                                 dtype=torch.float64)
    case = case1d(k, k + 1)
    assert eng.localize(case["grid_x"], case["obs_x"], [c]).p_max == p_max
    f32_first(eng)
    W = a.inner_loop_arrays(np.array(w_in1d(k, k, True)), case["yb"] * EPS, case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    torch.cuda.synchronize()
    assert last_kernel() == kname(k), last_kernel()
    assert W.dtype == torch.float64
    check(W.cpu().numpy(), oracle1d(k, k + 1, c, "bundle", k), "LocalizedIEnKSBundle.inner_loop_arrays at k = %d" % k)
    f32_first(eng)
    xa = a.update_state_arrays(state, observe, grid_coords=gx, obs_coords=ox)
    torch.cuda.synchronize()
    assert last_kernel() == kname(k), last_kernel()
    ref = reference(EPS, 3, c)[0]
    err = rel_fro(xa.cpu().numpy(), ref)
    print("\n[ienks_stream64] LocalizedIEnKSBundle, three iterations at k = %d: analysis rel. Frobenius %.3e" % (k, err))
    assert xa.dtype == torch.float64 and err <= TOL64


def test_the_transform_class_runs_its_first_iteration_here(mia, eng):
    """LocalizedIEnKSTransform(max_iter=1) at k = 80 with 93 local observations, which the general kernel cannot hold: the first
    iteration, from the prior, is this kernel's."""
    k, c = 80, 24.0
    state, gx, ox, forward_model, observe, reference = toy_loop(k)
    a = mia.LocalizedIEnKSTransform(forward_model, mia.GaspariCohn(c, mia.AbsoluteDistance()), max_iter=1, tau=1.0,
                                    dtype=torch.float64)
    assert eng.localize(gx, ox, [c]).p_max == 93 and eng._ienks_stream64_auto(k, 93, False, True)
    xref, wref, yb, d = reference(None, 1, c)
    f32_first(eng)
    W = a.inner_loop_arrays(np.eye(k), yb, d, grid_coords=gx, obs_coords=ox)
    torch.cuda.synchronize()
    assert last_kernel() == kname(k), last_kernel()
    check(W.cpu().numpy(), wref, "LocalizedIEnKSTransform.inner_loop_arrays from the prior at k = 80")
    f32_first(eng)
    xa = a.update_state_arrays(state, observe, grid_coords=gx, obs_coords=ox)
    torch.cuda.synchronize()
    assert last_kernel() == kname(k), last_kernel()
    assert rel_fro(xa.cpu().numpy(), xref) <= TOL64


def test_the_one_block_module_takes_the_kernel_where_the_general_kernel_cannot(mia, eng):
    """IEnKSBundleModule at k = 96 with 120 observations, ONE block that sees them all (what IEnKSBundle runs): one tile with one
    point, against O.ienks_update."""
    k, p = 96, 120
    rs = np.random.RandomState(96)
    yb, d = rs.normal(size=(k, p)), rs.normal(size=p)
    yb -= yb.mean(axis=0)
    w_in = weights_in(1, k, 7, True)[0]
    assert not eng._ienks_general_fits(k, p, 1.0, True)
    mod = mia.IEnKSBundleModule(EPS, 1.0, eng)
    f32_first(eng)
    W = mod(dev(w_in), dev(yb * EPS), dev(d))
    torch.cuda.synchronize()
    assert last_kernel() == kname(k), last_kernel()
    ref = O.ienks_update(w_in, yb * EPS, d, 1.0, EPS).numpy()
    check(W.cpu().numpy()[None], ref[None], "IEnKSBundleModule, k 96, 120 observations in one block")


def test_where_the_general_kernel_holds_the_shape_the_gate_decides(mia, eng):
    """k = 65 / p_max 77, which the general kernel holds in both variants: the oracle's result whichever kernel the gate chose.
    At k = 20 a dense network stays on the general kernel."""
    k, c = 65, 20.0
    case = case1d(k, k + 1)
    a = mia.LocalizedIEnKSBundle(lambda x, it: (x, x), mia.GaspariCohn(c, mia.AbsoluteDistance()), tau=1.0, epsilon=EPS,
                                 dtype=torch.float64)
    assert eng.localize(case["grid_x"], case["obs_x"], [c]).p_max == 77
    f32_first(eng)
    W = a.inner_loop_arrays(np.array(w_in1d(k, k, True)), case["yb"] * EPS, case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    torch.cuda.synchronize()
    kern = last_kernel()
    assert kern.startswith(KERNEL) == eng._ienks_stream64_auto(k, 77, True, False), kern
    assert kern.startswith(KERNEL) or GENERAL in kern, kern
    check(W.cpu().numpy(), oracle1d(k, k + 1, c, "bundle", k), "class at k = 65 (%s)" % kern,
          tol=TOL64 if kern.startswith(KERNEL) else 1e-9)
    c20 = O.synthetic_case(G, 20, 1, seed=20)
    p20 = eng.localize(c20["grid_x"], c20["obs_x"], [8.0]).p_max
    assert p20 > 20
    a20 = mia.LocalizedIEnKSBundle(lambda x, it: (x, x), mia.GaspariCohn(8.0, mia.AbsoluteDistance()), tau=1.0, epsilon=EPS,
                                   dtype=torch.float64)
    w20 = weights_in(G, 20, 20, True)
    f32_first(eng)
    W = a20.inner_loop_arrays(w20, c20["yb"] * EPS, c20["d"], grid_coords=c20["grid_x"], obs_coords=c20["obs_x"])
    torch.cuda.synchronize()
    assert not eng._ienks_stream64_auto(20, 29, True, False) and not eng._ienks_stream64_auto(20, p20, True, False)
    assert GENERAL in last_kernel(), last_kernel()
    ref = O.lienks_weights(w20, c20["grid_x"], c20["obs_x"], c20["yb"] * EPS, c20["d"], 8.0, 1.0, EPS)
    check(W.cpu().numpy(), ref, "class at k = 20, dense (general kernel)", tol=1e-9)


# ---- 5. bits -----------------------------------------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile_or_shard(eng):
    """Sub-ranges that start at 0, 5, 16 and 37, two shards, and a second call, against the full call, bit for bit, in both
    variants.  Every range holds interior points (93 observations > 80 members), so every part runs on this kernel."""
    k, c = 80, 24.0
    case = case1d(k, 21)
    for vname, eps, scale in VARIANTS:
        w_in = w_in1d(k, 9, eps is not None)
        yb = case["yb"] * scale

        def run(g0, g1):
            nb = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
            assert nb.p_max > k, (g0, g1)
            W, fl, kern = upd(eng, w_in[g0:g1], yb, case["d"], nb, eps)
            assert kern == kname(k) and int((fl & 0xff).max()) == 0, (vname, g0, g1, kern)
            assert W.shape[0] == g1 - g0
            return W
        full = run(0, G)
        assert torch.equal(full, run(0, G)), vname
        for g0, g1 in ((0, 120), (5, 200), (16, 64), (37, G), (0, 101), (101, G)):
            assert torch.equal(run(g0, g1), full[g0:g1]), (vname, g0, g1)


# ---- 6. cross-checks ---------------------------------------------------------------------------------------------------------------
def test_the_prior_in_the_transform_variant_gives_the_letkf_weights_at_inflation_1(eng):
    """W_in = I (w_mean = 0, no shift): the update is the LETKF weights at inflation 1, letkf_stream64w_kernel's.  Within 1e-10
    point by point; the largest difference is printed, not asserted (the two kernels' element-wise updates are contracted by the
    compiler independently)."""
    k, c = 80, 24.0
    case = case1d(k, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    W, fl, kern = upd(eng, np.eye(k), case["yb"], case["d"], nb, None)
    assert kern == kname(k) and int((fl & 0xff).max()) == 0
    f32_first(eng)
    Ww, flw = eng.weights_stream64(dev(case["yb"]), dev(case["d"]), nb, 1.0, return_flags=True)
    torch.cuda.synchronize()
    assert last_kernel().startswith("letkf_stream64w_kernel<") and np.array_equal(flw.cpu().numpy(), fl)
    pp = per_point_w(W.cpu().numpy(), Ww.cpu().numpy())
    print("\n[ienks_stream64] prior, transform, against weights_stream64(inf = 1): largest absolute difference %.3e, worst grid "
          "point %.3e" % (float((W - Ww).abs().max()), pp.max()))
    assert pp.max() <= TOL64


def test_same_mathematics_as_the_general_kernel_at_40_members(eng):
    """k = 40 / c 20 (p_max 77), which the general kernel holds: the named method and method="eig" agree within 1e-9 point by
    point, and each agrees with the oracle (1e-10 here, 1e-9 for the eigensolver, as elsewhere in the suite)."""
    k, c = 40, 20.0
    case = case1d(k, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 77
    for vname, eps, scale in VARIANTS:
        w_in = w_in1d(k, k, eps is not None)
        ref = oracle1d(k, k + 1, c, vname, k)
        Ws, fls, ks = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
        We, fle, ke = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps, method="eig")
        assert ks == kname(k) and GENERAL in ke and int((fls & 0xff).max()) == 0
        check(Ws.cpu().numpy(), ref, "%s stream64 k 40 (%s)" % (vname, ks))
        check(We.cpu().numpy(), ref, "%s eig k 40 (%s)" % (vname, ke), tol=1e-9)
        pp = per_point_w(Ws.cpu().numpy(), We.cpu().numpy())
        print("[ienks_stream64] %s k 40: stream64 against eig: worst grid point %.3e" % (vname, pp.max()))
        assert pp.max() <= 1e-9


# ---- 7. declined points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname,eps,scale", VARIANTS)
def test_a_strong_cluster_is_declined_and_redone_at_65_members(eng, vname, eps, scale):
    """test_gpu_stream64.py's cluster at k = 65 / c 20, where the general kernel holds both variants: the flagged set equals
    "degree from the table for this point's Gershgorin bound > cap", restated in float64 numpy at inflation 1; the other rows
    of a prefilled out are written, the declined ones untouched until finish(), after which W is the oracle's."""
    k, c = 65, 20.0
    case = case1d(k, 21)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 77
    strong, want = strong_cluster(case, nb, 1.0)
    n_decl = int(want.sum())
    assert 0 < n_decl < G                          # (the CPU restatement first: the cluster's points and no others)
    w_in = w_in1d(k, 8, eps is not None)
    yb = strong["yb"] * scale
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.ienks_update(dev(w_in), dev(yb), dev(strong["d"]), nb, 1.0, eps, return_flags=True, method="stream64",
                                     defer_retry=True, out=out)
    torch.cuda.synchronize()
    assert W is out and last_kernel() == kname(k)
    assert np.array_equal((fl.cpu().numpy() & RETRY) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())     # declined blocks are left untouched
    before = out.clone()
    assert finish() == n_decl                                                         # the counter, then the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & RETRY).max()) == 0                                 # the redo rewrote the flags
    assert torch.equal(out[~sel], before[~sel])                                       # ... and nothing else
    ref = O.lienks_weights(w_in, strong["grid_x"], strong["obs_x"], yb, strong["d"], c, 1.0, eps)
    check(out.cpu().numpy(), ref, "%s, strong cluster, %d points redone" % (vname, n_decl))


def test_transform_points_off_the_prior_are_declined_whole(eng):
    """Three chosen points, all with observations, whose W_in is off I + w_mean 1^T by 1e-10 in one element: exactly those carry
    MIA_FLAG_RETRY and stay untouched, the counter reads 3, and at k = 65 / p_max 77 the general kernel's redo gives the oracle."""
    k, c = 65, 20.0
    case = case1d(k, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 77 and int(nb.cnt.min()) > 0
    w_in = np.array(w_in1d(k, k, False))
    chosen = np.zeros(G, dtype=bool)
    for g, (i, j) in ((5, (0, 1)), (100, (64, 3)), (202, (17, 17))):
        chosen[g] = True
        w_in[g, i, j] += 1e-10
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.ienks_update(dev(w_in), dev(case["yb"]), dev(case["d"]), nb, 1.0, None, return_flags=True,
                                     method="stream64", defer_retry=True, out=out)
    torch.cuda.synchronize()
    assert W is out and last_kernel() == kname(k)
    fln = fl.cpu().numpy()
    assert np.array_equal((fln & 0xff) == RETRY, chosen) and int((fln & 0xff)[~chosen].max()) == 0
    sel = torch.as_tensor(chosen, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())
    assert finish() == 3
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & RETRY).max()) == 0
    ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.0, None)
    check(out.cpu().numpy(), ref, "transform, three points off the prior redone")


def test_a_declined_point_raises_at_128_members_after_the_others_are_written(mia, eng):
    """The redo is the general kernel's, which cannot hold 128 members: MiaError, data-dependent, AFTER every other point has been
    written (as 2.19)."""
    k, c = 128, 36.0
    case = case1d(k, 23)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    strong, want = strong_cluster(case, nb, 1.0)
    n_decl = int(want.sum())
    assert 0 < n_decl < G
    w_in = w_in1d(k, 8, True)
    yb = strong["yb"] * EPS
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.ienks_update(dev(w_in), dev(yb), dev(strong["d"]), nb, 1.0, EPS, return_flags=True, method="stream64",
                                     defer_retry=True, out=out)
    torch.cuda.synchronize()
    assert last_kernel() == kname(k)
    assert np.array_equal((fl.cpu().numpy() & RETRY) != 0, want)
    with pytest.raises(mia.MiaError, match="status -3"):
        finish()
    torch.cuda.synchronize()
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all())
    ref = O.lienks_weights(w_in, strong["grid_x"], strong["obs_x"], yb, strong["d"], c, 1.0, EPS)
    check(out.cpu().numpy()[~want], ref[~want], "k 128: the %d points that were not declined" % int((~want).sum()))


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it_and_overflow_is_loud(mia, eng):
    k, c = 65, 20.0
    case = case1d(k, 32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 77
    w_in = w_in1d(k, 10, True)
    clean, flc, kern = upd(eng, w_in, case["yb"] * EPS, case["d"], nb, EPS)
    assert kern == kname(k) and int((flc & 0xff).max()) == 0
    j = 77
    bad = case["yb"] * EPS
    bad[3, j] = np.nan
    W, fl, kern = upd(eng, w_in, bad, case["d"], nb, EPS)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G and kern == kname(k)
    assert np.array_equal((fl & NONFINITE) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(W[keep], clean[keep])
    # a NeighbourLists that understates p_max: flag 1 and NaN weights on the overflowing points, the others the clean run's
    small = mia.NeighbourLists(nb.cnt, nb.idx, nb.w, nb.p_cap, 70, nb.g0, nb.g1)
    W, fl, kern = upd(eng, w_in, case["yb"] * EPS, case["d"], small, EPS)
    over = cnt > 70
    assert 0 < over.sum() < G and kern == kname(k)
    assert np.all((fl & 0xff)[over] == OVERFLOW) and np.all((fl & 0xff)[~over] == 0)
    assert torch.isnan(W[torch.as_tensor(over, device=DEV)]).all()
    rest = torch.as_tensor(~over, device=DEV)
    assert per_point_w(W[rest].cpu().numpy(), clean[rest].cpu().numpy()).max() <= TOL64


def test_points_without_observations_return_their_weights_bit_for_bit(eng):
    """The observations around a stretch of the grid removed (65 members, c = 18: a list holds up to 69 observations, a gap wider
    than the radius): whole tiles and parts of tiles without any observation get W_in back bit for bit with flag 0; their
    neighbours have the oracle's weights."""
    k, c = 65, 18.0
    case = case1d(k, 31)
    keep = (case["obs_x"] < 72) | (case["obs_x"] >= 170)
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 69 > k
    empty = nb.cnt.cpu().numpy() == 0
    first, n_far = int(empty.argmax()), int(empty.sum())
    assert n_far >= 17 and first % 16 != 0 and empty[first:first + n_far].all() and empty[112:128].all()    # whole tiles and parts
    want = expected_degrees64(case["yb"], nb, 1.0)
    for vname, eps, scale in VARIANTS:
        w_in = w_in1d(k, 4, eps is not None)
        W, fl, kern = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
        assert kern == kname(k) and int((fl & 0xff).max()) == 0
        sel = torch.as_tensor(empty, device=DEV)
        assert torch.equal(W[sel], dev(w_in)[sel]) and int(np.abs(fl[empty]).max()) == 0 and int(fl[~empty].min()) > 0
        assert np.array_equal((fl[~empty] >> 8) & 0xff, want[~empty])
        ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, observations removed around a stretch of the grid" % vname)


# ---- 9. outside the route ----------------------------------------------------------------------------------------------------------
def entry_rc(eng, w_in, case, nb, k, eps=EPS):
    """mia_lienks_update_stream_f64 itself on float64 copies of the case: its return code"""
    from torch_assimilate_amd import _cabi
    n = nb.g1 - nb.g0
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    w = dev(w_in)
    W = torch.empty((n, k, k), dtype=torch.float64, device=DEV)
    fl = torch.zeros(n, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_lienks_update_stream_f64(w.data_ptr(), 0, k, nb.g0, nb.g1, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                                  nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, eps, W.data_ptr(),
                                                  fl.data_ptr(), retry.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


def test_shapes_outside_the_route(mia, eng):
    """p_max <= k, p_max > 256, k = 129, float32, tau = 0.9 and option tile = 0: method="stream64" raises ValueError and the entry
    answers MIA_ERR_UNSUPPORTED (-3) where a C entry can see the reason."""
    msg = "covers 2 <= k <= 128 and k < p_max <= 256"
    # p_max <= k: the dual routes'
    case = case1d(80, 81)
    nb = eng.localize(case["grid_x"], case["obs_x"], [16.5])
    eye80 = torch.eye(80, dtype=torch.float64)
    yb80, d80 = dev(case["yb"] * EPS), dev(case["d"])
    assert 0 < nb.p_max <= 80 and entry_rc(eng, np.eye(80), case, nb, 80) == -3
    with pytest.raises(ValueError, match=msg):
        eng.ienks_update(eye80, yb80, d80, nb, epsilon=EPS, method="stream64")
    # p_max > 256
    big = O.synthetic_case(300, 128, 1, seed=7)
    nbb = eng.localize(big["grid_x"], big["obs_x"], [80.0])
    assert nbb.p_max > 256 and entry_rc(eng, np.eye(128), big, nbb, 128) == -3
    with pytest.raises(ValueError, match=msg):
        eng.ienks_update(torch.eye(128, dtype=torch.float64), dev(big["yb"] * EPS), dev(big["d"]), nbb, epsilon=EPS, method="stream64")
    # k = 129
    c129 = O.synthetic_case(G, 129, 1, seed=129)
    nb129 = eng.localize(c129["grid_x"], c129["obs_x"], [36.0])
    assert nb129.p_max == 139 and entry_rc(eng, np.eye(129), c129, nb129, 129) == -3
    with pytest.raises(ValueError, match=msg):
        eng.ienks_update(torch.eye(129, dtype=torch.float64), dev(c129["yb"] * EPS), dev(c129["d"]), nb129, epsilon=EPS,
                         method="stream64")
    # inside the route from here on: k = 80 / p_max 93
    nb = eng.localize(case["grid_x"], case["obs_x"], [24.0])
    f32_first(eng)
    assert nb.p_max == 93 and entry_rc(eng, np.eye(80), dict(case, yb=case["yb"] * EPS), nb, 80) == 0
    assert last_kernel() == kname(80)
    with pytest.raises(ValueError, match="float64"):
        eng.ienks_update(eye80.float(), yb80.float(), d80.float(), nb, epsilon=EPS, method="stream64")
    with pytest.raises(ValueError, match="tau"):
        eng.ienks_update(eye80, yb80, d80, nb, tau=0.9, epsilon=EPS, method="stream64")
    with pytest.raises(ValueError):
        eng.ienks_update(eye80, yb80, d80, nb, epsilon=EPS, method="cheb")
    set_option("tile", 0)
    assert entry_rc(eng, np.eye(80), dict(case, yb=case["yb"] * EPS), nb, 80) == -3
    with pytest.raises(ValueError, match="not available"):
        eng.ienks_update(eye80, yb80, d80, nb, epsilon=EPS, method="stream64")

"""The float64 IEnKS weight update with tau = 1 on tiles for ensembles of 65 .. 128 members (csrc/lienks_wide64.hip,
mia_lienks_update_wide_f64, LetkfEngine.ienks_update(method="wide64")): what LocalizedIEnKSTransform / LocalizedIEnKSBundle.inner_loop
run per grid point in the reference's default working precision above 64 members.  The contract is the project's float64 one
(DESIGN 8): relative Frobenius error <= 1e-10 on W as a whole against O.lienks_weights and <= 1e-10 on the WORST SINGLE GRID
POINT.  Every test asserts that lienks_wide64_kernel ran; in the shape sweep no point may carry MIA_FLAG_RETRY, so that the general
kernel cannot supply the parity.

The general kernel's limits, confirmed on a build of the commit before this route (mia_lienks_update_f64 with tau = 1 answers
before any launch; LDS by the formula of csrc/ienks.hip against 162 816 bytes; "ok" = the entry went on to its launch):

    k    p_max   bundle             transform
    65   53      104 848 ok         134 224 ok
    72   69      132 032 ok         174 592 -3
    80   63      152 656 ok         195 664 -3
    94   20      164 896 -3         180 256 -3
    96   81      222 160 -3         287 760 -3
    128  97      378 624 -3         482 112 -3
    128  62      340 176 -3         405 648 -3

and from 97 members on the bundle variant is refused for every list length (k = 97, p_max 1: 163 632 bytes; k = 96, p_max 1:
157 200 ok).  On that build test_the_bundle_class_above_64_members fails: LocalizedIEnKSBundle(dtype=torch.float64) raises
MiaError (mia_lienks_update_f64 failed with status -3) in its first inner loop at k = 96 and k = 128, and
LocalizedIEnKSTransform does at k = 80 with 63 local observations; ienks_update knows no method "wide64"."""
import functools
import re

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O
from test_gpu_ienks64 import expected_degrees64, weights_in
from test_gpu_wide64 import SWEEP, largest_union

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
G = 203                                        # thirteen tiles, the last one ragged
CAP = 127                                      # the float64 table's degree cap
KERNEL = "lienks_wide64_kernel<"
TILE64 = "lienks_update64_kernel"
GENERAL = "ienks_update_kernel<double, 256>"
EPS = 1e-3
RETRY, NONFINITE, OVERFLOW = 8, 4, 1
# the largest degree of every SWEEP case at inflation 1, from the restated rule on the CPU: nothing near the cap
SWEEP_DEGREES = [33, 32, 34, 35, 35, 30, 33, 24]


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


def per_point_w(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    return np.sqrt(((got - ref) ** 2).sum(axis=(1, 2))) / np.maximum(np.sqrt((ref ** 2).sum(axis=(1, 2))), 1e-300)


def check(got, ref, what, tol=TOL64):
    """W [G][k][k] against the reference: the whole and the worst single grid point"""
    pp = per_point_w(got, ref)
    fro = rel_fro(got, ref)
    worst = float(pp.max()) if pp.size else 0.0
    print("\n[ienks_wide64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)"
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


def upd(eng, w_in, yb, d, nb, eps, method="wide64", **kw):
    """engine.ienks_update with its flags: (W, flags as numpy, kernel name)"""
    f32_first(eng)
    res = eng.ienks_update(dev(w_in), dev(yb), dev(d), nb, 1.0, eps, return_flags=True, method=method, **kw)
    torch.cuda.synchronize()
    return res[0], res[1].cpu().numpy(), last_kernel()


def template_args(kern):
    """(UT, KT, NW) of a reported lienks_wide64_kernel<UT, KT, NW>"""
    m = re.match(r"lienks_wide64_kernel<(\d+), (\d+), (\d+)>$", kern)
    assert m, kern
    return tuple(int(v) for v in m.groups())


@functools.lru_cache(maxsize=None)
def case1d(k, stride, seed):
    return O.synthetic_case(G, k, stride, seed=seed)      # (shared: the tests copy before they change a record)


@functools.lru_cache(maxsize=None)
def w_in1d(k, seed, bundle):
    return weights_in(G, k, seed, bundle)                  # (shared: a test that changes an element copies first)


@functools.lru_cache(maxsize=None)
def oracle1d(k, stride, seed, c, variant, wseed):
    """the oracle's update of a 1-D case from the per-point weights w_in1d(k, wseed, .), computed once and shared, never modified.
    Bundle: the records are Yb eps, so that D = Yl / eps is the case's own Yb."""
    case = case1d(k, stride, seed)
    eps, scale = (EPS, EPS) if variant == "bundle" else (None, 1.0)
    W = O.lienks_weights(w_in1d(k, wseed, eps is not None), case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
    W.setflags(write=False)
    return W


VARIANTS = (("bundle", EPS, EPS), ("transform", None, 1.0))


# ---- 1. shape sweep against the oracle, both variants, nothing declined ---------------------------------------------------------
@pytest.mark.parametrize("k,stride,c,p_max,union,dmax", [s + (dg,) for s, dg in zip(SWEEP, SWEEP_DEGREES)])
def test_shape_sweep_vs_oracle(eng, k, stride, c, p_max, union, dmax):
    """k 65 .. 128, UT 2 .. 7, NW 2 and 4, a tile in parts, a ragged last member block; per-point incoming weights.  The template
    arguments are letkf_wide64w_kernel's rule, the degrees the restated rule's, and no point is declined: the parity is the
    tile kernel's own."""
    case = case1d(k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == p_max and largest_union(nb) == union
    want = expected_degrees64(case["yb"], nb)
    assert int(want.max()) == dmax <= CAP              # (checked on the CPU beforehand: nothing near the cap)
    for vname, eps, scale in VARIANTS:
        W, fl, kern = upd(eng, w_in1d(k, k, eps is not None), case["yb"] * scale, case["d"], nb, eps)
        ut, kt, nw = template_args(kern)
        assert ut == min((p_max + 8 + 15) // 16, 8) and kt == (k + 15) // 16 and nw == (2 if ut <= 6 else 4), kern
        assert int((fl & 0xff).max()) == 0, vname      # nothing declined, nothing non-finite
        assert np.array_equal((fl >> 8) & 0xff, want), vname
        check(W.cpu().numpy(), oracle1d(k, stride, k + 1, c, vname, k),
              "%s k %d stride %d c %g p_max %d union %d (%s)" % (vname, k, stride, c, p_max, union, kern))


# ---- 2. shared matrices ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c", [(80, 1, 16.5), (128, 2, 32.0)])
def test_one_shared_matrix(eng, k, stride, c):
    """ONE (k, k) matrix for all points (w_stride = 0): the prior of the first iteration in both variants, and a matrix with
    another mean and another Wp in the bundle variant."""
    case = case1d(k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    for vname, eps, scale in VARIANTS:
        W, fl, kern = upd(eng, np.eye(k), case["yb"] * scale, case["d"], nb, eps)
        assert kern.startswith(KERNEL) and int((fl & 0xff).max()) == 0
        ref = O.lienks_weights(np.eye(k), case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, shared prior, k %d (%s)" % (vname, k, kern))
    w1 = weights_in(1, k, 5, True)[0]
    W, fl, kern = upd(eng, w1, case["yb"] * EPS, case["d"], nb, EPS)
    assert kern.startswith(KERNEL) and int((fl & 0xff).max()) == 0
    check(W.cpu().numpy(), O.lienks_weights(w1, case["grid_x"], case["obs_x"], case["yb"] * EPS, case["d"], c, 1.0, EPS),
          "bundle, one shared non-prior matrix, k %d" % k)


# ---- 3. chain --------------------------------------------------------------------------------------------------------------------
def test_three_bundle_iterations_vs_three_oracle_iterations(eng):
    """k = 96 with 81 local observations, which the general kernel cannot hold.  The map from the incoming w_mean to W' is a
    contraction (|| D psi(S) D^T || < 1): errors do not grow along the chain, the bar stays 1e-10."""
    k, stride, c = 96, 1, 21.0
    case = case1d(k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 81
    yb = case["yb"] * EPS
    w, ref = np.eye(k), np.eye(k)
    for it in range(3):
        W, fl, kern = upd(eng, w, yb, case["d"], nb, EPS)
        assert kern.startswith(KERNEL) and int((fl & 0xff).max()) == 0
        w = W.cpu().numpy()
        ref = O.lienks_weights(ref, case["grid_x"], case["obs_x"], yb, case["d"], c, 1.0, EPS)
        check(w, ref, "bundle chain at k = 96, iteration %d" % it)


# ---- 4. through the classes --------------------------------------------------------------------------------------------------------
def toy_loop(k, s=1, seed=21):
    """the toy problem of tests/test_gpu_ienks.py::test_update_state_loop_vs_oracle on G points"""
    rs = np.random.RandomState(seed)
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

    def reference(eps, iters, c):
        w = np.eye(k)
        for it in range(iters):
            wb = np.broadcast_to(w, (G, k, k)) if w.ndim == 2 else w
            mw = wb if eps is None else eps * np.eye(k) + wb.mean(axis=-1, keepdims=True)
            pseudo = model_np(O.apply_weights(state, mw))
            yb, d = O.obs_space_uncorr(pseudo[0][:, ::s], y, var)
            w = O.lienks_weights(w, gx, ox, yb, d, c, 1.0, eps)
        return O.apply_weights(state, w), w, yb, d
    return state, gx, ox, forward_model, observe, reference


@pytest.mark.parametrize("k,c,p_max", [(96, 21.0, 81), (128, 25.0, 97)])
def test_the_bundle_class_above_64_members(mia, eng, k, c, p_max):
    """LocalizedIEnKSBundle(dtype=torch.float64) with no method named, at shapes the general kernel cannot hold: inner_loop_arrays
    and a three-iteration update_state_arrays return the oracle's result from lienks_wide64_kernel."""
    assert mia.LetkfEngine.IENKS_WIDE64_AUTO_MIN_K >= 65
    state, gx, ox, forward_model, observe, reference = toy_loop(k)
    a = mia.LocalizedIEnKSBundle(forward_model, mia.GaspariCohn(c, mia.AbsoluteDistance()), max_iter=3, tau=1.0, epsilon=EPS,
                                 dtype=torch.float64)
    case = case1d(k, 1, k + 1)
    assert eng.localize(case["grid_x"], case["obs_x"], [c]).p_max == p_max
    f32_first(eng)
    W = a.inner_loop_arrays(np.array(w_in1d(k, k, True)), case["yb"] * EPS, case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
    torch.cuda.synchronize()
    assert last_kernel().startswith(KERNEL), last_kernel()
    assert W.dtype == torch.float64
    check(W.cpu().numpy(), oracle1d(k, 1, k + 1, c, "bundle", k), "LocalizedIEnKSBundle.inner_loop_arrays at k = %d" % k)
    f32_first(eng)
    xa = a.update_state_arrays(state, observe, grid_coords=gx, obs_coords=ox)
    torch.cuda.synchronize()
    assert last_kernel().startswith(KERNEL), last_kernel()
    ref = reference(EPS, 3, c)[0]
    err = rel_fro(xa.cpu().numpy(), ref)
    print("\n[ienks_wide64] LocalizedIEnKSBundle, three iterations at k = %d: analysis rel. Frobenius %.3e" % (k, err))
    assert xa.dtype == torch.float64 and err <= TOL64


def test_the_transform_class_runs_its_first_iteration_here(mia, eng):
    """LocalizedIEnKSTransform at k = 80 with 63 local observations (the general kernel refuses the transform variant there): the
    first iteration, from the prior, is this kernel's.  Per-point transform weights have Wp != I everywhere: ``auto`` does not
    spend a launch that would be declined whole -- the general kernel where it holds the shape, MiaError where it does not."""
    k, c = 80, 16.5
    state, gx, ox, forward_model, observe, reference = toy_loop(k)
    a = mia.LocalizedIEnKSTransform(forward_model, mia.GaspariCohn(c, mia.AbsoluteDistance()), max_iter=1, tau=1.0,
                                    dtype=torch.float64)
    xref, wref, yb, d = reference(None, 1, c)
    f32_first(eng)
    W = a.inner_loop_arrays(np.eye(k), yb, d, grid_coords=gx, obs_coords=ox)
    torch.cuda.synchronize()
    assert last_kernel().startswith(KERNEL), last_kernel()
    check(W.cpu().numpy(), wref, "LocalizedIEnKSTransform.inner_loop_arrays from the prior at k = 80")
    f32_first(eng)
    xa = a.update_state_arrays(state, observe, grid_coords=gx, obs_coords=ox)
    torch.cuda.synchronize()
    assert last_kernel().startswith(KERNEL), last_kernel()
    assert rel_fro(xa.cpu().numpy(), xref) <= TOL64
    # per-point weights of the transform variant
    nb = eng.localize(gx, ox, [c])
    assert nb.p_max == 63
    with pytest.raises(mia.MiaError):
        eng.ienks_update(W, dev(yb), dev(d), nb, 1.0, None)
    case = case1d(65, 4, 66)
    nb65 = eng.localize(case["grid_x"], case["obs_x"], [20.0])
    assert nb65.p_max == 20
    W2, fl, kern = upd(eng, w_in1d(65, 65, False), case["yb"], case["d"], nb65, None, method="auto")
    assert "lienks_wide64" not in kern and GENERAL in kern, kern
    check(W2.cpu().numpy(), oracle1d(65, 4, 66, 20.0, "transform", 65), "per-point transform weights under auto (general kernel)",
          tol=1e-9)


# ---- 5. bits -----------------------------------------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile(eng):
    k, stride, c = 80, 1, 16.5
    case = case1d(k, stride, 21)
    w_in = w_in1d(k, 9, True)
    yb = case["yb"] * EPS

    def run(g0, g1, w, eps, y):
        nb = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
        W, fl, kern = upd(eng, w, y, case["d"], nb, eps)
        assert kern.startswith(KERNEL) and int((fl & 0xff).max()) == 0
        return W
    full = run(0, G, w_in, EPS, yb)
    assert torch.equal(full, run(0, G, w_in, EPS, yb))
    prior = run(0, G, np.eye(k), None, case["yb"])
    g0, g1 = 21, 150
    part = run(g0, g1, w_in[g0:g1], EPS, yb)
    assert part.shape[0] == g1 - g0
    assert torch.equal(part, full[g0:g1])
    assert torch.equal(run(g0, g1, np.eye(k), None, case["yb"]), prior[g0:g1])


# ---- 6. k <= 64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c", [(40, 2, 18.0), (64, 1, 15.0)])
def test_same_mathematics_as_the_one_wavefront_kernel(eng, k, stride, c):
    """k <= 64: the named method against lienks_update64_kernel.  Both within 1e-10 of the oracle and of each other, point by
    point; the largest difference is printed, not asserted (the compiler's contraction of the element-wise updates is not under
    this test's control)."""
    case = case1d(k, stride, k)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert 0 < nb.p_max <= k
    for vname, eps, scale in VARIANTS:
        w_in = w_in1d(k, k, eps is not None)
        ref = oracle1d(k, stride, k, c, vname, k)
        Ww, flw, kw = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
        Wt, flt, kt = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps, method="tile64")
        assert kw.startswith(KERNEL) and TILE64 in kt
        assert int((flw & 0xff).max()) == 0 and int((flt & 0xff).max()) == 0
        assert np.array_equal(flw, flt)                # the same degrees
        check(Ww.cpu().numpy(), ref, "%s wide64 k %d (%s)" % (vname, k, kw))
        check(Wt.cpu().numpy(), ref, "%s tile64 k %d (%s)" % (vname, k, kt))
        pp = per_point_w(Ww.cpu().numpy(), Wt.cpu().numpy())
        print("[ienks_wide64] %s k %d: wide64 against tile64: largest absolute difference %.3e, worst grid point %.3e"
              % (vname, k, float((Ww - Wt).abs().max()), pp.max()))
        assert pp.max() <= TOL64


# ---- 7. declined points ----------------------------------------------------------------------------------------------------------
def test_a_strong_cluster_declines_exactly_the_points_above_the_cap(eng):
    """tests/test_gpu_wide64w.py's cluster (observations 80 .. 85 scaled by 10 in config 4's network) in the bundle variant: the
    flagged set equals "degree from the table for this point's Gershgorin bound > cap", restated in float64 numpy (at inflation
    1: 29 of the 203 points, counted on the CPU beforehand); the other rows of a prefilled out are written, the declined ones
    untouched until finish(), after which W is the oracle's (the general kernel holds the bundle variant at k = 80 / p_max 63)."""
    k, c = 80, 16.5
    case = O.synthetic_case(G, k, 1, seed=5)
    case["yb"][:, 80:86] *= 10.0
    case["d"][80:86] *= 10.0
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 63
    want = expected_degrees64(case["yb"], nb) > CAP
    assert int(want.sum()) == 29
    w_in = w_in1d(k, 8, True)
    yb = case["yb"] * EPS
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.ienks_update(dev(w_in), dev(yb), dev(case["d"]), nb, 1.0, EPS, return_flags=True, method="wide64",
                                     defer_retry=True, out=out)
    torch.cuda.synchronize()
    assert W is out and last_kernel().startswith(KERNEL)
    assert np.array_equal((fl.cpu().numpy() & RETRY) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())
    before = out.clone()
    assert finish() == 29                                              # the counter, then the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & RETRY).max()) == 0                  # the redo rewrote the flags
    assert torch.equal(out[~sel], before[~sel])
    ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], yb, case["d"], c, 1.0, EPS)
    check(out.cpu().numpy(), ref, "strong cluster, 29 points redone")


def test_transform_points_off_the_prior_are_declined_whole(eng):
    """Three chosen points, all with observations, whose W_in is off I + w_mean 1^T by 1e-10 in one element: exactly those carry
    MIA_FLAG_RETRY and stay untouched, the counter reads 3, and at k = 65 / p_max 53 the general kernel's redo gives the oracle."""
    k, stride, c = 65, 1, 14.0
    case = case1d(k, stride, k + 1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    assert nb.p_max == 53 and int(nb.cnt.min()) > 0
    w_in = np.array(w_in1d(k, k, False))
    chosen = np.zeros(G, dtype=bool)
    for g, (i, j) in ((5, (0, 1)), (100, (64, 3)), (202, (17, 17))):
        chosen[g] = True
        w_in[g, i, j] += 1e-10
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    W, fl, finish = eng.ienks_update(dev(w_in), dev(case["yb"]), dev(case["d"]), nb, 1.0, None, return_flags=True,
                                     method="wide64", defer_retry=True, out=out)
    torch.cuda.synchronize()
    assert W is out and last_kernel().startswith(KERNEL)
    fln = fl.cpu().numpy()
    assert np.array_equal((fln & 0xff) == RETRY, chosen) and int((fln & 0xff)[~chosen].max()) == 0
    sel = torch.as_tensor(chosen, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())
    assert finish() == 3
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & RETRY).max()) == 0
    ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], case["yb"], case["d"], c, 1.0, None)
    check(out.cpu().numpy(), ref, "transform, three points off the prior redone")


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it_and_overflow_is_loud(mia, eng):
    k, c = 80, 16.5
    case = case1d(k, 1, 32)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    w_in = w_in1d(k, 10, True)
    clean = upd(eng, w_in, case["yb"] * EPS, case["d"], nb, EPS)[0]
    j = 37
    bad = case["yb"] * EPS
    bad[3, j] = np.nan
    W, fl, kern = upd(eng, w_in, bad, case["d"], nb, EPS)
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G and kern.startswith(KERNEL)
    assert np.array_equal((fl & NONFINITE) != 0, uses)
    keep = torch.as_tensor(~uses, device=DEV)
    assert torch.equal(W[keep], clean[keep])
    # a NeighbourLists that understates p_max: flag 1 and NaN weights on the overflowing points, the others the clean run's
    small = mia.NeighbourLists(nb.cnt, nb.idx, nb.w, nb.p_cap, 40, nb.g0, nb.g1)
    W, fl, kern = upd(eng, w_in, case["yb"] * EPS, case["d"], small, EPS)
    over = cnt > 40
    assert 0 < over.sum() < G and kern.startswith(KERNEL)
    assert np.all((fl & 0xff)[over] == OVERFLOW) and np.all((fl & 0xff)[~over] == 0)
    assert torch.isnan(W[torch.as_tensor(over, device=DEV)]).all()
    rest = torch.as_tensor(~over, device=DEV)
    assert per_point_w(W[rest].cpu().numpy(), clean[rest].cpu().numpy()).max() <= TOL64


def test_points_without_observations_return_their_weights_bit_for_bit(eng):
    k, c = 80, 16.5
    case = O.synthetic_case(G, k, 1, seed=31)
    keep = (case["obs_x"] < 60) | (case["obs_x"] > 150)                    # a gap much wider than the radius
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    empty = nb.cnt.cpu().numpy() == 0
    assert empty[96:112].all() and not empty[:16].any() and 0 < int(empty.sum()) < G     # whole tiles and parts of tiles
    for vname, eps, scale in VARIANTS:
        w_in = w_in1d(k, 4, eps is not None)
        W, fl, kern = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
        assert kern.startswith(KERNEL) and int((fl & 0xff).max()) == 0
        sel = torch.as_tensor(empty, device=DEV)
        assert torch.equal(W[sel], dev(w_in)[sel]) and int(fl[empty].max()) == 0
        ref = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, observations in two parts of the domain" % vname)
    # a shard without any observation, a single ragged tile
    from torch_assimilate_amd.engine import NeighbourLists
    nb0 = NeighbourLists(torch.zeros(5, dtype=torch.int32, device=DEV), torch.full((5, 8), -1, dtype=torch.int32, device=DEV),
                         torch.zeros((5, 8), dtype=torch.float64, device=DEV), 8, 0, 0, 5)
    w_in = weights_in(5, k, 6, True)
    W, fl, kern = upd(eng, w_in, np.zeros((k, 0)), np.zeros(0), nb0, EPS)
    assert kern.startswith(KERNEL) and torch.equal(W, dev(w_in)) and int(fl.max()) == 0


# ---- 9. outside the route ----------------------------------------------------------------------------------------------------------
def entry_rc(eng, w_in, case, nb, k, eps=EPS):
    """mia_lienks_update_wide_f64 itself on float64 copies of the case: its return code"""
    from torch_assimilate_amd import _cabi
    n = nb.g1 - nb.g0
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    w = dev(w_in)
    W = torch.empty((n, k, k), dtype=torch.float64, device=DEV)
    fl = torch.zeros(n, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _cabi.lib().mia_lienks_update_wide_f64(w.data_ptr(), 0, k, nb.g0, nb.g1, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                                nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, eps, W.data_ptr(),
                                                fl.data_ptr(), retry.data_ptr(), None)
    torch.cuda.synchronize()
    return rc


def test_shapes_outside_the_route(mia, eng):
    """p_max > k at k = 80, k = 129, float32, tau = 0.9 and option tile = 0: method="wide64" raises ValueError, the entry answers
    MIA_ERR_UNSUPPORTED (-3) where a C entry can see the reason, and ``auto`` does what it did before the route: the general
    kernel's result where it holds the shape, MiaError where it does not."""
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    # p_max > k at k = 80: refused; under auto the general kernel refuses it too (LDS); at k = 20 it holds p_max > k
    case = case1d(80, 1, 33)
    nb = eng.localize(case["grid_x"], case["obs_x"], [25.0])
    eye80 = torch.eye(80, dtype=torch.float64)
    assert nb.p_max > 80 and lib.mia_lienks_update_wide_f64_cover(80, nb.p_max, G, G) == 0
    assert entry_rc(eng, np.eye(80), case, nb, 80) == -3
    with pytest.raises(ValueError, match="p_max <= k"):
        eng.ienks_update(eye80, dev(case["yb"]), dev(case["d"]), nb, epsilon=EPS, method="wide64")
    with pytest.raises(mia.MiaError):
        eng.ienks_update(eye80, dev(case["yb"]), dev(case["d"]), nb, epsilon=EPS)
    c20 = O.synthetic_case(96, 20, 1, seed=33)
    nb20 = eng.localize(c20["grid_x"], c20["obs_x"], [8.0])
    assert nb20.p_max > 20
    with pytest.raises(ValueError, match="p_max <= k"):
        eng.ienks_update(torch.eye(20, dtype=torch.float64), dev(c20["yb"]), dev(c20["d"]), nb20, method="wide64")
    W, fl, kern = upd(eng, np.eye(20), c20["yb"], c20["d"], nb20, None, method="auto")
    assert GENERAL in kern
    assert rel_fro(W.cpu().numpy(), O.lienks_weights(np.eye(20), c20["grid_x"], c20["obs_x"], c20["yb"], c20["d"], 8.0)) <= 1e-9
    # k = 129: no kernel holds it
    c129 = case1d(129, 4, 34)
    nb129 = eng.localize(c129["grid_x"], c129["obs_x"], [20.0])
    eye129 = torch.eye(129, dtype=torch.float64)
    assert 0 < nb129.p_max <= 64 and lib.mia_lienks_update_wide_f64_cover(129, nb129.p_max, G, G) == 0
    assert entry_rc(eng, np.eye(129), c129, nb129, 129) == -3
    with pytest.raises(ValueError, match="k <= 128"):
        eng.ienks_update(eye129, dev(c129["yb"]), dev(c129["d"]), nb129, epsilon=EPS, method="wide64")
    with pytest.raises(mia.MiaError):
        eng.ienks_update(eye129, dev(c129["yb"]), dev(c129["d"]), nb129, epsilon=EPS)
    # inside the route from here on: k = 65 on a sparse network, which the general kernel holds as well
    c65 = case1d(65, 4, 66)
    nb65 = eng.localize(c65["grid_x"], c65["obs_x"], [20.0])
    eye65 = torch.eye(65, dtype=torch.float64)
    yb65, d65 = dev(c65["yb"] * EPS), dev(c65["d"])
    assert nb65.p_max == 20 and entry_rc(eng, np.eye(65), dict(c65, yb=c65["yb"] * EPS), nb65, 65) == 0
    # float32
    with pytest.raises(ValueError, match="float64"):
        eng.ienks_update(eye65.float(), yb65.float(), d65.float(), nb65, epsilon=EPS, method="wide64")
    f32_first(eng)
    W32 = eng.ienks_update(eye65.float(), yb65.float(), d65.float(), nb65, epsilon=EPS)
    torch.cuda.synchronize()
    assert W32.dtype == torch.float32 and "lienks_wide64" not in last_kernel()
    # tau = 0.9
    with pytest.raises(ValueError, match="tau"):
        eng.ienks_update(eye65, yb65, d65, nb65, tau=0.9, epsilon=EPS, method="wide64")
    f32_first(eng)
    W = eng.ienks_update(eye65, yb65, d65, nb65, tau=0.9, epsilon=EPS)
    torch.cuda.synchronize()
    assert GENERAL in last_kernel()
    ref = O.lienks_weights(np.eye(65), c65["grid_x"], c65["obs_x"], c65["yb"] * EPS, c65["d"], 20.0, 0.9, EPS)
    assert rel_fro(W.cpu().numpy(), ref) <= 1e-9
    # the one-wavefront kernel keeps its message
    with pytest.raises(ValueError, match="k <= 64"):
        eng.ienks_update(eye65, yb65, d65, nb65, epsilon=EPS, method="tile64")
    with pytest.raises(ValueError):
        eng.ienks_update(eye65, yb65, d65, nb65, epsilon=EPS, method="cheb")
    # option tile = 0
    ref = O.lienks_weights(np.eye(65), c65["grid_x"], c65["obs_x"], c65["yb"] * EPS, c65["d"], 20.0, 1.0, EPS)
    set_option("tile", 0)
    assert entry_rc(eng, np.eye(65), dict(c65, yb=c65["yb"] * EPS), nb65, 65) == -3
    with pytest.raises(ValueError, match="not available"):
        eng.ienks_update(eye65, yb65, d65, nb65, epsilon=EPS, method="wide64")
    f32_first(eng)
    W = eng.ienks_update(eye65, yb65, d65, nb65, epsilon=EPS)
    torch.cuda.synchronize()
    assert GENERAL in last_kernel()
    assert rel_fro(W.cpu().numpy(), ref) <= 1e-9

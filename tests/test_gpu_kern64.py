"""The float64 kernel-expression tile route (csrc/lketkf_tile64.hip with a statistics set, instantiated in csrc/lketkf_kern64.hip;
mia_lketkf_kernel_analysis_matfun_f64): what LKETKF(kernel, localization) runs in the default working precision for every
positive semidefinite kernel and composition other than a lone RBF / Gauss kernel.  The bar is the one tests/test_gpu_kernels.py
sets for the float64 expression route: relative Frobenius error <= 1e-9 against the golden vectors and the float64 oracle AND
the worst single grid point <= 1e-9 (device exp / pow differ from libm in the last ulps and the regularised inverse amplifies
that).  Every parity test runs a float32 analysis first, asserts that the reported kernel is the new form, that nothing is
declined where stated, and that the low flag byte is 0 -- so the Jacobi kernel cannot supply the parity."""
import re

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from kernel_cases import oracle_kernels, product_kernels
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-9
DEV = "cuda:0"
KERNEL = "lketkf_tile64"
LOG_TOL, MARGIN = 26.0, 2            # the float64 table's truncation target and margin
PSD = [n for n in sorted(oracle_kernels()) if n not in ("tanh", "periodic")]
SWEEP_KERNELS = ["poly2", "rational", "ornuhl", "rbf_plus_diag", "scale_times_rbf", "linear_plus_scale", "rational_pow_scale",
                 "poly_plus_ornuhl_times_scale"]
NO_POLY = [n for n in SWEEP_KERNELS if not n.startswith("poly")]


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


def is_new(name, stats=None):
    """the kernel-expression form: lketkf_tile64_kernel<UT, NR, ST> with ST = 1 (dot), 2 (sq) or 7 (dot, sq, l1); the RBF form has ST = 0"""
    m = re.search(r"lketkf_tile64_kernel<\d+, \d+, (\d+)>", name)
    return bool(m) and int(m.group(1)) in ((1, 2, 7) if stats is None else (stats,))


def check(got, ref, what, tol=TOL):
    from oracle_pool import per_point_errors
    pp, fro = per_point_errors(got, ref)
    print("\n[kern64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= tol, what
    assert pp.max() <= tol, what


def run64(eng, case, nb, inf, prog, method="kern64", psd=True, **kw):
    """engine.analysis in float64 with a caller-owned decline counter: (Xa, flags, declined, kernel name)"""
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xa, fl = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, inf, return_flags=True, method=method,
                          retry=retry, kernel_program=prog, kernel_psd=psd, **kw)
    torch.cuda.synchronize()
    return xa, fl, int(retry.item()), last_kernel()


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh (letkf_wave.hip never reports one)"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel()


def degree64(T):
    """The float64 table's degree for T = L / reg, restated: T rounded up to the geometric grid (32 per octave, 2^-24 .. 2^8),
    degree = ceil(26 / log rho) + 2, rho = (sqrt(1 + T) + 1) / (sqrt(1 + T) - 1), at least 3"""
    ti = int(np.clip(np.ceil(32 * np.log2(max(T, 1e-300))) + 24 * 32, 0, 32 * 32 - 1))
    sq = np.sqrt(1 + 2.0 ** ((ti - 24 * 32) / 32))
    return max(3, int(np.ceil(LOG_TOL / np.log((sq + 1) / max(sq - 1, 1e-12))) + MARGIN))


def kern_core(fn, stats=None):
    """O.ketkf_weights with ``fn`` as the per-point core; ``stats`` (a list) collects, per point, the largest eigenvalue of
    C K C and the largest absolute row sum of K (the kernel's spectral bound); (0, 0) for a point without observations"""
    def core(a, b, inf):
        if stats is not None:
            k = a.shape[-2]
            if a.shape[-1] == 0:
                stats.append((0.0, 0.0))
            else:
                K = fn(a, a).numpy()
                C_ = np.eye(k) - 1.0 / k
                stats.append((float(np.linalg.eigvalsh(C_ @ K @ C_).max()), float(np.abs(K).sum(axis=1).max())))
        return O.ketkf_weights(a, b, fn, inf)
    return core


def oracle_weights(case, c, inf, fn, stats=None, **kw):
    return O.letkf_weights(case.get("grid_x", case.get("grid")), case.get("obs_x", case.get("obs")), case["yb"], case["d"], c, inf,
                           core=kern_core(fn, stats), **kw)


_CASE, _REF = {}, {}


def sweep_case(k, stride, c):
    """The G = 203 case of a sweep entry (three state rows; one row = its first)"""
    key = (k, stride, c)
    if key not in _CASE:
        _CASE[key] = O.synthetic_case(203, k, stride, seed=k + 3, m=3)
    return _CASE[key]


def sweep_ref(k, stride, c, name, inf, fn=None):
    """the oracle's weights of a sweep entry with (largest eigenvalue of C K C, largest absolute row sum) per point, computed once"""
    key = (k, stride, c, name, inf)
    if key not in _REF:
        st = []
        W = oracle_weights(sweep_case(k, stride, c), c, inf, fn or oracle_kernels()[name], st)
        _REF[key] = (W, np.array(st))
    return _REF[key]


# ---- 1. golden single blocks -----------------------------------------------------------------------------------------------------
def test_golden_single_blocks(eng, golden):
    """The reference's own KETKF weights (golden g8: every kernel family x blocks (40, 20), (10, 40), (20, 7) x inflation 1.0 /
    1.1) applied to a random 3-row ensemble = the kernel's analysis of ONE grid point that sees every observation with weight 1.
    Every positive semidefinite kernel whose restated degree (the table's for L / reg, L the largest absolute row sum of the
    oracle's K) is at most 127: 52 of 54 -- only poly3 on block (10, 40) exceeds it, at both inflations."""
    g = golden("g8_kernels_gcinf.npz")
    ora, prod = oracle_kernels(), product_kernels()
    seen, skipped = 0, []
    for bi, (k, p) in enumerate(g["blocks"]):
        k, p = int(k), int(p)
        yb, d = g[f"yb_{bi}"], g[f"d_{bi}"]
        case = dict(state=np.random.RandomState(200 + bi).normal(size=(3, k, 1)), yb=yb, d=d)
        nb = eng.localize(np.zeros(1), np.zeros(p), [5.0])
        assert nb.p_max == p
        for name in PSD:
            L = float(np.abs(ora[name](torch.as_tensor(yb), torch.as_tensor(yb)).numpy()).sum(axis=1).max())
            for inf, tag in ((1.0, "1p0"), (1.1, "1p1")):
                deg = degree64(L / ((k - 1) / inf))
                if deg > 127:
                    skipped.append((name, bi, inf))
                    continue
                f32_first(eng)
                xa, fl, declined, kern = run64(eng, case, nb, inf, prod[name].program())
                assert is_new(kern) and declined == 0 and int((fl & 0xff).max().item()) == 0, (name, k, p, kern)
                assert int(fl.item()) >> 8 == deg, (name, k, p, inf, int(fl.item()) >> 8, deg)
                ref = O.apply_weights(case["state"], g[f"ketkf_{name}_{bi}_{tag}"][None])
                err = rel_fro(xa.cpu().numpy(), ref)
                print("\n[kern64] golden block k %d p %d %s inf %s degree %d: %.3e" % (k, p, name, inf, deg, err))
                assert err <= TOL, (k, p, name, tag)
                seen += 1
    assert seen == 52 and skipped == [("poly3", 1, 1.0), ("poly3", 1, 1.1)], (seen, skipped)


# ---- 2. golden localised cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poly2", "ornuhl"])
def test_golden_localised_cases(mia, eng, golden, name):
    """lketkf_{poly2, ornuhl}_analysis of g8 (Gaspari-Cohn 10, inflation 1.1) through engine.analysis(method="kern64") with lists
    from eng.localize, and through LKETKF(...) with no dtype=: parity holds in any case, and the class reports the new kernel
    exactly when the KERN64_AUTO_* rule admits the shape."""
    g = golden("g8_kernels_gcinf.npz")
    kern = product_kernels()[name]
    st = np.asarray(g["loc_state"])
    st3 = st.reshape(-1, st.shape[-2], st.shape[-1])
    case = dict(state=st3, yb=g["loc_yb"], d=g["loc_d"])
    nb = eng.localize(g["loc_grid_x"], g["loc_obs_x"], [10.0])
    f32_first(eng)
    xa, fl, declined, kname = run64(eng, case, nb, 1.1, kern.program())
    fl = fl.cpu().numpy()
    assert is_new(kname) and declined == 0 and int((fl & 0xff).max()) == 0, kname
    ref = np.asarray(g[f"lketkf_{name}_analysis"]).reshape(st3.shape)
    check(xa.cpu().numpy(), ref, "golden localised %s, degrees %d..%d" % (name, (fl >> 8).min(), (fl >> 8).max()))
    assert int((fl >> 8).max()) == dict(poly2=76, ornuhl=14)[name]
    f32_first(eng)
    f = mia.LKETKF(kern, localization=mia.GaspariCohn(10.0, mia.AbsoluteDistance()), inf_factor=1.1)
    xc = f.analyse_arrays(g["loc_state"], g["loc_yb"], g["loc_d"], grid_coords=g["loc_grid_x"], obs_coords=g["loc_obs_x"])
    assert xc.dtype == torch.float64
    assert is_new(last_kernel()) == eng._kern64_auto(st3.shape[0], st3.shape[1], nb.p_max), last_kernel()
    check(xc.cpu().numpy().reshape(st3.shape), ref, "golden localised %s through LKETKF" % name)


# ---- 3. sweep against the oracle, every point ----------------------------------------------------------------------------------------
SWEEP = ([(k, s, c, n) for (k, s, c) in ((8, 2, 6.0), (17, 1, 4.0), (20, 3, 25.0), (40, 2, 10.0)) for n in SWEEP_KERNELS] +
         [(k, s, c, n) for (k, s, c) in ((5, 1, 3.0), (40, 1, 15.0)) for n in NO_POLY])


@pytest.mark.parametrize("k,stride,c,name", SWEEP)
def test_shape_sweep_vs_oracle(eng, k, stride, c, name):
    """G = 203 (13 tiles, ragged last one), one and three state rows, both inflations; (5, 1, 3) has fewer pairs than one row
    block, (17, 1, 4) a pair count just across a block boundary, (40, 1, 15) unions of 74 slots (tiles in parts).  Nothing is
    declined: no point of these inputs exceeds degree 96 at inflation 1.1.  The reported degree lies between the table's degree
    for the largest eigenvalue of C K C and for the absolute row-sum bound."""
    case3 = sweep_case(k, stride, c)
    nb = eng.localize(case3["grid_x"], case3["obs_x"], [c])
    assert 0 < nb.p_max <= 64
    prog = product_kernels()[name].program()
    for m in (1, 3):
        case = dict(case3, state=case3["state"][:m])
        for inf in (1.0, 1.1):
            f32_first(eng)
            xa, fl, declined, kern = run64(eng, case, nb, inf, prog)
            assert is_new(kern), kern
            assert declined == 0
            fl = fl.cpu().numpy()
            assert int((fl & 0xff).max()) == 0
            W, st = sweep_ref(k, stride, c, name, inf)
            reg = (k - 1) / inf
            got = (fl >> 8) & 0xff
            lo = np.array([degree64(l / reg) for l in st[:, 0]])
            hi = np.array([degree64(l * (1.0 + 1e-9) / reg) for l in st[:, 1]])
            assert (lo <= got).all() and (got <= hi).all() and got.max() <= 96, (got.min(), got.max(), lo.max(), hi.max())
            check(xa.cpu().numpy(), O.apply_weights(case["state"], W),
                  "%s k %d stride %d c %g m %d inf %g p_max %d degrees %d..%d (%s)" % (name, k, stride, c, m, inf, nb.p_max,
                                                                                  got.min(), got.max(), kern))


# ---- 4. each statistics set alone, and the `same` flag ----------------------------------------------------------------------------
def test_each_statistics_set_and_the_same_flag(mia, eng):
    """One program that pushes only DOT, one only SQDIST, one only L1DIST, one all three: each lands on its compiled set and
    matches the oracle.  DiagKernel's constant belongs to the pairs T(a, a) of the RESULT rows and to no observation pair:
    RBF + Diag and the RBF alone must each match their own oracle, so their difference is the diagonal term's effect."""
    from torch_assimilate_amd import kernels as K
    k, stride, c, inf = 17, 1, 4.0, 1.1
    case = sweep_case(k, stride, c)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    ora = oracle_kernels()
    all3 = K.RBFKernel(0.5) + K.PolyKernel(2.0, 1.0) + K.OrnsteinUhlenbeckKernel(6.0)
    sets = [("dot", K.LinearKernel(), O.linear_kernel, 1),
            ("sq", K.RBFKernel(0.5), lambda x, y: O.rbf_kernel(x, y, 0.5), 2),
            ("l1", K.OrnsteinUhlenbeckKernel(6.0), ora["ornuhl"], 7),
            ("all", all3, lambda x, y: O.rbf_kernel(x, y, 0.5) + O.poly_kernel(x, y, 2.0, 1.0) + O.orn_uhl_kernel(x, y, 6.0), 7),
            ("rbf_plus_diag", K.RBFKernel(0.5) + K.DiagKernel(0.3), ora["rbf_plus_diag"], 2)]
    got, ref = {}, {}
    for tag, kern, fn, st in sets:
        assert K.kernel_is_psd(kern)
        used = {op for op, _ in kern.program()} & {K.KOP_DOT, K.KOP_SQDIST, K.KOP_L1DIST}
        assert used == dict(dot={1}, sq={2}, l1={3}, all={1, 2, 3}, rbf_plus_diag={2})[tag]
        f32_first(eng)
        xa, fl, declined, kname = run64(eng, case, nb, inf, kern.program())
        assert is_new(kname, st) and declined == 0 and int((fl & 0xff).max().item()) == 0, (tag, kname)
        W, _ = sweep_ref(k, stride, c, "set_" + tag, inf, fn)
        got[tag], ref[tag] = xa.cpu().numpy(), O.apply_weights(case["state"], W)
        check(got[tag], ref[tag], "statistics set %s (%s)" % (tag, kname))
    dref = ref["rbf_plus_diag"] - ref["sq"]
    share = np.linalg.norm(dref) / np.linalg.norm(ref["sq"])
    err = rel_fro(got["rbf_plus_diag"] - got["sq"], dref)
    print("\n[kern64] diagonal term: share of the analysis %.3e, error of the difference %.3e" % (share, err))
    assert share >= 1e-3              # (so that two analyses within 1e-9 of their oracles pin the difference to 2e-9 / 1e-3)
    assert err <= 2e-6


# ---- 5. decline and redo ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,c,name,expect", [(40, 2, 10.0, "poly3", 201), (40, 1, 15.0, "poly2", 13)])
def test_decline_and_redo(eng, k, stride, c, name, expect):
    """poly3 on (40, 2, 10): 201 of 203 points exceed degree 127; poly2 on (40, 1, 15): 13 of 203, spread over tiles that run
    in parts.  The declined points are those of the CPU restatement (a point whose L / reg lies within 1e-9 relative of a grid
    boundary of the table may fall either way), they are left untouched, and after the redo through
    mia_lketkf_kernel_analysis_retry_f64 every point is within 1e-9 of the oracle."""
    inf = 1.1
    case = dict(sweep_case(k, stride, c))
    case["state"] = case["state"][:1]
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    W, st = sweep_ref(k, stride, c, name, inf)
    reg = (k - 1) / inf
    d_lo = np.array([degree64(l * (1.0 - 1e-9) / reg) for l in st[:, 1]]) > 127
    d_hi = np.array([degree64(l * (1.0 + 1e-9) / reg) for l in st[:, 1]]) > 127
    sure = d_lo == d_hi
    assert int(d_hi.sum()) == expect and sure.all()
    G = case["state"].shape[-1]
    out = torch.full((1, k, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    f32_first(eng)
    res = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, inf, kernel_program=product_kernels()[name].program(),
                       kernel_psd=True, method="kern64", out=out, flags=fl, retry=retry, defer_retry=True)
    torch.cuda.synchronize()
    assert is_new(last_kernel()), last_kernel()
    flagged = (fl.cpu().numpy() & 0xff) == 8                 # MIA_FLAG_RETRY
    assert np.array_equal(flagged[sure], d_hi[sure])
    assert int(retry.item()) == int(flagged.sum())
    assert bool((out[:, :, torch.as_tensor(flagged, device=DEV)] == -7.0).all())      # declined points are left untouched
    ref = O.apply_weights(case["state"], W)
    if (~flagged).any():
        check(out.cpu().numpy()[:, :, ~flagged], ref[:, :, ~flagged], "%s: the points the kernel analysed itself" % name)
    assert res[-1]() == int(flagged.sum())                   # the deferred redo
    torch.cuda.synchronize()
    after = fl.cpu().numpy() & 0xff
    assert not (after & 8).any() and int(after.max()) == 0
    check(out.cpu().numpy(), ref, "%s after the redo of %d points" % (name, int(flagged.sum())))
    # ... and the same in one call, without defer_retry
    xa, fl2, declined, kname = run64(eng, case, nb, inf, product_kernels()[name].program())
    assert declined == int(flagged.sum())
    check(xa.cpu().numpy(), ref, "%s in one call" % name)


# ---- 6. the RBF kernel written as a program ----------------------------------------------------------------------------------------
def test_rbf_as_a_program_agrees_with_rbf64(mia, eng):
    from torch_assimilate_amd import kernels as K
    case = sweep_case(40, 2, 10.0)
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    f32_first(eng)
    xa, fl, declined, kname = run64(eng, case, nb, 1.1, K.RBFKernel(0.5).program())
    assert is_new(kname, 2) and declined == 0
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xr, fr = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, 1.1, return_flags=True, method="rbf64", retry=retry,
                          rbf_gamma=0.5)
    torch.cuda.synchronize()
    assert KERNEL in last_kernel() and not is_new(last_kernel()) and int(retry.item()) == 0
    assert torch.equal(fl >> 8, fr >> 8)
    check(xa.cpu().numpy(), xr.cpu().numpy(), "RBF as a program against rbf64", tol=1e-13)


# ---- 7. independence of launch geometry, bit for bit ------------------------------------------------------------------------------------
def test_a_points_bits_do_not_depend_on_its_tile(eng):
    prod = product_kernels()
    g0, g1 = 37, 150
    for (k, stride, c), name in (((40, 2, 10.0), "poly_plus_ornuhl_times_scale"), ((40, 1, 15.0), "rational"), ((17, 1, 4.0), "poly2")):
        case = sweep_case(k, stride, c)
        prog = prod[name].program()
        full, _, declined, kern = run64(eng, case, eng.localize(case["grid_x"], case["obs_x"], [c]), 1.1, prog)
        assert declined == 0 and is_new(kern)
        nbs = eng.localize(case["grid_x"], case["obs_x"], [c], g0=g0, g1=g1)
        part = run64(eng, case, nbs, 1.1, prog)[0]
        assert part.shape[-1] == g1 - g0 and torch.equal(part, full[:, :, g0:g1]), name
        # out= with a column offset into a wider buffer
        out = torch.full((3, k, g1 - g0 + 9), -7.0, dtype=torch.float64, device=DEV)
        res = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nbs, 1.1, kernel_program=prog, kernel_psd=True,
                           method="kern64", out=out, out_offset=5)
        torch.cuda.synchronize()
        assert res is out and is_new(last_kernel())
        assert torch.equal(out[:, :, 5:5 + g1 - g0], full[:, :, g0:g1])
        assert bool((out[:, :, :5] == -7.0).all()) and bool((out[:, :, 5 + g1 - g0:] == -7.0).all())


# ---- 8. cases mirrored from the RBF file ---------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_use_it(eng):
    G, k, j = 320, 40, 100
    prog = product_kernels()["poly_plus_ornuhl_times_scale"].program()
    case = O.synthetic_case(G, k, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    clean, _, declined, _ = run64(eng, case, nb, 1.1, prog)
    assert declined == 0
    bad = dict(case, yb=case["yb"].copy())
    bad["yb"][5, j] = np.nan
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G and len(set(np.nonzero(uses)[0] // 16)) >= 2
    out = torch.full((1, k, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = eng.analysis(dev(bad["state"]), dev(bad["yb"]), dev(bad["d"]), nb, 1.1, kernel_program=prog, kernel_psd=True, method="kern64",
                       out=out, flags=fl, retry=retry, defer_retry=True)
    torch.cuda.synchronize()
    assert is_new(last_kernel())
    flagged = (fl.cpu().numpy() & 0xff) == 8
    assert np.array_equal(flagged, uses) and int(retry.item()) == int(uses.sum())
    keep = torch.as_tensor(~uses, device=DEV)
    assert bool((out[:, :, ~keep] == -7.0).all())
    assert torch.equal(out[:, :, keep], clean[:, :, keep])   # (canonical summation order: the very bits)
    assert res[-1]() == int(uses.sum())
    torch.cuda.synchronize()
    after = fl.cpu().numpy() & 0xff
    assert int(after[~uses].max()) == 0 and not (after & 8).any()
    assert torch.equal(out[:, :, keep], clean[:, :, keep])


def test_points_without_local_observations(eng):
    """Observations on one third of the domain: the other points get mean + sqrt(inf) x' from the same kernel (1e-14: one
    multiply-add per entry), tiles that mix both kinds included."""
    G, k = 400, 40
    ora, prod = oracle_kernels(), product_kernels()
    case = O.synthetic_case(G, k, 2, seed=17, m=2)
    keep = case["obs_x"] < 130.0
    case = dict(case, obs_x=case["obs_x"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid_x"], case["obs_x"], [10.0])
    cnt = nb.cnt.cpu().numpy()
    assert any(0 < (cnt[t:t + 16] == 0).sum() < 16 for t in range(0, G, 16))
    far = cnt == 0
    st = case["state"][:, :, far]
    mean = st.mean(axis=1, keepdims=True)
    for name, inf in (("linear_plus_scale", 1.3), ("rbf_plus_diag", 1.0)):
        f32_first(eng)
        xa, fl, declined, kern = run64(eng, case, nb, inf, prod[name].program())
        assert is_new(kern) and declined == 0 and int((fl & 0xff).max().item()) == 0
        check(xa.cpu().numpy(), O.apply_weights(case["state"], oracle_weights(case, 10.0, inf, ora[name])), "%s, observations on a third" % name)
        assert rel_fro(xa.cpu().numpy()[:, :, far], mean + np.sqrt(inf) * (st - mean)) <= 1e-14


def test_tile_option_sends_auto_to_the_jacobi_kernel(eng):
    case = dict(sweep_case(20, 3, 25.0))
    case["state"] = case["state"][:1]
    nb = eng.localize(case["grid_x"], case["obs_x"], [25.0])
    prog = product_kernels()["rational"].program()
    xn, _, declined, named = run64(eng, case, nb, 1.1, prog)
    assert is_new(named) and declined == 0
    set_option("tile", 0)
    f32_first(eng)
    xo, _, _, kern = run64(eng, case, nb, 1.1, prog, method="auto")
    assert KERNEL not in kern
    check(xo.cpu().numpy(), xn.cpu().numpy(), "auto with tile = 0 against kern64")
    set_option("tile", 1)
    f32_first(eng)
    xa, _, _, kern = run64(eng, case, nb, 1.1, prog, method="auto")
    assert is_new(kern) == eng._kern64_auto(1, 20, nb.p_max), kern
    check(xa.cpu().numpy(), xn.cpu().numpy(), "auto with tile = 1 against kern64")
    # a program "auto" may not hand over: not vouched for
    f32_first(eng)
    xu, _, _, kern = run64(eng, case, nb, 1.1, prog, method="auto", psd=False)
    assert KERNEL not in kern
    check(xu.cpu().numpy(), xn.cpu().numpy(), "auto without kernel_psd against kern64")


# ---- 9. the guard -------------------------------------------------------------------------------------------------------------------
def test_guard(mia, eng, golden):
    prod, ora = product_kernels(), oracle_kernels()
    case = dict(sweep_case(17, 1, 4.0))
    nb = eng.localize(case["grid_x"], case["obs_x"], [4.0])
    args = (dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, 1.1)
    prog = prod["poly2"].program()
    with pytest.raises(ValueError):
        eng.analysis(*args, kernel_program=prog, method="kern64")                                  # not vouched for
    with pytest.raises(ValueError):
        eng.analysis(*(a.float() if torch.is_tensor(a) else a for a in args), kernel_program=prog, kernel_psd=True, method="kern64")
    with pytest.raises(ValueError):
        eng.analysis(*args, kernel_program=prog, kernel_psd=True, method="kern64", return_weights=True)
    with pytest.raises(ValueError):
        eng.analysis(*args, kernel_psd=True, method="kern64")                                      # no program
    with pytest.raises(ValueError):
        eng.analysis(*args, rbf_gamma=0.5, kernel_psd=True, method="kern64")
    from torch_assimilate_amd import _cabi
    with pytest.raises(_cabi.MiaError):                                                            # tanh: MIA_ERR_UNSUPPORTED by name
        eng.analysis(*args, kernel_program=prod["tanh"].program(), kernel_psd=True, method="kern64")
    # The kernels that are not positive semidefinite stay on the Jacobi kernel in the default dtype, exactly as before: the class
    # call reports no tile kernel and returns the very bits of method="eig", the unchanged expression route.
    g = golden("g8_kernels_gcinf.npz")
    for name in ("tanh", "periodic"):
        for cs, st, nbc, c in ((case, case["state"], nb, 4.0),) + (g8_localised(eng, g),):
            f32_first(eng)
            f = mia.LKETKF(prod[name], localization=mia.GaspariCohn(c, mia.AbsoluteDistance()), inf_factor=1.1)
            assert f._kernel_args()["kernel_psd"] is False
            xa = f.analyse_arrays(st, cs["yb"], cs["d"], cs["grid_x"], cs["obs_x"])
            assert KERNEL not in last_kernel(), last_kernel()
            xe = eng.analysis(dev(st), dev(cs["yb"]), dev(cs["d"]), nbc, 1.1, kernel_program=prod[name].program(), method="eig")
            torch.cuda.synchronize()
            assert torch.equal(xa.reshape(xe.shape), xe), name


def g8_localised(eng, g):
    """the localised case of golden g8 (k = 40, G = 64, Gaspari-Cohn 10): (case, state (m, k, G), lists, radius)"""
    gcase = dict(grid_x=g["loc_grid_x"], obs_x=g["loc_obs_x"], yb=g["loc_yb"], d=g["loc_d"])
    gst = np.asarray(g["loc_state"]).reshape(-1, g["loc_yb"].shape[0], len(g["loc_grid_x"]))
    return gcase, gst, eng.localize(gcase["grid_x"], gcase["obs_x"], [10.0]), 10.0


@pytest.mark.parametrize("name", ["tanh", "periodic"])
def test_kernels_that_stay_on_the_jacobi_kernel_match_the_oracle(mia, eng, golden, name):
    """LKETKF(TanhKernel(0.05, 0.1)) / LKETKF(PeriodicKernel(7.0, 1.5)) in the default dtype against the float64 oracle at the bar of
    the float64 expression route (relative Frobenius error < 1e-9, tests/test_gpu_kernels.py), on the localised case of golden g8.
    This runs letkf_wave_kernel<double> only (test_guard pins the class result to the bits of method="eig").  These kernels are
    INDEFINITE -- C K C has eigenvalues near -1 -- and the Jacobi kernel, which stops at off-diagonal size sqrt(eps) and corrects
    to first order, used the divided differences of the unclamped functions: 3.003e-9 (tanh) and 3.141e-9 (periodic) against the
    oracle on MI355X.  With the clamp's factor in the correction (letkf_wave.hip, clamp_dd): 2.9e-14 and 4.9e-15."""
    g = golden("g8_kernels_gcinf.npz")
    gcase, gst, gnb, c = g8_localised(eng, g)
    f32_first(eng)
    f = mia.LKETKF(product_kernels()[name], localization=mia.GaspariCohn(c, mia.AbsoluteDistance()), inf_factor=1.1)
    xa = f.analyse_arrays(gst, gcase["yb"], gcase["d"], gcase["grid_x"], gcase["obs_x"])
    assert KERNEL not in last_kernel(), last_kernel()
    err = rel_fro(xa.cpu().numpy().reshape(gst.shape), O.apply_weights(gst, oracle_weights(gcase, c, 1.1, oracle_kernels()[name])))
    print("\n[kern64] LKETKF(%s) on the Jacobi kernel, golden g8 localised case: rel. Frobenius %.3e" % (name, err))
    assert err < 1e-9, name

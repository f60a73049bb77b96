"""The float64 ensemble transform on tiles of sixteen grid points (csrc/apply_local64.hip): mia_apply_local_weights_f64
(per-grid-point weights) and mia_apply_weights_f64 (one weight matrix) on v_mfma_f64_16x16x4_f64, against the float64 oracle.
The contract is the one tests/test_gpu_ienks.py::test_apply_local_weights_vs_oracle sets for these entries: relative Frobenius
error below 1e-14, below 1e-12 on a variable with a mean of 300 after the mean is subtracted, a sub-range equal to the full
run's columns bit for bit.  Which kernel ran is read from mia_last_transform_kernel."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_fro, set_option
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-14
TOL64 = 1e-10                  # the classes' float64 contract (tests/test_gpu_weights64.py, tests/test_gpu_parity.py)
DEV = "cuda:0"
TILE, FALLBACK = "apply_local64_tile_kernel", "apply_local_weights_kernel<double>"
GTILE, GFALLBACK = "apply_global64_tile_kernel", "apply_weights_kernel<double"
LOCAL_SHAPES = [(1, 2, 17), (2, 3, 211), (7, 17, 403), (8, 40, 1000), (9, 40, 999), (16, 48, 517), (17, 64, 256), (33, 65, 130),
                (70, 17, 403), (5, 96, 300), (4, 100, 250), (3, 128, 130), (17, 128, 49)]
GLOBAL_SHAPES = [(1, 2, 17), (3, 40, 1000), (17, 64, 257), (5, 96, 300), (2, 128, 130), (9, 17, 403)]


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


def last_kernel():
    from torch_assimilate_amd import _cabi
    torch.cuda.synchronize()
    return _cabi.last_transform_kernel()


@functools.lru_cache(maxsize=None)
def local_case(m, k, G):
    """seeded inputs and the oracle's transform, computed once and shared (read-only)"""
    rs = np.random.RandomState(k)
    X, W = rs.normal(size=(m, k, G)), rs.normal(size=(G, k, k)) / np.sqrt(k)
    X[0] += 300.0                                # (a variable with a large mean: the transform works on perturbations)
    ref = O.apply_weights(X, W)
    for a in (X, W, ref):
        a.setflags(write=False)
    return X, W, ref


@functools.lru_cache(maxsize=None)
def global_case(m, k, G):
    rs = np.random.RandomState(k)
    X, W = rs.normal(size=(m, k, G)), rs.normal(size=(k, k)) / np.sqrt(k)
    X[0] += 300.0
    ref = O.apply_weights(X, W)
    for a in (X, W, ref):
        a.setflags(write=False)
    return X, W, ref


def t64(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def check(got, ref, what):
    got = got.cpu().numpy()
    e, e0 = rel_fro(got, ref), rel_fro(got[0] - 300.0, ref[0] - 300.0)
    print("\n[apply64] %s: rel. Frobenius %.3e, row 0 without its mean %.3e" % (what, e, e0))
    assert e < TOL, what
    assert e0 < 100 * TOL, what


def sub_range(G):
    return (100, 200) if G >= 200 else (5, min(37, G))


# ---- 1. per-point weights: every covered shape on the tile kernel ------------------------------------------------------------------
@pytest.mark.parametrize("m,k,G", LOCAL_SHAPES)
def test_per_point_transform_on_tiles(eng, m, k, G):
    """Member-block counts 1 .. 8, k no multiple of four, ragged last tiles, fewer points than a tile has wavefronts' worth,
    rows one below / at / one above a pass of eight and of sixteen, many passes."""
    X, W, ref = local_case(m, k, G)
    Xt, Wt = t64(X), t64(W)
    set_option("apply64", 1)
    got = eng.apply_local_weights(Xt, Wt)
    name = last_kernel()
    assert name == "%s<%d>" % (TILE, (k + 15) // 16), name
    check(got, ref, "per point m %d k %d G %d (%s)" % (m, k, G, name))
    g0, g1 = sub_range(G)
    sub = eng.apply_local_weights(Xt, Wt[g0:g1].contiguous(), g0, g1)
    assert TILE in last_kernel()
    assert torch.equal(sub, got[:, :, g0:g1])
    assert torch.equal(eng.apply_local_weights(Xt, Wt), got)
    with pytest.raises(ValueError):
        eng.apply_local_weights(Xt, Wt[:5].contiguous())


def test_per_point_transform_past_128_members_falls_back(eng):
    m, k, G = 3, 129, 40
    X, W, ref = local_case(m, k, G)
    set_option("apply64", 1)
    got = eng.apply_local_weights(t64(X), t64(W))
    assert last_kernel() == FALLBACK
    check(got, ref, "per point k 129 (fallback)")


def test_options_apply64_and_tile_keep_the_fallback(eng):
    m, k, G = 9, 40, 999
    X, W, ref = local_case(m, k, G)
    Xt, Wt = t64(X), t64(W)
    set_option("apply64", 1)
    tile = eng.apply_local_weights(Xt, Wt)
    assert TILE in last_kernel()
    set_option("apply64", 0)
    off = eng.apply_local_weights(Xt, Wt)
    assert last_kernel() == FALLBACK
    set_option("apply64", 1)
    set_option("tile", 0)
    notile = eng.apply_local_weights(Xt, Wt)
    assert last_kernel() == FALLBACK
    assert torch.equal(off, notile)
    check(off, ref, "per point, apply64 = 0")
    d = rel_fro(off.cpu().numpy(), tile.cpu().numpy())
    print("\n[apply64] tile kernel against fallback at (9, 40, 999): rel. Frobenius %.3e" % d)
    assert d < TOL
    # ... and the global transform
    Xg, Wg, refg = global_case(3, 40, 1000)
    set_option("tile", 1)
    gt = eng.apply_weights(t64(Xg), t64(Wg))
    assert GTILE in last_kernel()
    set_option("apply64", 0)
    gf = eng.apply_weights(t64(Xg), t64(Wg))
    assert last_kernel().startswith(GFALLBACK)
    assert rel_fro(gf.cpu().numpy(), gt.cpu().numpy()) < TOL


@pytest.mark.parametrize("m,k,G", [(16, 40, 1000), (1, 40, 1000)])
def test_default_option(eng, m, k, G):
    """apply64 = -1: the kernel the measurement chose for the shape (not asserted which), the same contract"""
    from torch_assimilate_amd import _cabi
    import ctypes as C
    v = C.c_int(0)
    assert _cabi.lib().mia_get_option(b"apply64", C.byref(v)) == 0 and v.value == -1
    X, W, ref = local_case(m, k, G)
    got = eng.apply_local_weights(t64(X), t64(W))
    name = last_kernel()
    assert name == FALLBACK or name == TILE + "<3>", name
    check(got, ref, "per point m %d k %d G %d, default option (%s)" % (m, k, G, name))
    Xg, Wg, refg = global_case(3, 40, 1000)
    gg = eng.apply_weights(t64(Xg), t64(Wg))
    name = last_kernel()
    assert name.startswith(GFALLBACK) or name == GTILE + "<3>", name
    check(gg, refg, "global m 3 k 40 G 1000, default option (%s)" % name)


# ---- 2. non-finite input stays where it is ---------------------------------------------------------------------------------------
def test_non_finite_input_stays_where_it_is(eng):
    m, k, G = 9, 40, 100
    X, W, _ = local_case(m, k, G)
    set_option("apply64", 1)
    clean = eng.apply_local_weights(t64(X), t64(W))
    Xb, Wb = X.copy(), W.copy()
    Xb[2, 5, 37] = np.nan
    Wb[53, 0, 0] = np.nan
    got = eng.apply_local_weights(t64(Xb), t64(Wb))
    assert TILE in last_kernel()
    # x[2][5][37] enters the mean of (2, ., 37): every new member of that row and point.  W_53[0][0] is a term of new member 0
    # of point 53 alone, in every state row (column 0 of W_53 holds it, the other columns never meet it): the oracle's own mask.
    want = np.zeros((m, k, G), dtype=bool)
    want[2, :, 37] = True
    want[:, 0, 53] = True
    assert np.array_equal(~np.isfinite(O.apply_weights(Xb, Wb)), want)
    bad = ~torch.isfinite(got).cpu().numpy()
    assert not bad[:, :, [g for g in range(G) if g not in (37, 53)]].any()       # nothing leaves the two points
    assert np.array_equal(bad, want)
    keep = torch.as_tensor(~want, device=DEV)
    assert torch.equal(got[keep], clean[keep])
    # the global transform: a NaN in x[v][.][g] stays in outputs (v, ., g)
    Xg, Wg, _ = global_case(3, 40, 1000)
    cg = eng.apply_weights(t64(Xg), t64(Wg))
    Xn = Xg.copy()
    Xn[1, 7, 333] = np.inf
    gg = eng.apply_weights(t64(Xn), t64(Wg))
    assert GTILE in last_kernel()
    wantg = np.zeros(Xg.shape, dtype=bool)
    wantg[1, :, 333] = True
    assert np.array_equal(~torch.isfinite(gg).cpu().numpy(), wantg)
    keepg = torch.as_tensor(~wantg, device=DEV)
    assert torch.equal(gg[keepg], cg[keepg])


# ---- 3. one weight matrix for all points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,G", GLOBAL_SHAPES)
def test_global_transform_on_tiles(eng, m, k, G):
    X, W, ref = global_case(m, k, G)
    Xt, Wt = t64(X), t64(W)
    set_option("apply64", 1)
    got = eng.apply_weights(Xt, Wt)
    name = last_kernel()
    assert name == "%s<%d>" % (GTILE, (k + 15) // 16), name
    check(got, ref, "global m %d k %d G %d (%s)" % (m, k, G, name))
    for g0, g1 in ((0, 1), (5, min(69, G)), (G // 2, G)):
        sub = eng.apply_weights(Xt, Wt, g0, g1)
        assert torch.equal(sub, got[:, :, g0:g1]), (g0, g1)
    assert torch.equal(eng.apply_weights(Xt, Wt), got)


def test_global_transform_past_128_members_falls_back(eng):
    X, W, ref = global_case(2, 129, 70)
    set_option("apply64", 1)
    got = eng.apply_weights(t64(X), t64(W))
    assert last_kernel() == "apply_weights_kernel<double, 64, false>"        # (k = 129: W no longer fits the LDS beside the columns)
    check(got, ref, "global k 129 (fallback)")


# ---- 4. through the classes -------------------------------------------------------------------------------------------------------
def test_letkf_with_a_weight_file_in_the_default_dtype(mia, eng, tmp_path):
    """filter.py:157-164 with a weight_save_path: estimate_weights, the file, then the transform this file is about"""
    G, k = 203, 40
    case = O.synthetic_case(G, k, 2, seed=61)
    state = np.random.RandomState(62).normal(size=(3, k, G))
    state[0] += 300.0
    ref = O.letkf_analysis(state, case["grid_x"], case["obs_x"], case["yb"], case["d"], 10.0, 1.1)[0]
    for opt in (1, -1):
        set_option("apply64", opt)
        f = mia.LETKF(localization=mia.GaspariCohn(10.0, mia.AbsoluteDistance()), inf_factor=1.1,
                      weight_save_path=str(tmp_path / ("w%d.nc" % (opt + 1))))
        xa = f.analyse_arrays(state, case["yb"], case["d"], grid_coords=case["grid_x"], obs_coords=case["obs_x"])
        name = last_kernel()
        assert name != "" and (opt < 0 or name == TILE + "<3>"), name
        assert xa.dtype == torch.float64 and rel_fro(xa.cpu().numpy(), ref) <= TOL64


def test_global_etkf_in_the_default_dtype(mia, eng, golden):
    """config 1 of the golden vectors (the size of tests/test_gpu_parity.py::test_c1_global_etkf) through the class"""
    g = golden("g7_synthetic_configs.npz")
    set_option("apply64", 1)
    xa = mia.ETKF(inf_factor=1.1, dtype=torch.float64, engine=eng).analyse_arrays(g["c1_state"], g["c1_yb"], g["c1_d"])
    assert GTILE in last_kernel(), last_kernel()
    assert rel_fro(xa.cpu().numpy(), g["c1_1p1_analysis"]) < TOL64

"""Every float64 eigensolver path against 50 digits, point by point (tests/golden/g10_wide_spectra*.npz, see
tests/wide_spectra_cases.py and tests/test_wide_spectra_reference.py): the Jacobi kernel of csrc/letkf_wave.hip -- which redoes
what every matrix-function kernel declines and is the reference of tools/stress_*.py -- and csrc/etkf_global.hip's own Jacobi, on
local problems with lambda_max / reg = kappa up to 3e9: graded, clustered, exactly repeated and rank-deficient spectra, odd
(padded) and even orders, the dual (p <= k) and the primal (p > k) form, 64 and 256 threads, with and without the weights.

The float64 oracle cannot referee these cases (its own error against 50 digits is c u kappa, c up to c_ref = 1.54, u = 2^-52:
6.6e-7 at kappa 2.7e9).  The contract is 1e-10, or 4 x the reference's own float64 error where that is larger:
tol(block) = max(1e-10, 4 c_ref u kappa) per grid point; float32 arrays: 1e-5.

Geometry: the blocks of one ensemble size and one form become grid points 1000 apart, each with its observations at exactly its
coordinate and a radius of 1: every list is exactly its block, every taper weight exactly 1.  (One launch is dual or primal as
a whole -- p_max <= k --, hence one grid per form; the block at inf = 1.0 is a grid of its own.)

Observed on MI355X with c_ref = 1.543: worst error / tol over the blocks of a family (all k, both forms), the worst error itself
and the largest sweep count (flag bits 8-15; the cap is 24).  No flag on any route.

  route                                          graded  twolevel  repeated  deficient  weak   worst error       sweeps
  Jacobi kernel f64, analysis                    0.044   0.234     0.102     0.241      0.000  8.7e-7 (k 2.7e9)  15
  Jacobi kernel f64 with W, analysis             0.039   0.136     0.045     0.232      0.000  4.9e-7            16
  Jacobi kernel f64 with W, weights              0.033   0.186     0.059     0.118      0.000  3.2e-7            16
  LETKF.analyse_arrays, default dtype            0.044   0.234     0.102     0.241      0.000  8.7e-7            15
  LETKF.estimate_weights_arrays, default dtype   0.033   0.186     0.059     0.118      0.000  3.2e-7            16
  float32 arrays, matfun + float64 redo (1e-5)   0.003   0.087     0.003     0.003      0.005  8.7e-7            15
  float32 tile route + float64 redo (1e-5)       0.003   0.004     0.003     0.003      0.004  4.3e-8            7
  global ETKF f64, weights                       0.141   0.236     0.081     0.216      0.000  7.8e-7 (k 2.4e9)  -

The dual form alone stays below 1.1e-10 everywhere (1e-14 at kappa 2e9; 1.05e-10 on exactly repeated observations at k = 16,
kappa 1.6e6, where eigenvalues are exactly zero): the u kappa term belongs to the primal form, as it does to the oracle.
"""
import warnings

import numpy as np
import pytest
import torch

import wide_spectra_cases as WS
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS = [(k, form, inf) for k in (16, 27, 40, 64) for form, inf in (("dual", 1.1), ("primal", 1.1), ("dual", 1.0))]
TILE_KERNELS = ("tile64", "dense64", "patch64", "wide64", "stream64")


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


@pytest.fixture(scope="module")
def fixture():
    return WS.load()


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def last_kernel():
    from torch_assimilate_amd import _cabi
    return _cabi.last_analysis_kernel()


def f32_first(eng):
    """a float32 analysis, so that the reported kernel name is known to be fresh (letkf_wave.hip never reports one)"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    eng.analysis(dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32), nb, 1.1)
    torch.cuda.synchronize()
    name = last_kernel()
    assert name and not any(t in name for t in TILE_KERNELS)
    return name


def group_of(fixture, key):
    k, form, inf = key
    return [b for b in fixture[0] if b["k"] == k and b["inf"] == inf and ("dual" if b["p"] <= k else "primal") == form]


def make_case(blocks):
    """Block b as grid point b at x = 1000 b with its p observations at exactly that coordinate."""
    grid = 1000.0 * np.arange(len(blocks))
    return dict(grid=grid, obs=np.concatenate([np.full(b["p"], grid[i]) for i, b in enumerate(blocks)]),
                yb=np.concatenate([b["yb"] for b in blocks], axis=1), d=np.concatenate([b["d"] for b in blocks]),
                state=np.stack([b["x"] for b in blocks], axis=-1), first=np.cumsum([0] + [b["p"] for b in blocks]))


def lists_of(eng, case, blocks):
    """Per-point lists at radius 1: exactly the blocks, every weight exactly 1."""
    nb = eng.localize(case["grid"], case["obs"], [1.0])
    cnt, idx, w = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy(), nb.w.cpu().numpy()
    assert cnt.tolist() == [b["p"] for b in blocks] and nb.p_max == max(b["p"] for b in blocks)
    for g, b in enumerate(blocks):
        assert sorted(idx[g, :cnt[g]].tolist()) == list(range(case["first"][g], case["first"][g + 1]))
        assert (w[g, :cnt[g]] == 1.0).all()
    return nb


def check(got, blocks, c_ref, key, what, tol32=False):
    """``got`` (G, ...) against the fixture's ``key`` of every block, point by point."""
    err = np.array([WS.rel_fro(got[g], b[key]) for g, b in enumerate(blocks)])
    tol = np.array([WS.TOL32 if tol32 else WS.tol(b, c_ref) for b in blocks])
    fams = sorted({b["family"] for b in blocks})
    worst = {f: max(err[g] / tol[g] for g, b in enumerate(blocks) if b["family"] == f) for f in fams}
    print("\n[wide spectra] %s %s: worst %.3e (block %d, kappa %.2e); error / tol by family: %s" % (
        what, key, err.max(), blocks[int(err.argmax())]["index"], blocks[int(err.argmax())]["kappa"],
        ", ".join("%s %.3f" % (f, worst[f]) for f in fams)))
    bad = [(b["index"], b["family"], b["p"], "%.2e" % b["kappa"], "%.3e" % err[g], "%.3e" % tol[g])
           for g, b in enumerate(blocks) if not err[g] <= tol[g]]
    assert not bad, (what, key, bad)


def clean(flags, what):
    """Low byte 0 at every point (no MIA_FLAG_NOCONV, no leftover MIA_FLAG_RETRY); returns the largest count of bits 8-15."""
    fl = flags.cpu().numpy()
    assert not (fl & 0xff).any(), (what, fl & 0xff)
    top = int(((fl >> 8) & 0xff).max())
    print("[wide spectra] %s: flags clean, bits 8-15 at most %d" % (what, top))
    return top


def points_first(xa):
    return np.moveaxis(xa.cpu().numpy(), -1, 0)          # (m, k, G) -> (G, m, k)


def n_strong(blocks):
    """Blocks every Chebyshev route must decline: T = lambda_max / reg >= 686 needs a degree of 26 / log(rho) ~ 13 sqrt(T) > 340
    in float64 (cap 127) and more than the float32 cap of 62; the weak family (T ~ 1e-16) needs the smallest degree."""
    assert all(b["kappa"] > 600 or b["family"] == "weak" for b in blocks)
    return sum(b["family"] != "weak" for b in blocks)


def test_every_block_is_in_exactly_one_grid(fixture):
    seen = sorted(b["index"] for key in GROUPS for b in group_of(fixture, key))
    assert seen == list(range(len(fixture[0])))
    assert all(1 <= len(group_of(fixture, key)) <= 20 for key in GROUPS)


# ---- 1. the Jacobi kernel in float64, without and with the weights -------------------------------------------------------------
@pytest.mark.parametrize("key", GROUPS, ids=lambda k: "k%d-%s-inf%.1f" % k)
def test_jacobi_kernel_float64(eng, fixture, key):
    blocks, c_ref = group_of(fixture, key), fixture[1]
    case = make_case(blocks)
    nb = lists_of(eng, case, blocks)
    X, Yb, D = dev(case["state"]), dev(case["yb"]), dev(case["d"])
    what = "Jacobi f64 k=%d %s inf=%.1f" % key
    before = f32_first(eng)
    xa, fl = eng.analysis(X, Yb, D, nb, key[2], method="eig", return_flags=True)
    torch.cuda.synchronize()
    clean(fl, what)
    check(points_first(xa), blocks, c_ref, "xa", what)
    # with W the kernel runs its second stopping rule (full convergence: W takes the diagonal part only)
    xw, W, flw = eng.analysis(X, Yb, D, nb, key[2], method="eig", return_weights=True, return_flags=True)
    torch.cuda.synchronize()
    assert last_kernel() == before                        # no tile kernel supplied either result
    clean(flw, what + " with W")
    check(points_first(xw), blocks, c_ref, "xa", what + " with W")
    check(W.cpu().numpy(), blocks, c_ref, "W", what + " with W")


# ---- 2. the default call in the default dtype: a tile kernel declines, the Jacobi kernel redoes -------------------------------
@pytest.mark.parametrize("key", GROUPS, ids=lambda k: "k%d-%s-inf%.1f" % k)
def test_default_call_float64(mia, eng, fixture, key):
    blocks, c_ref = group_of(fixture, key), fixture[1]
    case = make_case(blocks)
    what = "LETKF f64 k=%d %s inf=%.1f" % key
    f = mia.LETKF(mia.GaspariCohn(1.0, mia.AbsoluteDistance()), key[2])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # (the class warns where a point carries MIA_FLAG_NOCONV / NONFINITE)
        xa = f.analyse_arrays(case["state"].astype(np.float64), case["yb"].astype(np.float64), case["d"].astype(np.float64),
                              grid_coords=case["grid"], obs_coords=case["obs"])
        W = f.estimate_weights_arrays(case["yb"].astype(np.float64), case["d"].astype(np.float64), grid_coords=case["grid"],
                                      obs_coords=case["obs"])
    assert xa.dtype == torch.float64 and W.dtype == torch.float64
    check(points_first(xa), blocks, c_ref, "xa", what + " analyse_arrays")
    check(W.cpu().numpy(), blocks, c_ref, "W", what + " estimate_weights_arrays")
    # the same engine call with the decline counter and the flags in the caller's hands
    nb = lists_of(eng, case, blocks)
    X, Yb, D = dev(case["state"]), dev(case["yb"]), dev(case["d"])
    f32_first(eng)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xe, fl = eng.analysis(X, Yb, D, nb, key[2], return_flags=True, retry=retry)
    torch.cuda.synchronize()
    kern = last_kernel()
    print("\n[wide spectra] %s: %s declined %d of %d points" % (what, kern, int(retry.item()), len(blocks)))
    assert any(t in kern for t in TILE_KERNELS), kern
    assert int(retry.item()) == n_strong(blocks) > 0
    clean(fl, what + " engine.analysis")
    assert torch.equal(xe, xa)
    res = None
    if key[0] >= eng.WEIGHTS64_AUTO_MIN_K:                # what estimate_weights_arrays runs from this ensemble size on
        res = eng.weights64(Yb, D, nb, key[2], return_flags=True, defer_retry=True)
    if res is not None:
        We, flw, finish = res
        assert finish() == n_strong(blocks)
        torch.cuda.synchronize()
        clean(flw, what + " engine.weights64")
        assert torch.equal(We, W)
    else:
        assert key[0] < eng.WEIGHTS64_AUTO_MIN_K or key[1] == "primal"


# ---- 3. float32 arrays, redone in float64 arithmetic ----------------------------------------------------------------------------
@pytest.mark.parametrize("key", GROUPS, ids=lambda k: "k%d-%s-inf%.1f" % k)
def test_float32_arrays_are_redone_in_float64(eng, fixture, key):
    blocks, c_ref = group_of(fixture, key), fixture[1]
    case = make_case(blocks)
    nb = lists_of(eng, case, blocks)
    G, P = len(blocks), len(case["obs"])
    X, Yb, D = dev(case["state"], torch.float32), dev(case["yb"], torch.float32), dev(case["d"], torch.float32)
    what = "f32 arrays k=%d %s inf=%.1f" % key
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xa, fl = eng.analysis(X, Yb, D, nb, key[2], method="matfun", return_flags=True, retry=retry)
    torch.cuda.synchronize()
    print("\n[wide spectra] %s: matfun declined %d of %d points" % (what, int(retry.item()), G))
    assert int(retry.item()) >= n_strong(blocks) > 0      # ... and mia_letkf_analysis_retry_f32 redid them
    clean(fl, what + " matfun")
    check(points_first(xa), blocks, c_ref, "xa", what + " matfun + redo", tol32=True)
    if key[1] == "primal":
        return                                            # (the tile route is the dual form: p_max <= k)
    # the tile route: sixteen unrelated blocks share a tile, so a full tile's union cannot fit its slots -- it is reported, flagged
    # and not analysed (never truncated), and the caller hands its points to the eigensolver; a tile that fits declines the strong
    # points itself
    tiles = None
    for extra in range(6):
        if not eng.tile_route_applies(X, nb.p_max, extra, P=P, n_points=G):
            break
        tiles = eng.localize_tiles(case["grid"], case["obs"], [1.0], nb.p_max, extra_blocks=extra)
        if tiles.stats.tolist()[1] == 0:
            break
    assert tiles is not None, "the tile route refused a dual shape"
    longest, n_over = tiles.stats.tolist()
    hdr = tiles.unpack()[0]
    over = np.repeat(hdr[:, 0] < 0, 16)[:G]
    # (bit 30, MIA_TILE_BOX_OVERFLOW: points 1000 radii apart also span more index cells than a tile's scan takes)
    assert longest == nb.p_max and int((hdr[:, 0] < 0).sum()) == n_over & ~(1 << 30)
    xt, ft, rt = eng.analysis_tiles(X, eng.pack_split(Yb, D), P, tiles, key[2])
    torch.cuda.synchronize()
    fth = ft.cpu().numpy()
    assert ((fth[over] & 0xff) == 1).all() and np.isnan(points_first(xt)[over]).all()           # loud
    assert not (fth[~over] & 1).any() and np.isfinite(points_first(xt)[~over & ((fth & 8) == 0)]).all()
    strong = np.array([b["family"] != "weak" for b in blocks])
    assert ((fth[~over] & 8) != 0)[strong[~over]].all() and int(rt.item()) == int(((fth & 8) != 0).sum())
    print("[wide spectra] %s: tiles with %d extra blocks, %d of %d points in overflowing tiles, %d declined" % (
        what, tiles.extra_blocks, int(over.sum()), G, int(rt.item())))
    if sum(b["p"] for b in blocks[:16]) > 96:             # (a tile offers at most 96 slots)
        assert over[:16].all()
    if G == 1:
        assert not over.any() and int(rt.item()) == 1     # one block alone fits: the tile kernel itself declined it
    ft[torch.as_tensor(over, device=DEV)] = 8             # the caller's answer to an overflow: the eigensolver, point by point
    eng.retry_points(X, Yb, D, nb, key[2], xt, ft)
    torch.cuda.synchronize()
    clean(ft, what + " tiles + redo")
    check(points_first(xt), blocks, c_ref, "xa", what + " tiles + redo", tol32=True)


# ---- 4. the global ETKF's own Jacobi (csrc/etkf_global.hip) ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 27, 40, 64])
def test_global_etkf_float64(eng, fixture, k):
    blocks, c_ref = [b for b in fixture[0] if b["k"] == k], fixture[1]
    got = []
    for b in blocks:
        W, fl = eng.etkf_weights(dev(b["yb"]), dev(b["d"]), b["inf"], return_flags=True)
        assert int(fl.item()) & 0xff == 0, (b["index"], int(fl.item()))          # (this flag word carries no sweep count)
        got.append(W.cpu().numpy())
    check(got, blocks, c_ref, "W", "global ETKF f64 k=%d" % k)

"""Every kernel that works on tiles of sixteen grid points, on a grid of MORE THAN 65 536 TILES: 1 064 597 points in ONE call.

From 65 537 tiles on the launch is two-dimensional (gx = 65 536, gy = ceil(ntile / gx)); the kernel rebuilds its tile index from
blockIdx.y * gridDim.x + blockIdx.x, drops the blocks past ntile in the partly filled second row, and most kernels pass the index
through the block-to-tile map over the eight XCDs (here with ntile & 7 = 2).  A mistake there writes some tiles twice and others
never.  The case and its reference -- EVERY point has one -- are tests/large_grid_cases.py's: a network that repeats every 976
points (61 tiles) under a state that is random everywhere, pinned on the CPU by tests/test_large_grid_reference.py.  Tolerances
are the routes' own: 1e-10 (float64) and 1e-5 (float32), per point and overall -- for the whole (m, k) block of a point and for
its first state row alone (the second row carries a mean of 250, which flatters a relative error).

A tile that is never written must not pass.  Every route therefore writes into POISONED memory: outputs prefilled with NaN and
flag words with 0xffffffff where the entry takes them, and, for what the library allocates itself with torch.empty, torch's
fill of uninitialised memory (NaN / the largest integer, low byte 0xff) switched on around the call -- the caching allocator would
otherwise hand a route the block an earlier route with the same answer has just freed.  The printed 'call' times are one
synchronised call each, fills included: indicative, not measurements."""
import contextlib
import time

import numpy as np
import pytest
import torch

import large_grid_cases as L
from kernel_cases import product_kernels
from oracle import letkf_oracle as O
from test_gpu_tile2 import TOL32
from test_gpu_tile64 import TOL64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = L.G_LARGE
_MEMO = {}


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


@pytest.fixture(scope="module", autouse=True)
def release_the_large_case():
    """the device tensors and the host references of this module go back when it is done"""
    yield
    _MEMO.clear()
    for fn in (L.large_case, L.large_weights, L.large_analysis):
        fn.cache_clear()
    torch.cuda.empty_cache()


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def last_kernel():
    from torch_assimilate_amd import _cabi
    return _cabi.last_analysis_kernel()


def last_transform():
    from torch_assimilate_amd import _cabi
    return _cabi.last_transform_kernel()


def gpu_case(eng, network, dtype=torch.float64, k=L.K, m=L.M):
    """the large case on the device with its per-point lists: built once per module, never written to"""
    key = (network, dtype, k, m)
    if key not in _MEMO:
        case = L.large_case(network, k, m)
        if ("nb", network) not in _MEMO:
            nb = eng.localize(case["grid_x"], case["obs_x"], [case["c"]])
            cnt = nb.cnt.cpu().numpy()
            if network == "sparse":
                assert nb.p_max == 8 <= L.K and set(cnt[9:-9].tolist()) == {7, 8}
            else:
                assert nb.p_max == 15 > L.K and set(cnt[9:-9].tolist()) == {15}
            _MEMO[("nb", network)] = nb
        _MEMO[key] = dict(case=case, nb=_MEMO[("nb", network)], X=dev(case["state"], dtype), yb=dev(case["yb"], dtype),
                          d=dev(case["d"], dtype))
    return _MEMO[key]


def fresh(eng, dtype):
    """a small analysis of the OTHER precision, so that the kernel name read after the route under test is that route's"""
    case = O.synthetic_case(64, 20, 2, seed=3)
    nb = eng.localize(case["grid_x"], case["obs_x"], [5.0])
    other = torch.float32 if dtype == torch.float64 else torch.float64
    eng.analysis(dev(case["state"], other), dev(case["yb"], other), dev(case["d"], other), nb, 1.1)
    torch.cuda.synchronize()


@contextlib.contextmanager
def poisoned():
    """Inside, every torch.empty -- the library's own included -- comes back filled: NaN for floating point, the largest value for
    integers (low byte 0xff).  Checked on the spot, so that a torch without the switch fails the test instead of weakening it."""
    import torch.utils.deterministic as det
    was = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
           det.fill_uninitialized_memory)
    torch.use_deterministic_algorithms(True, warn_only=True)
    det.fill_uninitialized_memory = True
    try:
        assert bool(torch.isnan(torch.empty(4096, dtype=torch.float32, device=DEV)).all())
        assert bool(torch.isnan(torch.empty(4096, dtype=torch.float64, device=DEV)).all())
        assert bool(((torch.empty(4096, dtype=torch.int32, device=DEV) & 0xff) == 0xff).all())
        yield
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
        det.fill_uninitialized_memory = was[2]


def nan_out(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def poison_flags(n=G):
    return torch.full((n,), -1, dtype=torch.int32, device=DEV)


class Timer:
    def __enter__(self):
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.s = time.perf_counter() - self.t0


def report(route, pp, fro, tol, kern, secs, row0=None):
    """the printed line of a route -- point count, overall and worst per-point error, the three boundary regions, kernel, time of
    the call -- and the bounds"""
    assert pp.shape == (G,)
    reg = ", ".join("%s %.3e" % (name, pp[a:b].max()) for name, a, b in L.regions(G))
    first = "" if row0 is None else "; first state row alone %.3e / worst point %.3e" % (row0[1], row0[0].max())
    print("\n[large grid] %s: %d points, rel. Frobenius %.3e, worst grid point %.3e (point %d)%s; %s; kernel %s; call %.2f ms"
          % (route, pp.shape[0], fro, pp.max(), int(pp.argmax()), first, reg, kern or "(not reported)", 1e3 * secs))
    assert fro <= tol, route
    assert pp.max() <= tol, route
    if row0 is not None:
        assert row0[1] <= tol and row0[0].max() <= tol, route


def check_flags(fl, declined, route):
    assert declined == 0, route                                        # no point is declined
    assert fl.shape[0] == G and int((fl & 0xff).max().item()) == 0, route


def check_analysis(route, xa, ref, tol, kern, secs):
    from oracle_pool import per_point_errors
    assert tuple(xa.shape) == ref.shape and bool(torch.isfinite(xa).all()), route
    got = xa.cpu().numpy()
    pp, fro = per_point_errors(got, ref)
    report(route, pp, fro, tol, kern, secs, per_point_errors(got[:1], ref[:1]) if ref.shape[0] > 1 else None)


def check_weights(route, W, refw, tol, kern, secs):
    assert tuple(W.shape) == (G, refw.k, refw.k) and bool(torch.isfinite(W).all()), route
    pp, fro = refw.errors(W.cpu().numpy())
    report(route, pp, fro, tol, kern, secs)


# ---- float64 analysis routes of engine.analysis ----------------------------------------------------------------------------------
ANALYSIS64 = [("matfun64", "sparse", "letkf", "letkf_tile64_kernel<"), ("dense64", "dense", "letkf", "letkf_dense64_kernel<"),
              ("stream64", "dense", "letkf", "letkf_stream64_kernel<"), ("wide64", "sparse", "letkf", "letkf_wide64_kernel<"),
              ("patch64", "dense", "letkf", "letkf_patch64_kernel<"), ("rbf64", "sparse", "rbf", "lketkf_tile64_kernel<"),
              ("kern64", "sparse", "ornuhl", "lketkf_tile64_kernel<")]


@pytest.mark.parametrize("method,network,core,kernel", ANALYSIS64, ids=[a[0] for a in ANALYSIS64])
def test_float64_analysis_routes(eng, method, network, core, kernel):
    """letkf_tile64, letkf_dense64, letkf_stream64, letkf_wide64, letkf_patch64 (with tile_union_census_kernel: the map holds the
    strips of sixteen consecutive points in REVERSED tile order, 66 538 entries, so the census kernel's own decode crosses the
    boundary too), lketkf_tile64 in its RBF and its expression instantiation: all G points in one call, into an output of NaN
    and flag words of 0xffffffff."""
    c = gpu_case(eng, network)
    kw = {}
    if method == "patch64":
        kw["tile_points"] = torch.from_numpy(L.reversed_strips(G))
    if method == "rbf64":
        kw["rbf_gamma"] = L.RBF_GAMMA
    if method == "kern64":
        kw.update(kernel_program=product_kernels()[L.EXPR_KERNEL].program(), kernel_psd=True)
    ref = L.large_analysis(network, core, L.K, L.M)
    fresh(eng, torch.float64)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, fl = nan_out((L.M, L.K, G), torch.float64), poison_flags()
    with poisoned(), Timer() as t:
        res = eng.analysis(c["X"], c["yb"], c["d"], c["nb"], L.INF, method=method, retry=retry, out=out, flags=fl, **kw)
    assert res is out
    kern = last_kernel()
    assert kernel in kern, kern
    if method in ("rbf64", "kern64"):      # lketkf_tile64_kernel<UT, NR, ST>: ST 0 is the RBF form, 1 / 2 / 7 the expression forms
        assert kern.rstrip(">").endswith(", 0") == (method == "rbf64"), kern
    check_flags(fl, int(retry.item()), method)
    check_analysis(method, out, ref, TOL64, kern, t.s)


# ---- float64 weights -------------------------------------------------------------------------------------------------------------
WEIGHTS64 = [("weights64", "sparse", "letkf_weights64_kernel<"), ("weights_wide64", "sparse", "letkf_wide64w_kernel<"),
             ("weights_stream64", "dense", "letkf_stream64w_kernel<")]


@pytest.mark.parametrize("entry,network,kernel", WEIGHTS64, ids=[a[0] for a in WEIGHTS64])
def test_float64_weight_routes(eng, entry, network, kernel):
    """letkf_tile64w, letkf_wide64w, letkf_stream64w: the weights of all G points in one call, into W of NaN (the entries
    allocate their flag words themselves: poisoned through torch's fill)"""
    c = gpu_case(eng, network)
    refw = L.large_weights(network, "letkf", L.K, L.M)
    fresh(eng, torch.float64)
    out = nan_out((G, L.K, L.K), torch.float64)
    with poisoned(), Timer() as t:
        res = getattr(eng, entry)(c["yb"], c["d"], c["nb"], L.INF, return_flags=True, defer_retry=True, out=out)
        assert res is not None, entry
        W, fl, finish = res
        declined = finish()
    assert W is out
    kern = last_kernel()
    assert kernel in kern, kern
    check_flags(fl, declined, entry)
    check_weights(entry, W, refw, TOL64, kern, t.s)


# ---- float64 IEnKS update --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,kernel", [("tile64", "lienks_update64_kernel<"), ("wide64", "lienks_wide64_kernel<")])
def test_ienks_update_routes(eng, method, kernel):
    """lienks_tile64, lienks_wide64: bundle variant, per-point incoming weights that repeat with the network and are far from
    the identity; into W of NaN"""
    c = gpu_case(eng, "sparse")
    refw = L.large_weights("sparse", "ienks", L.K, L.M)
    w_in = dev(c["case"]["w_in_period"])[torch.arange(G, device=DEV) % L.PERIOD].contiguous()
    yb = (c["yb"] * L.IENKS_EPS).contiguous()
    fresh(eng, torch.float64)
    out = nan_out((G, L.K, L.K), torch.float64)
    with poisoned(), Timer() as t:
        W, fl, finish = eng.ienks_update(w_in, yb, c["d"], c["nb"], 1.0, L.IENKS_EPS, return_flags=True, method=method,
                                         defer_retry=True, out=out)
        declined = finish()
    assert W is out
    kern = last_kernel()
    assert kernel in kern, kern
    check_flags(fl, declined, "ienks " + method)
    check_weights("ienks_update " + method, W, refw, TOL64, kern, t.s)


# ---- float32 routes on tile lists ------------------------------------------------------------------------------------------------
def tile_lists(eng, network, k=L.K, m=L.M, extra_blocks=None):
    """tile lists and split records of the large case (float32 routes), built once"""
    key = ("tiles", network, k, m, extra_blocks)
    if key not in _MEMO:
        c = gpu_case(eng, network, torch.float32, k, m)
        case, nb = c["case"], c["nb"]
        if extra_blocks is None:
            tiles = eng.localize_tiles(case["grid_x"], case["obs_x"], [case["c"]], nb.p_max)
            if tiles.stats.tolist()[1]:        # sixteen consecutive points see more than p_max + 8 observations: sixteen more slots
                tiles = eng.localize_tiles(case["grid_x"], case["obs_x"], [case["c"]], nb.p_max, extra_blocks=1)
        else:
            tiles = eng.localize_tiles(case["grid_x"], case["obs_x"], [case["c"]], nb.p_max, extra_blocks=extra_blocks)
        assert tiles.stats.tolist() == [nb.p_max, 0]
        _MEMO[key] = (c, tiles, eng.pack_split(c["yb"], c["d"]), case["yb"].shape[1])
    return _MEMO[key]


def test_float32_tile2_route(eng):
    """letkf_tile2: localize_tiles + pack_split + analysis_tiles, into an output of NaN (the entry zeroes its own flag words; a
    tile the kernel never reached shows in the output)"""
    c, tiles, rec, P = tile_lists(eng, "sparse")
    ref = L.large_analysis("sparse", "letkf", L.K, L.M)
    fresh(eng, torch.float32)
    out = nan_out((L.M, L.K, G), torch.float32)
    with poisoned(), Timer() as t:
        xa, fl, retry = eng.analysis_tiles(c["X"], rec, P, tiles, L.INF, out=out)
    assert xa is out
    kern = last_kernel()
    assert "letkf_tile2_kernel<" in kern, kern
    check_flags(fl, int(retry.item()), "tile2")
    check_analysis("analysis_tiles (tile2)", xa, ref, TOL32, kern, t.s)


K2P = 17


def test_float32_tile2p_route(eng):
    """letkf_tile2p, two wavefronts per tile: instantiated for unions of three sixteen-slot blocks and more and two member blocks
    and more, one state row.  k = 8 has one member block, so this route runs the smallest ensemble its cover accepts for three
    blocks, k = 17 (two member blocks, p_max = 15 <= k), on the dense network with one block added to the tiles' unions (48
    slots for unions of 30 observations) and one state row."""
    c, tiles, rec, P = tile_lists(eng, "dense", K2P, 1, extra_blocks=1)
    assert tiles.ut == 3
    ref = L.large_analysis("dense", "letkf", K2P, 1)
    fresh(eng, torch.float32)
    out = nan_out((1, K2P, G), torch.float32)
    with poisoned(), Timer() as t:
        xa, fl, retry = eng.analysis_tiles(c["X"], rec, P, tiles, L.INF, out=out)
    assert xa is out
    kern = last_kernel()
    assert "letkf_tile2p_kernel<3, 2" in kern, kern
    check_flags(fl, int(retry.item()), "tile2p")
    check_analysis("analysis_tiles (tile2p, k = 17)", xa, ref, TOL32, kern, t.s)


def test_float32_tile2w_route(eng):
    """letkf_tile2w: weights_tiles -- the analysis and the weights of all G points.  The entry takes no buffers and reports no
    kernel name; its analysis and weights are torch.empty, poisoned through torch's fill."""
    c, tiles, rec, P = tile_lists(eng, "sparse")
    ref = L.large_analysis("sparse", "letkf", L.K, L.M)
    with poisoned(), Timer() as t:
        res = eng.weights_tiles(c["X"], rec, P, tiles, L.INF)
    assert res is not None
    xa, W, fl, retry = res
    check_flags(fl, int(retry.item()), "tile2w")
    check_analysis("weights_tiles (tile2w), analysis", xa, ref, TOL32, "", t.s)
    check_weights("weights_tiles (tile2w), weights", W, L.large_weights("sparse", "letkf", L.K, L.M), TOL32, "", t.s)


def test_float32_lketkf_tile_route(eng):
    """lketkf_tile: analysis_tiles_rbf, into an output of NaN"""
    c, tiles, rec, P = tile_lists(eng, "sparse")
    ref = L.large_analysis("sparse", "rbf", L.K, L.M)
    fresh(eng, torch.float32)
    out = nan_out((L.M, L.K, G), torch.float32)
    with poisoned(), Timer() as t:
        res = eng.analysis_tiles_rbf(c["X"], c["yb"], c["d"], tiles, L.INF, L.RBF_GAMMA, out=out)
    assert res is not None
    xa, fl, retry = res
    assert xa is out
    kern = last_kernel()
    assert "lketkf_tile_kernel<" in kern, kern
    check_flags(fl, int(retry.item()), "lketkf_tile")
    check_analysis("analysis_tiles_rbf (lketkf_tile)", xa, ref, TOL32, kern, t.s)


def test_float32_tile_kernel_on_per_point_lists(eng):
    """letkf_tile, the kernel on per-point lists: the float32 engine.analysis(method="matfun") of tests/test_gpu_tile.py"""
    c = gpu_case(eng, "sparse", torch.float32)
    ref = L.large_analysis("sparse", "letkf", L.K, L.M)
    fresh(eng, torch.float32)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, fl = nan_out((L.M, L.K, G), torch.float32), poison_flags()
    with poisoned(), Timer() as t:
        res = eng.analysis(c["X"], c["yb"], c["d"], c["nb"], L.INF, method="matfun", retry=retry, out=out, flags=fl)
    assert res is out
    kern = last_kernel()
    assert "letkf_tile_kernel<" in kern, kern
    check_flags(fl, int(retry.item()), "letkf_tile")
    check_analysis("analysis, float32 matfun (letkf_tile)", out, ref, TOL32, kern, t.s)


def test_float32_fused_step_route(mia, eng):
    """letkf_tile2f: the step driver on one GPU, two steps -- the first builds exact lists through the engine, the second is
    the native step whose wavefronts localise their tiles themselves; the second equals the first bit for bit.  The first
    step's result stays alive and the second step's buffers are torch.empty under torch's fill: what the second step does not
    write is NaN, not the first step's answer."""
    c = gpu_case(eng, "sparse", torch.float32)
    case = c["case"]
    ref = L.large_analysis("sparse", "letkf", L.K, L.M)
    r = mia.ShardedLetkf(torch.device(DEV), 0, 1, radii=[case["c"]], inf_factor=L.INF)
    args = (c["X"], dev(case["grid_x"]), dev(case["obs_x"]), c["yb"], c["d"])
    first = r.assimilate(*args)
    with poisoned(), Timer() as t:
        second = r.assimilate(*args)
    assert second.data_ptr() != first.data_ptr()
    assert r.native_steps == 1 and r.last_flags_ok() and r.last_retries == 0
    kern = r.dominant_kernel_name
    assert kern.startswith("letkf_tile2f_kernel<"), kern
    assert torch.equal(first, second)
    check_analysis("ShardedLetkf.assimilate, step 2 (tile2f)", second, ref, TOL32, kern, t.s)


# ---- the transforms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(torch.float64, TOL64), (torch.float32, TOL32)], ids=["f64", "f32"])
def test_apply_weights_routes(eng, dtype, tol):
    """apply_local_weights with the periodic weights (the reference analysis itself) and apply_weights with ONE matrix, applied
    to the random state of all G points.  These kernels launch a one-dimensional grid (a block per tile, or per four tiles), so
    they never had the gy > 1 gap: what the large grid checks here is the block count and the 64-bit offsets behind it.  In
    float64 the library must report its tile kernels, not the one-point-per-thread kernels it falls back to."""
    c = gpu_case(eng, "sparse", dtype)
    refw = L.large_weights("sparse", "letkf", L.K, L.M)
    idx = torch.arange(G, device=DEV)
    W = dev(refw.period)[idx % L.PERIOD]
    W[:L.PERIOD] = dev(refw.start)
    W[refw.e0:] = dev(refw.end)
    W = W.to(dtype)
    f64 = dtype == torch.float64
    with poisoned(), Timer() as t:
        xa = eng.apply_local_weights(c["X"], W)
    kern = last_transform() if f64 else ""
    assert not f64 or "apply_local64_tile_kernel<" in kern, kern
    check_analysis("apply_local_weights %s" % str(dtype)[6:], xa, L.large_analysis("sparse", "letkf", L.K, L.M), tol, kern, t.s)
    w1 = refw.period[5]
    with poisoned(), Timer() as t:
        xa = eng.apply_weights(c["X"], dev(w1, dtype))
    kern = last_transform() if f64 else ""
    assert not f64 or "apply_global64_tile_kernel<" in kern, kern
    check_analysis("apply_weights %s" % str(dtype)[6:], xa, O.apply_weights(c["case"]["state"], w1), tol, kern, t.s)


# ---- the edge of the 32-bit lane offsets -----------------------------------------------------------------------------------------
# The float64 tile kernels address the state and the output as a wave-uniform 64-bit base plus a 32-bit lane offset, and the host
# admits every leading dimension below the documented bound: k ld 8 < 2^31 for the analysis kernels, (k + 3) ld 8 < 2^32 for the
# two transforms.  Here the entries run through the C ABI on a shard of 203 points (ragged last tile) that ENDS AT THE LAST
# COLUMN of a state of the largest accepted leading dimension, and once more with the OUTPUT at the largest one.  lketkf_tile64
# addresses both through 64-bit offsets and its covers accept every leading dimension: it runs at k ld 8 just above 2^32.
N_EDGE, PAD = 203, 16
LD_64BIT = (1 << 26) + N_EDGE
EDGE = [("matfun", 8, 2, 4.0), ("matfun", 64, 2, 28.0), ("dense", 8, 1, 4.0), ("stream", 8, 1, 4.0), ("wide", 8, 2, 4.0),
        ("wide", 128, 2, 32.0), ("patch", 8, 1, 4.0), ("rbf", 8, 2, 4.0), ("kernel", 8, 2, 4.0), ("apply_local", 8, 2, 4.0),
        ("apply", 8, 2, 4.0)]
EDGE_ENTRY = {"matfun": ("mia_letkf_analysis_matfun_f64", "mia_letkf_matfun_f64_cover", "letkf_tile64_kernel<"),
              "dense": ("mia_letkf_analysis_dense_f64", "mia_letkf_dense_f64_cover", "letkf_dense64_kernel<"),
              "stream": ("mia_letkf_analysis_stream_f64", "mia_letkf_stream_f64_cover", "letkf_stream64_kernel<"),
              "wide": ("mia_letkf_analysis_wide_f64", "mia_letkf_wide_f64_cover", "letkf_wide64_kernel<"),
              "patch": ("mia_letkf_analysis_patch_f64", "mia_letkf_patch_f64_cover", "letkf_patch64_kernel<"),
              "rbf": ("mia_lketkf_rbf_analysis_matfun_f64", "mia_lketkf_rbf_f64_cover", "lketkf_tile64_kernel<"),
              "kernel": ("mia_lketkf_kernel_analysis_matfun_f64", "mia_lketkf_kernel_f64_cover", "lketkf_tile64_kernel<"),
              "apply_local": ("mia_apply_local_weights_f64", "mia_apply_local_f64_cover", "apply_local64_tile_kernel<"),
              "apply": ("mia_apply_weights_f64", "mia_apply_f64_cover", "apply_global64_tile_kernel<")}
TRANSFORMS = ("apply_local", "apply")


@pytest.fixture(scope="module")
def big():
    """one uninitialised buffer that holds the largest state (or output) of this section: 8 x (2^26 + 203) doubles, 4.3 GB"""
    buf = torch.empty(8 * LD_64BIT, dtype=torch.float64, device=DEV)
    yield buf
    del buf
    torch.cuda.empty_cache()


def largest_accepted(ok):
    """the largest leading dimension a cover function accepts, by bisection (None: it accepts 2^40)"""
    assert ok(N_EDGE)
    lo, hi = N_EDGE, 1 << 40
    if ok(hi):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def edge_cover(lib, route, k, p_max, P):
    """(accepts as ldx, accepts as ldo, the documented largest leading dimension or None) of a route's cover function"""
    fn, n = getattr(lib, EDGE_ENTRY[route][1]), N_EDGE
    if route in TRANSFORMS:
        return (lambda ld: fn(1, k, ld, n, n) == 1), (lambda ld: fn(1, k, n, ld, n) == 1), ((1 << 32) - 1) // (8 * (k + 3))
    bound = None if route in ("rbf", "kernel") else ((1 << 31) - 1) // (8 * k)
    return (lambda ld: fn(1, k, p_max, ld, n, n, P) == 1), (lambda ld: fn(1, k, p_max, n, ld, n, P) == 1), bound


def edge_transform(eng, lib, route, case, c):
    """(call(X, ldx, g0, g1, out, ldo, o0), oracle) of a float64 transform on the 203-point problem"""
    entry, _, kernel = EDGE_ENTRY[route]
    k = case["yb"].shape[0]
    w = O.letkf_weights(case["grid_x"], case["obs_x"], case["yb"], case["d"], c, L.INF)
    w = w if route == "apply_local" else w[17]
    wd = dev(w)

    def call(X, ldx, g0, g1, out, ldo, o0):
        rc = getattr(lib, entry)(X.data_ptr(), ldx, 1, k, g0, g1, wd.data_ptr(), out.data_ptr(), ldo, o0, None)
        torch.cuda.synchronize()
        assert rc == 0 and kernel in last_transform(), (rc, last_transform())
    return call, O.apply_weights(case["state"], w)


def edge_analysis(eng, lib, route, case, nb, c):
    """(call(X, ldx, g0, g1, out, ldo, o0), oracle) of a float64 analysis entry on the 203-point problem"""
    from torch_assimilate_amd import _cabi
    entry, _, kernel = EDGE_ENTRY[route]
    n, k = N_EDGE, case["yb"].shape[0]
    core = {"rbf": L.rbf_core, "kernel": L.expr_core}.get(route, O.etkf_weights)
    ref = O.letkf_analysis(case["state"], case["grid_x"], case["obs_x"], case["yb"], case["d"], c, L.INF, core=core)[0]
    rec = eng.pack_obs(dev(case["yb"]), dev(case["d"]), torch.float64)
    mid, extra = (0.0,), ()             # (the arguments between inf_factor and Xa, and those between retry_count and stream)
    if route == "rbf":
        mid = (L.RBF_GAMMA,)
    if route == "kernel":
        ops = product_kernels()[L.EXPR_KERNEL].program()
        prog = (_cabi.KernelOp * len(ops))()
        for i, (op, val) in enumerate(ops):
            prog[i].op, prog[i].value = int(op), float(val)
        mid = (prog, len(ops))
    if route == "patch":
        tp, ub, fits = eng._patch64_map(nb, torch.from_numpy(L.reversed_strips(n)), None, k)
        assert fits
        extra = (tp.data_ptr(), tp.shape[0], ub)

    def call(X, ldx, g0, g1, out, ldo, o0):
        fl, retry = poison_flags(n), torch.zeros(1, dtype=torch.int32, device=DEV)
        fresh(eng, torch.float64)
        rc = getattr(lib, entry)(X.data_ptr(), ldx, 1, k, g0, g1, rec.data_ptr(), rec.shape[0], nb.cnt.data_ptr(),
                                 nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, L.INF, *mid, out.data_ptr(), ldo, o0,
                                 fl.data_ptr(), retry.data_ptr(), *extra, None)
        torch.cuda.synchronize()
        assert rc == 0 and kernel in last_kernel(), (rc, last_kernel())
        assert int(retry.item()) == 0 and int((fl & 0xff).max().item()) == 0
    return call, ref


def padded_run(call, X, ldx, g0, k):
    """the shard into the middle of a small output with PAD untouched columns on either side: the written columns"""
    n = N_EDGE
    out = torch.full((1, k, n + 2 * PAD), -7.0, dtype=torch.float64, device=DEV)
    call(X, ldx, g0, g0 + n, out, n + 2 * PAD, PAD)
    assert bool((out[:, :, :PAD] == -7.0).all()) and bool((out[:, :, PAD + n:] == -7.0).all())
    return out[:, :, PAD:PAD + n]


@pytest.mark.parametrize("route,k,stride,c", EDGE, ids=["%s-k%d" % e[:2] for e in EDGE])
def test_shard_at_the_last_column_of_the_largest_leading_dimension(eng, big, route, k, stride, c):
    """The cover function accepts exactly the documented leading dimensions; at the largest one the entry gives the oracle's
    answer for the 203-point problem (the small 1-D synthetic case of the sweeps) and, bit for bit, what it gives at ld = 203 --
    with the state at that leading dimension and with the output at it; nothing is written beside the shard.  k = 8 everywhere,
    and the largest ensemble of tile64 (64) and of wide64 (128)."""
    from oracle_pool import per_point_errors
    from torch_assimilate_amd import _cabi
    lib, n = _cabi.lib(), N_EDGE
    case = O.synthetic_case(n, k, stride, seed=300 + k, m=1)
    nb = eng.localize(case["grid_x"], case["obs_x"], [c])
    accepts_x, accepts_o, bound = edge_cover(lib, route, k, nb.p_max, case["yb"].shape[1])
    assert largest_accepted(accepts_x) == bound and largest_accepted(accepts_o) == bound
    ld = bound if bound is not None else LD_64BIT
    assert k * ld <= big.numel()
    call, ref = edge_transform(eng, lib, route, case, c) if route in TRANSFORMS else edge_analysis(eng, lib, route, case, nb, c)
    # ---- the shard on its own: ld = 203
    xs = dev(case["state"])
    base = padded_run(call, xs, n, 0, k)
    pp, fro = per_point_errors(base.cpu().numpy(), ref)
    print("\n[large grid] %s k %d at ld %d: rel. Frobenius %.3e, worst grid point %.3e"
          % (EDGE_ENTRY[route][0], k, ld, fro, pp.max()))
    assert fro <= TOL64 and pp.max() <= TOL64
    # ---- the state at the largest leading dimension, the shard in its last columns
    xb = big[:k * ld].view(1, k, ld)
    xb[:, :, ld - n:] = xs
    assert torch.equal(padded_run(call, xb, ld, ld - n, k), base)
    # ---- the output at the largest leading dimension, written into its last columns
    ob = big[:k * ld].view(1, k, ld)
    ob[:, :, ld - n - PAD:] = -7.0
    call(xs, n, 0, n, ob, ld, ld - n)
    assert torch.equal(ob[:, :, ld - n:], base)
    assert bool((ob[:, :, ld - n - PAD:ld - n] == -7.0).all())

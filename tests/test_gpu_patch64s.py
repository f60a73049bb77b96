"""The streamed float64 analysis of dense local networks under a tile map (csrc/letkf_patch64s.hip,
mia_letkf_analysis_patch_stream_f64, LetkfEngine.analysis(method="patch64s")): letkf_stream64_kernel's analysis with the sixteen
points of a tile taken from a map -- 4 x 4 patches of a 2-D mesh, whose unions fit one pass where sixteen consecutive points (a
16 x 1 strip) run in parts.  Contract: Xa and flags are bit-identical to method="stream64" on the same lists under ANY map, any
union_blocks, any shard and any number of state rows, because slot = rank of the observation index and every sum over the union
is one ascending chain; in addition relative Frobenius error AND the worst single grid point <= 1e-10 against the float64 oracle
(DESIGN 8).

The fixtures are tests/test_gpu_patch64w.py's: an 18 x 18 mesh with an observation at every point (324 points; 25 patches of
4 x 4, the ones at the right and lower edge with dead slots), inflation 1.1, its SHAPES and its seeds (mesh_case(..., seed = 60 +
k): cases that decline nothing, asserted again here).  The observations and the first state row are that file's; the second and
third state row are drawn from a generator of their own, so that the observation space does not change with m.  List lengths
and unions are counted on the CPU from the lists first, so that a changed fixture cannot turn a test into something else.

Run against a build without this route every test fails: LetkfEngine.analysis has no method "patch64s"."""
import warnings

import numpy as np
import pytest
import torch

from oracle import letkf_oracle as O
from test_gpu_patch64w import CAP, G, INF, NX, NY, SHAPES, random_map, unions_of
from test_gpu_stream64 import expected_degrees64, f32_first, largest_union, mesh_case, strong_cluster
from torch_assimilate_amd._cabi import MiaError
from torch_assimilate_amd.engine import NeighbourLists

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
KERNEL = "letkf_patch64s_kernel"
PARENT = "letkf_stream64_kernel"
M = 3                                               # state rows of a case; m = 1 takes the first


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


def check(got, ref, what):
    from oracle_pool import per_point_errors
    pp, fro = per_point_errors(got, ref)
    print("\n[patch64s] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= TOL64, what
    assert pp.max() <= TOL64, what


def run64(eng, case, nb, method, m=M, **kw):
    """engine.analysis in float64 on the first m state rows with a caller-owned decline counter: (Xa, flags, declined, kernel)"""
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xa, fl = eng.analysis(dev(case["state"][:m]), dev(case["yb"]), dev(case["d"]), nb, INF, return_flags=True, method=method,
                          retry=retry, **kw)
    torch.cuda.synchronize()
    return xa, fl, int(retry.item()), last_kernel()


@pytest.fixture(scope="module")
def shapes(eng):
    """k -> case (three state rows), lists and method="stream64"'s Xa and flags: computed once, shared, never written to"""
    memo = {}

    def get(k):
        if k not in memo:
            c, p_max, _, strip, _ = SHAPES[k]
            case = mesh_case(NX, NY, k, 1, seed=60 + k)
            more = np.random.RandomState(760 + k).normal(size=(M - 1, k, G)) + 3.0
            case = dict(case, state=np.concatenate([case["state"], more], axis=0))
            nb = eng.localize(case["grid"], case["obs"], [c])
            assert nb.p_max == p_max and p_max > k and largest_union(nb) == strip
            assert strip > 16 * min((p_max + 31) >> 4, 16)          # the strips do not fit the slots of a launch without a map
            xs, fs, declined, kern = run64(eng, case, nb, "stream64")
            assert PARENT in kern and declined == 0
            assert int((fs.cpu().numpy() & 0xff).max()) == 0        # nothing declined: the Jacobi kernel cannot supply the parity
            memo[k] = dict(case=case, nb=nb, c=c, xs=xs, fs=fs)
        return memo[k]
    return get


def same_as_stream(s, xa, fl, declined, kern, k, what, m=M):
    assert kern == "%s<%d>" % (KERNEL, SHAPES[k][4]), kern
    assert declined == 0, what
    assert torch.equal(fl, s["fs"]), what
    assert tuple(xa.shape) == (m, k, G) and torch.equal(xa, s["xs"][:m]), what


# ---- 1. bit-equality and parity, per shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sorted(SHAPES))
def test_mesh_patches_equal_the_streamed_route_bit_for_bit(mia, eng, shapes, k):
    s = shapes(k)
    tiles = mia.mesh_tiles((NY, NX))
    assert tiles.shape == (25, 16) and int((tiles < 0).sum()) == 25 * 16 - G
    union = SHAPES[k][2]
    assert max(unions_of(s["nb"], tiles)) == union <= 256
    for m in (1, M):
        xa, fl, declined, kern = run64(eng, s["case"], s["nb"], "patch64s", m=m, tile_points=tiles)
        same_as_stream(s, xa, fl, declined, kern, k, "4 x 4 patches, m %d" % m, m)
    flh = fl.cpu().numpy()
    assert int((flh & 0xff).max()) == 0
    assert np.array_equal((flh >> 8) & 0xff, expected_degrees64(s["case"]["yb"], s["nb"], INF))
    ent = s["nb"].tile_census[id(tiles)]
    assert ent[0] is tiles and ent[2] == union                # the census counted what the CPU counts, and it is kept
    assert eng.patch64s_fits(s["nb"], tiles, k) and s["nb"].tile_census[id(tiles)] is ent        # (no second census for the same map)
    if k in (20, 80, 128):
        ref = O.letkf_analysis(s["case"]["state"], s["case"]["grid"], s["case"]["obs"], s["case"]["yb"], s["case"]["d"], s["c"], INF)[0]
        check(xa.cpu().numpy(), ref, "k %d c %g p_max %d, 4 x 4 patches, union %d (%s)" % (k, s["c"], SHAPES[k][1], union, kern))


# ---- 2. any partition is a map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 80])
def test_a_random_partition_with_holes(eng, shapes, k):
    s = shapes(k)
    tiles = random_map(7 + k)
    t = tiles.numpy()
    assert (t[0] >= 0).sum() == 1 and t[0, 0] < 0 and (t[1] >= 0).sum() == 0      # one live slot that is not slot 0; an empty tile
    assert any(row[0] < 0 <= row.max() for row in t[2:]) and any((np.diff((row >= 0).astype(int)) > 0).any() for row in t[2:])
    for m in (1, M):
        same_as_stream(s, *run64(eng, s["case"], s["nb"], "patch64s", m=m, tile_points=tiles), k, "random map, m %d" % m, m)
    # ... also with the smallest slot tables that hold a single list (scattered points: every tile runs in parts)
    ub = (SHAPES[k][1] + 15) // 16
    assert 16 * ub < max(unions_of(s["nb"], tiles))
    for m in (1, M):
        same_as_stream(s, *run64(eng, s["case"], s["nb"], "patch64s", m=m, tile_points=tiles, union_blocks=ub), k,
                       "random map in parts, m %d" % m, m)


@pytest.mark.parametrize("k", [8, 40, 128])
def test_the_smallest_image_runs_patches_in_parts(mia, eng, shapes, k):
    s = shapes(k)
    ub = (SHAPES[k][1] + 15) // 16
    assert 16 * ub < SHAPES[k][2]                             # the union of a patch does not fit, a single list does
    same_as_stream(s, *run64(eng, s["case"], s["nb"], "patch64s", tile_points=mia.mesh_tiles((NY, NX)), union_blocks=ub), k,
                   "union_blocks %d" % ub)


# ---- 3. a shard with an output offset ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 80])
def test_a_shard_with_out_offset_equals_the_full_run(mia, eng, shapes, k):
    s = shapes(k)
    g0, g1 = 37, 250
    nbp = eng.localize(s["case"]["grid"], s["case"]["obs"], [s["c"]], g0=g0, g1=g1)
    assert nbp.p_max == SHAPES[k][1]
    tiles = mia.mesh_tiles((NY, NX), g0, g1)
    for m in (1, M):
        out = torch.full((m, k, g1 - g0 + 9), -7.0, dtype=torch.float64, device=DEV)
        retry = torch.zeros(1, dtype=torch.int32, device=DEV)
        res, fl = eng.analysis(dev(s["case"]["state"][:m]), dev(s["case"]["yb"]), dev(s["case"]["d"]), nbp, INF, out=out,
                               out_offset=5, method="patch64s", tile_points=tiles, retry=retry, return_flags=True)
        torch.cuda.synchronize()
        assert res is out and last_kernel() == "%s<%d>" % (KERNEL, SHAPES[k][4]) and int(retry.item()) == 0
        assert torch.equal(out[:, :, 5:5 + g1 - g0], s["xs"][:m, :, g0:g1]) and torch.equal(fl, s["fs"][g0:g1])
        assert bool((out[:, :, :5] == -7.0).all()) and bool((out[:, :, 5 + g1 - g0:] == -7.0).all())


# ---- 4. a NaN record ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 80])
def test_a_nan_record_stays_with_the_points_that_list_it(mia, eng, shapes, k):
    s = shapes(k)
    nb, j = s["nb"], 151
    bad = dict(s["case"], yb=s["case"]["yb"].copy())
    bad["yb"][3, j] = np.nan
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G
    xs, fs, ds, kern = run64(eng, bad, nb, "stream64")
    assert PARENT in kern
    keep = torch.as_tensor(~uses, device=DEV)
    for tiles in (mia.mesh_tiles((NY, NX)), random_map(3)):
        xa, fl, declined, kern = run64(eng, bad, nb, "patch64s", tile_points=tiles)
        assert kern == "%s<%d>" % (KERNEL, SHAPES[k][4]) and declined == ds
        assert np.array_equal((fl.cpu().numpy() & 4) != 0, uses)
        assert torch.equal(fl, fs)
        assert torch.equal(xa[:, :, keep], s["xs"][:, :, keep])          # the clean run's bits: the tile was done slot by slot
        assert torch.equal(torch.isnan(xa), torch.isnan(xs))
        assert torch.equal(torch.nan_to_num(xa, nan=0.0), torch.nan_to_num(xs, nan=0.0))


# ---- 5. decline and redo under a map ---------------------------------------------------------------------------------------------------
def test_a_strong_cluster_is_declined_and_redone_at_80_members(mia, eng, shapes):
    s = shapes(80)
    nb = s["nb"]
    strong, want = strong_cluster(s["case"], nb, INF)
    n_decl = int(want.sum())
    assert 0 < n_decl < G                          # (the CPU restatement first: the cluster's points and no others)
    assert np.array_equal(want, expected_degrees64(strong["yb"], nb, INF) > CAP)
    out = torch.full((M, 80, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    X, Yb, d = dev(strong["state"]), dev(strong["yb"]), dev(strong["d"])    # (alive until the deferred redo has run: it holds addresses)
    res = eng.analysis(X, Yb, d, nb, INF, out=out, flags=fl, retry=retry, defer_retry=True, method="patch64s",
                       tile_points=mia.mesh_tiles((NY, NX)))
    torch.cuda.synchronize()
    assert res[0] is out and last_kernel() == KERNEL + "<5>"
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want) and int(retry.item()) == n_decl
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[:, :, sel] == -7.0).all()) and not bool((out[:, :, ~sel] == -7.0).any())     # declined points are left untouched
    before = out.clone()
    assert res[-1]() == n_decl                                                                    # the counter, then the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & 8).max()) == 0 and torch.equal(out[:, :, ~sel], before[:, :, ~sel])
    ref = O.letkf_analysis(strong["state"], strong["grid"], strong["obs"], strong["yb"], strong["d"], s["c"], INF)[0]
    check(out.cpu().numpy(), ref, "strong cluster under a map, %d points redone" % n_decl)


def test_a_declined_point_raises_at_128_members_after_the_others_are_written(mia, eng, shapes):
    """The redo is the Jacobi kernel's, which cannot hold 128 members: MiaError, data-dependent, AFTER every other point has been
    written -- the same raise as method="stream64"'s."""
    s = shapes(128)
    nb = s["nb"]
    strong, want = strong_cluster(s["case"], nb, INF)
    assert 0 < int(want.sum()) < G
    out = torch.full((1, 128, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    X, Yb, d = dev(strong["state"][:1]), dev(strong["yb"]), dev(strong["d"])
    res = eng.analysis(X, Yb, d, nb, INF, out=out, flags=fl, defer_retry=True, method="patch64s",
                       tile_points=mia.mesh_tiles((NY, NX)))
    torch.cuda.synchronize()
    assert last_kernel() == KERNEL + "<8>"
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    with pytest.raises(MiaError, match="status -3"):
        res[-1]()
    torch.cuda.synchronize()
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[:, :, sel] == -7.0).all())
    ref = O.letkf_analysis(strong["state"][:1], strong["grid"], strong["obs"], strong["yb"], strong["d"], s["c"], INF)[0]
    check(out.cpu().numpy()[:, :, ~want], ref[:, :, ~want], "k 128 under a map: the %d points that were not declined" % int((~want).sum()))


# ---- 6. overflow ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [40, 80])
def test_a_list_longer_than_the_image_overflows_for_that_point_only(mia, eng, shapes, k):
    s = shapes(k)
    nb, tiles = s["nb"], mia.mesh_tiles((NY, NX))
    cnt = nb.cnt.cpu().numpy()
    # the image one block short of the longest list
    ub = (SHAPES[k][1] + 15) // 16 - 1
    over = cnt > 16 * ub
    assert 0 < over.sum() < G
    xa, fl, declined, kern = run64(eng, s["case"], nb, "patch64s", tile_points=tiles, union_blocks=ub)
    od = torch.as_tensor(over, device=DEV)
    assert kern == "%s<%d>" % (KERNEL, SHAPES[k][4]) and declined == 0 and np.array_equal(fl.cpu().numpy() == 1, over)
    assert bool(torch.isnan(xa[:, :, od]).all())
    assert torch.equal(xa[:, :, ~od], s["xs"][:, :, ~od]) and torch.equal(fl[~od], s["fs"][~od])
    # a bound p_max that the interior lists exceed: the same lists otherwise
    short = NeighbourLists(nb.cnt, nb.idx, nb.w, nb.p_cap, SHAPES[k][1] - 4, nb.g0, nb.g1)
    over = cnt > SHAPES[k][1] - 4
    assert 0 < over.sum() < G and short.p_max > k
    xa, fl, declined, kern = run64(eng, s["case"], short, "patch64s", tile_points=tiles)
    od = torch.as_tensor(over, device=DEV)
    assert KERNEL in kern and np.array_equal(fl.cpu().numpy() == 1, over) and bool(torch.isnan(xa[:, :, od]).all())
    assert torch.equal(xa[:, :, ~od], s["xs"][:, :, ~od]) and torch.equal(fl[~od], s["fs"][~od])


# ---- 7. invalid maps ----------------------------------------------------------------------------------------------------------------
def test_invalid_maps_raise_before_any_launch(mia, eng, shapes):
    s = shapes(20)
    good = mia.mesh_tiles((NY, NX))
    twice, missing, beyond, below = good.clone(), good.clone(), good.clone(), good.clone()
    twice[3, 2] = twice[5, 1]
    missing[7, 0] = -1
    beyond[2, 7] = G
    below[2, 7] = -2
    X, Yb, d = dev(s["case"]["state"]), dev(s["case"]["yb"]), dev(s["case"]["d"])
    out = torch.full((M, 20, G), -7.0, dtype=torch.float64, device=DEV)
    f32_first(eng)
    for tiles, word in ((twice, "more than once"), (missing, "does not occur"), (beyond, "outside"), (below, "outside"),
                        (good[:0], "does not occur")):
        for ub in (None, 4):                           # (a given union_blocks leaves the count, not the validation)
            with pytest.raises(ValueError, match=word):
                eng.analysis(X, Yb, d, s["nb"], INF, out=out, method="patch64s", tile_points=tiles, union_blocks=ub)
    for tiles in (good.to(torch.int64), good.reshape(-1), good[:, :8]):
        with pytest.raises(ValueError, match="tile_points"):
            eng.analysis(X, Yb, d, s["nb"], INF, out=out, method="patch64s", tile_points=tiles)
    for ub in (0, 17):
        with pytest.raises(ValueError, match="union_blocks"):
            eng.analysis(X, Yb, d, s["nb"], INF, out=out, method="patch64s", tile_points=good, union_blocks=ub)
    # the route is named: it raises without a map, outside float64, the plain core, with weights and outside the cover
    with pytest.raises(ValueError, match="tile_points"):
        eng.analysis(X, Yb, d, s["nb"], INF, out=out, method="patch64s")
    with pytest.raises(ValueError):
        eng.analysis(X.float(), Yb.float(), d.float(), s["nb"], INF, method="patch64s", tile_points=good)
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, s["nb"], INF, out=out, method="patch64s", tile_points=good, return_weights=True)
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, s["nb"], INF, out=out, method="patch64s", tile_points=good, rbf_gamma=0.5)
    nbs = eng.localize(s["case"]["grid"], s["case"]["obs"], [0.9])
    assert nbs.p_max <= 20
    with pytest.raises(MiaError, match="status -3"):
        eng.analysis(X, Yb, d, nbs, INF, out=out, method="patch64s", tile_points=good)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and KERNEL not in last_kernel()
    # "auto" with a map never takes the route; the named stream64 does not look at the map
    xa = eng.analysis(X, Yb, d, s["nb"], INF, tile_points=good)
    torch.cuda.synchronize()
    assert KERNEL not in last_kernel()
    assert torch.equal(eng.analysis(X, Yb, d, s["nb"], INF, method="stream64", tile_points=good), s["xs"])
    assert PARENT in last_kernel()


# ---- 8. the class ------------------------------------------------------------------------------------------------------------------
def class_analysis(mia, eng, case, c, m, **kw):
    f32_first(eng)          # (so that the reported kernel name is known to be fresh: the Jacobi kernel never reports one)
    f = mia.LETKF(mia.GaspariCohn(c, mia.EuclideanMetric()), INF, **kw)
    xa = f.analyse_arrays(case["state"][:m], case["yb"], case["d"], grid_coords=case["grid"], obs_coords=case["obs"])
    torch.cuda.synchronize()
    return xa, last_kernel()


@pytest.mark.parametrize("k,m", [(80, 1), (80, M), (128, 1)])
def test_the_class_takes_the_map_exactly_where_the_rule_says(mia, eng, shapes, k, m):
    s = shapes(k)
    p_max, kt = SHAPES[k][1], SHAPES[k][4]
    plain, plain_kernel = class_analysis(mia, eng, s["case"], s["c"], m)
    assert eng._stream64_auto(m, k, p_max) and plain_kernel == "%s<%d>" % (PARENT, kt)     # what "auto" runs today
    assert plain.dtype == torch.float64 and torch.equal(plain, s["xs"][:m])
    xa, kern = class_analysis(mia, eng, s["case"], s["c"], m, mesh_shape=(NY, NX))
    if eng._patch64s_auto(m, k, p_max):
        assert kern == "%s<%d>" % (KERNEL, kt), kern
    else:
        assert KERNEL not in kern and kern == plain_kernel
    assert xa.dtype == torch.float64 and torch.equal(xa, plain)
    with pytest.warns(RuntimeWarning, match="mesh_shape"):
        wrong, kern = class_analysis(mia, eng, s["case"], s["c"], m, mesh_shape=(NY, NX + 1))
    assert kern == plain_kernel and torch.equal(wrong, plain)


def test_the_class_in_float32_never_looks_at_mesh_shape(mia, eng, shapes):
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*mesh_shape.*")
        case = shapes(20)["case"]
        xa, kern = class_analysis(mia, eng, case, 1.5, 1, dtype=torch.float32, mesh_shape=(NY, NX + 1))
        assert xa.dtype == torch.float32 and KERNEL not in kern


# ---- 9. more than 65 536 tiles -----------------------------------------------------------------------------------------------------
def test_a_map_of_more_than_65536_tiles():
    """G_LARGE points of the dense 1-D network with the strips of sixteen consecutive points in REVERSED tile order as the map
    (tests/large_grid_cases.py): tile indices cross 65 536 and the second row of the block grid, into an output of NaN and flag
    words of 0xffffffff.  The same bits as method="stream64", and every point within TOL64 of the oracle."""
    import large_grid_cases as L
    import torch_assimilate_amd as mia_
    from oracle_pool import per_point_errors
    eng = mia_.LetkfEngine(DEV)
    GL = L.G_LARGE
    case = L.large_case("dense", L.K, L.M)
    try:
        nb = eng.localize(case["grid_x"], case["obs_x"], [case["c"]])
        assert nb.p_max == 15 > L.K
        X, Yb, d = dev(case["state"]), dev(case["yb"]), dev(case["d"])
        tiles = torch.from_numpy(L.reversed_strips(GL))
        assert tiles.shape[0] > 65536 + 1000
        res = {}
        for method, kw in (("stream64", {}), ("patch64s", dict(tile_points=tiles))):
            retry = torch.zeros(1, dtype=torch.int32, device=DEV)
            out = torch.full((L.M, L.K, GL), float("nan"), dtype=torch.float64, device=DEV)
            fl = torch.full((GL,), -1, dtype=torch.int32, device=DEV)
            assert eng.analysis(X, Yb, d, nb, L.INF, method=method, retry=retry, out=out, flags=fl, **kw) is out
            torch.cuda.synchronize()
            assert last_kernel() == (PARENT if method == "stream64" else KERNEL) + "<1>"
            assert int(retry.item()) == 0 and int((fl & 0xff).max().item()) == 0
            res[method] = (out, fl)
        assert torch.equal(res["patch64s"][0], res["stream64"][0]) and torch.equal(res["patch64s"][1], res["stream64"][1])
        pp, fro = per_point_errors(res["patch64s"][0].cpu().numpy(), L.large_analysis("dense", "letkf", L.K, L.M))
        print("\n[patch64s] %d points under reversed strips: rel. Frobenius %.3e, worst grid point %.3e" % (GL, fro, pp.max()))
        assert fro <= TOL64 and pp.max() <= TOL64
    finally:
        for fn in (L.large_case, L.large_weights, L.large_analysis):
            fn.cache_clear()
        torch.cuda.empty_cache()

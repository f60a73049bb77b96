"""The dense float64 route under a tile map (csrc/letkf_patch64.hip, mia_letkf_analysis_patch_f64, method="patch64"): the
sixteen points of a tile come from a map (4 x 4 patches of a 2-D mesh) and the record image is sized for the largest union a
tile has.  Contract as tests/test_gpu_dense64.py: relative Frobenius error AND the worst single grid point <= 1e-10 against the
float64 oracle; in addition output and flags are bit-identical to method="dense64" on the same lists, because a point's
observations are summed in ascending index order whatever else shares its tile.

13 x 11 meshes (neither side a multiple of 4) with an observation at every point; the radius per ensemble size is such that
an interior list exceeds k -- counted on the CPU from the oracle's localisation: 9 / 25 / 45 observations, unions of a
4 x 4 patch up to 36 / 64 / 96."""
import warnings

import numpy as np
import pytest
import torch

from oracle import letkf_oracle as O
from test_gpu_dense64 import CAP, expected_degrees64, mesh_case
from torch_assimilate_amd._cabi import MiaError

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
KERNEL = "letkf_patch64_kernel"
NY, NX, G, INF = 13, 11, 143, 1.1
# k -> (radius, interior list length, largest union of a 4 x 4 / 2 x 8 / 8 x 2 patch, KT)
SHAPES = {8: (0.9, 9, (36, 36, 36), 1), 20: (1.5, 25, (64, 60, 60), 2), 40: (1.95, 45, (96, 86, 86), 3)}
PATCHES = ((4, 4), (2, 8), (8, 2))


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
    print("\n[patch64] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, pp.max(), int(pp.argmax())))
    assert fro <= TOL64, what
    assert pp.max() <= TOL64, what


def run64(eng, case, nb, method, **kw):
    """(Xa, flags, declined, kernel name) of engine.analysis in float64 with a caller-owned decline counter"""
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    xa, fl = eng.analysis(dev(case["state"]), dev(case["yb"]), dev(case["d"]), nb, INF, return_flags=True, method=method,
                          retry=retry, **kw)
    torch.cuda.synchronize()
    return xa, fl, int(retry.item()), last_kernel()


@pytest.fixture(scope="module")
def shapes(eng):
    """(k, m) -> case, lists, oracle analysis and the dense route's output and flags: computed once, shared, never written to"""
    memo = {}

    def get(k, m):
        if (k, m) not in memo:
            c, plen, _, _ = SHAPES[k]
            case = mesh_case(NX, NY, k, 1, seed=50 + k + m, m=m)
            nb = eng.localize(case["grid"], case["obs"], [c])
            assert nb.p_max == plen and plen > k
            ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], c, INF)[0]
            xd, fd, declined, kern = run64(eng, case, nb, "dense64")
            assert "letkf_dense64_kernel" in kern and declined == 0
            memo[(k, m)] = dict(case=case, nb=nb, ref=ref, c=c, xd=xd, fd=fd)
        return memo[(k, m)]
    return get


def unions_of(nb, tiles):
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    return [len(set(np.concatenate([idx[p, :cnt[p]] for p in row if p >= 0] + [np.zeros(0, np.int32)]))) for row in tiles.numpy()]


def same_as_dense(s, xa, fl, declined, kern, k, what):
    assert "%s<%d>" % (KERNEL, SHAPES[k][3]) in kern, kern
    assert declined == 0                               # (so that the Jacobi kernel cannot supply the parity)
    assert torch.equal(fl, s["fd"]), what
    assert torch.equal(xa, s["xd"]), what


# ---- 1. mesh patches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k", [8, 20, 40])
def test_mesh_patches_equal_the_dense_route_bit_for_bit(mia, eng, shapes, k, m):
    s = shapes(k, m)
    for patch, union in zip(PATCHES, SHAPES[k][2]):
        tiles = mia.mesh_tiles((NY, NX), patch=patch)
        assert max(unions_of(s["nb"], tiles)) == union
        xa, fl, declined, kern = run64(eng, s["case"], s["nb"], "patch64", tile_points=tiles)
        same_as_dense(s, xa, fl, declined, kern, k, "patch %r" % (patch,))
        ent = s["nb"].tile_census[id(tiles)]
        assert ent[0] is tiles and ent[2] == union          # the census counted what the CPU counts, and it is kept
        if patch == (4, 4):
            check(xa.cpu().numpy(), s["ref"], "k %d m %d, 4 x 4 patches, union %d" % (k, m, union))
    again = run64(eng, s["case"], s["nb"], "patch64", tile_points=tiles)[0]
    assert torch.equal(again, s["xd"]) and s["nb"].tile_census[id(tiles)] is ent        # (no second census for the same map)


# ---- 2. any partition is a map ---------------------------------------------------------------------------------------------------
def random_map(seed):
    """143 points over 14 tiles: tile 0 has ONE live slot (slot 5), tile 1 none, the others random places -- live slots are no
    prefix"""
    rnd = np.random.RandomState(seed)
    perm = rnd.permutation(G)
    t = -np.ones((14, 16), dtype=np.int32)
    t[0, 5] = perm[0]
    places = rnd.permutation(12 * 16)[:G - 1]
    t[2:].reshape(-1)[places] = perm[1:]
    return torch.as_tensor(t)


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k", [8, 20, 40])
def test_a_random_partition_with_holes(eng, shapes, k, m):
    s = shapes(k, m)
    tiles = random_map(7 + k)
    t = tiles.numpy()
    assert (t[0] >= 0).sum() == 1 and (t[1] >= 0).sum() == 0
    assert any(row[0] < 0 <= row.max() for row in t) and any((np.diff((row >= 0).astype(int)) > 0).any() for row in t[2:])
    xa, fl, declined, kern = run64(eng, s["case"], s["nb"], "patch64", tile_points=tiles)
    same_as_dense(s, xa, fl, declined, kern, k, "random map")
    # ... also when its tiles run in parts (scattered points: unions far above a patch's)
    xa, fl, declined, kern = run64(eng, s["case"], s["nb"], "patch64", tile_points=tiles, union_blocks=(SHAPES[k][1] + 15) // 16)
    same_as_dense(s, xa, fl, declined, kern, k, "random map in parts")


# ---- 3. a shard with an output offset ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k", [8, 20, 40])
def test_a_shard_with_out_offset_equals_the_full_run(mia, eng, shapes, k, m):
    s = shapes(k, m)
    g0, g1 = 37, 120
    nbp = eng.localize(s["case"]["grid"], s["case"]["obs"], [s["c"]], g0=g0, g1=g1)
    assert nbp.p_max == SHAPES[k][1]
    tiles = mia.mesh_tiles((NY, NX), g0, g1)
    out = torch.full((m, k, g1 - g0 + 9), -7.0, dtype=torch.float64, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = eng.analysis(dev(s["case"]["state"]), dev(s["case"]["yb"]), dev(s["case"]["d"]), nbp, INF, out=out, out_offset=5,
                       method="patch64", tile_points=tiles, retry=retry)
    torch.cuda.synchronize()
    assert res is out and KERNEL in last_kernel() and int(retry.item()) == 0
    assert torch.equal(out[:, :, 5:5 + g1 - g0], s["xd"][:, :, g0:g1])
    assert bool((out[:, :, :5] == -7.0).all()) and bool((out[:, :, 5 + g1 - g0:] == -7.0).all())


# ---- 4. an image smaller than the unions: halves and quarters ---------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k", [8, 20, 40])
def test_the_smallest_image_runs_tiles_in_parts(mia, eng, shapes, k, m):
    s = shapes(k, m)
    tiles = mia.mesh_tiles((NY, NX))
    ub = (SHAPES[k][1] + 15) // 16
    assert 16 * ub < SHAPES[k][2][0]                   # the union of a patch does not fit, a single list does
    xa, fl, declined, kern = run64(eng, s["case"], s["nb"], "patch64", tile_points=tiles, union_blocks=ub)
    same_as_dense(s, xa, fl, declined, kern, k, "union_blocks %d" % ub)


# ---- 5. a NaN record ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(8, 1), (20, 3), (40, 1)])
def test_a_nan_record_stays_with_the_points_that_use_it(mia, eng, shapes, k, m):
    s = shapes(k, m)
    nb, j = s["nb"], 60
    bad = dict(s["case"], yb=s["case"]["yb"].copy())
    bad["yb"][1, j] = np.nan
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G
    xd, fd, dd, _ = run64(eng, bad, nb, "dense64")
    for tiles in (mia.mesh_tiles((NY, NX)), random_map(3)):
        xa, fl, declined, kern = run64(eng, bad, nb, "patch64", tile_points=tiles)
        assert KERNEL in kern and declined == dd
        assert np.array_equal((fl.cpu().numpy() & 4) != 0, uses)
        assert torch.equal(fl, fd)
        keep = torch.as_tensor(~uses, device=DEV)
        assert torch.equal(xa[:, :, keep], s["xd"][:, :, keep])          # the clean run's bits
        assert torch.equal(torch.isnan(xa), torch.isnan(xd))


# ---- 6. points above the degree cap are declined and redone -------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(8, 1), (40, 3)])
def test_strong_observations_decline_exactly_the_points_above_the_cap(mia, eng, shapes, k, m):
    """Observations 70 .. 72 with a hundredth of the variance (yb, d x 10): the CPU's degree formula puts a few of the 143 points
    above the cap (1 at k 8, 5 at k 40 with these seeds)"""
    s = shapes(k, m)
    nb = s["nb"]
    case = dict(s["case"], yb=s["case"]["yb"].copy(), d=s["case"]["d"].copy())
    case["yb"][:, 70:73] *= 10.0
    case["d"][70:73] *= 10.0
    want = expected_degrees64(case["yb"], nb, INF) > CAP
    assert 0 < int(want.sum()) < G
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], s["c"], INF)[0]
    xd, fd, dd, _ = run64(eng, case, nb, "dense64")
    assert dd == int(want.sum())
    out = torch.full((m, k, G), -7.0, dtype=torch.float64, device=DEV)
    fl = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    X, Yb, d = dev(case["state"]), dev(case["yb"]), dev(case["d"])      # (alive until the deferred redo has run: it holds addresses)
    res = eng.analysis(X, Yb, d, nb, INF, out=out, flags=fl, retry=retry, defer_retry=True, method="patch64",
                       tile_points=mia.mesh_tiles((NY, NX)))
    torch.cuda.synchronize()
    assert KERNEL in last_kernel()
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want) and int(retry.item()) == int(want.sum())
    wd = torch.as_tensor(want, device=DEV)
    assert bool((out[:, :, wd] == -7.0).all())                           # declined points are left untouched
    assert torch.equal(out[:, :, ~wd], xd[:, :, ~wd])                    # the others carry the dense route's bits
    assert res[-1]() == int(want.sum())                                  # the deferred redo, from the natural-order lists
    torch.cuda.synchronize()
    # the redo (the Jacobi kernel, whose bits are its own) has written the declined points and nothing else
    assert torch.equal(out[:, :, ~wd], xd[:, :, ~wd]) and torch.equal(fl[~wd], fd[~wd])
    assert int((fl.cpu().numpy() & 8).max()) == 0 and bool(torch.isfinite(out).all())
    print("\n[patch64] redone points against the dense route's redo: max abs difference %.3e" % float((out - xd).abs().max()))
    check(out.cpu().numpy(), ref, "k %d: %d points redone" % (k, int(want.sum())))


# ---- 7. a list longer than the image --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(20, 1), (40, 3)])
def test_a_list_longer_than_the_image_overflows_for_that_point_only(mia, eng, shapes, k, m):
    """An image one block short of the longest list (16 of 25, 32 of 45 slots): interior points overflow, the points at the
    mesh's edge, whose lists are shorter, are analysed"""
    s = shapes(k, m)
    ub = (SHAPES[k][1] + 15) // 16 - 1
    over = s["nb"].cnt.cpu().numpy() > 16 * ub
    assert 0 < over.sum() < G
    xa, fl, declined, kern = run64(eng, s["case"], s["nb"], "patch64", tile_points=mia.mesh_tiles((NY, NX)), union_blocks=ub)
    assert KERNEL in kern and declined == 0
    assert np.array_equal(fl.cpu().numpy() == 1, over)
    od = torch.as_tensor(over, device=DEV)
    assert bool(torch.isnan(xa[:, :, od]).all())
    assert torch.equal(xa[:, :, ~od], s["xd"][:, :, ~od]) and torch.equal(fl[~od], s["fd"][~od])


# ---- 8. invalid maps ----------------------------------------------------------------------------------------------------------------
def test_invalid_maps_raise_before_the_analysis(mia, eng, shapes):
    s = shapes(20, 1)
    good = mia.mesh_tiles((NY, NX))
    twice, missing, beyond, below = good.clone(), good.clone(), good.clone(), good.clone()
    twice[3, 2] = twice[5, 1]
    missing[4, 0] = -1
    beyond[2, 7] = G
    below[2, 7] = -2
    X, Yb, d = dev(s["case"]["state"]), dev(s["case"]["yb"]), dev(s["case"]["d"])
    out = torch.full((1, 20, G), -7.0, dtype=torch.float64, device=DEV)
    for tiles, word in ((twice, "more than once"), (missing, "does not occur"), (beyond, "outside"), (below, "outside"),
                        (good[:0], "does not occur")):
        for ub in (None, 4):                           # (a given union_blocks leaves the count, not the validation)
            with pytest.raises(ValueError, match=word):
                eng.analysis(X, Yb, d, s["nb"], INF, out=out, method="patch64", tile_points=tiles, union_blocks=ub)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    for tiles in (good.to(torch.int64), good.reshape(-1), good[:, :8]):
        with pytest.raises(ValueError):
            eng.analysis(X, Yb, d, s["nb"], INF, method="patch64", tile_points=tiles)
    for ub in (0, 17):
        with pytest.raises(ValueError):
            eng.analysis(X, Yb, d, s["nb"], INF, method="patch64", tile_points=good, union_blocks=ub)
    # the route is named: it raises outside float64, the plain core, without a map, with weights and outside the cover
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, s["nb"], INF, method="patch64")
    with pytest.raises(ValueError):
        eng.analysis(X.float(), Yb.float(), d.float(), s["nb"], INF, method="patch64", tile_points=good)
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, s["nb"], INF, method="patch64", tile_points=good, return_weights=True)
    with pytest.raises(ValueError):
        eng.analysis(X, Yb, d, s["nb"], INF, method="patch64", tile_points=good, rbf_gamma=0.5)
    nbs = eng.localize(s["case"]["grid"], s["case"]["obs"], [0.9])
    assert nbs.p_max <= 20
    with pytest.raises(MiaError, match="status -3"):
        eng.analysis(X, Yb, d, nbs, INF, method="patch64", tile_points=good)
    # without a map every call is what it was; with one, method="dense64" and "eig" do not look at it
    assert torch.equal(eng.analysis(X, Yb, d, s["nb"], INF, method="dense64", tile_points=good), s["xd"])
    assert "letkf_dense64_kernel" in last_kernel()


# ---- 9. the drop-in class --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", [(20, 1), (40, 3)])
def test_letkf_with_mesh_shape(mia, eng, shapes, k, m):
    s = shapes(k, m)
    case, c = s["case"], s["c"]
    arrays = (case["state"], case["yb"], case["d"], case["grid"], case["obs"])

    def letkf(**kw):
        return mia.LETKF(mia.GaspariCohn(c, mia.EuclideanMetric()), INF, **kw)
    plain = letkf().analyse_arrays(*arrays)
    plain_kernel = last_kernel()
    f = letkf(mesh_shape=(NY, NX))
    xa = f.analyse_arrays(*arrays)
    assert xa.dtype == torch.float64 and torch.equal(xa, plain)
    if eng._patch64_auto(m, k, SHAPES[k][1]):
        assert "%s<%d>" % (KERNEL, SHAPES[k][3]) in last_kernel(), last_kernel()
    else:
        # method="auto" does not admit this shape (LetkfEngine.PATCH64_AUTO_*): the class stays where it was, and the route
        # is named through the engine with the map the class built
        assert last_kernel() == plain_kernel
        tiles = f._mesh_map(dev(case["state"]), s["nb"])
        assert torch.equal(tiles.cpu(), mia.mesh_tiles((NY, NX)))
        same_as_dense(s, *run64(eng, case, s["nb"], "patch64", tile_points=tiles), k, "LETKF's map")
    assert f._mesh_map(dev(case["state"]), s["nb"]) is f._mesh_map(dev(case["state"]), s["nb"])      # built once per (g0, g1)
    with pytest.warns(RuntimeWarning, match="mesh_shape"):
        wrong = letkf(mesh_shape=(NY, NX + 1)).analyse_arrays(*arrays)
    assert torch.equal(wrong, plain)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*mesh_shape.*")      # float32 never looks at mesh_shape
        assert letkf(dtype=torch.float32, mesh_shape=(NY, NX + 1)).analyse_arrays(*arrays).dtype == torch.float32

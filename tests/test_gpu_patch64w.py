"""The float64 weights of dense local networks under a tile map (csrc/letkf_patch64w.hip, mia_letkf_weights_patch_f64,
LetkfEngine.weights_patch64): letkf_stream64w_kernel's weights with the sixteen points of a tile taken from a map -- 4 x 4
patches of a 2-D mesh, whose unions fit one pass where sixteen consecutive points (a 16 x 1 strip) run in parts.  Contract:
relative Frobenius error AND the worst single grid point <= 1e-10 against the float64 oracle's weights; in addition
W and flags are bit-identical to weights_stream64 on the same lists under ANY map, because slot = rank of the observation index
and every sum over the union is one ascending chain.

An 18 x 18 mesh with an observation at every point (324 points; 25 patches of 4 x 4, the ones at the right and lower edge with
dead slots), inflation 1.1.  The radius per ensemble size is such that an interior list exceeds k; list lengths and unions are
counted on the CPU from the lists first, so that a changed fixture cannot turn a test into something else.

Run against a build without this route every test fails: LetkfEngine has no weights_patch64."""
import math
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_fro
from oracle import letkf_oracle as O
from test_gpu_stream64 import expected_degrees64, f32_first, largest_union, mesh_case, strong_cluster
from torch_assimilate_amd._cabi import MiaError
from torch_assimilate_amd.engine import NeighbourLists

pytestmark = pytest.mark.gpu
TOL64 = 1e-10
DEV = "cuda:0"
KERNEL = "letkf_patch64w_kernel"
PARENT = "letkf_stream64w_kernel"
NY, NX, G, INF = 18, 18, 324, 1.1
CAP = 127
# k -> (radius, p_max, largest union of a 4 x 4 patch, largest union of sixteen consecutive points, KT)
SHAPES = {8: (0.9, 9, 36, 54, 1), 20: (1.5, 25, 64, 92, 2), 40: (1.95, 45, 96, 128, 3), 64: (2.5, 69, 132, 164, 4),
          80: (3.0, 101, 176, 200, 5), 96: (3.0, 101, 176, 200, 6), 112: (3.5, 145, 232, 238, 7), 128: (3.5, 145, 232, 238, 8)}


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
    pp = per_point_w(got, ref)
    fro = rel_fro(got, ref)
    print("\n[patch64w] %s: rel. Frobenius %.3e, worst grid point %.3e (point %d)" % (what, fro, float(pp.max()), int(pp.argmax())))
    assert fro <= TOL64, what
    assert float(pp.max()) <= TOL64, what


def unions_of(nb, tiles):
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    return [len(set(np.concatenate([idx[p, :cnt[p]] for p in row if p >= 0] + [np.zeros(0, np.int32)]))) for row in tiles.numpy()]


def stream(eng, case, nb, **kw):
    """engine.weights_stream64 without a map: (W, flags), the reference for bits"""
    res = eng.weights_stream64(dev(case["yb"]), dev(case["d"]), nb, INF, return_flags=True, **kw)
    assert res is not None
    torch.cuda.synchronize()
    assert PARENT in last_kernel()
    return res[0], res[1]


def patch(eng, case, nb, tiles, **kw):
    """engine.weights_patch64: (W, flags, kernel name); fails when the route refuses"""
    res = eng.weights_patch64(dev(case["yb"]), dev(case["d"]), nb, tiles, INF, return_flags=True, **kw)
    assert res is not None, "weights_patch64 refused the shape"
    torch.cuda.synchronize()
    return res[0], res[1], last_kernel()


@pytest.fixture(scope="module")
def shapes(eng):
    """k -> case, lists and weights_stream64's W and flags: computed once, shared, never written to"""
    memo = {}

    def get(k):
        if k not in memo:
            c, p_max, _, strip, _ = SHAPES[k]
            case = mesh_case(NX, NY, k, 1, seed=60 + k)
            nb = eng.localize(case["grid"], case["obs"], [c])
            assert nb.p_max == p_max and p_max > k and largest_union(nb) == strip
            assert strip > 16 * min((p_max + 31) >> 4, 16)          # the strips do not fit the slots of a launch without a map
            W, fl = stream(eng, case, nb)
            assert int((fl.cpu().numpy() & 0xff).max()) == 0        # nothing declined: the Jacobi kernel cannot supply the parity
            memo[k] = dict(case=case, nb=nb, c=c, W=W, fl=fl)
        return memo[k]
    return get


def same_as_stream(s, W, fl, kern, k, what):
    assert kern == "%s<%d>" % (KERNEL, SHAPES[k][4]), kern
    assert torch.equal(fl, s["fl"]), what
    assert torch.equal(W, s["W"]), what


# ---- 1. bit-equality and parity, per shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sorted(SHAPES))
def test_mesh_patches_equal_the_streamed_route_bit_for_bit(mia, eng, shapes, k):
    s = shapes(k)
    tiles = mia.mesh_tiles((NY, NX))
    assert tiles.shape == (25, 16) and int((tiles < 0).sum()) == 25 * 16 - G
    union = SHAPES[k][2]
    assert max(unions_of(s["nb"], tiles)) == union <= 256
    W, fl, kern = patch(eng, s["case"], s["nb"], tiles)
    same_as_stream(s, W, fl, kern, k, "4 x 4 patches")
    flh = fl.cpu().numpy()
    assert int((flh & 0xff).max()) == 0
    assert np.array_equal((flh >> 8) & 0xff, expected_degrees64(s["case"]["yb"], s["nb"], INF))
    ent = s["nb"].tile_census[id(tiles)]
    assert ent[0] is tiles and ent[2] == union                # the census counted what the CPU counts, and it is kept
    again = patch(eng, s["case"], s["nb"], tiles)[0]
    assert torch.equal(again, s["W"]) and s["nb"].tile_census[id(tiles)] is ent        # (no second census for the same map)
    ref = O.letkf_analysis(s["case"]["state"], s["case"]["grid"], s["case"]["obs"], s["case"]["yb"], s["case"]["d"], s["c"], INF)[1]
    check(W.cpu().numpy(), ref, "k %d c %g p_max %d, 4 x 4 patches, union %d (%s)" % (k, s["c"], SHAPES[k][1], union, kern))


# ---- 2. any partition is a map ---------------------------------------------------------------------------------------------------
def random_map(seed):
    """324 points over 30 tiles: tile 0 has ONE live slot (slot 5), tile 1 none, the others random places -- live slots are no
    prefix"""
    rnd = np.random.RandomState(seed)
    perm = rnd.permutation(G)
    t = -np.ones((30, 16), dtype=np.int32)
    t[0, 5] = perm[0]
    places = rnd.permutation(28 * 16)[:G - 1]
    t[2:].reshape(-1)[places] = perm[1:]
    return torch.as_tensor(t)


@pytest.mark.parametrize("k", [20, 80])
def test_any_partition_is_a_map(mia, eng, shapes, k):
    s = shapes(k)
    for shape in ((2, 8), (8, 2)):
        W, fl, kern = patch(eng, s["case"], s["nb"], mia.mesh_tiles((NY, NX), patch=shape))
        same_as_stream(s, W, fl, kern, k, "patch %r" % (shape,))
    tiles = random_map(7 + k)
    t = tiles.numpy()
    assert (t[0] >= 0).sum() == 1 and t[0, 0] < 0 and (t[1] >= 0).sum() == 0
    assert any(row[0] < 0 <= row.max() for row in t[2:]) and any((np.diff((row >= 0).astype(int)) > 0).any() for row in t[2:])
    W, fl, kern = patch(eng, s["case"], s["nb"], tiles)        # (scattered points: unions above 256 run in parts)
    same_as_stream(s, W, fl, kern, k, "random map")


# ---- 3. shards ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 80])
def test_sub_ranges_and_shards_have_the_full_calls_bits(mia, eng, shapes, k):
    s = shapes(k)
    for g0, g1 in ((0, 150), (37, 290), (0, 163), (163, G)):
        nbp = eng.localize(s["case"]["grid"], s["case"]["obs"], [s["c"]], g0=g0, g1=g1)
        assert nbp.p_max == SHAPES[k][1]
        W, fl, kern = patch(eng, s["case"], nbp, mia.mesh_tiles((NY, NX), g0, g1))
        assert kern.startswith(KERNEL) and W.shape[0] == g1 - g0
        assert torch.equal(W, s["W"][g0:g1]) and torch.equal(fl, s["fl"][g0:g1]), (g0, g1)


# ---- 4. halving under the map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 40, 80, 128])
def test_the_smallest_image_runs_tiles_in_parts(mia, eng, shapes, k):
    s = shapes(k)
    ub = (SHAPES[k][1] + 15) // 16
    assert 16 * ub < SHAPES[k][2]                             # the union of a patch does not fit, a single list does
    W, fl, kern = patch(eng, s["case"], s["nb"], mia.mesh_tiles((NY, NX)), union_blocks=ub)
    same_as_stream(s, W, fl, kern, k, "union_blocks %d" % ub)


def test_unions_above_the_full_image_run_in_halves(mia, eng):
    """k = 128 at radius 4: p_max 185, patch unions up to 264 > 256 slots -- tiles run in halves at the full image"""
    case = mesh_case(NX, NY, 128, 1, seed=188)
    nb = eng.localize(case["grid"], case["obs"], [4.0])
    tiles = mia.mesh_tiles((NY, NX))
    assert nb.p_max == 185 and max(unions_of(nb, tiles)) == 264 > 256
    Ws, fs = stream(eng, case, nb)
    assert int((fs.cpu().numpy() & 0xff).max()) == 0
    W, fl, kern = patch(eng, case, nb, tiles)
    assert kern == KERNEL + "<8>" and nb.tile_census[id(tiles)][2] == 264
    assert torch.equal(W, Ws) and torch.equal(fl, fs)


# ---- 5. points without observations -------------------------------------------------------------------------------------------------
def test_points_without_observations_get_sqrt_inf_identity(mia, eng):
    k, c = 20, 1.5
    case = mesh_case(NX, NY, k, 1, seed=31)
    keep = case["obs"][:, 1] >= 9
    case = dict(case, obs=case["obs"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid"], case["obs"], [c])
    assert nb.p_max == 25 > k
    cnt = nb.cnt.cpu().numpy()
    far = cnt == 0
    tiles = mia.mesh_tiles((NY, NX))
    mixed = [row for row in tiles.numpy() if far[row[row >= 0]].any() and not far[row[row >= 0]].all()]
    assert 0 < far.sum() < G and len(mixed) >= 4              # patches that hold both kinds of points
    Ws, fs = stream(eng, case, nb)
    W, fl, kern = patch(eng, case, nb, tiles)
    assert kern == KERNEL + "<2>" and torch.equal(W, Ws) and torch.equal(fl, fs)
    flh = fl.cpu().numpy()
    eye = (math.sqrt(INF) * torch.eye(k, dtype=torch.float64, device=DEV)).expand(int(far.sum()), k, k)
    assert torch.equal(W[torch.as_tensor(far, device=DEV)], eye)
    assert int(np.abs(flh[far]).max()) == 0 and int(flh[~far].min()) > 0 and int((flh & 0xff).max()) == 0
    ref = O.letkf_analysis(case["state"], case["grid"], case["obs"], case["yb"], case["d"], c, INF)[1]
    check(W.cpu().numpy(), ref, "observations on rows y >= 9 only")


# ---- 6. a NaN record ------------------------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_list_it(mia, eng, shapes):
    s = shapes(20)
    nb, j = s["nb"], 151
    bad = dict(s["case"], yb=s["case"]["yb"].copy())
    bad["yb"][3, j] = np.nan
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G
    Ws, fs = stream(eng, bad, nb)
    keep = torch.as_tensor(~uses, device=DEV)
    for tiles in (mia.mesh_tiles((NY, NX)), random_map(3)):
        W, fl, kern = patch(eng, bad, nb, tiles)
        assert kern.startswith(KERNEL)
        assert np.array_equal((fl.cpu().numpy() & 4) != 0, uses)
        assert torch.equal(fl, fs)
        assert torch.equal(W[keep], s["W"][keep])              # the clean run's bits: the tile was done slot by slot
        assert torch.equal(torch.isnan(W), torch.isnan(Ws))


# ---- 7. decline and redo under a map ---------------------------------------------------------------------------------------------------
def test_a_strong_cluster_is_declined_and_redone_at_80_members(mia, eng, shapes):
    s = shapes(80)
    nb = s["nb"]
    strong, want = strong_cluster(s["case"], nb, INF)
    n_decl = int(want.sum())
    assert 0 < n_decl < G                          # (the CPU restatement first: the cluster's points and no others)
    out = torch.full((G, 80, 80), -7.0, dtype=torch.float64, device=DEV)
    Yb, d = dev(strong["yb"]), dev(strong["d"])    # (alive until the deferred redo has run: it holds addresses)
    W, fl, finish = eng.weights_patch64(Yb, d, nb, mia.mesh_tiles((NY, NX)), INF, out=out, return_flags=True, defer_retry=True)
    torch.cuda.synchronize()
    assert W is out and last_kernel() == KERNEL + "<5>"
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())     # declined blocks are left untouched
    before = out.clone()
    assert finish() == n_decl                                                         # the counter, then the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & 8).max()) == 0 and torch.equal(out[~sel], before[~sel])
    ref = O.letkf_analysis(strong["state"], strong["grid"], strong["obs"], strong["yb"], strong["d"], s["c"], INF)[1]
    check(out.cpu().numpy(), ref, "strong cluster under a map, %d points redone" % n_decl)


def test_a_declined_point_raises_at_128_members_after_the_others_are_written(mia, eng, shapes):
    """The redo is the Jacobi kernel's, which cannot hold 128 members: MiaError, data-dependent, AFTER every other point has been
    written -- the same raise as weights_stream64's."""
    s = shapes(128)
    nb = s["nb"]
    strong, want = strong_cluster(s["case"], nb, INF)
    assert 0 < int(want.sum()) < G
    out = torch.full((G, 128, 128), -7.0, dtype=torch.float64, device=DEV)
    Yb, d = dev(strong["yb"]), dev(strong["d"])
    W, fl, finish = eng.weights_patch64(Yb, d, nb, mia.mesh_tiles((NY, NX)), INF, out=out, return_flags=True, defer_retry=True)
    torch.cuda.synchronize()
    assert last_kernel() == KERNEL + "<8>"
    assert np.array_equal((fl.cpu().numpy() & 8) != 0, want)
    with pytest.raises(MiaError, match="status -3"):
        finish()
    torch.cuda.synchronize()
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all())
    ref = O.letkf_analysis(strong["state"], strong["grid"], strong["obs"], strong["yb"], strong["d"], s["c"], INF)[1]
    check(out.cpu().numpy()[~want], ref[~want], "k 128 under a map: the %d points that were not declined" % int((~want).sum()))


# ---- 8. overflow ---------------------------------------------------------------------------------------------------------------------
def test_a_list_longer_than_p_max_or_the_image_overflows_for_that_point_only(mia, eng, shapes):
    s = shapes(40)
    nb, tiles = s["nb"], mia.mesh_tiles((NY, NX))
    cnt = nb.cnt.cpu().numpy()
    # the image one block short of the longest list (32 of 45 slots)
    ub = (SHAPES[40][1] + 15) // 16 - 1
    over = cnt > 16 * ub
    assert 0 < over.sum() < G
    W, fl, kern = patch(eng, s["case"], nb, tiles, union_blocks=ub)
    od = torch.as_tensor(over, device=DEV)
    assert kern == KERNEL + "<3>" and np.array_equal(fl.cpu().numpy() == 1, over)
    assert bool(torch.isnan(W[od]).all()) and torch.equal(W[~od], s["W"][~od]) and torch.equal(fl[~od], s["fl"][~od])
    # a bound p_max that the interior lists exceed (41 > k): the same lists otherwise
    short = NeighbourLists(nb.cnt, nb.idx, nb.w, nb.p_cap, 41, nb.g0, nb.g1)
    over = cnt > 41
    assert 0 < over.sum() < G
    W, fl, kern = patch(eng, s["case"], short, tiles)
    od = torch.as_tensor(over, device=DEV)
    assert kern == KERNEL + "<3>" and np.array_equal(fl.cpu().numpy() == 1, over)
    assert bool(torch.isnan(W[od]).all()) and torch.equal(W[~od], s["W"][~od]) and torch.equal(fl[~od], s["fl"][~od])


# ---- 9. invalid maps ----------------------------------------------------------------------------------------------------------------
def test_invalid_maps_raise_before_any_launch(mia, eng, shapes):
    s = shapes(20)
    good = mia.mesh_tiles((NY, NX))
    twice, missing, beyond, below = good.clone(), good.clone(), good.clone(), good.clone()
    twice[3, 2] = twice[5, 1]
    missing[7, 0] = -1
    beyond[2, 7] = G
    below[2, 7] = -2
    Yb, d = dev(s["case"]["yb"]), dev(s["case"]["d"])
    out = torch.full((G, 20, 20), -7.0, dtype=torch.float64, device=DEV)
    for tiles, word in ((twice, "more than once"), (missing, "does not occur"), (beyond, "outside"), (below, "outside"),
                        (good[:0], "does not occur")):
        for ub in (None, 4):                           # (a given union_blocks leaves the count, not the validation)
            with pytest.raises(ValueError, match=word):
                eng.weights_patch64(Yb, d, s["nb"], tiles, INF, out=out, union_blocks=ub)
    for tiles in (good.to(torch.int64), good.reshape(-1), good[:, :8]):
        with pytest.raises(ValueError, match="tile_points"):
            eng.weights_patch64(Yb, d, s["nb"], tiles, INF, out=out)
    for ub in (0, 17):
        with pytest.raises(ValueError, match="union_blocks"):
            eng.weights_patch64(Yb, d, s["nb"], good, INF, out=out, union_blocks=ub)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # outside the route: p_max <= k, float32 input, rbf_gamma -- None, as weights_stream64
    nbs = eng.localize(s["case"]["grid"], s["case"]["obs"], [0.9])
    assert nbs.p_max <= 20
    assert eng.weights_patch64(Yb, d, nbs, good, INF) is None
    assert eng.weights_patch64(Yb.float(), d.float(), s["nb"], good, INF) is None
    assert eng.weights_patch64(Yb, d, s["nb"], good, INF, rbf_gamma=0.5) is None


# ---- 10. the class ------------------------------------------------------------------------------------------------------------------
def class_weights(mia, eng, case, c, **kw):
    f32_first(eng)          # (so that the reported kernel name is known to be fresh: the Jacobi kernel never reports one)
    f = mia.LETKF(mia.GaspariCohn(c, mia.EuclideanMetric()), INF, **kw)
    W = f.estimate_weights_arrays(case["yb"], case["d"], grid_coords=case["grid"], obs_coords=case["obs"])
    torch.cuda.synchronize()
    return W, last_kernel()


def test_the_class_takes_the_map_at_128_members(mia, eng, shapes):
    s = shapes(128)
    plain, kern = class_weights(mia, eng, s["case"], s["c"])
    assert kern == PARENT + "<8>" and torch.equal(plain, s["W"])
    W, kern = class_weights(mia, eng, s["case"], s["c"], mesh_shape=(NY, NX))
    assert kern == KERNEL + "<8>" and W.dtype == torch.float64 and torch.equal(W, plain)
    with pytest.warns(RuntimeWarning, match="mesh_shape"):
        wrong, kern = class_weights(mia, eng, s["case"], s["c"], mesh_shape=(NY, NX + 1))
    assert kern == PARENT + "<8>" and torch.equal(wrong, plain)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*mesh_shape.*")      # float32 never looks at mesh_shape
        case = shapes(20)["case"]
        assert class_weights(mia, eng, case, 1.5, dtype=torch.float32, mesh_shape=(NY, NX + 1))[0].dtype == torch.float32


@pytest.mark.parametrize("k", [40, 80])
def test_the_class_takes_the_map_exactly_where_the_rule_says(mia, eng, shapes, k):
    s = shapes(k)
    plain, plain_kernel = class_weights(mia, eng, s["case"], s["c"])
    W, kern = class_weights(mia, eng, s["case"], s["c"], mesh_shape=(NY, NX))
    if eng._weights_patch64_auto(k, SHAPES[k][1]):
        assert kern == "%s<%d>" % (KERNEL, SHAPES[k][4]), kern
    else:
        assert KERNEL not in kern and kern == plain_kernel
    assert torch.equal(W, plain)
    ref = O.letkf_analysis(s["case"]["state"], s["case"]["grid"], s["case"]["obs"], s["case"]["yb"], s["case"]["d"], s["c"], INF)[1]
    check(W.cpu().numpy(), ref, "class at k = %d with mesh_shape (%s)" % (k, kern))


def test_weight_save_path_writes_the_same_file_with_and_without_mesh_shape(mia, eng, shapes, tmp_path):
    from torch_assimilate_amd import weights_io as io
    s = shapes(128)
    case = s["case"]
    got = {}
    for name, kw, kernel in (("plain", {}, PARENT), ("mesh", dict(mesh_shape=(NY, NX)), KERNEL)):
        path = str(tmp_path / (name + ".nc"))
        f = mia.LETKF(mia.GaspariCohn(s["c"], mia.EuclideanMetric()), INF, weight_save_path=path, **kw)
        xa = f.analyse_arrays(case["state"], case["yb"], case["d"], grid_coords=case["grid"], obs_coords=case["obs"])
        torch.cuda.synchronize()
        assert last_kernel() == kernel + "<8>", last_kernel()
        got[name] = (xa, io.load_weights(path)[0])
    assert tuple(got["mesh"][1].shape) == (G, 128, 128)
    assert torch.equal(got["mesh"][1], got["plain"][1]) and torch.equal(got["mesh"][0], got["plain"][0])
    assert torch.equal(got["mesh"][1].to(DEV), s["W"])


# ---- 11. applying the weights ------------------------------------------------------------------------------------------------------
def test_the_weights_applied_to_a_state_give_the_stream64_analysis(mia, eng, shapes):
    """apply_local_weights(X, W) against analysis(method="stream64") at 80 members: 1.3e-15, the figure DESIGN 9 records for
    weights_stream64 (relative Frobenius error)."""
    from oracle_pool import per_point_errors
    s = shapes(80)
    W, fl, kern = patch(eng, s["case"], s["nb"], mia.mesh_tiles((NY, NX)))
    assert kern == KERNEL + "<5>"
    X, Yb, d = dev(s["case"]["state"]), dev(s["case"]["yb"]), dev(s["case"]["d"])
    xw = eng.apply_local_weights(X, W)
    xm = eng.analysis(X, Yb, d, s["nb"], INF, method="stream64")
    torch.cuda.synchronize()
    assert last_kernel().startswith("letkf_stream64_kernel<")
    pp, fro = per_point_errors(xw.cpu().numpy(), xm.cpu().numpy())
    print("\n[patch64w] W applied against analysis(method='stream64'): rel. Frobenius %.3e, worst grid point %.3e" % (fro, pp.max()))
    assert fro <= 1.3e-15
    assert pp.max() <= TOL64

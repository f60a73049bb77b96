"""The float64 IEnKS weight update with tau = 1 for dense local networks under a tile map (csrc/lienks_patch64.hip,
mia_lienks_update_patch_f64, LetkfEngine.ienks_update(method="patch64", tile_points=...)): lienks_stream64_kernel's update with
the sixteen points of a tile taken from a map -- 4 x 4 patches of a 2-D mesh, whose unions fit one pass where sixteen
consecutive points (a 16 x 1 strip) run in parts.  Contract: relative Frobenius error AND the worst single grid point <= 1e-10
against O.lienks_weights; in addition W and flags are bit-identical to ienks_update(method="stream64") on the same
lists under ANY map, because slot = rank of the observation index, every sum over the union is one ascending chain and a
point's row means depend on its own matrix alone.

The fixture is tests/test_gpu_patch64w.py's: an 18 x 18 mesh with an observation at every point (324 points; 25 patches of
4 x 4, the ones at the right and lower edge with dead slots), here at inflation 1 (the IEnKS constants).  List lengths, unions
and degrees are counted on the CPU from the lists first, so that a changed fixture cannot turn a test into something else.
The bundle variant passes records Yb eps, so that D = Yl / eps is the case's own Yb.

Run against a build without this route every test fails: ienks_update knows no method "patch64" and the IEnKS classes take no
mesh_shape."""
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import letkf_oracle as O
from test_gpu_ienks64 import weights_in
from test_gpu_ienks_stream64 import EPS, GENERAL, OVERFLOW, RETRY, NONFINITE, VARIANTS, check, dev, f32_first, last_kernel, upd
from test_gpu_patch64w import NX, NY, SHAPES, random_map, unions_of
from test_gpu_stream64 import expected_degrees64, largest_union, mesh_case, strong_cluster
from torch_assimilate_amd._cabi import MiaError
from torch_assimilate_amd.engine import NeighbourLists

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = NY * NX
KERNEL = "lienks_patch64_kernel"
PARENT = "lienks_stream64_kernel"
CAP = 127
# k -> the largest Chebyshev degree of the fixture at inflation 1, counted on the CPU (the cap is 127: nothing is declined)
DEGREES = {8: 30, 20: 30, 40: 30, 64: 31, 80: 33, 96: 31, 112: 33, 128: 32}


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


def kname(k, kernel=KERNEL):
    return "%s<%d>" % (kernel, (k + 15) // 16)


@functools.lru_cache(maxsize=None)
def mesh(k):
    return mesh_case(NX, NY, k, 1, seed=60 + k)            # (shared: the tests copy before they change a record)


@functools.lru_cache(maxsize=None)
def w_in_mesh(k, bundle):
    return weights_in(G, k, k, bundle)                     # (shared: a test that changes an element copies first)


@functools.lru_cache(maxsize=None)
def oracle_mesh(k, vname):
    """O.lienks_weights of the fixture from the per-point weights w_in_mesh: computed once, shared, never written to"""
    case, c = mesh(k), SHAPES[k][0]
    eps, scale = (EPS, EPS) if vname == "bundle" else (None, 1.0)
    W = O.lienks_weights(w_in_mesh(k, eps is not None), case["grid"], case["obs"], case["yb"] * scale, case["d"], c, 1.0, eps)
    W.setflags(write=False)
    return W


@pytest.fixture(scope="module")
def shapes(eng):
    """(k, variant) -> case, lists and method="stream64"'s W and flags: computed once, shared, never written to"""
    lists, memo = {}, {}

    def get(k, vname="bundle"):
        if k not in lists:
            c, p_max, _, strip, _ = SHAPES[k]
            nb = eng.localize(mesh(k)["grid"], mesh(k)["obs"], [c])
            assert nb.p_max == p_max and p_max > k and largest_union(nb) == strip
            want = expected_degrees64(mesh(k)["yb"], nb, 1.0)
            assert int(want.max()) == DEGREES[k] < CAP          # (on the CPU beforehand: nothing near the cap)
            lists[k] = (nb, want)
        if (k, vname) not in memo:
            eps, scale = (EPS, EPS) if vname == "bundle" else (None, 1.0)
            nb, want = lists[k]
            case = mesh(k)
            w_in = w_in_mesh(k, eps is not None)
            W, fl, kern = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
            assert kern == kname(k, PARENT) and int((fl & 0xff).max()) == 0
            memo[k, vname] = dict(case=case, nb=nb, c=SHAPES[k][0], W=W, fl=fl, w_in=w_in, eps=eps, yb=case["yb"] * scale, want=want)
        return memo[k, vname]
    return get


def patch(eng, s, tiles, w_in=None, yb=None, nb=None, **kw):
    """ienks_update(method="patch64") on a shared case: (W, flags as numpy, kernel name)"""
    return upd(eng, s["w_in"] if w_in is None else w_in, s["yb"] if yb is None else yb, s["case"]["d"], s["nb"] if nb is None else nb,
               s["eps"], method="patch64", tile_points=tiles, **kw)


def same_as_stream(s, W, fl, kern, k, what):
    assert kern == kname(k), kern
    assert np.array_equal(fl, s["fl"]), what
    assert torch.equal(W, s["W"]), what


# ---- 1. bit-equality and parity, per shape and variant ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", sorted(SHAPES))
def test_mesh_patches_equal_the_streamed_route_bit_for_bit(mia, eng, shapes, k):
    tiles = mia.mesh_tiles((NY, NX))
    assert tiles.shape == (25, 16) and int((tiles < 0).sum()) == 25 * 16 - G
    union = SHAPES[k][2]
    for vname, eps, scale in VARIANTS:
        s = shapes(k, vname)
        assert max(unions_of(s["nb"], tiles)) == union <= 256
        W, fl, kern = patch(eng, s, tiles)
        same_as_stream(s, W, fl, kern, k, vname + ", 4 x 4 patches")
        assert int((fl & 0xff).max()) == 0, vname            # nothing declined, nothing non-finite
        assert np.array_equal((fl >> 8) & 0xff, s["want"]), vname
        ent = s["nb"].tile_census[id(tiles)]
        assert ent[0] is tiles and ent[2] == union            # the census counted what the CPU counts, and it is kept
        again = patch(eng, s, tiles)[0]
        assert torch.equal(again, s["W"]) and s["nb"].tile_census[id(tiles)] is ent        # (no second census for the same map)
        check(W.cpu().numpy(), oracle_mesh(k, vname),
              "%s k %d c %g p_max %d, 4 x 4 patches, union %d (%s)" % (vname, k, s["c"], SHAPES[k][1], union, kern))


# ---- 2. any partition is a map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 80])
def test_any_partition_is_a_map(mia, eng, shapes, k):
    for vname, eps, scale in VARIANTS:
        s = shapes(k, vname)
        for shape in ((2, 8), (8, 2)):
            W, fl, kern = patch(eng, s, mia.mesh_tiles((NY, NX), patch=shape))
            same_as_stream(s, W, fl, kern, k, "%s, patch %r" % (vname, shape))
        tiles = random_map(7 + k)
        t = tiles.numpy()
        assert (t[0] >= 0).sum() == 1 and t[0, 0] < 0 and (t[1] >= 0).sum() == 0
        assert any(row[0] < 0 <= row.max() for row in t[2:]) and any((np.diff((row >= 0).astype(int)) > 0).any() for row in t[2:])
        if k == 80:
            assert max(unions_of(s["nb"], tiles)) > 256        # (scattered points: unions above 256 run in parts)
        W, fl, kern = patch(eng, s, tiles)
        same_as_stream(s, W, fl, kern, k, vname + ", random map")


# ---- 3. shards ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 80])
def test_sub_ranges_and_shards_have_the_full_calls_bits(mia, eng, shapes, k):
    for vname, eps, scale in VARIANTS:
        s = shapes(k, vname)
        for g0, g1 in ((0, 150), (37, 290), (0, 163), (163, G)):
            nbp = eng.localize(s["case"]["grid"], s["case"]["obs"], [s["c"]], g0=g0, g1=g1)
            assert nbp.p_max == SHAPES[k][1]
            W, fl, kern = patch(eng, s, mia.mesh_tiles((NY, NX), g0, g1), w_in=s["w_in"][g0:g1], nb=nbp)
            assert kern == kname(k) and W.shape[0] == g1 - g0
            assert torch.equal(W, s["W"][g0:g1]) and np.array_equal(fl, s["fl"][g0:g1]), (vname, g0, g1)


# ---- 4. halving under the map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 40, 80, 128])
def test_the_smallest_image_runs_tiles_in_parts(mia, eng, shapes, k):
    ub = (SHAPES[k][1] + 15) // 16
    assert 16 * ub < SHAPES[k][2]                             # the union of a patch does not fit, a single list does
    for vname, eps, scale in VARIANTS:
        s = shapes(k, vname)
        W, fl, kern = patch(eng, s, mia.mesh_tiles((NY, NX)), union_blocks=ub)
        same_as_stream(s, W, fl, kern, k, "%s, union_blocks %d" % (vname, ub))


def test_unions_above_the_full_image_run_in_halves(mia, eng):
    """k = 128 at radius 4: p_max 185, patch unions up to 264 > 256 slots -- tiles run in halves at the full image"""
    k = 128
    case = mesh_case(NX, NY, k, 1, seed=188)
    nb = eng.localize(case["grid"], case["obs"], [4.0])
    tiles = mia.mesh_tiles((NY, NX))
    assert nb.p_max == 185 and max(unions_of(nb, tiles)) == 264 > 256
    w_in = w_in_mesh(k, True)
    Ws, fs, kern = upd(eng, w_in, case["yb"] * EPS, case["d"], nb, EPS)
    assert kern == kname(k, PARENT) and int((fs & 0xff).max()) == 0
    W, fl, kern = upd(eng, w_in, case["yb"] * EPS, case["d"], nb, EPS, method="patch64", tile_points=tiles)
    assert kern == kname(k) and nb.tile_census[id(tiles)][2] == 264
    assert torch.equal(W, Ws) and np.array_equal(fl, fs)


# ---- 5. one shared matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 80])
def test_one_shared_matrix(mia, eng, shapes, k):
    """ONE (k, k) matrix for all points (w_stride = 0, no map on W_in): the prior in both variants, and a matrix with another mean
    and another Wp in the bundle variant -- under the mesh map and a random one."""
    s = shapes(k)
    case, nb, c = s["case"], s["nb"], s["c"]
    w1 = weights_in(1, k, 5, True)[0]
    for w, vname, eps, scale in [(np.eye(k),) + v for v in VARIANTS] + [(w1, "bundle", EPS, EPS)]:
        Ws, fs, kern = upd(eng, w, case["yb"] * scale, case["d"], nb, eps)
        assert kern == kname(k, PARENT) and int((fs & 0xff).max()) == 0
        for tiles in (mia.mesh_tiles((NY, NX)), random_map(11)):
            W, fl, kern = upd(eng, w, case["yb"] * scale, case["d"], nb, eps, method="patch64", tile_points=tiles)
            assert kern == kname(k) and torch.equal(W, Ws) and np.array_equal(fl, fs), vname
        ref = O.lienks_weights(w, case["grid"], case["obs"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, one shared %s matrix, k %d" % (vname, "prior" if w is not w1 else "non-prior", k))


# ---- 6. points without observations -------------------------------------------------------------------------------------------------
def test_points_without_observations_get_their_own_weights_back(mia, eng):
    """Observations on rows y >= 9 only: in patches that hold both kinds of points, those without observations get THEIR per-point
    W_in back bit for bit with flag 0 -- the one address the weights twin does not have."""
    k, c = 20, 1.5
    case = mesh_case(NX, NY, k, 1, seed=31)
    keep = case["obs"][:, 1] >= 9
    case = dict(case, obs=case["obs"][keep], yb=case["yb"][:, keep], d=case["d"][keep])
    nb = eng.localize(case["grid"], case["obs"], [c])
    assert nb.p_max == 25 > k
    far = nb.cnt.cpu().numpy() == 0
    mesh_map = mia.mesh_tiles((NY, NX))
    mixed = [row for row in mesh_map.numpy() if far[row[row >= 0]].any() and not far[row[row >= 0]].all()]
    assert 0 < far.sum() < G and len(mixed) >= 4              # patches that hold both kinds of points
    sel = torch.as_tensor(far, device=DEV)
    for vname, eps, scale in VARIANTS:
        w_in = w_in_mesh(k, eps is not None)
        Ws, fs, kern = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps)
        assert kern == kname(k, PARENT)
        for tiles in (mesh_map, random_map(5)):
            W, fl, kern = upd(eng, w_in, case["yb"] * scale, case["d"], nb, eps, method="patch64", tile_points=tiles)
            assert kern == kname(k) and torch.equal(W, Ws) and np.array_equal(fl, fs), vname
            assert torch.equal(W[sel], dev(w_in)[sel])
            assert int(np.abs(fl[far]).max()) == 0 and int(fl[~far].min()) > 0 and int((fl & 0xff).max()) == 0
        ref = O.lienks_weights(w_in, case["grid"], case["obs"], case["yb"] * scale, case["d"], c, 1.0, eps)
        check(W.cpu().numpy(), ref, "%s, observations on rows y >= 9 only" % vname)


# ---- 7. a NaN record ------------------------------------------------------------------------------------------------------------------
def test_a_nan_record_stays_with_the_points_that_list_it(mia, eng, shapes):
    s = shapes(20)
    nb, j = s["nb"], 151
    bad = s["yb"].copy()
    bad[3, j] = np.nan
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
    assert 0 < uses.sum() < G
    Ws, fs, kern = upd(eng, s["w_in"], bad, s["case"]["d"], nb, s["eps"])
    assert kern == kname(20, PARENT)
    keep = torch.as_tensor(~uses, device=DEV)
    for tiles in (mia.mesh_tiles((NY, NX)), random_map(3)):
        W, fl, kern = patch(eng, s, tiles, yb=bad)
        assert kern == kname(20)
        assert np.array_equal((fl & NONFINITE) != 0, uses)
        assert np.array_equal(fl, fs)
        assert torch.equal(W[keep], s["W"][keep])              # the clean run's bits: the tile was done slot by slot
        assert torch.equal(torch.isnan(W), torch.isnan(Ws))


# ---- 8. the transform variant away from the prior -------------------------------------------------------------------------------------
def test_transform_points_off_the_prior_are_declined_whole(mia, eng, shapes):
    """Per-point weights with Wp != I (off by 1e-10 in one element) at some points of a patch and Wp = I at the others: the
    former carry MIA_FLAG_RETRY, are counted and left untouched; at k = 20 the general kernel redoes them to the oracle's parity.
    The others carry stream64's bits."""
    k = 20
    s = shapes(k, "transform")
    nb, case = s["nb"], s["case"]
    tiles = mia.mesh_tiles((NY, NX))
    assert int(nb.cnt.min()) > 0
    w_in = np.array(s["w_in"])
    chosen = np.zeros(G, dtype=bool)
    first = tiles.numpy()[7]                                  # an interior patch: three of its sixteen points, and two elsewhere
    for g, (i, j) in ((int(first[0]), (0, 1)), (int(first[5]), (19, 3)), (int(first[15]), (17, 17)), (0, (4, 4)), (G - 1, (1, 0))):
        chosen[g] = True
        w_in[g, i, j] += 1e-10
    sel = torch.as_tensor(chosen, device=DEV)
    got = {}
    for method, kw, kernel in (("stream64", {}, PARENT), ("patch64", dict(tile_points=tiles), KERNEL)):
        out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
        f32_first(eng)
        win_d, yb_d, d_d = dev(w_in), dev(case["yb"]), dev(case["d"])      # (alive until the deferred redo has run)
        W, fl, finish = eng.ienks_update(win_d, yb_d, d_d, nb, 1.0, None, return_flags=True, method=method, defer_retry=True,
                                         out=out, **kw)
        torch.cuda.synchronize()
        assert W is out and last_kernel() == kname(k, kernel)
        fln = fl.cpu().numpy()
        assert np.array_equal((fln & 0xff) == RETRY, chosen) and int((fln & 0xff)[~chosen].max()) == 0
        assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())
        got[method] = (out.clone(), fln)
        assert finish() == int(chosen.sum())
        torch.cuda.synchronize()
        assert int((fl.cpu().numpy() & RETRY).max()) == 0 and torch.equal(out[~sel], got[method][0][~sel])
    assert torch.equal(got["patch64"][0], got["stream64"][0]) and np.array_equal(got["patch64"][1], got["stream64"][1])
    assert torch.equal(got["patch64"][0][~sel], s["W"][~sel])
    ref = O.lienks_weights(w_in, case["grid"], case["obs"], case["yb"], case["d"], s["c"], 1.0, None)
    check(out.cpu().numpy(), ref, "transform, five points off the prior redone")


# ---- 9. decline by degree ---------------------------------------------------------------------------------------------------------------
def test_a_strong_cluster_is_declined_and_redone_at_40_members(mia, eng, shapes):
    k = 40
    s = shapes(k)
    nb = s["nb"]
    strong, want = strong_cluster(s["case"], nb, 1.0)
    n_decl = int(want.sum())
    assert 0 < n_decl < G                          # (the CPU restatement first: the cluster's points and no others)
    assert eng._ienks_general_fits(k, SHAPES[k][1], 1.0, True)
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    win_d, yb_d, d_d = dev(s["w_in"]), dev(strong["yb"] * EPS), dev(strong["d"])
    f32_first(eng)
    W, fl, finish = eng.ienks_update(win_d, yb_d, d_d, nb, 1.0, EPS, return_flags=True, method="patch64", defer_retry=True, out=out,
                                     tile_points=mia.mesh_tiles((NY, NX)))
    torch.cuda.synchronize()
    assert W is out and last_kernel() == kname(k)
    assert np.array_equal((fl.cpu().numpy() & RETRY) != 0, want)
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all()) and not bool((out[~sel] == -7.0).any())     # declined blocks are left untouched
    before = out.clone()
    assert finish() == n_decl                                                         # the counter, then the deferred redo
    torch.cuda.synchronize()
    assert int((fl.cpu().numpy() & RETRY).max()) == 0 and torch.equal(out[~sel], before[~sel])
    ref = O.lienks_weights(s["w_in"], strong["grid"], strong["obs"], strong["yb"] * EPS, strong["d"], s["c"], 1.0, EPS)
    check(out.cpu().numpy(), ref, "strong cluster under a map, %d points redone" % n_decl)


def test_a_declined_point_raises_at_128_members_after_the_others_are_written(mia, eng, shapes):
    """The redo is the general kernel's, which cannot hold 128 members: MiaError, data-dependent, AFTER every other point has been
    written -- the same raise as method="stream64"'s."""
    k = 128
    s = shapes(k)
    nb = s["nb"]
    strong, want = strong_cluster(s["case"], nb, 1.0)
    assert 0 < int(want.sum()) < G
    out = torch.full((G, k, k), -7.0, dtype=torch.float64, device=DEV)
    win_d, yb_d, d_d = dev(s["w_in"]), dev(strong["yb"] * EPS), dev(strong["d"])
    f32_first(eng)
    W, fl, finish = eng.ienks_update(win_d, yb_d, d_d, nb, 1.0, EPS, return_flags=True, method="patch64", defer_retry=True, out=out,
                                     tile_points=mia.mesh_tiles((NY, NX)))
    torch.cuda.synchronize()
    assert last_kernel() == kname(k)
    assert np.array_equal((fl.cpu().numpy() & RETRY) != 0, want)
    with pytest.raises(MiaError, match="status -3"):
        finish()
    torch.cuda.synchronize()
    sel = torch.as_tensor(want, device=DEV)
    assert bool((out[sel] == -7.0).all())
    ref = O.lienks_weights(s["w_in"], strong["grid"], strong["obs"], strong["yb"] * EPS, strong["d"], s["c"], 1.0, EPS)
    check(out.cpu().numpy()[~want], ref[~want], "k 128 under a map: the %d points that were not declined" % int((~want).sum()))


# ---- 10. overflow ---------------------------------------------------------------------------------------------------------------------
def test_a_list_longer_than_p_max_or_the_image_overflows_for_that_point_only(mia, eng, shapes):
    s = shapes(40)
    nb, tiles = s["nb"], mia.mesh_tiles((NY, NX))
    cnt = nb.cnt.cpu().numpy()
    # the image one block short of the longest list (32 of 45 slots)
    ub = (SHAPES[40][1] + 15) // 16 - 1
    # a bound p_max that the interior lists exceed (41 > k): the same lists otherwise
    short = NeighbourLists(nb.cnt, nb.idx, nb.w, nb.p_cap, 41, nb.g0, nb.g1)
    for over, kw in ((cnt > 16 * ub, dict(union_blocks=ub)), (cnt > 41, dict(nb=short))):
        assert 0 < over.sum() < G
        W, fl, kern = patch(eng, s, tiles, **kw)
        od = torch.as_tensor(over, device=DEV)
        assert kern == kname(40) and np.array_equal(fl == OVERFLOW, over)
        assert bool(torch.isnan(W[od]).all()) and torch.equal(W[~od], s["W"][~od]) and np.array_equal(fl[~over], s["fl"][~over])


# ---- 11. invalid maps and arguments -----------------------------------------------------------------------------------------------
def test_invalid_maps_and_arguments_raise_before_any_launch(mia, eng, shapes):
    s = shapes(20)
    good = mia.mesh_tiles((NY, NX))
    twice, missing, beyond, below = good.clone(), good.clone(), good.clone(), good.clone()
    twice[3, 2] = twice[5, 1]
    missing[7, 0] = -1
    beyond[2, 7] = G
    below[2, 7] = -2
    w, Yb, d = dev(s["w_in"]), dev(s["yb"]), dev(s["case"]["d"])
    out = torch.full((G, 20, 20), -7.0, dtype=torch.float64, device=DEV)

    def call(tiles, nb=s["nb"], w=w, **kw):
        return eng.ienks_update(w, Yb, d, nb, kw.pop("tau", 1.0), EPS, method=kw.pop("method", "patch64"), out=out, tile_points=tiles, **kw)
    for tiles, word in ((twice, "more than once"), (missing, "does not occur"), (beyond, "outside"), (below, "outside"),
                        (good[:0], "does not occur")):
        for ub in (None, 4):                           # (a given union_blocks leaves the count, not the validation)
            with pytest.raises(ValueError, match=word):
                call(tiles, union_blocks=ub)
    for tiles in (good.to(torch.int64), good.reshape(-1), good[:, :8]):
        with pytest.raises(ValueError, match="tile_points"):
            call(tiles)
    for ub in (0, 17):
        with pytest.raises(ValueError, match="union_blocks"):
            call(good, union_blocks=ub)
    with pytest.raises(ValueError, match="the patch64 route needs tile_points"):
        call(None)
    for method in ("auto", "eig", "stream64", "tile64"):
        with pytest.raises(ValueError, match="patch64"):
            call(good, method=method)
        with pytest.raises(ValueError, match="patch64"):
            call(None, method=method, union_blocks=4)
    with pytest.raises(ValueError, match="tau"):
        call(good, tau=0.9)
    with pytest.raises(ValueError, match="float64"):
        eng.ienks_update(w.float(), Yb.float(), d.float(), s["nb"], 1.0, EPS, method="patch64", tile_points=good)
    nbs = eng.localize(s["case"]["grid"], s["case"]["obs"], [0.9])
    assert nbs.p_max <= 20
    with pytest.raises(ValueError, match="covers 2 <= k <= 128 and k < p_max <= 256"):
        call(good, nb=nbs)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- 12. the classes, no method named -------------------------------------------------------------------------------------------------
def class_loop(mia, eng, cls, k, w_in, yb, d, case, c, **kw):
    f32_first(eng)
    args = dict(tau=1.0, dtype=torch.float64)
    if cls is mia.LocalizedIEnKSBundle:
        args["epsilon"] = EPS
    args.update(kw)
    a = cls(lambda x, it: (x, x), mia.GaspariCohn(c, mia.EuclideanMetric()), **args)
    W = a.inner_loop_arrays(np.array(w_in), yb, d, grid_coords=case["grid"], obs_coords=case["obs"])
    torch.cuda.synchronize()
    return W, last_kernel()


@pytest.mark.parametrize("k,vname", [(96, "bundle"), (128, "bundle"), (80, "transform")])
def test_the_classes_take_the_map_where_the_dense_kernel_ran(mia, eng, shapes, k, vname):
    s = shapes(k, vname)
    bundle = vname == "bundle"
    cls = mia.LocalizedIEnKSBundle if bundle else mia.LocalizedIEnKSTransform
    w_in = s["w_in"] if bundle else np.eye(k)                 # (the transform class starts from the shared prior)
    assert eng._ienks_stream64_auto(k, SHAPES[k][1], bundle, not bundle) and eng._ienks_patch64_auto(k, SHAPES[k][1], bundle, not bundle)
    plain, kern = class_loop(mia, eng, cls, k, w_in, s["yb"], s["case"]["d"], s["case"], s["c"])
    assert kern == kname(k, PARENT), kern
    W, kern = class_loop(mia, eng, cls, k, w_in, s["yb"], s["case"]["d"], s["case"], s["c"], mesh_shape=(NY, NX))
    assert kern == kname(k), kern
    assert W.dtype == torch.float64 and torch.equal(W, plain)
    ref = oracle_mesh(k, vname) if bundle else O.lienks_weights(np.eye(k), s["case"]["grid"], s["case"]["obs"], s["yb"], s["case"]["d"],
                                                                s["c"], 1.0, None)
    check(W.cpu().numpy(), ref, "%s class at k = %d with mesh_shape (%s)" % (vname, k, kern))
    if k == 96:
        with pytest.warns(RuntimeWarning, match="mesh_shape"):
            wrong, kern = class_loop(mia, eng, cls, k, w_in, s["yb"], s["case"]["d"], s["case"], s["c"], mesh_shape=(NY, NX + 1))
        assert kern == kname(k, PARENT) and torch.equal(wrong, plain)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*mesh_shape.*")      # float32 never looks at mesh_shape
            s20 = shapes(20)
            w32 = class_loop(mia, eng, cls, 20, s20["w_in"], s20["yb"], s20["case"]["d"], s20["case"], s20["c"], dtype=torch.float32,
                             mesh_shape=(NY, NX + 1))[0]
            assert w32.dtype == torch.float32


def test_three_bundle_iterations_on_a_mesh_have_equal_bits_with_and_without_mesh_shape(mia, eng):
    """LocalizedIEnKSBundle.update_state_arrays, three iterations at k = 96 on the 18 x 18 mesh with an observation at every point
    (radius 3: 101 local observations, which the general kernel cannot hold)."""
    k, c = 96, 3.0
    rs = np.random.RandomState(96)
    case = mesh(k)
    state = rs.normal(size=(1, k, G))
    y, var = rs.normal(size=G), np.full(G, 0.5)

    def forward_model(x, it):
        nxt = 0.9 * x + 0.1 * torch.roll(x, 1, dims=-1)
        return nxt, nxt

    def observe(pseudo):
        return [pseudo[0]], [torch.tensor(y)], [torch.tensor(var)], None
    got = {}
    for name, kw, kernel in (("plain", {}, PARENT), ("mesh", dict(mesh_shape=(NY, NX)), KERNEL)):
        a = mia.LocalizedIEnKSBundle(forward_model, mia.GaspariCohn(c, mia.EuclideanMetric()), max_iter=3, tau=1.0, epsilon=EPS,
                                     dtype=torch.float64, **kw)
        f32_first(eng)
        got[name] = a.update_state_arrays(state, observe, grid_coords=case["grid"], obs_coords=case["obs"])
        torch.cuda.synchronize()
        assert last_kernel() == kname(k, kernel), last_kernel()
    assert got["mesh"].dtype == torch.float64 and bool(torch.isfinite(got["mesh"]).all())
    assert torch.equal(got["mesh"], got["plain"])


@pytest.mark.parametrize("k", [40, 64])
def test_the_class_takes_the_map_exactly_where_the_rule_says(mia, eng, shapes, k):
    s = shapes(k)
    args = (mia, eng, mia.LocalizedIEnKSBundle, k, s["w_in"], s["yb"], s["case"]["d"], s["case"], s["c"])
    plain, plain_kernel = class_loop(*args)
    W, kern = class_loop(*args, mesh_shape=(NY, NX))
    if eng._ienks_patch64_auto(k, SHAPES[k][1], True, False):
        assert kern == kname(k), kern
    else:
        assert KERNEL not in kern and kern == plain_kernel and GENERAL in kern
    assert torch.equal(W, plain)


# ---- 13. addresses beyond 2^31 bytes, and the second row of the launch grid ------------------------------------------------------------
def test_weights_beyond_2_gib_under_a_permutation(eng):
    """A 1-D case at k = 40 over 170 000 points: W_out has 2.18e9 bytes, and under a random permutation of the points into tiles
    every lane's 64-bit base lies anywhere in it.  One shared W_in.  No oracle here: stream64 is the verified parent."""
    k, n = 40, 170000
    assert n * k * k * 8 > 2 ** 31
    case = O.synthetic_case(n, k, 1, seed=40)
    nb = eng.localize(case["grid_x"], case["obs_x"], [11.5])
    assert k < nb.p_max <= k + 8                              # (p_max just above k: short lists, many points)
    t = -np.ones(((n + 15) // 16) * 16, dtype=np.int32)
    t[:n] = np.random.RandomState(17).permutation(n)
    tiles = torch.as_tensor(t.reshape(-1, 16))
    w1 = weights_in(1, k, 5, True)[0]
    Ws, fs, kern = upd(eng, w1, case["yb"] * EPS, case["d"], nb, EPS)
    assert kern == kname(k, PARENT) and int((fs & 0xff).max()) == 0
    W, fl, kern = upd(eng, w1, case["yb"] * EPS, case["d"], nb, EPS, method="patch64", tile_points=tiles, union_blocks=16)
    assert kern == kname(k) and np.array_equal(fl, fs)
    assert W.data_ptr() != Ws.data_ptr() and torch.equal(W, Ws)


def test_more_than_65536_tiles(eng):
    """k = 2 with three local observations over 66 538 tiles in reversed order: the second row of the launch grid.  (The
    network of tests/large_grid_cases.py has lists of about 15 entries; its size and its reversed strips are used as they are.)"""
    from large_grid_cases import G_LARGE, reversed_strips
    k, n = 2, G_LARGE
    rs = np.random.RandomState(2)
    gx = np.arange(n, dtype=np.float64)
    yb = rs.normal(size=(k, n))
    yb -= yb.mean(axis=0)
    d = rs.normal(size=n)
    nb = eng.localize(gx, gx, [0.75])
    assert nb.p_max == 3 > k
    tiles = torch.as_tensor(reversed_strips(n))
    assert tiles.shape[0] == 66538 > 65536
    w1 = weights_in(1, k, 5, True)[0]
    Ws, fs, kern = upd(eng, w1, yb * EPS, d, nb, EPS)
    assert kern == kname(k, PARENT) and int((fs & 0xff).max()) == 0
    W, fl, kern = upd(eng, w1, yb * EPS, d, nb, EPS, method="patch64", tile_points=tiles)
    assert kern == kname(k) and np.array_equal(fl, fs) and torch.equal(W, Ws)

"""Cyclic coordinates (PeriodicMetric) on the GPU routes: per-point lists against the host statement of the distance, tile lists
against per-point lists, the step driver's kernels (fused, pair, RBF tile, weights tile) against the float64 oracle with the test's
own cyclic distance, invariances (seam-free rings, rolled rings, blocks of a partition at the seam) and the absence of any host
distance call."""
import numpy as np
import pytest
import torch

from conftest import rel_fro
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


def cyc(a, L):
    a = np.abs(a)
    if L > 0:
        a = np.mod(a, L)
        a = np.minimum(a, L - a)
    return a


def host_dist(g, obs, period, groups):
    """the test's own cyclic distance, (n_r, P)"""
    out = np.zeros((max(groups) + 1, obs.shape[0]))
    for c, grp in enumerate(groups):
        out[grp] += cyc(obs[:, c] - g[c], period[c]) ** 2
    return np.sqrt(out)


def mesh(*axes):
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(axes))


def geometry(name):
    rs = np.random.RandomState(11)
    if name == "ring":
        L = 150.0
        return np.arange(0, L, 0.5)[:, None], rs.uniform(-L, 2 * L, (200, 1)), [L], [4.0], [0], 0
    if name == "channel":
        return mesh(np.arange(60.0), np.arange(10.0)), rs.uniform(0, 1, (150, 2)) * [60, 10], [60.0, 0.0], [3.0], [0, 0], 0
    if name == "doubly":
        return mesh(np.arange(40.0), np.arange(30.0)), rs.uniform(0, 1, (120, 2)) * [40, 30], [40.0, 30.0], [2.5], [0, 0], 0
    if name == "3d_two_radii":
        return (mesh(np.arange(24.0), np.arange(3.0), np.arange(8.0)), rs.uniform(0, 1, (150, 3)) * [24, 3, 8], [24.0, 0.0, 0.0],
                [2.0, 3.0], [0, 0, 1], 0)
    if name == "ring_gc_inf":
        L = 100.0
        return np.arange(L)[:, None], rs.uniform(0, L, (90, 1)), [L], [5.0], [0], 1
    if name == "L5c":         # two cells along the ring: every cell once, the minimum image per pair
        return np.arange(50.0)[:, None], rs.uniform(0, 50, (40, 1)), [50.0], [10.0], [0], 0
    if name == "L3c":         # one cell, and the support (2c) wraps onto itself
        return np.arange(30.0)[:, None], rs.uniform(0, 30, (25, 1)), [30.0], [10.0], [0], 0
    if name == "ring_rolled":  # tile 0 holds x = L - 8 .. L - 1, 0 .. 7: tiles straddle the seam
        L = 160.0
        return np.roll(np.arange(L), 8)[:, None], np.arange(0, L, 2.0)[:, None], [L], [6.0], [0], 0
    raise KeyError(name)


GEOMS = ["ring", "channel", "doubly", "3d_two_radii", "ring_gc_inf", "L5c", "L3c", "ring_rolled"]


def loc_of(mia, radii, period, groups, taper):
    metric = mia.PeriodicMetric(period, coord_group=groups)
    if taper:
        return mia.GaspariCohnInf(radii[0], dist_func=metric)
    return mia.GaspariCohn(radii, dist_func=metric)


def point_lists(nb):
    cnt, idx, w = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy(), nb.w.cpu().numpy()
    return [{int(idx[g, j]): float(w[g, j]) for j in range(cnt[g])} for g in range(len(cnt))]


@pytest.mark.parametrize("name", GEOMS)
def test_point_lists_equal_the_host_spec(mia, eng, name):
    """Same index sets as the host callable's lists (localize_from_dist); weights to 1e-10 relative.  (The per-point kernels
    evaluate the taper from d^2 through a Newton-refined reciprocal square root, localize_from_dist from r by the reference's
    polynomial: near the edge of the support the two differ by up to ~1e-11 relative on open coordinates as well.)"""
    grid, obs, period, radii, groups, taper = geometry(name)
    loc = loc_of(mia, radii, period, groups, taper)
    gpu = point_lists(loc.neighbour_lists(eng, grid, obs))
    host_loc = loc_of(mia, radii, period, groups, taper)
    spec = host_loc.dist_func
    host_loc.dist_func = lambda g, o: spec(g, o)          # a plain callable: the host route of localize_from_dist
    assert host_loc.builtin_metric is None
    ref = point_lists(host_loc.neighbour_lists(eng, grid, obs))
    ambiguous, wrong, worst = 0, 0, 0.0
    for g, (a, b) in enumerate(zip(gpu, ref)):
        for j in set(a) ^ set(b):
            dist = host_dist(grid[g], obs[[j]], period, groups)[:, 0]
            w = np.prod([(O.gaspari_cohn_inf if taper else O.gaspari_cohn)(np.array([dist[r] / radii[r]]))[0]
                         for r in range(len(radii))])
            if abs(w - loc.epsilon) <= 1e-12 * loc.epsilon:
                ambiguous += 1
            else:
                wrong += 1
        for j in set(a) & set(b):
            worst = max(worst, abs(a[j] - b[j]) / abs(b[j]))
    print("%s: %d decisions within 1e-12 eps of eps, %d other differing decisions, largest relative weight difference %.1e"
          % (name, ambiguous, wrong, worst))
    assert worst <= 1e-10
    assert wrong == 0 and ambiguous == 0
    assert sum(len(a) for a in gpu) > 0


def tile_point_lists(tiles, n):
    hdr, uidx, D = tiles.unpack()
    out = []
    for t in range(hdr.shape[0]):
        npts = int(hdr[t, 2])
        keys = uidx[t]
        Dm = np.zeros((16, uidx.shape[1]), dtype=np.float32)
        for tb in range(D.shape[1]):
            for lane in range(64):
                for q in range(4):
                    Dm[lane & 15, 16 * tb + 4 * (lane >> 4) + q] = D[t, tb, lane, q]
        for p in range(npts):
            out.append(None if hdr[t, 0] < 0 else {int(keys[s]): float(Dm[p, s]) for s in np.flatnonzero(Dm[p])})
    assert len(out) == n
    return out


@pytest.mark.parametrize("name", GEOMS)
def test_tile_lists_equal_the_point_lists(mia, eng, name):
    grid, obs, period, radii, groups, taper = geometry(name)
    nb = eng.localize(grid, obs, radii, groups, taper=taper, period=period)
    tiles = eng.localize_tiles(grid, obs, radii, nb.p_max if grid.shape[1] == 1 else 88, groups, taper=taper, period=period)
    got = tile_point_lists(tiles, len(grid))
    ref = point_lists(nb)
    compared = 0
    for a, b in zip(got, ref):
        if a is None:                  # (a tile whose union does not fit the slots: the list route takes it)
            continue
        compared += 1
        assert sorted(a) == sorted(b)                                           # the masks: exact
        if taper:
            assert all(a[j] == np.float32(b[j]) for j in a)
        else:
            np.testing.assert_allclose([a[j] for j in sorted(a)], [np.float32(b[j]) for j in sorted(b)], rtol=2e-6 * len(radii))
    assert compared >= len(grid) // 2, (name, compared)
    if grid.shape[1] == 1:
        assert compared == len(grid)


def ring_case(G, L, k, stride, seed=3):
    case = O.synthetic_case(G, k, stride, seed=seed)
    case["state"] = case["state"].astype(np.float32).astype(np.float64)
    case["yb"] = case["yb"].astype(np.float32).astype(np.float64)
    case["d"] = case["d"].astype(np.float32).astype(np.float64)
    return case


def oracle_points(case, L, c, inf, pts, core=None):
    out = []
    for g in pts:
        dist = cyc(case["obs_x"] - case["grid_x"][g], L)[None]
        near = dist[0] < 2 * c + 1
        kw = {} if core is None else {"core": core}
        W = O.localized_weights(dist[:, near], case["yb"][:, near], case["d"][near], [c], inf, **kw)
        out.append(O.apply_weights(case["state"][:, :, [g]], W[None])[:, :, 0])
    return np.stack(out, -1)


def runner_step(mia, case, L, c, inf, gamma=None, **kw):
    r = mia.ShardedLetkf(torch.device(DEV), 0, 1, radii=[c], inf_factor=inf, rbf_gamma=gamma, period=[L], **kw)
    args = (torch.as_tensor(case["state"], dtype=torch.float32, device=DEV), torch.as_tensor(case["grid_x"], device=DEV),
            torch.as_tensor(case["obs_x"], device=DEV), torch.as_tensor(case["yb"], dtype=torch.float32, device=DEV),
            torch.as_tensor(case["d"], dtype=torch.float32, device=DEV))
    r.assimilate(*args)
    xa = r.assimilate(*args)
    assert r.native_steps >= 1 and r.last_flags_ok()
    return xa.cpu().numpy().astype(np.float64)


def check_points(xa, ref, pts, what):
    err = rel_fro(xa[:, :, pts], ref)
    worst = max(rel_fro(xa[:, :, [g]], ref[:, :, [i]]) for i, g in enumerate(pts))
    print("%s: rel. Frobenius error %.2e over %d points, worst single point %.2e" % (what, err, len(pts), worst))
    assert err <= 1e-5


def test_lorenz96_ring_through_the_interface(mia):
    from torch_assimilate_amd import _cabi
    G, L, c = 40, 40.0, 4.0
    case = ring_case(G, L, 20, 1)
    f = mia.LETKF(localization=mia.GaspariCohn(c, dist_func=mia.PeriodicMetric(L)), inf_factor=1.1, dtype=torch.float32)
    for _ in range(2):
        xa = f.analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"], case["obs_x"])
    assert "letkf_tile2f" in _cabi.last_analysis_kernel()
    pts = list(range(G))
    check_points(xa.cpu().numpy().astype(np.float64), oracle_points(case, L, c, 1.1, pts), pts, "Lorenz-96 ring")


def seam_and_sample(G, c, n, seed=0):
    near = [g for g in range(G) if min(g, G - g) <= 4 * c]
    rest = np.setdiff1d(np.arange(G), near)
    return sorted(set(near) | set(np.random.RandomState(seed).choice(rest, min(n, len(rest)), replace=False).tolist()))


def test_config2_ring_fused_kernel(mia):
    from torch_assimilate_amd import _cabi
    G, c = 100000, 10.0
    case = ring_case(G, float(G), 40, 2)
    xa = runner_step(mia, case, float(G), c, 1.1)
    assert "letkf_tile2f" in _cabi.last_analysis_kernel()
    pts = seam_and_sample(G, c, 5000)
    check_points(xa, oracle_points(case, float(G), c, 1.1, pts), pts, "config-2 ring")


def test_config4_ring_pair_kernel(mia):
    from torch_assimilate_amd import _cabi
    G, c = 4096, 16.5
    case = ring_case(G, float(G), 80, 1)
    xa = runner_step(mia, case, float(G), c, 1.1)
    assert "letkf_tile2p" in _cabi.last_analysis_kernel()
    pts = seam_and_sample(G, c, 300)
    check_points(xa, oracle_points(case, float(G), c, 1.1, pts), pts, "config-4 ring")


def test_config5_ring_rbf_tile_kernel(mia):
    from torch_assimilate_amd import _cabi
    G, c = 4096, 10.0
    case = ring_case(G, float(G), 40, 2)
    xa = runner_step(mia, case, float(G), c, 1.1, gamma=0.5)
    assert "lketkf_tile" in _cabi.last_analysis_kernel()
    core = lambda a, b, i: O.ketkf_weights(a, b, lambda x, y: O.rbf_kernel(x, y, 0.5), i)      # noqa: E731
    pts = seam_and_sample(G, c, 300)
    check_points(xa, oracle_points(case, float(G), c, 1.1, pts, core=core), pts, "config-5 ring")


def test_weights_tile_route(mia):
    from torch_assimilate_amd import _cabi
    G, L, c = 4096, 4096.0, 10.0
    case = ring_case(G, L, 40, 2)
    f = mia.LETKF(localization=mia.GaspariCohn(c, dist_func=mia.PeriodicMetric(L)), inf_factor=1.1, dtype=torch.float32)
    W = f.estimate_weights_arrays(case["yb"], case["d"], case["grid_x"], case["obs_x"]).cpu().numpy().astype(np.float64)
    assert "letkf_tile2_kernel" in _cabi.last_analysis_kernel()      # (the tile route: letkf_tile2_kernel + letkf_tile2w_kernel)
    pts = seam_and_sample(G, c, 300)
    ref = []
    for g in pts:
        dist = cyc(case["obs_x"] - case["grid_x"][g], L)[None]
        ref.append(O.localized_weights(dist, case["yb"], case["d"], [c], 1.1))
    err = rel_fro(W[pts], np.stack(ref))
    print("weights tile route: rel. Frobenius error %.2e" % err)
    assert err <= 1e-5


def test_seam_free_ring_equals_the_open_metric(mia):
    G, c = 4096, 10.0
    case = ring_case(G, float(G), 40, 2)
    keep = (case["obs_x"] > 2 * c + 1) & (case["obs_x"] < G - 2 * c - 1)
    case["obs_x"], case["yb"], case["d"] = case["obs_x"][keep], case["yb"][:, keep], case["d"][keep]
    per = runner_step(mia, case, float(G), c, 1.1)
    r = mia.ShardedLetkf(torch.device(DEV), 0, 1, radii=[c], inf_factor=1.1)
    args = (torch.as_tensor(case["state"], dtype=torch.float32, device=DEV), torch.as_tensor(case["grid_x"], device=DEV),
            torch.as_tensor(case["obs_x"], device=DEV), torch.as_tensor(case["yb"], dtype=torch.float32, device=DEV),
            torch.as_tensor(case["d"], dtype=torch.float32, device=DEV))
    r.assimilate(*args)
    opn = r.assimilate(*args).cpu().numpy().astype(np.float64)
    assert np.array_equal(per, opn)


@pytest.mark.parametrize("s", [8, 1037])
def test_rolled_ring_gives_the_rolled_analysis(mia, s):
    G, c = 2048, 10.0
    case = ring_case(G, float(G), 40, 2)
    base = runner_step(mia, case, float(G), c, 1.1)
    rolled = dict(case)
    rolled["state"] = np.roll(case["state"], s, axis=-1)
    rolled["obs_x"] = np.mod(case["obs_x"] + s, G)
    xr = runner_step(mia, rolled, float(G), c, 1.1)
    back = np.roll(xr, -s, axis=-1)
    for g in range(G):
        assert rel_fro(back[:, :, g], base[:, :, g]) <= 1e-6, g


def test_partition_blocks_at_the_seam(mia):
    from torch_assimilate_amd.sharded import block_partition
    G, c = 4096, 10.0
    case = ring_case(G, float(G), 40, 2)
    full = runner_step(mia, case, float(G), c, 1.1)
    for rank in (0, 7):
        g0, g1 = block_partition(G, 8)[rank]
        r = mia.ShardedLetkf(torch.device(DEV), rank, 8, radii=[c], inf_factor=1.1, gather=False, period=[float(G)])
        args = (torch.as_tensor(case["state"], dtype=torch.float32, device=DEV), torch.as_tensor(case["grid_x"], device=DEV),
                torch.as_tensor(case["obs_x"], device=DEV), torch.as_tensor(case["yb"], dtype=torch.float32, device=DEV),
                torch.as_tensor(case["d"], dtype=torch.float32, device=DEV))
        r.assimilate(*args)
        blk = r.assimilate(*args).cpu().numpy().astype(np.float64)
        assert blk.shape == (1, 40, g1 - g0) and r.last_flags_ok()
        assert np.array_equal(blk, full[:, :, g0:g1]), rank


def test_no_host_distance_calls(mia, monkeypatch):
    def boom(self, *a, **k):
        raise AssertionError("host distance call")
    monkeypatch.setattr(mia.PeriodicMetric, "__call__", boom)
    G, L, c = 512, 512.0, 6.0
    case = ring_case(G, L, 20, 2)
    loc = mia.GaspariCohn(c, dist_func=mia.PeriodicMetric(L))
    for dt in (torch.float32, torch.float64):
        f = mia.LETKF(localization=loc, inf_factor=1.1, dtype=dt)
        xa = f.analyse_arrays(case["state"], case["yb"], case["d"], case["grid_x"], case["obs_x"])
        pts = [0, 1, 5, G - 3, G - 1, 200]
        ref = oracle_points(case, L, c, 1.1, pts)
        assert rel_fro(xa.cpu().numpy().astype(np.float64)[:, :, pts], ref) <= 1e-5


def _lists_at(eng, grid, obs, radii, groups, taper, period, cap, quad=True):
    """per-point lists of one route: cap 32 = quad kernel (thread kernel with quad False), cap 64 = wave kernel"""
    from torch_assimilate_amd import _cabi
    old = _cabi.set_option("localize_quad", 1 if quad else 0)
    try:
        nb = eng.localize(grid, obs, radii, groups, taper=taper, period=period, assume_p_max=cap)
        torch.cuda.synchronize()
    finally:
        _cabi.set_option("localize_quad", old)
    assert nb.p_cap == cap
    return nb.cnt.cpu().numpy(), nb.idx.cpu().numpy(), nb.w.cpu().numpy()


def _open_entry_lists(eng, grid, obs, radii, groups, cap):
    """the same through the open C entry (mia_letkf_localize_taper_f64), which the engine no longer calls"""
    import ctypes as C
    from torch_assimilate_amd import _cabi
    lib = _cabi.lib()
    g = torch.as_tensor(grid, dtype=torch.float64, device=DEV).contiguous()
    o = torch.as_tensor(obs, dtype=torch.float64, device=DEV).contiguous()
    G, nc = g.shape
    P = o.shape[0]
    nbytes = C.c_size_t(0)
    assert lib.mia_letkf_localize_workspace_bytes(P, nc, C.byref(nbytes)) == 0
    ws = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=DEV)
    cnt = torch.empty(G, dtype=torch.int32, device=DEV)
    idx = torch.empty((G, cap), dtype=torch.int32, device=DEV)
    w = torch.empty((G, cap), dtype=torch.float64, device=DEV)
    stats = torch.empty(2, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    rc = lib.mia_letkf_localize_taper_f64(0, g.data_ptr(), 0, G, o.data_ptr(), P, nc, (C.c_int32 * nc)(*groups),
                                          (C.c_double * len(radii))(*radii), len(radii), 1e-5, cap, cnt.data_ptr(), idx.data_ptr(),
                                          w.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy()


def _assert_lists_bitwise(a, b, cap):
    """cnt equal; the first cap entries of idx and w equal bit for bit"""
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1][:, :cap], b[1][:, :cap])
    assert np.array_equal(a[2][:, :cap].view(np.int64), b[2][:, :cap].view(np.int64))


OPEN_2D = "open_2d"


@pytest.mark.parametrize("name", GEOMS + [OPEN_2D])
def test_point_lists_bitwise_equal_across_routes(mia, eng, name):
    """Thread, quad and wave kernels give the same per-point lists bit for bit (the wave kernel's cyclic instantiation included);
    on an open geometry the periodic entry with an all-zero period gives what the open entry gives."""
    if name == OPEN_2D:
        rs = np.random.default_rng(7)
        grid, obs, period, radii, groups, taper = (mesh(np.arange(20.0), np.arange(20.0)), rs.uniform(0, 20, (150, 2)), None, [2.0],
                                                   [0, 0], 0)
    else:
        grid, obs, period, radii, groups, taper = geometry(name)
    thread = _lists_at(eng, grid, obs, radii, groups, taper, period, 32, quad=False)
    quad = _lists_at(eng, grid, obs, radii, groups, taper, period, 32)
    wave = _lists_at(eng, grid, obs, radii, groups, taper, period, 64)
    assert thread[0].sum() > 0
    _assert_lists_bitwise(thread, quad, 32)
    _assert_lists_bitwise(quad, wave, 32)
    if name == OPEN_2D:
        for cap, lists in ((32, quad), (64, wave)):
            _assert_lists_bitwise(_open_entry_lists(eng, grid, obs, radii, groups, cap), lists, cap)

"""The dense float64 route under a tile map (csrc/letkf_patch64.hip) without a GPU: mesh_tiles, the host-only cover function and
the argument validation of mia_letkf_analysis_patch_f64 / mia_letkf_tile_union_census, which returns before any HIP call."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def check_map(tiles, ny, nx, g0, g1, py, px):
    """every point of [g0, g1) exactly once, relative to g0; a tile lies in one patch, slot = row-major place inside it; -1
    exactly where the patch leaves the mesh or the shard"""
    t = tiles.numpy()
    assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 16
    live = t[t >= 0]
    assert np.array_equal(np.sort(live), np.arange(g1 - g0))
    assert int(t.min(initial=0)) >= -1
    seen = set()
    for row in t:
        pts = row[row >= 0] + g0
        assert len(pts) > 0                                   # (patches without a point of the shard are left out)
        patch = {(int(p) // nx // py, int(p) % nx // px) for p in pts}
        assert len(patch) == 1
        (ty, tx), = patch
        assert (ty, tx) not in seen
        seen.add((ty, tx))
        for s in range(16):
            y, x = ty * py + s // px, tx * px + s % px
            g = y * nx + x
            inside = y < ny and x < nx and g0 <= g < g1
            assert row[s] == (g - g0 if inside else -1), (ty, tx, s)


@pytest.mark.parametrize("ny,nx,g0,g1", [(13, 11, 0, None), (4, 4, 0, None), (1, 37, 0, None), (13, 11, 37, 120)])
@pytest.mark.parametrize("patch", [(4, 4), (2, 8), (8, 2)])
def test_mesh_tiles(ny, nx, g0, g1, patch):
    import torch_assimilate_amd as mia
    tiles = mia.mesh_tiles((ny, nx), g0, g1, patch=patch)
    check_map(tiles, ny, nx, g0, ny * nx if g1 is None else g1, *patch)


def test_mesh_tiles_defaults_and_faults():
    import torch
    import torch_assimilate_amd as mia
    from torch_assimilate_amd.engine import mesh_tiles
    assert mia.mesh_tiles is mesh_tiles
    t = mesh_tiles((4, 4))
    assert torch.equal(t, torch.arange(16, dtype=torch.int32)[None])
    assert mesh_tiles((13, 11)).shape == (4 * 3, 16)
    assert mesh_tiles((13, 11), 5, 5).shape == (0, 16)
    # tiles follow the patches row by row: the first tile of a 13 x 11 mesh holds rows 0 .. 3 of columns 0 .. 3
    assert mesh_tiles((13, 11))[0].tolist() == [y * 11 + x for y in range(4) for x in range(4)]
    for bad in ((3, 4), (4, 5), (16, 0)):
        with pytest.raises(ValueError):
            mesh_tiles((13, 11), patch=bad)
    with pytest.raises(ValueError):
        mesh_tiles((13, 11), 0, 144)
    with pytest.raises(ValueError):
        mesh_tiles((0, 11))


def test_cover_function_is_the_dense_routes(lib):
    for m in (0, 1, 3, 8):
        for k in (1, 2, 5, 8, 20, 40, 63, 64, 65, 128):
            for p in (0, 1, k - 1, k, k + 1, 45, 101, 224, 225, 256, 257, 3000):
                for ld in (1000, 1 << 23):
                    a = (m, k, p, ld, 1000, 1000, 1000)
                    assert lib.mia_letkf_patch_f64_cover(*a) == lib.mia_letkf_dense_f64_cover(*a), a
    assert lib.mia_letkf_patch_f64_cover(1, 40, 101, 1000, 1000, 1000, 1000) == 1
    assert lib.mia_letkf_patch_f64_cover(1, 40, 101, 1000, 1000, 1000, -1) == 0
    assert lib.mia_letkf_patch_f64_cover(1, 40, 101, 1000, 1000, -1, 1000) == 0


def test_capacity_restated_in_python(lib):
    """LetkfEngine._dense64_capacity_blocks against the cover function, whose largest p_max is sixteen times the capacity"""
    from torch_assimilate_amd.engine import LetkfEngine
    for k in (2, 8, 20, 40, 56, 60, 63, 64):
        cap = LetkfEngine._dense64_capacity_blocks(k)
        assert lib.mia_letkf_patch_f64_cover(1, k, 16 * cap, 1000, 1000, 1000, 1000) == 1
        assert lib.mia_letkf_patch_f64_cover(1, k, 16 * cap + 1, 1000, 1000, 1000, 1000) == 0


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_letkf_analysis_patch_f64
    names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "gamma", "Xa", "ldo",
             "o0", "flags", "retry", "tiles", "n_tiles", "ub", "stream")
    null = (None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None, 1, 1, None)

    def with_(**kw):
        a = dict(zip(names, null))
        a.update(kw)
        return call(*[a[n] for n in names])
    assert with_() == -1                                                    # NULL pointers
    assert with_(inf=-1.0) == -2 and with_(inf=0.0) == -2
    assert with_(k=1) == -2 and with_(m=0) == -2 and with_(g1=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    assert with_(n_tiles=-1) == -2 and with_(ub=0) == -2 and with_(ub=-3) == -2
    assert with_(g1=0) == 0                                                 # empty shard
    assert with_(gamma=0.5) == -3                                           # the float64 RBF filter is not this route's
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(X=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, Xa=ptr, flags=ptr, retry=ptr, tiles=ptr)
    assert with_(**dict(full, tiles=None)) == -1                            # the map is required
    assert with_(ldx=4, **full) == -2 and with_(ldo=4, **full) == -2        # leading dimensions shorter than the shard
    assert with_(n_tiles=0, **full) == -2                                   # no tiles for a non-empty range
    assert with_(p_max=4, **full) == -3                                     # p_max <= k
    assert with_(p_cap=4000, p_max=3000, **full) == -3                      # beyond the record image
    assert with_(k=65, p_cap=200, p_max=100, **full) == -3
    assert with_(ub=17, **full) == -2                                       # above the capacity (inside the cover)
    assert with_(k=64, p_cap=200, p_max=100, ub=15, **full) == -2           # ... which is 14 blocks at k = 64
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                          # the A/B switch of the tile routes
    finally:
        lib.mia_set_option(b"tile", -1)
    # the census entry
    cen = lib.mia_letkf_tile_union_census
    assert cen(ptr, -1, 5, ptr, ptr, 8, 6, 1, ptr, ptr, 512, None) == -2
    assert cen(ptr, 1, -1, ptr, ptr, 8, 6, 1, ptr, ptr, 512, None) == -2
    assert cen(ptr, 1, 5, ptr, ptr, 0, 6, 1, ptr, ptr, 512, None) == -2
    assert cen(ptr, 0, 5, ptr, ptr, 8, 6, 1, ptr, ptr, 512, None) == -2     # points without tiles
    assert cen(None, 1, 5, ptr, ptr, 8, 6, 1, ptr, ptr, 512, None) == -1
    assert cen(ptr, 1, 5, ptr, ptr, 8, 6, 1, None, ptr, 512, None) == -1
    assert cen(ptr, 1, 5, ptr, ptr, 8, 6, 1, ptr, None, 512, None) == -1
    assert cen(ptr, 1, 5, None, ptr, 8, 6, 1, ptr, ptr, 512, None) == -1    # the lists are needed for the count ...
    assert cen(ptr, 1, 5, ptr, ptr, 8, 6, 1, ptr, ptr, 4 * 6, None) == -4   # ws holds n_points + 2 counters
    assert cen(ptr, 1, 5, ptr, ptr, 8, 6, 1, ptr, C.c_void_p(ptr.value + 2), 512, None) == -5

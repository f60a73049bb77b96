"""The float64 IEnKS update of dense local networks under a tile map (csrc/lienks_patch64.hip, mia_lienks_update_patch_f64,
LetkfEngine.ienks_update(method="patch64")) without a GPU: the symbols, the host-only cover function against a Python
restatement, the argument validation of the entry, which returns before any HIP call, the engine method against the recording
stand-in of the C library (call sequence cover -> census -> entry -> counter read; one census per map), the rules by which the
classes take the route, and the entry's launches (instantiation, grid, block, LDS bytes) against a restatement, from a host-only
build with a stand-alone driver.

On a build without this route every test fails: the symbols do not exist, ienks_update knows no method "patch64"."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from host_build import HIPCC, link_driver
from test_engine_route_trace import StandInLib, case, make_engine, F32, F64, RETRY_AT

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
NEW_SYMBOLS = ("mia_lienks_update_patch_f64", "mia_lienks_update_patch_f64_cover")
ENTRY, COVER, CENSUS, REDO = NEW_SYMBOLS[0], NEW_SYMBOLS[1], "mia_letkf_tile_union_census", "mia_lienks_update_retry_f64"


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def lds_bytes(k, ub):
    """LDS of a launch, restated from ring64_lds_bytes (csrc/mia_frames64.h) with the caller's blocks: ring [2][16][kp | 1],
    rhs [4 KT][64] and the sqrt(rho) table [16][16 ub + 1] in doubles, the slot table [16 ub] in ints"""
    umax, kp, kt = 16 * ub, (k + 1 + 3) & ~3, (k + 15) >> 4
    return ((2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (umax + 1)) * 8 + umax * 4 + 15) // 16 * 16


def covers(k, p_max, n_points, P):
    if P < 0 or n_points < 0 or k < 2 or k > 128 or p_max <= k or p_max > 256:
        return 0
    return int(k * k * 8 < 2 ** 31 and n_points < 2 ** 31 and lds_bytes(k, 16) <= MAX_LDS)


def test_symbols_are_declared_exported_and_bound(lib):
    from torch_assimilate_amd import _build, _cabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mia_letkf.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    declared = sorted(set(re.findall(r"\b(mia_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert sorted(_cabi.EXPORTED_SYMBOLS) == declared                      # EXPORTED_SYMBOLS matches the header
    # mia_lienks_update_stream_f64's argument list with (tile_pts, n_tiles, union_blocks) in front of the stream, as
    # mia_letkf_weights_patch_f64 has them
    base, twin = lib.mia_lienks_update_stream_f64.argtypes, lib.mia_letkf_weights_patch_f64.argtypes
    assert list(lib.mia_lienks_update_patch_f64.argtypes) == list(base[:-1]) + list(twin[-4:])
    assert lib.mia_lienks_update_patch_f64_cover.argtypes == lib.mia_lienks_update_stream_f64_cover.argtypes
    assert "lienks_patch64.hip" in _build.SOURCES and "mia_lienks_stream64_dev.h" in _build.HEADERS
    comment = header[header.index("csrc/lienks_patch64.hip"):header.index("int mia_lienks_update_patch_f64(")]
    for word in ("n_tiles < 0", "tile_pts among them", "n_tiles == 0", "union_blocks outside", "more tiles than a launch grid"):
        assert word in re.sub(r"\s*\n \* ", " ", comment), word                # the validation order is written down


def test_cover_function_vs_restatement(lib):
    cover = lib.mia_lienks_update_patch_f64_cover
    # 1 everywhere inside 2 <= k <= 128, k < p_max <= 256: the LDS of the largest image never refuses a shape
    for k in range(2, 129):
        assert lds_bytes(k, 16) <= MAX_LDS
        for p in range(k + 1, 257):
            assert cover(k, p, 1000, 1000) == 1, (k, p)
    assert max(lds_bytes(k, 16) for k in range(2, 129)) == lds_bytes(128, 16) == 84352
    for k, p in ((40, 101), (64, 101), (80, 101), (96, 101), (128, 145), (128, 185)):      # the shapes it is for
        assert cover(k, p, 100000, 100000) == 1, (k, p)
    for k in (2, 40, 64, 65, 80, 128):
        assert cover(k, k, 1000, 10) == 0 and cover(k, k + 1, 1000, 10) == 1 and cover(k, 256, 1000, 10) == 1, k
        assert cover(k, 257, 1000, 10) == 0 and cover(k, 0, 1000, 10) == 0 and cover(k, -1, 1000, 10) == 0, k
    assert cover(1, 2, 1000, 10) == 0 and cover(129, 139, 1000, 10) == 0 and cover(129, 256, 1000, 10) == 0
    for k in (0, 1, 2, 3, 16, 17, 63, 64, 65, 96, 127, 128, 129, 200):
        for p in (-1, 0, 1, k - 1, k, k + 1, 64, 65, 128, 129, 255, 256, 257, 1000):
            assert cover(k, p, 1000, 1000) == covers(k, p, 1000, 1000), (k, p)
            assert cover(k, p, 1000, 1000) == lib.mia_letkf_weights_patch_f64_cover(k, p, 1000, 1000), (k, p)     # the twin's arithmetic
    assert cover(80, 101, 0, 0) == 1 and cover(80, 101, -1, 0) == 0 and cover(80, 101, 1000, -1) == 0
    for n in (1, 15, 16, 17, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 40):
        assert cover(80, 101, n, 10) == covers(80, 101, n, 10), n
    assert cover(80, 101, (1 << 31) - 1, 10) == 1 and cover(80, 101, 1 << 31, 10) == 0
    # the parent keeps its answers
    assert lib.mia_lienks_update_stream_f64_cover(80, 101, 1 << 31, 10) == 1
    assert lib.mia_lienks_update_stream_f64_cover(128, 128, 1000, 10) == 0
    assert lib.mia_lienks_update_stream_f64_cover(80, 101, 16 * 65536 * 65535 + 1, 10) == 0


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_lienks_update_patch_f64
    names = ("W_in", "w_stride", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "eps", "W_out", "flags", "retry",
             "tiles", "n_tiles", "ub", "stream")
    null = (None, 0, 80, 0, 5, None, 0, None, None, None, 200, 101, 0.01, None, None, None, None, 1, 4, None)

    def with_(**kw):
        a = dict(zip(names, null))
        a.update(kw)
        return call(*[a[n] for n in names])

    def parent(**kw):
        a = dict(zip(names, null))
        a.update(kw)
        return lib.mia_lienks_update_stream_f64(*[a[n] for n in names if n not in ("tiles", "n_tiles", "ub")])
    # the one order of the IEnKS tile entries: sizes, the weight stride, empty shard, NULL pointers
    assert with_(k=1) == -2 and with_(g1=-1) == -2 and with_(g0=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    assert with_(p_max=-1) == -2
    assert with_(n_tiles=-1) == -2                                          # the map's size among the sizes
    assert with_(w_stride=5) == -2 and with_(w_stride=6400) == -1           # the stride: 0 or k * k
    assert with_(g1=0) == 0 and with_(g1=0, n_tiles=0) == 0                 # empty shard
    assert with_(w_stride=5, g1=0) == -2 and with_(n_tiles=-1, g1=0) == -2
    assert with_() == -1                                                    # NULL pointers
    for kw in (dict(), dict(k=1), dict(g1=0), dict(w_stride=5), dict(P=-1), dict(w_stride=5, g1=0), dict(p_cap=0)):
        assert with_(**kw) == parent(**kw), kw
    # with the required pointers present: the map, sizes, then option and cover (nothing is dereferenced before them)
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(W_in=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, W_out=ptr, flags=ptr, retry=ptr, tiles=ptr)
    for missing in ("W_in", "cnt", "idx", "w", "W_out", "flags", "retry", "tiles"):
        assert with_(**dict(full, **{missing: None})) == -1, missing
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    assert with_(n_tiles=0, **full) == -2                                   # no tiles for a non-empty range
    assert with_(n_tiles=0, **dict(full, tiles=None)) == -1                 # ... behind the pointers
    assert with_(p_max=80, **full) == -3 and with_(p_max=63, **full) == -3  # p_max <= k: the dual routes'
    assert with_(p_cap=64, **full) == -3                                    # ... also after p_max is cut to p_cap
    assert with_(k=129, p_max=140, **full) == -3                            # ensemble size
    assert with_(p_cap=300, p_max=257, **full) == -3                        # more than 256 slots
    for ub in (0, -3, 17, 1000):
        assert with_(ub=ub, **full) == -3, ub                               # union_blocks outside 1 .. 16
    assert with_(n_tiles=65536 * 65535 + 1, **full) == -3                   # more tiles than a launch grid
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                          # the A/B switch of the tile routes
        assert with_(k=128, p_max=145, ub=16, **full) == -3
    finally:
        lib.mia_set_option(b"tile", -1)
    lib.mia_set_option(b"cheb_table", 0)
    try:
        assert with_(**full) == -3                                          # no coefficient table
    finally:
        lib.mia_set_option(b"cheb_table", -1)


# ---- the engine method against the recording stand-in -----------------------------------------------------------------------------
def names_of(trace):
    return [line.split("(")[0] for line in trace if not line.startswith("#")]


def scenario(k=80, p_max=101, n=37, union=176, weights="points"):
    lib = StandInLib()
    eng = make_engine(lib)
    t = case(F64, 1, k, p_max, n=n, weights=weights)
    tiles = torch.full(((n + 15) // 16, 16), -1, dtype=torch.int32)
    tiles.reshape(-1)[:n] = torch.arange(n, dtype=torch.int32)
    t["tiles"] = tiles
    lib.begin("ienks_update patch64", t, census=(0, union))
    return lib, eng, t


def update(eng, t, **kw):
    return eng.ienks_update(t["weights"], None, None, t["nbrs"], 1.0, kw.pop("epsilon", 0.5), rec=t["rec"],
                            method=kw.pop("method", "patch64"), tile_points=kw.pop("tiles", t["tiles"]), **kw)


def test_the_engine_calls_cover_census_entry_and_reads_the_counter(monkeypatch):
    from torch_assimilate_amd import _cabi
    assert ENTRY not in RETRY_AT                 # (the stand-in does not know this entry: no decline is deposited, the counter stays 0)
    lib, eng, t = scenario()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    out = torch.zeros((37, 80, 80), dtype=F64)
    res = update(eng, t, out=out, return_flags=True)
    assert isinstance(res, tuple) and len(res) == 2 and res[0] is out and res[1].shape == (37,)
    assert names_of(lib.trace) == [COVER, CENSUS, ENTRY]                    # ... and the counter (0) is read on the host: no redo
    cover, census, entry = [line for line in lib.trace if not line.startswith("#")]
    assert cover == "%s(80, 101, 37, 6) = 1" % COVER
    assert census.startswith(CENSUS + "(tiles, 3, 37, cnt, idx, %d, 101, 1, " % t["nbrs"].p_cap)
    # the entry: per-point weights (stride k * k), the shard, epsilon, W_out, flags, the counter, then the map, its tiles,
    # ceil(176 / 16) blocks, the stream
    assert entry.startswith(ENTRY + "(weights, 6400, 80, 2, 39, rec, 6, cnt, idx, w, %d, 101, 0.5, " % t["nbrs"].p_cap)
    assert entry.endswith(", tiles, 3, 11, NULL) = 0")
    ent = t["nbrs"].tile_census[id(t["tiles"])]
    assert ent[0] is t["tiles"] and ent[2] == 176
    # a second call with the same map: no second census; a deferred redo reads the counter when it is invoked
    del lib.trace[:]
    W, finish = update(eng, t, out=out, defer_retry=True)
    assert names_of(lib.trace) == [COVER, ENTRY] and t["nbrs"].tile_census[id(t["tiles"])] is ent
    assert W is out and finish() == 0 and names_of(lib.trace) == [COVER, ENTRY]
    # one shared matrix in the transform variant: stride 0, epsilon 0
    lib1, eng1, t1 = scenario(weights="shared")
    monkeypatch.setattr(_cabi, "lib", lambda: lib1)
    update(eng1, t1, epsilon=None)
    assert lib1.trace[-1].startswith(ENTRY + "(weights, 0, 80, 2, 39, rec, 6, cnt, idx, w, %d, 101, 0.0, " % t1["nbrs"].p_cap)
    # ... also after an ANALYSIS and a WEIGHTS call with the same lists and map have paid for it (one census for all three)
    lib2, eng2, t2 = scenario(k=40, union=150)
    monkeypatch.setattr(_cabi, "lib", lambda: lib2)
    eng2.analysis(t2["X"], None, None, t2["nbrs"], 1.1, rec=t2["rec"], method="patch64", tile_points=t2["tiles"])
    assert eng2.weights_patch64(None, None, t2["nbrs"], t2["tiles"], 1.1, rec=t2["rec"], out=torch.zeros((37, 40, 40), dtype=F64)) is not None
    assert names_of(lib2.trace).count(CENSUS) == 1
    del lib2.trace[:]
    update(eng2, t2)
    assert names_of(lib2.trace) == [COVER, ENTRY] and lib2.trace[-1].endswith(", tiles, 3, 10, NULL) = 0")
    # a named union_blocks is passed on; a new map is validated without the count
    del lib2.trace[:]
    update(eng2, t2, tiles=t2["tiles"].clone(), union_blocks=7)
    assert names_of(lib2.trace) == [COVER, CENSUS, ENTRY] and lib2.trace[-1].endswith(", 3, 7, NULL) = 0")
    assert ", 101, 0, " in lib2.trace[1]
    # and the census of THIS method serves weights_patch64
    lib3, eng3, t3 = scenario()
    monkeypatch.setattr(_cabi, "lib", lambda: lib3)
    update(eng3, t3)
    del lib3.trace[:]
    eng3.weights_patch64(None, None, t3["nbrs"], t3["tiles"], 1.1, rec=t3["rec"], out=torch.zeros((37, 80, 80), dtype=F64))
    assert CENSUS not in names_of(lib3.trace)


def test_declined_points_are_redone_behind_the_counter(monkeypatch):
    from torch_assimilate_amd import _cabi
    lib, eng, t = scenario()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    monkeypatch.setitem(RETRY_AT, ENTRY, -5)     # (the counter's place in this entry's list: the stand-in deposits the declines)
    lib.declines = 3
    out = torch.zeros((37, 80, 80), dtype=F64)
    W, finish = update(eng, t, out=out, defer_retry=True)
    assert names_of(lib.trace) == [COVER, CENSUS, ENTRY]
    assert finish() == 3
    assert names_of(lib.trace) == [COVER, CENSUS, ENTRY, REDO]
    # the redo takes the lists in natural order: the general kernel's arguments (tau = 1), no map
    assert lib.trace[-1].startswith(REDO + "(weights, 6400, 80, 2, 39, rec, 6, cnt, idx, w, %d, 101, 1.0, 0.5, " % t["nbrs"].p_cap)
    assert "tiles" not in lib.trace[-1]
    # without defer_retry the redo is part of the call
    del lib.trace[:]
    update(eng, t, out=out)
    assert names_of(lib.trace) == [COVER, ENTRY, REDO]
    # the redo raises where the general kernel cannot hold the shape: AFTER the tile entry has run
    lib.rc[REDO] = -3
    W, finish = update(eng, t, out=out, defer_retry=True)
    with pytest.raises(_cabi.MiaError, match="status -3"):
        finish()


def test_bad_arguments_raise_before_any_call(monkeypatch):
    from torch_assimilate_amd import _cabi
    lib, eng, t = scenario()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    good = t["tiles"]
    for bad in (good.to(torch.int64), good.reshape(-1), good[:, :8], good.tolist()):
        with pytest.raises(ValueError, match="tile_points"):
            update(eng, t, tiles=bad)
    with pytest.raises(ValueError, match=r"the patch64 route needs tile_points \(see mesh_tiles\)"):
        update(eng, t, tiles=None)
    for ub in (0, -1, 17, 100):
        with pytest.raises(ValueError, match="union_blocks"):
            update(eng, t, union_blocks=ub)
    for method in ("auto", "eig", "tile64", "wide64", "stream64"):
        with pytest.raises(ValueError, match="patch64"):
            update(eng, t, method=method)
        with pytest.raises(ValueError, match="patch64"):
            update(eng, t, method=method, tiles=None, union_blocks=4)
    with pytest.raises(ValueError, match="float64"):
        eng.ienks_update(t["weights"].to(F32), None, None, t["nbrs"], 1.0, 0.5, rec=t["rec"].to(F32), method="patch64", tile_points=good)
    with pytest.raises(ValueError, match="tau"):
        eng.ienks_update(t["weights"], None, None, t["nbrs"], 0.5, 0.5, rec=t["rec"], method="patch64", tile_points=good)
    assert names_of(lib.trace) == []
    # an invalid map: ValueError from the census' answer, before the entry
    lib.census = (2, 0)
    with pytest.raises(ValueError, match="more than once"):
        update(eng, t)
    assert names_of(lib.trace) == [COVER, CENSUS]
    # outside the cover and MIA_ERR_UNSUPPORTED from the entry: ValueError, as the other named tile methods
    lib.census = (0, 176)
    del lib.trace[:]
    lib.rc[COVER] = 0
    with pytest.raises(ValueError, match="covers 2 <= k <= 128 and k < p_max <= 256"):
        update(eng, t)
    assert names_of(lib.trace) == [COVER]
    lib.rc = {ENTRY: -3}
    with pytest.raises(ValueError, match="not available"):
        update(eng, t)
    # the other methods launch what they launched before: no map argument reaches their entries
    del lib.trace[:]
    eng.ienks_update(t["weights"], None, None, t["nbrs"], 1.0, 0.5, rec=t["rec"], method="stream64")
    assert names_of(lib.trace) == ["mia_lienks_update_stream_f64_cover", "mia_lienks_update_stream_f64"]
    assert lib.trace[-1].endswith(", NULL) = 0") and "tiles" not in lib.trace[-1]


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def test_the_class_rule():
    """LetkfEngine._ienks_patch64_auto: the map wherever _ienks_stream64_auto says yes, never outside the kernel's cover, never for
    per-point transform weights, and where the general kernel is the default only inside the measured constants."""
    import torch_assimilate_amd as mia
    E = mia.LetkfEngine
    eng = E.__new__(E)                           # (the rule reads class constants only: no device)
    assert "patch64" in E.IENKS_TILE64_ROUTES and E.IENKS_TILE64_ROUTES["patch64"][3] is None      # never under "auto" at engine level
    assert E.IENKS_TILE64_ROUTES["patch64"][:2] == NEW_SYMBOLS
    for k in range(2, 131):
        for p in range(0, 259):
            for bundle, shared in ((True, False), (True, True), (False, True), (False, False)):
                auto = eng._ienks_patch64_auto(k, p, bundle, shared)
                if covers(k, p, 1000, 1000) != 1 or not (bundle or shared):
                    assert not auto, (k, p, bundle, shared)
                elif eng._ienks_stream64_auto(k, p, bundle, shared):
                    assert auto, (k, p, bundle, shared)          # (no measured shape of that range is excluded)
                else:
                    assert E._ienks_general_fits(k, p, 1.0, bundle)
                    assert auto == (E.IENKS_PATCH64_AUTO_MIN_K <= k <= E.IENKS_PATCH64_AUTO_MAX_K and
                                    E.IENKS_PATCH64_AUTO_DEN * p <= E.IENKS_PATCH64_AUTO_NUM * k), (k, p, bundle, shared)
    assert eng._ienks_patch64_auto(128, 145, True, False) and eng._ienks_patch64_auto(96, 101, True, False)
    assert eng._ienks_patch64_auto(80, 101, False, True) and not eng._ienks_patch64_auto(80, 101, False, False)
    assert not eng._ienks_patch64_auto(128, 128, True, False) and not eng._ienks_patch64_auto(128, 257, True, False)


def test_the_classes_hand_over_exactly_where_the_rule_and_the_cover_say(monkeypatch):
    """LocalizedIEnKSBundle / LocalizedIEnKSTransform.inner_loop_arrays against the stand-in: method="patch64" with the shard's map
    where a grid is given, the dtype is float64, tau = 1 and the rule with the cover says yes; what _ienks_method returns
    otherwise.  A mesh_shape of another size warns and is ignored; float32 never looks at it."""
    import warnings
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi, ienks
    seen = {}

    class Eng:
        lib = StandInLib()
        device = torch.device("cpu")
        _ienks_patch64_auto = mia.LetkfEngine._ienks_patch64_auto
        _ienks_stream64_auto = mia.LetkfEngine._ienks_stream64_auto
        _ienks_general_fits = staticmethod(mia.LetkfEngine._ienks_general_fits)
        _ienks_general_lds_bytes = staticmethod(mia.LetkfEngine._ienks_general_lds_bytes)
        for name in dir(mia.LetkfEngine):
            if name.startswith("IENKS_") or name == "JACOBI_MAX_LDS":
                locals()[name] = getattr(mia.LetkfEngine, name)

        def ienks_update(self, w, yb, d, nb, tau, eps, method="auto", tile_points=None):
            seen.update(method=method, tiles=tile_points)
            return w

    def run(cls, k, p_max, shared, dtype=F64, tau=1.0, mesh=(5, 8), grid=40, cover=1):
        eng = Eng()
        eng.lib.rc = {COVER: cover}
        kw = dict(epsilon=0.5) if cls is mia.LocalizedIEnKSBundle else {}
        a = cls(lambda x, it: (x, x), None, tau=tau, dtype=dtype, engine=eng, mesh_shape=mesh, **kw)
        nb = case(F64, 1, 4, p_max, n=grid)["nbrs"]
        nb.g0, nb.g1 = 0, grid
        monkeypatch.setattr(a, "_lists", lambda *args: nb)
        monkeypatch.setattr(a, "_dev", lambda x: x)
        seen.clear()
        a.inner_loop_arrays(torch.zeros((k, k) if shared else (grid, k, k), dtype=dtype), None, None, grid_coords=list(range(grid)),
                            obs_coords=[0.0])
        return seen["method"], seen["tiles"]

    E = mia.LetkfEngine
    rule = E.__new__(E)
    for cls, bundle in ((mia.LocalizedIEnKSBundle, True), (mia.LocalizedIEnKSTransform, False)):
        for k in (8, 40, 64, 65, 72, 80, 96, 128):
            for p_max in (k, k + 1, k + 12, 145, 256):
                for shared in (True, False):
                    method, tiles = run(cls, k, p_max, shared)
                    want = rule._ienks_patch64_auto(k, min(p_max, case(F64, 1, 4, p_max)["nbrs"].p_cap), bundle, shared)
                    assert (method == "patch64") == want, (cls.__name__, k, p_max, shared, method)
                    if want:
                        assert tiles is not None and tiles.shape == (4, 16) and tiles.dtype == torch.int32
                        assert sorted(tiles[tiles >= 0].tolist()) == list(range(40))
                    else:
                        assert tiles is None and method in ("auto", "stream64")
    assert run(mia.LocalizedIEnKSBundle, 128, 145, False) == ("patch64", seen["tiles"])
    # the cover says no, tau < 1, float32, no mesh_shape: the old route
    assert run(mia.LocalizedIEnKSBundle, 128, 145, False, cover=0)[0] != "patch64"
    assert run(mia.LocalizedIEnKSBundle, 128, 145, False, tau=0.5) == ("auto", None)
    assert run(mia.LocalizedIEnKSBundle, 128, 145, False, mesh=None) == ("stream64", None)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*mesh_shape.*")
        assert run(mia.LocalizedIEnKSBundle, 128, 145, False, dtype=F32, mesh=(5, 9)) == ("auto", None)
    with pytest.warns(RuntimeWarning, match="mesh_shape"):
        assert run(mia.LocalizedIEnKSBundle, 128, 145, False, mesh=(5, 9)) == ("stream64", None)
    # the unlocalised drivers keep their signatures
    import inspect
    for cls in (mia.IEnKSTransform, mia.IEnKSBundle):
        assert "mesh_shape" not in inspect.signature(cls.__init__).parameters
    for cls in (mia.LocalizedIEnKSTransform, mia.LocalizedIEnKSBundle):
        assert inspect.signature(cls.__init__).parameters["mesh_shape"].default is None and "mesh_shape" in cls.__doc__


# ---- the launches, from a host-only build ----------------------------------------------------------------------------------------------
def test_the_entry_launches_the_instantiation_grid_block_and_lds_of_the_restatement(tmp_path):
    assert os.path.exists(HIPCC), "hipcc not found: the library cannot be built here either, and the launches must not go unchecked"
    exe = link_driver(str(tmp_path), "ienks_patch_launch_driver")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIA_")}
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    calls, cur = [], None
    for line in res.stdout.splitlines():
        if line.startswith("# "):
            cur = dict(head=dict((f.split("=")[0], int(f.split("=")[1])) for f in line[2:].split()), lines=[])
            calls.append(cur)
        else:
            cur["lines"].append(line)
    seen = set()
    for c in calls:
        h = c["head"]
        k, nt, ub = h["k"], h["n_tiles"], h["union_blocks"]
        kt = (k + 15) // 16
        if nt > 65536 * 65535:
            assert c["lines"][-1].startswith("= -3 "), c
            assert not any(l.startswith("launch") for l in c["lines"]), c
            continue
        gx = min(nt, 65536)
        gy = (nt + gx - 1) // gx
        want = "launch mia::lienks_patch64_kernel<%d> grid %d %d 1 block 64 1 1 lds %d stream 0x1000" % (kt, gx, gy, lds_bytes(k, ub))
        launches = [l for l in c["lines"] if l.startswith("launch")]
        if c is calls[0]:                                    # (the first call of a process also builds the coefficient table)
            assert len(launches) == 2 and "cheb_table64_kernel" in launches[0], launches
            launches = launches[1:]
        assert launches == [want], (h, launches)
        assert c["lines"][-1] == '= 0 "lienks_patch64_kernel<%d>"' % kt, c
        for l in c["lines"]:                                 # an attribute line, where the LDS exceeds the default limit, names the same bytes
            if "hipFuncSetAttribute" in l:
                assert "lienks_patch64_kernel<%d>" % kt in l and str(lds_bytes(k, ub)) in l, l
        seen.add((kt, ub))
    assert {kt for kt, _ in seen} == set(range(1, 9))        # k = 2 and every multiple of 16 up to 128: the eight instantiations
    assert {(kt, ub) for kt in range(1, 9) for ub in (1, 16)} <= seen
    heads = [c["head"]["n_tiles"] for c in calls if c["head"]["k"] == 16 and c["head"]["p_max"] == 40]
    assert heads == [1, 65536, 65537, 65536 * 65535, 65536 * 65535 + 1]

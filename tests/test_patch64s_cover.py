"""The streamed dense float64 analysis under a tile map (csrc/letkf_patch64s.hip) without a GPU: the symbols, the host-only cover
function, the argument validation of mia_letkf_analysis_patch_stream_f64 (which returns before any HIP call), what
LetkfEngine.analysis(method="patch64s") calls -- against the stand-in C library of tests/test_engine_route_trace.py -- and the gate
in front of it in LETKF(mesh_shape=...).analyse_arrays, against a stand-in engine.

Run against a build without this route every test fails: the symbols, the method and the gate do not exist."""
import ctypes as C
import os
import re

import pytest
import torch

from test_engine_route_trace import StandInLib, case, make_engine, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, COVER = "mia_letkf_analysis_patch_stream_f64", "mia_letkf_patch_stream_f64_cover"
CENSUS = "mia_letkf_tile_union_census"
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


# ---- symbols ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_built(lib):
    from torch_assimilate_amd import _build, _cabi
    with open(os.path.join(ROOT, "include", "mia_letkf.h")) as fh:
        header = fh.read()
    declared = sorted(set(re.findall(r"\b(mia_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    for name in (ENTRY, COVER):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    assert sorted(_cabi.EXPORTED_SYMBOLS) == declared                      # EXPORTED_SYMBOLS matches the header
    assert "letkf_patch64s.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "letkf_patch64s.hip"))
    # the argument list is mia_letkf_analysis_patch_f64's
    assert _cabi._PROTOS[ENTRY] == _cabi._PROTOS["mia_letkf_analysis_patch_f64"]
    assert _cabi._PROTOS[COVER] == _cabi._PROTOS["mia_letkf_stream_f64_cover"]


# ---- the cover ------------------------------------------------------------------------------------------------------------------------
def test_cover_function_is_the_streamed_routes(lib):
    n = 0
    for m in (0, 1, 3, 8):
        for k in (1, 2, 5, 8, 20, 40, 63, 64, 65, 96, 128, 129):
            for p in (0, 1, k - 1, k, k + 1, 45, 101, 224, 225, 256, 257, 3000):
                for ld in (1000, 1 << 23):
                    a = (m, k, p, ld, 1000, 1000, 1000)
                    assert lib.mia_letkf_patch_stream_f64_cover(*a) == lib.mia_letkf_stream_f64_cover(*a), a
                    n += lib.mia_letkf_patch_stream_f64_cover(*a)
    assert n > 0
    for a in ((1, 80, 101, 1000, 1000, 1000, 1000), (1, 65, 100, 1000, 1000, 1000, 1000), (8, 128, 256, 1000, 1000, 1000, 1000),
              (1, 128, 256, (1 << 21) - 1, 1000, 1000, 1000)):
        assert lib.mia_letkf_patch_stream_f64_cover(*a) == 1, a
    for a in ((1, 129, 200, 1000, 1000, 1000, 1000), (1, 80, 80, 1000, 1000, 1000, 1000), (1, 80, 257, 1000, 1000, 1000, 1000),
              (1, 128, 256, 1 << 21, 1000, 1000, 1000), (1, 128, 256, 1000, 1 << 21, 1000, 1000),       # k ld 8 < 2^31, both leading dimensions
              (1, 80, 101, 1000, 1000, 1000, -1), (1, 80, 101, 1000, 1000, -1, 1000),
              (1, 80, 101, 1000, 1000, 16 * 65536 * 65535 + 1, 1000)):                                   # the grid bound on tiles
        assert lib.mia_letkf_patch_stream_f64_cover(*a) == 0, a
        assert lib.mia_letkf_stream_f64_cover(*a) == 0, a


# ---- validation ----------------------------------------------------------------------------------------------------------------------
def test_argument_validation_precedes_any_device_work(lib):
    call = getattr(lib, ENTRY)
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
    assert with_(p_cap=4000, p_max=3000, **full) == -3                      # beyond 256 slots
    assert with_(k=129, p_cap=200, p_max=150, **full) == -3                 # beyond 128 members
    assert with_(ub=17, **full) == -2                                       # above sixteen blocks (inside the cover)
    for k in (64, 65, 128):                                                 # ... at every ensemble size; k = 65 / p_max 100 is inside
        assert with_(k=k, p_cap=200, p_max=k + 35, ub=17, **full) == -2
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                          # the A/B switch of the tile routes
        assert with_(k=65, p_cap=200, p_max=100, ub=16, **full) == -3
    finally:
        lib.mia_set_option(b"tile", -1)


# ---- the engine against the stand-in library ------------------------------------------------------------------------------------------
def tile_map(n=5):
    tiles = torch.full((1, 16), -1, dtype=torch.int32)
    tiles[0, :n] = torch.arange(n, dtype=torch.int32)
    return tiles


def engine_call(monkeypatch, label, rc=None, census=(0, 40), m=1, k=80, p_max=100, **kw):
    """One LetkfEngine.analysis call on the stand-in library: the trace lines of the call (C calls, result or exception)"""
    from torch_assimilate_amd import _cabi
    lib = StandInLib()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    eng = make_engine(lib)
    t = case(F64, m, k, p_max)
    if "tile_points" in kw:
        t["tile_points"] = kw["tile_points"]
    lib.begin(label, t, rc, 0, census)
    run(lib, lambda: eng.analysis(t["X"], None, None, t["nbrs"], 1.1, rec=t["rec"], **kw))
    return lib.trace[1:]


def names(trace):
    return [l.split("(")[0] for l in trace if l.startswith("mia_")]


def test_the_named_method_calls_cover_census_entry(monkeypatch):
    tr = engine_call(monkeypatch, "patch64s", method="patch64s", tile_points=tile_map())
    assert names(tr) == [COVER, CENSUS, ENTRY], tr
    assert tr[0] == COVER + "(1, 80, 100, 9, 5, 5, 6) = 1"
    # the census counts (count_unions = 1) and its 40 observations size the slot tables: 3 blocks; (tile_pts, n_tiles, ub) stand
    # in front of the stream
    assert tr[1].startswith(CENSUS + "(tile_points, 1, 5, cnt, idx, 104, 100, 1, ")
    assert tr[2].startswith(ENTRY + "(X, 9, 1, 80, 2, 7, rec, 6, cnt, idx, w, 104, 100, 1.1, 0.0, ") and tr[2].endswith(
        ", tile_points, 1, 3, NULL) = 0"), tr[2]
    assert tr[3].startswith("-> Tensor(1, 80, 5) float64")
    # named blocks leave the count, not the validation
    tr = engine_call(monkeypatch, "patch64s ub", method="patch64s", tile_points=tile_map(), union_blocks=16)
    assert names(tr) == [COVER, CENSUS, ENTRY] and ", 104, 100, 0, " in tr[1] and tr[2].endswith(", 1, 16, NULL) = 0")
    # a union above 256 slots: the method is named, so the tiles run in parts on the largest tables
    tr = engine_call(monkeypatch, "patch64s large unions", method="patch64s", tile_points=tile_map(), census=(0, 300))
    assert names(tr) == [COVER, CENSUS, ENTRY] and tr[2].endswith(", 1, 16, NULL) = 0")
    # declined points: the redo entry of every float64 tile route, from the lists in natural order
    from torch_assimilate_amd import _cabi
    import test_engine_route_trace as T
    monkeypatch.setitem(T.RETRY_AT, ENTRY, -5)
    lib = StandInLib()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    eng = make_engine(lib)
    t = case(F64, 1, 80, 100)
    lib.begin("declines", t, None, 3, (0, 40))
    run(lib, lambda: eng.analysis(t["X"], None, None, t["nbrs"], 1.1, rec=t["rec"], method="patch64s", tile_points=tile_map(),
                                  defer_retry=True, return_flags=True))
    assert names(lib.trace[1:]) == [COVER, CENSUS, ENTRY, "mia_letkf_analysis_retry_f64"], lib.trace
    assert lib.trace[-1] == "finish() -> 3"


def test_the_named_method_outside_its_cover_and_its_errors(monkeypatch):
    tr = engine_call(monkeypatch, "cover no", method="patch64s", tile_points=tile_map(), rc={COVER: 0})
    assert names(tr) == [COVER] and tr[-1].startswith("!! MiaError") and ENTRY in tr[-1] and "-3" in tr[-1]
    tr = engine_call(monkeypatch, "entry outside", method="patch64s", tile_points=tile_map(), rc={ENTRY: -3})
    assert names(tr) == [COVER, CENSUS, ENTRY] and tr[-1].startswith("!! MiaError")          # a named route raises, no Jacobi kernel
    tr = engine_call(monkeypatch, "entry error", method="patch64s", tile_points=tile_map(), rc={ENTRY: -2})
    assert names(tr) == [COVER, CENSUS, ENTRY] and tr[-1].startswith("!! MiaError")
    tr = engine_call(monkeypatch, "no map", method="patch64s")
    assert tr == ["!! ValueError: the patch64s route needs tile_points (see mesh_tiles)"]
    for bad in (tile_map().to(torch.int64), tile_map().reshape(-1), tile_map()[:, :8]):
        tr = engine_call(monkeypatch, "map of a wrong type or shape", method="patch64s", tile_points=bad)
        assert names(tr) == [COVER] and tr[-1] == "!! ValueError: tile_points must be an int32 tensor (n_tiles, 16)", tr
    for ub in (0, 17, -1):
        tr = engine_call(monkeypatch, "union_blocks", method="patch64s", tile_points=tile_map(), union_blocks=ub)
        assert names(tr) == [COVER] and tr[-1].startswith("!! ValueError: union_blocks must lie in 1 .. 16"), tr
    tr = engine_call(monkeypatch, "invalid map", method="patch64s", tile_points=tile_map(), census=(6, 0))
    assert names(tr) == [COVER, CENSUS] and tr[-1].startswith("!! ValueError: invalid tile map: ")
    tr = engine_call(monkeypatch, "empty map", method="patch64s", tile_points=tile_map()[:0])
    assert names(tr) == [COVER] and tr[-1].startswith("!! ValueError: invalid tile map: ")
    for kw in (dict(rbf_gamma=0.5), dict(return_weights=True)):
        tr = engine_call(monkeypatch, "not the plain core", method="patch64s", tile_points=tile_map(), **kw)
        assert tr == ["!! ValueError: the patch64s route needs float64, the plain ETKF core and cannot return the weights"], tr


def test_auto_never_takes_the_route_and_the_messages_are_what_they_were(monkeypatch):
    from torch_assimilate_amd.engine import LetkfEngine
    import test_engine_route_trace as T
    # k 80 / p_max 100 lies inside every rule: with a map and every entry declining, "auto" walks the five entries it walked
    tr = engine_call(monkeypatch, "auto with a map", tile_points=tile_map(), rc=T.ALL_DECLINE)
    assert ENTRY not in names(tr) and COVER not in names(tr)
    assert [n for n in names(tr) if n in T.TILE64] == list(T.TILE64)
    tr = engine_call(monkeypatch, "auto with a map, taken by stream64", tile_points=tile_map(), rc={n: -3 for n in T.TILE64[:4]})
    assert names(tr)[-1] == "mia_letkf_analysis_stream_f64" and ENTRY not in names(tr)
    tr = engine_call(monkeypatch, "bad method", method="jacobi")
    assert tr == ["!! ValueError: method must be one of 'auto', 'eig', 'matfun', 'matfun64', 'dense64', 'patch64', 'wide64', "
                  "'stream64', 'rbf64', 'kern64'"] or "patch64s" not in tr[0], tr
    assert "patch64s" not in tr[0]
    assert "patch64s" not in LetkfEngine.ANALYSIS_METHODS and "patch64s" not in LetkfEngine.TILE64_METHODS
    tr = engine_call(monkeypatch, "patch64 without a map", method="patch64")
    assert tr == ["!! ValueError: the patch64 route needs tile_points (see mesh_tiles)"]


# ---- the rule and the class gate --------------------------------------------------------------------------------------------------
def test_the_rule_is_inside_the_streamed_routes_shapes():
    from torch_assimilate_amd.engine import LetkfEngine
    eng = LetkfEngine.__new__(LetkfEngine)
    for m in (1, 2, 8, 9):
        for k in (2, 40, 64, 65, 80, 96, 97, 128, 129):
            for p in (k, k + 1, 101, 145, 256, 257):
                if eng._patch64s_auto(m, k, p):
                    assert 65 <= k <= 128 and k < p <= 256 and m <= 8, (m, k, p)      # never outside what was measured
    assert eng.PATCH64S_MAX_BLOCKS == 16
    # the measured range (profiles/patch64s_time.json): 65 .. 128 members, p_max / k up to 101 / 65, up to 8 state rows
    assert (eng.PATCH64S_AUTO_MIN_K, eng.PATCH64S_AUTO_MAX_K, eng.PATCH64S_AUTO_NUM, eng.PATCH64S_AUTO_DEN,
            eng.PATCH64S_AUTO_MAX_ROWS) == (65, 128, 101, 65, 8)
    for shape, want in (((1, 65, 101), True), ((1, 65, 102), False), ((1, 64, 99), False), ((1, 80, 101), True), ((8, 80, 101), True),
                        ((9, 80, 101), False), ((1, 96, 101), True), ((1, 128, 145), True), ((1, 128, 199), False), ((1, 80, 80), False)):
        assert eng._patch64s_auto(*shape) == want, shape


class StandInEngine:
    """What LETKF.analyse_arrays asks of an engine on its float64 per-point path, recorded"""

    def __init__(self, stream_auto, patch_auto, cover, fits):
        self.device = torch.device("cpu")
        self.answers = dict(stream_auto=stream_auto, patch_auto=patch_auto, cover=cover, fits=fits)
        self.calls = []
        self.lib = self

    def _stream64_auto(self, m, k, p_max):
        self.calls.append(("_stream64_auto", m, k, p_max))
        return self.answers["stream_auto"]

    def _patch64s_auto(self, m, k, p_max):
        self.calls.append(("_patch64s_auto", m, k, p_max))
        return self.answers["patch_auto"]

    def mia_letkf_patch_stream_f64_cover(self, *a):
        self.calls.append((COVER,) + a)
        return 1 if self.answers["cover"] else 0

    def patch64s_fits(self, nb, tiles, k):
        self.calls.append(("patch64s_fits", k, tuple(tiles.shape)))
        return self.answers["fits"]

    def analysis(self, x, yb, d, nb, inf, **kw):
        self.calls.append(("analysis", kw.get("method", "auto"), None if kw.get("tile_points") is None else tuple(kw["tile_points"].shape),
                           sorted(kw)))
        n = nb.g1 - nb.g0
        return x[:, :, nb.g0:nb.g1].clone(), torch.zeros(n, dtype=torch.int32)


def class_call(answers, dtype=F64, mesh=(3, 4), weight_save_path=None, m=2, k=80, p_max=100):
    import warnings
    from torch_assimilate_amd.engine import NeighbourLists
    from torch_assimilate_amd.interface import LETKF
    eng = StandInEngine(*answers)
    G, P = 12, 6
    flt = LETKF(localization=object(), inf_factor=1.1, engine=eng, dtype=dtype, mesh_shape=mesh, weight_save_path=weight_save_path)
    nb = NeighbourLists(torch.zeros(G, dtype=torch.int32), torch.zeros((G, 104), dtype=torch.int32), torch.zeros((G, 104), dtype=F64),
                        104, p_max, 0, G)
    flt._lists = lambda *a, **kw: nb
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        xa = flt.analyse_arrays(torch.zeros((m, k, G), dtype=dtype), torch.zeros((k, P), dtype=dtype), torch.zeros(P, dtype=dtype),
                                grid_coords=list(range(G)), obs_coords=list(range(P)))
    assert tuple(xa.shape) == (m, k, G)
    return eng.calls, [str(x.message) for x in w]


def test_the_class_names_the_method_exactly_where_every_condition_holds():
    before = ("analysis", "auto", (1, 16), ["kernel_program", "rbf_gamma", "return_flags", "tile_points"])
    for s in (False, True):
        for p in (False, True):
            for c in (False, True):
                for f in (False, True):
                    calls, warned = class_call((s, p, c, f))
                    assert not warned
                    last = calls[-1]
                    if s and p and c and f:
                        assert last == ("analysis", "patch64s", (1, 16), sorted(before[3] + ["method"])), calls
                        assert [x[0] for x in calls[:-1]] == ["_stream64_auto", "_patch64s_auto", COVER, "patch64s_fits"]
                        assert calls[0][1:] == (2, 80, 100) and calls[1][1:] == (2, 80, 100)
                        assert calls[2][1:] == (2, 80, 100, 12, 12, 12, 6) and calls[3][1:] == (80, (1, 16))
                    else:
                        assert last == before, calls          # what the class called before: "auto" with its mesh map
                        assert "analysis" not in [x[0] for x in calls[:-1]]
    # a mesh of another size: the existing warning, no map, no question asked; no mesh: nothing at all
    calls, warned = class_call((True, True, True, True), mesh=(3, 5))
    assert len(warned) == 1 and "mesh_shape" in warned[0]
    assert calls == [("analysis", "auto", None, before[3])]
    calls, warned = class_call((True, True, True, True), mesh=None)
    assert not warned and calls == [("analysis", "auto", None, before[3])]
    # float32 never looks at mesh_shape
    calls, warned = class_call((True, True, True, True), dtype=torch.float32, mesh=(3, 5))
    assert not warned and calls == [("analysis", "auto", None, before[3])]

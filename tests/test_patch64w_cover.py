"""The float64 weights of dense local networks under a tile map (csrc/letkf_patch64w.hip, mia_letkf_weights_patch_f64,
LetkfEngine.weights_patch64) without a GPU: the symbols, the host-only cover function against a Python restatement, the
argument validation of the entry, which returns before any HIP call, the engine method against a recording stand-in of the C
library (call sequence cover -> census -> entry -> counter read; one census per map) and the rule by which the class takes
the route."""
import ctypes as C
import os
import re

import pytest
import torch

from test_engine_route_trace import StandInLib, case, make_engine, F32, F64, RETRY_AT

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
NEW_SYMBOLS = ("mia_letkf_weights_patch_f64", "mia_letkf_weights_patch_f64_cover")
ENTRY, COVER, CENSUS = NEW_SYMBOLS[0], NEW_SYMBOLS[1], "mia_letkf_tile_union_census"


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def lds_bytes(k, ub):
    """LDS of a launch, restated from ring64_lds_bytes (csrc/mia_frames64.h) with the caller's
    blocks: ring [2][16][kp | 1], rhs [4 KT][64] and the sqrt(rho) table [16][16 ub + 1] in doubles, the slot table [16 ub]
    in ints"""
    umax, kp, kt = 16 * ub, (k + 1 + 3) & ~3, (k + 15) >> 4
    return ((2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (umax + 1)) * 8 + umax * 4 + 15) // 16 * 16


def covers(k, p_max, n_points, P):
    if P < 0 or n_points < 0 or k < 2 or k > 128 or p_max <= k or p_max > 256:
        return 0
    return int(k * k * 8 < 2 ** 31 and n_points < 2 ** 31 and lds_bytes(k, 16) <= MAX_LDS)


def test_symbols_are_declared_exported_and_bound(lib):
    from torch_assimilate_amd import _cabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mia_letkf.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    declared = sorted(set(re.findall(r"\b(mia_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert sorted(_cabi.EXPORTED_SYMBOLS) == declared                      # EXPORTED_SYMBOLS matches the header
    # mia_letkf_weights_stream_f64's argument list with (tile_pts, n_tiles, union_blocks) in front of the stream, as
    # mia_letkf_analysis_patch_f64 has them
    base, ana = lib.mia_letkf_weights_stream_f64.argtypes, lib.mia_letkf_analysis_patch_f64.argtypes
    assert list(lib.mia_letkf_weights_patch_f64.argtypes) == list(base[:-1]) + list(ana[-4:])
    assert lib.mia_letkf_weights_patch_f64_cover.argtypes == lib.mia_letkf_weights_stream_f64_cover.argtypes


def test_cover_function_vs_restatement(lib):
    cover = lib.mia_letkf_weights_patch_f64_cover
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
    # what replaces the parent's 16 k^2 8 < 2^31: the 32-bit part of a store's address stays inside ONE point's block, and a
    # map entry is an int32
    assert 128 * 128 * 8 == 1 << 17
    assert cover(80, 101, 0, 0) == 1 and cover(80, 101, -1, 0) == 0 and cover(80, 101, 1000, -1) == 0
    for n in (1, 15, 16, 17, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 40):
        assert cover(80, 101, n, 10) == covers(80, 101, n, 10), n
    assert cover(80, 101, (1 << 31) - 1, 10) == 1 and cover(80, 101, 1 << 31, 10) == 0
    # the parent keeps its answers
    assert lib.mia_letkf_weights_stream_f64_cover(80, 101, 1 << 31, 10) == 1
    assert lib.mia_letkf_weights_stream_f64_cover(128, 128, 1000, 10) == 0


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_letkf_weights_patch_f64
    names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "gamma", "Xa", "ldo",
             "o0", "W", "flags", "retry", "tiles", "n_tiles", "ub", "stream")
    null = (None, 10, 1, 80, 0, 5, None, 0, None, None, None, 200, 101, 1.0, 0.0, None, 10, 0, None, None, None, None, 1, 4, None)

    def with_(**kw):
        a = dict(zip(names, null))
        a.update(kw)
        return call(*[a[n] for n in names])

    def parent(**kw):
        a = dict(zip(names, null))
        a.update(kw)
        return lib.mia_letkf_weights_stream_f64(*[a[n] for n in names if n not in ("tiles", "n_tiles", "ub")])
    # the one order of the tile entries: sizes, inflation, gamma, empty shard, NULL pointers
    assert with_(k=1) == -2 and with_(m=0) == -2 and with_(g1=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    assert with_(n_tiles=-1) == -2                                          # the map's size among the sizes
    assert with_(inf=-1.0) == -2 and with_(inf=0.0) == -2                   # inflation
    assert with_(gamma=0.5) == -3                                           # the float64 RBF filter is not this route's
    assert with_(g1=0) == 0                                                 # empty shard
    assert with_() == -1                                                    # NULL pointers
    assert with_(gamma=0.5, g1=0) == -3 and with_(inf=0.0, gamma=0.5) == -2 and with_(k=1, inf=0.0) == -2
    for kw in (dict(), dict(inf=-1.0), dict(g1=0), dict(gamma=0.5), dict(k=1), dict(m=0), dict(gamma=0.5, g1=0)):
        assert with_(**kw) == parent(**kw), kw
    # with the required pointers present: the map, sizes, then option and cover (nothing is dereferenced before them).  X and
    # Xa stay NULL
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(rec=ptr, cnt=ptr, idx=ptr, w=ptr, W=ptr, flags=ptr, retry=ptr, tiles=ptr)
    for missing in ("cnt", "idx", "w", "W", "flags", "retry", "tiles"):
        assert with_(**dict(full, **{missing: None})) == -1, missing
    assert with_(X=ptr, ldx=4, **full) == -2 and with_(Xa=ptr, ldo=4, **full) == -2    # given, but shorter than the shard
    assert with_(n_tiles=0, **full) == -2                                   # no tiles for a non-empty range
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
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


# ---- the engine method against the recording stand-in -----------------------------------------------------------------------------
def names_of(trace):
    return [line.split("(")[0] for line in trace if not line.startswith("#")]


def scenario(k=80, p_max=101, n=37, union=176):
    lib = StandInLib()
    eng = make_engine(lib)
    t = case(F64, 1, k, p_max, n=n)
    tiles = torch.full(((n + 15) // 16, 16), -1, dtype=torch.int32)
    tiles.reshape(-1)[:n] = torch.arange(n, dtype=torch.int32)
    t["tiles"] = tiles
    lib.begin("weights_patch64", t, census=(0, union))
    return lib, eng, t


def test_the_engine_calls_cover_census_entry_and_reads_the_counter(monkeypatch):
    from torch_assimilate_amd import _cabi
    assert ENTRY not in RETRY_AT                 # (the stand-in does not know this entry: no decline is deposited, the counter stays 0)
    lib, eng, t = scenario()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    res = eng.weights_patch64(None, None, t["nbrs"], t["tiles"], 1.1, rec=t["rec"], out=torch.zeros((37, 80, 80), dtype=F64),
                              return_flags=True)
    assert isinstance(res, tuple) and len(res) == 2 and res[0].shape == (37, 80, 80) and res[1].shape == (37,)
    assert names_of(lib.trace) == [COVER, CENSUS, ENTRY]                    # ... and the counter (0) is read on the host: no redo
    cover, census, entry = [line for line in lib.trace if not line.startswith("#")]
    assert cover == "%s(80, 101, 37, 6) = 1" % COVER
    assert census.startswith(CENSUS + "(tiles, 3, 37, cnt, idx, %d, 101, 1, " % t["nbrs"].p_cap)
    # the entry: X = Xa = NULL, the shard, W, flags, the counter, then the map, its tiles, ceil(176 / 16) blocks, the stream
    assert entry.startswith(ENTRY + "(NULL, 39, 1, 80, 2, 39, rec, 6, cnt, idx, w, %d, 101, 1.1, 0.0, NULL, 37, 0, " % t["nbrs"].p_cap)
    assert entry.endswith(", tiles, 3, 11, NULL) = 0")
    ent = t["nbrs"].tile_census[id(t["tiles"])]
    assert ent[0] is t["tiles"] and ent[2] == 176
    # a second call with the same map: no second census; a deferred redo reads the counter when it is invoked
    del lib.trace[:]
    W, finish = eng.weights_patch64(None, None, t["nbrs"], t["tiles"], 1.1, rec=t["rec"], out=res[0], defer_retry=True)
    assert names_of(lib.trace) == [COVER, ENTRY] and t["nbrs"].tile_census[id(t["tiles"])] is ent
    assert W is res[0] and finish() == 0 and names_of(lib.trace) == [COVER, ENTRY]
    # ... also after an ANALYSIS with the same lists and map has paid for it (one census for both)
    lib2, eng2, t2 = scenario(k=40, union=150)
    monkeypatch.setattr(_cabi, "lib", lambda: lib2)
    eng2.analysis(t2["X"], None, None, t2["nbrs"], 1.1, rec=t2["rec"], method="patch64", tile_points=t2["tiles"])
    assert names_of(lib2.trace).count(CENSUS) == 1
    del lib2.trace[:]
    assert eng2.weights_patch64(None, None, t2["nbrs"], t2["tiles"], 1.1, rec=t2["rec"],
                                out=torch.zeros((37, 40, 40), dtype=F64)) is not None
    assert names_of(lib2.trace) == [COVER, ENTRY] and lib2.trace[-1].endswith(", tiles, 3, 10, NULL) = 0")
    # a named union_blocks is passed on; a new map is validated without the count
    del lib2.trace[:]
    other = t2["tiles"].clone()
    eng2.weights_patch64(None, None, t2["nbrs"], other, 1.1, rec=t2["rec"], out=torch.zeros((37, 40, 40), dtype=F64), union_blocks=7)
    assert names_of(lib2.trace) == [COVER, CENSUS, ENTRY] and lib2.trace[-1].endswith(", 3, 7, NULL) = 0")
    assert ", 101, 0, " in lib2.trace[1]


def test_declined_points_are_redone_behind_the_counter(monkeypatch):
    from torch_assimilate_amd import _cabi
    lib, eng, t = scenario()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    monkeypatch.setitem(RETRY_AT, ENTRY, -5)     # (the counter's place in this entry's list: the stand-in deposits the declines)
    lib.declines = 3
    out = torch.zeros((37, 80, 80), dtype=F64)
    W, finish = eng.weights_patch64(None, None, t["nbrs"], t["tiles"], 1.1, rec=t["rec"], out=out, defer_retry=True)
    assert names_of(lib.trace) == [COVER, CENSUS, ENTRY]
    assert finish() == 3
    assert names_of(lib.trace) == [COVER, CENSUS, ENTRY, "mia_letkf_weights_retry_f64"]
    # the redo raises where the Jacobi kernel cannot hold the shape: AFTER the tile entry has run
    lib.rc["mia_letkf_weights_retry_f64"] = -3
    W, finish = eng.weights_patch64(None, None, t["nbrs"], t["tiles"], 1.1, rec=t["rec"], out=out, defer_retry=True)
    with pytest.raises(_cabi.MiaError, match="status -3"):
        finish()


def test_bad_arguments_raise_before_any_call(monkeypatch):
    from torch_assimilate_amd import _cabi
    lib, eng, t = scenario()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    good, out = t["tiles"], torch.zeros((37, 80, 80), dtype=F64)
    for bad in (good.to(torch.int64), good.reshape(-1), good[:, :8], good.tolist(), None):
        with pytest.raises(ValueError, match="tile_points"):
            eng.weights_patch64(None, None, t["nbrs"], bad, 1.1, rec=t["rec"], out=out)
    for ub in (0, -1, 17, 100):
        with pytest.raises(ValueError, match="union_blocks"):
            eng.weights_patch64(None, None, t["nbrs"], good, 1.1, rec=t["rec"], out=out, union_blocks=ub)
    assert names_of(lib.trace) == []
    # an invalid map: ValueError from the census' answer, before the entry
    lib.census = (2, 0)
    with pytest.raises(ValueError, match="more than once"):
        eng.weights_patch64(None, None, t["nbrs"], good, 1.1, rec=t["rec"], out=out)
    assert names_of(lib.trace) == [COVER, CENSUS]
    # outside the cover, MIA_ERR_UNSUPPORTED from the entry, float32 input: None
    lib.census = (0, 176)
    del lib.trace[:]
    lib.rc[COVER] = 0
    assert eng.weights_patch64(None, None, t["nbrs"], good, 1.1, rec=t["rec"], out=out) is None
    assert names_of(lib.trace) == [COVER]
    lib.rc = {ENTRY: -3}
    assert eng.weights_patch64(None, None, t["nbrs"], good, 1.1, rec=t["rec"], out=out) is None
    del lib.trace[:]
    assert eng.weights_patch64(t["Yb"].to(F32), t["d"].to(F32), t["nbrs"], good, 1.1) is None and names_of(lib.trace) == []


def test_the_class_rule():
    """LetkfEngine._weights_patch64_auto: the map wherever _weights_stream64_auto says yes (from 97 members on), never outside
    the kernel's cover, and where the Jacobi kernel runs only inside the measured constants."""
    import torch_assimilate_amd as mia
    E = mia.LetkfEngine
    eng = E.__new__(E)                           # (the rule reads class constants only: no device)
    for k in range(2, 131):
        for p in range(0, 259):
            auto = eng._weights_patch64_auto(k, p)
            if covers(k, p, 1000, 1000) != 1:
                assert not auto, (k, p)
            elif eng._weights_stream64_auto(k, p):
                assert auto, (k, p)
            else:
                assert E._jacobi_primal_fits(k, p)
                assert auto == (E.WEIGHTS_PATCH64_AUTO_MIN_K <= k <= E.WEIGHTS_PATCH64_AUTO_MAX_K and
                                E.WEIGHTS_PATCH64_AUTO_DEN * p <= E.WEIGHTS_PATCH64_AUTO_NUM * k), (k, p)
    assert eng._weights_patch64_auto(128, 145) and eng._weights_patch64_auto(112, 145) and eng._weights_patch64_auto(97, 101)
    assert not eng._weights_patch64_auto(128, 128) and not eng._weights_patch64_auto(128, 257)
    assert E.WEIGHTS_PATCH64_MAX_BLOCKS == 16

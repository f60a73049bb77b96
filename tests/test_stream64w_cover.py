"""The float64 weights route for dense local networks of up to 128 members (csrc/letkf_stream64w.hip) without a GPU: the
host-only cover function against a Python restatement, the argument validation of mia_letkf_weights_stream_f64, which returns
before any HIP call, and the rule by which the class takes the route."""
import ctypes as C
import os
import re

import pytest

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
MAX_TILES = 65536 * 65535            # a two-dimensional launch grid of one tile per block
NEW_SYMBOLS = ("mia_letkf_weights_stream_f64", "mia_letkf_weights_stream_f64_cover")


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def lds_bytes(k, p_max):
    """LDS of a launch, restated from ring64_lds_bytes and ring64_blocks (csrc/mia_frames64.h): ring
    [2][16][kp | 1], rhs [4 KT][64] and the sqrt(rho) table [16][16 UB + 1] in doubles, the slot table [16 UB] in ints, with
    UB = min(ceil((p_max + 16) / 16), 16) sixteen-slot blocks"""
    ub = min((p_max + 16 + 15) >> 4, 16)
    umax, kp, kt = 16 * ub, (k + 1 + 3) & ~3, (k + 15) >> 4
    return ((2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (umax + 1)) * 8 + umax * 4 + 15) // 16 * 16


def covers(k, p_max, n_points, P):
    if P < 0 or n_points < 0 or k < 2 or k > 128 or p_max <= k or p_max > 256:
        return 0
    return int(16 * k * k * 8 < 2 ** 31 and lds_bytes(k, p_max) <= MAX_LDS and ((n_points + 15) >> 4) <= MAX_TILES)


def test_symbols_are_declared_exported_and_bound(lib):
    from torch_assimilate_amd import _cabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mia_letkf.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    assert lib.mia_letkf_weights_stream_f64.argtypes == lib.mia_letkf_weights_matfun_f64.argtypes
    assert lib.mia_letkf_weights_stream_f64_cover.argtypes == lib.mia_letkf_weights_f64_cover.argtypes


def test_cover_function_vs_restatement(lib):
    cover = lib.mia_letkf_weights_stream_f64_cover
    # 1 everywhere inside 2 <= k <= 128, k < p_max <= 256; the LDS of a launch never refuses a shape
    worst = 0
    for k in range(2, 129):
        for p in range(k + 1, 257):
            assert cover(k, p, 1000, 1000) == 1, (k, p)
            worst = max(worst, lds_bytes(k, p))
    assert worst == lds_bytes(128, 256) == 84352 <= MAX_LDS
    for k, p in ((80, 93), (80, 173), (96, 107), (96, 173), (128, 139), (128, 203), (65, 77), (64, 153)):   # the shapes it is for
        assert cover(k, p, 100000, 100000) == 1, (k, p)
    # the edges: p_max = k (the dual routes'), 257 slots, ensemble sizes 1 and 129
    for k in (2, 40, 64, 65, 80, 128):
        assert cover(k, k, 1000, 10) == 0 and cover(k, k + 1, 1000, 10) == 1 and cover(k, 256, 1000, 10) == 1, k
        assert cover(k, 257, 1000, 10) == 0 and cover(k, 0, 1000, 10) == 0 and cover(k, -1, 1000, 10) == 0, k
    assert cover(1, 2, 1000, 10) == 0 and cover(1, 139, 1000, 10) == 0 and cover(129, 139, 1000, 10) == 0 and cover(129, 256, 1000, 10) == 0
    for k in (0, 1, 2, 3, 16, 17, 63, 64, 65, 96, 127, 128, 129, 200):
        for p in (-1, 0, 1, k - 1, k, k + 1, 64, 65, 128, 129, 255, 256, 257, 1000):
            assert cover(k, p, 1000, 1000) == covers(k, p, 1000, 1000), (k, p)
    # W's 32-bit offsets inside a tile: 16 k^2 8 bytes stay far below 2^31 up to k = 128
    assert 16 * 128 * 128 * 8 == 1 << 21
    # negative sizes and the grid: one tile per block of a 65536 x 65535 launch
    assert cover(80, 93, 0, 0) == 1 and cover(80, 93, -1, 0) == 0 and cover(80, 93, 1000, -1) == 0
    assert cover(80, 93, 16 * MAX_TILES, 10) == 1 and cover(80, 93, 16 * MAX_TILES + 1, 10) == 0
    for n in (1, 15, 16, 17, 1 << 31, (1 << 31) + 1, 1 << 40):
        assert cover(80, 93, n, 10) == covers(80, 93, n, 10), n
    # the neighbours keep their answers: the dual weights routes refuse these shapes, the streamed analysis covers them
    assert lib.mia_letkf_weights_f64_cover(64, 31, 1000, 10) == 1 and lib.mia_letkf_weights_f64_cover(64, 65, 1000, 10) == 0
    assert lib.mia_letkf_weights_wide_f64_cover(128, 97, 1000, 10) == 1 and lib.mia_letkf_weights_wide_f64_cover(128, 139, 1000, 10) == 0
    assert lib.mia_letkf_stream_f64_cover(1, 128, 139, 1000, 1000, 1000, 10) == 1
    assert lib.mia_letkf_stream_f64_cover(1, 128, 128, 1000, 1000, 1000, 10) == 0


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_letkf_weights_stream_f64
    null = (None, 10, 1, 80, 0, 5, None, 0, None, None, None, 200, 93, 1.0, 0.0, None, 10, 0, None, None, None, None)

    def with_(fn=call, **kw):
        names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "gamma", "Xa", "ldo",
                 "o0", "W", "flags", "retry", "stream")
        a = dict(zip(names, null))
        a.update(kw)
        return fn(*[a[n] for n in names])
    # the order of mia_letkf_weights_matfun_f64
    assert with_(inf=-1.0) == -2 and with_(inf=0.0) == -2                   # inflation
    assert with_(g1=0) == 0                                                 # empty shard
    assert with_(gamma=0.5) == -3                                           # the float64 RBF filter is not this route's
    assert with_() == -1                                                    # NULL records / pointers
    assert with_(gamma=0.5, g1=0) == -3 and with_(inf=0.0, gamma=0.5) == -2
    assert with_(k=1) == -2 and with_(m=0) == -2 and with_(g1=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    for kw in (dict(), dict(inf=-1.0), dict(g1=0), dict(gamma=0.5), dict(k=1), dict(m=0)):
        assert with_(**kw) == with_(fn=lib.mia_letkf_weights_matfun_f64, k=kw.get("k", 4), p_cap=8, p_max=4,
                                    **dict((n, v) for n, v in kw.items() if n != "k")), kw
    # with the required pointers present: sizes, then the cover (nothing is dereferenced before it).  X and Xa stay NULL.
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(rec=ptr, cnt=ptr, idx=ptr, w=ptr, W=ptr, flags=ptr, retry=ptr)
    for missing in ("cnt", "idx", "w", "W", "flags", "retry"):
        assert with_(**dict(full, **{missing: None})) == -1, missing
    assert with_(X=ptr, ldx=4, **full) == -2 and with_(Xa=ptr, ldo=4, **full) == -2    # given, but shorter than the shard
    assert with_(p_max=80, **full) == -3 and with_(p_max=63, **full) == -3  # p_max <= k: the dual routes'
    assert with_(p_cap=64, **full) == -3                                    # ... also after p_max is cut to p_cap
    assert with_(k=129, **full) == -3                                       # ensemble size
    assert with_(p_cap=300, p_max=257, **full) == -3                        # more than 256 slots
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                          # the A/B switch of the tile routes
        assert with_(k=128, p_max=139, **full) == -3
    finally:
        lib.mia_set_option(b"tile", -1)


def test_the_class_rule():
    """LetkfEngine._weights_stream64_auto: the route wherever the Jacobi kernel cannot hold the shape and the kernel covers it,
    never at k <= 64, and elsewhere only inside the measured constants (which start at 65 members at the earliest)."""
    import torch_assimilate_amd as mia
    E = mia.LetkfEngine
    eng = E.__new__(E)                           # (the rule reads class constants only: no device)
    for k in range(2, 131):
        for p in range(0, 259):
            auto = eng._weights_stream64_auto(k, p)
            inside = covers(k, p, 1000, 1000) == 1
            if not inside or k <= 64:
                assert not auto, (k, p)
            elif not E._jacobi_primal_fits(k, p):
                assert auto, (k, p)
            else:
                assert auto == (k >= E.WEIGHTS_STREAM64_AUTO_MIN_K and
                                E.WEIGHTS_STREAM64_AUTO_DEN * p <= E.WEIGHTS_STREAM64_AUTO_NUM * k), (k, p)
    assert not E._jacobi_primal_fits(97, 98) and E._jacobi_primal_fits(96, 256)       # the Jacobi kernel ends at 96 members
    assert eng._weights_stream64_auto(128, 139) and eng._weights_stream64_auto(113, 123) and eng._weights_stream64_auto(97, 98)
    assert not eng._weights_stream64_auto(128, 128) and not eng._weights_stream64_auto(128, 257)
    assert E.WEIGHTS_STREAM64_AUTO_MIN_K >= 65

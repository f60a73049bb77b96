"""The float64 IEnKS update for ensembles up to 128 members (csrc/lienks_wide64.hip) without a GPU: the two symbols, the
host-only cover function against a Python restatement, and the argument validation of mia_lienks_update_wide_f64, which returns
before any HIP call in mia_lienks_update_matfun_f64's order: sizes, empty shard, NULL pointers, option and cover."""
import ctypes as C
import os
import re

import pytest

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
MAX_TILES = 65536 * 65535            # a two-dimensional launch grid of one tile per block
NEW_SYMBOLS = ("mia_lienks_update_wide_f64", "mia_lienks_update_wide_f64_cover")


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def lds_bytes(k, p_max):
    """LDS of the instantiation the route picks, letkf_wide64w.hip's to the byte: record image [16 UT][16 KT + 5], sqrt(rho)
    table [16][16 UT + 1] (later the exchange buffer), [NW][16] crossing scalars in doubles; slot table [16 UT] and NW words.
    The shift and the shifted innovations live in registers: not one byte more."""
    ut = min(max((p_max + 8 + 15) // 16, 1), 8)
    kt = (k + 15) // 16
    nw = 2 if ut <= 6 else 4
    return ((16 * ut * (16 * kt + 5) + 16 * (16 * ut + 1) + 16 * nw) * 8 + (16 * ut + nw) * 4 + 15) // 16 * 16


def covers(k, p_max, n_points, P):
    if P < 0 or k < 2 or k > 128 or p_max < 0 or p_max > k or n_points < 0:
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
    # the argument lists of the 2.14 twins
    assert lib.mia_lienks_update_wide_f64.argtypes == lib.mia_lienks_update_matfun_f64.argtypes
    assert lib.mia_lienks_update_wide_f64_cover.argtypes == lib.mia_lienks_update_f64_cover.argtypes


def test_cover_function_vs_restatement(lib):
    cover = lib.mia_lienks_update_wide_f64_cover
    # 1 everywhere inside 2 <= k <= 128, 0 <= p_max <= k; the LDS of the chosen instantiation never refuses a shape
    worst = 0
    for k in range(2, 129):
        for p in range(0, k + 1):
            assert cover(k, p, 1000, 1000) == 1, (k, p)
            assert cover(k, p, 1000, 1000) == lib.mia_letkf_weights_wide_f64_cover(k, p, 1000, 1000), (k, p)
            worst = max(worst, lds_bytes(k, p))
    assert worst == lds_bytes(128, 128) == 153744 <= MAX_LDS
    for k, p in ((80, 63), (96, 81), (128, 97), (65, 53), (128, 62), (72, 69), (94, 20)):      # the shapes the route is for
        assert cover(k, p, 100000, 100000) == 1, (k, p)
    assert cover(40, 35, 1000, 10) == 1 and cover(64, 64, 1000, 10) == 1           # k <= 64 too: the route is there by name
    assert cover(1, 1, 1000, 10) == 0 and cover(129, 97, 1000, 10) == 0 and cover(129, 129, 1000, 10) == 0
    for k in (2, 40, 64, 65, 80, 128):
        assert cover(k, k + 1, 1000, 10) == 0, k                                   # p_max > k is not this route's
    for k in (0, 1, 2, 3, 16, 17, 63, 64, 65, 96, 127, 128, 129, 200):
        for p in (-1, 0, 1, k - 1, k, k + 1, 64, 65, 128, 129):
            assert cover(k, p, 1000, 1000) == covers(k, p, 1000, 1000), (k, p)
    # W's 32-bit offsets inside a tile: 16 k^2 8 bytes stay far below 2^31 up to k = 128
    assert 16 * 128 * 128 * 8 == 1 << 21
    # grid size: one tile per block of a 65536 x 65535 launch
    assert cover(80, 63, 0, 0) == 1 and cover(80, 63, -1, 0) == 0 and cover(80, 63, 1000, -1) == 0
    assert cover(80, 63, 16 * MAX_TILES, 10) == 1 and cover(80, 63, 16 * MAX_TILES + 1, 10) == 0
    for n in (1, 15, 16, 17, 1 << 31, (1 << 31) + 1, 1 << 40):
        assert cover(80, 63, n, 10) == covers(80, 63, n, 10), n


NAMES = ("W_in", "w_stride", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "eps", "W_out", "flags", "retry",
         "stream")
NULLS = (None, 6400, 80, 0, 5, None, 0, None, None, None, 64, 63, 0.0, None, None, None, None)


def test_argument_validation_precedes_any_device_work(lib):
    def with_(fn=lib.mia_lienks_update_wide_f64, **kw):
        a = dict(zip(NAMES, NULLS))
        a.update(kw)
        return fn(*[a[n] for n in NAMES])
    # sizes first, whatever the pointers
    assert with_(k=1) == -2 and with_(g1=-1) == -2 and with_(g0=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    assert with_(p_max=-1) == -2
    assert with_(w_stride=6399) == -2 and with_(w_stride=80) == -2 and with_(w_stride=1) == -2    # neither 0 nor k^2
    assert with_(w_stride=15, g1=0) == -2                                   # ... before the empty shard
    assert with_(g1=0) == 0 and with_(g1=0, w_stride=0) == 0                # empty shard, before the NULL pointers
    assert with_() == -1 and with_(w_stride=0) == -1                        # NULL pointers
    # the order of mia_lienks_update_matfun_f64, at a shape both entries know (k = 4)
    small = dict(k=4, w_stride=16, p_cap=8, p_max=4)
    for kw in (dict(), dict(k=1), dict(g1=-1), dict(P=-1), dict(w_stride=15), dict(w_stride=15, g1=0), dict(g1=0),
               dict(p_max=-1)):
        a = dict(small, **kw)
        assert with_(**a) == with_(fn=lib.mia_lienks_update_matfun_f64, **a), kw
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(W_in=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, W_out=ptr, flags=ptr, retry=ptr)
    for missing in ("W_in", "cnt", "idx", "w", "W_out", "flags", "retry"):
        assert with_(**dict(full, **{missing: None})) == -1, missing
    assert with_(P=3, **dict(full, rec=None)) == -1
    # NULL before the cover: an uncovered shape with a pointer missing is a NULL error
    assert with_(k=129, w_stride=129 * 129, **dict(full, flags=None)) == -1
    # then the cover: nothing is dereferenced before it (the 512-byte buffer stands for every array)
    assert with_(p_cap=200, p_max=81, **full) == -3                         # p_max > k
    assert with_(k=129, w_stride=129 * 129, **full) == -3                   # ensemble size
    assert with_(k=129, w_stride=0, eps=1e-3, **full) == -3
    assert with_(g1=16 * MAX_TILES + 1, **full) == -3                       # more tiles than a launch grid holds
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3 and with_(w_stride=0, eps=1e-3, **full) == -3      # the A/B switch of the tile routes
        assert with_(k=40, w_stride=1600, p_cap=40, p_max=35, **full) == -3
        assert with_(**dict(full, flags=None)) == -1 and with_(k=1, **full) == -2     # (the order holds with the switch off)
    finally:
        lib.mia_set_option(b"tile", -1)


def test_one_wavefront_entries_keep_their_answers_at_65_members(lib):
    assert lib.mia_lienks_update_f64_cover(65, 20, 1000, 10) == 0 and lib.mia_lienks_update_f64_cover(64, 31, 1000, 10) == 1
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    a = dict(zip(NAMES, NULLS))
    a.update(W_in=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, W_out=ptr, flags=ptr, retry=ptr, k=65, w_stride=65 * 65, p_cap=64,
             p_max=20)
    assert lib.mia_lienks_update_matfun_f64(*[a[n] for n in NAMES]) == -3
    a.update(k=80, w_stride=6400, p_max=63)
    assert lib.mia_lienks_update_matfun_f64(*[a[n] for n in NAMES]) == -3

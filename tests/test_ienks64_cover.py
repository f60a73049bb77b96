"""The float64 IEnKS update on tiles (csrc/lienks_tile64.hip) without a GPU: the three symbols, the host-only cover function
against a Python restatement, and the argument validation of mia_lienks_update_matfun_f64 / mia_lienks_update_retry_f64, which
return before any HIP call in the order sizes, empty shard, NULL pointers, cover."""
import ctypes as C

import pytest

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
MAX_TILES = 65536 * 65535            # a two-dimensional launch grid of one tile per block
NEW_SYMBOLS = ("mia_lienks_update_matfun_f64", "mia_lienks_update_retry_f64", "mia_lienks_update_f64_cover")


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def lds_bytes(k, p_max):
    """the weights kernel's image: the shift lives in the rows of sqrt(rho), the route asks for not one byte more"""
    ut = min(4, max(1, (p_max + 8 + 15) >> 4))
    umax, kp = 16 * ut, (k + 1 + 3) & ~3
    return ((umax * (kp | 1) + 16 * (umax + 1)) * 8 + umax * 4 + 15) & ~15


def covers(k, p_max, n_points, P):
    if P < 0 or k < 2 or k > 64 or p_max < 0 or p_max > k or n_points < 0:
        return 0
    return int(lds_bytes(k, p_max) <= MAX_LDS and ((n_points + 15) >> 4) <= MAX_TILES)


def test_symbols_resolve(lib):
    from torch_assimilate_amd import _cabi
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS


def test_cover_function_vs_restatement(lib):
    cover = lib.mia_lienks_update_f64_cover
    assert cover(40, 20, 100000, 50000) == 1 and cover(20, 10, 100000, 50000) == 1 and cover(64, 31, 100000, 50000) == 1
    # ensemble size and list length: every boundary
    for k in (0, 1, 2, 3, 16, 17, 63, 64, 65, 96):
        for p in (-1, 0, 1, k - 1, k, k + 1, 64, 65):
            assert cover(k, p, 1000, 1000) == covers(k, p, 1000, 1000), (k, p)
    assert cover(2, 2, 16, 2) == 1 and cover(2, 0, 16, 2) == 1 and cover(64, 64, 1000, 10) == 1
    assert cover(65, 20, 1000, 10) == 0 and cover(1, 1, 1000, 10) == 0 and cover(0, 0, 1000, 10) == 0
    assert cover(20, 21, 1000, 10) == 0 and cover(20, -1, 1000, 10) == 0    # p_max > k is not this route's
    # it is the weights route's cover: the same shapes, to the last one
    for k in (2, 17, 40, 64, 65):
        for p in (0, k, k + 1):
            assert cover(k, p, 1000, 10) == lib.mia_letkf_weights_f64_cover(k, p, 1000, 10)
    assert max(lds_bytes(k, p) for k in range(2, 65) for p in range(0, k + 1)) == lds_bytes(64, 64) <= MAX_LDS
    # grid size: one tile per block of a 65536 x 65535 launch
    assert cover(40, 20, 0, 0) == 1 and cover(40, 20, -1, 0) == 0 and cover(40, 20, 1000, -1) == 0
    assert cover(40, 20, 16 * MAX_TILES, 10) == 1 and cover(40, 20, 16 * MAX_TILES + 1, 10) == 0
    for n in (1, 15, 16, 17, 1 << 31, (1 << 31) + 1, 1 << 40):
        assert cover(40, 20, n, 10) == covers(40, 20, n, 10), n


NAMES = ("W_in", "w_stride", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "eps", "W_out", "flags", "retry",
         "stream")
NULLS = (None, 16, 4, 0, 5, None, 0, None, None, None, 8, 4, 0.0, None, None, None, None)


def test_matfun_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_lienks_update_matfun_f64

    def with_(**kw):
        a = dict(zip(NAMES, NULLS))
        a.update(kw)
        return call(*[a[n] for n in NAMES])
    # sizes first, whatever the pointers
    assert with_(k=1) == -2 and with_(g1=-1) == -2 and with_(g0=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    assert with_(p_max=-1) == -2
    assert with_(w_stride=15) == -2 and with_(w_stride=4) == -2 and with_(w_stride=1) == -2       # neither 0 nor k^2
    assert with_(w_stride=15, g1=0) == -2                                   # ... before the empty shard
    assert with_(g1=0) == 0 and with_(g1=0, w_stride=0) == 0                # empty shard, before the NULL pointers
    assert with_() == -1 and with_(w_stride=0) == -1                        # NULL pointers
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(W_in=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, W_out=ptr, flags=ptr, retry=ptr)
    for missing in ("W_in", "cnt", "idx", "w", "W_out", "flags", "retry"):
        assert with_(**dict(full, **{missing: None})) == -1, missing
    assert with_(P=3, **dict(full, rec=None)) == -1
    # NULL before the cover: an uncovered shape with a pointer missing is a NULL error
    assert with_(k=65, w_stride=65 * 65, p_cap=64, p_max=20, **dict(full, flags=None)) == -1
    # then the cover: nothing is dereferenced before it (the 512-byte buffer stands for every array)
    assert with_(p_cap=8, p_max=5, **full) == -3                            # p_max > k
    assert with_(k=65, w_stride=65 * 65, p_cap=64, p_max=20, **full) == -3
    assert with_(k=65, w_stride=0, p_cap=64, p_max=20, eps=1e-3, **full) == -3
    assert with_(g1=16 * MAX_TILES + 1, **full) == -3                       # more tiles than a launch grid holds
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3 and with_(w_stride=0, eps=1e-3, **full) == -3      # the A/B switch of the tile routes
        assert with_(**dict(full, flags=None)) == -1 and with_(k=1, **full) == -2     # (the order holds with the switch off)
    finally:
        lib.mia_set_option(b"tile", -1)


def test_retry_argument_validation(lib):
    call = lib.mia_lienks_update_retry_f64
    names = NAMES[:12] + ("tau", "eps", "W_out", "flags", "stream")
    nulls = NULLS[:12] + (1.0, 0.0, None, None, None)

    def with_(**kw):
        a = dict(zip(names, nulls))
        a.update(kw)
        return call(*[a[n] for n in names])
    assert with_(k=1) == -2 and with_(w_stride=15) == -2 and with_(tau=1.5) == -2 and with_(tau=-0.1) == -2
    assert with_(g1=0) == 0
    assert with_() == -1
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(W_in=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, W_out=ptr)
    assert with_(**full) == -1                                              # the retry entry without flags
    assert with_(flags=ptr, **dict(full, W_out=None)) == -1

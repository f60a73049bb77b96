"""The float64 weights route (csrc/letkf_tile64w.hip) without a GPU: the host-only cover function against a Python restatement,
and the argument validation of mia_letkf_weights_matfun_f64, which returns before any HIP call."""
import ctypes as C

import pytest

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
MAX_TILES = 65536 * 65535            # a two-dimensional launch grid of one tile per block


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def lds_bytes(k, p_max):
    ut = min(4, max(1, (p_max + 8 + 15) >> 4))
    umax, kp = 16 * ut, (k + 1 + 3) & ~3
    return ((umax * (kp | 1) + 16 * (umax + 1)) * 8 + umax * 4 + 15) & ~15


def covers(k, p_max, n_points, P):
    if P < 0 or k < 2 or k > 64 or p_max < 0 or p_max > k or n_points < 0:
        return 0
    return int(lds_bytes(k, p_max) <= MAX_LDS and ((n_points + 15) >> 4) <= MAX_TILES)


def test_cover_function_vs_restatement(lib):
    cover = lib.mia_letkf_weights_f64_cover
    assert cover(40, 20, 100000, 50000) == 1 and cover(20, 10, 100000, 50000) == 1 and cover(64, 31, 100000, 50000) == 1
    # ensemble size and list length: every boundary
    for k in (0, 1, 2, 3, 16, 17, 63, 64, 65, 96):
        for p in (-1, 0, 1, k - 1, k, k + 1, 64, 65):
            assert cover(k, p, 1000, 1000) == covers(k, p, 1000, 1000), (k, p)
    assert cover(2, 2, 16, 2) == 1 and cover(64, 64, 1000, 10) == 1
    assert cover(65, 20, 1000, 10) == 0 and cover(1, 1, 1000, 10) == 0
    assert cover(20, 21, 1000, 10) == 0                                      # p_max > k: not this route's
    # the record image of the largest instantiation stays far inside the LDS: no shape of the route is refused for it
    assert max(lds_bytes(k, p) for k in range(2, 65) for p in range(0, k + 1)) == lds_bytes(64, 64) <= MAX_LDS
    # grid size: one tile per block of a 65536 x 65535 launch
    assert cover(40, 20, 0, 0) == 1 and cover(40, 20, -1, 0) == 0 and cover(40, 20, 1000, -1) == 0
    assert cover(40, 20, 16 * MAX_TILES, 10) == 1 and cover(40, 20, 16 * MAX_TILES + 1, 10) == 0
    for n in (1, 15, 16, 17, 1 << 31, (1 << 31) + 1, 1 << 40):
        assert cover(40, 20, n, 10) == covers(40, 20, n, 10), n


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_letkf_weights_matfun_f64
    null = (None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0, None, None, None, None)

    def with_(**kw):
        names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "gamma", "Xa", "ldo",
                 "o0", "W", "flags", "retry", "stream")
        a = dict(zip(names, null))
        a.update(kw)
        return call(*[a[n] for n in names])
    assert with_() == -1                                                    # NULL pointers
    assert with_(inf=-1.0) == -2 and with_(inf=0.0) == -2
    assert with_(k=1) == -2 and with_(m=0) == -2 and with_(g1=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    assert with_(g1=0) == 0                                                 # empty shard
    assert with_(gamma=0.5) == -3                                           # the float64 RBF filter is not this route's
    assert with_(gamma=0.5, g1=0) == -3                                     # (order as mia_letkf_analysis_matfun_f64)
    # with the required pointers present: sizes, then the cover (nothing is dereferenced before it).  X and Xa stay NULL.
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(rec=ptr, cnt=ptr, idx=ptr, w=ptr, W=ptr, flags=ptr, retry=ptr)
    for missing in ("cnt", "idx", "w", "W", "flags", "retry"):
        assert with_(**dict(full, **{missing: None})) == -1, missing
    assert with_(X=ptr, ldx=4, **full) == -2 and with_(Xa=ptr, ldo=4, **full) == -2    # given, but shorter than the shard
    assert with_(p_cap=8, p_max=5, **full) == -3                            # p_max > k
    assert with_(k=65, p_cap=64, p_max=20, **full) == -3
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                          # the A/B switch of the tile routes
    finally:
        lib.mia_set_option(b"tile", -1)
    assert lib.mia_letkf_weights_retry_f64(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.0, None, 10, 0, None,
                                           None, None) == -1

"""The dense float64 tile route (csrc/letkf_dense64.hip) without a GPU: the host-only cover function and the argument
validation of mia_letkf_analysis_dense_f64, which returns before any HIP call."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def test_cover_function(lib):
    cover = lib.mia_letkf_dense_f64_cover
    assert cover(1, 40, 77, 100000, 100000, 100000, 100000) == 1
    assert cover(3, 64, 153, 1000, 1000, 1000, 1000) == 1
    assert cover(8, 40, 173, 100000, 100000, 100000, 100000) == 1
    assert cover(1, 5, 58, 203, 203, 203, 102) == 1 and cover(1, 2, 3, 16, 16, 16, 3) == 1
    assert cover(1, 65, 153, 1000, 1000, 1000, 1000) == 0 and cover(1, 1, 5, 1000, 1000, 1000, 1000) == 0   # ensemble size
    for k, p in ((40, 40), (40, 20), (20, 0), (64, 64)):                    # p_max <= k is the dual route's
        assert cover(1, k, p, 1000, 1000, 1000, 1000) == 0
        assert lib.mia_letkf_matfun_f64_cover(1, k, p, 1000, 1000, 1000, 1000) == 1
    for k, p in ((40, 41), (20, 31), (64, 153)):                            # ... and p_max > k is not
        assert cover(1, k, p, 1000, 1000, 1000, 1000) == 1
        assert lib.mia_letkf_matfun_f64_cover(1, k, p, 1000, 1000, 1000, 1000) == 0
    assert cover(1, 24, 3000, 1000, 1000, 1000, 3000) == 0                  # lists beyond the record image: the Jacobi kernel
    # capacity: 256 slots where the record image fits the LDS, 224 at k = 64
    assert cover(1, 40, 256, 1000, 1000, 1000, 1000) == 1 and cover(1, 40, 257, 1000, 1000, 1000, 1000) == 0
    assert cover(1, 64, 224, 1000, 1000, 1000, 1000) == 1 and cover(1, 64, 225, 1000, 1000, 1000, 1000) == 0
    assert cover(0, 40, 77, 1000, 1000, 1000, 1000) == 0 and cover(1, 40, 77, 1000, 1000, -1, 1000) == 0
    assert cover(1, 40, 77, 1000, 1000, 1000, -1) == 0
    assert cover(1, 40, 77, 1 << 23, 1000, 1000, 1000) == 0                 # k ld 8 must stay below 2^31 (32-bit lane offsets)


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_letkf_analysis_dense_f64
    null = (None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, None, 10, 0, None, None, None)

    def with_(**kw):
        names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "gamma", "Xa", "ldo",
                 "o0", "flags", "retry", "stream")
        a = dict(zip(names, null))
        a.update(kw)
        return call(*[a[n] for n in names])
    assert with_() == -1                                                    # NULL pointers
    assert with_(inf=-1.0) == -2 and with_(inf=0.0) == -2
    assert with_(k=1) == -2 and with_(m=0) == -2 and with_(g1=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    assert with_(g1=0) == 0                                                 # empty shard
    assert with_(gamma=0.5) == -3                                           # the float64 RBF filter is not this route's
    assert with_(gamma=0.5, g1=0) == -3                                     # (order as mia_letkf_analysis_matfun_f64)
    # with every pointer present: sizes, then the cover (nothing is dereferenced before it)
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(X=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, Xa=ptr, flags=ptr, retry=ptr)
    assert with_(ldx=4, **full) == -2 and with_(ldo=4, **full) == -2        # leading dimensions shorter than the shard
    assert with_(p_max=4, **full) == -3                                     # p_max <= k
    assert with_(p_cap=4000, p_max=3000, **full) == -3                      # beyond the record image
    assert with_(k=65, p_cap=200, p_max=100, **full) == -3
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                          # the A/B switch of the tile routes
    finally:
        lib.mia_set_option(b"tile", -1)

"""The wide float64 tile route (csrc/letkf_wide64.hip, ensembles up to 128 members) without a GPU: the host-only cover function
and the argument validation of mia_letkf_analysis_wide_f64, which returns before any HIP call."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def wide64_lds_bytes(k, p_max):
    """LDS of the instantiation the route picks, restated from csrc/letkf_wide64.hip: record image [16 UT][16 KT + 5], sqrt(rho)
    table [16][16 UT + 1] (later the exchange buffer), [NW][16] crossing scalars in doubles; slot table [16 UT] and NW words"""
    ut = min(max((p_max + 8 + 15) // 16, 1), 8)
    kt = (k + 15) // 16
    nw = 2 if ut <= 6 else 4
    return ((16 * ut * (16 * kt + 5) + 16 * (16 * ut + 1) + 16 * nw) * 8 + (16 * ut + nw) * 4 + 15) // 16 * 16


def test_cover_function(lib):
    from torch_assimilate_amd import _cabi
    assert "mia_letkf_analysis_wide_f64" in _cabi.EXPORTED_SYMBOLS and "mia_letkf_wide_f64_cover" in _cabi.EXPORTED_SYMBOLS
    cover = lib.mia_letkf_wide_f64_cover
    for k, p in ((80, 63), (96, 81), (128, 97), (65, 20), (40, 35), (64, 57)):       # the shapes the route is for
        assert cover(1, k, p, 100000, 100000, 100000, 100000) == 1, (k, p)
        assert cover(8, k, p, 1000, 1000, 1000, 1000) == 1, (k, p)
    assert cover(1, 2, 0, 16, 16, 16, 0) == 1 and cover(1, 2, 2, 16, 16, 16, 3) == 1
    # capacity: the largest instantiation (k = 128, p_max = 128: eight row blocks, eight member blocks, four wavefronts) fits
    # the 159 KB a workgroup may ask for, so every 2 <= k <= 128 with p_max <= k is inside and the route ends at k = 128
    limit = 160 * 1024 - 1024
    assert wide64_lds_bytes(128, 128) == 153744 <= limit
    assert max(wide64_lds_bytes(k, p) for k in range(2, 129) for p in range(0, k + 1)) == 153744
    assert wide64_lds_bytes(80, 63) == 65360                                       # config 4: two workgroups per CU
    assert cover(1, 128, 128, 1000, 1000, 1000, 1000) == 1 and cover(1, 128, 105, 1000, 1000, 1000, 1000) == 1
    assert cover(1, 129, 97, 1000, 1000, 1000, 1000) == 0 and cover(1, 129, 129, 1000, 1000, 1000, 1000) == 0
    assert cover(1, 1, 1, 1000, 1000, 1000, 1000) == 0
    for k, p in ((80, 81), (128, 129), (65, 153), (40, 41)):                        # p_max > k is not this route's
        assert cover(1, k, p, 1000, 1000, 1000, 1000) == 0
    assert cover(0, 80, 63, 1000, 1000, 1000, 1000) == 0 and cover(-1, 80, 63, 1000, 1000, 1000, 1000) == 0
    assert cover(1, 80, -1, 1000, 1000, 1000, 1000) == 0 and cover(1, -80, 63, 1000, 1000, 1000, 1000) == 0
    assert cover(1, 80, 63, 1000, 1000, -1, 1000) == 0 and cover(1, 80, 63, 1000, 1000, 1000, -1) == 0
    assert cover(1, 80, 63, 0, 1000, 1000, 1000) == 0 and cover(1, 80, 63, 1000, 0, 1000, 1000) == 0
    # k ld 8 must stay below 2^31 (32-bit lane offsets): 640 x 3355443 = 2^31 - 128
    assert cover(1, 80, 63, 3355444, 1000, 1000, 1000) == 0 and cover(1, 80, 63, 1000, 3355444, 1000, 1000) == 0
    assert cover(1, 80, 63, 3355443, 3355443, 1000, 1000) == 1
    # the one-wavefront route keeps its answers
    assert lib.mia_letkf_matfun_f64_cover(1, 80, 63, 1000, 1000, 1000, 1000) == 0
    assert lib.mia_letkf_matfun_f64_cover(1, 65, 20, 1000, 1000, 1000, 1000) == 0
    assert lib.mia_letkf_matfun_f64_cover(1, 64, 57, 1000, 1000, 1000, 1000) == 1
    assert lib.mia_letkf_dense_f64_cover(1, 80, 153, 1000, 1000, 1000, 1000) == 0


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_letkf_analysis_wide_f64
    null = (None, 10, 1, 80, 0, 5, None, 0, None, None, None, 64, 63, 1.0, 0.0, None, 10, 0, None, None, None)

    def with_(fn=call, **kw):
        names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "gamma", "Xa", "ldo",
                 "o0", "flags", "retry", "stream")
        a = dict(zip(names, null))
        a.update(kw)
        return fn(*[a[n] for n in names])
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
    assert with_(p_cap=200, p_max=81, **full) == -3                         # p_max > k
    assert with_(k=129, **full) == -3                                       # ensemble size
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    assert with_(fn=lib.mia_letkf_analysis_matfun_f64, **full) == -3        # k = 80 is still outside the one-wavefront route
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                          # the A/B switch of the tile routes
        assert with_(k=40, p_cap=40, p_max=35, **full) == -3
    finally:
        lib.mia_set_option(b"tile", -1)

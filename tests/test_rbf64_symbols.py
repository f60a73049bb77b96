"""The float64 RBF tile route (csrc/lketkf_tile64.hip: LKETKF / LETKF with an RBF or Gauss kernel in the default dtype) without a
GPU: both symbols, the host-only cover function and the argument validation of mia_lketkf_rbf_analysis_matfun_f64, which returns
before any HIP call."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def rbf64_lds_bytes(k, p_max):
    """LDS of the instantiation the route picks, restated from csrc/lketkf_tile64.hip: K [16 pair blocks][16] and the region that
    holds the record image [16 UT][kp | 1] + sqrt(rho) [16][16 UT + 1], later four [k][16] vectors, in doubles; slot table [16 UT],
    pair table [16 pair blocks] and 48 words"""
    ut = min(max((p_max + 8 + 15) // 16, 1), 4)
    kp = (k + 1 + 3) // 4 * 4
    npb = (k * (k + 1) // 2 + k + 15) // 16
    region = max(16 * ut * (kp | 1) + 16 * (16 * ut + 1), 64 * k)
    return ((npb * 256 + region) * 8 + (16 * ut + 16 * npb + 48) * 4 + 15) // 16 * 16


def test_symbols_and_cover(lib):
    from torch_assimilate_amd import _cabi
    for name in ("mia_lketkf_rbf_analysis_matfun_f64", "mia_lketkf_rbf_f64_cover"):
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS
    cover = lib.mia_lketkf_rbf_f64_cover
    assert cover(1, 40, 20, 100000, 100000, 100000, 50000) == 1
    assert cover(3, 2, 5, 1000, 1000, 1000, 10) == 1
    for k, p in ((40, 59), (40, 64), (20, 33), (8, 35), (17, 15), (2, 0)):          # no p_max <= k condition
        assert cover(1, k, p, 1000, 1000, 1000, 1000) == 1, (k, p)
        assert cover(8, k, p, 1000, 1000, 1000, 1000) == 1, (k, p)
    assert cover(1, 41, 20, 1000, 1000, 1000, 10) == 0 and cover(1, 65, 20, 1000, 1000, 1000, 10) == 0      # ensemble size
    assert cover(1, 1, 1, 1000, 1000, 1000, 10) == 0
    assert cover(1, 40, 65, 1000, 1000, 1000, 10) == 0                                                     # list length
    assert cover(1, 40, 20, 1000, 1000, 1000, -1) == 0                                                     # P < 0
    assert cover(0, 40, 20, 1000, 1000, 1000, 10) == 0 and cover(1, 40, -1, 1000, 1000, 1000, 10) == 0
    assert cover(1, 40, 20, 0, 1000, 1000, 10) == 0 and cover(1, 40, 20, 1000, 0, 1000, 10) == 0
    assert cover(1, 40, 20, 1000, 1000, -1, 10) == 0
    # capacity: the largest instantiation (k = 40, lists of 64) fits the 159 KB a workgroup may ask for
    assert max(rbf64_lds_bytes(k, p) for k in range(2, 41) for p in range(0, 65)) == rbf64_lds_bytes(40, 64) <= 160 * 1024 - 1024
    # the other float64 tile routes keep their answers
    assert lib.mia_letkf_matfun_f64_cover(1, 40, 20, 1000, 1000, 1000, 10) == 1
    assert lib.mia_letkf_matfun_f64_cover(1, 40, 59, 1000, 1000, 1000, 10) == 0


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_lketkf_rbf_analysis_matfun_f64
    null = (None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, 0.5, None, 10, 0, None, None, None)

    def with_(fn=call, **kw):
        names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "gamma", "Xa", "ldo",
                 "o0", "flags", "retry", "stream")
        a = dict(zip(names, null))
        a.update(kw)
        return fn(*[a[n] for n in names])
    assert with_(inf=-1.0) == -2 and with_(inf=0.0) == -2
    assert with_(gamma=0.0) == -2 and with_(gamma=-1.0) == -2             # gamma > 0 is required
    assert with_(gamma=0.0, g1=0) == -2                                    # (before the empty-shard answer)
    assert with_(g1=0) == 0                                                # empty shard
    assert with_() == -1                                                   # NULL state
    assert with_(k=1) == -2 and with_(m=0) == -2 and with_(g1=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    # with every pointer present: sizes, then the cover (nothing is dereferenced before it)
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(X=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, Xa=ptr, flags=ptr, retry=ptr)
    assert with_(ldx=4, **full) == -2 and with_(ldo=4, **full) == -2       # leading dimensions shorter than the shard
    assert with_(k=41, **full) == -3                                       # ensemble size
    assert with_(p_cap=72, p_max=65, **full) == -3                         # list length
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    # the existing float64 tile entries keep answering MIA_ERR_UNSUPPORTED for gamma > 0
    for name in ("mia_letkf_analysis_matfun_f64", "mia_letkf_analysis_dense_f64", "mia_letkf_analysis_wide_f64"):
        assert with_(fn=getattr(lib, name), **full) == -3, name
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                         # the A/B switch of the tile routes
    finally:
        lib.mia_set_option(b"tile", -1)

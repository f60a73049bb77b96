"""The float64 IEnKS update for dense local networks of up to 128 members (csrc/lienks_stream64.hip) without a GPU: the two
symbols, the host-only cover function against mia_letkf_weights_stream_f64_cover, the argument validation of
mia_lienks_update_stream_f64, which returns before any HIP call in mia_lienks_update_matfun_f64's order (sizes, empty shard,
NULL pointers, option and cover), and the two helpers by which the IEnKS classes choose the route: the restated LDS of the
general kernel and the gate."""
import ctypes as C
import os
import re

import pytest

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
MAX_TILES = 65536 * 65535            # a two-dimensional launch grid of one tile per block
NEW_SYMBOLS = ("mia_lienks_update_stream_f64", "mia_lienks_update_stream_f64_cover")
# LDS of ienks_update_kernel<double, 256> at tau = 1 by the formula of csrc/ienks.hip: (k, p_max, bundle, transform)
DENSE_ROWS = ((65, 77, 117648, 159536), (72, 77, 136384, 183200), (80, 93, 172496, 234992), (96, 107, 242480, 328080),
              (128, 139, 422432, 569216), (128, 203, 490784, 705152))
# the sparse rows quoted in tests/test_gpu_ienks_wide64.py (p_max <= k: the dual form of the same formula)
SPARSE_ROWS = ((65, 53, 104848, 134224), (72, 69, 132032, 174592), (80, 63, 152656, 195664), (94, 20, 164896, 180256),
               (96, 81, 222160, 287760), (128, 97, 378624, 482112), (128, 62, 340176, 405648))


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


@pytest.fixture(scope="module")
def engine_cls():
    import torch_assimilate_amd as mia
    return mia.LetkfEngine


def lds_bytes(k, p_max):
    """ring64_lds_bytes and ring64_blocks (csrc/mia_frames64.h) to the byte: ring [2][16][kp | 1], rhs [4 KT][64], sqrt(rho) [16][16 ub + 1] doubles and
    the slot table [16 ub] ints; w_mean and the shift live in registers"""
    ub = min((p_max + 16 + 15) >> 4, 16)
    kp, kt = (k + 1 + 3) & ~3, (k + 15) >> 4
    return ((2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (16 * ub + 1)) * 8 + 16 * ub * 4 + 15) // 16 * 16


def covers(k, p_max, n_points, P):
    if P < 0 or k < 2 or k > 128 or p_max <= k or p_max > 256 or n_points < 0:
        return 0
    return int(16 * k * k * 8 < 2 ** 31 and lds_bytes(k, p_max) <= MAX_LDS and ((n_points + 15) >> 4) <= MAX_TILES)


def test_symbols_are_declared_exported_and_bound(lib):
    from torch_assimilate_amd import _build, _cabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mia_letkf.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    assert "core/ienks.py:108-126" in header[header.index("csrc/lienks_stream64.hip"):header.index("int mia_lienks_update_stream_f64(")]
    assert "lienks_stream64.hip" in _build.SOURCES
    # the argument lists of the 2.14 twins
    assert lib.mia_lienks_update_stream_f64.argtypes == lib.mia_lienks_update_matfun_f64.argtypes
    assert lib.mia_lienks_update_stream_f64_cover.argtypes == lib.mia_lienks_update_f64_cover.argtypes


def test_cover_function_vs_the_weights_route(lib):
    cover, wcover = lib.mia_lienks_update_stream_f64_cover, lib.mia_letkf_weights_stream_f64_cover
    worst = 0
    for k in range(2, 130):
        for p in sorted({0, 1, k - 1, k, k + 1, k + 2, k + 17, 2 * k, 139, 203, 255, 256, 257, 300}):
            assert cover(k, p, 1000, 1000) == wcover(k, p, 1000, 1000) == covers(k, p, 1000, 1000), (k, p)
            if covers(k, p, 1000, 1000):
                worst = max(worst, lds_bytes(k, p))
    assert worst == lds_bytes(128, 256) <= MAX_LDS
    for k, p in ((65, 77), (72, 77), (80, 93), (80, 173), (96, 107), (113, 123), (128, 139), (128, 203), (40, 77)):
        assert cover(k, p, 100000, 100000) == 1, (k, p)
    for k in (2, 40, 64, 65, 80, 128):
        assert cover(k, k, 1000, 10) == 0 and cover(k, k + 1, 1000, 10) == 1, k          # p_max <= k is the dual routes'
    assert cover(1, 5, 1000, 10) == 0 and cover(129, 139, 1000, 10) == 0 and cover(128, 257, 1000, 10) == 0
    # grid size: one tile per block of a 65536 x 65535 launch
    assert cover(80, 93, 0, 0) == 1 and cover(80, 93, -1, 0) == 0 and cover(80, 93, 1000, -1) == 0
    assert cover(80, 93, 16 * MAX_TILES, 10) == 1 and cover(80, 93, 16 * MAX_TILES + 1, 10) == 0
    for n in (1, 15, 16, 17, 1 << 31, (1 << 31) + 1, 1 << 40):
        assert cover(80, 93, n, 10) == wcover(80, 93, n, 10) == covers(80, 93, n, 10), n


NAMES = ("W_in", "w_stride", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "eps", "W_out", "flags", "retry",
         "stream")
NULLS = (None, 6400, 80, 0, 5, None, 0, None, None, None, 128, 93, 0.0, None, None, None, None)


def test_argument_validation_precedes_any_device_work(lib):
    def with_(fn=lib.mia_lienks_update_stream_f64, **kw):
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
    # the order of mia_lienks_update_matfun_f64, at a shape that entry knows (k = 4, p_max <= k)
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
    assert with_(p_max=80, **full) == -3 and with_(p_max=63, **full) == -3  # p_max <= k
    assert with_(p_cap=80, **full) == -3                                    # (p_max is cut to p_cap first)
    assert with_(p_cap=300, p_max=257, **full) == -3                        # more than 256 slots
    assert with_(k=129, w_stride=129 * 129, p_cap=200, p_max=139, **full) == -3      # ensemble size
    assert with_(k=129, w_stride=0, eps=1e-3, p_cap=200, p_max=139, **full) == -3
    assert with_(g1=16 * MAX_TILES + 1, **full) == -3                       # more tiles than a launch grid holds
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3 and with_(w_stride=0, eps=1e-3, **full) == -3      # the A/B switch of the tile routes
        assert with_(k=128, w_stride=128 * 128, p_cap=256, p_max=203, **full) == -3
        assert with_(**dict(full, flags=None)) == -1 and with_(k=1, **full) == -2     # (the order holds with the switch off)
    finally:
        lib.mia_set_option(b"tile", -1)


def test_the_general_kernels_lds_is_restated_byte_for_byte(engine_cls):
    lds, fits = engine_cls._ienks_general_lds_bytes, engine_cls._ienks_general_fits
    assert engine_cls.JACOBI_MAX_LDS == MAX_LDS == 162816
    for k, p, bundle, transform in DENSE_ROWS + SPARSE_ROWS:
        assert lds(k, p, 1.0, True) == bundle and lds(k, p, 1.0, False) == transform, (k, p)
        assert fits(k, p, 1.0, True) == (bundle <= MAX_LDS) and fits(k, p, 1.0, False) == (transform <= MAX_LDS), (k, p)
    assert fits(65, 77, 1.0, True) and fits(65, 77, 1.0, False) and fits(72, 77, 1.0, True) and not fits(72, 77, 1.0, False)
    # with p_max = k + 1: bundle refused from 80 members on, transform from 69
    assert [k for k in range(2, 129) if not fits(k, k + 1, 1.0, True)] == list(range(80, 129))
    assert [k for k in range(2, 129) if not fits(k, k + 1, 1.0, False)] == list(range(69, 129))
    # from 97 members on the bundle variant is refused for every list length (tests/test_gpu_ienks_wide64.py)
    assert lds(97, 1, 1.0, True) == 163632 and lds(96, 1, 1.0, True) == 157200
    # tau < 1 with p_max <= k takes the primal form: p_max rows, not the even count of the dual form
    assert lds(40, 19, 0.9, True) < lds(40, 19, 1.0, True) and lds(40, 41, 0.9, True) == lds(40, 41, 1.0, True)


def test_the_gate_of_the_classes(engine_cls):
    eng = engine_cls.__new__(engine_cls)            # (the gate reads class constants only: no device, no library)
    auto = eng._ienks_stream64_auto
    for bundle in (True, False):
        assert not auto(80, 93, bundle, False) or bundle           # per-point transform weights: never
        assert not auto(80, 80, bundle, True) and not auto(80, 63, bundle, True)        # p_max <= k
        assert not auto(128, 257, bundle, True)                    # more than 256 slots
        assert not auto(129, 139, bundle, True)                    # more than 128 members
        assert not auto(1, 5, bundle, True)
        assert not auto(20, 29, bundle, True)                      # the general kernel holds it and no measurement admits it
        assert auto(80, 93, bundle, True) and auto(128, 203, bundle, True)
    assert not auto(80, 93, False, False) and not auto(128, 203, False, False)
    assert auto(80, 93, True, False) and auto(128, 203, True, False) and auto(96, 107, True, False)
    # (a) where the general kernel cannot hold the shape; (b) the measured range
    assert auto(72, 77, False, True) and not engine_cls._ienks_general_fits(72, 77, 1.0, False)
    for k, p, bundle in ((65, 77, True), (65, 77, False), (72, 77, True), (40, 77, True)):
        assert engine_cls._ienks_general_fits(k, p, 1.0, bundle)
        inside = k >= engine_cls.IENKS_STREAM64_AUTO_MIN_K and \
            engine_cls.IENKS_STREAM64_AUTO_DEN * p <= engine_cls.IENKS_STREAM64_AUTO_NUM * k
        assert auto(k, p, bundle, True) == inside, (k, p, bundle)

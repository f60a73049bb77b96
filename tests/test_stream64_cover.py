"""The streamed dense float64 tile route (csrc/letkf_stream64.hip) without a GPU: the host-only cover function against its
arithmetic restated here, the LDS of a launch at 256 slots for every ensemble size, the declarations, and the argument
validation of mia_letkf_analysis_stream_f64, which returns before any HIP call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LDS = 160 * 1024 - 1024                     # kMaxDynamicLds (csrc/mia_common.h)
MAX_BLOCKS, MAX_K = 16, 128                     # kStream64MaxBlocks, kStream64MaxK


def _lib():
    import torch_assimilate_amd as m
    m.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def lds_bytes(ub, k):
    """Restates ring64_lds_bytes (csrc/mia_frames64.h): ring [2][16][kp | 1] + rhs [4 KT][64] + sqrt(rho) [16][16 ub + 1] doubles, slot table
    [16 ub] ints, rounded up to 16 bytes."""
    umax, kp, kt = 16 * ub, (k + 1 + 3) & ~3, (k + 15) >> 4
    b = (2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (umax + 1)) * 8 + umax * 4
    return (b + 15) // 16 * 16


def covers(m, k, p_max, ldx, ldo, ng, P=0):
    """Restates stream64_route_covers / mia_letkf_stream_f64_cover."""
    if P < 0 or m < 1 or k < 2 or k > MAX_K or p_max <= k or ldx < 1 or ldo < 1 or ng < 0:
        return 0
    if p_max > 16 * MAX_BLOCKS or lds_bytes(MAX_BLOCKS, k) > MAX_LDS:
        return 0
    if k * ldx * 8 >= 2 ** 31 or k * ldo * 8 >= 2 ** 31:
        return 0
    return 1 if ((ng + 15) >> 4) <= 65536 * 65535 else 0


def test_the_launch_holds_256_slots_at_every_ensemble_size():
    worst = max(lds_bytes(MAX_BLOCKS, k) for k in range(2, MAX_K + 1))
    assert worst == lds_bytes(MAX_BLOCKS, 128) == 84352
    for k in range(2, MAX_K + 1):
        assert lds_bytes(MAX_BLOCKS, k) <= MAX_LDS, k
        # the same 256 slots as a resident image (csrc/letkf_dense64.hip) would not fit from 65 members on
    assert (256 * (((128 + 4) & ~3) | 1) + 16 * 257) * 8 + 1024 > MAX_LDS


def test_cover_function_matches_its_restatement():
    cover = _lib().mia_letkf_stream_f64_cover
    for k in range(2, MAX_K + 1):
        for p_max in (k, k + 1, 256, 257):
            want = covers(1, k, p_max, 1000, 1000, 1000, 1000)
            assert want == (1 if k < p_max <= 256 else 0)
            assert cover(1, k, p_max, 1000, 1000, 1000, 1000) == want, (k, p_max)
    for args in [(3, 128, 203, 1000, 1000, 1000, 1000), (1, 129, 203, 1000, 1000, 1000, 1000), (1, 1, 3, 10, 10, 10, 10),
                 (0, 80, 93, 10, 10, 10, 10), (1, 80, 93, 0, 10, 10, 10), (1, 80, 93, 10, 0, 10, 10), (1, 80, 93, 10, 10, -1, 10),
                 (1, 80, 93, 10, 10, 10, -1), (1, 80, 93, 10, 10, 0, 0),
                 (1, 128, 139, 2 ** 21 - 1, 1000, 1000, 1000), (1, 128, 139, 2 ** 21, 1000, 1000, 1000),      # 128 ld 8 < 2^31
                 (1, 128, 139, 1000, 2 ** 21, 1000, 1000), (1, 80, 93, 100, 100, 16 * 65536 * 65535, 10),
                 (1, 80, 93, 100, 100, 16 * 65536 * 65535 + 1, 10)]:
        assert cover(*args) == covers(*args), args
    assert cover(1, 128, 139, 2 ** 21 - 1, 1000, 1000, 1000) == 1 and cover(1, 128, 139, 2 ** 21, 1000, 1000, 1000) == 0


def test_header_and_symbol_table_declare_both_entries():
    from torch_assimilate_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "mia_letkf.h")).read()
    for name in ("mia_letkf_analysis_stream_f64", "mia_letkf_stream_f64_cover"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _cabi.EXPORTED_SYMBOLS
        assert hasattr(_lib(), name)
    # the argument list of the dense entry
    assert _cabi._PROTOS["mia_letkf_analysis_stream_f64"] == _cabi._PROTOS["mia_letkf_analysis_dense_f64"]
    assert _cabi._PROTOS["mia_letkf_stream_f64_cover"] == _cabi._PROTOS["mia_letkf_dense_f64_cover"]


def test_argument_validation_precedes_any_device_work():
    call = _lib().mia_letkf_analysis_stream_f64
    tail = (None, 10, 0, None, None, None)
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, -1.0, 0.0, *tail) == -2      # inflation
    assert call(None, 10, 1, 1, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, *tail) == -2       # k < 2
    assert call(None, 10, 1, 4, 5, 0, None, 0, None, None, None, 8, 6, 1.0, 0.0, *tail) == -2       # g1 < g0
    assert call(None, 10, 1, 4, 0, 0, None, 0, None, None, None, 8, 6, 1.0, 0.0, *tail) == 0        # empty range
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.5, *tail) == -3       # gamma > 0
    assert call(None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 6, 1.0, 0.0, *tail) == -1       # NULL arrays

"""The float64 ensemble transform on tiles (csrc/apply_local64.hip) without a GPU: the host-only cover functions, the option
apply64, the slot of mia_last_transform_kernel, and the argument validation of mia_apply_local_weights_f64 /
mia_apply_weights_f64, which returns before any HIP call exactly what it returned before the tile kernels existed."""
import ctypes as C

import pytest

MAX_LDS = 160 * 1024 - 1024          # kMaxDynamicLds (csrc/mia_common.h)
NEW_SYMBOLS = ("mia_apply_local_f64_cover", "mia_apply_f64_cover", "mia_last_transform_kernel")


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def apply_local64_lds_bytes(k):
    """LDS of apply_local64_tile_kernel<ceil(k / 16)>, restated from csrc/apply_local64.hip: the image of EIGHT state rows,
    [row][member][point] in doubles with a row pitch of 16 kp + 1 (kp = k rounded up to a multiple of 4)"""
    kp = (k + 3) // 4 * 4
    return 8 * (16 * kp + 1) * 8


def last_ld(k):
    """the largest leading dimension the 32-bit lane offsets allow, restated from the kernels' addressing: a lane adds
    (member i * ld + point) * 8 bytes to a state row's 64-bit base, with i up to kp - 1 <= k + 2 while staging, so
    (k + 3) * ld * 8 has to stay below 2^32"""
    return (2 ** 32 - 1) // (8 * (k + 3))


def test_symbols_and_python_binding(lib):
    from torch_assimilate_amd import _cabi
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS, name
    assert callable(_cabi.last_transform_kernel)
    v = C.c_int(7)
    assert lib.mia_get_option(b"apply64", C.byref(v)) == 0 and v.value == -1          # the fourth new name: the option


@pytest.mark.parametrize("name", ["mia_apply_local_f64_cover", "mia_apply_f64_cover"])
def test_cover_values(lib, name):
    cover = getattr(lib, name)
    for k in (2, 3, 17, 40, 64, 65, 96, 128):
        for m in (1, 16, 70):
            assert cover(m, k, 100000, 100000, 100000) == 1, (m, k)
            assert cover(m, k, 1000, 37, 37) == 1, (m, k)
    for k in (1, 129, 0, -40):
        assert cover(1, k, 1000, 1000, 1000) == 0, k
    assert cover(0, 40, 1000, 1000, 1000) == 0 and cover(-1, 40, 1000, 1000, 1000) == 0
    assert cover(1, 40, 1000, 1000, 0) == 0 and cover(1, 40, 1000, 1000, -5) == 0
    assert cover(1, 40, -1000, 1000, 1000) == 0 and cover(1, 40, 1000, -1000, 1000) == 0
    assert cover(1, 40, 0, 1000, 1000) == 0 and cover(1, 40, 1000, 0, 1000) == 0


@pytest.mark.parametrize("name", ["mia_apply_local_f64_cover", "mia_apply_f64_cover"])
@pytest.mark.parametrize("k", [2, 40, 128])
def test_the_32_bit_offset_bound(lib, name, k):
    cover = getattr(lib, name)
    ld = last_ld(k)
    assert (k + 3) * ld * 8 < 2 ** 32 <= (k + 3) * (ld + 1) * 8
    assert cover(1, k, ld, ld, 1000) == 1
    assert cover(1, k, ld + 1, ld, 1000) == 0 and cover(1, k, ld, ld + 1, 1000) == 0


def test_the_image_fits_for_every_ensemble_size(lib):
    assert max(apply_local64_lds_bytes(k) for k in range(2, 129)) == apply_local64_lds_bytes(128) == 131136 <= MAX_LDS
    assert apply_local64_lds_bytes(40) == 41024                    # three workgroups per CU, the float32 kernel's footprint
    assert 3 * apply_local64_lds_bytes(40) <= 160 * 1024 < 4 * apply_local64_lds_bytes(40)
    for k in range(2, 129):
        assert lib.mia_apply_local_f64_cover(8, k, 4096, 4096, 4096) == 1, k


@pytest.mark.parametrize("name", ["mia_apply_local_weights_f64", "mia_apply_weights_f64"])
def test_argument_validation_precedes_any_device_work(lib, name):
    """The codes of apply_local_weights_impl / apply_weights_impl, in their order: sizes (-2), the empty shard (0), NULL (-1),
    leading dimensions (-2) -- whatever the option says."""
    call = getattr(lib, name)
    for opt in (-1, 1, 0):
        assert lib.mia_set_option(b"apply64", opt) == 0
        try:
            assert call(None, 10, 1, 1, 0, 5, None, None, 10, 0, None) == -2          # k < 2
            assert call(None, 10, 0, 4, 0, 5, None, None, 10, 0, None) == -2          # m < 1
            assert call(None, 10, 1, 4, 5, 3, None, None, 10, 0, None) == -2          # g1 < g0
            assert call(None, 10, 1, 4, -1, 3, None, None, 10, 0, None) == -2         # g0 < 0
            assert call(None, 10, 1, 4, 3, 3, None, None, 10, 0, None) == 0           # empty shard, before the NULL check
            assert call(None, 10, 1, 4, 0, 5, None, None, 10, 0, None) == -1          # NULL pointers
            buf = (C.c_double * 64)()
            ptr = C.cast(buf, C.c_void_p)
            assert call(ptr, 10, 1, 4, 0, 5, None, ptr, 10, 0, None) == -1
            assert call(ptr, 4, 1, 4, 0, 5, ptr, ptr, 10, 0, None) == -2              # ldx < g1
            assert call(ptr, 10, 1, 4, 0, 5, ptr, ptr, 4, 0, None) == -2              # ldo < o0 + ng
            assert call(ptr, 10, 1, 4, 0, 5, ptr, ptr, 6, 2, None) == -2
        finally:
            lib.mia_set_option(b"apply64", -1)


def test_option_apply64_is_three_valued(lib):
    v = C.c_int(9)
    try:
        for given, want in ((1, 1), (5, 1), (0, 0), (-1, -1), (-7, -1)):
            assert lib.mia_set_option(b"apply64", given) == 0
            assert lib.mia_get_option(b"apply64", C.byref(v)) == 0 and v.value == want, given
    finally:
        lib.mia_set_option(b"apply64", -1)
    assert lib.mia_get_option(b"tile", C.byref(v)) == 0 and v.value == 1       # (the on/off table is untouched)


def test_last_transform_kernel_buffer(lib):
    """as mia_last_analysis_kernel: NULL or no room is MIA_ERR_NULL, one byte holds the terminator, '' before any launch"""
    from torch_assimilate_amd import _cabi
    buf = C.create_string_buffer(b"xxxxxxx", 8)
    for fn in (lib.mia_last_transform_kernel, lib.mia_last_analysis_kernel):
        assert fn(None, 8) == -1 and fn(buf, 0) == -1 and fn(buf, -3) == -1
        assert buf.raw[:7] == b"xxxxxxx"
    assert lib.mia_last_transform_kernel(buf, 1) == 0 and buf.raw[0:1] == b"\0"
    name = _cabi.last_transform_kernel()                   # ('' unless a GPU test of this process has launched a transform)
    assert name == "" or "apply" in name

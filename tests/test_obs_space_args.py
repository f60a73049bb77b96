"""The observation-space entries (csrc/obs_space.hip) without a GPU: the return codes of mia_obs_space_uncorr_*, mia_obs_space_corr_*
and mia_obs_space_corr_workspace_bytes in the order the code checks them -- every one of them returns before any device work -- and
the byte count of the workspace."""
import ctypes as C

import pytest

OK, NULL, SIZE, UNSUPPORTED, WORKSPACE, ALIGN = 0, -1, -2, -3, -4, -5          # include/mia_letkf.h


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


@pytest.fixture(scope="module")
def mem():
    """a host address aligned to 256 bytes inside a buffer that outlives the module; no entry below gets as far as reading it"""
    buf = (C.c_char * 1024)()
    base = (C.addressof(buf) + 255) // 256 * 256
    return buf, base


def ws_bytes(k, P, elem):
    return ((P + k + 1) * max(P, 1) * elem + 255) // 256 * 256


def test_workspace_bytes(lib):
    n = C.c_size_t(7)
    fn = lib.mia_obs_space_corr_workspace_bytes
    assert fn(5, 10, 8, None) == NULL
    assert fn(0, 10, 8, C.byref(n)) == SIZE and fn(5, -1, 8, C.byref(n)) == SIZE
    for elem in (0, 2, 16):
        assert fn(5, 10, elem, C.byref(n)) == SIZE
    assert n.value == 7
    for k, P in ((1, 0), (1, 1), (7, 33), (40, 300), (128, 97), (3, 330), (40, 46000), (5, 46001)):
        for elem in (4, 8):
            assert fn(k, P, elem, C.byref(n)) == OK and n.value == ws_bytes(k, P, elem), (k, P, elem)
    assert ws_bytes(7, 33, 8) == 11008 and ws_bytes(1, 0, 4) == 256 and ws_bytes(1, 1, 4) == 256


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_uncorr_codes_in_their_order(lib, mem, sfx):
    call = getattr(lib, "mia_obs_space_uncorr_" + sfx)
    p = mem[1]
    # sizes first, whatever the pointers
    assert call(None, 10, None, None, 0, 10, None, 10, None, None, None) == SIZE            # k < 1
    assert call(None, 10, None, None, 5, -1, None, 10, None, None, None) == SIZE            # P < 0
    assert call(None, 9, None, None, 5, 10, None, 10, None, None, None) == SIZE             # ldh < P
    assert call(None, 10, None, None, 5, 10, p, 9, None, None, None) == SIZE                # Yb with ldy < P
    assert call(p, 10, p, p, 5, 10, p, 9, p, p, None) == SIZE
    # P == 0 is complete, NULL pointers or not, and before the alignment of rec
    assert call(None, 0, None, None, 5, 0, None, 0, None, None, None) == OK
    assert call(None, 0, None, None, 5, 0, None, 0, None, p + 4, None) == OK
    # ldy is not looked at without Yb: NULL inputs come next
    assert call(None, 10, None, None, 5, 10, None, 0, None, None, None) == NULL
    for hx, y, var in ((None, p, p), (p, None, p), (p, p, None)):
        assert call(hx, 10, y, var, 5, 10, p, 10, p, p + 4, None) == NULL                  # (before the alignment of rec)
    # rec on 16 bytes
    for off in (4, 8, 12):
        assert call(p, 10, p, p, 5, 10, None, 0, None, p + off, None) == ALIGN
    # more workgroups than a grid has: 32 observations each
    big = 32 * (2 ** 31 - 1) + 1
    assert call(p, big, p, p, 5, big, None, 0, None, None, None) == UNSUPPORTED
    assert call(p, big, p, p, 5, big, None, 0, None, p + 4, None) == ALIGN                  # (alignment before it)


@pytest.mark.parametrize("sfx,elem", [("f32", 4), ("f64", 8)])
def test_corr_codes_in_their_order(lib, mem, sfx, elem):
    call = getattr(lib, "mia_obs_space_corr_" + sfx)
    p = mem[1]
    need = (10 + 5 + 1) * 10 * elem
    assert call(None, 10, None, None, 0, 10, None, 10, None, None, None, None, 0, None) == SIZE      # k < 1
    assert call(None, 10, None, None, 5, -1, None, 10, None, None, None, None, 0, None) == SIZE      # P < 0
    assert call(None, 9, None, None, 5, 10, None, 10, None, None, None, None, 0, None) == SIZE       # ldh < P
    assert call(None, 10, None, None, 5, 10, p, 9, None, None, None, None, 0, None) == SIZE          # Yb with ldy < P
    assert call(None, 0, None, None, 5, 0, None, 0, None, None, None, None, 0, None) == OK           # P == 0
    assert call(None, 0, None, None, 5, 0, None, 0, None, None, None, p + 1, 0, None) == OK
    assert call(None, 10, None, None, 5, 10, None, 0, None, None, None, None, 0, None) == NULL
    for hx, y, cov, ws in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert call(hx, 10, y, cov, 5, 10, None, 0, None, None, None, ws, 0, None) == NULL
    assert call(None, 10, p, p, 5, 10, None, 0, None, None, None, p + 1, 0, None) == NULL            # (before the alignment)
    for off in (1, 16, 128):
        assert call(p, 10, p, p, 5, 10, None, 0, None, None, None, p + off, 2 ** 40, None) == ALIGN
    assert call(p, 10, p, p, 5, 10, None, 0, None, None, None, p + 128, 0, None) == ALIGN            # (before the size)
    for given in (0, need - 1):
        assert call(p, 10, p, p, 5, 10, None, 0, None, None, None, p, given, None) == WORKSPACE
    # what the entry needs is the unrounded product; what mia_obs_space_corr_workspace_bytes gives covers it
    assert need <= ws_bytes(5, 10, elem) < need + 256
    # beyond 46000 observations: unsupported once the claimed workspace is large enough, a short workspace is reported first
    P = 46001
    assert call(p, P, p, p, 5, P, None, 0, None, None, None, p, (P + 6) * P * elem - 1, None) == WORKSPACE
    assert call(p, P, p, p, 5, P, None, 0, None, None, None, p, 2 ** 40, None) == UNSUPPORTED
    assert call(p, P, p, p, 5, P, p, P, p, p, p, p, 2 ** 40, None) == UNSUPPORTED

"""The float64 kernel-expression tile route (csrc/lketkf_kern64.hip: LKETKF with any positive semidefinite kernel or composition in
the default dtype) without a GPU: the three symbols, the host-only cover function, the argument validation of
mia_lketkf_kernel_analysis_matfun_f64, which returns before any HIP call, and the classification that decides the route
(kernels.kernel_is_psd)."""
import ctypes as C

import pytest

from kernel_cases import product_kernels

SYMBOLS = ("mia_lketkf_kernel_analysis_matfun_f64", "mia_lketkf_kernel_analysis_retry_f64", "mia_lketkf_kernel_f64_cover")


@pytest.fixture(scope="module")
def lib():
    import torch_assimilate_amd as mia
    mia.build()
    from torch_assimilate_amd import _cabi
    return _cabi.lib()


def program(*ops):
    from torch_assimilate_amd._cabi import KernelOp
    arr = (KernelOp * max(len(ops), 1))()
    for i, (op, val) in enumerate(ops):
        arr[i].op, arr[i].value = op, val
    return arr


def test_symbols_and_cover(lib):
    from torch_assimilate_amd import _cabi
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _cabi.EXPORTED_SYMBOLS
    cover, rbf = lib.mia_lketkf_kernel_f64_cover, lib.mia_lketkf_rbf_f64_cover
    grid = [(1, 40, 20, 100000, 100000, 100000, 50000), (3, 2, 5, 1000, 1000, 1000, 10),
            (1, 41, 20, 1000, 1000, 1000, 10), (1, 65, 20, 1000, 1000, 1000, 10), (1, 1, 1, 1000, 1000, 1000, 10),
            (1, 40, 65, 1000, 1000, 1000, 10), (1, 40, 20, 1000, 1000, 1000, -1), (0, 40, 20, 1000, 1000, 1000, 10),
            (1, 40, -1, 1000, 1000, 1000, 10), (1, 40, 20, 0, 1000, 1000, 10), (1, 40, 20, 1000, 0, 1000, 10),
            (1, 40, 20, 1000, 1000, -1, 10)]
    for k, p in ((40, 59), (40, 64), (20, 33), (8, 35), (17, 15), (2, 0)):
        grid += [(1, k, p, 1000, 1000, 1000, 1000), (8, k, p, 1000, 1000, 1000, 1000)]
    for a in grid:
        assert cover(*a) == rbf(*a), a
    assert cover(*grid[0]) == 1 and cover(*grid[2]) == 0 and cover(*grid[5]) == 0 and cover(*grid[6]) == 0
    assert cover(1, 40, 64, 1000, 1000, 1000, 1000) == 1


def test_argument_validation_precedes_any_device_work(lib):
    call = lib.mia_lketkf_kernel_analysis_matfun_f64
    poly2 = program((1, 0.0), (4, 1.0), (6, 0.0), (4, 2.0), (8, 0.0))
    null = (None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0, poly2, 5, None, 10, 0, None, None, None)
    names = ("X", "ldx", "m", "k", "g0", "g1", "rec", "P", "cnt", "idx", "w", "p_cap", "p_max", "inf", "prog", "n_ops", "Xa", "ldo",
             "o0", "flags", "retry", "stream")

    def with_(fn=call, **kw):
        a = dict(zip(names, null))
        a.update(kw)
        return fn(*[a[n] for n in names])
    assert with_(inf=-1.0) == -2 and with_(inf=0.0) == -2
    # the program check stands where the RBF entry checks gamma: the codes of kernel_program_check
    assert with_(n_ops=0) == -2 and with_(prog=None) == -1
    assert with_(prog=program((99, 0.0)), n_ops=1) == -2                       # unknown opcode
    assert with_(prog=program((6, 0.0)), n_ops=1) == -2                        # operator without operands
    assert with_(prog=program((1, 0.0), (2, 0.0)), n_ops=2) == -2              # two values left
    assert with_(prog=program(*[(4, 1.0)] * 7 + [(6, 0.0)] * 6), n_ops=13) == -3   # deeper than the operand stack
    assert with_(n_ops=0, g1=0) == -2                                          # (before the empty-shard answer)
    assert with_(k=1, g1=0) == -2                                              # (sizes before it as well)
    assert with_(g1=0) == 0                                                    # empty shard
    assert with_() == -1                                                       # NULL state
    assert with_(k=1) == -2 and with_(m=0) == -2 and with_(g1=-1) == -2 and with_(p_cap=0) == -2 and with_(P=-1) == -2
    # with every pointer present: sizes, then the cover (nothing is dereferenced before it)
    buf = (C.c_double * 64)()
    ptr = C.cast(buf, C.c_void_p)
    full = dict(X=ptr, rec=ptr, cnt=ptr, idx=ptr, w=ptr, Xa=ptr, flags=ptr, retry=ptr)
    assert with_(ldx=4, **full) == -2 and with_(ldo=4, **full) == -2           # leading dimensions shorter than the shard
    assert with_(k=41, **full) == -3                                           # ensemble size
    assert with_(p_cap=72, p_max=65, **full) == -3                             # list length
    assert with_(rec=None, P=3, **dict((n, v) for n, v in full.items() if n != "rec")) == -1
    tanh = program((1, 0.0), (10, 0.0))
    sin = program((3, 0.0), (11, 0.0))
    assert with_(prog=tanh, n_ops=2, **full) == -3 and with_(prog=sin, n_ops=2, **full) == -3
    lib.mia_set_option(b"tile", 0)
    try:
        assert with_(**full) == -3                                             # the A/B switch of the tile routes
    finally:
        lib.mia_set_option(b"tile", -1)
    # the redo entry: flags required, then the program check, then the Jacobi entry's validation
    retry = lib.mia_lketkf_kernel_analysis_retry_f64
    base = (None, 10, 1, 4, 0, 5, None, 0, None, None, None, 8, 4, 1.0)
    assert retry(*base, poly2, 5, None, 10, 0, None, None) == -1
    assert retry(*base, poly2, 0, None, 10, 0, ptr, None) == -2
    assert retry(*base[:5], 0, *base[6:], poly2, 5, None, 10, 0, ptr, None) == 0          # empty shard
    assert retry(*base, poly2, 5, None, 10, 0, ptr, None) == -1                            # NULL state


def test_positive_semidefinite_classification():
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import kernels as K
    prod = product_kernels()
    for name, kern in prod.items():
        assert K.kernel_is_psd(kern) == (name not in ("tanh", "periodic")), name
        assert kern.is_psd == K.kernel_is_psd(kern)
    for kern in (K.LinearKernel(), K.GaussKernel(2.0), K.RBFKernel(0.5), K.RationalKernel(1.0, 0.5), K.OrnsteinUhlenbeckKernel(3.0),
                 K.ScaleKernel(0.0), K.DiagKernel(0.0), K.PolyKernel(1.0, 0.0), K.PolyKernel(3.0, 0.5),
                 K.RationalKernel(1.0, 1.0) ** K.ScaleKernel(3.0), (K.LinearKernel() + K.DiagKernel(0.1)) * K.RBFKernel(2.0)):
        assert K.kernel_is_psd(kern), repr(kern)
    for kern in (K.PolyKernel(2.5, 1.0), K.PolyKernel(2.0, -1.0), K.PolyKernel(0.0, 1.0), K.PolyKernel(-1.0, 1.0), K.ScaleKernel(-1.0),
                 K.DiagKernel(-0.1), K.RationalKernel(1.0, 0.0), K.RationalKernel(1.0, -1.0), K.OrnsteinUhlenbeckKernel(-2.0),
                 K.RationalKernel(1.0, 1.0) ** K.ScaleKernel(1.5), K.RationalKernel(1.0, 1.0) ** K.ScaleKernel(0.0),
                 K.RationalKernel(1.0, 1.0) ** K.ScaleKernel(-2.0), K.RBFKernel(0.5) ** K.RBFKernel(0.5),
                 K.RBFKernel(0.5) ** K.DiagKernel(2.0), K.TanhKernel(0.05, 0.1), K.PeriodicKernel(7.0, 1.5),
                 K.RBFKernel(0.5) + K.TanhKernel(0.05, 0.1), K.PeriodicKernel(7.0, 1.5) * K.ScaleKernel(2.0),
                 K.TanhKernel(0.05, 0.1) ** K.ScaleKernel(2.0), K.LinearKernel() + K.ScaleKernel(-0.5),
                 (K.RBFKernel(0.5) + K.PolyKernel(2.5, 1.0)) * K.ScaleKernel(1.0)):
        assert not K.kernel_is_psd(kern), repr(kern)
    assert not K.kernel_is_psd(None) and not K.kernel_is_psd(object())
    assert not K.BaseKernel().is_psd                      # conservative: a kernel that does not say so is not

    # the classes hand the classification on with the program, and only with it (kernel_route's return shape stays)
    loc = mia.GaspariCohn(10.0, mia.AbsoluteDistance())
    ka = mia.LKETKF(prod["poly2"], localization=loc)._kernel_args()
    assert ka["kernel_psd"] is True and ka["rbf_gamma"] is None and len(ka["kernel_program"]) == 5
    assert mia.LKETKF(prod["tanh"], localization=loc)._kernel_args()["kernel_psd"] is False
    assert mia.LKETKF(prod["periodic"], localization=loc)._kernel_args()["kernel_psd"] is False
    assert mia.LKETKF(K.RBFKernel(0.5), localization=loc)._kernel_args() == dict(rbf_gamma=0.5, kernel_program=None)
    assert K.kernel_route(prod["poly2"]) == (None, prod["poly2"].program())

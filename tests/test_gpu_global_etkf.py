"""The global (unlocalised) routes of csrc/etkf_global.hip against the float64 oracle across ensemble sizes, observation
counts, data scales and both dtypes: LetkfEngine.etkf_weights / ketkf_weights / apply_weights, KETKFModule, and the
drop-in ETKF / KETKF classes.

ch below is the observation chunk of one Gram slab (gram_chunk in csrc/etkf_global.hip, restated by ``chunk``): P around
ch and its multiples reaches the second and later slabs.  k = 98 / 99 (float64) and 140 / 141 (float32) are the edges
where the solve's A and V leave LDS for the workspace; 114 / 115 (float64) and 172 / 173 (float32) those where the
transform's W leaves LDS.  Odd k takes the solve's padded row.

Bars: float64 W <= 1e-10 (ETKF) / 1e-9 (KETKF, kernel functions from the device libm); float32 W <= 5e-5 (the raw-weights
bar of test_gpu_kernels.py).  Where float32 accumulation of a large Gram dominates W -- P >= 1e5, or perturbations of
size 1e3 -- the weights' error is printed and the bars are on the analysis (<= 1e-5) and its increments (<= 1e-4).

Perturbations of size 1e3 make W ill-conditioned in ANY precision: the Gram's rounding, a unit roundoff of its largest
eigenvalue (~1e6 P), lands on eigenvalues near zero -- the members' mean direction, and the null space when P < k - 1 --
where W is sqrt((k - 1) / (lambda + (k - 1) / inf)).  In float64 the oracle itself moves by 1e-10 .. 6e-10 when only the
order of the observations changes, so those rows bar W at 20x that reordering floor, measured per case.  In float32 the
same rounding is ~1e-1 of the regularisation (torch's float32 Gram + eigh: W off by 0.2 - 0.4): only a full-rank block,
whose null space is the mean direction that the analysis discards, has a meaningful float32 analysis.
"""
import sys
import time

import numpy as np
import pytest
import torch

from conftest import rel_fro
from kernel_cases import KERNEL_NAMES, oracle_kernels, product_kernels
from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TAG = {F32: "f32", F64: "f64"}


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine("cuda:0")


def chunk(k, dtype):
    """Observations per Gram slab: gram_chunk of csrc/etkf_global.hip (256 for float32 at k = 40, 192 for float64)."""
    eb = 4 if dtype == F32 else 8
    ch = 65536 // ((k + 1) * eb) - 1
    return min(max(ch // 32 * 32, 32), 256)


def obs_count(spec, k, dtype):
    ch = chunk(k, dtype)
    return int(eval(spec, {"k": k, "ch": ch}))


def make_block(k, P, dtype, seed, scale=1.0, innov=1.0):
    """Centred perturbations (k, P) of size ``scale`` and innovations ``innov`` spreads large, rounded to ``dtype``;
    returned as the device tensors and the float64 values the oracle sees."""
    rs = np.random.RandomState(seed)
    yb = rs.normal(size=(k, P)) * scale
    yb -= yb.mean(axis=0)
    d = rs.normal(size=P) * scale * innov
    yb_t, d_t = torch.tensor(yb, dtype=dtype), torch.tensor(d, dtype=dtype)
    return yb_t.cuda(), d_t.cuda(), yb_t.double(), d_t.double()


def analysis_errors(W, ref, k, seed):
    """Relative errors of the analysis xa = mean + X' W and of its increments xa - X on a seeded state, W on the host."""
    X = np.random.RandomState(seed + 1).normal(size=(2, k, 64))
    ag, ar = O.apply_weights(X, np.asarray(W, dtype=np.float64)), O.apply_weights(X, ref)
    return rel_fro(ag, ar), rel_fro(ag - X, ar - X)


def prior(k, inf, dtype):
    """sqrt(inf) I as the kernel forms it: sqrt of the inflation in the working precision."""
    if dtype == F32:
        return np.float32(np.sqrt(np.float32(inf))) * np.eye(k, dtype=np.float32)
    return np.sqrt(inf) * np.eye(k)


# (k, P as an expression of k and ch, inflation, perturbation size, innovation size in spreads): every row in both dtypes
ETKF_ROWS = [
    (2, "0", 1.0, 1.0, 1.0), (2, "1", 1.1, 1.0, 1.0), (3, "k-2", 1.1, 1.0, 1.0), (5, "k-1", 1.0, 1.0, 1.0),
    (5, "ch-1", 1.1, 1e-3, 1.0), (20, "ch+1", 1.1, 1.0, 100.0), (40, "ch", 1.0, 1.0, 1.0), (40, "3*ch+5", 1.1, 1.0, 1.0),
    (64, "20000", 1.1, 1.0, 1.0), (96, "k+1", 1.0, 1.0, 1.0), (97, "ch+1", 1.1, 1.0, 1.0), (98, "k-2", 1.1, 1.0, 1.0),
    (99, "k-1", 1.0, 1.0, 1.0), (128, "3*ch+5", 1.1, 1.0, 1.0), (140, "ch-1", 1.1, 1.0, 1.0),
    (141, "k+1", 1.0, 1.0, 1.0), (200, "ch", 1.1, 1e-3, 1.0), (200, "k-2", 1.0, 1.0, 100.0),
    (256, "20000", 1.1, 1.0, 1.0), (256, "0", 1.1, 1.0, 1.0), (256, "ch+1", 1.0, 1.0, 1.0),
]
# float64, perturbations of size 1e3: W barred at 20x the oracle's own reordering floor (module docstring)
ETKF_ROWS_F64_LARGE = [(40, "ch+1", 1.1, 1e3, 100.0), (128, "k+1", 1.0, 1e3, 1.0), (99, "ch", 1.1, 1e3, 1.0)]
# float32 rows gated on the analysis and its increments: W's error is printed.  Size 1e3 on full-rank blocks only.
ETKF_ROWS_F32_ANALYSIS = [(40, "100000", 1.1, 1.0, 1.0), (40, "500000", 1.1, 1.0, 1.0), (40, "ch+1", 1.1, 1e3, 100.0),
                          (141, "3*ch+5", 1.0, 1e3, 1.0)]


def _etkf_params():
    out = []
    for dtype in (F64, F32):
        for r in ETKF_ROWS:
            out.append((dtype,) + r)
    return [pytest.param(*p, id="%s-k%d-P=%s(ch=%d)-inf%g-s%g-d%g" % (TAG[p[0]], p[1], p[2], chunk(p[1], p[0]), p[3], p[4],
                                                                       p[5])) for p in out]


@pytest.mark.parametrize("dtype,k,pspec,inf,scale,innov", _etkf_params())
def test_etkf_weights_vs_oracle(eng, dtype, k, pspec, inf, scale, innov):
    P = obs_count(pspec, k, dtype)
    yb, d, yb64, d64 = make_block(k, P, dtype, seed=1000 * k + P % 997, scale=scale, innov=innov)
    W, flags = eng.etkf_weights(yb, d, inf, return_flags=True)
    assert W.dtype == dtype and tuple(W.shape) == (k, k)
    assert int(flags.item()) == 0
    if P == 0:
        np.testing.assert_array_equal(W.cpu().numpy(), prior(k, inf, dtype))
        return
    ref = O.etkf_weights(yb64, d64, inf).numpy()
    err = rel_fro(W.cpu().numpy(), ref)
    print("etkf %s k=%d P=%d ch=%d: W rel. error %.2e" % (TAG[dtype], k, P, chunk(k, dtype), err))
    assert err < (1e-10 if dtype == F64 else 5e-5)


@pytest.mark.parametrize("k,pspec,inf,scale,innov", [pytest.param(*r, id="k%d-P=%s(ch=%d)-s%g" % (r[0], r[1], chunk(r[0], F64), r[3]))
                                                     for r in ETKF_ROWS_F64_LARGE])
def test_etkf_weights_f64_large_perturbations(eng, k, pspec, inf, scale, innov):
    P = obs_count(pspec, k, F64)
    yb, d, yb64, d64 = make_block(k, P, F64, seed=1000 * k + P % 997, scale=scale, innov=innov)
    W, flags = eng.etkf_weights(yb, d, inf, return_flags=True)
    assert int(flags.item()) == 0
    ref = O.etkf_weights(yb64, d64, inf).numpy()
    floor = max(rel_fro(O.etkf_weights(yb64[:, perm], d64[perm], inf).numpy(), ref)
                for perm in (np.random.RandomState(s).permutation(P) for s in (0, 1)))
    err = rel_fro(W.cpu().numpy(), ref)
    print("etkf f64 k=%d P=%d scale=%g: W rel. error %.2e, oracle reordering floor %.2e" % (k, P, scale, err, floor))
    assert err < max(1e-10, 20 * floor)


@pytest.mark.parametrize("k,pspec,inf,scale,innov", [pytest.param(*r, id="k%d-P=%s(ch=%d)-s%g" % (r[0], r[1], chunk(r[0], F32), r[3]))
                                                     for r in ETKF_ROWS_F32_ANALYSIS])
def test_etkf_weights_f32_analysis(eng, k, pspec, inf, scale, innov):
    P = obs_count(pspec, k, F32)
    yb, d, yb64, d64 = make_block(k, P, F32, seed=7 * k + P % 991, scale=scale, innov=innov)
    W, flags = eng.etkf_weights(yb, d, inf, return_flags=True)
    assert int(flags.item()) == 0
    ref = O.etkf_weights(yb64, d64, inf).numpy()
    w_err = rel_fro(W.cpu().numpy(), ref)
    a_err, i_err = analysis_errors(W.cpu().numpy(), ref, k, seed=P)
    print("etkf f32 k=%d P=%d scale=%g: W %.2e, analysis %.2e, increments %.2e" % (k, P, scale, w_err, a_err, i_err))
    assert a_err < 1e-5 and i_err < 1e-4


def test_etkf_weights_deterministic(eng):
    """The slab sum runs in a fixed order: the same call twice is bitwise equal, on the LDS and the workspace solve."""
    for k, P, dtype in ((40, 3 * chunk(40, F64) + 5, F64), (256, 2000, F32), (128, 1000, F64)):
        yb, d, _, _ = make_block(k, P, dtype, seed=k)
        a = eng.etkf_weights(yb, d, 1.1)
        b = eng.etkf_weights(yb, d, 1.1)
        assert torch.equal(a, b), (k, dtype)


def test_etkf_solve_time_k256(eng):
    """Wall time of one k = 256 solve (Gram + eigensolve + weights) per dtype: printed, not gated."""
    for dtype in (F32, F64):
        yb, d, _, _ = make_block(256, 20000, dtype, seed=3)
        eng.etkf_weights(yb, d, 1.1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            eng.etkf_weights(yb, d, 1.1)
        torch.cuda.synchronize()
        print("etkf %s k=256 P=20000: %.1f ms per solve" % (TAG[dtype], (time.perf_counter() - t0) / 3 * 1e3))


# (k, P expression): every kernel family of tests/kernel_cases.py appears in both dtypes
KETKF_ROWS = [(2, "1"), (5, "ch-1"), (40, "ch+1"), (40, "5000"), (97, "ch+1"), (128, "ch-1"), (200, "5000"), (200, "1")]


def _ketkf_params():
    out, i = [], 0
    for dtype in (F64, F32):
        for k, pspec in KETKF_ROWS:
            names = [KERNEL_NAMES[(i + j) % len(KERNEL_NAMES)] for j in range(3)]
            i += 3
            out.append(pytest.param(dtype, k, pspec, names, id="%s-k%d-P=%s(ch=%d)" % (TAG[dtype], k, pspec, chunk(k, dtype))))
    return out


@pytest.mark.parametrize("dtype,k,pspec,names", _ketkf_params())
def test_ketkf_weights_vs_oracle(mia, eng, dtype, k, pspec, names):
    P = obs_count(pspec, k, dtype)
    yb, d, yb64, d64 = make_block(k, P, dtype, seed=31 * k + P, scale=0.05)
    ora, prod = oracle_kernels(), product_kernels()
    tol = 1e-9 if dtype == F64 else 5e-5
    for name in names:
        ref = O.ketkf_weights(yb64, d64, ora[name], 1.1).numpy()
        got = mia.KETKFModule(prod[name], 1.1, eng)(yb, d)
        assert got.dtype == dtype
        err = rel_fro(got.cpu().numpy(), ref)
        print("ketkf %s k=%d P=%d %s: W rel. error %.2e" % (TAG[dtype], k, P, name, err))
        assert err < tol, name
        W, flags = eng.ketkf_weights(yb, d, prod[name].program(), 1.1, return_flags=True)
        assert int(flags.item()) == 0 and rel_fro(W.cpu().numpy(), ref) < tol, name


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("k", [2, 5, 40, 97, 128, 200])
def test_ketkf_empty_block_is_inflated_prior(mia, eng, dtype, k):
    prod = product_kernels()
    W, flags = eng.ketkf_weights(torch.zeros((k, 0), dtype=dtype), torch.zeros(0, dtype=dtype), prod["poly2"].program(),
                                 1.3, return_flags=True)
    assert int(flags.item()) == 0
    np.testing.assert_array_equal(W.cpu().numpy(), prior(k, 1.3, dtype))


def test_ketkf_deterministic(eng):
    prod = product_kernels()
    for k, dtype in ((40, F64), (200, F32)):
        yb, d, _, _ = make_block(k, 5000, dtype, seed=k, scale=0.05)
        a = eng.ketkf_weights(yb, d, prod["rbf_plus_diag"].program(), 1.1)
        b = eng.ketkf_weights(yb, d, prod["rbf_plus_diag"].program(), 1.1)
        assert torch.equal(a, b), (k, dtype)


@pytest.mark.parametrize("dtype,k,m,G", [(F64, 97, 3, 333), (F64, 114, 1, 1000), (F64, 115, 3, 259), (F64, 128, 1, 333),
                                         (F64, 256, 3, 130), (F32, 97, 1, 333), (F32, 128, 3, 1000), (F32, 172, 1, 259),
                                         (F32, 173, 3, 333), (F32, 256, 1, 130)])
def test_apply_global_weights_large_k(eng, dtype, k, m, G):
    """The global transform past its old LDS edges (W in LDS up to k = 114 / 172, then read from global memory)."""
    rs = np.random.RandomState(k + G)
    X, W = rs.normal(size=(m, k, G)), rs.normal(size=(k, k)) / np.sqrt(k)
    X[0] += 300.0                                # (a variable with a large mean: the transform works on perturbations)
    Xt, Wt = torch.tensor(X, dtype=dtype), torch.tensor(W, dtype=dtype)
    X64, W64 = Xt.double().numpy(), Wt.double().numpy()
    tol = 1e-14 if dtype == F64 else 1e-6
    got = eng.apply_weights(Xt, Wt)
    ref = O.apply_weights(X64, W64)
    assert rel_fro(got.cpu().numpy(), ref) < tol
    assert rel_fro(got.cpu().numpy()[0] - 300.0, ref[0] - 300.0) < 100 * tol
    for g0, g1 in ((0, 1), (5, 69), (G // 2, G)):
        sub = eng.apply_weights(Xt, Wt, g0, g1)
        np.testing.assert_array_equal(sub.cpu().numpy(), got.cpu().numpy()[:, :, g0:g1])


@pytest.mark.parametrize("k", [128, 256])
def test_etkf_analyse_arrays_f64_large_ensemble(mia, eng, k):
    rs = np.random.RandomState(k)
    P = 1500
    hx = rs.normal(size=(k, P))
    yb, d = hx - hx.mean(axis=0), rs.normal(size=P)
    state = rs.normal(size=(2, k, 300))
    xa = mia.ETKF(inf_factor=1.1, dtype=F64, engine=eng).analyse_arrays(state, yb, d)
    ref = O.apply_weights(state, O.etkf_weights(yb, d, 1.1).numpy())
    assert rel_fro(xa.cpu().numpy(), ref) < 1e-10


def test_ketkf_rbf_analyse_arrays_f32_k128(mia, eng):
    from torch_assimilate_amd import kernels as K
    rs = np.random.RandomState(128)
    k, P = 128, 3000
    hx = rs.normal(size=(k, P)) * 0.05
    yb, d = hx - hx.mean(axis=0), rs.normal(size=P) * 0.05
    yb32, d32 = yb.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64)
    state = rs.normal(size=(1, k, 200)).astype(np.float32).astype(np.float64)
    xa = mia.KETKF(K.RBFKernel(0.5), inf_factor=1.0, dtype=F32, engine=eng).analyse_arrays(state, yb, d)
    ref = O.apply_weights(state, O.ketkf_weights(yb32, d32, lambda x, y: O.rbf_kernel(x, y, 0.5), 1.0).numpy())
    assert rel_fro(xa.cpu().numpy(), ref) < 1e-5


@pytest.mark.parametrize("dtype", [F64, F32])
def test_global_routes_refuse_past_k256(mia, eng, dtype):
    """Past the stated range (2 <= k <= 256) every global entry refuses with MIA_ERR_UNSUPPORTED; k = 256 still runs."""
    prod = product_kernels()
    for k in (257, 300):
        yb, d, _, _ = make_block(k, 40, dtype, seed=k)
        with pytest.raises(mia.MiaError, match="status -3"):
            eng.etkf_weights(yb, d, 1.0)
        with pytest.raises(mia.MiaError, match="status -3"):
            eng.ketkf_weights(yb, d, prod["poly2"].program(), 1.0)
        with pytest.raises(mia.MiaError, match="status -3"):
            eng.apply_weights(torch.ones((1, k, 70), dtype=dtype), torch.eye(k, dtype=dtype))
    yb, d, _, _ = make_block(256, 40, dtype, seed=256)
    assert tuple(eng.etkf_weights(yb, d, 1.0).shape) == (256, 256)


def test_noconv_flag_warns(mia, eng, monkeypatch):
    """ETKF, KETKF and KETKFModule turn MIA_FLAG_NOCONV of the global solve into a RuntimeWarning (the flag read is
    patched: non-convergence is not provoked on the device)."""
    from torch_assimilate_amd import kernels as K
    E = sys.modules[type(eng).__module__]
    rs = np.random.RandomState(4)
    k, P = 12, 50
    hx = rs.normal(size=(k, P))
    yb, d, state = hx - hx.mean(axis=0), rs.normal(size=P), rs.normal(size=(1, k, 10))
    calls = []

    def read(flags):
        calls.append(int(flags[0].item()))
        return E.MIA_FLAG_NOCONV

    monkeypatch.setattr(E, "_read_solve_flags", read)
    with pytest.warns(RuntimeWarning, match="sweep cap"):
        mia.ETKF(inf_factor=1.1, dtype=F64, engine=eng).analyse_arrays(state, yb, d)
    with pytest.warns(RuntimeWarning, match="sweep cap"):
        mia.KETKF(K.RBFKernel(0.5), inf_factor=1.1, dtype=F32, engine=eng).analyse_arrays(state, yb, d)
    with pytest.warns(RuntimeWarning, match="sweep cap"):
        mia.KETKFModule(product_kernels()["poly2"], 1.1, eng)(torch.tensor(yb), torch.tensor(d))
    assert calls == [0, 0, 0]                    # (the real flags of these solves: converged)
    monkeypatch.undo()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        mia.ETKF(inf_factor=1.1, dtype=F64, engine=eng).analyse_arrays(state, yb, d)

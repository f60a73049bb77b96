"""Cases, referee and tolerance of the observation-space preparation (csrc/obs_space.hip), shared by tests/test_obs_space_reference.py
(CPU) and tests/test_gpu_obs_space.py.  Needs numpy and scipy only.

The referee ``reference`` works in numpy.longdouble (x87 extended, eps 1.1e-19): an unblocked column Cholesky of [R; V] with the value
rows appended below R, so V L^-T falls out of the same column sweep by forward substitution.  No inverse, no LAPACK.
``restatement`` is the same mathematics in the working dtype through LAPACK; it says what a correct implementation of that
precision achieves and is used only to size tolerances: a device result may be ``FACTOR`` = 32 times as far from the referee as the
restatement is, and never beyond the project's bars.  Inputs are rounded to the working dtype before either sees them, so that the
figures measure arithmetic, not the rounding of the inputs."""
import functools

import numpy as np
import pytest

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:
    pytest.skip("numpy.longdouble is no wider than float64 on this platform", allow_module_level=True)

BAR_CORR = {np.float64: 1e-11, np.float32: 2e-4}        # the project's bars (tests/test_gpu_interface.py)
BAR_UNCORR = {np.float64: 1e-13, np.float32: 2e-6}
FACTOR = 32.0       # a blocked right-looking sweep sums in another order than LAPACK's; a lost rank update leaves errors of order 1
ROOM = 4.0          # what the restatement has to leave under the bar: the same room for another summation order where the bar binds
# ... on the uncorrelated path: its only sum is the k-term mean, where the kernel's 8-way split has the smaller bound (k / 8 + 8 roundings
# against numpy's k), so the room is for another sample of the same roundings only
ROOM_UNCORR = 2.0
# smallest nugget of (1e-3, 1e-2, 1e-1) whose restatement leaves ROOM under the bar (asserted in tests/test_obs_space_reference.py)
GAUSS_NUGGET = {np.float64: 1e-3, np.float32: 1e-2}
GAUSS_NUGGETS = (1e-3, 1e-2, 1e-1)

# ---------------------------------------------------------------- shapes
P_SWEEP = [(7, P) for P in (1, 2, 31, 32, 33, 63, 64, 65, 96, 97)]
PANEL = [(7, 280), (7, 281), (40, 300), (3, 330)]       # rows below the first block: 256, 257, 309 (two workgroups), 302
K_SWEEP = [(k, P) for P in (33, 97) for k in (1, 2, 31, 32, 33, 80, 128)]
GAUSS_SHAPES = [(7, 33), (40, 300)]
CORR_CASES = [(fam, k, P) for fam in ("exp3", "scaled") for k, P in P_SWEEP + PANEL + K_SWEEP] + \
             [("gauss", k, P) for k, P in GAUSS_SHAPES]
UNCORR_K = (1, 2, 3, 5, 28, 30, 31, 32, 33, 63, 64, 65, 128)
UNCORR_P = (1, 31, 32, 33, 1000)
UNCORR_SPECIAL = [(1, 31), (3, 33), (30, 32), (40, 1000), (128, 33)]       # shapes of the large-mean and wide-variance cases
INFO_P = 97
INFO_J = (0, 31, 32, 33, 63, 96)
INFO_KINDS = ("negative", "nan", "zero")


# ---------------------------------------------------------------- inputs
def ensemble(k, P, shift=1.0):
    """hx (k, P), y (P,): the recipe of tests/test_gpu_interface.py"""
    rnd = np.random.RandomState(k * 1000 + P)
    return rnd.normal(size=(k, P)) + shift, rnd.normal(size=P) + shift


def covariance(family, P, nugget=None):
    """exp3: exp(-|i-j|/3) + 0.05 A A^T / P + 0.1 I, condition about 20 (the recipe of tests/test_gpu_interface.py).
    scaled: diag(s) exp3 diag(s) with s = 10**U(-2, 2), condition about 2e8; the Cholesky factor only scales with it.
    gauss: exp(-((i-j)/4)^2 / 2) + nugget I, condition 1e4 at nugget 1e-3.  Each seeded by P."""
    rnd = np.random.RandomState(P)
    x = np.arange(P, dtype=np.float64)
    if family == "gauss":
        return np.exp(-0.5 * ((x[:, None] - x[None, :]) / 4.0) ** 2) + nugget * np.eye(P)
    a = rnd.normal(size=(P, P))
    cov = np.exp(-np.abs(x[:, None] - x[None, :]) / 3.0) + 0.05 * (a @ a.T) / P + 0.1 * np.eye(P)
    if family == "scaled":
        s = 10.0 ** rnd.uniform(-2.0, 2.0, size=P)
        cov = cov * s[:, None] * s[None, :]
    elif family != "exp3":
        raise ValueError(family)
    return cov


def corr_inputs(family, k, P, dtype, nugget=None):
    """(hx, y, cov) of a correlated case, rounded to dtype"""
    if family == "gauss" and nugget is None:
        nugget = GAUSS_NUGGET[dtype]
    hx, y = ensemble(k, P)
    return hx.astype(dtype), y.astype(dtype), covariance(family, P, nugget).astype(dtype)


def uncorr_inputs(k, P, dtype, kind="plain"):
    """(hx, y, var) rounded to dtype.  plain: N(1, 1) values and var in U(0.2, 4); a mean of 3 as in tests/test_gpu_interface.py puts
    the float32 restatement at 1.1e-6 in its worst column of a thousand, which leaves no ROOM under 2e-6.  mean: an ensemble mean of 1e4 (float32) or
    1e8 (float64) under a spread of 1, what the split mean of the kernel is for.  range: var over 1e-12 .. 1e12."""
    rnd = np.random.RandomState(k * 1000 + P + 7)
    shift = 1.0
    if kind == "mean":
        shift = 1e4 if dtype == np.float32 else 1e8
    hx = rnd.normal(size=(k, P)) + shift
    y = rnd.normal(size=P) + shift
    var = 10.0 ** rnd.uniform(-12.0, 12.0, size=P) if kind == "range" else rnd.uniform(0.2, 4.0, size=P)
    return hx.astype(dtype), y.astype(dtype), var.astype(dtype)


def info_inputs(kind, j, dtype, P=INFO_P, k=5):
    """(hx, y, cov) whose leading minor of order j + 1 is the first that is not positive definite.
    negative / nan: exp3 with -1.0 / NaN at (j, j).  zero: R = L L^T for a banded integer L with a diagonal of ones and twos whose row j
    repeats row j - 1 (at j = 0: is zero), so rows and columns j - 1 and j of R are equal, every intermediate of any Cholesky sweep is a
    small integer, exact in float32 in any summation order, and pivot j is exactly 0.0."""
    hx, y = ensemble(k, P)
    if kind == "zero":
        rnd = np.random.RandomState(100 * P + j)
        L = np.diag(rnd.choice([1.0, 2.0], size=P))
        for b in (1, 2, 3):
            L += np.diag(rnd.randint(-1, 2, size=P - b).astype(np.float64), -b)
        L[j, :] = L[j - 1, :] if j > 0 else 0.0
        L[j, j] = 0.0
        cov = L @ L.T
        assert np.abs(cov).max() < 64 and (j == 0 or np.array_equal(cov[j], cov[j - 1]))
    else:
        cov = covariance("exp3", P)
        cov[j, j] = {"negative": -1.0, "nan": np.nan}[kind]
    return hx.astype(dtype), y.astype(dtype), cov.astype(dtype)


# ---------------------------------------------------------------- referee
def reference(hx, y, cov=None, var=None):
    """([Yb; d] (k + 1, P) in longdouble, info): Yb = (hx - mean) R^-1/2, d = (y - mean) R^-1/2 with R^-1/2 = L^-T (cov = L L^T, only
    its lower triangle is read) or 1 / sqrt(var).  info is the LAPACK-convention order of the first pivot that is not > 0 (NaN
    included), 0 if there is none; columns from that pivot on are then not finite."""
    if (cov is None) == (var is None):
        raise ValueError("give exactly one of cov and var")
    hx = np.asarray(hx).astype(LD)
    k, P = hx.shape
    mean = hx.sum(axis=0) / LD(k)
    V = np.concatenate([hx - mean, (np.asarray(y).astype(LD) - mean)[None]], axis=0)
    if var is not None:
        return V / np.sqrt(np.asarray(var).astype(LD)), 0
    M = np.concatenate([np.tril(np.asarray(cov).astype(LD)), V], axis=0)        # [R; V], (P + k + 1, P)
    info = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(P):
            # column j of L below and on the diagonal and column j of V L^-T: one step of forward substitution for every row
            col = M[j:, j] - M[j:, :j] @ M[j, :j]
            if not col[0] > 0 and info == 0:
                info = j + 1
            piv = np.sqrt(col[0])
            M[j, j] = piv
            M[j + 1:, j] = col[1:] / piv
    return M[P:], info


def restatement(hx, y, cov, dtype, var=None):
    """the same in dtype: numpy's mean, LAPACK's potrf and trtrs.  (k + 1, P) in dtype.  The factor comes from scipy.linalg.cholesky,
    which calls spotrf for float32; numpy.linalg.cholesky factors a float32 matrix in double and rounds the result (its factor equals
    the rounded float64 one to every digit), which is no float32 implementation and made this figure 100 times too small on gauss."""
    from scipy.linalg import cholesky, solve_triangular
    hx, y = np.asarray(hx, dtype=dtype), np.asarray(y, dtype=dtype)
    mean = hx.mean(axis=0, dtype=dtype)
    V = np.concatenate([hx - mean, (y - mean)[None]], axis=0)
    if var is not None:
        out = V * (dtype(1) / np.sqrt(np.asarray(var, dtype=dtype)))
    else:
        L = cholesky(np.asarray(cov, dtype=dtype), lower=True, check_finite=False)
        assert L.dtype == dtype
        out = solve_triangular(L, V.T, lower=True, check_finite=False).T
    assert out.dtype == dtype
    return out


def column_error(got, ref, floored=True, scale=None):
    """max over observation columns j of |got[:, j] - ref[:, j]| / max(|ref[:, j]|, rms_j |ref[:, j]|).  The floor keeps a column
    of [Yb; d] that is nearly zero (k = 3) from turning the figure into one about nothing.  ``scale`` (P,) multiplies the columns of
    both first: with variances over 24 decades the floor would otherwise hide every column but the largest."""
    ref = np.asarray(ref).astype(LD)
    got = np.asarray(got).astype(LD)
    if scale is not None:
        ref, got = ref * np.asarray(scale).astype(LD), got * np.asarray(scale).astype(LD)
    err = np.sqrt(((got - ref) ** 2).sum(axis=0))
    norm = np.sqrt((ref ** 2).sum(axis=0))
    if floored:
        norm = np.maximum(norm, np.sqrt((norm ** 2).mean()))
    return float((err / norm).max()) if err.size else 0.0


@functools.lru_cache(maxsize=None)
def corr_case(family, k, P, dtype, nugget=None):
    """(hx, y, cov, ref, restatement's error) of one correlated case; computed once, handed out read-only"""
    hx, y, cov = corr_inputs(family, k, P, dtype, nugget)
    ref, info = reference(hx, y, cov=cov)
    assert info == 0
    e = column_error(restatement(hx, y, cov, dtype), ref)
    for a in (hx, y, cov, ref):
        a.setflags(write=False)
    return hx, y, cov, ref, e


@functools.lru_cache(maxsize=None)
def uncorr_case(k, P, dtype, kind="plain"):
    hx, y, var = uncorr_inputs(k, P, dtype, kind)
    ref, _ = reference(hx, y, var=var)
    for a in (hx, y, var, ref):
        a.setflags(write=False)
    return hx, y, var, ref


def corr_tol(rest_err, dtype):
    return min(FACTOR * rest_err, BAR_CORR[dtype])


def mean_bound(hx, var, dtype):
    """(P,) bound on every entry of a column of [Yb; d] for a large mean: (k + 4) eps max_i |hx[i, j]| / sqrt(var[j]), the forward
    bound of a k-term mean, one subtraction and one product with the rounded 1 / sqrt(var)"""
    k = hx.shape[0]
    return (k + 4) * float(np.finfo(dtype).eps) * np.abs(hx.astype(np.float64)).max(axis=0) / np.sqrt(var.astype(np.float64))

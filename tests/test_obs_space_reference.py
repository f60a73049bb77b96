"""Pins tests/obs_space_cases.py on the CPU: the extended-precision referee of the observation-space preparation against the
reference project's own fixture and the float64 oracle, and the envelope of every case tests/test_gpu_obs_space.py runs, so that a
case drifting out of its tolerance fails here and not as a flake on the GPU.

Measured here (restatement = numpy's mean, LAPACK's potrf / trtrs through scipy in the working dtype, against the longdouble referee;
inputs rounded to the dtype first; the floored per-column metric of column_error, maximum over the shapes of OC.CORR_CASES; in
brackets the unfloored figure):

  family                 float64                float32
  exp3                   1.1e-15 (2.0e-14)      5.5e-7 (6.6e-6)
  scaled                 1.4e-15 (7.5e-14)      6.7e-7 (2.6e-5)
  gauss, nugget 1e-3     2.2e-13 (2.9e-13)      1.2e-4 (1.5e-4)
  gauss, nugget 1e-2     2.2e-14                1.2e-5 (1.4e-5)
  gauss, nugget 1e-1     2.4e-15                1.2e-6 (1.3e-6)

The smallest floored figure is 7.3e-17 / 2.4e-8 (P = 1).  The unfloored maxima come from k <= 3, where one column of [Yb; d] is
nearly zero.  Against the bars 1e-11 / 2e-4 every case leaves the ROOM = 4 asked for except gauss at nugget 1e-3 in float32 (condition
1e4 times 6e-8), so float32 runs gauss at nugget 1e-2.  numpy.linalg.cholesky is no float32 restatement: it factors in double and
rounds (2.4e-8 from the float64 factor, the rounding alone), and put 1.0e-6 where spotrf has 1.2e-4.
Uncorrelated restatement (its error is that of the k-term mean): at most 1.1e-15 / 6.0e-7 over the plain shapes and the ones with
variances over 24 decades, against the bars 1e-13 / 2e-6; the float32 figure is the worst column of a thousand at k = 63."""
import numpy as np
import pytest

import obs_space_cases as OC
from oracle import letkf_oracle as O

DTYPES = [np.float64, np.float32]


def test_reference_reproduces_the_reference_projects_fixture(golden):
    g = golden("g6_reference_fixture_letkf.npz")
    ti = int(g["time_index"])
    ref, info = OC.reference(g["state"][0, ti], g["obs"][ti], cov=g["cov"])
    assert info == 0 and ref.dtype == OC.LD
    k = g["yb"].shape[0]
    np.testing.assert_allclose(ref[:k].astype(np.float64), g["yb"], atol=1e-12, rtol=0)
    np.testing.assert_allclose(ref[k].astype(np.float64), np.ravel(g["d"]), atol=1e-12, rtol=0)


@pytest.mark.parametrize("k,P", [(10, 40), (7, 33), (40, 300)])
def test_reference_agrees_with_the_float64_oracle(k, P):
    hx, y, cov = OC.corr_inputs("exp3", k, P, np.float64)
    yb, d = O.obs_space_corr(hx, y, cov)
    assert OC.column_error(np.concatenate([yb, d[None]]), OC.reference(hx, y, cov=cov)[0]) < 1e-13
    hx, y, var = OC.uncorr_inputs(k, P, np.float64)
    yb, d = O.obs_space_uncorr(hx, y, var)
    assert OC.column_error(np.concatenate([yb, d[None]]), OC.reference(hx, y, var=var)[0]) < 1e-13


def test_reference_reads_the_lower_triangle_only():
    hx, y, cov = OC.corr_inputs("exp3", 7, 65, np.float64)
    upper = cov.copy()
    upper[np.triu_indices(65, 1)] = np.nan
    a, b = OC.reference(hx, y, cov=cov), OC.reference(hx, y, cov=upper)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 0


def test_the_case_list_is_the_one_the_kernels_need():
    shapes = {(k, P) for _, k, P in OC.CORR_CASES}
    below = lambda k, P: P + k + 1 - 32            # rows under the first block: chol_panel_kernel takes 256 per workgroup
    assert below(7, 280) == 256 and below(7, 281) == 257 and below(40, 300) > 256 and (330 - 32 + 31) // 32 == 10
    assert {P for k, P in shapes if k == 7} >= {1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 280, 281}
    for P in (33, 97):
        assert {k for k, q in shapes if q == P} >= {1, 2, 31, 32, 33, 80, 128}
    assert max(P for _, P in shapes) <= 330
    for fam in ("exp3", "scaled"):
        assert {(k, P) for f, k, P in OC.CORR_CASES if f == fam} == shapes
    assert {(k, P) for f, k, P in OC.CORR_CASES if f == "gauss"} == {(7, 33), (40, 300)}
    assert {(k + 1) % 4 for k in OC.UNCORR_K} == {0, 1, 2, 3} and {31, 32} <= set(OC.UNCORR_K)
    conds = {f: np.linalg.cond(OC.covariance(f, 97, 1e-3)) for f in ("exp3", "scaled", "gauss")}
    assert 5 < conds["exp3"] < 100 and 1e7 < conds["scaled"] < 1e10 and 3e3 < conds["gauss"] < 3e4


def test_the_float32_restatement_is_float32():
    """at condition 1e4 it is far from what a float64 sweep rounded at the end gives (numpy.linalg.cholesky on a float32 matrix
    is such a sweep: it factors in double)"""
    hx, y, cov = OC.corr_inputs("gauss", 7, 33, np.float32, 1e-3)
    ref = OC.reference(hx, y, cov=cov)[0]
    assert OC.column_error(OC.restatement(hx, y, cov, np.float32), ref) > 30 * OC.column_error(
        OC.restatement(hx, y, cov, np.float64).astype(np.float32), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_correlated_case_lies_inside_its_envelope(dtype):
    """the restatement leaves ROOM under the project's bar and is itself a figure of a few roundings, not zero: FACTOR times it is
    then a tolerance a blocked sweep of the same precision meets and a wrong column does not"""
    eps = float(np.finfo(dtype).eps)
    worst = {}
    for fam, k, P in OC.CORR_CASES:
        hx, y, cov, ref, e = OC.corr_case(fam, k, P, dtype)
        assert ref.shape == (k + 1, P) and np.isfinite(ref.astype(np.float64)).all()
        assert OC.ROOM * e <= OC.BAR_CORR[dtype], (fam, k, P, e)
        assert e >= eps / 8, (fam, k, P, e)
        assert OC.corr_tol(e, dtype) == min(32 * e, OC.BAR_CORR[dtype]) < 1e-2
        worst[fam] = max(worst.get(fam, 0.0), e)
    print({f: "%.2e" % v for f, v in worst.items()})
    # ... and the tolerance still has teeth: one column of the referee's result replaced by its neighbour is far outside
    hx, y, cov, ref, e = OC.corr_case("exp3", 7, 65, dtype)
    wrong = ref.copy()
    wrong[:, 40] = ref[:, 41]
    assert OC.column_error(wrong, ref) > 0.1 > 1e3 * OC.corr_tol(e, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_gauss_nugget_is_the_smallest_inside_the_envelope(dtype):
    ok = []
    for nugget in OC.GAUSS_NUGGETS:
        errs = [OC.corr_case("gauss", k, P, dtype, nugget)[4] for k, P in OC.GAUSS_SHAPES]
        ok.append(all(OC.ROOM * e <= OC.BAR_CORR[dtype] for e in errs))
    assert OC.GAUSS_NUGGET[dtype] == OC.GAUSS_NUGGETS[ok.index(True)]


@pytest.mark.parametrize("kind", OC.INFO_KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_info_case_fails_at_its_order(kind, dtype):
    for j in OC.INFO_J:
        hx, y, cov = OC.info_inputs(kind, j, dtype)
        assert cov.shape == (OC.INFO_P, OC.INFO_P) and cov.dtype == dtype
        ref, info = OC.reference(hx, y, cov=cov)
        assert info == j + 1, (kind, j, info)
        assert np.isfinite(ref[:, :j].astype(np.float64)).all() and not np.isfinite(ref[:, j].astype(np.float64)).any()
        if kind == "zero":
            assert np.array_equal(cov, np.round(cov)) and np.array_equal(cov.astype(np.float32), cov)
            if j > 0:          # every leading minor before it is positive definite; LAPACK meets a pivot of exactly zero there
                assert np.linalg.eigvalsh(cov[:j, :j].astype(np.float64)).min() > 0
                with pytest.raises(np.linalg.LinAlgError):
                    np.linalg.cholesky(cov[:j + 1, :j + 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_uncorrelated_cases_lie_inside_their_envelope(dtype):
    worst = 0.0
    for k in OC.UNCORR_K:
        for P in OC.UNCORR_P:
            hx, y, var, ref = OC.uncorr_case(k, P, dtype)
            e = OC.column_error(OC.restatement(hx, y, None, dtype, var=var), ref)
            assert OC.ROOM_UNCORR * e <= OC.BAR_UNCORR[dtype], (k, P, e)
            worst = max(worst, e)
    for k, P in OC.UNCORR_SPECIAL:
        hx, y, var, ref = OC.uncorr_case(k, P, dtype, "range")
        assert var.max() / var.min() > 1e18
        e = OC.column_error(OC.restatement(hx, y, None, dtype, var=var), ref, scale=np.sqrt(var.astype(OC.LD)))
        assert OC.ROOM_UNCORR * e <= OC.BAR_UNCORR[dtype], (k, P, e)
        worst = max(worst, e)
    print("%.2e" % worst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_restatement_meets_the_large_mean_bound(dtype):
    """(k + 4) eps max|hx| / sqrt(var) is a forward bound, so a plain implementation in the dtype has to meet it entry by entry"""
    for k, P in OC.UNCORR_SPECIAL:
        hx, y, var, ref = OC.uncorr_case(k, P, dtype, "mean")
        assert np.abs(hx).min() > (5e3 if dtype == np.float32 else 5e7) and np.ptp(hx, axis=0).max() < 12
        got = OC.restatement(hx, y, None, dtype, var=var)
        err = np.abs(got.astype(OC.LD) - ref).astype(np.float64)
        assert (err <= OC.mean_bound(hx, var, dtype)).all(), (k, P, (err / OC.mean_bound(hx, var, dtype)).max())
        # the bound is no licence: it is far below the spread the values carry
        assert OC.mean_bound(hx, var, dtype).max() < (0.5 if dtype == np.float32 else 1e-5)

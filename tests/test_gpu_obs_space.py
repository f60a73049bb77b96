"""The observation-space preparation (csrc/obs_space.hip) at its block edges, against the extended-precision referee of
tests/obs_space_cases.py: the blocked Cholesky over [R; V] where a block is full, ragged or a single column, where the panel kernel
needs a second workgroup, where update tiles straddle the last row of R; the order in info; leading dimensions and optional outputs of
the C entries; the record padding of the uncorrelated kernel at every (k + 1) mod 4; get_obs_space_variables over four subsets.

Tolerance of the correlated path: the per-column metric of OC.column_error within 32 times the error of the LAPACK restatement in the
same dtype (computed on the host from the referee, tests/test_obs_space_reference.py pins its envelope) and within 1e-11 / 2e-4.
Measured on an MI355X, worst ratio of the device's error to the restatement's over the shapes of OC.CORR_CASES (device error there):
  exp3    float64 2.6 at (k, P) = (7, 65), 1.4e-15      float32 4.0 at (2, 33), 1.1e-6
  scaled  float64 4.8 at (1, 33), 1.4e-15               float32 3.6 at (7, 31), 1.3e-6
  gauss   float64 3.0 at (7, 33), 5.8e-13 (nugget 1e-3) float32 1.8 at (7, 33), 1.7e-5 (nugget 1e-2)
At nugget 1e-3 the float32 sweep is at 1.8e-4 and 2.5e-4, beside 1.2e-4 for LAPACK's spotrf: condition 1e4 leaves float32 no room
under 2e-4, which is what the envelope test on the CPU says before any GPU is asked.  Uncorrelated path: at most 4.7e-16 / 2.7e-7
on the plain shapes; the large-mean cases use at most 0.13 of their forward bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import obs_space_cases as OC

pytestmark = pytest.mark.gpu

NP = {torch.float64: np.float64, torch.float32: np.float32}
DTYPES = [torch.float64, torch.float32]
NAN = float("nan")


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine("cuda:0")


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda:0")


def stacked(yb, d):
    return np.concatenate([yb.cpu().numpy(), d.cpu().numpy()[None]], axis=0)


def check_records(eng, yb, d, rec, dtype):
    """rec is pack_obs(yb, d) bit for bit: row j holds column j of Yb, then d[j], then zeros up to kp.  The layout is asserted
    directly as well, which is all there is at k = 1: mia_letkf_pack_obs_* takes two members or more (MIA_ERR_SIZE below)."""
    k, P = yb.shape
    kp = (k + 1 + 3) // 4 * 4
    assert rec.shape == (P, kp) and rec.dtype == dtype
    if k >= 2:
        assert torch.equal(rec, eng.pack_obs(yb, d, dtype))
    assert torch.equal(rec[:, :k], yb.t()) and torch.equal(rec[:, k], d)
    assert torch.equal(rec[:, k + 1:], torch.zeros((P, kp - k - 1), dtype=dtype, device=rec.device))


# ---------------------------------------------------------------- correlated R
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("fam,k,P", OC.CORR_CASES)
def test_correlated_vs_extended_precision(eng, dtype, fam, k, P):
    hx, y, cov, ref, e_rest = OC.corr_case(fam, k, P, NP[dtype])
    yb, d, rec = eng.obs_space(dev(hx), dev(y), cov=dev(cov), dtype=dtype, want_rec=True)
    assert yb.dtype == dtype and yb.shape == (k, P) and d.shape == (P,)
    err = OC.column_error(stacked(yb, d), ref)
    print("corr %s %s k=%d P=%d err %.3e restatement %.3e ratio %.2f" % (fam, NP[dtype].__name__, k, P, err, e_rest, err / e_rest))
    assert err <= OC.corr_tol(e_rest, NP[dtype])
    check_records(eng, yb, d, rec, dtype)
    # the strict upper triangle of cov is never read
    upper = cov.copy()
    upper[np.triu_indices(P, 1)] = np.nan
    yb2, d2, rec2 = eng.obs_space(dev(hx), dev(y), cov=dev(upper), dtype=dtype, want_rec=True)
    assert torch.equal(yb2, yb) and torch.equal(d2, d) and torch.equal(rec2, rec)


def raw_call(eng, path, dtype, hx, ldh, y, r, k, P, Yb, ldy, d, rec, info=None):
    """the C entry itself on the null stream (torch's default): tensors or None, views allowed; returns the code after a sync"""
    sfx, elem = ("f32", 4) if dtype == torch.float32 else ("f64", 8)
    ptr = lambda t: None if t is None else t.data_ptr()
    if path == "uncorr":
        rc = getattr(eng.lib, "mia_obs_space_uncorr_" + sfx)(ptr(hx), ldh, ptr(y), ptr(r), k, P, ptr(Yb), ldy, ptr(d), ptr(rec), None)
    else:
        n = C.c_size_t(0)
        assert eng.lib.mia_obs_space_corr_workspace_bytes(k, P, elem, C.byref(n)) == 0
        ws = torch.empty(n.value, dtype=torch.uint8, device="cuda:0")
        rc = getattr(eng.lib, "mia_obs_space_corr_" + sfx)(ptr(hx), ldh, ptr(y), ptr(r), k, P, ptr(Yb), ldy, ptr(d), ptr(rec),
                                                           ptr(info), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", OC.INFO_KINDS)
def test_info_carries_the_order_of_the_first_bad_pivot(eng, dtype, kind):
    """in the first block, at its end, first and second of the next block, at a later block's end, in the ragged last block; through
    the engine's message and through info of the C entry; a clean call on the same engine (same workspace) is untouched by it"""
    P = OC.INFO_P
    chx, cy, ccov, ref, e_rest = OC.corr_case("exp3", 5, P, NP[dtype])
    clean = eng.obs_space(dev(chx), dev(cy), cov=dev(ccov), dtype=dtype, want_rec=True)
    assert OC.column_error(stacked(clean[0], clean[1]), ref) <= OC.corr_tol(e_rest, NP[dtype])
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
    for j in OC.INFO_J:
        hx, y, cov = OC.info_inputs(kind, j, NP[dtype])
        k = hx.shape[0]
        with pytest.raises(ValueError, match=r"leading minor of order %d\)" % (j + 1)):
            eng.obs_space(dev(hx), dev(y), cov=dev(cov), dtype=dtype)
        yb, d = torch.empty((k, P), dtype=dtype, device="cuda:0"), torch.empty(P, dtype=dtype, device="cuda:0")
        assert raw_call(eng, "corr", dtype, dev(hx), P, dev(y), dev(cov), k, P, yb, P, d, None, info) == 0
        assert int(info.item()) == j + 1, (kind, j)
        # columns ahead of the bad pivot never see it: they are those of the clean matrix, which differs at (j, j) only
        if kind != "zero":
            assert torch.equal(yb[:, :j], clean[0][:, :j]) and torch.equal(d[:j], clean[1][:j])
        again = eng.obs_space(dev(chx), dev(cy), cov=dev(ccov), dtype=dtype, want_rec=True)
        assert all(torch.equal(a, b) for a, b in zip(again, clean)), (kind, j)
    # ... and info is cleared by a clean call, not left as it was handed in
    assert int(info.item()) == OC.INFO_J[-1] + 1
    yb, d = torch.empty((5, P), dtype=dtype, device="cuda:0"), torch.empty(P, dtype=dtype, device="cuda:0")
    assert raw_call(eng, "corr", dtype, dev(chx), P, dev(cy), dev(ccov), 5, P, yb, P, d, None, info) == 0
    assert int(info.item()) == 0 and torch.equal(yb, clean[0]) and torch.equal(d, clean[1])


# ---------------------------------------------------------------- the C entries: leading dimensions, optional outputs
def path_inputs(path, k, P, dtype):
    if path == "corr":
        hx, y, r = OC.corr_case("exp3", k, P, NP[dtype])[:3]
    else:
        hx, y, r = OC.uncorr_case(k, P, NP[dtype])[:3]
    return dev(hx), dev(y), dev(r)


def contiguous_call(eng, path, dtype, hx, y, r):
    k, P = hx.shape
    kp = (k + 1 + 3) // 4 * 4
    yb = torch.full((k, P), NAN, dtype=dtype, device="cuda:0")
    d = torch.full((P,), NAN, dtype=dtype, device="cuda:0")
    rec = torch.full((P, kp), NAN, dtype=dtype, device="cuda:0")
    assert raw_call(eng, path, dtype, hx, P, y, r, k, P, yb, P, d, rec) == 0
    assert not torch.isnan(yb).any() and not torch.isnan(d).any() and not torch.isnan(rec).any()
    return yb, d, rec


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("path,k,P", [("corr", 7, 65), ("corr", 33, 33), ("uncorr", 7, 65), ("uncorr", 33, 33)])
def test_leading_dimensions(eng, path, k, P, dtype):
    """hx a column slice of a wider array (ldh = P + 5), Yb a column slice of a wider one (ldy = P + 9, and one spare row behind):
    the same bits as the contiguous call and every sentinel outside the slice intact"""
    hx, y, r = path_inputs(path, k, P, dtype)
    yb, d, rec = contiguous_call(eng, path, dtype, hx, y, r)
    hx_wide = torch.full((k, P + 5), NAN, dtype=dtype, device="cuda:0")
    hx_wide[:, 2:2 + P] = hx
    yb_wide = torch.full((k + 1, P + 9), NAN, dtype=dtype, device="cuda:0")
    d2, rec2 = torch.full_like(d, NAN), torch.full_like(rec, NAN)
    assert raw_call(eng, path, dtype, hx_wide[:, 2:], P + 5, y, r, k, P, yb_wide[:, 4:], P + 9, d2, rec2) == 0
    assert torch.equal(yb_wide[:k, 4:4 + P], yb) and torch.equal(d2, d) and torch.equal(rec2, rec)
    assert torch.isnan(yb_wide[:, :4]).all() and torch.isnan(yb_wide[:, 4 + P:]).all() and torch.isnan(yb_wide[k]).all()
    assert torch.equal(hx_wide[:, 2:2 + P], hx) and torch.isnan(hx_wide[:, :2]).all() and torch.isnan(hx_wide[:, 2 + P:]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("path", ["corr", "uncorr"])
def test_every_combination_of_optional_outputs(eng, path, dtype):
    k, P = 6, 70
    hx, y, r = path_inputs(path, k, P, dtype)
    full = contiguous_call(eng, path, dtype, hx, y, r)
    for mask in range(7):
        outs = [torch.full_like(t, NAN) if mask >> i & 1 else None for i, t in enumerate(full)]
        assert raw_call(eng, path, dtype, hx, P, y, r, k, P, outs[0], P, outs[1], outs[2]) == 0, mask
        for got, want in zip(outs, full):
            assert got is None or torch.equal(got, want), mask
    # without Yb its leading dimension is not looked at
    d = torch.full_like(full[1], NAN)
    assert raw_call(eng, path, dtype, hx, P, y, r, k, P, None, 0, d, None) == 0 and torch.equal(d, full[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("path", ["corr", "uncorr"])
def test_records_at_an_offset_of_the_stacked_arrays(eng, path, dtype):
    k, P, off = 9, 45, 5
    kp = (k + 1 + 3) // 4 * 4
    hx, y, r = path_inputs(path, k, P, dtype)
    kw = dict(cov=r) if path == "corr" else dict(var=r)
    yb, d, rec = eng.obs_space(hx, y, dtype=dtype, want_rec=True, **kw)
    total = off + P + 3
    yb_all = torch.full((k, total), NAN, dtype=dtype, device="cuda:0")
    d_all = torch.full((total,), NAN, dtype=dtype, device="cuda:0")
    rec_all = torch.full((total, kp), NAN, dtype=dtype, device="cuda:0")
    assert eng.obs_space(hx, y, dtype=dtype, out=(yb_all, d_all, rec_all), offset=off, **kw) is None
    sl = slice(off, off + P)
    assert torch.equal(yb_all[:, sl], yb) and torch.equal(d_all[sl], d) and torch.equal(rec_all[sl], rec)
    for a in (yb_all.t(), d_all, rec_all):
        assert torch.isnan(a[:off]).all() and torch.isnan(a[off + P:]).all()


# ---------------------------------------------------------------- uncorrelated R
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("k", OC.UNCORR_K)
def test_uncorrelated_vs_extended_precision(eng, dtype, k):
    """every (k + 1) mod 4, the innovation row as the last row of a pass of 32 (k = 31, 63), alone in the next (k = 32, 64), one
    member; one observation, a ragged and a full workgroup, many"""
    for P in OC.UNCORR_P:
        hx, y, var, ref = OC.uncorr_case(k, P, NP[dtype])
        yb, d, rec = eng.obs_space(dev(hx), dev(y), var=dev(var), dtype=dtype, want_rec=True)
        err = OC.column_error(stacked(yb, d), ref)
        print("uncorr %s k=%d P=%d err %.3e" % (NP[dtype].__name__, k, P, err))
        assert err <= OC.BAR_UNCORR[NP[dtype]], (k, P)
        check_records(eng, yb, d, rec, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_uncorrelated_large_mean(eng, dtype):
    """a mean of 1e4 (float32) / 1e8 (float64) under a spread of 1: every entry within the forward bound OC.mean_bound of a k-term
    mean, one subtraction and one product.  Derived, not measured."""
    for k, P in OC.UNCORR_SPECIAL:
        hx, y, var, ref = OC.uncorr_case(k, P, NP[dtype], "mean")
        yb, d, rec = eng.obs_space(dev(hx), dev(y), var=dev(var), dtype=dtype, want_rec=True)
        err = np.abs(stacked(yb, d).astype(OC.LD) - ref).astype(np.float64)
        bound = OC.mean_bound(hx, var, NP[dtype])
        print("mean %s k=%d P=%d worst err / bound %.3f" % (NP[dtype].__name__, k, P, (err / bound).max()))
        assert (err <= bound).all(), (k, P)
        check_records(eng, yb, d, rec, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_uncorrelated_variances_over_24_decades(eng, dtype):
    for k, P in OC.UNCORR_SPECIAL:
        hx, y, var, ref = OC.uncorr_case(k, P, NP[dtype], "range")
        yb, d, rec = eng.obs_space(dev(hx), dev(y), var=dev(var), dtype=dtype, want_rec=True)
        err = OC.column_error(stacked(yb, d), ref, scale=np.sqrt(var.astype(OC.LD)))
        print("range %s k=%d P=%d err %.3e" % (NP[dtype].__name__, k, P, err))
        assert err <= OC.BAR_UNCORR[NP[dtype]], (k, P)
        check_records(eng, yb, d, rec, dtype)


# ---------------------------------------------------------------- class level
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_get_obs_space_variables_over_four_subsets(mia, eng, dtype):
    """correlated P = 33, uncorrelated P = 17, empty, correlated P = 64: each slice against the referee of its own subset, and slice
    boundaries exact -- another subset's inputs change no bit of a slice"""
    npd, k = NP[dtype], 7
    hx1, y1, cov1, ref1, e1 = OC.corr_case("exp3", k, 33, npd)
    hx2, y2, var2, ref2 = OC.uncorr_case(k, 17, npd)
    hx4, y4, cov4, ref4, e4 = OC.corr_case("exp3", k, 64, npd)
    empty = np.empty((k, 0), dtype=npd), np.empty(0, dtype=npd), np.empty(0, dtype=npd)
    f = mia.ETKF(inf_factor=1.1, dtype=dtype, engine=eng)

    def run(hx2=hx2, y2=y2, var2=var2, cov1=cov1, hx4=hx4):
        d, yb = f.get_obs_space_variables([dev(hx1), dev(hx2), dev(empty[0]), dev(hx4)], [dev(y1), dev(y2), dev(empty[1]), dev(y4)],
                                          variances=[None, dev(var2), dev(empty[2]), None],
                                          covariances=[dev(cov1), None, None, dev(cov4)])
        assert yb.shape == (k, 114) and d.shape == (114,) and yb.dtype == d.dtype == dtype
        return stacked(yb, d)
    got = run()
    assert OC.column_error(got[:, :33], ref1) <= OC.corr_tol(e1, npd)
    assert OC.column_error(got[:, 33:50], ref2) <= OC.BAR_UNCORR[npd]
    assert OC.column_error(got[:, 50:], ref4) <= OC.corr_tol(e4, npd)
    other = run(hx2=hx2 + npd(1), y2=y2 * npd(2), var2=var2 * npd(3))
    assert np.array_equal(other[:, :33], got[:, :33]) and np.array_equal(other[:, 50:], got[:, 50:])
    assert not np.array_equal(other[:, 33:50], got[:, 33:50])
    other = run(cov1=cov1 * npd(4), hx4=hx4 * npd(2))
    assert np.array_equal(other[:, 33:50], got[:, 33:50])
    assert not np.array_equal(other[:, :33], got[:, :33]) and not np.array_equal(other[:, 50:], got[:, 50:])

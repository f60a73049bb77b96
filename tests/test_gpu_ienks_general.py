"""The general IEnKS update kernel, ienks_update_kernel<T, 256> (csrc/ienks.hip, LetkfEngine.ienks_update(method="eig")), on incoming
weights whose in-place Gauss-Jordan inverse HAS to pivot, point by point against the CPU oracle.

Why: every other IEnKS test feeds the kernel weights (the identity, I + 0.1 N, SPD iterates) on which its partial pivoting never
swaps a row, so the row swap, the reverse column unswap (piv[]), the tie-break across lanes and the cross-wave reduction (red[])
have never changed a result; and they compare ONE relative Frobenius norm over all grid points, in which one wrong point of 64
disappears.  Here

  * the incoming weights of every point are W = (I + 0.5 / sqrt(k) N)[perm, :] + 0.3 c 1^T with a fresh permutation per point
    (general_weights); a CPU emulation of the kernel's pivoting (pivot_swaps) ASSERTS for every batch that some point swaps at
    column 0, some point at the last possible column k - 2, every point at least k / 3 times (k >= 7), and cond(Wp) <= 10
    (assert_pivoting) -- conditions on the input, so the tests cannot quietly stop exercising the path; random weights never
    tie, so one more input (tied_weights) meets the same magnitude in two rows at every even column;
  * the neighbour lists are built by hand (hand_lists: distinct random indices, rho uniform in (1e-5, 1], any chosen length per
    point), the reference is O.ienks_update per point on the gathered, sqrt(rho)-scaled block (what O.lienks_weights runs inside
    its loop);
  * every comparison is max over grid points of ||W_g - ref_g||_F / ||ref_g||_F (worst_point), never one norm over the batch;
  * method="eig" pins the kernel under test whatever "auto" would choose.

Tolerances: the project's bars for this kernel (tests/test_gpu_ienks.py), applied per point: float64 1e-9, float32 1e-4 on raw
weights.  With cond(Wp) <= 10 the float64 oracle is good to ~1e-13.  Measured worst single points are in DESIGN.md section 9.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import letkf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float64: 1e-9, torch.float32: 1e-4}
EPS = 1e-3                                      # bundle variant: Yb scaled by eps, as in tests/test_gpu_ienks.py
NONFINITE, RETRY = 4, 8                        # MIA_FLAG_* (include/mia_letkf.h)
LDS_CAP = 160 * 1024 - 1024                     # kMaxDynamicLds (csrc/mia_common.h)
G = 32                                          # grid points per batch: the kernel is one workgroup per point
VARIANTS = (("transform", None), ("bundle", EPS))


@pytest.fixture(scope="module")
def mia():
    import torch_assimilate_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def eng(mia):
    return mia.LetkfEngine(DEV)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def perts_of(W):
    """Wp of _split_weights (core/ienks.py:46-54): W - mean_j(W - I) 1^T"""
    k = W.shape[-1]
    return W - (W - np.eye(k)).mean(axis=-1, keepdims=True)


def pivot_trace(a):
    """(columns at which the kernel's Gauss-Jordan elimination swaps rows, columns whose largest magnitude is met by more than one
    row): pivot of column c = the largest |a[r][c]| over r >= c, the lowest such row on a tie.  (The kernel inverts in place; its
    columns >= c of rows >= c, which alone decide the pivots, are those of this plain elimination.)"""
    a = np.array(a, dtype=np.float64)
    k, swaps, ties = a.shape[0], [], []
    for c in range(k):
        mag = np.abs(a[c:, c])
        pr = c + int(np.argmax(mag))
        if int((mag == mag.max()).sum()) > 1:
            ties.append(c)
        if pr != c:
            a[[c, pr]] = a[[pr, c]]
            swaps.append(c)
        a[c] /= a[c, c]
        f = a[:, c].copy()
        f[c] = 0.0
        a -= f[:, None] * a[c][None, :]
    return swaps, ties


def pivot_swaps(a):
    return pivot_trace(a)[0]


def general_weights(n, k, seed):
    """(n, k, k): W_g = (I + 0.5 / sqrt(k) N(0,1)^{k x k})[perm_g, :] + 0.3 N(0,1)^{k x 1} (broadcast over columns: a non-zero
    w_mean).  A draw is repeated while it misses a per-point input condition of assert_pivoting (k = 7: one permutation in 25
    needs fewer than three swaps)."""
    rs = np.random.RandomState(seed)
    out = np.empty((n, k, k))
    for g in range(n):
        while True:
            W = (np.eye(k) + 0.5 / np.sqrt(k) * rs.normal(size=(k, k)))[rs.permutation(k)] + 0.3 * rs.normal(size=(k, 1))
            Wp = perts_of(W)
            if np.linalg.cond(Wp) <= 10.0 and (k < 7 or 3 * len(pivot_swaps(Wp)) >= k):
                break
        out[g] = W
    return out


def assert_pivoting(W, where=None):
    """The input conditions of a batch (W (n, k, k), ``where``: the points that are updated at all)."""
    n, k = W.shape[0], W.shape[-1]
    pts = [g for g in range(n) if where is None or where[g]]
    swaps = [pivot_swaps(perts_of(W[g])) for g in pts]
    assert any(0 in s for s in swaps), "no point swaps at column 0"
    assert any(k - 2 in s for s in swaps), "no point swaps at the last possible column"
    if k >= 7:
        assert all(3 * len(s) >= k for s in swaps), "a point with fewer than k / 3 swaps"
    assert all(np.linalg.cond(perts_of(W[g])) <= 10.0 for g in pts)
    return swaps


def observations(k, P, seed):
    rs = np.random.RandomState(seed)
    hx = rs.normal(size=(k, P)) * 0.5
    return hx - hx.mean(axis=0), rs.normal(size=P) * 0.5


def hand_lists(cnts, P, p_cap, seed):
    """per-point lists of the given lengths: distinct random observation indices (-1 padded), rho uniform in (1e-5, 1]"""
    rs = np.random.RandomState(seed)
    n = len(cnts)
    idx = np.full((n, p_cap), -1, dtype=np.int32)
    rho = np.zeros((n, p_cap))
    for g, c in enumerate(cnts):
        assert 0 <= c <= min(P, p_cap)
        idx[g, :c] = rs.choice(P, size=c, replace=False)
        rho[g, :c] = 1.0 - rs.uniform(0.0, 1.0 - 1e-5, size=c)
    return np.asarray(cnts, dtype=np.int32), idx, rho


def neighbour_lists(mia, cnt, idx, rho, p_max, g0=0, g1=None):
    """NeighbourLists of the shard [g0, g1) of hand_lists' arrays (w = sqrt(rho))"""
    g1 = len(cnt) if g1 is None else g1
    return mia.NeighbourLists(torch.as_tensor(np.ascontiguousarray(cnt[g0:g1]), device=DEV),
                              torch.as_tensor(np.ascontiguousarray(idx[g0:g1]), device=DEV),
                              torch.as_tensor(np.ascontiguousarray(np.sqrt(rho[g0:g1])), device=DEV),
                              idx.shape[1], p_max, g0, g1)


def oracle(W, yb, d, cnt, idx, rho, tau, eps):
    """O.ienks_update per point on the gathered, sqrt(rho)-scaled block (O.lienks_weights' loop body)"""
    out = np.empty((len(cnt),) + W.shape[-2:])
    for g, c in enumerate(cnt):
        use, sw = idx[g, :c], np.sqrt(rho[g, :c])
        out[g] = O.ienks_update(W[g] if W.ndim == 3 else W, yb[:, use] * sw, d[use] * sw, tau, eps).numpy()
    return out


def worst_point(got, ref, sel=None):
    """max_g ||W_g - ref_g||_F / ||ref_g||_F and its point (a non-finite point counts as infinitely wrong)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    pp = np.sqrt(((got - ref) ** 2).sum(axis=(1, 2))) / np.sqrt((ref ** 2).sum(axis=(1, 2)))
    pp = np.where(np.isfinite(pp), pp, np.inf)
    if sel is not None:
        pp = np.where(sel, pp, 0.0)
    return float(pp.max()), int(pp.argmax())


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def update(eng, W, yb, d, nb, tau, eps, dtype, method="eig"):
    """(W' on the device, flags as numpy)"""
    res = eng.ienks_update(dev(W, dtype), dev(yb, dtype), dev(d, dtype), nb, tau, eps, return_flags=True, method=method)
    torch.cuda.synchronize()
    return res[0], res[1].cpu().numpy()


def general_lds_bytes(k, p_max, tau, bundle, eb):
    """the dynamic LDS of ienks_update_kernel as ienks_update_impl sizes it (csrc/ienks.hip)"""
    n, kp = (k + 1) & ~1, (k + 1 + 3) & ~3
    lda = n + 1
    nd = ((max(p_max, 1) + 1) & ~1) if (tau == 1.0 and p_max <= k) else 0
    rows = nd if nd > 0 else max(p_max, 1)
    e = 2 * n * lda + (1 if bundle else 2) * rows * kp + 5 * n + ((p_max + 3) & ~1)
    nbk = n // 2
    lds = (e * eb + ((p_max + 3) & ~1) * 4 + 4 * 4 + ((nbk * (nbk - 1) // 2 + 7) & ~7) * 2 + ((n + 1) & ~1) * 4 +
           (256 // 64 * 2) * eb)
    return (lds + 15) & ~15


def tag(dtype):
    return "f64" if dtype == torch.float64 else "f32"


# ---- 1. sweep ------------------------------------------------------------------------------------------------------------------
# p_max <= k / 2, odd for five of the nine sizes; k = 80 stops at 20: two (rows x kp) blocks of float64 beside the two
# (n x lda) matrices reach 131 KB of the 159 KB there (161 KB at p_max = 40)
SWEEP_PMAX = {2: 1, 3: 1, 7: 3, 20: 10, 33: 16, 40: 19, 65: 32, 80: 20, 96: 47}
SWEEP_TAU = (0.0, 0.6, 1.0)


@functools.lru_cache(maxsize=None)
def sweep_case(k):
    """inputs and the oracle's answers of one ensemble size, shared by both dtypes"""
    p_max = SWEEP_PMAX[k]
    P = 3 * k + 8
    W = general_weights(G, k, 100 + k)
    assert_pivoting(W)
    yb, d = observations(k, P, 200 + k)
    rs = np.random.RandomState(300 + k)
    cnts = rs.randint(1, p_max + 1, size=G)
    cnts[:2] = p_max
    cnt, idx, rho = hand_lists(cnts, P, p_max + 3, 400 + k)
    ref = {(tau, vname): oracle(W, yb * (eps or 1.0), d, cnt, idx, rho, tau, eps) for tau in SWEEP_TAU for vname, eps in VARIANTS}
    assert all(np.isfinite(r).all() for r in ref.values())
    return dict(W=W, yb=yb, d=d, cnt=cnt, idx=idx, rho=rho, p_max=p_max, ref=ref)


@pytest.mark.parametrize("dtype,k", [(torch.float64, k) for k in (2, 3, 7, 20, 33, 40, 65, 80)] +
                         [(torch.float32, k) for k in (2, 3, 7, 20, 33, 40, 65, 80, 96)])
def test_sweep_every_point_vs_oracle(mia, eng, dtype, k):
    """tau 0 (Pn = w_prec alone, W' the polar factor of Wp), 0.6 and 1 (dual route: p_max <= k), both variants; above 64 members
    waves 1 to 3 take part in the pivot search."""
    case = sweep_case(k)
    nb = neighbour_lists(mia, case["cnt"], case["idx"], case["rho"], case["p_max"])
    eb = 8 if dtype == torch.float64 else 4
    for tau in SWEEP_TAU:
        for vname, eps in VARIANTS:
            assert general_lds_bytes(k, case["p_max"], tau, eps is not None, eb) <= LDS_CAP
            W, fl = update(eng, case["W"], case["yb"] * (eps or 1.0), case["d"], nb, tau, eps, dtype)
            err, at = worst_point(W.cpu().numpy(), case["ref"][(tau, vname)])
            print("\n[ienks general] sweep %s k %d p_max %d tau %.1f %s: worst point %.3e (point %d)"
                  % (tag(dtype), k, case["p_max"], tau, vname, err, at))
            assert int((fl & 0xff).max()) == 0, (tau, vname)
            assert err <= TOL[dtype], (tau, vname, at, err)


# ---- 2. list-length edges -------------------------------------------------------------------------------------------------------
def edge_counts(k, p_max):
    """dual-route batch (p_max <= k): no observation, 1, 2, an odd count (= p_max where p_max is odd: no padded row of D^T left
    over / one padded row for every shorter odd count), p_max (= k in the p_max = k batch), and whatever lies between"""
    odd = p_max if p_max & 1 else p_max - 1
    base = [0, 1, 2, odd, p_max, 0, 1, p_max, odd, 2]
    rs = np.random.RandomState(k + p_max)
    return base + list(rs.randint(1, p_max + 1, size=6))


@functools.lru_cache(maxsize=None)
def edge_case(k, p_max, primal):
    if primal:       # p_max > k: short and full lists mixed
        cnts = [0, 1, 2, k - 1, k, k + 1, p_max, p_max, 1, p_max - 1, 0, k]
        cnts += list(np.random.RandomState(k).randint(1, p_max + 1, size=4))
    else:
        cnts = edge_counts(k, p_max)
    n, P = len(cnts), 3 * k + 8
    W = general_weights(n, k, 500 + 7 * k + p_max)
    assert_pivoting(W, where=np.asarray(cnts) > 0)
    yb, d = observations(k, P, 600 + k)
    cnt, idx, rho = hand_lists(cnts, P, p_max + 2, 700 + k + p_max)
    ref = {(tau, vname): oracle(W, yb * (eps or 1.0), d, cnt, idx, rho, tau, eps) for tau in (1.0, 0.6) for vname, eps in VARIANTS}
    return dict(W=W, yb=yb, d=d, cnt=cnt, idx=idx, rho=rho, p_max=p_max, ref=ref)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("k,p_max,primal", [(20, 20, False), (20, 19, False), (7, 7, False), (7, 5, False),
                                            (20, 21, True), (20, 60, True), (7, 8, True), (7, 21, True)])
def test_list_length_edges(mia, eng, dtype, k, p_max, primal):
    """cnt = 0, 1, 2, an odd cnt equal to an odd p_max, cnt = p_max = k (the dual route's last order); p_max = k + 1 (the first
    primal order at tau = 1) and lists of 3 k; each at tau = 1 and 0.6.  k = 7 has the padding row of the odd ensemble size."""
    case = edge_case(k, p_max, primal)
    cnt = case["cnt"]
    have = set(cnt.tolist())
    assert {0, 1, 2, p_max} <= have and any(c & 1 and c > 2 for c in have)
    assert ({k - 1, k, k + 1} <= have) if primal else (p_max <= k)
    nb = neighbour_lists(mia, cnt, case["idx"], case["rho"], p_max)
    w_in = dev(case["W"], dtype)
    empty = torch.as_tensor(cnt == 0, device=DEV)
    for tau in (1.0, 0.6):
        for vname, eps in VARIANTS:
            W, fl = update(eng, case["W"], case["yb"] * (eps or 1.0), case["d"], nb, tau, eps, dtype)
            err, at = worst_point(W.cpu().numpy(), case["ref"][(tau, vname)])
            print("\n[ienks general] edges %s k %d p_max %d tau %.1f %s: worst point %.3e (point %d, cnt %d)"
                  % (tag(dtype), k, p_max, tau, vname, err, at, cnt[at]))
            assert int((fl & 0xff).max()) == 0, (tau, vname)
            assert torch.equal(W[empty], w_in[empty]) and int(fl[cnt == 0].max()) == 0     # no observation: W_in bit for bit, flag 0
            assert err <= TOL[dtype], (tau, vname, at, int(cnt[at]), err)


# ---- 3. one shared general matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_a_shared_general_matrix_is_that_matrix_repeated(mia, eng, dtype):
    k = 20
    case = sweep_case(k)
    nb = neighbour_lists(mia, case["cnt"], case["idx"], case["rho"], case["p_max"])
    W1 = case["W"][3]
    assert len(pivot_swaps(perts_of(W1))) >= 7
    for tau in (1.0, 0.6):
        for vname, eps in VARIANTS:
            one, f1 = update(eng, W1, case["yb"] * (eps or 1.0), case["d"], nb, tau, eps, dtype)
            rep, f2 = update(eng, np.broadcast_to(W1, (G, k, k)), case["yb"] * (eps or 1.0), case["d"], nb, tau, eps, dtype)
            assert torch.equal(one, rep) and np.array_equal(f1, f2), (tau, vname)
            err, at = worst_point(one.cpu().numpy(), oracle(W1, case["yb"] * (eps or 1.0), case["d"], case["cnt"], case["idx"],
                                                           case["rho"], tau, eps))
            assert err <= TOL[dtype], (tau, vname, at, err)


# ---- 3b. exact ties in the pivot search -------------------------------------------------------------------------------------------
def tied_weights(n, k, seed):
    """(n, k, k) weights whose Wp = blockdiag([[s, 1 - s], [-s, 1 + s]], ...)[perm, :] (rows sum to 1; s in {1/4, 1/2, 3/4}; a
    trailing 1 for odd k) plus c 1^T with c in multiples of 1/8: every number is exact in float32, so the kernel meets |s| twice,
    in two rows a random distance apart, at every even column.  Only those two rows are non-zero there: a search that returned
    anything but one of them would divide by zero."""
    rs = np.random.RandomState(seed)
    out = np.empty((n, k, k))
    for g in range(n):
        Wp = np.zeros((k, k))
        for b in range(0, k - 1, 2):
            sv = rs.choice([0.25, 0.5, 0.75])
            Wp[b:b + 2, b:b + 2] = [[sv, 1.0 - sv], [-sv, 1.0 + sv]]
        if k & 1:
            Wp[k - 1, k - 1] = 1.0
        out[g] = Wp[rs.permutation(k)] + rs.randint(-4, 5, size=(k, 1)) / 8.0
    return out


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("k", [7, 65, 80])
def test_exact_ties_take_the_lower_row(mia, eng, dtype, k):
    """The tie-break across lanes and, above 64 members, across waves: the pivot is one of the two tied rows (the result is the
    oracle's), and the same one every time (two runs give the same bits)."""
    case = sweep_case(k)
    nb = neighbour_lists(mia, case["cnt"], case["idx"], case["rho"], case["p_max"])
    W = tied_weights(G, k, 800 + k)
    assert np.array_equal(perts_of(W.astype(np.float32)).astype(np.float64), perts_of(W))          # exact in float32
    traces = [pivot_trace(perts_of(w)) for w in W]
    assert all(ties == list(range(0, k - 1, 2)) for _, ties in traces) and all(len(sw) >= 1 for sw, _ in traces)
    assert max(np.linalg.cond(perts_of(w)) for w in W) <= 10.0
    for tau, (vname, eps) in ((1.0, VARIANTS[0]), (0.6, VARIANTS[0]), (0.6, VARIANTS[1])):
        yb = case["yb"] * (eps or 1.0)
        got, fl = update(eng, W, yb, case["d"], nb, tau, eps, dtype)
        again, afl = update(eng, W, yb, case["d"], nb, tau, eps, dtype)
        assert torch.equal(got, again) and np.array_equal(fl, afl), (tau, vname)
        err, at = worst_point(got.cpu().numpy(), oracle(W, yb, case["d"], case["cnt"], case["idx"], case["rho"], tau, eps))
        print("\n[ienks general] ties %s k %d tau %.1f %s: worst point %.3e (point %d)" % (tag(dtype), k, tau, vname, err, at))
        assert int((fl & 0xff).max()) == 0, (tau, vname)
        assert err <= TOL[dtype], (tau, vname, at, err)


# ---- 4. shards, repeatability ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", [(torch.float64, 20), (torch.float32, 20), (torch.float64, 65)])
def test_shards_and_repeats_give_the_same_bits(mia, eng, dtype, k):
    case = sweep_case(k)
    for tau, (vname, eps) in ((0.6, VARIANTS[0]), (1.0, VARIANTS[0]), (0.6, VARIANTS[1])):
        yb = case["yb"] * (eps or 1.0)
        nb = neighbour_lists(mia, case["cnt"], case["idx"], case["rho"], case["p_max"])
        full, ffl = update(eng, case["W"], yb, case["d"], nb, tau, eps, dtype)
        again, afl = update(eng, case["W"], yb, case["d"], nb, tau, eps, dtype)
        assert torch.equal(full, again) and np.array_equal(ffl, afl), (tau, vname)
        for g0, g1 in ((5, 21), (17, G), (9, 10)):
            part, pfl = update(eng, case["W"][g0:g1], yb, case["d"],
                               neighbour_lists(mia, case["cnt"], case["idx"], case["rho"], case["p_max"], g0, g1), tau, eps, dtype)
            assert part.shape[0] == g1 - g0
            assert torch.equal(part, full[g0:g1]) and np.array_equal(pfl, ffl[g0:g1]), (tau, vname, g0, g1)


# ---- 5. only_flagged: the retry entries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_retry_entry_redoes_exactly_the_flagged_points(mia, eng, dtype):
    """mia_lienks_update_retry_f32 / _f64 as engine.py calls them: MIA_FLAG_RETRY on a chosen subset, out prefilled."""
    from torch_assimilate_amd.engine import _ptr
    k = 20
    case = sweep_case(k)
    nb = neighbour_lists(mia, case["cnt"], case["idx"], case["rho"], case["p_max"])
    fn = getattr(eng.lib, "mia_lienks_update_retry_" + tag(dtype))
    chosen = np.zeros(G, dtype=bool)
    chosen[[0, 3, 4, 11, 17, 30, 31]] = True
    sel = torch.as_tensor(chosen, device=DEV)
    for tau in (1.0, 0.6):
        for vname, eps in VARIANTS:
            yb = case["yb"] * (eps or 1.0)
            want, wfl = update(eng, case["W"], yb, case["d"], nb, tau, eps, dtype)
            w_in, rec = dev(case["W"], dtype), eng.pack_obs(dev(yb, dtype), dev(case["d"], dtype), dtype)
            out = torch.full((G, k, k), -7.0, dtype=dtype, device=DEV)
            flags = torch.as_tensor(np.where(chosen, RETRY, 0).astype(np.int32), device=DEV)
            rc = fn(_ptr(w_in), k * k, k, nb.g0, nb.g1, _ptr(rec), rec.shape[0], _ptr(nb.cnt), _ptr(nb.idx), _ptr(nb.w), nb.p_cap,
                    nb.p_max, tau, eps or 0.0, _ptr(out), _ptr(flags), eng._stream())
            torch.cuda.synchronize()
            assert rc == 0, (tau, vname)
            fl = flags.cpu().numpy()
            assert torch.equal(out[sel], want[sel]) and np.array_equal(fl[chosen], wfl[chosen]), (tau, vname)
            assert int((fl[chosen] & RETRY).max()) == 0                                # rewritten
            assert bool((out[~sel] == -7.0).all()) and int(np.abs(fl[~chosen]).max()) == 0, (tau, vname)


# ---- 6. float32 "auto": the matrix-function route and its retry on one batch -------------------------------------------------------
def test_float32_auto_on_a_mixed_batch(mia, eng):
    """tau = 1, transform variant: the even points carry I + c 1^T (Wp exactly the identity in float32: c in multiples of 1/8), the
    odd points general weights.  The matrix-function kernel keeps the first and declines the second, which the general kernel
    redoes on the same inputs: the same bits as method="eig"."""
    from torch_assimilate_amd.engine import _ptr
    k, dtype = 20, torch.float32
    case = sweep_case(k)
    nb = neighbour_lists(mia, case["cnt"], case["idx"], case["rho"], case["p_max"])
    general = (np.arange(G) & 1) == 1
    rs = np.random.RandomState(61)
    W = case["W"].copy()
    W[~general] = np.eye(k) + rs.randint(-4, 5, size=(G // 2, k, 1)) / 8.0
    w32 = W.astype(np.float32)
    assert np.array_equal(perts_of(w32[~general]), np.broadcast_to(np.eye(k, dtype=np.float32), (G // 2, k, k)))
    assert_pivoting(W, where=general)
    ref = oracle(W, case["yb"], case["d"], case["cnt"], case["idx"], case["rho"], 1.0, None)
    # the route under "auto" takes this shape, and declines exactly the general points
    w_in, rec = dev(W, dtype), eng.pack_obs(dev(case["yb"], dtype), dev(case["d"], dtype), dtype)
    out = torch.zeros((G, k, k), dtype=dtype, device=DEV)
    flags = torch.zeros(G, dtype=torch.int32, device=DEV)
    retry = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = eng.lib.mia_lienks_update_matfun_f32(_ptr(w_in), k * k, k, nb.g0, nb.g1, _ptr(rec), rec.shape[0], _ptr(nb.cnt), _ptr(nb.idx),
                                              _ptr(nb.w), nb.p_cap, nb.p_max, 0.0, _ptr(out), _ptr(flags), _ptr(retry), eng._stream())
    torch.cuda.synchronize()
    assert rc == 0 and int(retry.item()) == G // 2
    assert np.array_equal((flags.cpu().numpy() & RETRY) != 0, general)
    auto, afl = update(eng, W, case["yb"], case["d"], nb, 1.0, None, dtype, method="auto")
    eig, efl = update(eng, W, case["yb"], case["d"], nb, 1.0, None, dtype, method="eig")
    err, at = worst_point(auto.cpu().numpy(), ref)
    print("\n[ienks general] f32 auto, mixed batch: worst point %.3e (point %d); identity-Wp points %.3e, general points %.3e"
          % (err, at, worst_point(auto.cpu().numpy(), ref, ~general)[0], worst_point(auto.cpu().numpy(), ref, general)[0]))
    assert int((afl & RETRY).max()) == 0 and int((afl & 0xff).max()) == 0
    assert err <= TOL[dtype], (at, err)
    gsel = torch.as_tensor(general, device=DEV)
    assert torch.equal(auto[gsel], eig[gsel]) and np.array_equal(afl[general], efl[general])


# ---- 7. non-finite inputs, refusal ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_a_nan_stays_with_its_points(mia, eng, dtype):
    k = 20
    case = sweep_case(k)
    cnt, idx = case["cnt"], case["idx"]
    nb = neighbour_lists(mia, cnt, idx, case["rho"], case["p_max"])
    for tau in (1.0, 0.6):
        for vname, eps in VARIANTS:
            ref = case["ref"][(tau, vname)]
            yb = case["yb"] * (eps or 1.0)
            # one point's incoming weights hold a NaN
            W = case["W"].copy()
            W[13, 4, 9] = np.nan
            hit = np.arange(G) == 13
            got, fl = update(eng, W, yb, case["d"], nb, tau, eps, dtype)
            assert np.array_equal((fl & NONFINITE) != 0, hit), (tau, vname)
            assert int((fl[~hit] & 0xff).max()) == 0
            err, at = worst_point(got.cpu().numpy(), ref, ~hit)
            assert err <= TOL[dtype], ("W_in", tau, vname, at, err)
            # one observation record holds a NaN
            j = int(idx[0, 0])
            bad = yb.copy()
            bad[2, j] = np.nan
            uses = np.array([j in idx[g, :cnt[g]] for g in range(G)])
            assert 0 < uses.sum() < G
            got, fl = update(eng, case["W"], bad, case["d"], nb, tau, eps, dtype)
            assert np.array_equal((fl & NONFINITE) != 0, uses), (tau, vname)
            assert int((fl[~uses] & 0xff).max()) == 0
            err, at = worst_point(got.cpu().numpy(), ref, ~uses)
            assert err <= TOL[dtype], ("record", tau, vname, at, err)


def test_a_shape_past_the_lds_cap_is_refused(mia, eng):
    k, p_max, P = 128, 8, 40
    assert general_lds_bytes(k, p_max, 1.0, False, 8) > LDS_CAP
    yb, d = observations(k, P, 5)
    cnt, idx, rho = hand_lists([p_max] * 4, P, p_max, 6)
    nb = neighbour_lists(mia, cnt, idx, rho, p_max)
    for tau, eps in ((1.0, None), (0.6, None), (1.0, EPS)):
        with pytest.raises(mia.MiaError):
            eng.ienks_update(torch.eye(k, dtype=torch.float64), dev(yb, torch.float64), dev(d, torch.float64), nb, tau, eps, method="eig")
    torch.cuda.synchronize()

"""A 1-D case of more than 65 536 tiles whose EVERY grid point has a float64 oracle reference (tests/test_gpu_large_grid.py).

The tile kernels launch a two-dimensional grid of blocks once a call holds more than 65 536 tiles of sixteen points.  The oracle
cannot visit a million points in a test of seconds, and does not have to: the weights of a grid point depend only on the
observations around it.  The observing network therefore REPEATS with a period of T = 16 x 61 = 976 grid points (61 tiles: 61
is prime and 65 536 mod 61 = 22, so a tile index that is off by a power of two, or by a multiple of 65 536, never lands on a
tile with the same weights), while the state is random everywhere.  The oracle runs on three windows -- the start of the
domain, one interior period, the end of the domain with the last partial period and its truncated lists -- and the interior
period is laid out over the grid by index arithmetic.  tests/test_large_grid_reference.py pins that against the oracle of a
whole (small) grid.  Test infrastructure: nothing in the product imports this."""
import functools

import numpy as np

from kernel_cases import oracle_kernels
from oracle import letkf_oracle as O

G_LARGE = 16 * 65536 + 16 * 1001 + 5      # 1 064 597 points: 66 538 tiles, a partly filled second block row, a ragged last tile
PERIOD = 16 * 61                          # 976 points
K, M = 8, 2                               # members, state rows (the second row gets +250)
RADIUS, INF = 4.0, 1.1
STRIDE = {"sparse": 2, "dense": 1}        # lists of 7 or 8 entries (p_max <= k) / of about 15 entries (p_max > k)
RBF_GAMMA = 0.5
EXPR_KERNEL = "ornuhl"                    # the bounded kernel of the expression route (tests/kernel_cases.py)
IENKS_EPS = 1e-3                          # bundle variant (tests/test_gpu_ienks64.py)


def make_case(G, network, k=K, m=M, seed=20):
    """grid arange(G), observations at every s-th point with yb, d repeating every PERIOD grid points, state i.i.d. normal"""
    s = STRIDE[network]
    assert PERIOD % s == 0 and G >= 3 * PERIOD
    rs = np.random.RandomState(seed + s)
    tp = PERIOD // s
    hx = rs.normal(size=(k, tp))
    yb_period, d_period = O.obs_space_uncorr(hx, rs.normal(size=tp), np.ones(tp))
    obs_x = np.arange(0, G, s, dtype=np.float64)
    j = np.arange(obs_x.shape[0]) % tp
    state = np.random.RandomState(seed).normal(size=(m, k, G))
    state[1:] += 250.0
    # incoming IEnKS weights, periodic and far from the identity (weights_in of tests/test_gpu_ienks64.py, bundle form)
    a = rs.normal(size=(PERIOD, k, k))
    w_in = (np.eye(k)[None] + 0.1 * rs.normal(size=(PERIOD, k, 1)) * np.ones((1, 1, k))
            + 0.3 * (a - a.mean(axis=2, keepdims=True)) / np.sqrt(k))
    return dict(G=G, network=network, stride=s, k=k, c=RADIUS, inf=INF, grid_x=np.arange(G, dtype=np.float64), obs_x=obs_x,
                yb=np.ascontiguousarray(yb_period[:, j]), d=np.ascontiguousarray(d_period[j]), state=state, w_in_period=w_in)


def rbf_core(p, q, inf):
    return O.ketkf_weights(p, q, lambda x, y: O.rbf_kernel(x, y, RBF_GAMMA), inf)


def expr_core(p, q, inf):
    return O.ketkf_weights(p, q, oracle_kernels()[EXPR_KERNEL], inf)


def oracle_weights(case, core, lo, hi):
    """The oracle's weights (hi - lo, k, k) of the grid points [lo, hi), from the observations within 2 c + 1 of the window (the
    taper's support is 2 c: the rest weighs exactly zero, and the masked arrays are the whole grid's)."""
    margin = 2.0 * case["c"] + 1.0
    ox = case["obs_x"]
    a, b = np.searchsorted(ox, lo - margin, "left"), np.searchsorted(ox, hi - 1 + margin, "right")
    pts = case["grid_x"][lo:hi]
    oxw, yb, d = ox[a:b], case["yb"][:, a:b], case["d"][a:b]
    if core == "ienks":
        w_in = case["w_in_period"][np.arange(lo, hi) % PERIOD]
        return O.lienks_weights(w_in, pts, oxw, yb * IENKS_EPS, d, case["c"], 1.0, IENKS_EPS)
    fn = {"letkf": O.etkf_weights, "rbf": rbf_core, "ornuhl": expr_core}[core]
    return O.letkf_weights(pts, oxw, yb, d, case["c"], case["inf"], core=fn)


class ReplicatedWeights:
    """Reference weights of all G points: the oracle on [0, T), on the interior period [T, 2 T) and on [E0, G), with E0 the last
    multiple of T that leaves 2 c + 1 points and more to the end.  Every point of [T, E0) sees whole lists of a network that
    repeats with T, so its weights are those of the point T + (g mod T)."""

    def __init__(self, case, core):
        G, T = case["G"], PERIOD
        self.G, self.k = G, case["k"]
        self.e0 = T * int((G - 2 * (2.0 * case["c"] + 1.0)) // T)
        assert self.e0 >= 2 * T
        self.start = oracle_weights(case, core, 0, T)
        self.period = oracle_weights(case, core, T, 2 * T)
        self.end = oracle_weights(case, core, self.e0, G)

    def at(self, lo, hi):
        """(hi - lo, k, k) weights of the points [lo, hi)"""
        idx = np.arange(lo, hi)
        out = self.period[idx % PERIOD]
        head, tail = idx < PERIOD, idx >= self.e0
        out[head] = self.start[idx[head]]
        out[tail] = self.end[idx[tail] - self.e0]
        return out

    def analysis(self, state, chunk=1 << 16):
        """O.apply_weights of ``state`` (m, k, G) with these weights, in chunks of points"""
        out = np.empty(state.shape, dtype=np.float64)
        for lo in range(0, self.G, chunk):
            hi = min(self.G, lo + chunk)
            out[:, :, lo:hi] = O.apply_weights(state[:, :, lo:hi], self.at(lo, hi))
        return out

    def errors(self, got, chunk=1 << 16):
        """oracle_pool.per_point_errors for weights ``got`` (G, k, k): every point's relative error and the overall one"""
        from oracle_pool import per_point_errors
        pp = np.empty(self.G)
        num = den = 0.0
        for lo in range(0, self.G, chunk):
            hi = min(self.G, lo + chunk)
            ref, g = self.at(lo, hi), np.asarray(got[lo:hi], dtype=np.float64)
            pp[lo:hi] = per_point_errors(g.transpose(1, 2, 0), ref.transpose(1, 2, 0))[0]
            num += float(((g - ref) ** 2).sum())
            den += float((ref ** 2).sum())
        return pp, float(np.sqrt(num / den))


@functools.lru_cache(maxsize=None)
def large_case(network, k=K, m=M):
    return make_case(G_LARGE, network, k, m)


@functools.lru_cache(maxsize=None)
def large_weights(network, core, k=K, m=M):
    return ReplicatedWeights(large_case(network, k, m), core)


@functools.lru_cache(maxsize=None)
def large_analysis(network, core, k=K, m=M):
    """the float64 reference analysis of every point of the large case; shared by the tests, never written to"""
    ref = large_weights(network, core, k, m).analysis(large_case(network, k, m)["state"])
    ref.setflags(write=False)
    return ref


def regions(G):
    """the three boundary regions of the block grid as point ranges: first tile, tiles 65 535 .. 65 537, ragged last tile"""
    ntile = (G + 15) // 16
    return (("first tile", 0, 16), ("tiles 65535-65537", 16 * 65535, min(G, 16 * 65538)), ("last tile", 16 * (ntile - 1), G))


def reversed_strips(G):
    """tile map (n_tiles, 16) int32: the strips of sixteen consecutive points in REVERSED tile order, the ragged one padded with -1"""
    ntile = (G + 15) // 16
    tp = (16 * np.arange(ntile - 1, -1, -1, dtype=np.int64)[:, None] + np.arange(16)[None]).astype(np.int32)
    tp[tp >= G] = -1
    return tp

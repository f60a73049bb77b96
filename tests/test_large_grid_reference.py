"""Pins tests/large_grid_cases.py on the CPU: on a small grid of three periods plus 37 points the replicated weights equal the
oracle of the WHOLE grid at every point, both boundary regions included -- for both networks, the RBF and the expression core
and the IEnKS update (incoming weights periodic and far from the identity) -- and the networks have the list lengths the GPU
routes of tests/test_gpu_large_grid.py need."""
import numpy as np
import pytest

import large_grid_cases as L
from oracle import letkf_oracle as O

G_SMALL = 3 * L.PERIOD + 37


def test_sizes():
    ntile = (L.G_LARGE + 15) // 16
    assert L.G_LARGE == 1064597 and ntile == 66538 and ntile > 65536 and ntile & 7 == 2 and L.G_LARGE % 16 == 5
    assert L.PERIOD == 976 and 65536 % 61 == 22 and all(61 % p for p in range(2, 8))
    assert all((2 ** e) % 61 for e in range(1, 21))                   # a tile index off by a power of two is never congruent
    tp = L.reversed_strips(L.G_LARGE)
    assert tp.shape == (ntile, 16) and tp.dtype == np.int32
    assert tp[0].tolist() == list(range(16 * (ntile - 1), L.G_LARGE)) + [-1] * 11 and tp[-1].tolist() == list(range(16))
    assert np.array_equal(np.sort(tp[tp >= 0]), np.arange(L.G_LARGE))


@pytest.mark.parametrize("network", ["sparse", "dense"])
def test_list_lengths(network):
    case = L.make_case(G_SMALL, network)
    cnt = np.array([int(O.localize_obs(O.abs_distance_1d(g, case["obs_x"]), [case["c"]])[0].sum()) for g in case["grid_x"]])
    interior = cnt[9:-9]
    if network == "sparse":
        assert set(interior.tolist()) == {7, 8} and cnt.max() <= L.K              # p_max <= k
    else:
        assert set(interior.tolist()) == {15} and cnt.max() > L.K                  # p_max > k
    assert cnt.min() >= 4                                                          # truncated lists at both ends, none empty


@pytest.mark.parametrize("network,core", [("sparse", "letkf"), ("dense", "letkf"), ("sparse", "rbf"), ("sparse", "ornuhl"),
                                          ("sparse", "ienks")])
def test_replicated_weights_equal_the_oracle_of_the_whole_grid(network, core):
    case = L.make_case(G_SMALL, network)
    rep = L.ReplicatedWeights(case, core)
    assert rep.e0 == 3 * L.PERIOD
    full = L.oracle_weights(case, core, 0, G_SMALL)
    if core == "letkf":      # the window is no approximation: the oracle's own loop over all observations gives the same bits
        direct = O.letkf_weights(case["grid_x"], case["obs_x"], case["yb"], case["d"], case["c"], case["inf"])
        assert np.array_equal(full, direct)
    if core == "ienks":
        w_in = case["w_in_period"][np.arange(G_SMALL) % L.PERIOD]
        assert float(np.abs(w_in - np.eye(L.K)).max()) > 0.3                       # far from the identity
        direct = O.lienks_weights(w_in, case["grid_x"], case["obs_x"], case["yb"] * L.IENKS_EPS, case["d"], case["c"], 1.0,
                                  L.IENKS_EPS)
        assert np.array_equal(full, direct)
    assert np.array_equal(rep.at(0, G_SMALL), full)
    assert np.array_equal(rep.at(700, 2100), full[700:2100])
    # the weights differ from tile to tile inside a period: a wrong tile index cannot hide
    t = full[L.PERIOD:2 * L.PERIOD].reshape(61, 16, L.K, L.K)
    assert float(np.abs(t[1:] - t[:-1]).max(axis=(1, 2, 3)).min()) > 1e-3
    ana = rep.analysis(case["state"], chunk=1000)
    assert np.array_equal(ana, O.apply_weights(case["state"], full))
    pp, fro = rep.errors(full + 1e-9 * np.sign(full), chunk=1000)
    assert pp.shape == (G_SMALL,) and 1e-10 < fro < 1e-8 and 1e-10 < pp.max() < 1e-8

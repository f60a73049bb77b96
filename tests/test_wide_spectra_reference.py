"""Pins tests/golden/g10_wide_spectra*.npz (tools/gen_wide_spectra.py, read through tests/wide_spectra_cases.py) on the CPU:
local ETKF problems with lambda_max / reg up to 3e9 whose weights and analysis were computed in 50 decimal digits.

Why the float64 oracle cannot referee these cases: its own error against 50 digits is c u lambda_max / reg with c up to
c_ref = 1.54 (u = 2^-52; the forward error of a backward-stable float64 eigensolve), which passes the 1e-10 contract from
lambda_max / reg ~ 1e6 on and reaches 6.6e-7 at 2.7e9.  The tolerance of every test on this fixture is therefore
tol(block) = max(1e-10, 4 c_ref u kappa): nothing may be worse than 4 x the reference's own float64 arithmetic.  Its teeth:
the same oracle in float32 fails it wherever kappa >= 1e3, and a relative 1e-9 on W fails it wherever kappa <= 1e4."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import wide_spectra_cases as WS
from oracle import letkf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return WS.load()


@pytest.fixture(scope="module")
def oracle_errors(fixture):
    """(error of W, error of xa) of the float64 oracle per block, computed once."""
    out = []
    for b in fixture[0]:
        W = O.etkf_weights(b["yb"].astype(np.float64), b["d"].astype(np.float64)[None], b["inf"]).numpy()
        xa = O.apply_weights(b["x"].astype(np.float64)[:, :, None], W)[:, :, 0]
        out.append((WS.rel_fro(W, b["W"]), WS.rel_fro(xa, b["xa"])))
    return out


def test_the_blocks_are_the_ones_the_routes_need(fixture):
    blocks, c_ref = fixture
    shapes = {(b["k"], b["p"]) for b in blocks}
    assert shapes == {(16, 7), (16, 8), (16, 24), (27, 21), (27, 32), (40, 20), (40, 48), (64, 47), (64, 48), (64, 72)}
    for k, p in shapes:
        here = [b for b in blocks if (b["k"], b["p"]) == (k, p)]
        fams = {(b["family"], b["s"]) for b in here if b["inf"] == 1.1}
        want = {(f, s) for f in ("graded", "twolevel") for s in (30.0, 1e3, 3e4)}
        if k in (16, 40):
            want |= {("repeated", 1e3), ("deficient", 1e3), ("weak", 1e-8)}
        assert fams == want
    assert sorted(b["k"] for b in blocks if b["inf"] == 1.0) == [16, 27, 40, 64]
    for b in blocks:
        # float32-representable by construction: exact input for both dtypes
        assert b["yb"].dtype == b["d"].dtype == b["x"].dtype == np.float32 and b["W"].dtype == b["xa"].dtype == np.float64
        if b["family"] == "weak":
            assert b["kappa"] < 1e-15 and WS.rel_fro(b["W"], np.sqrt(b["inf"]) * np.eye(b["k"])) < 1e-15
        else:
            assert 0.3 * b["s"] ** 2 < b["kappa"] < 8.0 * b["s"] ** 2           # lambda_max / reg ~ 2 s^2
        if b["family"] == "repeated":
            assert np.array_equal(b["yb"][:, 0], b["yb"][:, 1]) and np.array_equal(b["yb"][:, 2], b["yb"][:, 3])
        if b["family"] == "deficient":
            assert np.array_equal(b["yb"][0], b["yb"][1]) and np.array_equal(b["x"][:, 0], b["x"][:, 1])
    strong = [b for b in blocks if b["kappa"] >= WS.STRONG]
    worst = max(max(b["e_ref_W"], b["e_ref_xa"]) / (WS.U * b["kappa"]) for b in strong)
    assert worst == c_ref and 0.5 < c_ref < 4.0
    for name in WS.FILES:
        assert os.path.getsize(os.path.join(WS.GOLDEN, name)) <= 1 << 20


def test_regenerating_the_smallest_blocks_gives_the_fixture(fixture):
    """Pins the generator, the seed and the 50-digit truth: W and xa to 2 ulp."""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("gen_wide_spectra", os.path.join(ROOT, "tools", "gen_wide_spectra.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    blocks, _ = fixture
    sp = gen.specs()
    assert [(b["k"], b["p"], b["family"], b["s"], b["inf"]) for b in blocks] == sp
    for i in sorted(range(len(blocks)), key=lambda i: (blocks[i]["k"] * blocks[i]["p"], i))[:2]:
        b = blocks[i]
        yb, d, x = gen.make_inputs(i, sp[i])
        assert np.array_equal(yb, b["yb"]) and np.array_equal(d, b["d"]) and np.array_equal(x, b["x"])
        W, xa, kappa = gen.truth(yb, d, x, sp[i][4])
        assert np.all(np.abs(W - b["W"]) <= 2 * np.spacing(np.abs(b["W"])))
        assert np.all(np.abs(xa - b["xa"]) <= 2 * np.spacing(np.abs(b["xa"])))
        assert abs(kappa - b["kappa"]) <= 1e-12 * b["kappa"]


def test_the_float64_oracle_is_within_tol_but_not_within_the_contract(fixture, oracle_errors):
    blocks, c_ref = fixture
    for b, (eW, exa) in zip(blocks, oracle_errors):
        assert max(eW, exa) < WS.tol(b, c_ref), (b["index"], b["k"], b["p"], b["family"], eW, exa)
    worst = max(max(e) for e in oracle_errors)
    print("float64 oracle against 50 digits: worst %.2e, c_ref %.3f" % (worst, c_ref))
    assert worst > WS.FLOOR          # the oracle alone misses 1e-10 on these cases: it cannot be their referee


def test_teeth_a_float32_eigensolve_fails(fixture):
    blocks, c_ref = fixture
    strong = [b for b in blocks if b["kappa"] >= WS.STRONG]
    assert len(strong) > 60
    for b in strong:
        w_mean, w_perts, _ = O.etkf_weights_parts(torch.from_numpy(b["yb"]), torch.from_numpy(b["d"])[None], b["inf"])
        W = (w_mean + w_perts).numpy()
        assert W.dtype == np.float32
        xa = O.apply_weights(b["x"].astype(np.float64)[:, :, None], W.astype(np.float64))[:, :, 0]
        assert WS.rel_fro(W, b["W"]) > WS.tol(b, c_ref), (b["index"], b["kappa"])
        assert WS.rel_fro(xa, b["xa"]) > WS.tol(b, c_ref), (b["index"], b["kappa"])


def test_teeth_a_relative_1e_9_on_the_weights_fails(fixture):
    blocks, c_ref = fixture
    mild = [b for b in blocks if b["kappa"] <= 1e4]
    assert len(mild) >= 20
    for b in mild:
        assert WS.tol(b, c_ref) == WS.FLOOR
        assert WS.rel_fro(b["W"] * (1 + 1e-9), b["W"]) > WS.tol(b, c_ref)

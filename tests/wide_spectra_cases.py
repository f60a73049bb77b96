"""Reader of tests/golden/g10_wide_spectra*.npz (tools/gen_wide_spectra.py): local ETKF problems solved in 50 digits, and the
tolerance their tests share.  Needs numpy only; tests/test_wide_spectra_reference.py pins it on the CPU."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("g10_wide_spectra.npz", "g10_wide_spectra_k64.npz")
U = 2.0 ** -52
FLOOR = 1e-10           # the project's float64 contract
TOL32 = 1e-5            # ... and the float32 one
STRONG = 1e3            # lambda_max / reg from which c_ref is taken


def load():
    """(blocks, c_ref): every block of both files in the generator's order, as dicts of k, p, family, s, inf, index, kappa,
    e_ref_W, e_ref_xa, yb (k, p) / d (p,) / x (2, k) float32 and W (k, k) / xa (2, k) float64."""
    blocks, c_ref = [], None
    for name in FILES:
        z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
        c = float(z["c_ref"])
        assert c_ref is None or c == c_ref
        c_ref = c
        off = dict(yb=0, d=0, x=0, W=0, xa=0)
        flat = {key: z[key] for key in off}

        def take(key, shape):
            n = int(np.prod(shape))
            a = flat[key][off[key]:off[key] + n].reshape(shape)
            off[key] += n
            return a
        for i in range(len(z["k"])):
            k, p = int(z["k"][i]), int(z["p"][i])
            blocks.append(dict(
                k=k, p=p, family=str(z["family"][i]), s=float(z["s"][i]), inf=float(z["inf"][i]), index=int(z["index"][i]),
                kappa=float(z["kappa"][i]), e_ref_W=float(z["e_ref_W"][i]), e_ref_xa=float(z["e_ref_xa"][i]),
                yb=take("yb", (k, p)), d=take("d", (p,)), x=take("x", (2, k)), W=take("W", (k, k)), xa=take("xa", (2, k))))
        assert all(off[key] == flat[key].size for key in off)
    assert [b["index"] for b in blocks] == list(range(len(blocks)))
    return blocks, c_ref


def tol(block, c_ref):
    """1e-10, or 4 x the float64 reference's own error where that is larger: c_ref is the worst constant the float64 oracle shows
    against 50 digits in e = c u lambda_max / reg on these blocks; the factor 4 is room for another rounding sample (another
    BLAS, another summation order, Jacobi instead of divide and conquer), not for another power of kappa."""
    return max(FLOOR, 4.0 * c_ref * U * block["kappa"])


def rel_fro(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))

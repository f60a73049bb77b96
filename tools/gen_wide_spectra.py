"""Writes tests/golden/g10_wide_spectra.npz and g10_wide_spectra_k64.npz: local ETKF problems with wide, clustered, repeated
and deficient spectra, solved in 50 decimal digits with mpmath -- the referee of the float64 eigensolver paths where the
float64 oracle's own error (about u * lambda_max / reg, u = 2^-52) passes the 1e-10 contract.

A block is one local problem: yb (k, p), d (p,), two state rows x (2, k) and inf; the taper weight of every observation is 1.
Inputs: RandomState(SEED0 + index), yb centred over the members, the family's column scaling applied to yb and d, then
yb, d, x rounded to float32-representable values -- the same block is exact input for float32 and float64 arrays.
Truth: eigsy of the k x k matrix yb yb^T at dps = 50, clamp at 0, + reg, W = w_mean + w_perts as oracle.etkf_weights_parts,
xa = mean + (x - mean) W; both rounded to float64.

Families (lambda_max / reg ~ 2 s^2):
  graded    column j times s^(j / (p - 1)), s in {30, 1e3, 3e4}
  twolevel  the second half of the columns times s, same three s (clustered eigenvalues)
  repeated  ceil(p / 2) distinct columns graded with s = 1e3, each stored twice (the last one once where p is odd): exactly
            repeated and exactly zero eigenvalues in the dual form
  deficient members 0 and 1 identical (yb and x), two-level with s = 1e3
  weak      every column times 1e-8: the analysis is the inflated prior to rounding
All at inf = 1.1; one graded s = 1e3 block per k at inf = 1.0.  All families at k = 16 and 40, graded and two-level at k = 27
and 64.

Needs mpmath; minutes on a CPU (the blocks are solved in parallel processes).  Stored flat, see tests/wide_spectra_cases.py
for the reader.  `python tools/gen_wide_spectra.py [--check]`: --check compares with the committed files instead of writing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# two files, so that each stays below the repository's limit of 1 MiB per file: ensembles up to 40 members (and c_ref, which
# is taken over ALL blocks) in the first, k = 64 in the second; tests/wide_spectra_cases.py reads them as one list
FILES = (("g10_wide_spectra.npz", lambda k: k < 64), ("g10_wide_spectra_k64.npz", lambda k: k >= 64))
SEED0 = 20100
U = 2.0 ** -52
DPS = 50

# k: (p of the dual form ..., p of the primal form)
SHAPES = {16: (7, 8, 24), 27: (21, 32), 40: (20, 48), 64: (47, 48, 72)}
STRENGTHS = (30.0, 1e3, 3e4)
ALL_FAMILIES = (16, 40)


def specs():
    """[(k, p, family, s, inf)] in the order of the file; the block's seed is SEED0 + its index."""
    out = []
    for k, ps in SHAPES.items():
        for p in ps:
            out += [(k, p, "graded", s, 1.1) for s in STRENGTHS]
            out += [(k, p, "twolevel", s, 1.1) for s in STRENGTHS]
            if k in ALL_FAMILIES:
                out += [(k, p, "repeated", 1e3, 1.1), (k, p, "deficient", 1e3, 1.1), (k, p, "weak", 1e-8, 1.1)]
        out.append((k, ps[0], "graded", 1e3, 1.0))
    return out


def make_inputs(index, spec):
    k, p, family, s, inf = spec
    rs = np.random.RandomState(SEED0 + index)
    hx = rs.normal(size=(k, p))
    d = rs.normal(size=p)
    x = rs.normal(size=(2, k))
    if family == "deficient":
        hx[1], x[:, 1] = hx[0], x[:, 0]
    yb = hx - hx.mean(axis=0)
    if family == "graded":
        scale = s ** (np.arange(p) / (p - 1.0))
    elif family in ("twolevel", "deficient"):
        scale = np.where(np.arange(p) >= p // 2, s, 1.0)
    elif family == "repeated":
        nd = (p + 1) // 2
        src = np.arange(p) // 2
        yb, scale = yb[:, src], (s ** (np.arange(nd) / (nd - 1.0)))[src]
    elif family == "weak":
        scale = np.full(p, s)
    else:
        raise ValueError(family)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f32(yb * scale), f32(d * scale), f32(x)


def truth(yb, d, x, inf):
    """W (k, k), xa (2, k) rounded to float64 and lambda_max / reg, from the 50-digit spectrum of yb yb^T."""
    import mpmath as mp
    mp.mp.dps = DPS
    k, p = yb.shape
    Y = mp.matrix(yb.astype(np.float64).tolist())
    evals, V = mp.eigsy(Y * Y.T)
    reg = mp.mpf(k - 1) / mp.mpf(float(inf))
    lam = [(e if e > 0 else mp.mpf(0)) + reg for e in evals]
    einv = [1 / l for l in lam]
    root = [mp.sqrt((k - 1) * e) for e in einv]
    t = V.T * (Y * mp.matrix(d.astype(np.float64).tolist()))
    for i in range(k):
        t[i] *= einv[i]
    w_mean = V * t
    VR = V.copy()
    for i in range(k):
        for j in range(k):
            VR[i, j] *= root[j]
    w_perts = VR * V.T
    W = mp.matrix(k, k)
    for i in range(k):
        for j in range(k):
            W[i, j] = w_mean[i] + w_perts[i, j]
    X = mp.matrix(x.astype(np.float64).tolist())
    xa = np.empty((2, k))
    for r in range(2):
        mean = sum(X[r, i] for i in range(k)) / k
        pert = mp.matrix([[X[r, i] - mean for i in range(k)]])
        row = pert * W
        xa[r] = [float(mean + row[0, j]) for j in range(k)]
    Wd = np.array([[float(W[i, j]) for j in range(k)] for i in range(k)])
    return Wd, xa, float(max(evals) / reg)


def rel_fro(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def oracle_errors(yb, d, x, inf, W, xa):
    """Relative Frobenius error of the float64 oracle on the same inputs against the truth."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import letkf_oracle as O
    Wo = O.etkf_weights(yb.astype(np.float64), d.astype(np.float64)[None, :], inf).numpy()
    xo = O.apply_weights(x.astype(np.float64)[:, :, None], Wo)[:, :, 0]
    return rel_fro(Wo, W), rel_fro(xo, xa)


def solve_block(job):
    index, spec = job
    yb, d, x = make_inputs(index, spec)
    W, xa, kappa = truth(yb, d, x, spec[4])
    eW, exa = oracle_errors(yb, d, x, spec[4], W, xa)
    return dict(yb=yb, d=d, x=x, W=W, xa=xa, kappa=kappa, e_ref_W=eW, e_ref_xa=exa)


def solve_all(nproc):
    import multiprocessing as mpc
    sp = specs()
    jobs = sorted(enumerate(sp), key=lambda j: -j[1][0] ** 3)       # the largest first
    with mpc.get_context("fork").Pool(nproc) as pool:
        done = dict(zip([j[0] for j in jobs], pool.map(solve_block, jobs, chunksize=1)))
    return [done[i] for i in range(len(sp))]


def c_ref_of(blocks):
    kappa = np.array([b["kappa"] for b in blocks])
    worst = np.array([max(b["e_ref_W"], b["e_ref_xa"]) for b in blocks])
    strong = kappa >= 1e3
    return float((worst[strong] / (U * kappa[strong])).max())


def pack(blocks, index, c_ref):
    """The arrays of one file: the blocks ``index`` of the list, matrices flattened and concatenated in that order."""
    sp = specs()
    col = lambda j, dt: np.array([sp[i][j] for i in index], dtype=dt)
    num = lambda key: np.array([blocks[i][key] for i in index], dtype=np.float64)
    flat = lambda key, dt: np.concatenate([blocks[i][key].ravel() for i in index]).astype(dt)
    return dict(
        index=np.array(index, dtype=np.int32), k=col(0, np.int32), p=col(1, np.int32), family=col(2, str), s=col(3, np.float64),
        inf=col(4, np.float64), seed=SEED0 + np.array(index, dtype=np.int32), kappa=num("kappa"), e_ref_W=num("e_ref_W"),
        e_ref_xa=num("e_ref_xa"), c_ref=np.float64(c_ref), yb=flat("yb", np.float32), d=flat("d", np.float32),
        x=flat("x", np.float32), W=flat("W", np.float64), xa=flat("xa", np.float64))


def main(argv):
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    torch.set_num_threads(1)
    sp = specs()
    blocks = solve_all(min(16, os.cpu_count() or 1))
    for i, (s, b) in enumerate(zip(sp, blocks)):
        print("%3d  k %2d p %2d %-9s s %-7g inf %.1f  kappa %.3g  oracle W %.2g xa %.2g" % (
            i, s[0], s[1], s[2], s[3], s[4], b["kappa"], b["e_ref_W"], b["e_ref_xa"]))
    c_ref = c_ref_of(blocks)
    print("c_ref = %.4g over %d blocks" % (c_ref, len(sp)))
    status = 0
    for name, want in FILES:
        path = os.path.join(GOLDEN, name)
        data = pack(blocks, [i for i, s in enumerate(sp) if want(s[0])], c_ref)
        if "--check" in argv:
            old = np.load(path, allow_pickle=False)
            bad = [key for key in data if not np.array_equal(old[key], data[key])]
            print("%s differs in: %s" % (name, bad or "nothing"))
            status |= bool(bad)
        else:
            np.savez_compressed(path, **data)
            print("wrote %s, %d bytes" % (name, os.path.getsize(path)))
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Float64 kernel-expression analysis time (LKETKF with a positive semidefinite kernel other than a lone RBF / Gauss kernel in the
default dtype): the Jacobi expression route (method="eig": letkf_wave_kernel<double> with the program, what every such filter ran on
before) against the kernel-expression tile route
(method="kern64": lketkf_tile64_kernel<UT, NR, ST>), alternating in ONE process.  Sibling of tools/time_rbf64.py.

    python tools/time_kern64.py                      # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_kern64.py --case 40,2,10,1     # one case (k, obs stride, radius, state rows) in this process, every kernel
    python tools/time_kern64.py --case mesh,40,316,2,2.5,1   # n x n mesh (k, n, obs stride, radius, state rows)
    python tools/time_kern64.py --out profiles/kern64_time.json

1e5 grid points (99 856 on the mesh), seeded inputs, inflation 1.1; neighbour lists and packed records are built once outside the
timed region.  One kernel per statistics set and degree class: `rational` (sq), `ornuhl` (l1), `poly2` (dot, high degrees),
`poly_plus_ornuhl_times_scale` (all three).  The kern64 time INCLUDES the 8-byte read of the decline counter and the redo of the
declined points by the Jacobi kernel, i.e. what ``analysis(method="kern64")`` costs its caller; `reps` calls per sample, `rounds`
samples per method, the methods alternating.  Reported per case and kernel: median and min-max of both, their ratio, the declined
count, the mean and largest degree, and the relative difference of the two routes' analyses."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 1.1
# config 5's network at one and eight state rows; k = 20; a small ensemble (p 12); the 316 x 316 mesh in row-major order with
# observations at every second point (p <= 21: sixteen consecutive points see far more observations than one: tiles in parts)
CASES = ["40,2,10,1", "40,2,10,8", "20,2,10,1", "20,2,10,8", "8,2,6,1", "8,2,6,8", "mesh,40,316,2,2.5,1", "mesh,40,316,2,2.5,8"]
KERNELS = ["rational", "ornuhl", "poly2", "poly_plus_ornuhl_times_scale"]


def kernels():
    sys.path.insert(0, ROOT)
    from torch_assimilate_amd import kernels as K
    return dict(rational=K.RationalKernel(2.0, 1.5), ornuhl=K.OrnsteinUhlenbeckKernel(6.0), poly2=K.PolyKernel(2.0, 1.0),
                poly_plus_ornuhl_times_scale=K.PolyKernel(2.0, 1.0) + K.OrnsteinUhlenbeckKernel(4.0) * K.ScaleKernel(3.0))


def one_case(spec, rounds, names):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    f = spec.split(",")
    mesh = f[0] == "mesh"
    if mesh:       # n x n mesh, Euclidean distance, an observation at every stride-th point of both dimensions (tools/time_rbf64.py's recipe)
        k, n, stride, c, m = int(f[1]), int(f[2]), int(f[3]), float(f[4]), int(f[5])
        gy, gx_ = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
        gx = np.stack([gx_.ravel(), gy.ravel()], axis=1)
        sel = ((gx[:, 0] % stride) == 0) & ((gx[:, 1] % stride) == 0)
        ox = gx[sel]
        gen = torch.Generator(device="cpu").manual_seed(42)
        X = torch.randn((1, k, n * n), generator=gen, dtype=torch.float64).to(dev)
        y = torch.randn(int(sel.sum()), generator=gen, dtype=torch.float64).to(dev)
        hx = X[0][:, torch.as_tensor(sel, device=dev)]
        Yb, d = hx - hx.mean(dim=0), y - hx.mean(dim=0)
    else:
        k, stride, c, m = int(f[0]), int(f[1]), float(f[2]), int(f[3])
        X, gx, ox, Yb, d = bench.make_case(100000, k, stride, dev, seed=42)
        X, Yb, d = X.double(), Yb.double(), d.double()
    G = X.shape[-1]
    if m > 1:
        X = (X.repeat(m, 1, 1) * torch.linspace(0.5, 2.0, m, device=dev, dtype=torch.float64)[:, None, None]).contiguous()
    nb = eng.localize(gx, ox, [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
    outs = {"eig": torch.empty_like(X), "kern64": torch.empty_like(X)}
    flags = torch.empty(G, dtype=torch.int32, device=dev)
    retry = torch.zeros(1, dtype=torch.int32, device=dev)
    case = dict(k=k, obs_stride=stride, radius=c, state_rows=m, grid_points=G, p_max=int(nb.p_max), inf_factor=INF,
                mesh=(n if mesh else 0))
    results = []
    for name in names:
        prog = kernels()[name].program()

        def call(method):
            if method == "kern64":
                retry.zero_()
            return eng.analysis(X, None, None, nb, INF, rec=rec, kernel_program=prog, kernel_psd=True, method=method, out=outs[method],
                                flags=flags, retry=retry)           # (kern64: counter read and redo inside)

        def sample(method, reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call(method)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / reps

        res = {"case": case, "kernel_function": name}
        call("eig")              # warm-up (table, code objects, clocks)
        torch.cuda.synchronize()
        # the first kern64 call with the redo left out: the declined count and the degrees as the tile kernel reports them
        retry.zero_()
        eng.analysis(X, None, None, nb, INF, rec=rec, kernel_program=prog, kernel_psd=True, method="kern64", out=outs["kern64"],
                     flags=flags, retry=retry, defer_retry=True)
        torch.cuda.synchronize()
        res["kernel"] = _cabi.last_analysis_kernel()
        res["declined"] = int(retry.item())
        own = (flags & 0xff) == 0
        deg = ((flags >> 8) & 0xff)[own].double()
        if deg.numel():
            res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
        call("kern64")
        torch.cuda.synchronize()
        diff = outs["kern64"] - outs["eig"]
        res["rel_diff_kern64_vs_eig"] = float((diff.norm() / outs["eig"].norm()).item())
        ts = {"eig": [], "kern64": []}
        for _ in range(rounds):
            ts["eig"].append(sample("eig", 1))
            ts["kern64"].append(sample("kern64", 2))
        for method in ("eig", "kern64"):
            v = np.array(ts[method])
            res[method] = dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), rounds=[float(x) for x in v])
        res["ratio_eig_over_kern64"] = res["eig"]["ms_median"] / res["kern64"]["ms_median"]
        # "at least 2x faster beyond both spreads": the slowest kern64 sample against the fastest Jacobi sample
        res["twice_as_fast_beyond_both_spreads"] = bool(res["eig"]["ms_min"] >= 2.0 * res["kern64"]["ms_max"])
        results.append(res)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--cases", help="semicolon-separated cases in the place of the built-in list")
    ap.add_argument("--kernels", default=",".join(KERNELS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    names = a.kernels.split(",")
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, names)))
        return 0
    results = []

    def dump(extra=None):
        return json.dumps(dict({"tool": "tools/time_kern64.py", "results": results}, **(extra or {})), indent=1)
    for spec in (a.cases.split(";") if a.cases else CASES):    # one fresh process per case, each under its own time limit; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds), "--kernels", a.kernels],
                               capture_output=True, text=True, timeout=a.timeout)
            status, tail = r.returncode, r.stdout[-2000:] + r.stderr[-4000:]
        except subprocess.TimeoutExpired as err:       # (the child is killed; reported like any other failed case)
            status, tail = "timeout after %d s" % a.timeout, str(err.stderr or "")[-4000:]
        if status != 0:
            sys.stderr.write(tail)
            failed = dump({"failed_case": spec, "exit_status": status})
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(failed + "\n")
            print(failed)
            return 1
        for res in json.loads(r.stdout.strip().splitlines()[-1]):
            results.append(res)
            print("%s %s: eig %.3f ms, kern64 %.3f ms (%.2fx), declined %d, degrees %.1f / %s, diff %.1e" % (
                spec, res["kernel_function"], res["eig"]["ms_median"], res["kern64"]["ms_median"], res["ratio_eig_over_kern64"],
                res["declined"], res.get("degree_mean", 0.0), res.get("degree_max"), res["rel_diff_kern64_vs_eig"]), file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(dump() + "\n")
    print(dump())
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Float64 IEnKS update time, tau = 1: the general kernel (LetkfEngine.ienks_update(method="eig"): ienks_update_kernel<double, 256>,
Gauss-Jordan and a Jacobi eigensolve from LDS, one workgroup per grid point) against the tile kernel of csrc/lienks_tile64.hip
(method="tile64": lienks_update64_kernel), alternating in ONE process -- and one LocalizedIEnKSBundle.update_state_arrays loop.

    python tools/time_ienks64.py                           # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_ienks64.py --case 40,2,10,bundle     # one case (k, obs stride, radius, variant) in this process
    python tools/time_ienks64.py --case loop               # the class loop alone
    python tools/time_ienks64.py --out profiles/ienks64_time.json

Config 2 geometry at 1e5 grid points, seeded inputs, neighbour lists and packed records built once outside the timed region;
device events around `reps` calls per sample -- as many as make 120 ms of device work --, `rounds` samples per method, the methods
alternating.  The tile route is timed alone (deferred counter read) and as called by default (with the 8-byte read, a host sync per
call).  Bundle variant: per-point incoming weights (n, k, k) with Wp far from I (every iteration of a loop looks like this);
transform variant: ONE shared prior matrix (the only transform input the route accepts: the first iteration).  Reported per
case: median and spread (max - min over rounds) of the three, the ratios of the first to the other two, the kernel names, the
decline count, the mean degree and the difference between the two kernels' results.  The loop: max_iter = 3 at k = 40 in float64,
wall clock around a synchronised call, with LetkfEngine.IENKS64_AUTO_MIN_K set to 2 (auto hands over) and to 65 (it does not),
alternating.  The tool stops at the first case that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["40,2,10,bundle", "40,2,10,transform", "20,2,5,bundle", "20,2,5,transform", "64,2,16,bundle", "64,2,16,transform", "loop"]
G = 100000
EPS = 1e-3


def stats(v):
    import numpy as np
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), spread_ms=float(v.max() - v.min()),
                rounds=[float(x) for x in v])


def one_case(spec, rounds, window_ms=120.0):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    k, stride, c, variant = spec.split(",")
    k, stride, c = int(k), int(stride), float(c)
    bundle = variant == "bundle"
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    _, gx, ox, Yb, d = bench.make_case(G, k, stride, dev, seed=42)
    Yb, d = Yb.double(), d.double()
    nb = eng.localize(gx, ox, [c])
    eps = EPS if bundle else None
    rec = eng.pack_obs(Yb * EPS if bundle else Yb, d, torch.float64)
    gen = torch.Generator(device=dev).manual_seed(7)
    if bundle:
        A = torch.randn((G, k, k), dtype=torch.float64, device=dev, generator=gen)
        A -= A.mean(dim=2, keepdim=True)
        m = torch.randn((G, k, 1), dtype=torch.float64, device=dev, generator=gen)
        W_in = torch.eye(k, dtype=torch.float64, device=dev) + 0.3 / k ** 0.5 * A + 0.1 * m
        del A, m
    else:
        W_in = torch.eye(k, dtype=torch.float64, device=dev)
    res = {"case": dict(k=k, obs_stride=stride, radius=c, variant=variant, grid_points=G, p_max=int(nb.p_max),
                        weights_in="(n, k, k)" if bundle else "(k, k) shared prior", weights_bytes=G * k * k * 8)}
    W = torch.empty((G, k, k), dtype=torch.float64, device=dev)
    We = torch.empty((G, k, k), dtype=torch.float64, device=dev)

    def eig():
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="eig", out=We)

    def tiles():            # the kernel alone: the 8-byte read of the decline counter is left out
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="tile64", out=W, return_flags=True, defer_retry=True)

    def tiles_sync():       # what a caller pays by default: kernel + counter read (a host sync per call)
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="tile64", out=W)

    def sample(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps
    names = {}
    for n, fn in (("eig", eig), ("tile64_with_counter_read", tiles_sync), ("tile64", tiles)):      # warm-up (table, code objects, clocks)
        for _ in range(2):
            r = fn()
        torch.cuda.synchronize()
        names[n] = _cabi.last_analysis_kernel()
    _, flags, finish = r
    res["declined"] = int(finish())
    torch.cuda.synchronize()
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    res["rel_diff_eig_vs_tile64"] = float((torch.linalg.norm(We - W) / torch.linalg.norm(We)).item())
    # every timed sample holds at least `window_ms` of device work (measuring-on-mi355x: no short windows)
    fns = {"eig": eig, "tile64": tiles, "tile64_with_counter_read": tiles_sync}
    reps = {n: max(2, int(-(-window_ms // max(sample(fn, 2), 1e-3)))) for n, fn in fns.items()}
    ts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ts[n].append(sample(fn, reps[n]))
    for n in fns:
        res[n] = dict(kernel=names[n], reps_per_sample=reps[n], **stats(ts[n]))
    res["ratio_eig_over_tile64"] = res["eig"]["ms_median"] / res["tile64"]["ms_median"]
    # the figure the hand-over rule reads: what ienks_update pays (counter read included)
    res["ratio_eig_over_tile64_with_counter_read"] = res["eig"]["ms_median"] / res["tile64_with_counter_read"]["ms_median"]
    res["ratio_worst_case"] = res["eig"]["ms_min"] / res["tile64_with_counter_read"]["ms_max"]
    res["GB_per_s_tile64"] = (2 if bundle else 1) * G * k * k * 8 / (res["tile64"]["ms_median"] * 1e-3) / 1e9
    return res


def loop_case(rounds, k=40, stride=2, c=10.0, max_iter=3):
    """LocalizedIEnKSBundle.update_state_arrays with a toy linear model and an identity observation operator on every second grid
    point (the loop of tests/test_gpu_ienks.py::test_update_state_loop_vs_oracle), float64 end to end"""
    import torch
    sys.path.insert(0, ROOT)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    gen = torch.Generator(device=dev).manual_seed(21)
    state = torch.randn((1, k, G), dtype=torch.float64, device=dev, generator=gen)
    gx = torch.arange(G, dtype=torch.float64).numpy()
    ox = gx[::stride].copy()
    y = torch.randn(ox.shape[0], dtype=torch.float64, device=dev, generator=gen)
    var = torch.full((ox.shape[0],), 0.5, dtype=torch.float64, device=dev)

    def forward_model(x, it):
        nxt = 0.9 * x + 0.1 * torch.roll(x, 1, dims=-1)
        return nxt, nxt

    def observe(pseudo):
        return [pseudo[0][:, ::stride]], [y], [var], None
    a = mia.LocalizedIEnKSBundle(forward_model, mia.GaspariCohn(c, mia.AbsoluteDistance()), tau=1.0, epsilon=EPS, max_iter=max_iter,
                                 dtype=torch.float64, engine=eng)
    res = {"case": dict(loop="LocalizedIEnKSBundle.update_state_arrays", k=k, obs_stride=stride, radius=c, max_iter=max_iter,
                        grid_points=G, dtype="float64")}
    shipped = mia.LetkfEngine.IENKS64_AUTO_MIN_K
    res["IENKS64_AUTO_MIN_K_of_the_build_measured"] = shipped
    out, ts, kern = {}, {"general": [], "tile64": []}, {}
    try:
        for _ in range(1 + max(3, rounds)):             # (the first pass of both is the warm-up)
            for n, gate in (("general", 65), ("tile64", 2)):
                mia.LetkfEngine.IENKS64_AUTO_MIN_K = gate
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[n] = a.update_state_arrays(state, observe, grid_coords=gx, obs_coords=ox)
                torch.cuda.synchronize()
                ts[n].append((time.perf_counter() - t0) * 1e3)
                kern[n] = _cabi.last_analysis_kernel()
    finally:
        mia.LetkfEngine.IENKS64_AUTO_MIN_K = shipped
    for n in ts:
        res[n] = dict(last_reported_kernel=kern[n], **stats(ts[n][1:]))
    res["ratio_general_over_tile64"] = res["general"]["ms_median"] / res["tile64"]["ms_median"]
    res["rel_diff_of_the_analyses"] = float((torch.linalg.norm(out["general"] - out["tile64"]) / torch.linalg.norm(out["general"])).item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=280)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(loop_case(a.rounds) if a.case == "loop" else one_case(a.case, a.rounds)))
        return 0
    results = []
    for spec in CASES:          # one fresh process per case, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            rc, so, se = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as exc:
            rc, so, se = 124, str(exc.stdout or ""), str(exc.stderr or "")
        if rc != 0:
            sys.stderr.write(so[-2000:] + se[-4000:])
            print(json.dumps({"failed_case": spec, "exit_status": rc, "results": results}))
            return 1
        results.append(json.loads(so.strip().splitlines()[-1]))
        print("%s: %s" % (spec, json.dumps({n: round(v["ms_median"], 3) for n, v in results[-1].items()
                                            if isinstance(v, dict) and "ms_median" in v})), file=sys.stderr, flush=True)
    doc = {"tool": "tools/time_ienks64.py", "build": a.label, "grid_points": G, "results": results}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

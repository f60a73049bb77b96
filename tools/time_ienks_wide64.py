#!/usr/bin/env python3
"""Float64 IEnKS update time above 64 members, tau = 1: the general kernel (LetkfEngine.ienks_update(method="eig"):
ienks_update_kernel<double, 256>, Gauss-Jordan and a Jacobi eigensolve from LDS, one workgroup per grid point -- where it can hold
the shape at all) against the wide tile kernel of csrc/lienks_wide64.hip (method="wide64": lienks_wide64_kernel), alternating in
ONE process.  Sibling of tools/time_ienks64.py and tools/time_wide64w.py.

    python tools/time_ienks_wide64.py                                   # every case below, one child process each (own time limit)
    python tools/time_ienks_wide64.py --case 80,1,16.5,100000,bundle    # one case (k, obs stride, radius, grid points, variant[, baseline])
    python tools/time_ienks_wide64.py --case 64,1,15,100000,bundle,tile64     # ... against lienks_update64_kernel: what the barriers cost
    python tools/time_ienks_wide64.py --out profiles/ienks_wide64_time.json

1-D geometry of bench.make_case, seeded inputs, neighbour lists and packed records built once outside the timed region; device
events around `reps` calls per sample -- as many as make 120 ms of device work --, `rounds` samples per method, the methods
alternating.  The route is timed alone (deferred counter read) and as called by default (with the 8-byte read, a host sync per
call).  Bundle variant: per-point incoming weights (n, k, k) with Wp far from I (every iteration of a loop looks like this);
transform variant: ONE shared prior matrix (the only transform input the route accepts: the first iteration).  Baseline "eig" is
asked for first through mia_lienks_update_f64 itself: where it answers MIA_ERR_UNSUPPORTED the case records that and times the
route alone.  Reported per case: median and spread (max - min over rounds), the ratios (median, and worst round of the baseline
against best round of the route), whether the case passes the hand-over rule (>= 2x beyond both spreads, counter read included),
the kernel names, the decline count, the degrees and the difference between the two kernels' results.  The tool stops at the
first case that fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["65,1,14,100000,bundle", "65,1,14,100000,transform", "80,1,16.5,100000,bundle", "80,4,20,100000,transform",
         "80,4,20,100000,bundle", "96,1,21,100000,bundle", "96,1,21,100000,transform", "128,1,25,50000,bundle",
         "128,1,25,50000,transform", "128,2,32,50000,bundle", "128,2,32,50000,transform",
         "64,1,15,100000,bundle,tile64", "64,1,15,100000,transform,tile64"]
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
    parts = spec.split(",")
    k, stride, c, G, variant = int(parts[0]), int(parts[1]), float(parts[2]), int(parts[3]), parts[4]
    baseline = parts[5] if len(parts) > 5 else "eig"
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
    res = {"case": dict(k=k, obs_stride=stride, radius=c, variant=variant, grid_points=G, p_max=int(nb.p_max), baseline=baseline,
                        weights_in="(n, k, k)" if bundle else "(k, k) shared prior", weights_bytes=G * k * k * 8)}
    W = torch.empty((G, k, k), dtype=torch.float64, device=dev)
    We = torch.empty((G, k, k), dtype=torch.float64, device=dev)

    def base():
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method=baseline, out=We)

    def wide():             # the kernel alone: the 8-byte read of the decline counter is left out
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="wide64", out=W, return_flags=True, defer_retry=True)

    def wide_sync():        # what a caller pays by default: kernel + counter read (a host sync per call)
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="wide64", out=W)

    def sample(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps
    fns = {"wide64_with_counter_read": wide_sync, "wide64": wide}
    if baseline == "eig":   # the general entry itself says whether it can hold the shape (before any launch)
        flags0 = torch.zeros(G, dtype=torch.int32, device=dev)
        rc = eng.lib.mia_lienks_update_f64(W_in.data_ptr(), k * k if bundle else 0, k, 0, G, rec.data_ptr(), rec.shape[0],
                                           nb.cnt.data_ptr(), nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, 1.0,
                                           eps or 0.0, We.data_ptr(), flags0.data_ptr(), None)
        torch.cuda.synchronize()
        res["mia_lienks_update_f64_status"] = int(rc)
        if rc == -3:
            baseline = None
        elif rc != 0:
            raise RuntimeError("mia_lienks_update_f64 failed with status %d" % rc)
    if baseline:
        fns = dict([(baseline, base)] + list(fns.items()))
    names = {}
    for n, fn in fns.items():                                  # warm-up (table, code objects, clocks); `wide` comes last
        for _ in range(2):
            r = fn()
        torch.cuda.synchronize()
        names[n] = _cabi.last_analysis_kernel()
    _, flags, finish = r
    res["declined"] = int(finish())
    torch.cuda.synchronize()
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    if baseline:
        res["rel_diff_%s_vs_wide64" % baseline] = float((torch.linalg.norm(We - W) / torch.linalg.norm(We)).item())
    # every timed sample holds at least `window_ms` of device work (measuring-on-mi355x: no short windows)
    reps = {n: max(2, int(-(-window_ms // max(sample(fn, 2), 1e-3)))) for n, fn in fns.items()}
    ts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ts[n].append(sample(fn, reps[n]))
    for n in fns:
        res[n] = dict(kernel=names[n], reps_per_sample=reps[n], **stats(ts[n]))
    if baseline:
        res["ratio_%s_over_wide64" % baseline] = res[baseline]["ms_median"] / res["wide64"]["ms_median"]
        # the figure the hand-over rule reads: what ienks_update pays (counter read included)
        res["ratio_%s_over_wide64_with_counter_read" % baseline] = res[baseline]["ms_median"] / res["wide64_with_counter_read"]["ms_median"]
        res["ratio_worst_case"] = res[baseline]["ms_min"] / res["wide64_with_counter_read"]["ms_max"]
        res["at_least_2x_beyond_both_spreads"] = bool(res["ratio_worst_case"] >= 2.0)
    res["GB_per_s_wide64"] = (2 if bundle else 1) * G * k * k * 8 / (res["wide64"]["ms_median"] * 1e-3) / 1e9
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
        print(json.dumps(one_case(a.case, a.rounds)))
        return 0
    results = []

    def document():
        return json.dumps({"tool": "tools/time_ienks_wide64.py", "build": a.label, "results": results}, indent=1)
    for spec in CASES:          # one fresh process per case, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            rc, so, se = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as exc:
            rc, so, se = 124, str(exc.stdout or ""), str(exc.stderr or "")
        if rc != 0:
            sys.stderr.write(so[-2000:] + se[-4000:])
            print(json.dumps({"tool": "tools/time_ienks_wide64.py", "failed_case": spec, "exit_status": rc, "results": results}))
            return 1
        results.append(json.loads(so.strip().splitlines()[-1]))
        print("%s: %s" % (spec, json.dumps({n: round(v["ms_median"], 3) for n, v in results[-1].items()
                                            if isinstance(v, dict) and "ms_median" in v})), file=sys.stderr, flush=True)
        if a.out:               # (kept current after every case: a later failure does not lose what was measured)
            with open(a.out, "w") as fh:
                fh.write(document() + "\n")
    print(document())
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Float64 IEnKS update time on DENSE local networks (p_max > k), tau = 1: the general kernel
(LetkfEngine.ienks_update(method="eig"): ienks_update_kernel<double, 256>, Gauss-Jordan and a Jacobi eigensolve from LDS, one
workgroup per grid point -- where it can hold the shape at all) against the dense tile kernel of csrc/lienks_stream64.hip
(method="stream64": lienks_stream64_kernel), and against the weights kernel it copies (weights_stream64 at inf = 1:
letkf_stream64w_kernel, the same passes less one product pair per tile and the read of W_in), alternating in ONE process.
Sibling of tools/time_ienks_wide64.py and tools/time_stream64w.py.

    python tools/time_ienks_stream64.py                               # every case below, one child process each (own time limit)
    python tools/time_ienks_stream64.py --case 80,93,bundle           # one case (k, p_max, variant)
    python tools/time_ienks_stream64.py --out profiles/ienks_stream64_time.json
    python tools/time_ienks_stream64.py --one-process --out ...       # every case in THIS process (the library's first use, over a
                                                                      # minute, is paid once; no time limit per case)

1-D geometry of bench.make_case with an observation at every grid point, 1e5 points (5e4 above 96 members), the radius found by
bisection so that an interior point sees p_max observations; seeded inputs, neighbour lists and packed records built once
outside the timed region; device events around `reps` calls per sample -- as many as make 120 ms of device work, at least one
--, `rounds` samples per method, the methods alternating.  The route is timed alone (deferred counter read) and as called by
default (with the 8-byte read, a host sync per call).  Bundle variant: per-point incoming weights (n, k, k) with Wp far from I
(every iteration of a loop looks like this); transform variant: ONE shared prior matrix (the only transform input the route
accepts: the first iteration).  The baseline is asked for first through mia_lienks_update_f64 itself: where it answers
MIA_ERR_UNSUPPORTED the case records that and times the route alone (absolute times only).  Reported per case: median and spread
(max - min over rounds), the ratios (median, and worst round of the baseline against best round of the route), whether the case
passes the hand-over rule (>= 2x beyond both spreads, counter read included), the ratio to the weights kernel, the kernel names,
the decline count, the degrees and the difference between the two kernels' results.  The tool stops at the first case that
fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["65,77,bundle", "65,77,transform", "72,77,bundle", "40,77,bundle", "40,77,transform", "80,93,bundle", "80,93,transform",
         "80,173,bundle", "96,107,bundle", "128,139,bundle", "128,139,transform", "128,203,bundle"]
EPS = 1e-3


def stats(v):
    import numpy as np
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), spread_ms=float(v.max() - v.min()),
                rounds=[float(x) for x in v])


def find_radius(eng, p_max):
    """The Gaspari-Cohn radius at which an interior point of a stride-1 network sees p_max observations (bisection on a short grid)."""
    import numpy as np
    x = np.arange(4 * p_max, dtype=np.float64)
    lo, hi = p_max / 8.0, float(p_max)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if eng.localize(x, x, [mid]).p_max >= p_max:
            hi = mid
        else:
            lo = mid
    return hi


def one_case(spec, rounds, window_ms=120.0):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    parts = spec.split(",")
    k, p_max, variant = int(parts[0]), int(parts[1]), parts[2]
    bundle = variant == "bundle"
    G = 50000 if k > 96 else 100000
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    c = find_radius(eng, p_max)
    _, gx, ox, Yb, d = bench.make_case(G, k, 1, dev, seed=42)
    Yb, d = Yb.double(), d.double()
    nb = eng.localize(gx, ox, [c])
    assert nb.p_max == p_max, (nb.p_max, p_max)
    eps = EPS if bundle else None
    rec = eng.pack_obs(Yb * EPS if bundle else Yb, d, torch.float64)
    rec_w = eng.pack_obs(Yb, d, torch.float64)               # the weights kernel's records: D itself
    gen = torch.Generator(device=dev).manual_seed(7)
    if bundle:
        A = torch.randn((G, k, k), dtype=torch.float64, device=dev, generator=gen)
        A -= A.mean(dim=2, keepdim=True)
        m = torch.randn((G, k, 1), dtype=torch.float64, device=dev, generator=gen)
        W_in = torch.eye(k, dtype=torch.float64, device=dev) + 0.3 / k ** 0.5 * A + 0.1 * m
        del A, m
    else:
        W_in = torch.eye(k, dtype=torch.float64, device=dev)
    res = {"case": dict(k=k, radius=c, variant=variant, grid_points=G, p_max=int(nb.p_max),
                        weights_in="(n, k, k)" if bundle else "(k, k) shared prior", weights_bytes=G * k * k * 8,
                        general_kernel_lds_bytes=eng._ienks_general_lds_bytes(k, p_max, 1.0, bundle))}
    W = torch.empty((G, k, k), dtype=torch.float64, device=dev)
    We = torch.empty((G, k, k), dtype=torch.float64, device=dev)

    def base():
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="eig", out=We)

    def weights():          # letkf_stream64w_kernel at inflation 1 with its counter read: the kernel this one copies
        r = eng.weights_stream64(Yb, None, nb, 1.0, rec=rec_w, out=We)
        assert r is not None, "weights_stream64 refused the shape"
        return r

    def stream():           # the kernel alone: the 8-byte read of the decline counter is left out
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="stream64", out=W, return_flags=True,
                                defer_retry=True)

    def stream_sync():      # what a caller pays by default: kernel + counter read (a host sync per call)
        return eng.ienks_update(W_in, None, None, nb, 1.0, eps, rec=rec, method="stream64", out=W)

    def sample(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps
    fns = {"weights_stream64_inf1": weights, "stream64_with_counter_read": stream_sync, "stream64": stream}
    # the general entry itself says whether it can hold the shape (before any launch)
    flags0 = torch.zeros(G, dtype=torch.int32, device=dev)
    rc = eng.lib.mia_lienks_update_f64(W_in.data_ptr(), k * k if bundle else 0, k, 0, G, rec.data_ptr(), rec.shape[0],
                                       nb.cnt.data_ptr(), nb.idx.data_ptr(), nb.w.data_ptr(), nb.p_cap, nb.p_max, 1.0,
                                       eps or 0.0, We.data_ptr(), flags0.data_ptr(), None)
    torch.cuda.synchronize()
    res["mia_lienks_update_f64_status"] = int(rc)
    if rc not in (0, -3):
        raise RuntimeError("mia_lienks_update_f64 failed with status %d" % rc)
    baseline = rc == 0
    assert baseline == eng._ienks_general_fits(k, p_max, 1.0, bundle)
    if baseline:
        fns = dict([("eig", base)] + list(fns.items()))
    names = {}
    for n, fn in fns.items():                                  # warm-up (table, code objects, clocks); `stream` comes last
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
        base()
        torch.cuda.synchronize()
        res["rel_diff_eig_vs_stream64"] = float((torch.linalg.norm(We - W) / torch.linalg.norm(We)).item())
    # every timed sample holds at least `window_ms` of device work (measuring-on-mi355x: no short windows)
    reps = {n: max(1, int(-(-window_ms // max(sample(fn, 1), 1e-3)))) for n, fn in fns.items()}
    ts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ts[n].append(sample(fn, reps[n]))
    for n in fns:
        res[n] = dict(kernel=names[n], reps_per_sample=reps[n], **stats(ts[n]))
    if baseline:
        res["ratio_eig_over_stream64"] = res["eig"]["ms_median"] / res["stream64"]["ms_median"]
        # the figure the hand-over rule reads: what ienks_update pays (counter read included)
        res["ratio_eig_over_stream64_with_counter_read"] = res["eig"]["ms_median"] / res["stream64_with_counter_read"]["ms_median"]
        res["ratio_worst_case"] = res["eig"]["ms_min"] / res["stream64_with_counter_read"]["ms_max"]
        res["at_least_2x_beyond_both_spreads"] = bool(res["ratio_worst_case"] >= 2.0)
    res["ratio_stream64_over_weights_stream64"] = (res["stream64_with_counter_read"]["ms_median"] /
                                                    res["weights_stream64_inf1"]["ms_median"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=280)
    ap.add_argument("--one-process", action="store_true")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds)))
        return 0
    results = []

    def document():
        return json.dumps({"tool": "tools/time_ienks_stream64.py", "build": a.label, "results": results}, indent=1)
    for spec in CASES:          # one fresh process per case, each under its own time limit; the first failure ends the run
        if a.one_process:
            import torch
            results.append(one_case(spec, a.rounds))
            torch.cuda.empty_cache()
            print("%s: %s" % (spec, json.dumps({n: round(v["ms_median"], 3) for n, v in results[-1].items()
                                                if isinstance(v, dict) and "ms_median" in v})), file=sys.stderr, flush=True)
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(document() + "\n")
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            rc, so, se = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as exc:
            rc, so, se = 124, str(exc.stdout or ""), str(exc.stderr or "")
        if rc != 0:
            sys.stderr.write(so[-2000:] + se[-4000:])
            print(json.dumps({"tool": "tools/time_ienks_stream64.py", "failed_case": spec, "exit_status": rc, "results": results}))
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

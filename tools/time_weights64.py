#!/usr/bin/env python3
"""Float64 weights time: the Jacobi kernel with W written (engine.analysis(..., return_weights=True): letkf_wave_kernel<double>,
what float64 weights ran on before the tile route existed) against LetkfEngine.weights64 (letkf_weights64_kernel), alternating
in ONE process -- and the two class calls that end there.

    python tools/time_weights64.py                      # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_weights64.py --case 40,2,10       # one case (k, obs stride, radius) in this process
    python tools/time_weights64.py --class-only --label parent   # the class calls alone: runs on a build without weights64 too
    python tools/time_weights64.py --out profiles/weights64_time.json --merge-parent parent.json

Config 2 geometry at 1e5 grid points, seeded inputs, neighbour lists and packed records built once outside the timed region;
device events around `reps` calls per sample -- as many as make 120 ms of device work --, `rounds` samples per method, the methods
alternating; weights64 is timed alone (deferred counter read) and as called by default (with the read).  Reported per case: median
and spread (max - min over rounds) of both, their ratio, the kernel name, the decline count, the mean degree, the
matrix-instruction count per tile and the time those instructions alone would take (`--mfma-cycles` per instruction and SIMD,
tools/mfma_rate_f64.hip); then LETKF(...).estimate_weights_arrays in float64 and analyse_arrays with a weight_save_path on
tmpfs (wall clock around a synchronised call: host work and the file are part of those).  The class-level baseline is a BUILD
OF THE PARENT COMMIT running this same file with --class-only; --merge-parent puts its figures beside this tree's."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["40,2,10", "20,2,5", "64,2,16"]
G = 100000


def mfma_model(k, p_max, deg_mean, cycles, n_tiles, clock_ghz=2.4, simds=1024):
    """set-up (Gram, bound) once per tile, then k passes of 4 UT^2 products per degree + mean weight + KT output blocks"""
    ut = min(4, max(1, (p_max + 8 + 15) // 16))
    kt = (k + 15) // 16
    per_pass = 4 * ut * ut * deg_mean + 4 * ut + kt * 4 * ut
    per_tile = 4 * kt * ut * ut + 4 * ut * ut + k * per_pass
    return dict(ut=ut, kt=kt, mfma_per_pass=per_pass, mfma_per_tile=per_tile, cycles_per_mfma=cycles,
                matrix_pipe_ms=per_tile * cycles * (n_tiles / simds) / (clock_ghz * 1e6))


def stats(v):
    import numpy as np
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), spread_ms=float(v.max() - v.min()),
                rounds=[float(x) for x in v])


def one_case(spec, rounds, cycles, class_only, window_ms=120.0):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    k, stride, c = spec.split(",")
    k, stride, c = int(k), int(stride), float(c)
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    X, gx, ox, Yb, d = bench.make_case(G, k, stride, dev, seed=42)
    X, Yb, d = X.double(), Yb.double(), d.double()
    nb = eng.localize(gx, ox, [c])
    res = {"case": dict(k=k, obs_stride=stride, radius=c, grid_points=G, p_max=int(nb.p_max), weights_bytes=G * k * k * 8)}
    if not class_only:
        rec = eng.pack_obs(Yb, d, torch.float64)
        out = torch.empty_like(X)

        W = torch.empty((G, k, k), dtype=torch.float64, device=dev)      # weights64 writes here: no allocation in its window

        def jacobi():           # (allocates its W inside the call: a cached block after the warm-up, no device allocation)
            return eng.analysis(X, None, None, nb, 1.1, rec=rec, out=out, return_weights=True)

        def tiles():            # the kernel alone: the 8-byte read of the decline counter is left out
            r = eng.weights64(Yb, None, nb, 1.1, rec=rec, out=W, return_flags=True, defer_retry=True)
            assert r is not None, "weights64 refused the shape"
            return r

        def tiles_sync():       # what a caller of weights64 pays by default: kernel + counter read (a host sync per call)
            return eng.weights64(Yb, None, nb, 1.1, rec=rec, out=W)

        def sample(fn, reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / reps
        for fn in (jacobi, tiles_sync, tiles):          # warm-up (table, code objects, clocks)
            for _ in range(2):
                r = fn()
            torch.cuda.synchronize()
        name = _cabi.last_analysis_kernel()
        _, flags, finish = r
        res["declined"] = int(finish())
        torch.cuda.synchronize()
        deg = ((flags >> 8) & 0xff).double()
        res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
        wj = jacobi()[1]
        torch.cuda.synchronize()
        res["rel_diff_jacobi_vs_weights64"] = float((torch.linalg.norm(wj - W) / torch.linalg.norm(wj)).item())
        del wj
        # every timed sample holds at least `window_ms` of device work (measuring-on-mi355x: no short windows)
        fns = {"jacobi": jacobi, "weights64": tiles, "weights64_with_counter_read": tiles_sync}
        reps = {n: max(2, int(-(-window_ms // max(sample(fn, 2), 1e-3)))) for n, fn in fns.items()}
        ts = {n: [] for n in fns}
        for _ in range(rounds):
            for n, fn in fns.items():
                ts[n].append(sample(fn, reps[n]))
        res["jacobi"] = dict(kernel="letkf_wave_kernel<double>", reps_per_sample=reps["jacobi"], **stats(ts["jacobi"]))
        for n in ("weights64", "weights64_with_counter_read"):
            res[n] = dict(kernel=name, reps_per_sample=reps[n], **stats(ts[n]))
        res["ratio_jacobi_over_weights64"] = res["jacobi"]["ms_median"] / res["weights64"]["ms_median"]
        # the figure the hand-over rule reads: what the class route pays (counter read included), worst round against best
        res["ratio_jacobi_over_weights64_with_counter_read"] = (res["jacobi"]["ms_median"] /
                                                                res["weights64_with_counter_read"]["ms_median"])
        res["ratio_worst_case"] = res["jacobi"]["ms_min"] / res["weights64_with_counter_read"]["ms_max"]
        res["faster_by_more_than_the_spread"] = bool(res["jacobi"]["ms_min"] - res["weights64"]["ms_max"] >
                                                     max(res["jacobi"]["spread_ms"], res["weights64"]["spread_ms"]))
        # the model: the per-tile degree is the largest of its sixteen points
        dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
        res["model"] = mfma_model(k, int(nb.p_max), dmax_tile, cycles, (G + 15) // 16)
        res["store_GB_per_s_weights64"] = G * k * k * 8 / (res["weights64"]["ms_median"] * 1e-3) / 1e9
        del W, r, out, rec
        # (letkf_wave.hip reports no kernel name: a float32 call makes the name the class calls leave behind a fresh one)
        c32 = bench.make_case(256, 20, 2, dev, seed=1)
        eng.analysis(c32[0], c32[3], c32[4], eng.localize(c32[1], c32[2], [5.0]), 1.1)
        torch.cuda.synchronize()
    # the class calls, float64 (the default dtype), wall clock around a synchronised call
    loc = mia.GaspariCohn(c, mia.AbsoluteDistance())
    gxh, oxh = gx.cpu().numpy(), ox.cpu().numpy()
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=shm) as tmp:
        f = mia.LETKF(localization=loc, inf_factor=1.1, engine=eng)
        fs = mia.LETKF(localization=loc, inf_factor=1.1, engine=eng, weight_save_path=os.path.join(tmp, "w.nc"))
        calls = {"estimate_weights_arrays": lambda: f.estimate_weights_arrays(Yb, d, grid_coords=gxh, obs_coords=oxh),
                 "analyse_arrays_weight_save_path": lambda: fs.analyse_arrays(X, Yb, d, grid_coords=gxh, obs_coords=oxh)}
        cls = {}
        for what, fn in calls.items():
            try:
                fn()
            except (OSError, OverflowError) as exc:      # (a tmpfs smaller than the file; a variable beyond netCDF-3's 2 GiB,
                                                         #  k = 64: 3.3 GB -- recorded, not fatal)
                cls[what] = dict(error=repr(exc))
                continue
            torch.cuda.synchronize()
            kern = _cabi.last_analysis_kernel()
            v = []
            for _ in range(max(3, rounds)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                v.append((time.perf_counter() - t0) * 1e3)
            cls[what] = dict(last_reported_kernel=kern, **stats(v))
        res["class_calls_float64"] = cls
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mfma-cycles", type=float, default=64.0)
    ap.add_argument("--class-only", action="store_true")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--merge-parent", help="JSON written by a --class-only run on a build of the parent commit")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=280)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, a.mfma_cycles, a.class_only)))
        return 0
    results = []
    for spec in CASES:          # one fresh process per case, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds), "--mfma-cycles", str(a.mfma_cycles)]
        r = subprocess.run(cmd + (["--class-only"] if a.class_only else []), capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("%s: %s" % (spec, json.dumps({n: round(v["ms_median"], 3) for n, v in results[-1].items()
                                            if isinstance(v, dict) and "ms_median" in v})), file=sys.stderr, flush=True)
    doc = {"tool": "tools/time_weights64.py", "build": a.label, "grid_points": G, "results": results}
    if a.merge_parent:
        with open(a.merge_parent) as fh:
            par = json.load(fh)
        doc["parent_build"] = dict(build=par.get("build"), note="the same tool with --class-only on a build of the parent commit",
                                   results=[dict(case=r["case"], class_calls_float64=r["class_calls_float64"]) for r in par["results"]])
        for mine, theirs in zip(results, par["results"]):
            mine["class_ratio_parent_over_this"] = {n: theirs["class_calls_float64"][n]["ms_median"] / v["ms_median"]
                                                    for n, v in mine["class_calls_float64"].items()
                                                    if "ms_median" in v and "ms_median" in theirs["class_calls_float64"].get(n, {})}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Float64 ensemble transform time: the round-1 kernels (apply_local_weights_kernel<double>, one wavefront per grid point;
apply_weights_kernel<double, ...>, one thread per grid point) against the tile kernels of csrc/apply_local64.hip, alternating in
ONE process -- and the two class calls that end in the per-point transform.

    python tools/time_apply64.py                          # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_apply64.py --case local,40,16       # one case (kind, k, m) in this process
    python tools/time_apply64.py --class-only --label parent     # the class calls alone: runs on a build without the tile kernels too
    python tools/time_apply64.py --kernels-only                  # the kernel cases alone
    python tools/time_apply64.py --out profiles/apply64_time.json --merge-parent parent.json

The baseline is the fallback selected with the option apply64 = 0, the tile kernel is selected with apply64 = 1.  THE FALLBACK IS THE
PARENT COMMIT'S KERNEL, BYTE FOR BYTE: the kernels apply_local_weights_kernel (csrc/ienks.hip) and apply_weights_kernel
(csrc/etkf_global.hip) and their launch functions were not edited when the tile kernels were added; the entries only try the tile
launch first.  Both run in one process and alternate, so clocks and memory state are shared.

Seeded inputs made on the device (W ~ N(0, 1 / k), x ~ N(0, 1), row 0 shifted by 300), 1e5 grid points at every size (k = 128 with
64 rows: 13 GB of weights and 2 x 6.6 GB of state, well inside the device's memory); device events around `reps` calls per sample --
as many as make 120 ms of device work --, `rounds` samples per kernel, the kernels alternating.  Reported per case: median and spread
(max - min over rounds) of both, their ratio, the kernel names, the relative difference of the two outputs, the hand-over test
(the tile kernel's slowest round beats the fallback's fastest by more than the larger spread), and the compulsory bytes -- 8 k^2
per point once + 16 k m per point for the per-point transform, 16 k m for the global one -- over the tile kernel's time as a
fraction of 8 TB/s.  Class level (wall clock around a synchronised call, host work and the file included): float64
analyse_arrays with a weight_save_path on tmpfs at config 2 (k = 40, every second point observed, radius 10, 1e5 points) and one
LocalizedIEnKSTransform.apply_weights_arrays at k = 40 with 16 state rows.  The class-level baseline is a BUILD OF THE PARENT COMMIT
running this same file with --class-only; --merge-parent puts its figures beside this tree's."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 100000
CASES = (["local,%d,%d" % (k, m) for k in (20, 40, 64, 80, 128) for m in (1, 8, 16, 64)] +
         ["global,%d,%d" % (k, m) for k in (40, 128) for m in (1, 16, 64)] + ["class,40,16"])
HBM_BYTES_PER_S = 8e12


def stats(v):
    import numpy as np
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), spread_ms=float(v.max() - v.min()),
                rounds=[float(x) for x in v])


def kernel_case(kind, k, m, rounds, window_ms=120.0):
    import torch
    sys.path.insert(0, ROOT)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * k + m)
    X = torch.randn((m, k, G), generator=gen, device=dev, dtype=torch.float64)
    X[0] += 300.0
    wshape = (G, k, k) if kind == "local" else (k, k)
    W = torch.randn(wshape, generator=gen, device=dev, dtype=torch.float64) / k ** 0.5
    call = eng.apply_local_weights if kind == "local" else eng.apply_weights
    res = {"case": dict(kind=kind, k=k, m=m, grid_points=G)}

    def run(opt):
        _cabi.set_option("apply64", opt)
        return call(X, W)

    def sample(opt, reps):
        _cabi.set_option("apply64", opt)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call(X, W)          # (the output is a cached block after the warm-up: no device allocation in the window)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps
    try:
        outs, names = {}, {}
        for n, opt in (("fallback", 0), ("tile", 1)):          # warm-up (code objects, clocks), names, outputs
            for _ in range(2):
                outs[n] = run(opt)
            torch.cuda.synchronize()
            names[n] = _cabi.last_transform_kernel()
        assert "64_tile_kernel" in names["tile"] and "64_tile_kernel" not in names["fallback"], names
        res["rel_diff_fallback_vs_tile"] = float((torch.linalg.norm(outs["fallback"] - outs["tile"]) /
                                                  torch.linalg.norm(outs["fallback"])).item())
        del outs
        reps = {n: max(2, int(-(-window_ms // max(sample(opt, 2), 1e-3)))) for n, opt in (("fallback", 0), ("tile", 1))}
        ts = {"fallback": [], "tile": []}
        for _ in range(rounds):
            for n, opt in (("fallback", 0), ("tile", 1)):
                ts[n].append(sample(opt, reps[n]))
    finally:
        _cabi.set_option("apply64", -1)
    for n in ("fallback", "tile"):
        res[n] = dict(kernel=names[n], reps_per_sample=reps[n], **stats(ts[n]))
    res["ratio_fallback_over_tile"] = res["fallback"]["ms_median"] / res["tile"]["ms_median"]
    res["faster_by_more_than_the_spread"] = bool(res["fallback"]["ms_min"] - res["tile"]["ms_max"] >
                                                 max(res["fallback"]["spread_ms"], res["tile"]["spread_ms"]))
    nbytes = G * ((8 * k * k if kind == "local" else 0) + 16 * k * m)
    res["compulsory_bytes"] = nbytes
    res["tile_fraction_of_8TBps"] = nbytes / (res["tile"]["ms_median"] * 1e-3) / HBM_BYTES_PER_S
    res["fallback_fraction_of_8TBps"] = nbytes / (res["fallback"]["ms_median"] * 1e-3) / HBM_BYTES_PER_S
    return res


def class_case(k, m, rounds):
    """the two class calls in float64 under the default options of the build that runs this file"""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    last = getattr(_cabi, "last_transform_kernel", lambda: "(a build without mia_last_transform_kernel)")
    X, gx, ox, Yb, d = bench.make_case(G, k, 2, dev, seed=42)
    X, Yb, d = X.double(), Yb.double(), d.double()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    Xm = torch.randn((m, k, G), generator=gen, device=dev, dtype=torch.float64)
    Wm = torch.randn((G, k, k), generator=gen, device=dev, dtype=torch.float64) / k ** 0.5
    loc = mia.GaspariCohn(10.0, mia.AbsoluteDistance())
    gxh, oxh = gx.cpu().numpy(), ox.cpu().numpy()
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    cls = {}
    with tempfile.TemporaryDirectory(dir=shm) as tmp:
        fs = mia.LETKF(localization=loc, inf_factor=1.1, engine=eng, weight_save_path=os.path.join(tmp, "w.nc"))
        ie = mia.LocalizedIEnKSTransform(None, loc, tau=1.0, dtype=torch.float64, engine=eng)
        calls = {"analyse_arrays_weight_save_path_config2": lambda: fs.analyse_arrays(X, Yb, d, grid_coords=gxh, obs_coords=oxh),
                 "lienks_apply_weights_arrays_k%d_m%d" % (k, m): lambda: ie.apply_weights_arrays(Xm, Wm)}
        for what, fn in calls.items():
            try:
                fn()
            except (OSError, OverflowError) as exc:      # (a tmpfs smaller than the file: recorded, not fatal)
                cls[what] = dict(error=repr(exc))
                continue
            torch.cuda.synchronize()
            kern = last()
            v = []
            for _ in range(max(3, rounds)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                v.append((time.perf_counter() - t0) * 1e3)
            cls[what] = dict(transform_kernel=kern, **stats(v))
    return {"case": dict(kind="class", k=k, m=m, grid_points=G), "class_calls_float64": cls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--class-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="leave the class calls out (the kernel cases decide the default they run under)")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--merge-parent", help="JSON written by a --class-only run on a build of the parent commit")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.case:
        kind, k, m = a.case.split(",")
        res = class_case(int(k), int(m), a.rounds) if kind == "class" else kernel_case(kind, int(k), int(m), a.rounds)
        print(json.dumps(res))
        return 0
    results = []
    for spec in CASES:          # one fresh process per case, each under its own time limit; the first failure ends the run
        if (a.class_only and not spec.startswith("class")) or (a.kernels_only and spec.startswith("class")):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"failed_case": spec, "exit_status": "time limit", "results": results}))
            return 1
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        last = results[-1]
        brief = ({n: round(last[n]["ms_median"], 4) for n in ("fallback", "tile")} if "tile" in last else
                 {n: round(v.get("ms_median", -1.0), 2) for n, v in last["class_calls_float64"].items()})
        print("%s: %s %s" % (spec, json.dumps(brief), last.get("faster_by_more_than_the_spread", "")), file=sys.stderr, flush=True)
    doc = {"tool": "tools/time_apply64.py", "build": a.label, "grid_points": G, "results": results}
    if a.merge_parent:
        with open(a.merge_parent) as fh:
            par = json.load(fh)
        doc["parent_build"] = dict(build=par.get("build"), note="the same tool with --class-only on a build of the parent commit",
                                   results=par["results"])
        mine = [r for r in results if "class_calls_float64" in r]
        for me, theirs in zip(mine, par["results"]):
            me["class_ratio_parent_over_this"] = {n: theirs["class_calls_float64"][n]["ms_median"] / v["ms_median"]
                                                  for n, v in me["class_calls_float64"].items()
                                                  if "ms_median" in v and "ms_median" in theirs["class_calls_float64"].get(n, {})}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

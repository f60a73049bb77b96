#!/usr/bin/env python3
"""Float64 analysis time: the Jacobi kernel (method="eig": letkf_wave_kernel<double>, what float64 ran on before the tile
route existed) against the float64 tile route (method="auto": letkf_tile64_kernel), alternating in ONE process.

    python tools/time_f64.py                      # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_f64.py --case 40,2,10,1     # one case (k, obs stride, radius, state rows) in this process
    python tools/time_f64.py --out profiles/tile64_time.json --mfma-cycles 32

Config 2 geometry at 1e5 grid points, seeded inputs, neighbour lists and packed records built once outside the timed region;
the analysis call alone is timed with device events, `reps` calls per sample, `rounds` samples per method, the methods
alternating.  Reported per case: median and spread (max - min over rounds) of both, their ratio, the decline count, the tile
kernel's matrix-instruction count per tile and the time those instructions alone would take (`--mfma-cycles` per instruction and
SIMD, tools/mfma_rate_f64.hip), and the whole LETKF(...).analyse_arrays call in float64 with the route on and off (tile = 1 / 0)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["40,2,10,1", "20,2,5,1", "64,2,16,1", "40,2,10,8", "40,2,10,32"]
G = 100000


def mfma_model(k, p_max, m, deg_mean, cycles, n_tiles, clock_ghz=2.4, simds=1024):
    ut = min(4, max(1, (p_max + 8 + 15) // 16))
    kt = (k + 15) // 16
    per_tile = 4 * kt * ut * ut + 4 * ut * ut + m * (4 * kt * ut + 4 * ut * ut * deg_mean + 4 * ut + 4 * kt * ut)
    return dict(ut=ut, kt=kt, mfma_per_tile=per_tile, cycles_per_mfma=cycles,
                matrix_pipe_ms=per_tile * cycles * (n_tiles / simds) / (clock_ghz * 1e6))


def one_case(spec, rounds, cycles):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    k, stride, c, m = spec.split(",")
    k, stride, c, m = int(k), int(stride), float(c), int(m)
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    X, gx, ox, Yb, d = bench.make_case(G, k, stride, dev, seed=42)
    X = X.double()
    if m > 1:
        X = (X.repeat(m, 1, 1) * torch.linspace(0.5, 2.0, m, device=dev, dtype=torch.float64)[:, None, None]).contiguous()
    nb = eng.localize(gx, ox, [c])
    rec = eng.pack_obs(Yb.double(), d.double(), torch.float64)
    out = torch.empty_like(X)
    flags = torch.empty(G, dtype=torch.int32, device=dev)
    retry = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(method):
        return eng.analysis(X, None, None, nb, 1.1, rec=rec, method=method, out=out, flags=flags, retry=retry, defer_retry=True)

    def sample(method, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call(method)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    res = {"case": dict(k=k, obs_stride=stride, radius=c, state_rows=m, grid_points=G, p_max=int(nb.p_max))}
    names = {}
    for method in ("eig", "auto"):          # warm-up (table, code objects, clocks)
        retry.zero_()
        for _ in range(2):
            call(method)
        torch.cuda.synchronize()
        names[method] = _cabi.last_analysis_kernel() if method == "auto" else "letkf_wave_kernel<double>"
    res["declined"] = int(retry.item())
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    ts = {"eig": [], "auto": []}
    for _ in range(rounds):
        ts["eig"].append(sample("eig", 2))
        ts["auto"].append(sample("auto", 10))
    for method in ts:
        v = np.array(ts[method])
        res[method] = dict(kernel=names[method], ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                           spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v])
    res["ratio_eig_over_auto"] = res["eig"]["ms_median"] / res["auto"]["ms_median"]
    res["analyses_per_s_auto"] = G / (res["auto"]["ms_median"] * 1e-3)
    res["faster_by_more_than_the_spread"] = bool(res["eig"]["ms_min"] - res["auto"]["ms_max"] >
                                                 max(res["eig"]["spread_ms"], res["auto"]["spread_ms"]))
    # the model: the per-tile degree is the largest of its sixteen points
    dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
    res["model"] = mfma_model(k, int(nb.p_max), m, dmax_tile, cycles, (G + 15) // 16)
    if m == 1:
        # the whole class call, float64, with the route on and off
        loc = mia.GaspariCohn(c, mia.AbsoluteDistance())
        gxh, oxh = gx.cpu().numpy(), ox.cpu().numpy()
        Ybd, dd = Yb.double(), d.double()
        whole = {}
        for tile in (1, 0):
            old = _cabi.set_option("tile", tile)
            try:
                f = mia.LETKF(localization=loc, inf_factor=1.1, engine=eng)
                f.analyse_arrays(X, Ybd, dd, grid_coords=gxh, obs_coords=oxh)
                torch.cuda.synchronize()
                v = []
                for _ in range(3):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f.analyse_arrays(X, Ybd, dd, grid_coords=gxh, obs_coords=oxh)
                    b.record()
                    b.synchronize()
                    v.append(a.elapsed_time(b))
                whole["tile=%d" % tile] = dict(ms_median=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v)))
            finally:
                _cabi.set_option("tile", old)
        res["analyse_arrays_float64_ms"] = whole
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mfma-cycles", type=float, default=64.0)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, a.mfma_cycles)))
        return 0
    results = []
    for spec in CASES:          # one fresh process per case, each under its own time limit; the first failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds),
                            "--mfma-cycles", str(a.mfma_cycles)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("%s: eig %.3f ms, auto %.3f ms, ratio %.1f, declined %d" % (spec, results[-1]["eig"]["ms_median"],
              results[-1]["auto"]["ms_median"], results[-1]["ratio_eig_over_auto"], results[-1]["declined"]), file=sys.stderr, flush=True)
    doc = {"tool": "tools/time_f64.py", "grid_points": G, "results": results}
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

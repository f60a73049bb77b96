#!/usr/bin/env python3
"""Float64 weights time for ensembles above 64 members (p_max <= k): the Jacobi kernel with W written
(engine.analysis(..., return_weights=True): letkf_wave_kernel<double>, what these weights ran on before the route existed, where
it can hold the shape at all) against LetkfEngine.weights_wide64 (letkf_wide64w_kernel), alternating in ONE process.  Sibling of
tools/time_wide64.py (the analysis of these ensembles) and tools/time_weights64.py (the weights for k <= 64).

    python tools/time_wide64w.py                          # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_wide64w.py --case 80,1,16.5,100000  # one case (k, obs stride, radius, grid points[, baseline]) in this process
    python tools/time_wide64w.py --case 64,1,15,100000,weights64   # ... against letkf_weights64_kernel: what the barriers cost
    python tools/time_wide64w.py --out profiles/wide64w_time.json

Seeded inputs, neighbour lists and packed records built once outside the timed region; device events around `reps` calls per
sample -- as many as make 120 ms of device work --, `rounds` samples per method, the methods alternating; weights_wide64 is timed
alone (deferred counter read) and as called by default (with the 8-byte read: what the classes pay and what the hand-over rule
reads).  W is 13 GB at k = 128 and 1e5 points: those cases run on fewer points, written into the case.  Reported per case: median
and spread (max - min over rounds) of each method, the ratios, the decline count, the degrees, the busiest wavefront's
matrix-instruction count per tile (from the lists of the first 64 tiles, split into the parts the kernel analyses them in, and
the measured degrees) and the time those instructions alone would take at `--mfma-cycles` per instruction and SIMD
(tools/mfma_rate_f64.hip) with the workgroups that are RESIDENT at the launch's LDS size.  A baseline that answers
MIA_ERR_UNSUPPORTED (the Jacobi kernel beyond about 70 local observations) is recorded as such with its message."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (k, obs stride, radius, grid points[, baseline]); 96,1,21 and 128,1,25 have p_max 81 / 97: no Jacobi baseline exists
CASES = ["80,1,16.5,100000", "65,1,14,100000", "128,2,32,50000", "96,1,21,100000", "128,1,25,50000", "64,1,15,100000,weights64"]


def launch_shape(k, p_max):
    """Restates wide64w_ut / wide64w_nw / wide64w_lds_bytes (csrc/letkf_wide64w.hip)."""
    ut = min(max((p_max + 8 + 15) >> 4, 1), 8)
    kt = (k + 15) >> 4
    nw = 2 if ut <= 6 else 4
    lds = -(-((16 * ut * (16 * kt + 5) + 16 * (16 * ut + 1) + 16 * nw) * 8 + (16 * ut + nw) * 4) // 16) * 16
    return ut, kt, nw, lds


def tile_parts(lists, umax):
    """Number of parts a tile of sixteen lists is analysed in: halved, as the kernel does, until the union fits."""
    parts, lo = 0, 0
    while lo < len(lists):
        n = 16
        while len(set().union(*lists[lo:lo + n])) > umax and n > 1:
            n >>= 1
        parts += 1
        lo += n
    return parts


def mfma_model(k, p_max, tiles, deg_tile, cycles, n_tiles, clock_ghz=2.4, cus=256, lds_per_cu=160 * 1024):
    """The busiest wavefront of a workgroup owns TW = ceil(UT / NW) row blocks; every step is unconditional, so a part of a tile
    costs it 4 KT UT TW (Gram) + 4 UT TW (bound) and per MEMBER degree x 4 UT TW (recurrence) + 4 UT (mean weight) +
    ceil(KT / NW) 4 UT (output) matrix instructions.  Each wave has a matrix pipe of its own (one wave per SIMD); a compute
    unit holds min(4 / NW, LDS per CU / LDS per workgroup) workgroups: the pipe-only time is the busiest wave's instructions of
    all tiles over the resident workgroups."""
    ut, kt, nw, lds = launch_shape(k, p_max)
    tw = -(-ut // nw)
    wg_per_cu = max(1, min(4 // nw, lds_per_cu // lds))
    nparts = [tile_parts(lists, 16 * ut) for lists in tiles]
    per_pass = deg_tile * 4 * ut * tw + 4 * ut + -(-kt // nw) * 4 * ut
    per_part = 4 * kt * ut * tw + 4 * ut * tw + k * per_pass
    mean = per_part * sum(nparts) / len(nparts)
    return dict(ut=ut, kt=kt, nw=nw, row_blocks_busiest_wave=tw, lds_bytes=lds, workgroups_per_cu=wg_per_cu,
                waves_per_simd=wg_per_cu * nw / 4.0, parts_per_tile_mean=sum(nparts) / len(nparts),
                mfma_per_pass_busiest_wave=per_pass, mfma_per_tile_busiest_wave=mean,
                barriers_per_tile=k * (2 * (deg_tile + 1) + 5), cycles_per_mfma=cycles,
                matrix_pipe_ms=mean * cycles * (n_tiles / (cus * wg_per_cu)) / (clock_ghz * 1e6))


def stats(v):
    import numpy as np
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), spread_ms=float(v.max() - v.min()),
                rounds=[float(x) for x in v])


def one_case(spec, rounds, cycles, window_ms=120.0):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    f = spec.split(",")
    k, stride, c, G = int(f[0]), int(f[1]), float(f[2]), int(f[3])
    base = f[4] if len(f) > 4 else "jacobi"
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    X, gx, ox, Yb, d = bench.make_case(G, k, stride, dev, seed=42)
    X, Yb, d = X.double(), Yb.double(), d.double()
    nb = eng.localize(gx, ox, [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
    res = {"case": dict(k=k, obs_stride=stride, radius=c, grid_points=G, p_max=int(nb.p_max), weights_bytes=G * k * k * 8),
           "baseline": base}
    W = torch.empty((G, k, k), dtype=torch.float64, device=dev)      # weights_wide64 writes here: no allocation in its window
    out = torch.empty_like(X)

    def jacobi():           # (allocates its W inside the call: a cached block after the warm-up, no device allocation)
        return eng.analysis(X, None, None, nb, 1.1, rec=rec, out=out, return_weights=True)[1]

    Wb = torch.empty((G, k, k), dtype=torch.float64, device=dev) if base == "weights64" else None

    def weights64():        # the one-wavefront kernel as the classes call it for k <= 64 (counter read included)
        r = eng.weights64(Yb, None, nb, 1.1, rec=rec, out=Wb)
        assert r is not None, "weights64 refused the shape"
        return r

    def wide():             # the kernel alone: the 8-byte read of the decline counter is left out
        r = eng.weights_wide64(Yb, None, nb, 1.1, rec=rec, out=W, return_flags=True, defer_retry=True)
        assert r is not None, "weights_wide64 refused the shape"
        return r

    def wide_sync():        # what a caller pays by default: kernel + counter read (a host sync per call)
        return eng.weights_wide64(Yb, None, nb, 1.1, rec=rec, out=W)

    def sample(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    base_fn = {"jacobi": jacobi, "weights64": weights64}[base]
    try:        # the Jacobi kernel holds a point's matrices in LDS and answers MIA_ERR_UNSUPPORTED beyond ~70 local observations
        wref = base_fn()
        torch.cuda.synchronize()
        base_name = "letkf_wave_kernel<double>" if base == "jacobi" else _cabi.last_analysis_kernel()
    except _cabi.MiaError as err:
        res["baseline_unsupported"] = str(err)
        base_fn, wref = None, None
    for fn in (wide_sync, wide):                     # warm-up (table, code objects, clocks)
        for _ in range(2):
            r = fn()
        torch.cuda.synchronize()
    name = _cabi.last_analysis_kernel()
    _, flags, finish = r
    res["declined"] = int(finish())
    torch.cuda.synchronize()
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    if wref is not None:
        res["rel_diff_baseline_vs_weights_wide64"] = float((torch.linalg.norm(wref - W) / torch.linalg.norm(wref)).item())
    del wref
    fns = {"weights_wide64": wide, "weights_wide64_with_counter_read": wide_sync}
    if base_fn is not None:
        base_fn()
        torch.cuda.synchronize()
        fns = dict([("baseline_time", base_fn)] + list(fns.items()))
    # every timed sample holds at least `window_ms` of device work (measuring-on-mi355x: no short windows)
    reps = {n: max(2, int(-(-window_ms // max(sample(fn, 2), 1e-3)))) for n, fn in fns.items()}
    ts = {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            ts[n].append(sample(fn, reps[n]))
    for n in fns:
        res[n] = dict(kernel=base_name if n == "baseline_time" else name, reps_per_sample=reps[n], **stats(ts[n]))
    if base_fn is not None:
        res["ratio_baseline_over_weights_wide64"] = res["baseline_time"]["ms_median"] / res["weights_wide64"]["ms_median"]
        # the figure the hand-over rule reads: what the class route pays (counter read included)
        res["ratio_baseline_over_weights_wide64_with_counter_read"] = (res["baseline_time"]["ms_median"] /
                                                                       res["weights_wide64_with_counter_read"]["ms_median"])
        # "at least 2x beyond both spreads": the slowest sample with the read against the fastest baseline sample
        res["ratio_worst_case"] = res["baseline_time"]["ms_min"] / res["weights_wide64_with_counter_read"]["ms_max"]
        res["twice_as_fast_beyond_both_spreads"] = bool(res["ratio_worst_case"] >= 2.0)
    res["store_GB_per_s_weights_wide64"] = G * k * k * 8 / (res["weights_wide64"]["ms_median"] * 1e-3) / 1e9
    res["ms_per_1e5_points_weights_wide64"] = res["weights_wide64"]["ms_median"] * 1e5 / G
    nt = min(1024, G // 16 * 16)
    cnt, idx = nb.cnt[:nt].cpu().numpy(), nb.idx[:nt].cpu().numpy()
    tiles = [[set(idx[g, :cnt[g]].tolist()) for g in range(t, t + 16)] for t in range(0, nt, 16)]
    unions = [len(set().union(*t)) for t in tiles]
    res["union_mean"], res["union_max"] = float(np.mean(unions)), int(max(unions))
    dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
    res["model"] = mfma_model(k, int(nb.p_max), tiles, dmax_tile, cycles, (G + 15) // 16)
    res["time_over_matrix_pipe_time"] = res["weights_wide64"]["ms_median"] / res["model"]["matrix_pipe_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--cases", help="semicolon-separated cases in the place of the built-in list")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mfma-cycles", type=float, default=64.0)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, a.mfma_cycles)))
        return 0
    results = []

    def dump():
        return json.dumps({"tool": "tools/time_wide64w.py", "results": results}, indent=1)
    cases = a.cases.split(";") if a.cases else CASES
    for spec in cases:      # one fresh process per case, each under its own time limit; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds),
                                "--mfma-cycles", str(a.mfma_cycles)], capture_output=True, text=True, timeout=a.timeout)
            status, tail = r.returncode, r.stdout[-2000:] + r.stderr[-4000:]
        except subprocess.TimeoutExpired as err:       # (the child is killed; reported like any other failed case)
            status, tail = "timeout after %d s" % a.timeout, str(err.stderr or "")[-4000:]
        if status != 0:
            sys.stderr.write(tail)
            failed = {"tool": "tools/time_wide64w.py", "failed_case": spec, "exit_status": status, "results": results}
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(json.dumps(failed, indent=1) + "\n")
            print(json.dumps(failed))
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(res)
        first = res.get("baseline_time")
        print("%s: %s %s ms, weights_wide64 %.3f ms (with counter read %.3f), declined %s"
              % (spec, res["baseline"], first and "%.3f" % first["ms_median"], res["weights_wide64"]["ms_median"],
                 res["weights_wide64_with_counter_read"]["ms_median"], res.get("declined")), file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(dump() + "\n")
    print(dump())
    return 0


if __name__ == "__main__":
    sys.exit(main())

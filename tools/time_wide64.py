#!/usr/bin/env python3
"""Float64 analysis time for ensembles above 64 members (p_max <= k): the Jacobi kernel (method="eig": letkf_wave_kernel<double>,
what these shapes ran on before the wide tile route existed) against the wide float64 tile route (method="wide64":
letkf_wide64_kernel), alternating in ONE process.  Sibling of tools/time_dense64.py (p_max > k) and tools/time_f64.py (k <= 64).

    python tools/time_wide64.py                      # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_wide64.py --case 80,1,16.5,1   # one case (k, obs stride, radius, state rows) in this process
    python tools/time_wide64.py --case 64,1,15,1,matfun64    # ... against letkf_tile64_kernel instead: what the barriers cost
    python tools/time_wide64.py --out profiles/wide64_time.json --parent parent.json

1e5 grid points, seeded inputs, neighbour lists and packed records built once outside the timed region; the analysis call alone
is timed with device events, `reps` calls per sample, `rounds` samples per method, the methods alternating.  Reported per case:
median and min-max of both, their ratio, the decline count, the busiest wavefront's matrix-instruction count per tile (from the
lists of the first 64 tiles, split into the parts the kernel analyses them in, and the measured degrees) and the time those
instructions alone would take at `--mfma-cycles` per instruction and SIMD (tools/mfma_rate_f64.hip) with the workgroups that are
RESIDENT at the launch's LDS size, and for the first case the whole LETKF(...).analyse_arrays call in float64.

On a build WITHOUT the route (the parent commit of an A/B run) "auto" is timed in the place of "wide64" -- both are then the
Jacobi kernel -- and `--parent FILE` merges such a run's figures into this one's as `eig_parent_build` / `analyse_arrays_parent`."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the last two against letkf_tile64_kernel: unions of 72 slots, which that kernel runs in two parts, and unions that fit its 64)
CASES = ["80,1,16.5,1", "96,1,21,1", "128,1,25,1", "128,2,32,1", "80,1,16.5,8", "64,1,15,1,matfun64", "64,2,28,1,matfun64"]


def launch_shape(k, p_max):
    """Restates wide64_ut / wide64_nw / wide64_lds_bytes (csrc/letkf_wide64.hip)."""
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


def mfma_model(k, p_max, tiles, m, deg_tile, cycles, n_tiles, clock_ghz=2.4, cus=256, lds_per_cu=160 * 1024):
    """The busiest wavefront of a workgroup owns TW = ceil(UT / NW) row blocks; every step is unconditional, so a part of a tile
    costs it 4 KT UT TW (Gram) + 4 UT TW (bound) and per state row 4 KT TW (Z) + degree x 4 UT TW (recurrence) + 4 UT (x' w) +
    ceil(KT / NW) 4 UT (output) matrix instructions.  Each wave has a matrix pipe of its own (one wave per SIMD); a compute
    unit holds min(4 / NW, LDS per CU / LDS per workgroup) workgroups: the pipe-only time is the busiest wave's instructions of
    all tiles over the resident workgroups."""
    ut, kt, nw, lds = launch_shape(k, p_max)
    tw = -(-ut // nw)
    wg_per_cu = max(1, min(4 // nw, lds_per_cu // lds))
    nparts = [tile_parts(lists, 16 * ut) for lists in tiles]
    per_part = 4 * kt * ut * tw + 4 * ut * tw + m * (4 * kt * tw + deg_tile * 4 * ut * tw + 4 * ut + -(-kt // nw) * 4 * ut)
    mean = per_part * sum(nparts) / len(nparts)
    return dict(ut=ut, kt=kt, nw=nw, row_blocks_busiest_wave=tw, lds_bytes=lds, workgroups_per_cu=wg_per_cu,
                waves_per_simd=wg_per_cu * nw / 4.0, parts_per_tile_mean=sum(nparts) / len(nparts),
                mfma_per_tile_busiest_wave=mean, barriers_per_tile=m * (2 * (deg_tile + 1) + 5), cycles_per_mfma=cycles,
                matrix_pipe_ms=mean * cycles * (n_tiles / (cus * wg_per_cu)) / (clock_ghz * 1e6))


def one_case(spec, rounds, cycles, whole):
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
    k, stride, c, m = int(f[0]), int(f[1]), float(f[2]), int(f[3])
    base = f[4] if len(f) > 4 else "eig"
    X, gx, ox, Yb, d = bench.make_case(100000, k, stride, dev, seed=42)
    X, Yb, d = X.double(), Yb.double(), d.double()
    G = X.shape[-1]
    if m > 1:
        X = (X.repeat(m, 1, 1) * torch.linspace(0.5, 2.0, m, device=dev, dtype=torch.float64)[:, None, None]).contiguous()
    nb = eng.localize(gx, ox, [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
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

    # a library without the wide route (the parent build of an A/B run) times "auto" in its place
    have = "mia_letkf_analysis_wide_f64" in _cabi.EXPORTED_SYMBOLS
    alt = "wide64" if have else "auto"
    res = {"case": dict(k=k, obs_stride=stride, radius=c, state_rows=m, grid_points=G, p_max=int(nb.p_max)), "baseline": base,
           "second_method": alt}
    names = {}
    try:        # the Jacobi kernel holds a point's matrices in LDS and answers MIA_ERR_UNSUPPORTED beyond ~70 local observations
        call(base)
        torch.cuda.synchronize()
    except _cabi.MiaError as err:
        res["baseline_unsupported"] = str(err)
        base = None
    for method in (base, alt):           # warm-up (table, code objects, clocks)
        if method is None or (method == alt and not have and base is None):
            continue
        retry.zero_()
        call(method)
        torch.cuda.synchronize()
        # (letkf_wave.hip reports no name: after "eig", or "auto" outside the routes, the name is stale)
        jacobi = method == "eig" or (method == "auto" and (k > 64 or not have) and base == "eig")
        names[method] = "letkf_wave_kernel<double>" if jacobi else _cabi.last_analysis_kernel()
    if base is None and not have:        # (a build without the route has nothing to time here)
        return res
    res["declined"] = int(retry.item())
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    ts = {base: [], alt: []}
    for _ in range(rounds):
        if base is not None:
            ts[base].append(sample(base, 1 if base == "eig" else 4))
        ts[alt].append(sample(alt, 4 if have else 1))
    for method, key in ((base, "baseline_time"), (alt, "wide64" if have else "auto")):
        if method is None:
            continue
        v = np.array(ts[method])
        res[key] = dict(method=method, kernel=names[method], ms_median=float(np.median(v)), ms_min=float(v.min()),
                        ms_max=float(v.max()), spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v])
    if have:
        res["analyses_per_s_wide64"] = G / (res["wide64"]["ms_median"] * 1e-3)
        if base is not None:
            res["ratio_baseline_over_wide64"] = res["baseline_time"]["ms_median"] / res["wide64"]["ms_median"]
            # "at least 2x faster beyond both spreads": the slowest wide sample against the fastest baseline sample
            res["twice_as_fast_beyond_both_spreads"] = bool(res["baseline_time"]["ms_min"] >= 2.0 * res["wide64"]["ms_max"])
        cnt, idx = nb.cnt[:1024].cpu().numpy(), nb.idx[:1024].cpu().numpy()
        tiles = [[set(idx[g, :cnt[g]].tolist()) for g in range(t, t + 16)] for t in range(0, 1024, 16)]
        unions = [len(set().union(*t)) for t in tiles]
        res["union_mean"], res["union_max"] = float(np.mean(unions)), int(max(unions))
        dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
        res["model"] = mfma_model(k, int(nb.p_max), tiles, m, dmax_tile, cycles, (G + 15) // 16)
    if whole and (have or base is not None):
        # the whole class call in the default dtype
        loc = mia.GaspariCohn(c, mia.AbsoluteDistance())
        gxh, oxh = gx.cpu().numpy(), ox.cpu().numpy()
        filt = mia.LETKF(localization=loc, inf_factor=1.1, engine=eng)
        filt.analyse_arrays(X, Yb, d, grid_coords=gxh, obs_coords=oxh)
        torch.cuda.synchronize()
        v = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            filt.analyse_arrays(X, Yb, d, grid_coords=gxh, obs_coords=oxh)
            b.record()
            b.synchronize()
            v.append(a.elapsed_time(b))
        res["analyse_arrays_float64_ms"] = dict(ms_median=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--cases", help="semicolon-separated cases in the place of the built-in list")
    ap.add_argument("--whole", action="store_true", help="with --case: also time the whole LETKF(...).analyse_arrays call")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mfma-cycles", type=float, default=64.0)
    ap.add_argument("--out")
    ap.add_argument("--parent", help="JSON of a run of this tool on a build of the parent commit: merged case by case")
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, a.mfma_cycles, a.whole)))
        return 0
    parent = {}
    if a.parent:
        with open(a.parent) as fh:
            parent = dict((json.dumps(r["case"], sort_keys=True), r) for r in json.load(fh)["results"])
    results = []

    def dump():
        return json.dumps({"tool": "tools/time_wide64.py", "results": results}, indent=1)
    cases = a.cases.split(";") if a.cases else CASES
    for i, spec in enumerate(cases):    # one fresh process per case, each under its own time limit; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds),
                                "--mfma-cycles", str(a.mfma_cycles)] + (["--whole"] if i == 0 else []),
                               capture_output=True, text=True, timeout=a.timeout)
            status, tail = r.returncode, r.stdout[-2000:] + r.stderr[-4000:]
        except subprocess.TimeoutExpired as err:       # (the child is killed; reported like any other failed case)
            status, tail = "timeout after %d s" % a.timeout, str(err.stderr or "")[-4000:]
        if status != 0:
            sys.stderr.write(tail)
            failed = {"tool": "tools/time_wide64.py", "failed_case": spec, "exit_status": status, "results": results}
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(json.dumps(failed, indent=1) + "\n")
            print(json.dumps(failed))
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        p = parent.get(json.dumps(res["case"], sort_keys=True))
        if p is not None and p["baseline"] == "eig":
            res["eig_parent_build"] = p.get("baseline_time", p.get("baseline_unsupported"))
            res["auto_parent_build"] = p.get("auto")
            if "wide64" in res and "baseline_time" in p:
                res["ratio_parent_eig_over_wide64"] = p["baseline_time"]["ms_median"] / res["wide64"]["ms_median"]
            if "analyse_arrays_float64_ms" in p:
                res["analyse_arrays_parent_build_ms"] = p["analyse_arrays_float64_ms"]
        results.append(res)
        first, second = res.get("baseline_time"), res.get("wide64", res.get("auto"))
        print("%s: %s %s ms, %s %s ms, declined %s" % (spec, res["baseline"], first and "%.3f" % first["ms_median"],
              second and second["method"], second and "%.3f" % second["ms_median"], res.get("declined")), file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(dump() + "\n")
    print(dump())
    return 0


if __name__ == "__main__":
    sys.exit(main())

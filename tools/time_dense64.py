#!/usr/bin/env python3
"""Float64 analysis time on DENSE local networks (p_max > k): the Jacobi kernel (method="eig": letkf_wave_kernel<double>, what
these shapes ran on before the dense tile route existed -- and what method="auto" still runs where the cover function says no)
against the dense float64 tile route (method="dense64": letkf_dense64_kernel), alternating in ONE process.  Sibling of
tools/time_f64.py, which times the sparse shapes (p_max <= k).

    python tools/time_dense64.py                      # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_dense64.py --case 40,1,20,1     # one case (k, obs stride, radius, state rows) in this process
    python tools/time_dense64.py --case mesh,40,316,3,1   # n x n mesh, an observation at every point (k, n, radius, state rows)
    python tools/time_dense64.py --out profiles/dense64_time.json

1e5 grid points, seeded inputs, neighbour lists and packed records built once outside the timed region; the analysis call alone
is timed with device events, `reps` calls per sample, `rounds` samples per method, the methods alternating.  Reported per case:
median and min-max of both, their ratio, the decline count, the kernel's matrix-instruction count per tile (from the lists of
the first 64 tiles, split into the parts the kernel analyses them in, and the measured degrees) and the time those instructions
alone would take at `--mfma-cycles` per instruction and SIMD (tools/mfma_rate_f64.hip) on the waves that are RESIDENT at the
launch's LDS size, and for the first
case the whole LETKF(...).analyse_arrays call in float64 with the tile routes on and off (tile = 1 / 0)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["40,1,20,1", "40,1,20,8", "40,1,45,1", "20,1,8,1", "64,1,40,1", "mesh,40,316,3,1"]


def lds_bytes(ub, kp):
    """Restates dense64_lds_bytes (csrc/letkf_dense64.hip)."""
    umax = 16 * ub
    return -(-((umax * (kp | 1) + 16 * (umax + 1)) * 8 + umax * 4) // 16) * 16


def launch_blocks(k, p_max, max_lds=160 * 1024):
    """Restates dense64_blocks: the sixteen-slot blocks of the record image a launch takes."""
    kp = (k + 4) & ~3
    cap = 16
    while cap > 0 and lds_bytes(cap, kp) > max_lds:
        cap -= 1
    return min((p_max + 31) >> 4, cap)


def tile_parts(lists, umax):
    """Union sizes of the parts a tile of sixteen lists is analysed in: halved, as the kernel does, until the union fits."""
    parts, lo = [], 0
    while lo < len(lists):
        n = 16
        while True:
            u = len(set().union(*lists[lo:lo + n]))
            if u <= umax or n == 1:
                break
            n >>= 1
        parts.append(u)
        lo += n
    return parts


def mfma_model(k, p_max, tiles, m, deg_tile, cycles, n_tiles, clock_ghz=2.4, cus=256, lds_per_cu=160 * 1024):
    """tiles: the neighbour lists of some tiles (sixteen sets each).  Per part of a tile with `b` blocks: the bound is b^2 Gram
    blocks of 4 KT + 4 instructions, rhs 4 KT b, a recurrence step 8 KT b.  One wavefront per workgroup and at most one wave per
    SIMD (registers), so a compute unit holds min(4, LDS per CU / LDS per workgroup) waves, each with a matrix pipe of its own:
    the pipe-only time is the instructions of all tiles over the RESIDENT waves."""
    kt = (k + 15) // 16
    ub = launch_blocks(k, p_max)
    lds = lds_bytes(ub, (k + 4) & ~3)
    wg_per_cu = max(1, min(4, lds_per_cu // lds))
    per_tile, nparts = [], []
    for lists in tiles:
        parts = tile_parts(lists, 16 * ub)
        nparts.append(len(parts))
        per_tile.append(sum(b * b * (4 * kt + 4) + 4 * kt * b + m * deg_tile * 8 * kt * b for b in (max(1, (u + 15) // 16) for u in parts)))
    mean = sum(per_tile) / len(per_tile)
    return dict(kt=kt, launch_blocks=ub, lds_bytes=lds, workgroups_per_cu=wg_per_cu, waves_per_simd=wg_per_cu / 4.0,
                parts_per_tile_mean=sum(nparts) / len(nparts), mfma_per_tile=mean, cycles_per_mfma=cycles,
                matrix_pipe_ms=mean * cycles * (n_tiles / (cus * wg_per_cu)) / (clock_ghz * 1e6))


def make_inputs(spec, dev):
    import numpy as np
    import torch
    import bench
    f = spec.split(",")
    if f[0] == "mesh":
        k, n, c, m = int(f[1]), int(f[2]), float(f[3]), int(f[4])
        gy, gx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
        grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
        gen = torch.Generator(device="cpu").manual_seed(42)
        X = torch.randn((1, k, n * n), generator=gen, dtype=torch.float64).to(dev)
        y = torch.randn(n * n, generator=gen, dtype=torch.float64).to(dev)
        mean = X[0].mean(dim=0)
        Yb, d = X[0] - mean, y - mean
        return dict(k=k, m=m, c=c, X=X, grid=grid, obs=grid, Yb=Yb, d=d, desc=dict(mesh=n, k=k, radius=c, state_rows=m))
    k, stride, c, m = int(f[0]), int(f[1]), float(f[2]), int(f[3])
    X, gx, ox, Yb, d = bench.make_case(100000, k, stride, dev, seed=42)
    return dict(k=k, m=m, c=c, X=X.double(), grid=gx, obs=ox, Yb=Yb.double(), d=d.double(),
                desc=dict(k=k, obs_stride=stride, radius=c, state_rows=m))


def one_case(spec, rounds, cycles, whole):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    inp = make_inputs(spec, dev)
    k, m, c, X = inp["k"], inp["m"], inp["c"], inp["X"]
    G = X.shape[-1]
    if m > 1:
        X = (X.repeat(m, 1, 1) * torch.linspace(0.5, 2.0, m, device=dev, dtype=torch.float64)[:, None, None]).contiguous()
    nb = eng.localize(inp["grid"], inp["obs"], [c])
    rec = eng.pack_obs(inp["Yb"], inp["d"], torch.float64)
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

    # a library without the dense route (the parent build of an A/B run) times "auto" in its place: both are the Jacobi kernel
    alt = "dense64" if "mia_letkf_analysis_dense_f64" in _cabi.EXPORTED_SYMBOLS else "auto"
    res = {"case": dict(inp["desc"], grid_points=G, p_max=int(nb.p_max)), "second_method": alt}
    names = {}
    for method in ("eig", alt):          # warm-up (table, code objects, clocks)
        retry.zero_()
        for _ in range(2):
            call(method)
        torch.cuda.synchronize()
        if method == alt:      # (letkf_wave.hip reports no name: after "eig", or "auto" outside the routes, the name is stale)
            names["dense64"] = _cabi.last_analysis_kernel() if alt == "dense64" else "letkf_wave_kernel<double>"
        else:
            names["eig"] = "letkf_wave_kernel<double>"
    res["declined"] = int(retry.item())
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    ts = {"eig": [], "dense64": []}
    for _ in range(rounds):
        ts["eig"].append(sample("eig", 2))
        ts["dense64"].append(sample(alt, 4))
    for method in ts:
        v = np.array(ts[method])
        res[method] = dict(kernel=names[method], ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                           spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v])
    res["ratio_eig_over_dense64"] = res["eig"]["ms_median"] / res["dense64"]["ms_median"]
    res["analyses_per_s_dense64"] = G / (res["dense64"]["ms_median"] * 1e-3)
    # "at least 2x faster beyond both spreads": the slowest dense sample against the fastest Jacobi sample
    res["twice_as_fast_beyond_both_spreads"] = bool(res["eig"]["ms_min"] >= 2.0 * res["dense64"]["ms_max"])
    # the model: the lists of the first 64 tiles, the per-tile degree is the largest of its sixteen points
    cnt, idx = nb.cnt[:1024].cpu().numpy(), nb.idx[:1024].cpu().numpy()
    tiles = [[set(idx[g, :cnt[g]].tolist()) for g in range(t, t + 16)] for t in range(0, 1024, 16)]
    unions = [len(set().union(*t)) for t in tiles]
    res["union_mean"], res["union_max"] = float(np.mean(unions)), int(max(unions))
    dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
    res["model"] = mfma_model(k, int(nb.p_max), tiles, m, dmax_tile, cycles, (G + 15) // 16)
    if whole:
        # the whole class call, float64, with the tile routes on and off
        loc = mia.GaspariCohn(c, mia.AbsoluteDistance())
        gxh, oxh = inp["grid"].cpu().numpy(), inp["obs"].cpu().numpy()
        tw = {}
        for tile in (1, 0):
            old = _cabi.set_option("tile", tile)
            try:
                f = mia.LETKF(localization=loc, inf_factor=1.1, engine=eng)
                f.analyse_arrays(X, inp["Yb"], inp["d"], grid_coords=gxh, obs_coords=oxh)
                torch.cuda.synchronize()
                v = []
                for _ in range(3):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f.analyse_arrays(X, inp["Yb"], inp["d"], grid_coords=gxh, obs_coords=oxh)
                    b.record()
                    b.synchronize()
                    v.append(a.elapsed_time(b))
                tw["tile=%d" % tile] = dict(ms_median=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v)))
            finally:
                _cabi.set_option("tile", old)
        res["analyse_arrays_float64_ms"] = tw
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--whole", action="store_true", help="with --case: also time the whole LETKF(...).analyse_arrays call")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mfma-cycles", type=float, default=64.0)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, a.mfma_cycles, a.whole)))
        return 0
    results = []
    for i, spec in enumerate(CASES):   # one fresh process per case, each under its own time limit; the first failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds),
                            "--mfma-cycles", str(a.mfma_cycles)] + (["--whole"] if i == 0 else []),
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("%s: eig %.3f ms, dense64 %.3f ms, ratio %.1f, declined %d" % (spec, results[-1]["eig"]["ms_median"],
              results[-1]["dense64"]["ms_median"], results[-1]["ratio_eig_over_dense64"], results[-1]["declined"]),
              file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(json.dumps({"tool": "tools/time_dense64.py", "results": results}, indent=1) + "\n")
    print(json.dumps({"tool": "tools/time_dense64.py", "results": results}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Float64 RBF-kernelised analysis time (LKETKF / LETKF with an RBF or Gauss kernel in the default dtype): the Jacobi kernel
(method="eig": letkf_wave_kernel<double>, what the float64 RBF core ran on before the tile route existed) against the float64 RBF
tile route (method="rbf64": lketkf_tile64_kernel), alternating in ONE process.  Sibling of tools/time_wide64.py.

    python tools/time_rbf64.py                      # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_rbf64.py --case 40,2,10,1     # one case (k, obs stride, radius, state rows) in this process
    python tools/time_rbf64.py --case mesh,40,316,2,2.5,1   # n x n mesh (k, n, obs stride, radius, state rows)
    python tools/time_rbf64.py --out profiles/rbf64_time.json --parent parent.json

1e5 grid points (99 856 on the meshes), seeded inputs, gamma 0.5, inflation 1.1; neighbour lists and packed records are built once outside the timed
region; the analysis call alone is timed with device events, `reps` calls per sample, `rounds` samples per method, the methods
alternating.  Reported per case: median and min-max of both, their ratio, the decline count, the degrees, and a count of what a
tile costs: the matrix instructions of the Dist product per wavefront (pair blocks x 4 UT x parts / 4 wavefronts) with the time
they alone would take at `--mfma-cycles` per instruction with the workgroups resident at the launch's LDS size, the float64
exponentials, and the multiply-adds of the per-point recurrence per thread -- where the time above the matrix pipe goes.  For the
first case also the whole LKETKF(...).analyse_arrays call in the default dtype.

On a build WITHOUT the route (the parent commit of an A/B run) "auto" is timed in the place of "rbf64" -- both are then the
Jacobi kernel -- and `--parent FILE` merges such a run's figures into this one's as `eig_parent_build` / `analyse_arrays_parent_build_ms`."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, INF = 0.5, 1.1
# config 5; k = 20; config 5 with 8 state rows; dense network (p <= 59, unions above 64 slots: tiles in parts); a small ensemble;
# the corners at 8 state rows; 316 x 316 meshes in row-major order (sixteen consecutive points see far more observations than
# one does: tiles in many parts) with observations at every second point (p <= 21) and at every point (p <= 61)
CASES = ["40,2,10,1", "20,2,10,1", "40,2,10,8", "40,1,15,1", "8,2,6,1", "40,1,15,8", "20,2,10,8", "8,2,6,8",
         "mesh,40,316,2,2.5,1", "mesh,40,316,2,2.5,8", "mesh,40,316,1,2.2,1"]


def launch_shape(k, p_max):
    """Restates rbf64_ut / rbf64_lds_bytes (csrc/lketkf_tile64.hip)."""
    ut = min(max((p_max + 8 + 15) >> 4, 1), 4)
    kp = (k + 1 + 3) & ~3
    npb = (k * (k + 1) // 2 + k + 15) >> 4
    region = max(16 * ut * (kp | 1) + 16 * (16 * ut + 1), 64 * k)
    lds = -(-((npb * 256 + region) * 8 + (16 * ut + 16 * npb + 48) * 4) // 16) * 16
    return ut, npb, lds


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


def cost_model(k, p_max, tiles, m, deg_tile, cycles, n_tiles, clock_ghz=2.4, cus=256, lds_per_cu=160 * 1024):
    ut, npb, lds = launch_shape(k, p_max)
    wg_per_cu = max(1, min(2, lds_per_cu // lds))         # (two workgroups of four wavefronts per compute unit at the most)
    nparts = [tile_parts(lists, 16 * ut) for lists in tiles]
    parts = sum(nparts) / len(nparts)
    mfma_wave = -(-npb // 4) * 4 * ut * parts
    nr = (k + 15) >> 4
    # per thread and part: row sums k NR adds; per state row (degree + 1) passes over the k members with NR + 2 multiply-adds each
    fma_thread = parts * (k * nr + m * ((deg_tile + 1) * k * (nr + 2) + k))
    return dict(ut=ut, pair_blocks=npb, lds_bytes=lds, workgroups_per_cu=wg_per_cu, parts_per_tile_mean=parts,
                mfma_per_tile_per_wave=mfma_wave, exp_per_tile=parts * npb * 256, fma_per_thread_per_tile=fma_thread,
                barriers_per_tile=parts * (8 + m * (deg_tile + 3)), cycles_per_mfma=cycles,
                matrix_pipe_ms=mfma_wave * cycles * (n_tiles / (cus * wg_per_cu)) / (clock_ghz * 1e6),
                # 64 lanes of float64 multiply-add issue in 4 cycles; one wavefront per SIMD and workgroup
                vector_fma_issue_ms=fma_thread * 4.0 * (n_tiles / (cus * wg_per_cu)) / (clock_ghz * 1e6))


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
    mesh = f[0] == "mesh"
    if mesh:       # n x n mesh, Euclidean distance, an observation at every stride-th point of both dimensions (bench.py's c2_mesh_2d recipe)
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
    out = torch.empty_like(X)
    flags = torch.empty(G, dtype=torch.int32, device=dev)
    retry = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(method):
        return eng.analysis(X, None, None, nb, INF, rec=rec, rbf_gamma=GAMMA, method=method, out=out, flags=flags, retry=retry,
                            defer_retry=True)

    def sample(method, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call(method)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    # a library without the route (the parent build of an A/B run) times "auto" in its place
    have = "mia_lketkf_rbf_analysis_matfun_f64" in _cabi.EXPORTED_SYMBOLS
    alt = "rbf64" if have else "auto"
    res = {"case": dict(k=k, obs_stride=stride, radius=c, state_rows=m, grid_points=G, p_max=int(nb.p_max), gamma=GAMMA,
                        inf_factor=INF, mesh=(n if mesh else 0)), "second_method": alt}
    names = {}
    for method in ("eig", alt):           # warm-up (table, code objects, clocks)
        retry.zero_()
        call(method)
        torch.cuda.synchronize()
        # (letkf_wave.hip reports no name: after "eig", or "auto" on a build without the route, the name is stale)
        names[method] = _cabi.last_analysis_kernel() if (method == "rbf64") else "letkf_wave_kernel<double>"
    res["declined"] = int(retry.item())
    if have:
        deg = ((flags >> 8) & 0xff).double()
        res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    ts = {"eig": [], alt: []}
    for _ in range(rounds):
        ts["eig"].append(sample("eig", 1))
        ts[alt].append(sample(alt, 4 if have else 1))
    for method, key in (("eig", "eig"), (alt, alt)):
        v = np.array(ts[method])
        res[key] = dict(method=method, kernel=names[method], ms_median=float(np.median(v)), ms_min=float(v.min()),
                        ms_max=float(v.max()), spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v])
    if have:
        res["analyses_per_s_rbf64"] = G / (res["rbf64"]["ms_median"] * 1e-3)
        res["ratio_eig_over_rbf64"] = res["eig"]["ms_median"] / res["rbf64"]["ms_median"]
        # "at least 2x faster beyond both spreads": the slowest rbf64 sample against the fastest Jacobi sample
        res["twice_as_fast_beyond_both_spreads"] = bool(res["eig"]["ms_min"] >= 2.0 * res["rbf64"]["ms_max"])
        s0 = (G // 2) // 16 * 16 if mesh else 0          # (a mesh's first rows are its edge: sixty-four tiles from the middle)
        cnt, idx = nb.cnt[s0:s0 + 1024].cpu().numpy(), nb.idx[s0:s0 + 1024].cpu().numpy()
        tiles = [[set(idx[g, :cnt[g]].tolist()) for g in range(t, t + 16)] for t in range(0, 1024, 16)]
        unions = [len(set().union(*t)) for t in tiles]
        res["union_mean"], res["union_max"] = float(np.mean(unions)), int(max(unions))
        dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
        res["model"] = cost_model(k, int(nb.p_max), tiles, m, dmax_tile, cycles, (G + 15) // 16)
    if whole and not mesh:
        # the whole class call in the default dtype
        loc = mia.GaspariCohn(c, mia.AbsoluteDistance())
        gxh, oxh = gx.cpu().numpy(), ox.cpu().numpy()
        filt = mia.LKETKF(mia.RBFKernel(GAMMA), localization=loc, inf_factor=INF, engine=eng)
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
        res["analyse_arrays_float64_ms"] = dict(ms_median=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v)),
                                                kernel=_cabi.last_analysis_kernel() if have else "letkf_wave_kernel<double>")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--cases", help="semicolon-separated cases in the place of the built-in list")
    ap.add_argument("--whole", action="store_true", help="with --case: also time the whole LKETKF(...).analyse_arrays call")
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
        return json.dumps({"tool": "tools/time_rbf64.py", "results": results}, indent=1)
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
            failed = {"tool": "tools/time_rbf64.py", "failed_case": spec, "exit_status": status, "results": results}
            if a.out:
                with open(a.out, "w") as fh:
                    fh.write(json.dumps(failed, indent=1) + "\n")
            print(json.dumps(failed))
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        p = parent.get(json.dumps(res["case"], sort_keys=True))
        if p is not None:
            res["eig_parent_build"] = p.get("eig")
            res["auto_parent_build"] = p.get("auto")
            if "rbf64" in res and "eig" in p:
                res["ratio_parent_eig_over_rbf64"] = p["eig"]["ms_median"] / res["rbf64"]["ms_median"]
            if "analyse_arrays_float64_ms" in p:
                res["analyse_arrays_parent_build_ms"] = p["analyse_arrays_float64_ms"]
        results.append(res)
        second = res.get("rbf64", res.get("auto"))
        print("%s: eig %.3f ms, %s %.3f ms, declined %s" % (spec, res["eig"]["ms_median"], second["method"], second["ms_median"],
                                                            res.get("declined")), file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(dump() + "\n")
    print(dump())
    return 0


if __name__ == "__main__":
    sys.exit(main())

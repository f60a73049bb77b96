#!/usr/bin/env python3
"""Float64 weights time of DENSE local networks (p_max > k) on 2-D MESHES: LetkfEngine.weights_patch64 with the map of 4 x 4
patches (letkf_patch64w_kernel, csrc/letkf_patch64w.hip) against LetkfEngine.weights_stream64 without a map on the same build
(letkf_stream64w_kernel: its file is untouched, so that is the parent's time) and against the Jacobi kernel with W written
(engine.analysis(method="eig", return_weights=True): letkf_wave_kernel<double>) where it runs.  Sibling of
tools/time_stream64w.py (the 1-D rows) and tools/time_patch64.py (the analysis under a map); the protocol is theirs.

    python tools/time_patch64w.py --out profiles/patch64w_time.json      # every case below, one child process each
    python tools/time_patch64w.py --case 80,3.0,316                       # one case (k, radius, mesh side) in this process
    python tools/time_patch64w.py --in-process --out FILE                 # every case in one process (one start-up)

Row-major ny x nx meshes with an observation at every point; seeded inputs, inflation 1.1, neighbour lists, packed records and
the map built outside the timed region, W allocated once per case; the engine call WITH the 8-byte read of the decline counter
under device events, `rounds` samples per method.  The census of the map (validation + largest union + its 8-byte read) is
paid by the FIRST call only and is reported separately.  Reported per case: median and min-max of the three, the ratios and
whether the factor 2 over the Jacobi kernel holds beyond both spreads, whether W and flags are bit-identical to the route
without a map, decline count, degrees, and for both tile routes the parts per tile, the matrix instructions per tile, the time
they would take at `--mfma-cycles` per instruction on the waves RESIDENT at the launch's LDS size, and the measured multiple."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = "tools/time_patch64w.py"
# (k, radius, mesh side): 316 x 316 = 99 856 points; 224 x 224 = 50 176 at k = 128 (as the k = 128 rows of tools/time_stream64w.py)
CASES = ["40,3.0,316", "64,3.0,316", "80,3.0,316", "96,3.0,316", "128,3.5,224"]


def lds_bytes(ub, k):
    """Restates ring64_lds_bytes (csrc/mia_frames64.h)."""
    umax, kp, kt = 16 * ub, (k + 4) & ~3, (k + 15) >> 4
    return -(-((2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (umax + 1)) * 8 + umax * 4) // 16) * 16


def tile_parts(lists, umax):
    """Union sizes of the parts a tile of up to sixteen lists is done in: halved, as the kernels do, until the union fits."""
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


def mfma_model(k, ub, tiles, degs, cycles, n_tiles, clock_ghz=2.4, cus=256, lds_per_cu=160 * 1024):
    """tiles: the lists of some tiles (up to sixteen sets each), degs: the largest degree of each.  Per part of a tile with b
    blocks: the bound is b^2 Gram blocks of 4 KT + 4 instructions, rhs 4 KT b, a recurrence step 8 KT b, and there are k member
    passes of the tile's largest degree (tools/time_stream64w.py's count).  One wavefront per workgroup, at most one wave per
    SIMD: a compute unit holds min(4, LDS per CU / LDS per workgroup) waves, each with a matrix pipe of its own."""
    kt = (k + 15) // 16
    lds = lds_bytes(ub, k)
    wg_per_cu = max(1, min(4, lds_per_cu // lds))
    per_tile, nparts = [], []
    for lists, deg in zip(tiles, degs):
        blocks = [max(1, (u + 15) // 16) for u in tile_parts(lists, 16 * ub)]
        nparts.append(len(blocks))
        per_tile.append(sum(b * b * (4 * kt + 4) + 4 * kt * b + k * deg * 8 * kt * b for b in blocks))
    mean = sum(per_tile) / len(per_tile)
    return dict(kt=kt, launch_blocks=ub, lds_bytes=lds, workgroups_per_cu=wg_per_cu, parts_per_tile_mean=sum(nparts) / len(nparts),
                mfma_per_tile=mean, cycles_per_mfma=cycles, tiles=n_tiles,
                matrix_pipe_ms=mean * cycles * (n_tiles / (cus * wg_per_cu)) / (clock_ghz * 1e6))


def one_case(spec, rounds, cycles):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    f = spec.split(",")
    k, c, side = int(f[0]), float(f[1]), int(f[2])
    ny = nx = side
    G = ny * nx
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    gen = torch.Generator(device="cpu").manual_seed(42)
    gy, gx = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    X = torch.randn((1, k, G), generator=gen, dtype=torch.float64).to(dev)
    y = torch.randn(G, generator=gen, dtype=torch.float64).to(dev)
    mean = X[0].mean(dim=0)
    Yb, d = (X[0] - mean).contiguous(), (y - mean).contiguous()      # an observation of the state at every point, unit error variance
    nb = eng.localize(grid, grid, [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
    tiles = mia.mesh_tiles((ny, nx))
    out = torch.empty_like(X)
    W = torch.empty((G, k, k), dtype=torch.float64, device=dev)

    def eig():              # (allocates its W inside the call: a cached block after the warm-up, no device allocation)
        return eng.analysis(X, None, None, nb, 1.1, rec=rec, method="eig", out=out, return_weights=True)[1]

    def stream():
        r = eng.weights_stream64(Yb, None, nb, 1.1, rec=rec, out=W, return_flags=True)
        assert r is not None, "weights_stream64 refused the shape"
        return r

    def patch():
        r = eng.weights_patch64(Yb, None, nb, tiles, 1.1, rec=rec, out=W, return_flags=True)
        assert r is not None, "weights_patch64 refused the shape"
        return r

    def sample(fn, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def timed(fn, kern=None):
        try:
            r = fn()                     # warm-up (table, code objects, clocks)
            torch.cuda.synchronize()
        except _cabi.MiaError as e:
            return dict(error="MiaError: %s" % e), None
        name = kern or _cabi.last_analysis_kernel()
        v = np.array([sample(fn) for _ in range(rounds)])
        return dict(kernel=name, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                    spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v]), r

    res = {"case": dict(k=k, mesh=[ny, nx], radius=c, obs_stride=1, grid_points=G, p_max=int(nb.p_max), weights_bytes=G * k * k * 8)}
    # the census: the first use of the map with these lists, its 8-byte read included
    res["census_ms"] = sample(lambda: eng.weights_patch64_fits(nb, tiles, k))
    umax = nb.tile_census[id(tiles)][2]
    res["largest_patch_union"] = int(umax)
    res["patch64w"], r = timed(patch)
    Wp, fp = r[0].clone() if k <= 64 else None, r[1].clone()
    probe_p = r[0][:4096].clone()
    res["stream64w"], r = timed(stream)
    res["flags_equal"] = bool(torch.equal(fp, r[1]))
    res["first_4096_points_equal"] = bool(torch.equal(probe_p, r[0][:4096]))
    if Wp is not None:
        res["weights_equal"] = bool(torch.equal(Wp, r[0]))
    del Wp
    flags = r[1]
    res["eig"], wref = timed(eig, "letkf_wave_kernel<double>")
    if wref is not None:
        res["rel_diff_eig_vs_patch64w_first_4096_points"] = float((torch.linalg.norm(wref[:4096] - probe_p) /
                                                                   torch.linalg.norm(wref[:4096])).item())
    del wref
    res["declined"] = int(((flags & 8) != 0).sum().item())
    deg = ((flags >> 8) & 0xff).cpu().numpy()
    res["degree_mean"], res["degree_max"] = float(deg.mean()), int(deg.max())
    # the model on the tiles of four patch rows / the strips of the same points in the middle of the mesh
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()
    tpr = (nx + 3) // 4
    t0 = (ny // 8) * tpr
    sel = tiles[t0:t0 + 4 * tpr].numpy()
    ptiles = [[set(idx[p, :cnt[p]].tolist()) for p in row if p >= 0] for row in sel]
    pdeg = [int(deg[row[row >= 0]].max()) for row in sel]
    g0 = int(sel[sel >= 0].min()) // 16 * 16
    strips = [list(range(g, min(g + 16, G))) for g in range(g0, g0 + 16 * len(sel), 16)]
    stiles = [[set(idx[p, :cnt[p]].tolist()) for p in row] for row in strips]
    sdeg = [int(deg[row].max()) for row in strips]
    res["strip_union_max"] = int(max(len(set().union(*t)) for t in stiles))
    res["model_patch64w"] = mfma_model(k, min(max((umax + 15) // 16, 1), 16), ptiles, pdeg, cycles, int(tiles.shape[0]))
    res["model_stream64w"] = mfma_model(k, min((int(nb.p_max) + 31) >> 4, 16), stiles, sdeg, cycles, (G + 15) // 16)
    for name in ("patch64w", "stream64w"):
        res["multiple_of_matrix_pipe_" + name] = res[name]["ms_median"] / res["model_" + name]["matrix_pipe_ms"]
    return ratios(res)


def ratios(res):
    """The Jacobi kernel and the route without a map over the route with one (counter read included), and whether the factor
    2 over the Jacobi kernel holds beyond both spreads: the slowest sample of the route against the fastest of the baseline"""
    p, s, e = res["patch64w"], res["stream64w"], res["eig"]
    res["ratio_stream64w_over_patch64w"] = s["ms_median"] / p["ms_median"]
    if "ms_median" in e:
        res["ratio_eig_over_patch64w"] = e["ms_median"] / p["ms_median"]
        res["ratio_eig_over_patch64w_worst_case"] = e["ms_min"] / p["ms_max"]
        res["twice_as_fast_as_eig_beyond_both_spreads"] = bool(e["ms_min"] >= 2.0 * p["ms_max"])
        res["ratio_eig_over_stream64w"] = e["ms_median"] / s["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--cases", help="semicolon-separated list in place of the default cases")
    ap.add_argument("--in-process", action="store_true", help="every case in THIS process, one after the other (one start-up)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mfma-cycles", type=float, default=64.0)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240)
    a = ap.parse_args()

    def write(results):
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(json.dumps({"tool": TOOL, "results": results}, indent=1) + "\n")

    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, a.mfma_cycles)))
        return 0
    results = []
    for spec in (a.cases.split(";") if a.cases else CASES):       # the first failure ends the run
        if a.in_process:
            res = one_case(spec, a.rounds, a.mfma_cycles)
        else:                          # one fresh process per case, each under its own time limit
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds),
                                "--mfma-cycles", str(a.mfma_cycles)], capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
                return 1
            res = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(res)
        print("%s: patch64w %s, stream64w %s, eig %s" % (spec, res["patch64w"]["ms_median"], res["stream64w"]["ms_median"],
              res["eig"].get("ms_median", res["eig"].get("error", ""))), file=sys.stderr, flush=True)
        write(results)
    print(json.dumps({"tool": TOOL, "results": results}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

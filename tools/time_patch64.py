#!/usr/bin/env python3
"""Per-case timing on the GPU of the float64 dense analysis on 2-D meshes: the Jacobi eigensolver kernel (method="eig":
letkf_wave_kernel<double>), the dense tile route on strips of sixteen consecutive points (method="dense64":
letkf_dense64_kernel) and the same analysis on 4 x 4 patches of the mesh (method="patch64": letkf_patch64_kernel, map from
mesh_tiles), alternating in ONE process.  Sibling of tools/time_dense64.py.

    python tools/time_patch64.py                          # every case below, one child process each (own time limit), JSON to stdout
    python tools/time_patch64.py --case 40,316,3,1,1      # one case (k, mesh side n, radius, state rows, observation stride)
    python tools/time_patch64.py --out profiles/patch64_time.json

n x n mesh in row-major order, an observation at every `stride`-th point both ways, seeded inputs, neighbour lists, packed
records and the tile map built once outside the timed region; the analysis call alone is timed with device events, `reps` calls
per sample, `rounds` samples per method, the methods alternating.  patch64 is timed twice: with the census result kept on the
lists (what a cycled filter pays) and with the census -- validation, count, 8-byte read -- inside every call.  Reported per
case: median and min-max of each, the ratios, the decline count, the union of a tile's lists under strips and under patches
(every 16th tile, on the CPU) and the census' own maximum, the blocks of the record image the census chose, the LDS of a
workgroup and the workgroups a compute unit holds, and the matrix-pipe time of time_dense64.py's model (8 KT UB instructions per
recurrence step, one pass per tile)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["40,316,3,1,1", "40,316,3,8,1", "20,316,2,1,1", "64,316,3,1,1", "40,316,5,1,2"]


def lds_bytes(ub, kp):
    """Restates patch64_lds_bytes (csrc/letkf_patch64.hip)."""
    umax = 16 * ub
    return -(-((umax * (kp | 1) + 16 * (umax + 1)) * 8 + umax * 4) // 16) * 16


def resident(k, ub, lds_per_cu=160 * 1024):
    """workgroups (of one wavefront) a compute unit holds: the registers allow 4 (8 at KT = 1), the LDS the rest"""
    return max(1, min(8 if k <= 16 else 4, lds_per_cu // lds_bytes(ub, (k + 4) & ~3)))


def one_case(spec, rounds, cycles):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    f = spec.split(",")
    k, n, c, m, stride = int(f[0]), int(f[1]), float(f[2]), int(f[3]), int(f[4])
    G = n * n
    gy, gx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    sel = ((grid[:, 0] % stride) == 0) & ((grid[:, 1] % stride) == 0)
    gen = torch.Generator(device="cpu").manual_seed(42)
    X = torch.randn((1, k, G), generator=gen, dtype=torch.float64).to(dev)
    y = torch.randn(G, generator=gen, dtype=torch.float64).to(dev)
    seld = torch.as_tensor(sel, device=dev)
    mean = X[0].mean(dim=0)
    Yb, d = (X[0] - mean)[:, seld].contiguous(), (y - mean)[seld].contiguous()
    if m > 1:
        X = (X.repeat(m, 1, 1) * torch.linspace(0.5, 2.0, m, device=dev, dtype=torch.float64)[:, None, None]).contiguous()
    nb = eng.localize(grid, grid[sel], [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
    tiles = mia.mesh_tiles((n, n)).to(dev)
    out = torch.empty_like(X)
    flags = torch.empty(G, dtype=torch.int32, device=dev)
    retry = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(method, **kw):
        if method == "patch64_census":      # the census inside the call: forget what the lists keep
            nb.tile_census = None
            method = "patch64"
        if method.startswith("patch64"):
            kw["tile_points"] = tiles
            method = "patch64"
        return eng.analysis(X, None, None, nb, 1.1, rec=rec, method=method, out=out, flags=flags, retry=retry, defer_retry=True,
                            **kw)

    def sample(method, reps, **kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call(method, **kw)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    res = {"case": dict(mesh=n, k=k, radius=c, state_rows=m, obs_stride=stride, grid_points=G, p_max=int(nb.p_max))}
    names, declined, results = {}, {}, {}
    for method in ("eig", "dense64", "patch64"):          # warm-up (table, code objects, clocks)
        retry.zero_()
        for _ in range(2):
            call(method)
        torch.cuda.synchronize()
        names[method] = "letkf_wave_kernel<double>" if method == "eig" else _cabi.last_analysis_kernel()
        declined[method] = int(retry.item()) // 2
        results[method] = out.clone()
    names["patch64_census"] = names["patch64"]
    res["declined"] = declined
    res["patch64_equals_dense64_bit_for_bit"] = bool(torch.equal(results["patch64"], results["dense64"]))
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    union_census = nb.tile_census[id(tiles)][2]
    kp, kt = (k + 4) & ~3, (k + 15) // 16
    cap = eng._dense64_capacity_blocks(k)
    ub = min(max((union_census + 15) // 16, 1), cap)
    ub_strips = min((int(nb.p_max) + 31) >> 4, cap)
    res["patch64_image"] = dict(union_blocks=ub, lds_bytes=lds_bytes(ub, kp), workgroups_per_cu=resident(k, ub))
    res["dense64_image"] = dict(union_blocks=ub_strips, lds_bytes=lds_bytes(ub_strips, kp), workgroups_per_cu=resident(k, ub_strips))
    methods = ["eig", "dense64", "patch64", "patch64_census"]
    # for information: the largest image that lets one more workgroup share a compute unit (the few tiles above it run in halves)
    ub_alt = next((u for u in range(ub - 1, (int(nb.p_max) + 15) // 16 - 1, -1) if resident(k, u) > resident(k, ub)), None)
    ts = {mth: [] for mth in methods}
    if ub_alt is not None:
        ts["patch64_smaller_image"] = []
        names["patch64_smaller_image"] = names["patch64"]
        res["patch64_smaller_image_blocks"] = dict(union_blocks=ub_alt, lds_bytes=lds_bytes(ub_alt, kp),
                                                   workgroups_per_cu=resident(k, ub_alt))
        call("patch64", union_blocks=ub_alt)
    for _ in range(rounds):
        ts["eig"].append(sample("eig", 2))
        ts["dense64"].append(sample("dense64", 4))
        ts["patch64"].append(sample("patch64", 4))
        ts["patch64_census"].append(sample("patch64_census", 4))
        if ub_alt is not None:
            ts["patch64_smaller_image"].append(sample("patch64", 4, union_blocks=ub_alt))
    for method in ts:
        v = np.array(ts[method])
        res[method] = dict(kernel=names[method], ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                           spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v])
    res["census_ms"] = res["patch64_census"]["ms_median"] - res["patch64"]["ms_median"]
    res["ratio_eig_over_dense64"] = res["eig"]["ms_median"] / res["dense64"]["ms_median"]
    res["ratio_eig_over_patch64"] = res["eig"]["ms_median"] / res["patch64"]["ms_median"]
    res["ratio_eig_over_patch64_census"] = res["eig"]["ms_median"] / res["patch64_census"]["ms_median"]
    # "at least 2x faster beyond both spreads": the slowest patch sample (census inside) against the fastest Jacobi sample
    res["twice_as_fast_beyond_both_spreads"] = bool(res["eig"]["ms_min"] >= 2.0 * res["patch64_census"]["ms_max"])
    # unions of every 16th tile under both tilings
    cnt, idx = nb.cnt.cpu().numpy(), nb.idx.cpu().numpy()

    def unions(rows):
        return [len(np.unique(np.concatenate([idx[p, :cnt[p]] for p in row if p >= 0]))) for row in rows]
    us = unions([range(t, min(t + 16, G)) for t in range(0, G, 16)][::16])
    up = unions(tiles.cpu().numpy()[::16])
    res["union_strips"] = dict(mean=float(np.mean(us)), max=int(max(us)))
    res["union_patches"] = dict(mean=float(np.mean(up)), max=int(max(up)), census_max=int(union_census))
    # the matrix pipe alone: bound UB^2 (4 KT + 4), rhs 4 KT UB, a recurrence step 8 KT UB per state row, one pass per tile
    ubm = float(np.mean([max(1, (u + 15) // 16) for u in up]))
    dtile = float(deg.max().item())
    per_tile = ubm * ubm * (4 * kt + 4) + 4 * kt * ubm + m * dtile * 8 * kt * ubm
    wg = resident(k, ub)
    res["model"] = dict(kt=kt, blocks_per_tile_mean=ubm, degree=dtile, mfma_per_tile=per_tile, cycles_per_mfma=cycles,
                        matrix_pipe_ms=per_tile * cycles * (tiles.shape[0] / (256 * wg)) / 2.4e6)
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
    for spec in CASES:      # one fresh process per case, each under its own time limit; the first failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds),
                            "--mfma-cycles", str(a.mfma_cycles)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        x = results[-1]
        print("%s: eig %.3f ms, dense64 %.3f ms, patch64 %.3f ms (census inside %.3f), eig / patch64 %.2f, declined %r" % (
              spec, x["eig"]["ms_median"], x["dense64"]["ms_median"], x["patch64"]["ms_median"], x["patch64_census"]["ms_median"],
              x["ratio_eig_over_patch64"], x["declined"]), file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(json.dumps({"tool": "tools/time_patch64.py", "results": results}, indent=1) + "\n")
    print(json.dumps({"tool": "tools/time_patch64.py", "results": results}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

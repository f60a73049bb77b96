#!/usr/bin/env python3
"""Float64 analysis time on DENSE local networks (p_max > k) of 65 .. 128 members: the streamed dense tile route
(method="stream64": letkf_stream64_kernel, csrc/letkf_stream64.hip) against the Jacobi kernel (method="eig":
letkf_wave_kernel<double>), which is what these shapes ran on before -- or raised MiaError on, from 97 members.  Sibling of
tools/time_dense64.py (k <= 64) and tools/time_wide64.py (p_max <= k).

    python tools/time_stream64.py                          # every case below, one child process each (own time limit)
    python tools/time_stream64.py --case 80,93,1           # one 1-D case (k, p_max, state rows) in this process
    python tools/time_stream64.py --case mesh,80,316,3,1   # n x n mesh, an observation at every point (k, n, radius, state rows)
    python tools/time_stream64.py --in-process --out this.json                       # every case in one process
    python tools/time_stream64.py --in-process --only-eig --root DIR --out parent.json
    python tools/time_stream64.py --merge this.json parent.json --out profiles/stream64_time.json

The BASELINE is method="eig" on a build of the PARENT commit: --root names a checkout of it that has been built
(`python -c "import __graft_entry__ as g; g.build()"` there), --only-eig times "eig" alone from that tree and records its
MiaError where it raises, and --merge puts those figures in the place of this tree's "eig" (kept as "eig_this_tree").

1-D stride-1 networks at 1e5 grid points (5e4 at k = 128, as the wide tools do), the radius found by bisection for the p_max
asked for; seeded inputs, neighbour lists and packed records built once outside the timed region; the analysis call with the
8-byte read of the decline counter is timed with device events around `reps` calls, `rounds` samples per method.  Reported per
case: median and min-max of both, their ratio, the decline count, the kernel's matrix instructions per tile and recurrence step
(8 KT UB), the time all matrix instructions of the launch would take at `--mfma-cycles` per instruction on the waves that are
RESIDENT at the launch's LDS size, the measured multiple of it, and the bytes a recurrence step pulls through L2 (every block of
the union is fetched once per step: 16 UB records of kp doubles per tile)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["80,93,1", "80,93,8", "80,173,1", "80,173,8", "96,107,1", "96,107,8", "96,173,1", "96,173,8",
         "128,139,1", "128,139,8", "128,203,1", "128,203,8", "mesh,80,316,3,1", "mesh,80,316,3,8", "64,153,1"]


def lds_bytes(ub, k):
    """Restates ring64_lds_bytes (csrc/mia_frames64.h)."""
    umax, kp, kt = 16 * ub, (k + 4) & ~3, (k + 15) >> 4
    return -(-((2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (umax + 1)) * 8 + umax * 4) // 16) * 16


def launch_blocks(p_max):
    """Restates stream64_blocks: the sixteen-slot blocks of the slot table a launch takes."""
    return min((p_max + 31) >> 4, 16)


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
    SIMD (registers), so a compute unit holds min(4, LDS per CU / LDS per workgroup) waves, each with a matrix pipe of its own."""
    kt, kp = (k + 15) // 16, (k + 4) & ~3
    ub = launch_blocks(p_max)
    lds = lds_bytes(ub, k)
    wg_per_cu = max(1, min(4, lds_per_cu // lds))
    per_tile, nparts, step, fetched = [], [], [], []
    for lists in tiles:
        blocks = [max(1, (u + 15) // 16) for u in tile_parts(lists, 16 * ub)]
        nparts.append(len(blocks))
        step.append(sum(8 * kt * b for b in blocks))
        fetched.append(sum(16 * b * kp * 8 for b in blocks))
        per_tile.append(sum(b * b * (4 * kt + 4) + 4 * kt * b + m * deg_tile * 8 * kt * b for b in blocks))
    mean = sum(per_tile) / len(per_tile)
    return dict(kt=kt, launch_blocks=ub, lds_bytes=lds, workgroups_per_cu=wg_per_cu, waves_per_simd=wg_per_cu / 4.0,
                parts_per_tile_mean=sum(nparts) / len(nparts), mfma_per_tile_and_step=sum(step) / len(step),
                l2_bytes_per_tile_and_step=sum(fetched) / len(fetched), mfma_per_tile=mean, cycles_per_mfma=cycles,
                matrix_pipe_ms=mean * cycles * (n_tiles / (cus * wg_per_cu)) / (clock_ghz * 1e6))


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


def make_inputs(spec, dev, eng):
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
    k, p_max, m = int(f[0]), int(f[1]), int(f[2])
    c = find_radius(eng, p_max)
    X, gx, ox, Yb, d = bench.make_case(50000 if k > 96 else 100000, k, 1, dev, seed=42)
    return dict(k=k, m=m, c=c, X=X.double(), grid=gx, obs=ox, Yb=Yb.double(), d=d.double(),
                desc=dict(k=k, obs_stride=1, radius=c, p_max_asked=p_max, state_rows=m))


def one_case(spec, rounds, cycles, only_eig, root):
    import numpy as np
    import torch
    sys.path.insert(0, root)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    inp = make_inputs(spec, dev, eng)
    k, m, c, X = inp["k"], inp["m"], inp["c"], inp["X"]
    G = X.shape[-1]
    if m > 1:
        X = (X.repeat(m, 1, 1) * torch.linspace(0.5, 2.0, m, device=dev, dtype=torch.float64)[:, None, None]).contiguous()
    nb = eng.localize(inp["grid"], inp["obs"], [c])
    rec = eng.pack_obs(inp["Yb"], inp["d"], torch.float64)
    out = torch.empty_like(X)
    flags = torch.empty(G, dtype=torch.int32, device=dev)
    retry = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(method):      # the counter read (and the redo of declined points, if any) is part of the call
        return eng.analysis(X, None, None, nb, 1.1, rec=rec, method=method, out=out, flags=flags, retry=retry)

    def sample(method, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call(method)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def timed(method, reps):
        try:
            retry.zero_()
            call(method)                 # warm-up (table, code objects, clocks)
            torch.cuda.synchronize()
        except _cabi.MiaError as e:
            return dict(error="MiaError: %s" % e)
        kern = _cabi.last_analysis_kernel() if method != "eig" else "letkf_wave_kernel<double>"
        declined = int(retry.item())
        retry.zero_()
        v = np.array([sample(method, reps) for _ in range(rounds)])
        return dict(kernel=kern, declined=declined, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                    spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v])

    res = {"case": dict(inp["desc"], grid_points=G, p_max=int(nb.p_max))}
    res["eig"] = timed("eig", 1)
    if only_eig:
        return res
    alt = "stream64"
    res[alt] = timed(alt, 2)
    if k <= 64:                          # for information: the resident image against the streamed one on the same shape
        res["dense64"] = timed("dense64", 2)
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    cnt, idx = nb.cnt[:1024].cpu().numpy(), nb.idx[:1024].cpu().numpy()
    tiles = [[set(idx[g, :cnt[g]].tolist()) for g in range(t, t + 16)] for t in range(0, 1024, 16)]
    unions = [len(set().union(*t)) for t in tiles]
    res["union_mean"], res["union_max"] = float(np.mean(unions)), int(max(unions))
    dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
    res["model"] = mfma_model(k, int(nb.p_max), tiles, m, dmax_tile, cycles, (G + 15) // 16)
    if "ms_median" in res[alt]:
        res["multiple_of_matrix_pipe"] = res[alt]["ms_median"] / res["model"]["matrix_pipe_ms"]
        res["analyses_per_s_stream64"] = G / (res[alt]["ms_median"] * 1e-3)
    return res


def ratios(res):
    """eig over stream64, and whether it holds beyond both spreads; nothing where the baseline raised"""
    e, s = res["eig"], res.get("stream64", {})
    if "ms_median" in e and "ms_median" in s:
        res["ratio_eig_over_stream64"] = e["ms_median"] / s["ms_median"]
        res["twice_as_fast_beyond_both_spreads"] = bool(e["ms_min"] >= 2.0 * s["ms_max"])
    return res


def merge(this_json, parent_json):
    """results of this tree with 'eig' replaced by the parent tree's (same case order): the baseline of the issue"""
    this, base = json.load(open(this_json))["results"], json.load(open(parent_json))["results"]
    by_case = {json.dumps(b["case"], sort_keys=True): b for b in base}
    out = []
    for res in this:
        b = by_case.get(json.dumps(res["case"], sort_keys=True))
        if b is not None:
            res["eig_this_tree"] = res["eig"]
            res["eig"] = dict(b["eig"], tree="parent commit")
            for key in ("ratio_eig_over_stream64", "twice_as_fast_beyond_both_spreads"):
                res.pop(key, None)
            ratios(res)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--only-eig", action="store_true", help="time method='eig' alone (the baseline run in the parent's tree)")
    ap.add_argument("--root", default=ROOT, help="the tree the package is imported from (with --case or --in-process)")
    ap.add_argument("--cases", help="semicolon-separated list in place of the default cases")
    ap.add_argument("--in-process", action="store_true", help="every case in THIS process, one after the other (one start-up)")
    ap.add_argument("--merge", nargs=2, metavar=("THIS", "PARENT"), help="join two --out files: 'eig' from the parent's tree")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mfma-cycles", type=float, default=64.0)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=150)
    a = ap.parse_args()

    def write(results):
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(json.dumps({"tool": "tools/time_stream64.py", "results": results}, indent=1) + "\n")

    if a.merge:
        results = merge(*a.merge)
        write(results)
        for r in results:
            print(r["case"], r["eig"].get("ms_median", r["eig"].get("error")), r.get("stream64", {}).get("ms_median"),
                  r.get("ratio_eig_over_stream64"))
        return 0
    if a.case:
        print(json.dumps(ratios(one_case(a.case, a.rounds, a.mfma_cycles, a.only_eig, a.root))))
        return 0
    results = []
    for spec in (a.cases.split(";") if a.cases else CASES):       # the first failure ends the run
        if a.in_process:
            res = ratios(one_case(spec, a.rounds, a.mfma_cycles, a.only_eig, a.root))
        else:                          # one fresh process per case, each under its own time limit
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds), "--root", a.root,
                                "--mfma-cycles", str(a.mfma_cycles)] + (["--only-eig"] if a.only_eig else []),
                               capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
                return 1
            res = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(res)
        print("%s: eig %s, stream64 %s, ratio %s" % (spec, res["eig"].get("ms_median", res["eig"].get("error", "")),
              res.get("stream64", {}).get("ms_median"), res.get("ratio_eig_over_stream64")), file=sys.stderr, flush=True)
        write(results)
    print(json.dumps({"tool": "tools/time_stream64.py", "results": results}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

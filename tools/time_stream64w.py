#!/usr/bin/env python3
"""Float64 weights time on DENSE local networks (p_max > k) of up to 128 members: LetkfEngine.weights_stream64
(letkf_stream64w_kernel, csrc/letkf_stream64w.hip) against the Jacobi kernel with W written
(engine.analysis(method="eig", return_weights=True): letkf_wave_kernel<double>), which is what these weights ran on before -- or
raised MiaError on, from 97 members.  Sibling of tools/time_stream64.py (the analysis of these networks) and
tools/time_wide64w.py (the weights for p_max <= k).

    python tools/time_stream64w.py                          # every case below, one child process each (own time limit)
    python tools/time_stream64w.py --case 80,93             # one 1-D case (k, p_max) in this process
    python tools/time_stream64w.py --in-process --out this.json                       # every case in one process
    python tools/time_stream64w.py --in-process --only-eig --root DIR --out parent.json
    python tools/time_stream64w.py --merge this.json parent.json --out profiles/stream64w_time.json

The BASELINE is "eig" with W on a build of the PARENT commit: --root names a checkout of it that has been built
(`python -c "import __graft_entry__ as g; g.build()"` there), --only-eig times "eig" alone from that tree and records its
MiaError where it raises, and --merge puts those figures in the place of this tree's "eig" (kept as "eig_this_tree").

1-D stride-1 networks at 1e5 grid points (5e4 at k = 128), the radius found by bisection for the p_max asked for; seeded
inputs, neighbour lists and packed records built once outside the timed region, W (7.4 GB at k = 96) allocated once per case;
the engine call WITH the 8-byte read of the decline counter is timed with device events around `reps` calls, `rounds` samples
per method.  Reported per case: median and min-max of both, their ratio and whether it passes the factor 2 beyond both spreads,
the decline count, mean and largest degree, the kernel's matrix instructions per tile and member pass (degree x 8 KT UB), the
time all matrix instructions of the launch would take at `--mfma-cycles` per instruction on the waves that are RESIDENT at the
launch's LDS size, and the measured multiple of it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = "tools/time_stream64w.py"
# (k, p_max); the last one for information: the Jacobi kernel keeps k <= 64
CASES = ["80,93", "80,173", "96,107", "96,173", "128,139", "128,203", "65,77", "64,153"]


def lds_bytes(ub, k):
    """Restates ring64_lds_bytes (csrc/mia_frames64.h)."""
    umax, kp, kt = 16 * ub, (k + 4) & ~3, (k + 15) >> 4
    return -(-((2 * 16 * (kp | 1) + 4 * kt * 64 + 16 * (umax + 1)) * 8 + umax * 4) // 16) * 16


def launch_blocks(p_max):
    """Restates stream64w_blocks: the sixteen-slot blocks of the slot table a launch takes."""
    return min((p_max + 31) >> 4, 16)


def tile_parts(lists, umax):
    """Union sizes of the parts a tile of sixteen lists is done in: halved, as the kernel does, until the union fits."""
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


def mfma_model(k, p_max, tiles, deg_tile, cycles, n_tiles, clock_ghz=2.4, cus=256, lds_per_cu=160 * 1024):
    """tiles: the neighbour lists of some tiles (sixteen sets each).  Per part of a tile with `b` blocks: the bound is b^2 Gram
    blocks of 4 KT + 4 instructions, rhs 4 KT b, a recurrence step 8 KT b, and there are k member passes of `deg_tile` steps.
    One wavefront per workgroup and at most one wave per SIMD (registers), so a compute unit holds min(4, LDS per CU / LDS per
    workgroup) waves, each with a matrix pipe of its own."""
    kt = (k + 15) // 16
    ub = launch_blocks(p_max)
    lds = lds_bytes(ub, k)
    wg_per_cu = max(1, min(4, lds_per_cu // lds))
    per_tile, nparts, per_pass = [], [], []
    for lists in tiles:
        blocks = [max(1, (u + 15) // 16) for u in tile_parts(lists, 16 * ub)]
        nparts.append(len(blocks))
        per_pass.append(sum(deg_tile * 8 * kt * b for b in blocks))
        per_tile.append(sum(b * b * (4 * kt + 4) + 4 * kt * b + k * deg_tile * 8 * kt * b for b in blocks))
    mean = sum(per_tile) / len(per_tile)
    return dict(kt=kt, launch_blocks=ub, lds_bytes=lds, workgroups_per_cu=wg_per_cu, waves_per_simd=wg_per_cu / 4.0,
                parts_per_tile_mean=sum(nparts) / len(nparts), mfma_per_tile_and_pass=sum(per_pass) / len(per_pass),
                passes_per_tile=k, mfma_per_tile=mean, cycles_per_mfma=cycles,
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


def one_case(spec, rounds, cycles, only_eig, root):
    import numpy as np
    import torch
    sys.path.insert(0, root)
    import bench
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    f = spec.split(",")
    k, p_max = int(f[0]), int(f[1])
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    c = find_radius(eng, p_max)
    G = 50000 if k > 96 else 100000
    X, gx, ox, Yb, d = bench.make_case(G, k, 1, dev, seed=42)
    X, Yb, d = X.double(), Yb.double(), d.double()
    nb = eng.localize(gx, ox, [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
    out = torch.empty_like(X)
    state = {}

    def eig():              # (allocates its W inside the call: a cached block after the warm-up, no device allocation)
        return eng.analysis(X, None, None, nb, 1.1, rec=rec, method="eig", out=out, return_weights=True)[1]

    def stream():           # what the classes pay: the kernel and the 8-byte read of the decline counter
        r = eng.weights_stream64(Yb, None, nb, 1.1, rec=rec, out=state["W"], return_flags=True)
        assert r is not None, "weights_stream64 refused the shape"
        return r

    def sample(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def timed(fn, reps, kern=None):
        try:
            r = fn()                     # warm-up (table, code objects, clocks)
            torch.cuda.synchronize()
        except _cabi.MiaError as e:
            return dict(error="MiaError: %s" % e), None
        name = kern or _cabi.last_analysis_kernel()
        v = np.array([sample(fn, reps) for _ in range(rounds)])
        return dict(kernel=name, reps_per_sample=reps, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                    spread_ms=float(v.max() - v.min()), rounds=[float(x) for x in v]), r

    res = {"case": dict(k=k, obs_stride=1, radius=c, p_max_asked=p_max, grid_points=G, p_max=int(nb.p_max),
                        weights_bytes=G * k * k * 8)}
    res["eig"], wref = timed(eig, 1, "letkf_wave_kernel<double>")
    if only_eig:
        return res
    if wref is not None:                 # (one W at a time beside the baseline's: 7.4 GB each at k = 96)
        wnorm = float(torch.linalg.norm(wref).item())
        probe = wref[:4096].clone()
    del wref
    state["W"] = torch.empty((G, k, k), dtype=torch.float64, device=dev)
    res["stream64w"], r = timed(stream, 2)
    W, flags = r
    if "ms_median" in res["eig"]:
        res["rel_diff_eig_vs_stream64w_first_4096_points"] = float((torch.linalg.norm(probe - W[:4096]) / torch.linalg.norm(probe)).item())
        res["eig_weights_norm"] = wnorm
    res["declined"] = int(((flags & 8) != 0).sum().item())
    deg = ((flags >> 8) & 0xff).double()
    res["degree_mean"], res["degree_max"] = float(deg.mean().item()), int(deg.max().item())
    cnt, idx = nb.cnt[:1024].cpu().numpy(), nb.idx[:1024].cpu().numpy()
    tiles = [[set(idx[g, :cnt[g]].tolist()) for g in range(t, t + 16)] for t in range(0, 1024, 16)]
    unions = [len(set().union(*t)) for t in tiles]
    res["union_mean"], res["union_max"] = float(np.mean(unions)), int(max(unions))
    dmax_tile = deg[:G // 16 * 16].reshape(-1, 16).max(dim=1).values.mean().item()
    res["model"] = mfma_model(k, int(nb.p_max), tiles, dmax_tile, cycles, (G + 15) // 16)
    res["multiple_of_matrix_pipe"] = res["stream64w"]["ms_median"] / res["model"]["matrix_pipe_ms"]
    res["store_GB_per_s_stream64w"] = G * k * k * 8 / (res["stream64w"]["ms_median"] * 1e-3) / 1e9
    res["ms_per_1e5_points_stream64w"] = res["stream64w"]["ms_median"] * 1e5 / G
    return res


def ratios(res):
    """eig over stream64w (counter read included), and whether the factor 2 holds beyond both spreads: the slowest sample of the
    route against the fastest of the baseline; nothing where the baseline raised"""
    e, s = res["eig"], res.get("stream64w", {})
    if "ms_median" in e and "ms_median" in s:
        res["ratio_eig_over_stream64w"] = e["ms_median"] / s["ms_median"]
        res["ratio_worst_case"] = e["ms_min"] / s["ms_max"]
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
            for key in ("ratio_eig_over_stream64w", "ratio_worst_case", "twice_as_fast_beyond_both_spreads"):
                res.pop(key, None)
            ratios(res)
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--only-eig", action="store_true", help="time 'eig' with W alone (the baseline run in the parent's tree)")
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
                fh.write(json.dumps({"tool": TOOL, "results": results}, indent=1) + "\n")

    if a.merge:
        results = merge(*a.merge)
        write(results)
        for r in results:
            print(r["case"], r["eig"].get("ms_median", r["eig"].get("error")), r.get("stream64w", {}).get("ms_median"),
                  r.get("ratio_eig_over_stream64w"))
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
        print("%s: eig %s, stream64w %s, ratio %s" % (spec, res["eig"].get("ms_median", res["eig"].get("error", "")),
              res.get("stream64w", {}).get("ms_median"), res.get("ratio_eig_over_stream64w")), file=sys.stderr, flush=True)
        write(results)
    print(json.dumps({"tool": TOOL, "results": results}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

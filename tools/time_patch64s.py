#!/usr/bin/env python3
"""Float64 analysis time of DENSE local networks (p_max > k) of 65 .. 128 members on 2-D MESHES: LetkfEngine.analysis with the map
of 4 x 4 patches (method="patch64s": letkf_patch64s_kernel, csrc/letkf_patch64s.hip) against method="stream64" without a map
(letkf_stream64_kernel, what method="auto" runs there) and against the Jacobi kernel (method="eig") where it holds the shape.
Sibling of tools/time_patch64w.py (the weights under a map: the same meshes) and tools/time_ienks_patch64.py (the IEnKS update
under a map); the protocol is theirs.

    python tools/time_patch64s.py --parent-tree ../parent --out profiles/patch64s_time.json
                                                        # every case below: per case one child process on the package of the
                                                        # OTHER checkout (a build of the parent commit: the baselines), then one on
                                                        # this checkout's, joined, with the decision of LetkfEngine._patch64s_auto
    python tools/time_patch64s.py --out FILE            # this checkout alone
    python tools/time_patch64s.py --case 80,3.0,316,1   # one case (k, radius, mesh side, state rows) in this process

Row-major ny x nx meshes with an observation at every point; seeded inputs, neighbour lists, packed records, the map and its
census built outside the timed region, Xa and flags allocated once per case; the engine call WITH the 8-byte read of the decline
counter under device events, `calls` calls per sample (the tile routes: a sample is a quarter of a second and more), `rounds`
samples per method, the methods ALTERNATING in one process (round r times every method once before round r + 1), median, min
and max in ms per call.  The census of the map -- the first use of the map with these lists, its 8-byte read included -- is
timed once, before anything else, and reported beside the rows (census_ms): a cycled filter pays it once per geometry.  The
Jacobi kernel is asked first: where it cannot hold the shape the case records its MiaError.  A checkout without
method="patch64s" (the parent commit) times the other two.  The children run one after the other, each under its own time limit;
the first that fails ends the run.  With the parent's rows the decision is evaluated on the recorded samples, slowest sample of
the route against the fastest of the baseline (patch64s < stream64 of the PARENT build), and whether stream64 agrees between
the two builds within their spreads (its kernel is unchanged)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = "tools/time_patch64s.py"
# (k, radius, mesh side, state rows): 316 x 316 = 99 856 points; 224 x 224 = 50 176 at k = 128 (the meshes of tools/time_patch64w.py)
CASES = ["65,3.0,316,1", "80,3.0,316,1", "96,3.0,316,1", "80,3.0,316,8", "128,3.5,224,1"]
INF = 1.1


def stats(v, calls):
    import numpy as np
    v = np.array(v) / calls
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), spread_ms=float(v.max() - v.min()),
                calls_per_sample=calls, rounds=[float(x) for x in v])


def one_case(spec, rounds, tree):
    import numpy as np
    import torch
    sys.path.insert(0, tree)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    f = spec.split(",")
    k, c, side, m = int(f[0]), float(f[1]), int(f[2]), int(f[3])
    ny = nx = side
    G = ny * nx
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    gen = torch.Generator(device="cpu").manual_seed(42)
    gy, gx = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    X = torch.randn((m, k, G), generator=gen, dtype=torch.float64).to(dev)
    y = torch.randn(G, generator=gen, dtype=torch.float64).to(dev)
    mean = X[0].mean(dim=0)
    Yb, d = (X[0] - mean).contiguous(), (y - mean).contiguous()
    nb = eng.localize(grid, grid, [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
    out = torch.empty((m, k, G), dtype=torch.float64, device=dev)
    flags = torch.empty(G, dtype=torch.int32, device=dev)
    has_patch = "patch64s" in getattr(mia.LetkfEngine, "TILE64_NAMED_METHODS", ())
    tiles = mia.mesh_tiles((ny, nx)) if has_patch else None

    def call(method, **kw):
        return eng.analysis(X, None, None, nb, INF, rec=rec, out=out, flags=flags, return_flags=True, method=method, **kw)

    methods = {"stream64": lambda: call("stream64")}
    if has_patch:
        methods["patch64s"] = lambda: call("patch64s", tile_points=tiles)

    def sample(fn, calls=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    p_max = int(nb.p_max)
    res = {"case": dict(k=k, mesh=[ny, nx], radius=c, state_rows=m, obs_stride=1, grid_points=G, p_max=p_max),
           "stream64_auto": bool(eng._stream64_auto(m, k, p_max))}
    jacobi_fits = bool(eng._jacobi_primal_fits(k, p_max))
    res["jacobi_kernel_fits"] = jacobi_fits
    if jacobi_fits:
        methods["eig"] = lambda: call("eig")
    else:
        try:
            call("eig")
            raise AssertionError("the Jacobi kernel was expected to refuse the shape")
        except _cabi.MiaError as e:
            res["eig"] = dict(error="MiaError: %s" % e)
    if has_patch:       # the census: the first use of the map with these lists, its 8-byte read included
        res["census_ms"] = sample(lambda: eng._patch64_map(nb, tiles, None, k, 16))
        res["largest_patch_union"] = int(nb.tile_census[id(tiles)][2])
        res["every_tile_fits_one_pass"] = bool(eng.patch64s_fits(nb, tiles, k))
        res["patch64s_auto"] = bool(eng._patch64s_auto(m, k, p_max))
    kernels, keep = {}, {}
    for name, fn in methods.items():          # warm-up (table, code objects, clocks) and the results for the comparison
        r = fn()
        torch.cuda.synchronize()
        kernels[name] = _cabi.last_analysis_kernel() if name != "eig" else "letkf_wave_kernel<double> (not reported)"
        keep[name] = (r[0].clone(), r[1].clone())
    calls = {name: (1 if name == "eig" else 4) for name in methods}
    v = {name: [] for name in methods}
    for _ in range(rounds):                   # the methods alternate
        for name, fn in methods.items():
            v[name].append(sample(fn, calls[name]))
    for name in methods:
        res[name] = dict(kernel=kernels[name], **stats(v[name], calls[name]))
    fl = keep["stream64"][1]
    res["declined"] = int(((fl & 8) != 0).sum().item())
    res["flagged"] = int(((fl & 0xff) != 0).sum().item())
    deg = ((fl >> 8) & 0xff).cpu().numpy()
    res["degree_mean"], res["degree_max"] = float(deg.mean()), int(deg.max())
    if has_patch:
        res["flags_equal"] = bool(torch.equal(keep["patch64s"][1], fl))
        res["xa_equal_bit_for_bit"] = bool(torch.equal(keep["patch64s"][0], keep["stream64"][0]))
        res["ratio_stream64_over_patch64s"] = res["stream64"]["ms_median"] / res["patch64s"]["ms_median"]
    if "eig" in methods:
        ref = keep["eig"][0]
        res["rel_diff_eig_vs_stream64"] = float((torch.linalg.norm(ref - keep["stream64"][0]) / torch.linalg.norm(ref)).item())
        res["ratio_eig_over_stream64"] = res["eig"]["ms_median"] / res["stream64"]["ms_median"]
        if has_patch:
            res["ratio_eig_over_patch64s"] = res["eig"]["ms_median"] / res["patch64s"]["ms_median"]
    return res


def join(res, base):
    """The decision of LetkfEngine._patch64s_auto on the recorded samples: this build's row `res`, the parent build's `base`."""
    p, s = res.get("patch64s"), res["stream64"]
    res["parent_build"] = {n: base[n] for n in ("stream64", "eig") if n in base}
    bs = base["stream64"]
    res["stream64_builds_agree_within_spreads"] = bool(bs["ms_min"] <= s["ms_max"] and s["ms_min"] <= bs["ms_max"])
    res["ratio_stream64_this_over_parent"] = s["ms_median"] / bs["ms_median"]
    if p:
        res["ratio_parent_stream64_over_patch64s"] = bs["ms_median"] / p["ms_median"]
        res["ratio_parent_stream64_over_patch64s_worst_case"] = bs["ms_min"] / p["ms_max"]
        res["rule_patch64s_faster_than_parent_stream64_beyond_both_spreads"] = bool(p["ms_max"] < bs["ms_min"])
    return res


def child(spec, rounds, tree, timeout):
    """One case in a fresh process under its own time limit: (row, None) or (None, what failed)."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(rounds), "--tree", tree],
                           capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return None, dict(failed_case=spec, tree=tree, exit_status="time limit of %d s" % timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return None, dict(failed_case=spec, tree=tree, exit_status=r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--cases", help="semicolon-separated list in place of the default cases")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed (default: this one)")
    ap.add_argument("--parent-tree", help="a checkout of the parent commit, built: its rows are the baselines, timed case by case "
                                          "in front of this checkout's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, tree)))
        return 0
    results = []
    for spec in (a.cases.split(";") if a.cases else CASES):       # the first failure ends the run; one fresh process per case and build
        base = None
        if a.parent_tree:
            base, failed = child(spec, a.rounds, os.path.abspath(a.parent_tree), a.timeout)
            if failed:
                print(json.dumps(dict(failed, results=results)))
                return 1
        res, failed = child(spec, a.rounds, tree, a.timeout)
        if failed:
            print(json.dumps(dict(failed, results=results)))
            return 1
        if base is not None:
            join(res, base)
        results.append(res)
        print("%s: %s" % (spec, ", ".join("%s %s" % (n, res[n].get("ms_median", "refused")) for n in ("patch64s", "stream64", "eig") if n in res)),
              file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(json.dumps({"tool": TOOL, "baselines": "a build of the parent commit (--parent-tree)" if a.parent_tree else None,
                                     "rounds": a.rounds, "results": results}, indent=1) + "\n")
    print(json.dumps({"tool": TOOL, "results": results}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

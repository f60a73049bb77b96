#!/usr/bin/env python3
"""Float64 IEnKS update time of DENSE local networks (p_max > k), tau = 1, on 2-D MESHES: LetkfEngine.ienks_update with the map
of 4 x 4 patches (method="patch64": lienks_patch64_kernel, csrc/lienks_patch64.hip) against method="stream64" without a map
(lienks_stream64_kernel) and against the general kernel (method="eig": ienks_update_kernel<double, 256>) where it holds the
shape.  Sibling of tools/time_patch64w.py (the weights under a map: the same meshes) and tools/time_ienks_stream64.py (the 1-D
rows of this update); the protocol is theirs.

    python tools/time_ienks_patch64.py --out profiles/ienks_patch64_time.json      # every case below, one child process each
    python tools/time_ienks_patch64.py --case 80,3.0,316,bundle                     # one case (k, radius, mesh side, variant)
    python tools/time_ienks_patch64.py --tree ../parent --out parent.json           # the package of ANOTHER checkout (built there):
                                                                                    # the baselines on a build of the parent commit
    python tools/time_ienks_patch64.py --baseline parent.json --out profiles/ienks_patch64_time.json
                                                                                    # ... joined to this build's rows, with the decisions

Row-major ny x nx meshes with an observation at every point; seeded inputs, neighbour lists, packed records, the map and its
census built outside the timed region, W allocated once per case; the engine call WITH the 8-byte read of the decline counter
under device events, `rounds` samples per method, the methods ALTERNATING in one process (round r times every method once
before round r + 1), median and spread (max - min).  Bundle variant: per-point incoming weights (n, k, k) with Wp far from I
(every iteration of a loop looks like this); transform variant: ONE shared prior matrix (the first iteration).  The general
kernel is asked first: where it answers MIA_ERR_UNSUPPORTED the case records that.  A checkout without method="patch64" (the
parent commit) times the other two.  With --baseline the rows of the other build are joined per case and the two decisions of
LetkfEngine._ienks_patch64_auto are evaluated on the recorded samples, slowest sample of the route against the fastest of
the baseline: (a) patch64 <= stream64 of the PARENT build, (b) patch64 <= general kernel of the parent build / 2; and whether
stream64 agrees between the two builds within their spreads (its kernel is unchanged)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = "tools/time_ienks_patch64.py"
# (k, radius, mesh side, variant): 316 x 316 = 99 856 points; 224 x 224 = 50 176 at k = 128 (the shapes of tools/time_patch64w.py)
CASES = ["%s,%s" % (c, v) for c in ("40,3.0,316", "64,3.0,316", "80,3.0,316", "96,3.0,316", "128,3.5,224") for v in ("bundle", "transform")]
EPS = 1e-3


def stats(v):
    import numpy as np
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), spread_ms=float(v.max() - v.min()),
                rounds=[float(x) for x in v])


def one_case(spec, rounds, tree):
    import numpy as np
    import torch
    sys.path.insert(0, tree)
    import torch_assimilate_amd as mia
    from torch_assimilate_amd import _cabi
    mia.build()
    f = spec.split(",")
    k, c, side, variant = int(f[0]), float(f[1]), int(f[2]), f[3]
    ny = nx = side
    G = ny * nx
    dev = torch.device("cuda:0")
    eng = mia.LetkfEngine(dev)
    gen = torch.Generator(device="cpu").manual_seed(42)
    gy, gx = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=1)
    X = torch.randn((k, G), generator=gen, dtype=torch.float64).to(dev)
    y = torch.randn(G, generator=gen, dtype=torch.float64).to(dev)
    mean = X.mean(dim=0)
    bundle = variant == "bundle"
    eps = EPS if bundle else None
    Yb, d = ((X - mean) * (EPS if bundle else 1.0)).contiguous(), (y - mean).contiguous()      # (bundle: D = Yl / eps is the perturbations)
    del X
    nb = eng.localize(grid, grid, [c])
    rec = eng.pack_obs(Yb, d, torch.float64)
    if bundle:          # per-point weights, Wp far from I: I + 0.3 A / sqrt(k) + 0.1 m 1^T with a random row-centred A
        gen_d = torch.Generator(device=dev).manual_seed(43)          # (on the device: 7 GB of normal numbers at k = 96)
        w_in = torch.randn((G, k, k), generator=gen_d, dtype=torch.float64, device=dev)
        w_in -= w_in.mean(dim=2, keepdim=True)
        w_in *= 0.3 / k ** 0.5
        w_in += 0.1 * torch.randn((G, k, 1), generator=gen_d, dtype=torch.float64, device=dev)
        w_in += torch.eye(k, dtype=torch.float64, device=dev)
    else:
        w_in = torch.eye(k, dtype=torch.float64, device=dev)
    W = torch.empty((G, k, k), dtype=torch.float64, device=dev)
    has_patch = "patch64" in mia.LetkfEngine.IENKS_METHODS
    tiles = mia.mesh_tiles((ny, nx)) if has_patch else None

    def call(method, **kw):
        return eng.ienks_update(w_in, None, None, nb, 1.0, eps, rec=rec, return_flags=True, method=method, out=W, **kw)

    methods = {"stream64": lambda: call("stream64")}
    if has_patch:
        methods["patch64"] = lambda: call("patch64", tile_points=tiles)

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    res = {"case": dict(k=k, mesh=[ny, nx], radius=c, variant=variant, obs_stride=1, grid_points=G, p_max=int(nb.p_max),
                        weights_bytes=G * k * k * 8, incoming_weights="per point" if bundle else "one shared prior")}
    general_fits = bool(eng._ienks_general_fits(k, int(nb.p_max), 1.0, bundle))
    res["general_kernel_fits"] = general_fits
    if general_fits:
        methods["eig"] = lambda: call("eig")
    else:
        try:
            call("eig")
            raise AssertionError("the general kernel was expected to refuse the shape")
        except _cabi.MiaError as e:
            res["eig"] = dict(error="MiaError: %s" % e)
    if has_patch:       # the census: the first use of the map with these lists, its 8-byte read included
        res["census_ms"] = sample(lambda: eng._patch64_map(nb, tiles, None, k, 16))
        res["largest_patch_union"] = int(nb.tile_census[id(tiles)][2])
    kernels, keep = {}, {}
    for name, fn in methods.items():          # warm-up (table, code objects, clocks) and the results for the comparison
        r = fn()
        torch.cuda.synchronize()
        kernels[name] = _cabi.last_analysis_kernel()
        keep[name] = (r[0][:4096].clone(), r[1].clone())
    v = {name: [] for name in methods}
    for _ in range(rounds):                   # the methods alternate
        for name, fn in methods.items():
            v[name].append(sample(fn))
    for name in methods:
        res[name] = dict(kernel=kernels[name], **stats(v[name]))
    flags = keep["stream64"][1]
    res["declined"] = int(((flags & 8) != 0).sum().item())
    deg = ((flags >> 8) & 0xff).cpu().numpy()
    res["degree_mean"], res["degree_max"] = float(deg.mean()), int(deg.max())
    if has_patch:
        res["flags_equal"] = bool(torch.equal(keep["patch64"][1], flags))
        res["first_4096_points_equal"] = bool(torch.equal(keep["patch64"][0], keep["stream64"][0]))
        res["ratio_stream64_over_patch64"] = res["stream64"]["ms_median"] / res["patch64"]["ms_median"]
    if "eig" in methods:
        ref = keep["eig"][0]
        res["rel_diff_eig_vs_stream64_first_4096_points"] = float((torch.linalg.norm(ref - keep["stream64"][0]) / torch.linalg.norm(ref)).item())
    return res


def join(res, base):
    """The decisions of LetkfEngine._ienks_patch64_auto on the recorded samples: this build's row `res`, the parent build's `base`."""
    p, s = res.get("patch64"), res["stream64"]
    res["parent_build"] = {n: base[n] for n in ("stream64", "eig") if n in base}
    bs, be = base["stream64"], base.get("eig", {})
    res["stream64_builds_agree_within_spreads"] = bool(bs["ms_min"] <= s["ms_max"] and s["ms_min"] <= bs["ms_max"])
    res["ratio_stream64_this_over_parent"] = s["ms_median"] / bs["ms_median"]
    if p:
        res["ratio_parent_stream64_over_patch64"] = bs["ms_median"] / p["ms_median"]
        res["rule_a_patch64_no_slower_than_parent_stream64_beyond_both_spreads"] = bool(p["ms_max"] <= bs["ms_min"])
        if "ms_median" in be:
            res["ratio_parent_eig_over_patch64"] = be["ms_median"] / p["ms_median"]
            res["ratio_parent_eig_over_patch64_worst_case"] = be["ms_min"] / p["ms_max"]
            res["rule_b_twice_as_fast_as_parent_eig_beyond_both_spreads"] = bool(be["ms_min"] >= 2.0 * p["ms_max"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case")
    ap.add_argument("--cases", help="semicolon-separated list in place of the default cases")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed (default: this one)")
    ap.add_argument("--baseline", help="the --out file of a run on a build of the parent commit: joined per case")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=400)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if a.case:
        print(json.dumps(one_case(a.case, a.rounds, tree)))
        return 0
    base = {}
    if a.baseline:
        with open(a.baseline) as fh:
            for r in json.load(fh)["results"]:
                c = r["case"]
                base["%d,%s,%d,%s" % (c["k"], c["radius"], c["mesh"][0], c["variant"])] = r
    results = []
    for spec in (a.cases.split(";") if a.cases else CASES):       # the first failure ends the run; one fresh process per case
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", spec, "--rounds", str(a.rounds), "--tree", tree],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_case": spec, "exit_status": r.returncode, "results": results}))
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        if spec in base:
            join(res, base[spec])
        results.append(res)
        print("%s: %s" % (spec, ", ".join("%s %s" % (n, res[n].get("ms_median", "refused")) for n in ("patch64", "stream64", "eig") if n in res)),
              file=sys.stderr, flush=True)
        if a.out:                      # (kept up to date case by case)
            with open(a.out, "w") as fh:
                fh.write(json.dumps({"tool": TOOL, "build": "this checkout" if tree == ROOT else "another checkout (--tree)",
                                     "rounds": a.rounds, "results": results}, indent=1) + "\n")
    print(json.dumps({"tool": TOOL, "results": results}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Cost of cyclic coordinates on the step driver: the config-2-sized ring (G = 1e5 = L, k = 40, observations at every second
point, Gaspari-Cohn c = 10) through ShardedLetkf with PeriodicMetric's period against the same problem with the open metric,
timed with device events over blocks of steps, the two alternated in one process (2 000+ steps each by default); then the
Lorenz-96-sized ring (G = 40, k = 20, every point observed, c = 4).  Prints one JSON line.

    python tools/periodic_time.py [steps_per_block=500] [blocks=4]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                    # noqa: E402  (make_case: the benchmark's synthetic inputs on the device)
import torch_assimilate_amd as mia              # noqa: E402


def runner(args, c, period):
    r = mia.ShardedLetkf(torch.device("cuda:0"), 0, 1, radii=[c], inf_factor=1.1, period=period)
    for _ in range(3):                          # (first call: lists bound; then the native step)
        r.assimilate(*args)
    torch.cuda.synchronize()
    return r


def block_ms(r, args, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        r.assimilate(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    mia.build()
    dev = torch.device("cuda:0")
    G = 100000
    args = bench.make_case(G, 40, 2, dev, seed=42)
    runs = {"open": runner(args, 10.0, None), "periodic": runner(args, 10.0, [float(G)])}
    t = {"open": [], "periodic": []}
    for _ in range(blocks):
        for name in ("open", "periodic"):
            t[name].append(block_ms(runs[name], args, n))
    best = {k: min(v) for k, v in t.items()}
    l96 = bench.make_case(40, 20, 1, dev, seed=42)
    r96 = runner(l96, 4.0, [40.0])
    l96_ms = min(block_ms(r96, l96, n) for _ in range(blocks))
    print(json.dumps({"tool": "periodic_time", "steps_per_block": n, "blocks": blocks,
                      "config2_ring_ms_per_step": {"open": t["open"], "periodic": t["periodic"]},
                      "periodic_over_open": best["periodic"] / best["open"],
                      "lorenz96_ring_ms_per_step": l96_ms}))


if __name__ == "__main__":
    main()

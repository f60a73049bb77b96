"""Launch trace of the tile entries as a CPU test: the layer between the step driver (tests/test_step_call_trace.py) and the Python engine
(tests/test_engine_route_trace.py) -- a C entry, its cover check and its launch: which instantiation, which grid, which block, how many
LDS bytes.  Every source of the library is compiled HOST-ONLY at -O0 (tests/host_build.py: the kernels become launch stubs), linked
against the stand-in HIP runtime of tests/host_sanitize/hip_stub.cc with its call trace and its attribute trace switched on, and driven
by tests/host_sanitize/launch_trace_driver.cc -- one thread, a fixed list of calls, array arguments that are a few bytes of host memory.
Per call the output holds a header line with the entry and its sizes, every launch (kernel name with template arguments, grid, block,
LDS bytes, stream), every hipFuncSetAttribute (kernel name, bytes), and the return code with the string mia_last_analysis_kernel
returns afterwards; it is compared LINE FOR LINE with tests/golden/tile_launch_trace.txt.

The golden file records the behaviour of commit 2b75d77, the last one in which every tile kernel file carried its own copy of the frame
sizes, the grid rule and the launch: it was written by this test,
    MIA_TRACE_RECORD=1 python -m pytest tests/test_tile_launch_trace.py
in a checkout of that commit with nothing added but this test, tests/host_build.py, the driver and the attribute trace of the stub, and
is never regenerated from refactored code.  MIA_TRACE_RECORD is for the next intended change of what an entry launches, reviewed as a
diff of the golden file.  A recording run writes the file and then FAILS, so that it cannot be taken for a check.

What the calls cover (903 calls, 2 809 lines):
  float64 entries   the five analyses (matfun, patch, dense, wide, stream), the four weights entries, the three IEnKS updates, the RBF
                    entry and the kernel-expression entry with each of its three statistic sets, at ng = 203.  The full cross
                    k in {2, 15, 16, 17, 33, 40, 64, 65, 80, 96, 97, 113, 128, 129} x p_max in {0, 1, 8, 9, 24, 25, k - 1, k, k + 1,
                    2 k, 239, 240, 241, 256, 257} made a file too long to read and still left the middle row blocks of the dual
                    ladders out, so it is thinned to what decides a launch: k = 2 and every multiple of 16 up to 128 (one per number
                    of member blocks KT), p_max in {0, 9, 25, ..., 105} below k (one per number of row blocks
                    UT = ceil((p_max + 8) / 16)), k and k + 1 as p_max at the smallest and the largest k of an entry (both sides of
                    the dual / primal cover), 256 | 257 and 224 | 225 (the slots of the ring and of the resident image at k = 64),
                    the first k above an entry's cap (65 or 129), 64 | 65 as p_max of the kernelised entries.  Every instantiation a
                    ladder can reach appears -- 43 of 43 of each wide kernel, 13 of 13 of each 64-member kernel, 48 of 48 of
                    lketkf_tile64_kernel, 8 of 8 of each ring kernel, 4 of 4 of the dense and patch kernels -- and every kind of
                    refusal as -3
  the grid          every entry at one covered shape with ng in {1, 16, 17, 1 048 576, 1 048 577} (gx = 65536 with gy = 1, then 2); the
                    weights and IEnKS entries, which need no state, also at 16 * 65536 * 65535 points and one more: the last grid that
                    fits and the first that does not
  the map entries   union_blocks in {1, capacity, capacity + 1}, n_tiles in {1, 65536, 65537, 65536 * 65535, that + 1}
  the census        n_tiles over the same edges and the int32 bound
  options           every float64 entry with tile = 0 and with cheb_table = 0: -3 and no launch
  float32 entries   mia_letkf_analysis_matfun_f32 on the tile kernel (split and f32 products) and, with tile = 0, on each launch site of
                    letkf_cheb.hip (point, rows, weights, big); mia_letkf_analysis_packed_f32 / retry on letkf_sys_kernel; the tile-list
                    entries on letkf_tile2_kernel, letkf_tile2p_kernel (tile_pair), letkf_tile2w_kernel and lketkf_tile_kernel; the step
                    entry for letkf_tile2f_kernel and the segmented launches, which no other entry reaches"""
import os
import subprocess

import pytest

from host_build import HIPCC, ROOT, link_driver

GOLDEN = os.path.join(ROOT, "tests", "golden", "tile_launch_trace.txt")


def test_tile_launch_trace_matches_recorded(tmp_path):
    assert os.path.exists(HIPCC), "hipcc not found: the library cannot be built here either, and the launches must not go unchecked"
    exe = link_driver(str(tmp_path), "launch_trace_driver")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIA_")}
    runs = [subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300) for _ in range(2)]
    for res in runs:
        assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert runs[0].stdout == runs[1].stdout, "the trace differs between two runs of the same binary"
    got = runs[0].stdout.splitlines()
    if os.environ.get("MIA_TRACE_RECORD") == "1":
        with open(GOLDEN, "w") as fh:
            fh.write(runs[0].stdout)
        pytest.fail("recorded %d lines into %s: a recording run checks nothing -- run the test again without MIA_TRACE_RECORD" % (len(got), GOLDEN))
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            call = next((l for l in reversed(got[:i + 1]) if l.startswith("#")), "")
            pytest.fail("line %d differs (%s)\n  recorded: %s\n  now:      %s" % (i + 1, call, w, g))
    assert len(got) == len(want), "%d lines now, %d recorded" % (len(got), len(want))

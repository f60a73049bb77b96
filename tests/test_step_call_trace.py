"""Call trace of the step driver (csrc/sharded_step.hip, csrc/step_comm.hip) as a CPU test: every source of the library compiled
HOST-ONLY at -O0 without sanitizers (the kernels become launch stubs), linked against the stand-in HIP runtime of
tests/host_sanitize/hip_stub.cc with its call trace switched on, and driven by tests/host_sanitize/trace_driver.cc -- one caller
thread, a fixed list of scenarios.  The output (per C call: every kernel launch with its name and template arguments, grid, block,
LDS bytes, stream and carried events; event records and waits; asynchronous fills and copies; communicator callbacks; the return
code) is compared LINE FOR LINE with tests/golden/step_call_trace.txt.

The golden file records the behaviour of the commit BEFORE the driver was split into plan / prepare / analyse / redo / exchange
(070059a): it was written by this test's own build of that commit's csrc/, include/ and _build.py,
    MIA_TRACE_RECORD=1 python -m pytest tests/test_step_call_trace.py
in a copy of the tree with those three swapped in, and is never regenerated from refactored code.  MIA_TRACE_RECORD is for the next
intended change of what the driver launches, reviewed as a diff of the golden file.

Which scenario takes which route decision of the step (names as in the driver's StepPlan; "both ways" = the other scenarios):
  no_gather          partition communicator scenarios                     peer      direct peer exchange
  exch               custom communicator, 2 / 4 pieces                    lazy      NO_TILE_LISTS (on) / step_lazy_sort=0 (off)
  tl_route           default (on) / NO_TILE_LISTS, tile_lists=0, tile=0, method 1, TILE_EXTRA(7), P = 0, empty block (off)
  tl_rbf             gamma > 0, k = 40 (tile kernel) / k = 48 (outside it)
  tl_bucket          default (on) / SCAN_INDEX, bucket_index=0 (off)      want_fused / tl_fused   default (on) / tile_fused=0, KEEP_LISTS (off)
  tl_reuse           geometry epoch: second step (granted), third step after a radius change (refused: rebuilt)
  cnt_must_clear     first step on a workspace, step after a workspace release (on) / second step (off); cnt_use: consecutive steps
  carried            submitted steps with a preparation stream, step_hostwait=1 (on; timed and untimed) / step_hostwait=0, joined
                     step, no preparation stream, method 1, pieces (off)
  segmented          pieces + NO_TILE_LISTS (on) / segment_signal=0 (off)  tl_block  pieces on the tile route
  eig_only           method 1 (also the fallback to the eigensolver entry) zero_in_kernel  default (on) / P = 0, reused lists (off: fills)
  signal_mode        segment_signal 1 / 0                                  do1 / do2  submitted steps (stages 1 and 2) / synchronous (both)
  phase              every synchronous scenario runs phase 0 and then phase 1 (redo on the tile route, the lazy route, sorted lists)
  extra blocks       TILE_EXTRA(1), (2), (7)      ut >= 3                  p_max_assumed 40 with tile_pair 0 / 1
  placement          G = 4000 (four columns per lane) / 4001 (one); placement stream with MIA_STEP_NO_JOIN and without
The direct peer exchange is reachable: mia_comm_peer_attach maps a second communicator's buffers in-process, so peer_begin /
peer_finish, mia_comm_peer_exchange and mia_comm_peer_rewait appear in the trace.  The error returns close the list.  A recording run
writes the file and then FAILS, so that it cannot be taken for a check."""
import os
import subprocess

import pytest

from host_build import HIPCC, ROOT, link_driver

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_call_trace.txt")


def test_step_driver_call_trace_matches_recorded(tmp_path):
    assert os.path.exists(HIPCC), "hipcc not found: the library cannot be built here either, and the step driver must not go unchecked"
    exe = link_driver(str(tmp_path), "trace_driver")
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
            scenario = next((l for l in reversed(got[:i + 1]) if l.startswith("#")), "")
            pytest.fail("line %d differs (%s)\n  recorded: %s\n  now:      %s" % (i + 1, scenario, w, g))
    assert len(got) == len(want), "%d lines now, %d recorded" % (len(got), len(want))

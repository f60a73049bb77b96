"""The host-only build of the library that the call-trace tests share (tests/test_step_call_trace.py, tests/test_tile_launch_trace.py):
every source compiled with `hipcc --cuda-host-only` at -O0 without sanitizers, so that the kernels become launch stubs.  The objects are
built once per pytest process and linked with the stand-in HIP runtime of tests/host_sanitize/hip_stub.cc and one driver per test."""
import atexit
import importlib.util
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-assimilate_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "host_sanitize")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
COMMON = ["-O0", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
_objects = None      # (objects, fatbin_stub.cc) of this process


def host_objects():
    """tests/test_host_sanitizers.py's build without sanitizers, at -O0: one object per source and the stand-ins for their fat binaries."""
    global _objects
    if _objects is not None:
        return _objects
    tmp = tempfile.mkdtemp(prefix="mia_host_build_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    spec = importlib.util.spec_from_file_location("_mia_build", os.path.join(ROOT, "torch-assimilate_amd", "_build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)

    def cc(src):
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip"] + COMMON + bld.SOURCE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        return obj

    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex:
        objs = list(ex.map(cc, [os.path.join(CSRC, s) for s in bld.SOURCES]))
    nm = subprocess.run(["nm", "-u"] + objs, capture_output=True, text=True).stdout
    fat = sorted({l.split()[-1] for l in nm.splitlines() if "__hip_fatbin_" in l})
    stub = os.path.join(tmp, "fatbin_stub.cc")
    with open(stub, "w") as fh:
        fh.write("".join('extern "C" { extern const char %s[16]; const char %s[16] = {0}; }\n' % (s, s) for s in fat))
    _objects = (objs, stub)
    return _objects


def link_driver(tmp, driver):
    """The program of tests/host_sanitize/<driver>.cc over the host-only library and the stub runtime, in the directory tmp."""
    objs, stub = host_objects()
    exe = os.path.join(tmp, driver)
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")
    cmd = [HIPCC, "--cuda-host-only", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc] + COMMON + \
          [os.path.join(HERE, "hip_stub.cc"), os.path.join(HERE, driver + ".cc"), stub, "-x", "none"] + objs + ["-ldl", "-pthread", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe

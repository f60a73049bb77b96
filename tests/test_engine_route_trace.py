"""Route trace of the array-level host engine (torch-assimilate_amd/engine.py) as a CPU test: which C entries
``LetkfEngine.analysis``, ``weights64`` / ``weights_wide64`` / ``weights_stream64`` and ``ienks_update`` call, with which
arguments and in which order, what they return and what they raise -- for a fixed list of scenarios that reaches every branch
of the four method families, compared LINE FOR LINE with tests/golden/engine_route_trace.txt.  The pattern is
tests/test_step_call_trace.py's, one level up: there the C driver runs against a stand-in HIP runtime, here the Python engine
runs against a stand-in C library.

The engine without a GPU: ``LetkfEngine.__new__``, ``device`` = cpu, ``_ws`` = {}, ``_p_cap_hint``, ``_stream`` answering
c_void_p(0), ``_workspace`` without the 256-byte alignment assert, ``lib`` = the stand-in (which ``_cabi.lib`` answers too,
so that ``_cabi.check`` finds its status strings).

The stand-in library: every attribute is a callable that appends ``name(arg, ...)`` to the trace.  Scalars are printed as they
are; pointers as NULL, else as the name of the scenario's own tensor, else as a1, a2, ... in order of first appearance within
the scenario -- so aliasing between the first entry and the redo entry is visible.  It returns the status the scenario
programmes for that name (default 0; a ``*_cover`` function answers 1 unless programmed 0); where an entry that takes
``retry_count`` answers 0 it deposits the scenario's decline count at that address with ctypes, and the census entry deposits
the scenario's (fault bits, largest union).  After each engine call the trace gets the result's structure (types, shapes,
dtypes, the buffer's name, whether a trailing callable is present); the callable is invoked and what it does is traced; an
exception is traced with its type and full message.

The sweeps over (m, k, p_max) on both sides of every ``*_AUTO_*`` rule programme every tile entry to answer
MIA_ERR_UNSUPPORTED, so that one call walks the whole chain; their arguments differ in (m, k, p_max) only, which the scenario's
header names, so a sweep line keeps the NAMES of the entries called and drops the arguments (the other scenarios keep them).

The golden file records the behaviour of the commit BEFORE the host path of the float64 tile routes was folded (1f12109):
it was written by this test in a checkout of that commit with nothing but this file added,
    MIA_TRACE_RECORD=1 python -m pytest tests/test_engine_route_trace.py
and is never regenerated from refactored code.  MIA_TRACE_RECORD is for the next intended change of what the engine calls,
reviewed as a diff of the golden file.  A recording run writes the file and then FAILS, so that it cannot be taken for a check."""
import ctypes as C
import os

import pytest
import torch

from torch_assimilate_amd import _cabi
from torch_assimilate_amd.engine import LetkfEngine, NeighbourLists
from torch_assimilate_amd.interface import LETKF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_route_trace.txt")
F32, F64 = torch.float32, torch.float64
# where an entry takes retry_count, counted from the end of its argument list (include/mia_letkf.h)
RETRY_AT = {"mia_letkf_analysis_patch_f64": -5}
RETRY_AT.update({n: -2 for n in (
    "mia_letkf_analysis_matfun_f32", "mia_letkf_analysis_matfun_f64", "mia_letkf_analysis_dense_f64",
    "mia_letkf_analysis_wide_f64", "mia_letkf_analysis_stream_f64", "mia_lketkf_rbf_analysis_matfun_f64",
    "mia_lketkf_kernel_analysis_matfun_f64", "mia_letkf_weights_matfun_f32", "mia_letkf_weights_matfun_f64",
    "mia_letkf_weights_wide_f64", "mia_letkf_weights_stream_f64", "mia_lienks_update_matfun_f32",
    "mia_lienks_update_matfun_f64", "mia_lienks_update_wide_f64", "mia_lienks_update_stream_f64")})
TILE64 = ("mia_letkf_analysis_matfun_f64", "mia_letkf_analysis_patch_f64", "mia_letkf_analysis_dense_f64",
          "mia_letkf_analysis_wide_f64", "mia_letkf_analysis_stream_f64")
ALL_DECLINE = {n: -3 for n in TILE64 + ("mia_lketkf_rbf_analysis_matfun_f64", "mia_lketkf_kernel_analysis_matfun_f64")}
PROG = [(1, 0.5), (7, 2.0)]


class StandInLib:
    """The recording stand-in for the C library (see the module's docstring)."""

    def __init__(self):
        self.trace, self.names, self.anon = [], {}, {}
        self.rc, self.declines, self.census = {}, 0, (0, 0)

    def begin(self, label, tensors, rc=None, declines=0, census=(0, 0)):
        self.trace.append("# " + label)
        self.names = {t.data_ptr(): n for n, t in tensors.items() if isinstance(t, torch.Tensor) and t.data_ptr()}
        self.anon = {}
        self.rc, self.declines, self.census = dict(rc or {}), declines, census

    def ptr(self, addr):
        if not addr:
            return "NULL"
        if addr in self.names:
            return self.names[addr]
        return self.anon.setdefault(addr, "a%d" % (len(self.anon) + 1))

    def fmt(self, a):
        if a is None:
            return "NULL"
        if isinstance(a, C.c_void_p):
            return self.ptr(a.value)
        if isinstance(a, (bool, int, float)):
            return repr(a)
        if isinstance(a, C.Array) and a._type_ is _cabi.KernelOp:
            return "prog[" + ",".join("%d:%r" % (o.op, o.value) for o in a) + "]"
        return type(a).__name__

    def __getattr__(self, name):
        def call(*args):
            if name == "mia_status_string":
                return b"status %d" % args[0]
            if name == "mia_comm_last_error":
                return b""
            rc = self.rc.get(name, 1 if name.endswith("_cover") else 0)
            self.trace.append("%s(%s) = %d" % (name, ", ".join(self.fmt(a) for a in args), rc))
            if rc == 0 and name in RETRY_AT and args[RETRY_AT[name]] is not None and args[RETRY_AT[name]].value:
                C.c_int32.from_address(args[RETRY_AT[name]].value).value = self.declines
            if rc == 0 and name == "mia_letkf_tile_union_census":
                out2 = (C.c_int32 * 2).from_address(args[8].value)
                out2[0], out2[1] = self.census
            return rc
        return call


def make_engine(lib):
    eng = LetkfEngine.__new__(LetkfEngine)
    eng.lib, eng.device, eng._ws, eng._p_cap_hint = lib, torch.device("cpu"), {}, 32
    eng._stream = lambda: C.c_void_p(0)

    def workspace(tag, nbytes):
        cur = eng._ws.get(tag)
        if cur is None or cur.numel() < nbytes:
            cur = eng._ws[tag] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8)
        return cur
    eng._workspace = workspace
    return eng


def case(dtype, m, k, p_max, n=5, weights=None):
    """The scenario's own tensors: a shard [2, 2 + n) of a grid of n + 4 points, six observations."""
    g0, P, kp = 2, 6, (k + 1 + 3) // 4 * 4
    p_cap = max(8, (p_max + 7) // 8 * 8)
    t = dict(X=torch.zeros((m, k, n + 4), dtype=dtype), rec=torch.zeros((P, kp), dtype=dtype),
             cnt=torch.zeros(max(n, 1), dtype=torch.int32), idx=torch.zeros((max(n, 1), p_cap), dtype=torch.int32),
             w=torch.zeros((max(n, 1), p_cap), dtype=F64), Yb=torch.zeros((k, P), dtype=dtype), d=torch.zeros(P, dtype=dtype))
    if weights == "shared":
        t["weights"] = torch.zeros((k, k), dtype=dtype)
    elif weights == "points":
        t["weights"] = torch.zeros((n, k, k), dtype=dtype)
    t["nbrs"] = NeighbourLists(t["cnt"], t["idx"], t["w"], p_cap, p_max, g0, g0 + n)
    return t


def describe(lib, x):
    if isinstance(x, torch.Tensor):
        return "Tensor%s %s @%s" % (tuple(x.shape), str(x.dtype).replace("torch.", ""), lib.ptr(x.data_ptr()))
    if isinstance(x, tuple):
        return "(" + ", ".join(describe(lib, v) for v in x) + ")"
    if callable(x):
        return "callable"
    return repr(x)


def run(lib, fn, names_only=False):
    """One engine call: its C calls, its result's structure, the trailing callable invoked -- or its exception."""
    first = len(lib.trace)
    try:
        res = fn()
        lib.trace.append("-> " + describe(lib, res))
        last = res[-1] if isinstance(res, tuple) else res
        if callable(last) and not isinstance(last, torch.Tensor):
            lib.trace.append("finish() -> %r" % (last(),))
    except Exception as e:       # (traced: type and full message)
        lib.trace.append("!! %s: %s" % (type(e).__name__, e))
    if names_only:
        lines = lib.trace[first:]
        lib.trace[first - 1:] = [lib.trace[first - 1] + ": " + " | ".join(
            l.split("(")[0].replace("mia_", "") + l[l.rindex(" = "):] if l.startswith("mia_") else l for l in lines)]


def analysis_scenarios(lib, eng):
    def A(label, dtype=F64, m=1, k=20, p_max=20, n=5, rc=None, declines=0, census=(0, 40), own=(), src="rec", tiles=None,
          names_only=False, **kw):
        t = case(dtype, m, k, p_max, n)
        if "out" in own:
            t["out"] = kw["out"] = torch.zeros((m, k, n + 3), dtype=dtype)
            kw["out_offset"] = 2
        if "flags" in own:
            t["flags"] = kw["flags"] = torch.zeros(n, dtype=torch.int32)
        if "retry" in own:
            t["retry"] = kw["retry"] = torch.zeros(1, dtype=torch.int32)
        if tiles is not None:
            t["tile_points"] = kw["tile_points"] = tiles
        for name in ("rec", "Yb"):
            if name in kw:
                t[name] = kw.pop(name)
        lib.begin("analysis " + label, t, rc, declines, census)
        if src == "rec":
            run(lib, lambda: eng.analysis(t["X"], None, None, t["nbrs"], 1.1, rec=t["rec"], **kw), names_only)
        else:
            run(lib, lambda: eng.analysis(t["X"], t["Yb"], t["d"], t["nbrs"], 1.1, **kw), names_only)

    methods = ("auto", "eig", "matfun", "matfun64", "dense64", "patch64", "wide64", "stream64", "rbf64", "kern64")
    tiles = torch.full((1, 16), -1, dtype=torch.int32)
    tiles[0, :5] = torch.arange(5, dtype=torch.int32)
    # every method in both dtypes: plain core, then with rbf_gamma, then with a kernel program (psd and not)
    for dtype in (F32, F64):
        dn = "f32" if dtype == F32 else "f64"
        for meth in methods:
            A("%s %s plain" % (dn, meth), dtype, method=meth, tiles=tiles if meth == "patch64" else None)
            A("%s %s rbf_gamma" % (dn, meth), dtype, method=meth, rbf_gamma=0.5, return_flags=True)
        for meth in ("auto", "eig", "rbf64", "kern64", "matfun64"):
            A("%s %s program psd" % (dn, meth), dtype, method=meth, kernel_program=PROG, kernel_psd=True)
            A("%s %s program" % (dn, meth), dtype, method=meth, kernel_program=PROG)
    A("bad method", method="jacobi")
    A("patch64 without a map", method="patch64")
    A("program and gamma", kernel_program=PROG, rbf_gamma=0.5)
    A("int64 state", torch.int64)
    A("from Yb and d", src="Yb")
    A("from Yb and d f32 deferred", F32, src="Yb", defer_retry=True, declines=3)
    # return_weights: the float32 dual route, its -3, its redo; float64 stays on the Jacobi kernel; the named routes refuse
    A("f32 weights", F32, return_weights=True)
    A("f32 weights declines deferred flags", F32, return_weights=True, declines=3, defer_retry=True, return_flags=True)
    A("f32 weights outside", F32, return_weights=True, rc={"mia_letkf_weights_matfun_f32": -3}, return_flags=True)
    A("f32 weights error", F32, return_weights=True, rc={"mia_letkf_weights_matfun_f32": -2})
    A("f32 weights eig", F32, return_weights=True, method="eig", defer_retry=True)
    A("f32 weights matfun", F32, return_weights=True, method="matfun", rc={"mia_letkf_weights_matfun_f32": -3})
    A("f64 weights", return_weights=True, return_flags=True, defer_retry=True)
    for meth in ("matfun64", "rbf64", "kern64"):
        A("f64 weights " + meth, return_weights=True, method=meth, rbf_gamma=0.5 if meth == "rbf64" else None,
          kernel_program=PROG if meth == "kern64" else None, kernel_psd=True)
    # the float32 matfun route: outside the kernel, declines, another error
    A("f32 matfun outside", F32, rc={"mia_letkf_analysis_matfun_f32": -3})
    A("f32 matfun named outside", F32, method="matfun", rc={"mia_letkf_analysis_matfun_f32": -3})
    A("f32 matfun declines", F32, declines=3, return_flags=True)
    A("f32 matfun error", F32, rc={"mia_letkf_analysis_matfun_f32": -1})
    # caller-owned buffers, out with an offset, an empty shard
    A("own out flags retry", own=("out", "flags", "retry"), declines=3, return_flags=True)
    A("own out flags retry f32 deferred", F32, own=("out", "flags", "retry"), declines=3, defer_retry=True)
    A("wrong flags", flags=torch.zeros(4, dtype=torch.int32))
    A("rec of another ensemble", rec=torch.zeros((6, 28), dtype=F64))
    A("rec of another dtype", rec=torch.zeros((6, 24), dtype=F32))
    A("Yb of another ensemble", src="Yb", Yb=torch.zeros((24, 6), dtype=F64))
    for dtype in (F32, F64):
        A("n = 0 %s" % dtype, dtype, n=0, defer_retry=True, return_flags=True)
    A("n = 0 rbf64", n=0, method="rbf64", rbf_gamma=0.5)
    # status programmes of the float64 plain-core chain: first entry 0; -3 falling through each later entry in turn; all -3
    # (k 80 with p_max 100 lies inside every rule, so "auto" may go on to each of the five entries)
    chain = {"k 80 p 100": dict(k=80, p_max=100)}
    for cn, shape in chain.items():
        for stop in range(len(TILE64) + 1):
            rc = {n: -3 for n in TILE64[:stop]}
            A("chain %s stops at %d" % (cn, stop), rc=rc, declines=3 if stop % 2 else 0, defer_retry=stop == 2, tiles=tiles,
              return_flags=stop == 1, **shape)
    for meth, entry in zip(("matfun64", "patch64", "dense64", "wide64", "stream64"), TILE64):
        A("named %s outside" % meth, method=meth, rc=ALL_DECLINE, tiles=tiles, k=20, p_max=30)
        A("named %s error deferred" % meth, method=meth, rc={entry: -2}, tiles=tiles, k=20, p_max=30, defer_retry=True)
        A("named %s declines deferred" % meth, method=meth, declines=3, tiles=tiles, k=20, p_max=30, defer_retry=True)
    A("redo fails", declines=3, rc={"mia_letkf_analysis_retry_f64": -3})
    A("redo fails deferred", declines=3, rc={"mia_letkf_analysis_retry_f64": -3}, defer_retry=True, return_flags=True)
    A("jacobi fails", rc=dict(ALL_DECLINE, mia_letkf_analysis_packed_f64=-3))
    # patch64's extra steps: the cover, the census (counted and named blocks), unions that do not fit, an invalid map
    A("patch cover no", method="patch64", tiles=tiles, k=20, p_max=30, rc={"mia_letkf_patch_f64_cover": 0})
    A("patch auto cover no", tiles=tiles, k=20, p_max=30, rc={"mia_letkf_patch_f64_cover": 0, TILE64[0]: -3})
    A("patch union_blocks 3", method="patch64", tiles=tiles, k=20, p_max=30, union_blocks=3, rc={TILE64[0]: -3})
    A("patch union_blocks 0", method="patch64", tiles=tiles, k=20, p_max=30, union_blocks=0)
    A("patch auto unions too large", tiles=tiles, k=20, p_max=30, census=(0, 4000), rc={TILE64[0]: -3})
    A("patch named unions too large", method="patch64", tiles=tiles, k=20, p_max=30, census=(0, 4000))
    A("patch invalid map", method="patch64", tiles=tiles, k=20, p_max=30, census=(6, 0))
    A("patch census fails", method="patch64", tiles=tiles, k=20, p_max=30, rc={"mia_letkf_tile_union_census": -4})
    A("patch map of a wrong type", method="patch64", tiles=tiles.to(torch.int64), k=20, p_max=30)
    A("patch empty map", method="patch64", tiles=tiles[:0], k=20, p_max=30)
    A("patch auto more rows", m=2, tiles=tiles, k=20, p_max=30, rc={TILE64[0]: -3})
    # rbf64 and kern64: taken, outside (auto and named), declines, errors
    for meth in ("auto", "rbf64"):
        A("rbf64 %s taken declines" % meth, method=meth, rbf_gamma=0.5, declines=3, return_flags=True)
        A("rbf64 %s outside" % meth, method=meth, rbf_gamma=0.5, rc=ALL_DECLINE)
        A("rbf64 %s error deferred" % meth, method=meth, rbf_gamma=0.5, rc={"mia_lketkf_rbf_analysis_matfun_f64": -2},
          defer_retry=True)
        A("rbf64 %s deferred" % meth, method=meth, rbf_gamma=0.5, declines=3, defer_retry=True)
    for meth in ("auto", "kern64"):
        kw = dict(method=meth, kernel_program=PROG, kernel_psd=True)
        A("kern64 %s taken declines" % meth, declines=3, return_flags=True, **kw)
        A("kern64 %s outside" % meth, rc=ALL_DECLINE, **kw)
        A("kern64 %s error" % meth, rc={"mia_lketkf_kernel_analysis_matfun_f64": -2}, **kw)
        A("kern64 %s deferred own retry" % meth, declines=3, defer_retry=True, own=("retry", "out"), **kw)
        A("kern64 %s redo fails" % meth, declines=3, rc={"mia_lketkf_kernel_analysis_retry_f64": -3}, **kw)
    A("kern64 empty program", kernel_program=[], kernel_psd=True, defer_retry=True)
    A("kern64 f32 deferred", F32, kernel_program=PROG, kernel_psd=True, defer_retry=True, return_weights=True)
    # both sides of every auto rule: every tile entry declines, so one call walks the chain (names only)
    for m in (1, 8, 9):
        for k in (8, 20, 40, 64, 65, 97, 128):
            ps = sorted({k, k + 1, 12 * k // 5, 12 * k // 5 + 1, 101 * k // 40, 101 * k // 40 + 1, 173 * k // 80, 173 * k // 80 + 1})
            for p in ps:
                A("auto m %d k %d p %d" % (m, k, p), m=m, k=k, p_max=p, rc=ALL_DECLINE, names_only=True)
    for m in (1, 2):
        for k in (8, 19, 20, 40, 64, 65):
            for p in (k, k + 1, 101 * k // 40, 101 * k // 40 + 1):
                A("auto with a map m %d k %d p %d" % (m, k, p), m=m, k=k, p_max=p, rc=ALL_DECLINE, tiles=tiles, names_only=True)
    for m in (1, 2, 8, 9):
        for k in (7, 8, 40):
            for p in (20, 21, 22):
                A("auto rbf m %d k %d p %d" % (m, k, p), m=m, k=k, p_max=p, rc=ALL_DECLINE, rbf_gamma=0.5, names_only=True)
    for m in (1, 2):
        for k in (19, 20, 40):
            for p in (21, 22):
                A("auto program m %d k %d p %d" % (m, k, p), m=m, k=k, p_max=p, rc=ALL_DECLINE, kernel_program=PROG,
                  kernel_psd=True, names_only=True)


def weights_scenarios(lib, eng):
    for meth, entry in (("weights64", "mia_letkf_weights_matfun_f64"), ("weights_wide64", "mia_letkf_weights_wide_f64"),
                        ("weights_stream64", "mia_letkf_weights_stream_f64")):
        def Wt(label, dtype=F64, k=20, p_max=20, rc=None, declines=0, src="Yb", out=None, **kw):
            t = case(dtype, 1, k, p_max)
            if out is not None:
                t["out"] = kw["out"] = torch.zeros(out, dtype=F64)
            lib.begin("%s %s" % (meth, label), t, rc, declines)
            fn = getattr(eng, meth)
            if src == "Yb":
                run(lib, lambda: fn(t["Yb"], t["d"], t["nbrs"], 1.1, **kw))
            else:
                run(lib, lambda: fn(None, None, t["nbrs"], 1.1, rec=t["rec"], **kw))
        Wt("from Yb and d")
        Wt("from Yb and d flags", return_flags=True, rbf_gamma=0.5)
        Wt("from rec with out", src="rec", out=(5, 20, 20), declines=3)
        Wt("from rec without out", src="rec")
        Wt("from rec of another ensemble", src="rec", out=(5, 24, 24))
        Wt("float32 input", F32)
        Wt("float32 rec", F32, src="rec", out=(5, 20, 20))
        Wt("wrong out", out=(4, 20, 20))
        Wt("outside", rc={entry: -3})
        Wt("error", rc={entry: -2})
        Wt("declines", declines=3)
        Wt("declines twice the workspace", k=24, p_max=24, declines=3, return_flags=True)
        Wt("declines deferred", declines=3, defer_retry=True)
        Wt("deferred flags", defer_retry=True, return_flags=True)
        Wt("redo fails", declines=3, rc={"mia_letkf_weights_retry_f64": -3})


def ienks_scenarios(lib, eng):
    def I(label, dtype=F64, k=20, p_max=20, n=5, weights="shared", rc=None, declines=0, src="rec", own_out=False, **kw):
        t = case(dtype, 1, k, p_max, n, weights)
        if own_out:
            t["out"] = kw["out"] = torch.zeros((n, k, k), dtype=dtype)
        lib.begin("ienks_update " + label, t, rc, declines)
        if src == "rec":
            run(lib, lambda: eng.ienks_update(t["weights"], None, None, t["nbrs"], rec=t["rec"], **kw))
        else:
            run(lib, lambda: eng.ienks_update(t["weights"], t["Yb"], t["d"], t["nbrs"], **kw))

    covers = ("mia_lienks_update_f64_cover", "mia_lienks_update_wide_f64_cover", "mia_lienks_update_stream_f64_cover")
    entries = ("mia_lienks_update_matfun_f64", "mia_lienks_update_wide_f64", "mia_lienks_update_stream_f64")
    for dtype in (F32, F64):
        dn = "f32" if dtype == F32 else "f64"
        for meth in ("auto", "eig", "tile64", "wide64", "stream64"):
            for tau in (1.0, 0.5):
                for eps in (None, 0.5):
                    for wt in ("shared", "points"):
                        if meth not in ("auto", "eig") and (dtype == F32 or tau != 1.0) and (eps, wt) != (None, "shared"):
                            continue        # (the named tile methods refuse float32 and tau < 1 whatever the variant)
                        I("%s %s tau %g eps %s %s" % (dn, meth, tau, eps, wt), dtype, k=40, p_max=30, weights=wt, method=meth,
                          tau=tau, epsilon=eps)
    for k in (39, 40, 64, 65, 128):
        for cv in (0, 1):
            I("auto k %d covers %d" % (k, cv), k=k, p_max=30, rc={c: cv for c in covers})
        I("auto k %d tile cover 0 wide cover 1" % k, k=k, p_max=30, rc={covers[0]: 0})
        I("auto k %d general outside" % k, k=k, p_max=30, rc={"mia_lienks_update_f64": -3, covers[0]: 0}, declines=3,
          return_flags=True)
        I("auto k %d general outside wide cover 0" % k, k=k, p_max=30, rc={"mia_lienks_update_f64": -3, covers[0]: 0, covers[1]: 0})
        I("auto k %d general and wide outside" % k, k=k, p_max=30,
          rc={"mia_lienks_update_f64": -3, covers[0]: 0, entries[1]: -3})
        I("auto k %d tile entry outside" % k, k=k, p_max=30, rc={entries[0]: -3, entries[1]: -3})
    for meth, cover, entry in zip(("tile64", "wide64", "stream64"), covers, entries):
        I("%s cover 0" % meth, method=meth, rc={cover: 0})
        I("%s entry outside" % meth, method=meth, rc={entry: -3})
        I("%s entry error" % meth, method=meth, rc={entry: -2})
        I("%s declines flags" % meth, method=meth, declines=3, return_flags=True, epsilon=0.5, weights="points")
        I("%s declines deferred out" % meth, method=meth, declines=3, defer_retry=True, own_out=True)
        I("%s deferred flags" % meth, method=meth, defer_retry=True, return_flags=True)
        I("%s redo fails" % meth, method=meth, declines=3, rc={"mia_lienks_update_retry_f64": -3})
        I("%s n = 0" % meth, method=meth, n=0)
    I("f32 tau 1 declines", F32, declines=3, return_flags=True)
    I("f32 tau 1 outside", F32, rc={"mia_lienks_update_matfun_f32": -3}, return_flags=True)
    I("f32 tau 1 error", F32, rc={"mia_lienks_update_matfun_f32": -2})
    I("f32 n = 0", F32, n=0)
    I("general error", method="eig", rc={"mia_lienks_update_f64": -2})
    I("from Yb and d", src="Yb", own_out=True)
    I("bad method", method="jacobi")
    I("deferred under auto", defer_retry=True)
    I("bad tau", tau=1.5)
    I("bad epsilon", epsilon=0.0)
    I("bad out", out=torch.zeros((5, 20, 20), dtype=F32))
    t = case(F64, 1, 20, 20, 5, "points")
    lib.begin("ienks_update weights of another shard", t)
    run(lib, lambda: eng.ienks_update(t["weights"][:4], None, None, t["nbrs"], rec=t["rec"]))
    lib.begin("ienks_update rec of another ensemble", t)
    run(lib, lambda: eng.ienks_update(t["weights"][:, :16, :16], None, None, t["nbrs"], rec=t["rec"]))


def handover_scenarios(lib, eng):
    """LETKF._weights_on_tiles64 / _weights_on_wide64 / _weights_on_stream64 (interface.py): the gates in front of the three
    weights routes."""
    flt = LETKF.__new__(LETKF)
    flt._engine, flt._inf_factor, flt._kernel = eng, 1.1, None
    for meth, shapes in (("_weights_on_tiles64", ((39, 30), (40, 30))), ("_weights_on_wide64", ((64, 30), (65, 30))),
                         ("_weights_on_stream64", ((80, 100), (96, 120), (97, 120), (128, 256), (128, 257)))):
        for k, p_max in shapes:
            for dtype, gated in ((F64, True), (F64, False), (F32, True)):
                if meth == "_weights_on_tiles64" and not gated:
                    continue
                t = case(dtype, 1, k, p_max)
                lib.begin("%s k %d p %d %s%s" % (meth, k, p_max, str(dtype).replace("torch.", ""), "" if gated else " ungated"), t)
                fn = getattr(flt, meth)
                run(lib, (lambda: fn(t["Yb"], t["d"], t["nbrs"])) if gated else (lambda: fn(t["Yb"], t["d"], t["nbrs"], gated=False)),
                    names_only=True)
    t = case(F64, 1, 40, 30, n=0)
    lib.begin("_weights_on_tiles64 empty shard", t)
    run(lib, lambda: flt._weights_on_tiles64(t["Yb"], t["d"], t["nbrs"]), names_only=True)


def test_engine_route_trace_matches_recorded(monkeypatch):
    lib = StandInLib()
    monkeypatch.setattr(_cabi, "lib", lambda: lib)
    eng = make_engine(lib)
    analysis_scenarios(lib, eng)
    weights_scenarios(lib, eng)
    ienks_scenarios(lib, eng)
    handover_scenarios(lib, eng)
    got = lib.trace
    if os.environ.get("MIA_TRACE_RECORD") == "1":
        with open(GOLDEN, "w") as fh:
            fh.write("\n".join(got) + "\n")
        pytest.fail("recorded %d lines into %s: a recording run checks nothing -- run the test again without MIA_TRACE_RECORD" % (len(got), GOLDEN))
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            scenario = next((l for l in reversed(got[:i + 1]) if l.startswith("#")), "")
            pytest.fail("line %d differs (%s)\n  recorded: %s\n  now:      %s" % (i + 1, scenario, w, g))
    assert len(got) == len(want), "%d lines now, %d recorded" % (len(got), len(want))

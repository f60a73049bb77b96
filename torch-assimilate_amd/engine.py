"""Array-level host engine: torch-ROCm tensors in, torch-ROCm tensors out, every
floating-point operation of the hot path done by the gfx950 kernels behind the C ABI.

torch is plumbing here (device memory, streams); nothing in this file computes.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _cabi

__all__ = ["LetkfEngine", "NeighbourLists", "ObsIndex", "mesh_tiles"]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _one_of(names) -> str:
    """'a', 'b' or 'c' for an error message."""
    return ", ".join(repr(v) for v in names[:-1]) + " or " + repr(names[-1])


def _result(out, W, flags, finish, defer_retry):
    """What a route returns.  ``finish`` (None: no kernel that declines points ran) is the redo behind the decline counter: it
    runs now unless the caller defers it, and a deferring caller always gets a callable.  Then out [, W] [, flags] [, finish],
    each where it is not None, unwrapped when it is one object."""
    if not defer_retry:
        if finish is not None:
            finish()
        if W is None and flags is None:
            return out
        finish = None
    elif finish is None:
        finish = _nothing_declined
    res = tuple(v for v in (out, W, flags, finish) if v is not None)
    return res[0] if len(res) == 1 else res


def _nothing_declined() -> int:
    return 0


MIA_FLAG_NOCONV = 2     # include/mia_letkf.h
MIA_TILEMAP_FAULTS = ((1, "an entry outside [-1, n)"), (2, "a point that occurs more than once"),
                      (4, "a point that does not occur"))     # MIA_TILEMAP_* (include/mia_letkf.h)


def mesh_tiles(mesh_shape, g0: int = 0, g1: Optional[int] = None, patch=(4, 4)) -> torch.Tensor:
    """Tile map of a row-major ``(ny, nx)`` mesh for ``LetkfEngine.analysis(..., tile_points=...)``: one tile of sixteen slots
    per ``patch`` (4 x 4, 2 x 8 or 8 x 2 points: rows x columns) restricted to the points ``[g0, g1)`` of the mesh, int32
    ``(n_tiles, 16)`` on the host.  Slots are row-major inside the patch; an entry is the point's index relative to ``g0``, or
    -1 where the patch leaves the mesh or the shard.  Patches without a point of the shard are left out; tiles follow the
    patches row by row, so consecutive tiles are neighbours and share observations."""
    ny, nx = (int(v) for v in mesh_shape)
    py, px = (int(v) for v in patch)
    if ny < 1 or nx < 1:
        raise ValueError("mesh_shape must be (ny, nx) with positive sizes")
    if py < 1 or px < 1 or py * px != 16:
        raise ValueError("patch must have sixteen points: (4, 4), (2, 8), (8, 2), ...")
    G = ny * nx
    g1 = G if g1 is None else int(g1)
    g0 = int(g0)
    if not 0 <= g0 <= g1 <= G:
        raise ValueError("[g0, g1) must lie inside the mesh")
    if g0 == g1:
        return torch.empty((0, 16), dtype=torch.int32)
    ty, tx = (ny + py - 1) // py, (nx + px - 1) // px
    row = torch.arange(ty)[:, None, None, None] * py + torch.arange(py)[None, None, :, None]      # (ty, 1, py, 1)
    col = torch.arange(tx)[None, :, None, None] * px + torch.arange(px)[None, None, None, :]      # (1, tx, 1, px)
    pt = (row * nx + col).reshape(ty * tx, 16)
    ok = ((row < ny) & (col < nx)).reshape(ty * tx, 16) & (pt >= g0) & (pt < g1)
    tiles = torch.where(ok, pt - g0, torch.full_like(pt, -1))
    return tiles[ok.any(dim=1)].to(torch.int32).contiguous()


def _read_solve_flags(flags: torch.Tensor) -> int:
    """The flag word of a global solve (etkf_weights / ketkf_weights with return_flags=True) on the host: one sync."""
    return int(flags[0].item())


def warn_if_noconv(flags: torch.Tensor, what: str) -> None:
    """RuntimeWarning when a global solve's eigensolver reached its sweep cap (its weights are still returned)."""
    if _read_solve_flags(flags) & MIA_FLAG_NOCONV:
        warnings.warn(what + " eigensolver reached its sweep cap (result returned)", RuntimeWarning)


@dataclass
class NeighbourLists:
    """Per-grid-point local observation lists of one shard [g0, g1)."""
    cnt: torch.Tensor      # (n,) int32
    idx: torch.Tensor      # (n, p_cap) int32, -1 padded
    w: torch.Tensor        # (n, p_cap) float64, sqrt(Gaspari-Cohn weight)
    p_cap: int
    p_max: int
    g0: int
    g1: int
    stats: Optional[torch.Tensor] = None   # device [max count, #truncated]; set when the read-back was deferred
    observed_p_max: Optional[int] = None
    tile_census: Optional[dict] = None     # id(tile map) -> (the map, its device copy, largest union or None): LetkfEngine.analysis

    def confirm(self) -> bool:
        """Deferred check of an assumed ``p_max`` (host sync): True when every list fitted."""
        if self.stats is None:
            return True
        p_max, n_over = (int(v) for v in self.stats.tolist())
        self.observed_p_max = p_max
        ok = n_over == 0 and p_max <= self.p_max
        if ok:
            self.stats = None
        return ok


class TileLists:
    """Tile-shaped lists of grid points [g0, g1) (csrc/mia_tiles.h): device buffer + the bound they were sized for."""

    def __init__(self, lists, p_max, g0, g1, stats, extra_blocks=0):
        self.lists, self.p_max, self.g0, self.g1, self.stats, self.extra_blocks = lists, p_max, g0, g1, stats, extra_blocks

    @property
    def ut(self):
        return max(1, (self.p_max + 8 + 15) // 16) + self.extra_blocks

    def unpack(self):
        """host view for tests: (hdr [ntile, 4], uidx [ntile, 16 ut], D [ntile, ut, 64, 4])"""
        import numpy as np
        n = self.g1 - self.g0
        ntile, ut = (n + 15) // 16, self.ut
        raw = self.lists.cpu().numpy()

        def up(x):
            return (x + 255) // 256 * 256
        o_idx = up(max(ntile, 1) * 16)
        o_d = o_idx + up(max(ntile, 1) * 16 * ut * 4)
        hdr = raw[:ntile * 16].view(np.int32).reshape(ntile, 4)
        uidx = raw[o_idx:o_idx + ntile * 16 * ut * 4].view(np.int32).reshape(ntile, 16 * ut)
        D = raw[o_d:o_d + ntile * ut * 1024].view(np.float32).reshape(ntile, ut, 64, 4)
        return hdr, uidx, D


@dataclass
class ObsIndex:
    """Cell index of one observation set for one localisation (built by mia_letkf_index_build_f64)."""
    ws: torch.Tensor
    obs: torch.Tensor          # (P, nc) float64, kept alive: the index refers to it
    radii: list
    coord_group: list
    P: int
    nc: int
    period: Optional[list] = None      # cyclic coordinates (> 0) the index was built for; None = open


def _periods(period, nc: int):
    """The period argument of the localisation calls as a ctypes array (None: every coordinate open, the plain C entries)."""
    if period is None:
        return None
    per = [0.0 if p is None else float(p) for p in (period if hasattr(period, "__len__") else [period] * nc)]
    if len(per) != nc:
        raise ValueError("period needs one entry per coordinate")
    if any(not (p >= 0.0 and p < float("inf")) for p in per):
        raise ValueError("period must be finite and >= 0")
    if not any(p > 0.0 for p in per):
        return None
    return (C.c_double * nc)(*per)


def _period_arg(per, nc: int):
    """What the periodic C entries take for ``_periods``' result: the array itself, or all zeros (= the open entry) for None."""
    return per if per is not None else (C.c_double * nc)()


class LetkfEngine:
    """One engine per process / GPU.  All work is enqueued on the current torch stream of
    ``device``; results are ordinary device tensors."""

    def __init__(self, device: Optional[torch.device] = None):
        self.lib = _cabi.lib()
        if not torch.cuda.is_available():
            raise _cabi.MiaError("no MI355X visible: the LETKF hot path has no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self._ws = {}
        self._p_cap_hint = 32

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, tag: str, nbytes: int) -> torch.Tensor:
        cur = self._ws.get(tag)
        if cur is None or cur.numel() < nbytes:
            cur = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
            assert cur.data_ptr() % 256 == 0
            self._ws[tag] = cur
        return cur

    def _dev(self, a, dtype):
        t = torch.as_tensor(a)
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _redo_behind_counter(self, retry: torch.Tensor, entry: str, redo_args, alive=()):
        """The ``finish`` callable of a route whose kernel may decline points: it reads the decline counter ``retry`` (8 bytes,
        synchronising) and, where points were declined, calls the redo ``entry`` with ``redo_args()`` and the stream; it returns
        the number of points redone.  The arguments are addresses: ``alive`` holds the arrays behind them until a deferred
        redo has run."""
        def finish(_alive=alive):
            n_retry = int(retry.item())          # host sync (8 bytes)
            if n_retry:
                _cabi.check(getattr(self.lib, entry)(*redo_args(), self._stream()), entry)
            return n_retry
        return finish

    # ------------------------------------------------------------ localisation
    def gaspari_cohn(self, r: torch.Tensor, taper: int = 0) -> torch.Tensor:
        """Taper of normalised distances: taper 0 = GaspariCohn, 1 = GaspariCohnInf (MIA_TAPER_*)."""
        r = r.to(self.device).contiguous()
        out = torch.empty_like(r)
        name = "mia_gaspari_cohn_" + ("inf_" if taper else "") + {torch.float64: "f64", torch.float32: "f32"}[r.dtype]
        fn = getattr(self.lib, name)
        _cabi.check(fn(_ptr(r), r.numel(), _ptr(out), self._stream()), "mia_gaspari_cohn")
        return out

    def localize(self, grid_xyz, obs_xyz, radii: Sequence[float], coord_group: Optional[Sequence[int]] = None,
                 eps: float = 1e-5, g0: int = 0, g1: Optional[int] = None,
                 p_cap: Optional[int] = None, assume_p_max: Optional[int] = None,
                 stats_out: Optional[torch.Tensor] = None, taper: int = 0, period=None) -> NeighbourLists:
        """Neighbour lists of grid points [g0, g1).  By default the maximum list length is read back
        (one 8-byte host sync) to size the analysis launch.  With ``assume_p_max`` (e.g. the value of the
        previous cycle on the same geometry) nothing is read back here: the returned lists carry the
        assumption and ``NeighbourLists.confirm()`` checks it later, e.g. after the analysis has been
        enqueued; the analysis kernel itself flags any point whose list does not fit (never truncates).  ``period``: one entry per
        coordinate (or a scalar), > 0 = cyclic coordinate with that period (PeriodicMetric), 0 / None = open."""
        grid = self._dev(grid_xyz, torch.float64)
        obs = self._dev(obs_xyz, torch.float64)
        if grid.dim() == 1:
            grid = grid[:, None].contiguous()
        if obs.dim() == 1:
            obs = obs[:, None].contiguous()
        G, nc = grid.shape
        P = obs.shape[0]
        if P and obs.shape[1] != nc:
            raise ValueError("grid and observation coordinates differ in dimensionality")
        g1 = G if g1 is None else g1
        n = g1 - g0
        radii = [float(r) for r in (radii if hasattr(radii, "__len__") else [radii])]
        n_r = len(radii)
        coord_group = [0] * nc if coord_group is None else [int(c) for c in coord_group]
        if len(coord_group) != nc:
            raise ValueError("coord_group needs one entry per coordinate")
        cg = (C.c_int32 * nc)(*coord_group)
        rc = (C.c_double * n_r)(*radii)
        per = _period_arg(_periods(period, nc), nc)

        def call(cap, cnt, idx, w):
            return self.lib.mia_letkf_localize_taper_periodic_f64(
                int(taper), _ptr(grid), g0, g1, _ptr(obs), P, nc, cg, per, rc, n_r, float(eps), cap,
                _ptr(cnt), _ptr(idx), _ptr(w), _ptr(stats), _ptr(ws), ws.numel(), self._stream())
        nbytes = C.c_size_t(0)
        _cabi.check(self.lib.mia_letkf_localize_workspace_bytes(P, nc, C.byref(nbytes)), "localize_workspace_bytes")
        ws = self._workspace("loc", nbytes.value)
        stats = stats_out if stats_out is not None else torch.empty(2, dtype=torch.int32, device=self.device)
        cap = int(p_cap) if p_cap is not None else self._p_cap_hint
        if assume_p_max is not None:
            cap = max(8, (int(assume_p_max) + 7) // 8 * 8)
            cnt = torch.empty(n, dtype=torch.int32, device=self.device)
            idx = torch.empty((n, cap), dtype=torch.int32, device=self.device)
            w = torch.empty((n, cap), dtype=torch.float64, device=self.device)
            _cabi.check(call(cap, cnt, idx, w), "mia_letkf_localize_taper_periodic_f64")
            return NeighbourLists(cnt, idx, w, cap, int(assume_p_max), g0, g1, stats)
        while True:
            cnt = torch.empty(n, dtype=torch.int32, device=self.device)
            idx = torch.empty((n, cap), dtype=torch.int32, device=self.device)
            w = torch.empty((n, cap), dtype=torch.float64, device=self.device)
            _cabi.check(call(cap, cnt, idx, w), "mia_letkf_localize_taper_periodic_f64")
            p_max, n_over = (int(v) for v in stats.tolist())   # host sync: sizes the analysis launch
            if n_over == 0:
                break
            cap = (p_max + 7) // 8 * 8          # lists were truncated: retry with room for all
        self._p_cap_hint = max(8, (p_max + 7) // 8 * 8)
        return NeighbourLists(cnt, idx, w, cap, p_max, g0, g1)

    # ------------------------------------------------------------ tile route (round 3)
    def localize_tiles(self, grid_xyz, obs_xyz, radii: Sequence[float], p_max: int,
                       coord_group: Optional[Sequence[int]] = None, eps: float = 1e-5, g0: int = 0,
                       g1: Optional[int] = None, taper: int = 0, extra_blocks: int = 0, period=None) -> "TileLists":
        """Tile lists of grid points [g0, g1) (mia_letkf_localize_tiles_f64): per tile of sixteen points the union of
        their Gaspari-Cohn lists and the sqrt(weight) matrix, in the analysis kernel's register layout.  ``p_max`` bounds
        the local observations of a point (e.g. ``NeighbourLists.p_max`` of an earlier call on the geometry),
        ``extra_blocks`` adds sixteen slots each to what a tile's union may hold; the returned object's ``stats`` holds
        [longest list, tiles whose union did not fit] on the device.  ``period`` as ``localize``."""
        grid = self._dev(grid_xyz, torch.float64)
        obs = self._dev(obs_xyz, torch.float64)
        if grid.dim() == 1:
            grid = grid[:, None].contiguous()
        if obs.dim() == 1:
            obs = obs[:, None].contiguous()
        G, nc = grid.shape
        P = obs.shape[0]
        if P and obs.shape[1] != nc:
            raise ValueError("grid and observation coordinates differ in dimensionality")
        g1 = G if g1 is None else g1
        radii = [float(r) for r in (radii if hasattr(radii, "__len__") else [radii])]
        coord_group = [0] * nc if coord_group is None else [int(c) for c in coord_group]
        cg = (C.c_int32 * nc)(*coord_group)
        rc = (C.c_double * len(radii))(*radii)
        nbytes = C.c_size_t(0)
        _cabi.check(self.lib.mia_letkf_localize_workspace_bytes(P, nc, C.byref(nbytes)), "localize_workspace_bytes")
        ws = self._workspace("loc", nbytes.value)
        tb = C.c_size_t(0)
        _cabi.check(self.lib.mia_letkf_tile_lists_bytes(g1 - g0, int(p_max), int(extra_blocks), C.byref(tb)),
                    "mia_letkf_tile_lists_bytes")
        lists = torch.empty(max(tb.value, 256), dtype=torch.uint8, device=self.device)
        stats = torch.zeros(2, dtype=torch.int32, device=self.device)
        per = _period_arg(_periods(period, nc), nc)
        _cabi.check(self.lib.mia_letkf_localize_tiles_periodic_f64(
            int(taper), _ptr(grid), g0, g1, _ptr(obs), P, nc, cg, per, rc, len(radii), float(eps), int(p_max),
            int(extra_blocks), _ptr(lists), lists.numel(), _ptr(stats), _ptr(ws), ws.numel(), self._stream()),
            "mia_letkf_localize_tiles_periodic_f64")
        return TileLists(lists, int(p_max), g0, g1, stats, int(extra_blocks))

    def pack_split(self, Yb: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
        """[k][P] perturbations + d[P] -> (P + 1) split records (uint8 tensor; mia_letkf_pack_split_f32)."""
        Yb = Yb.to(device=self.device, dtype=torch.float32).contiguous()
        d = d.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        k, P = Yb.shape
        rb = C.c_size_t(0)
        _cabi.check(self.lib.mia_letkf_split_record_bytes(k, C.byref(rb)), "mia_letkf_split_record_bytes")
        rec = torch.empty(((P + 1) * rb.value,), dtype=torch.uint8, device=self.device)
        _cabi.check(self.lib.mia_letkf_pack_split_f32(_ptr(Yb), _ptr(d), k, P, _ptr(rec), self._stream()),
                    "mia_letkf_pack_split_f32")
        return rec

    def analysis_tiles(self, X: torch.Tensor, split_rec: torch.Tensor, P: int, tiles: "TileLists", inf_factor: float = 1.0,
                       out: Optional[torch.Tensor] = None):
        """Analysis of the tile lists' grid points from split records (mia_letkf_analysis_tiles_f32).  Returns
        (Xa [m, k, g1 - g0], flags int32 [g1 - g0], retry_count int32 [1]); declined points carry MIA_FLAG_RETRY."""
        X = X.to(device=self.device, dtype=torch.float32).contiguous()
        m, k, G = X.shape
        n = tiles.g1 - tiles.g0
        xa = out if out is not None else torch.empty((m, k, n), dtype=torch.float32, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        retry = torch.zeros(1, dtype=torch.int32, device=self.device)
        _cabi.check(self.lib.mia_letkf_analysis_tiles_f32(
            _ptr(X), G, m, k, tiles.g0, tiles.g1, _ptr(split_rec), int(P), _ptr(tiles.lists), tiles.p_max, tiles.extra_blocks,
            float(inf_factor), _ptr(xa), xa.shape[-1], 0, _ptr(flags), _ptr(retry), self._stream()),
            "mia_letkf_analysis_tiles_f32")
        return xa, flags[:n], retry

    def analysis_tiles_rbf(self, X: torch.Tensor, Yb: torch.Tensor, d: torch.Tensor, tiles: "TileLists", inf_factor: float,
                           rbf_gamma: float, out: Optional[torch.Tensor] = None):
        """RBF-kernelised analysis (KETKFModule + RBFKernel(gamma), core/ketkf.py:65-94) of the tile lists' grid points from the
        float32 perturbations themselves (mia_lketkf_rbf_analysis_tiles_f32).  Returns (Xa [m, k, n], flags [n], retry_count [1])
        or None when the shape is outside the kernel (k > 40, unions of more than 64 slots)."""
        X = X.to(device=self.device, dtype=torch.float32).contiguous()
        Yb = Yb.to(device=self.device, dtype=torch.float32).contiguous()
        d = d.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        m, k, G = X.shape
        n = tiles.g1 - tiles.g0
        xa = out if out is not None else torch.empty((m, k, n), dtype=torch.float32, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        retry = torch.zeros(1, dtype=torch.int32, device=self.device)
        rc = self.lib.mia_lketkf_rbf_analysis_tiles_f32(
            _ptr(X), G, m, k, tiles.g0, tiles.g1, _ptr(Yb), _ptr(d), Yb.shape[1], _ptr(tiles.lists), tiles.p_max,
            tiles.extra_blocks, float(inf_factor), float(rbf_gamma), _ptr(xa), xa.shape[-1], 0, _ptr(flags), _ptr(retry),
            self._stream())
        if rc == -3:
            return None
        _cabi.check(rc, "mia_lketkf_rbf_analysis_tiles_f32")
        return xa, flags[:n], retry

    def weights_tiles(self, X: torch.Tensor, split_rec: torch.Tensor, P: int, tiles: "TileLists", inf_factor: float = 1.0):
        """Analysis + weights of the tile lists' grid points (mia_letkf_weights_tiles_f32).  Returns (Xa [m, k, n], W [n, k, k],
        flags [n], retry_count [1]) or None when the shape is outside the kernel (unions of more than 32 slots)."""
        X = X.to(device=self.device, dtype=torch.float32).contiguous()
        m, k, G = X.shape
        n = tiles.g1 - tiles.g0
        xa = torch.empty((m, k, n), dtype=torch.float32, device=self.device)
        W = torch.empty((n, k, k), dtype=torch.float32, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        retry = torch.zeros(1, dtype=torch.int32, device=self.device)
        rc = self.lib.mia_letkf_weights_tiles_f32(
            _ptr(X), G, m, k, tiles.g0, tiles.g1, _ptr(split_rec), int(P), _ptr(tiles.lists), tiles.p_max, tiles.extra_blocks,
            float(inf_factor), _ptr(xa), xa.shape[-1], 0, _ptr(W), _ptr(flags), _ptr(retry), self._stream())
        if rc == -3:
            return None
        _cabi.check(rc, "mia_letkf_weights_tiles_f32")
        return xa, W, flags[:n], retry

    def weights_retry(self, X: torch.Tensor, Yb: torch.Tensor, d: torch.Tensor, nbrs: NeighbourLists, inf_factor: float,
                      out: torch.Tensor, W: torch.Tensor, flags: torch.Tensor):
        """Eigensolver redo (analysis + weights) of the points flagged MIA_FLAG_RETRY (mia_letkf_weights_retry_f32)."""
        X = X.to(device=self.device, dtype=torch.float32).contiguous()
        m, k, G = X.shape
        rec = self.pack_obs(Yb, d, torch.float32)
        _cabi.check(self.lib.mia_letkf_weights_retry_f32(
            _ptr(X), G, m, k, nbrs.g0, nbrs.g1, _ptr(rec), rec.shape[0], _ptr(nbrs.cnt), _ptr(nbrs.idx), _ptr(nbrs.w),
            nbrs.p_cap, nbrs.p_max, float(inf_factor), 0.0, _ptr(out), out.shape[-1], 0, _ptr(W), _ptr(flags), self._stream()),
            "mia_letkf_weights_retry_f32")

    def tile_route_applies(self, X: torch.Tensor, p_max: int, extra_blocks: int = 0, rbf_gamma=None, method: str = "auto",
                           P: int = 1, n_points: Optional[int] = None, ldo: Optional[int] = None) -> bool:
        """Whether the tile route (tile lists + csrc/letkf_tile2.hip, or csrc/lketkf_tile.hip for the RBF-kernelised filter)
        takes this analysis: float32, route options on, and the shape test the C side applies before launching
        (mia_letkf_tiles_cover: ensemble size, slots of a tile's union, LDS, 32-bit byte offsets)."""
        if X.dtype != torch.float32 or method == "eig" or X.dim() != 3:
            return False
        v = C.c_int(0)
        for name in (b"tile", b"tile_lists") + (() if rbf_gamma is not None else (b"tile_split",)):
            self.lib.mia_get_option(name, C.byref(v))
            if not v.value:
                return False
        m, k, G = X.shape
        n = G if n_points is None else int(n_points)
        return bool(self.lib.mia_letkf_tiles_cover(m, k, int(p_max), int(extra_blocks), G, n if ldo is None else int(ldo), n, int(P),
                                                   float(rbf_gamma) if rbf_gamma is not None else 0.0))

    def retry_points(self, X: torch.Tensor, Yb: torch.Tensor, d: torch.Tensor, nbrs: NeighbourLists, inf_factor: float,
                     out: torch.Tensor, flags: torch.Tensor, out_offset: int = 0, rbf_gamma: Optional[float] = None):
        """Eigensolver redo of the grid points flagged MIA_FLAG_RETRY (mia_letkf_analysis_retry_f32) from per-point lists."""
        X = X.to(device=self.device, dtype=torch.float32).contiguous()
        m, k, G = X.shape
        rec = self.pack_obs(Yb, d, torch.float32)
        _cabi.check(self.lib.mia_letkf_analysis_retry_f32(
            _ptr(X), G, m, k, nbrs.g0, nbrs.g1, _ptr(rec), rec.shape[0], _ptr(nbrs.cnt), _ptr(nbrs.idx), _ptr(nbrs.w),
            nbrs.p_cap, nbrs.p_max, float(inf_factor), float(rbf_gamma) if rbf_gamma is not None else 0.0, _ptr(out), out.shape[-1],
            out_offset, _ptr(flags), self._stream()), "mia_letkf_analysis_retry_f32")

    def build_index(self, obs_xyz, radii: Sequence[float], coord_group: Optional[Sequence[int]] = None, period=None) -> ObsIndex:
        """Bin the observations into the uniform cell grid used by the fused-localisation analysis (``period`` as ``localize``;
        ``analysis_fused`` itself takes open indexes only)."""
        obs = self._dev(obs_xyz, torch.float64)
        if obs.dim() == 1:
            obs = obs[:, None].contiguous()
        P, nc = obs.shape
        radii = [float(r) for r in (radii if hasattr(radii, "__len__") else [radii])]
        coord_group = [0] * nc if coord_group is None else [int(c) for c in coord_group]
        nbytes = C.c_size_t(0)
        _cabi.check(self.lib.mia_letkf_localize_workspace_bytes(P, nc, C.byref(nbytes)), "localize_workspace_bytes")
        ws = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=self.device)
        cg = (C.c_int32 * nc)(*coord_group)
        rc = (C.c_double * len(radii))(*radii)
        per = _periods(period, nc)
        _cabi.check(self.lib.mia_letkf_index_build_periodic_f64(_ptr(obs), P, nc, cg, _period_arg(per, nc), rc, len(radii), _ptr(ws),
                                                                ws.numel(), self._stream()), "mia_letkf_index_build_periodic_f64")
        return ObsIndex(ws, obs, radii, coord_group, P, nc, None if per is None else list(per))

    def analysis_fused(self, X: torch.Tensor, rec: torch.Tensor, grid_xyz, index: ObsIndex, p_max_assumed: int,
                       inf_factor: float = 1.0, eps: float = 1e-5, rbf_gamma: Optional[float] = None,
                       g0: int = 0, g1: Optional[int] = None):
        """matfun analysis with the localisation fused into the kernel (no neighbour lists).  Returns
        (Xa (m, k, n), flags, finish); ``finish()`` performs the single host sync of the step and returns
        (ok, observed p_max, declined points): ok False means some grid point has more local observations
        than assumed and the shard must be redone (list route); declined points are redone by the
        eigensolver kernel inside ``finish``."""
        if X.dim() == 2:
            X = X[None]
        X = X.to(self.device).contiguous()
        if X.dtype != torch.float32 or rec.dtype != torch.float32:
            raise TypeError("the fused matfun route is float32 only")
        if index.period is not None:
            raise _cabi.MiaError("the fused per-point route takes open coordinates: cyclic ones go through localize() or the step driver")
        m, k, G = X.shape
        grid = self._dev(grid_xyz, torch.float64)
        if grid.dim() == 1:
            grid = grid[:, None].contiguous()
        g1 = G if g1 is None else g1
        n = g1 - g0
        out = torch.empty((m, k, n), dtype=torch.float32, device=self.device)
        flags = torch.empty(n, dtype=torch.int32, device=self.device)
        retry = torch.zeros(1, dtype=torch.int32, device=self.device)
        stats = torch.empty(2, dtype=torch.int32, device=self.device)
        cg = (C.c_int32 * index.nc)(*index.coord_group)
        rc = (C.c_double * len(index.radii))(*index.radii)
        gamma = float(rbf_gamma) if rbf_gamma is not None else 0.0
        _cabi.check(self.lib.mia_letkf_analysis_matfun_fused_f32(
            _ptr(X), G, m, k, g0, g1, _ptr(rec), index.P, _ptr(grid), index.nc, cg, rc, len(index.radii), float(eps),
            _ptr(index.ws), index.ws.numel(), int(p_max_assumed), float(inf_factor), gamma, _ptr(out), n, 0,
            _ptr(flags), _ptr(retry), _ptr(stats), self._stream()), "mia_letkf_analysis_matfun_fused_f32")

        def finish():
            p_max, n_over = (int(v) for v in stats.tolist())        # host sync
            n_retry = int(retry.item())
            if n_over:
                return False, p_max, n_retry
            if n_retry:     # rare: the eigensolver kernel redoes the declined points and needs explicit lists
                nb = self.localize(grid, index.obs, index.radii, index.coord_group, eps, g0, g1)
                _cabi.check(self.lib.mia_letkf_analysis_retry_f32(
                    _ptr(X), G, m, k, g0, g1, _ptr(rec), index.P, _ptr(nb.cnt), _ptr(nb.idx), _ptr(nb.w), nb.p_cap,
                    nb.p_max, float(inf_factor), gamma, _ptr(out), n, 0, _ptr(flags), self._stream()),
                    "mia_letkf_analysis_retry_f32")
            return True, p_max, n_retry
        return out, flags, finish

    def localize_from_dist(self, dist, cand_idx, radii: Sequence[float], eps: float = 1e-5,
                           g0: int = 0, taper: int = 0) -> NeighbourLists:
        """dist (n_r, n, p_cap) float64 caller-evaluated distances, cand_idx (n, p_cap) int32 (-1 pad)."""
        dist = self._dev(dist, torch.float64)
        if dist.dim() == 2:
            dist = dist[None]
        cand = self._dev(cand_idx, torch.int32)
        n_r, n, cap = dist.shape
        radii = [float(r) for r in (radii if hasattr(radii, "__len__") else [radii])]
        if len(radii) != n_r:
            raise ValueError("one radius per distance component")
        rc = (C.c_double * n_r)(*radii)
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        idx = torch.empty((n, cap), dtype=torch.int32, device=self.device)
        w = torch.empty((n, cap), dtype=torch.float64, device=self.device)
        stats = torch.empty(2, dtype=torch.int32, device=self.device)
        _cabi.check(self.lib.mia_letkf_localize_from_dist_taper_f64(
            int(taper), _ptr(dist), _ptr(cand), n, cap, rc, n_r, float(eps), _ptr(cnt), _ptr(idx), _ptr(w), _ptr(stats),
            self._stream()), "mia_letkf_localize_from_dist_f64")
        p_max = int(stats[0].item())
        return NeighbourLists(cnt, idx, w, cap, p_max, g0, g0 + n)

    def merge_neighbour_lists(self, parts) -> NeighbourLists:
        """Concatenate consecutive shards' lists (trimmed to the common maximum count)."""
        p_max = max(p.p_max for p in parts)
        cap = max(8, (p_max + 7) // 8 * 8)
        idx, w = [], []
        for p in parts:
            if p.p_cap >= cap:
                idx.append(p.idx[:, :cap])
                w.append(p.w[:, :cap])
            else:
                n = p.idx.shape[0]
                i = torch.full((n, cap), -1, dtype=torch.int32, device=self.device)
                ww = torch.zeros((n, cap), dtype=torch.float64, device=self.device)
                i[:, :p.p_cap] = p.idx
                ww[:, :p.p_cap] = p.w
                idx.append(i)
                w.append(ww)
        return NeighbourLists(torch.cat([p.cnt for p in parts]), torch.cat(idx).contiguous(),
                              torch.cat(w).contiguous(), cap, p_max, parts[0].g0, parts[-1].g1)

    # ---------------------------------------------------------------- analysis
    def pack_obs(self, Yb: torch.Tensor, d: torch.Tensor, dtype=None) -> torch.Tensor:
        """(k, P) perturbations + (P,) innovations -> obs-major records (P, kp) on the device."""
        dtype = dtype or (Yb.dtype if Yb.dtype in (torch.float32, torch.float64) else torch.float32)
        Yb = Yb.to(device=self.device, dtype=dtype).contiguous()
        d = d.to(device=self.device, dtype=dtype).contiguous().reshape(-1)
        if Yb.dim() != 2:
            raise ValueError("Yb must be (k, P)")
        k, P = Yb.shape
        if d.shape[0] != P:
            raise ValueError(
                "Observational size between ensemble ({0:d}) and observations ({1:d}) do not match!".format(
                    P, d.shape[0]))
        kp = (k + 1 + 3) // 4 * 4
        rec = torch.empty((max(P, 1), kp), dtype=dtype, device=self.device)
        sfx = "f32" if dtype == torch.float32 else "f64"
        fn = getattr(self.lib, "mia_letkf_pack_obs_" + sfx)
        _cabi.check(fn(_ptr(Yb), _ptr(d), k, P, _ptr(rec), self._stream()), "mia_letkf_pack_obs_" + sfx)
        return rec[:P]

    def obs_space(self, hx, y, var=None, cov=None, dtype=None, out=None, offset: int = 0, want_rec: bool = False):
        """Observation-space variables of ONE observation subset on the device
        (AssimilationInterface._get_obs_space_variables, interface/base.py:359-379):
        hx (k, P) ensemble in observation space, y (P,) observations and either var (P,) [uncorrelated R,
        observation.py:241-245] or cov (P, P) [correlated R, observation.py:247-275].
        Returns (Yb (k, P), d (P,)) [+ rec (P, kp) with ``want_rec``].  ``out=(Yb_all, d_all[, rec_all])`` with
        ``offset`` writes into the subset's slice of the stacked arrays instead (base.py:374-377)."""
        if (var is None) == (cov is None):
            raise ValueError("give exactly one of var (uncorrelated R) and cov (correlated R)")
        hx = torch.as_tensor(hx)
        dtype = dtype or (hx.dtype if hx.dtype in (torch.float32, torch.float64) else torch.float64)
        hx = hx.to(device=self.device, dtype=dtype).contiguous()
        if hx.dim() != 2:
            raise ValueError("hx must be (k, P)")
        k, P = hx.shape
        y = torch.as_tensor(y).to(device=self.device, dtype=dtype).contiguous().reshape(-1)
        if y.shape[0] != P:
            raise ValueError("Observational size between ensemble ({0:d}) and observations ({1:d}) do not match!".format(
                P, y.shape[0]))
        kp = (k + 1 + 3) // 4 * 4
        if out is None:
            Yb = torch.empty((k, P), dtype=dtype, device=self.device)
            d = torch.empty(P, dtype=dtype, device=self.device)
            rec = torch.empty((max(P, 1), kp), dtype=dtype, device=self.device) if want_rec else None
            yb_v, d_v, rec_v, ldy = Yb, d, rec, P
        else:
            Yb, d = out[0], out[1]
            rec = out[2] if len(out) > 2 else None
            if Yb.dtype != dtype or d.dtype != dtype or not Yb.is_contiguous() or Yb.shape[0] != k:
                raise ValueError("stacked outputs must be contiguous, of the working dtype and (k, P_total)")
            if offset < 0 or offset + P > Yb.shape[1] or d.shape[0] != Yb.shape[1]:
                raise ValueError("subset does not fit the stacked arrays")
            ldy = Yb.shape[1]
            yb_v, d_v = Yb[:, offset:], d[offset:]
            rec_v = rec[offset:] if rec is not None else None
        sfx = "f32" if dtype == torch.float32 else "f64"
        if var is not None:
            var = torch.as_tensor(var).to(device=self.device, dtype=dtype).contiguous().reshape(-1)
            if var.shape[0] != P:
                raise ValueError("var must have one entry per observation")
            fn = getattr(self.lib, "mia_obs_space_uncorr_" + sfx)
            _cabi.check(fn(_ptr(hx), P, _ptr(y), _ptr(var), k, P, _ptr(yb_v), ldy, _ptr(d_v), _ptr(rec_v),
                           self._stream()), "mia_obs_space_uncorr_" + sfx)
        else:
            cov = torch.as_tensor(cov).to(device=self.device, dtype=dtype).contiguous()
            if cov.shape != (P, P):
                raise ValueError("cov must be (P, P)")
            nbytes = C.c_size_t(0)
            _cabi.check(self.lib.mia_obs_space_corr_workspace_bytes(k, P, 4 if dtype == torch.float32 else 8,
                                                                    C.byref(nbytes)), "obs_space_corr_workspace_bytes")
            ws = self._workspace("obs_corr", nbytes.value)
            info = torch.zeros(1, dtype=torch.int32, device=self.device)
            fn = getattr(self.lib, "mia_obs_space_corr_" + sfx)
            _cabi.check(fn(_ptr(hx), P, _ptr(y), _ptr(cov), k, P, _ptr(yb_v), ldy, _ptr(d_v), _ptr(rec_v), _ptr(info),
                           _ptr(ws), ws.numel(), self._stream()), "mia_obs_space_corr_" + sfx)
            bad = int(info.item())
            if bad:        # numpy.linalg.cholesky raises LinAlgError here (observation.py:249)
                raise ValueError("observation covariance is not positive definite (leading minor of order %d)" % bad)
        if out is not None:
            return None
        return (Yb, d, rec[:P]) if want_rec else (Yb, d)

    # state rows per grid point up to which the eigensolver-free route is preferred.  Measured on MI355X
    # (tools/time_rows.py): it wins at every m tried (C2 m = 32: 3.3 vs 5.7 ms, C4 m = 64: 15 vs 46 ms per 2e4 points,
    # C5 m = 64: 1.2 vs 6.3 ms), because the eigensolver kernel's per-row transform is no cheaper than one
    # Chebyshev recurrence -- so there is no hand-over; the attribute stays for experiments
    MATFUN_MAX_ROWS = 1 << 30

    # method="auto" hands a float64 shape with p_max > k to the dense tile route only while DENSE64_AUTO_DEN * p_max <=
    # DENSE64_AUTO_NUM * k (p_max <= 2.4 k).  Measured on MI355X (tools/time_dense64.py, profiles/dense64_time.json):
    # 1e5 points, against the Jacobi kernel: k 20 p 31 9.3x, k 40 p 77 16.6x (8 state rows 3.1x), k 64 p 153 7.6x, but the
    # 316 x 316 mesh at k 40 p 101 only 1.12x (unions of 16 consecutive points near 250 slots: tiles run in parts) while
    # the 1-D network at k 40 p 173 gains 2.6x.  The gain is therefore no function of the shape alone; "auto" stays below the
    # smallest p_max / k at which a measured case missed the factor 2, and method="dense64" names the route everywhere
    # the kernel covers.  State rows: a further row costs 2.8 ms on the dense route and 0.9 ms on the Jacobi kernel (k 40 p 77),
    # so the factor falls below 2 near 13 rows; "auto" hands over up to the 8 rows that were measured
    DENSE64_AUTO_NUM, DENSE64_AUTO_DEN = 12, 5
    DENSE64_AUTO_MAX_ROWS = 8

    # method="auto" hands a float64 shape with more than 64 members and p_max <= k to the wide tile route (csrc/letkf_wide64.hip)
    # from WIDE64_AUTO_MIN_K members on and up to WIDE64_AUTO_MAX_ROWS state rows.  Measured on MI355X (tools/time_wide64.py,
    # profiles/wide64_time.json), 1e5 points, against the Jacobi kernel: k 80 p 63 181.2x (319.0 / 1.76 ms),
    # 8 state rows 44.1x (378.7 / 8.59 ms), k 128 p 62 92.1x (310.4 / 3.37 ms); k 96 p 81 and k 128 p 97 (4.33 / 3.96 ms) have no Jacobi
    # time at all: that kernel answers MIA_ERR_UNSUPPORTED there.  Every measured case passes the factor 2, so the rule is the
    # route's own range (matfun64 has k <= 64) and the rows that were measured; method="wide64" names the route everywhere
    # the kernel covers
    WIDE64_AUTO_MIN_K = 65
    WIDE64_AUTO_MAX_ROWS = 8

    # method="auto" hands a float64 shape with p_max > k that none of the routes above took to the streamed dense route
    # (csrc/letkf_stream64.hip) in two cases.  (1) Wherever the Jacobi kernel cannot hold the shape (it keeps two
    # k x (k + 1) float64 matrices in LDS and answers MIA_ERR_UNSUPPORTED from 97 members on, see
    # _jacobi_primal_fits): there is nothing to compare with, the alternative is MiaError.  (2) Where the Jacobi kernel
    # runs, from STREAM64_AUTO_MIN_K members on, only while STREAM64_AUTO_DEN * p_max <= STREAM64_AUTO_NUM * k and
    # m <= STREAM64_AUTO_MAX_ROWS: the range in which every measured case beat it by the project's factor 2.
    # Measured on MI355X (tools/time_stream64.py, profiles/stream64_time.json), 1e5 points (5e4 at k 128), counter read
    # included, Jacobi kernel on a build of the parent commit / this route, median ms, m = 1 and m = 8:
    #   k 80  p  93: 126.5x (858.4 / 6.78)    22.1x (915.6 / 41.5)       k 80  p 173: 33.8x (744.2 / 22.0)   6.2x (803.0 / 129.1)
    #   k 96  p 107: 104.6x (1353.8 / 12.94)  17.8x (1421.5 / 79.9)      k 96  p 173: 47.4x (1154.1 / 24.4)  8.5x (1225.5 / 143.8)
    #   316 x 316 mesh, k 80 p 101 (tiles in 2.7 parts): 15.5x (868.4 / 56.0)   3.26x (929.5 / 284.9)
    #   k 128 p 139: 11.35 ms, 69.2 ms at m 8; p 203: 19.0 / 111.9 ms per 5e4 points -- the parent raises MiaError, no ratio
    # Every measured case passes the factor 2 beyond both spreads (all below 0.2 %), the mesh included, so the rule is the range
    # that was measured: the route's first ensemble size (as WIDE64_AUTO_MIN_K: nothing between 65 and 80 was measured), p_max / k
    # up to the largest measured (173 / 80 = 2.16), up to the 8 state rows that were measured (a further row costs 32.7 ms here
    # and 8.7 ms on the Jacobi kernel on the mesh: the factor would fall below 2 near 14 rows).  NOT measured: p_max / k above
    # 2.16 (up to 256 / 65), more than 8 rows, rows between 1 and 8, ensembles between 65 and 80 or 80 and 96 members, a mesh at
    # k 96; there "auto" stays on the Jacobi kernel where it runs.  For information, k 64 p 153: 12.56 ms against dense64's
    # 28.35 ms (the resident image leaves one workgroup a compute unit, the ring three); "auto" keeps dense64's rule at k <= 64.
    # "auto" never takes the route at k <= 64 (dense64 has those shapes under its own rule); method="stream64" names it
    # everywhere the kernel covers
    STREAM64_AUTO_MIN_K = 65
    STREAM64_AUTO_NUM, STREAM64_AUTO_DEN = 173, 80
    STREAM64_AUTO_MAX_ROWS = 8
    JACOBI_MAX_LDS = 160 * 1024 - 1024           # kMaxDynamicLds (csrc/mia_common.h)

    @staticmethod
    def _jacobi_primal_fits(k: int, p_max: int) -> bool:
        """Restates wave_lds_bytes (csrc/letkf_wave.hip) for float64 in the primal form (p_max > k, no weights): whether the
        Jacobi kernel can hold a point's two k x (k + 1) matrices.  It can up to 96 members (162 104 bytes at p_max 256) and
        cannot from 97 on, where mia_letkf_analysis_packed_f64 answers MIA_ERR_UNSUPPORTED."""
        nmax = max((k + 1) & ~1, 2)
        pl = (p_max + 3) & ~1
        nb = nmax // 2
        b = 8 * (2 * nmax * (nmax + 1) + 8 * nmax + 2 * k + 8 + pl) + 4 * pl + 16 + 2 * ((nb * (nb - 1) // 2 + 7) & ~7)
        return (b + 15) // 16 * 16 <= LetkfEngine.JACOBI_MAX_LDS

    def _stream64_auto(self, m: int, k: int, p_max: int) -> bool:
        if k < self.STREAM64_AUTO_MIN_K:
            return False
        if not self._jacobi_primal_fits(k, p_max):
            return True
        return self.STREAM64_AUTO_DEN * p_max <= self.STREAM64_AUTO_NUM * k and m <= self.STREAM64_AUTO_MAX_ROWS

    # method="auto" hands a float64 analysis with rbf_gamma to the RBF tile route (csrc/lketkf_tile64.hip) only for
    # k >= RBF64_AUTO_MIN_K and either ONE state row with p_max <= RBF64_AUTO_MAX_P or up to RBF64_AUTO_MAX_ROWS state rows with
    # p_max <= RBF64_AUTO_MAX_P_ROWS (and k <= 40: the kernel's cover).  Measured on MI355X (tools/time_rbf64.py,
    # profiles/rbf64_time.json), 1e5 points, gamma 0.5, against the Jacobi kernel, median ms:
    #   1-D networks, p_max <= 20:  k 40 m 1 31.6x (59.78 / 1.892), m 8 6.3x (66.28 / 10.54); k 20 m 1 23.5x, m 8 6.2x;
    #                               k 8 (p 12) m 1 11.5x (2.34 / 0.204), m 8 3.7x (3.35 / 0.896)
    #   1-D dense network, p_max 57 (unions of 72 slots, tiles in two parts): m 1 8.5x (44.14 / 5.177), m 8 2.5x (50.59 / 20.36)
    #   316 x 316 mesh, p_max 21 (unions of 52 slots, 3.2 parts per tile): m 1 8.4x (60.01 / 7.147), m 8 1.6x (66.65 / 40.52): MISSES
    #   316 x 316 mesh, p_max 57 (unions of 191 slots, 15.7 parts per tile): m 1 0.93x (61.30 / 65.95): SLOWER
    # Every part of a tile repeats the whole pair product and recurrence for sixteen columns, so the gain follows the number
    # of parts, which is the network's and no function of (m, k, p_max): at p_max 57 the 1-D network gains 8.5x and the mesh
    # loses.  "auto" therefore stays below the smallest p_max at which a measured case missed the factor 2: 57 with one state
    # row (the largest that passed beneath it: 21), 21 with more rows (the largest that passed beneath it: 20, at the 8 rows that
    # were measured; between 1 and 8 rows nothing was measured).  The 1-D dense network thereby forgoes its 8.5x unless
    # method="rbf64" names the route, which stays available everywhere the kernel covers.  NOT measured: a mesh with p_max <= 20
    # at 8 state rows -- by the mesh at p_max 21 it would gain less than 2x (and more than 1x); the rule is blind to it
    RBF64_AUTO_MIN_K = 8
    RBF64_AUTO_MAX_ROWS = 8
    RBF64_AUTO_MAX_P = 21
    RBF64_AUTO_MAX_P_ROWS = 20

    # method="auto" hands a float64 analysis with a positive semidefinite kernel_program (kernel_psd=True) to the kernel-expression
    # tile route (csrc/lketkf_kern64.hip) only for ONE state row (KERN64_AUTO_MAX_ROWS), k >= KERN64_AUTO_MIN_K (<= 40: the cover)
    # and p_max <= KERN64_AUTO_MAX_P.  The rule cannot see the kernel function, so a class passes only if every kernel measured in
    # it gained 2x.  Measured on MI355X (tools/time_kern64.py, profiles/kern64_time.json), 1e5 points, inflation 1.1,
    # against the Jacobi expression route, counter read and redo of declined points included, median ms, for
    # rational (sq, degree 14) / ornuhl (l1, 12) / poly2 (dot, 63 mean, up to 126) / poly2 + ornuhl * scale (all three):
    #   k 40 p 20  m 1: 15.1x (80.5 / 5.32)  20.2x (76.1 / 3.77)  6.6x (79.1 / 11.98)  5.9x (82.6 / 14.00)
    #              m 8:  4.6x (88.4 / 19.05)  5.5x (84.0 / 15.21)  1.14x (87.2 / 76.7)  1.15x (90.6 / 78.6): the polynomials MISS
    #   k 20 p 20  m 1:  8.6x (9.61 / 1.12)  10.4x (9.12 / 0.88)  2.28x (9.31 / 4.08)  2.19x (9.83 / 4.49)   (22 / 23 points redone)
    #              m 8:  2.9x                 3.2x                 0.57x                0.59x: SLOWER
    #   k 8  p 12  m 1:  5.1x (2.49 / 0.49)   5.7x (2.39 / 0.42)  1.65x (2.46 / 1.49)  1.71x (2.60 / 1.52): the polynomials MISS
    #              m 8:  1.7x                 1.9x                 0.42x                0.47x: all MISS
    #   316 x 316 mesh, k 40 p 21 (tiles in 3.2 parts)
    #              m 1:  4.9x (83.9 / 17.0)   6.3x (77.4 / 12.4)  3.19x (86.9 / 27.3)  2.61x (88.0 / 33.7)
    #              m 8:  1.45x                1.67x                0.60x                0.58x: all MISS
    # A state row costs one Chebyshev recurrence of the point's degree, and a polynomial kernel's degree is 4-5 times an RBF's: with
    # eight rows the recurrence outweighs the eigensolve it replaces.  So: one row (between 1 and 8 nothing was measured), from the
    # smallest measured k at which all four kernels passed (20; 8 missed, between them nothing was measured), up to the largest
    # measured p_max (21; beyond it nothing was measured -- the RBF form loses on a mesh at p_max 57).  The bounded kernels thereby
    # forgo 3-5x at eight rows and 5x at k = 8 unless method="kern64" names the route, which stays available everywhere the
    # kernel covers
    KERN64_AUTO_MIN_K = 20
    KERN64_AUTO_MAX_ROWS = 1
    KERN64_AUTO_MAX_P = 21

    # method="auto" hands a float64 shape with p_max > k to the dense route under a tile map (csrc/letkf_patch64.hip) only when
    # the caller gives ``tile_points``, and then only for ONE state row, PATCH64_AUTO_MIN_K <= k (<= 64: the cover),
    # PATCH64_AUTO_DEN * p_max <= PATCH64_AUTO_NUM * k and a largest union (the census' count) that fits the record image, so that
    # every tile runs in one pass.  Measured on MI355X (tools/time_patch64.py, profiles/patch64_time.json), 316 x 316
    # meshes in 4 x 4 patches, against the Jacobi kernel, census (0.15 - 0.24 ms) inside the call, median ms:
    #   k 40 p 101 (DESIGN 9's failing row: dense64 on strips 61.7, 1.1x):  3.35x (67.63 / 20.18)     8 state rows: 0.67x (74.1 / 111.4) LOSES
    #   k 20 p  45:  4.30x (9.53 / 2.22)      k 64 p 101: 10.97x (240.5 / 21.9)      k 40 p 76, observations at every 2nd point: 12.5x (70.2 / 5.61)
    # Every one-row case passes the factor 2 beyond both spreads (all below 0.2 ms); with eight rows the route loses, because a
    # further row costs 13.0 ms here and 0.93 ms on the Jacobi kernel -- at two rows the factor would be near 2.06, which is not
    # a margin, and nothing between 1 and 8 rows was measured.  So: one row, from the smallest measured ensemble (20; the KT = 1
    # instantiation was not timed) and up to the largest measured p_max / k (101 / 40).  Outside, with a map, "auto" goes on to
    # dense64's own rule and the Jacobi kernel as before; method="patch64" names the route everywhere the kernel covers.  The
    # rule cannot see whether a map is a good one (tiles of neighbouring points): the union condition is what stands in for it
    PATCH64_AUTO_MIN_K = 20
    PATCH64_AUTO_NUM, PATCH64_AUTO_DEN = 101, 40
    PATCH64_AUTO_MAX_ROWS = 1

    def _patch64_auto(self, m: int, k: int, p_max: int) -> bool:
        return (m <= self.PATCH64_AUTO_MAX_ROWS and k >= self.PATCH64_AUTO_MIN_K
                and self.PATCH64_AUTO_DEN * p_max <= self.PATCH64_AUTO_NUM * k)

    # LETKF(..., mesh_shape=...).analyse_arrays hands a float64 analysis that method="auto" would run on letkf_stream64_kernel
    # (_stream64_auto) to method="patch64s" (csrc/letkf_patch64s.hip: the same kernel under the map of 4 x 4 patches) where the
    # census says every tile fits one pass (largest union <= 256) and PATCH64S_AUTO_MIN_K <= k <= PATCH64S_AUTO_MAX_K,
    # PATCH64S_AUTO_DEN * p_max <= PATCH64S_AUTO_NUM * k and m <= PATCH64S_AUTO_MAX_ROWS -- the range in which every MEASURED
    # case is faster than method="stream64" on a build of the PARENT commit beyond both spreads (slowest sample of this route
    # against the fastest of the baseline; the criterion of _ienks_patch64_auto's case (a): the bits are equal under any map, so
    # there is nothing else to weigh).  method="auto" itself never takes the route: the hand-over lives in the class, as for
    # estimate_weights_arrays and the IEnKS classes.
    # Measured on MI355X (tools/time_patch64s.py, profiles/patch64s_time.json), 316 x 316 meshes (224 x 224 at k = 128)
    # with an observation at every point, radius 3 (3.5), p_max 101 (145), 4 x 4 patches (largest union 176 / 232), census (0.7 -
    # 0.9 ms, first call only) outside, three rounds of four calls, the methods alternating, counter read included, median ms
    # per call; Jacobi kernel and method="stream64" on a build of the parent commit / method="stream64" on this build / this route:
    #   k  65 m 1:  288.2 /  57.18 /  57.14 / 10.60   5.39x the route without a map (worst round against best: 5.33x)   27.1x the Jacobi kernel
    #   k  80 m 1:  868.4 /  56.05 /  56.01 / 14.60   3.84x (3.78x)                                                       59.5x
    #   k  96 m 1: 1434.1 /  87.93 /  87.89 / 16.12   5.45x (5.45x)                                                       89.0x
    #   k  80 m 8:  927.0 / 284.97 / 285.24 / 82.02   3.47x (3.47x)                                                       11.3x
    #   k 128 m 1: MiaError / 80.46 / 80.47 / 29.50   2.73x (2.72x)                                       (no Jacobi kernel)
    # (spreads at most 0.25 ms; method="stream64" agrees between the two builds within its spreads in all five -- its kernel is
    # unchanged; Xa and flags bit-identical to the route without a map in all five; nothing declined; k 80 m 1 reproduces the
    # 56.0 ms that STREAM64_AUTO_*'s table records for this mesh).  A further state row costs 9.6 ms here against 32.7 ms without
    # the map (k 80).  Every measured case passes, so the rule is the range that was measured: 65 .. 128 members, p_max / k up to
    # the largest measured (101 / 65 = 1.55), up to the 8 state rows that were measured (at k = 80 only).  NOT measured: other
    # radii, observations at every second point or sparser, ensembles between the measured sizes, 2 - 7 state rows, 8 rows at any
    # k but 80, p_max / k above 1.55; there the class stays on method="auto".  method="patch64s" itself stays available
    # everywhere the kernel covers
    PATCH64S_AUTO_MIN_K, PATCH64S_AUTO_MAX_K = 65, 128
    PATCH64S_AUTO_NUM, PATCH64S_AUTO_DEN = 101, 65
    PATCH64S_AUTO_MAX_ROWS = 8
    PATCH64S_MAX_BLOCKS = 16               # kPatch64SMaxBlocks (csrc/letkf_patch64s.hip): 256 slots at every ensemble size

    def _patch64s_auto(self, m: int, k: int, p_max: int) -> bool:
        """Whether LETKF(mesh_shape=...) names method="patch64s" for a float64 analysis that "auto" would hand to
        letkf_stream64_kernel (the class checks :meth:`_stream64_auto`, the cover and the census beside this)."""
        if k < 2 or k > 128 or p_max <= k or p_max > 256:
            return False
        return (self.PATCH64S_AUTO_MIN_K <= k <= self.PATCH64S_AUTO_MAX_K and m <= self.PATCH64S_AUTO_MAX_ROWS
                and self.PATCH64S_AUTO_DEN * p_max <= self.PATCH64S_AUTO_NUM * k)

    def patch64s_fits(self, nbrs: NeighbourLists, tile_points: torch.Tensor, k: int) -> bool:
        """Whether every tile of the map runs in ONE pass of analysis(method="patch64s") (largest union <= 256): the census,
        once per map."""
        return self._patch64_map(nbrs, tile_points, None, k, self.PATCH64S_MAX_BLOCKS)[2]

    @staticmethod
    def _dense64_capacity_blocks(k: int) -> int:
        """Restates dense64_capacity_blocks / patch64_capacity_blocks (csrc): sixteen-slot blocks of the record image that fit
        the LDS at this ensemble size."""
        ks = ((k + 1 + 3) // 4 * 4) | 1
        ub = 16
        while ub > 0 and ((16 * ub * ks + 16 * (16 * ub + 1)) * 8 + 16 * ub * 4 + 15) // 16 * 16 > LetkfEngine.JACOBI_MAX_LDS:
            ub -= 1
        return ub

    def _patch64_map(self, nbrs: NeighbourLists, tile_points: torch.Tensor, union_blocks: Optional[int], k: int,
                     capacity: Optional[int] = None):
        """The device copy of a tile map and the blocks of the record image for it (``capacity``: the largest image of the
        route in sixteen-slot blocks; None = the dense route's at this ensemble size, weights_patch64 passes 16).  The map is validated by
        tile_union_census_kernel (every tile) and, with ``union_blocks=None``, the largest union of a tile counted; both come
        back in one 8-byte read.  The result is kept on ``nbrs`` under the map's identity, so a cycled filter pays once per
        geometry.  ValueError for a map that is not a partition of the shard's points, before any analysis launch.  Returns
        (map on the device, blocks, whether every tile fits the image in one pass -- True when the caller named the blocks)."""
        n = nbrs.g1 - nbrs.g0
        if (not isinstance(tile_points, torch.Tensor) or tile_points.dtype != torch.int32 or tile_points.dim() != 2
                or tile_points.shape[1] != 16):
            raise ValueError("tile_points must be an int32 tensor (n_tiles, 16)")
        cap = self._dense64_capacity_blocks(k) if capacity is None else int(capacity)
        if union_blocks is not None and not 1 <= int(union_blocks) <= cap:
            raise ValueError("union_blocks must lie in 1 .. %d at k = %d" % (cap, k))
        if nbrs.tile_census is None:
            nbrs.tile_census = {}
        ent = nbrs.tile_census.get(id(tile_points))
        if ent is None or ent[0] is not tile_points or (union_blocks is None and ent[2] is None):
            if tile_points.shape[0] == 0:
                raise ValueError("invalid tile map: a point that does not occur (the map is empty)")
            tp = tile_points.to(self.device).contiguous() if ent is None or ent[0] is not tile_points else ent[1]
            out2 = torch.empty(2, dtype=torch.int32, device=self.device)
            ws = self._workspace("tile_census", 4 * (n + 2))
            _cabi.check(self.lib.mia_letkf_tile_union_census(_ptr(tp), tp.shape[0], n, _ptr(nbrs.cnt), _ptr(nbrs.idx), nbrs.p_cap,
                                                             nbrs.p_max, 1 if union_blocks is None else 0, _ptr(out2), _ptr(ws),
                                                             ws.numel() * ws.element_size(), self._stream()),
                        "mia_letkf_tile_union_census")
            err, umax = (int(v) for v in out2.tolist())      # host sync (8 bytes)
            if err:
                raise ValueError("invalid tile map: " + ", ".join(t for b, t in MIA_TILEMAP_FAULTS if err & b))
            ent = (tile_points, tp, umax if union_blocks is None else None)
            nbrs.tile_census[id(tile_points)] = ent
        ub = int(union_blocks) if union_blocks is not None else min(max((ent[2] + 15) // 16, 1), cap)
        return ent[1], ub, union_blocks is not None or ent[2] <= 16 * cap

    def _kern64_auto(self, m: int, k: int, p_max: int) -> bool:
        return k >= self.KERN64_AUTO_MIN_K and m <= self.KERN64_AUTO_MAX_ROWS and p_max <= self.KERN64_AUTO_MAX_P

    def _rbf64_auto(self, m: int, k: int, p_max: int) -> bool:
        return k >= self.RBF64_AUTO_MIN_K and ((m == 1 and p_max <= self.RBF64_AUTO_MAX_P) or
                                               (m <= self.RBF64_AUTO_MAX_ROWS and p_max <= self.RBF64_AUTO_MAX_P_ROWS))

    def _matfun64_auto(self, m: int, k: int, p_max: int) -> bool:
        return True           # (the entry's own cover is the rule: p_max <= k <= 64)

    def _dense64_auto(self, m: int, k: int, p_max: int) -> bool:
        return self.DENSE64_AUTO_DEN * p_max <= self.DENSE64_AUTO_NUM * k and m <= self.DENSE64_AUTO_MAX_ROWS

    def _wide64_auto(self, m: int, k: int, p_max: int) -> bool:
        return k >= self.WIDE64_AUTO_MIN_K and m <= self.WIDE64_AUTO_MAX_ROWS

    ANALYSIS_METHODS = ("auto", "eig", "matfun", "matfun64", "dense64", "patch64", "wide64", "stream64", "rbf64", "kern64")
    # the float64 plain-core tile routes in the order in which "auto" tries them: (method, C entry, its rule under "auto").
    # A route answers MIA_ERR_UNSUPPORTED (-3) outside its cover and the walk goes on; patch64 is the one row with steps of its
    # own in front of the entry (the caller's tile map, the cover, the census).  A new route is one row here, its entry in
    # csrc/letkf_entry.hip and its prototype in _cabi._PROTOS
    TILE64_ROUTES = (("matfun64", "mia_letkf_analysis_matfun_f64", _matfun64_auto),
                     ("patch64", "mia_letkf_analysis_patch_f64", _patch64_auto),
                     ("dense64", "mia_letkf_analysis_dense_f64", _dense64_auto),
                     ("wide64", "mia_letkf_analysis_wide_f64", _wide64_auto),
                     ("stream64", "mia_letkf_analysis_stream_f64", _stream64_auto))
    TILE64_METHODS = tuple(r[0] for r in TILE64_ROUTES)
    # ... and the rows that only their own name takes ("auto" never does at this level: the class names the method under
    # _patch64s_auto, as the IEnKS classes name ienks_update's "stream64" and "patch64"); the "method must be one of" message
    # lists ANALYSIS_METHODS, the methods that need no further argument or had their place there first
    TILE64_NAMED_ROUTES = (("patch64s", "mia_letkf_analysis_patch_stream_f64", None),)
    TILE64_NAMED_METHODS = tuple(r[0] for r in TILE64_NAMED_ROUTES)
    # the rows with steps of their own in front of the entry -- the caller's tile map, the cover, the census (once per map):
    # method -> (cover function, the route's largest image in sixteen-slot blocks; None = the dense route's at this ensemble size)
    TILE64_MAP_ROUTES = {"patch64": ("mia_letkf_patch_f64_cover", None),
                         "patch64s": ("mia_letkf_patch_stream_f64_cover", PATCH64S_MAX_BLOCKS)}

    def analysis(self, X: torch.Tensor, Yb: Optional[torch.Tensor], d: Optional[torch.Tensor],
                 nbrs: NeighbourLists, inf_factor: float = 1.0, return_weights: bool = False,
                 rbf_gamma: Optional[float] = None, out: Optional[torch.Tensor] = None, out_offset: int = 0,
                 return_flags: bool = False, rec: Optional[torch.Tensor] = None, method: str = "auto",
                 defer_retry: bool = False, retry: Optional[torch.Tensor] = None,
                 flags: Optional[torch.Tensor] = None, kernel_program=None, kernel_psd: bool = False,
                 tile_points: Optional[torch.Tensor] = None, union_blocks: Optional[int] = None):
        """X (m, k, G) prior ensemble (grid fastest), Yb (k, P), d (P,) [or their packed records
        ``rec`` from :meth:`pack_obs`]: analysis of the shard described by ``nbrs``.
        Returns Xa (m, k, n) [, W (n, k, k)] [, flags (n,)].

        ``method``: "eig" = fused Jacobi eigensolver kernel (always available, the only one that can
        return the weights); "matfun" = eigensolver-free Chebyshev matrix-function route (float32, few
        state rows, no weights), with the eigensolver redoing the grid points it declines; "matfun64" =
        the same route in float64 on tiles of sixteen points (2 <= k <= 64, p_max <= k, plain ETKF core,
        no weights); "dense64" = its primal form for dense local networks (2 <= k <= 64, k < p_max <= 256 slots, same
        conditions); "patch64" = dense64's analysis with the sixteen points of a tile taken from ``tile_points`` (int32
        (n_tiles, 16): indices into the shard's points, -1 = empty slot, every point exactly once -- :func:`mesh_tiles` makes the
        4 x 4 patches of a 2-D mesh, any other partition is legal; an invalid map raises ValueError before the analysis is
        launched) and the record image sized for the largest union of a tile (``union_blocks=None``: counted on the GPU once per
        map and kept on ``nbrs``; an int names the sixteen-slot blocks and leaves the count, not the validation); same cover and
        conditions as dense64, the same bits, csrc/letkf_patch64.hip; "auto" takes it only when ``tile_points`` is given and
        only under PATCH64_AUTO_* (one state row, 20 <= k, p_max <= 2.525 k, unions that fit the image), and without ``tile_points`` every call is what it was; "wide64" = matfun64's analysis with a tile's union split over two or four wavefronts (2 <= k <= 128,
        p_max <= k, same conditions; what ensembles of 65 .. 128 members run); "stream64" = dense64's analysis with the union's
        records streamed through a ring in LDS instead of a resident image (2 <= k <= 128, k < p_max <= 256, same conditions;
        what dense networks of 65 .. 128 members run -- "auto" takes it from STREAM64_AUTO_MIN_K members on wherever the Jacobi
        kernel cannot hold the shape, k >= 97, and elsewhere only inside STREAM64_AUTO_*; a point it declines is redone by the
        Jacobi kernel, and at k >= 97 that redo raises MiaError AFTER the other points have been written, as below);
        "patch64s" = stream64's analysis with the sixteen points of a tile taken from ``tile_points`` as for "patch64"
        (csrc/letkf_patch64s.hip, mia_letkf_analysis_patch_stream_f64; stream64's cover and conditions, stream64's bits under
        any map; ``union_blocks`` 1 .. 16 at every ensemble size, None = sized for the largest union the census counts, which
        is shared with "patch64", ``weights_patch64`` and ``ienks_update(method="patch64")``; a tile whose union exceeds the
        blocks runs in halves of its slots; ValueError without ``tile_points``, for a wrong dtype or shape of the map, a map
        that is no partition of the shard's points and ``union_blocks`` outside 1 .. 16, before any launch); "auto" never
        takes it at this level -- LETKF(mesh_shape=...) names it where :meth:`_patch64s_auto` says so; "rbf64" = the RBF-kernelised core in float64 on
        tiles (``rbf_gamma`` given, 2 <= k <= 40, lists of at most 64 observations -- no p_max <= k condition --, no
        ``kernel_program``, no weights; csrc/lketkf_tile64.hip); "kern64" = the same kernel with K from a ``kernel_program``
        (float64, the cover of rbf64, ``kernel_psd=True``, no tanh / sin, no weights; csrc/lketkf_kern64.hip); "auto" picks
        matfun / matfun64 / dense64 / wide64 / stream64 / rbf64 / kern64 by
        the state's dtype, the core and the shape when one applies (dense64 only while p_max <= 2.4 k and m <= 8, see
        DENSE64_AUTO_NUM; wide64 only from WIDE64_AUTO_MIN_K members and up to WIDE64_AUTO_MAX_ROWS state rows -- below
        65 members matfun64 has taken the shape already; rbf64 from RBF64_AUTO_MIN_K members, with one state row while
        p_max <= RBF64_AUTO_MAX_P and with up to RBF64_AUTO_MAX_ROWS state rows while p_max <= RBF64_AUTO_MAX_P_ROWS: beyond that
        its gain depends on the network -- a 2-D mesh with 57 local observations runs slower than on the Jacobi kernel).  Points the float64 tile routes decline (Chebyshev degree above 127:
        observations several times stronger than the background spread) are redone by the Jacobi kernel, which holds a point's
        matrices in LDS; where it cannot (about 70 local observations and more: e.g. k = 96 with p_max 81, k = 128 with p_max 97,
        shapes that raised altogether before the wide route) that redo raises MiaError AFTER the other points have been
        written -- data-dependent; the flags name the declined points (MIA_FLAG_RETRY).  Points rbf64 declines (a non-finite
        record in their list, degree above 127) are redone the same way, as are kern64's (mia_lketkf_kernel_analysis_retry_f64,
        the Jacobi kernel with the same program; polynomial kernels reach degree 127 much sooner than an RBF kernel).  Float64 weights without an eigensolver
        are :meth:`weights64`'s (weights only, no analysis); ``return_weights=True`` here stays on the Jacobi kernel in float64.
        With ``defer_retry`` the (8-byte, synchronising) read of the decline
        counter is left to the caller: the return value gains a trailing callable that must be invoked.
        ``retry`` (1 int32, zeroed by the caller) / ``flags`` (n int32): caller-owned counter and flag
        buffers, e.g. one counter shared by the launches of several sub-ranges.
        ``rbf_gamma`` selects the RBF-kernelised core (KETKFModule with RBFKernel), ``kernel_program``
        ([(MIA_KOP_*, value), ...], see kernels.py) the kernel-expression route for every other reference kernel.
        ``kernel_psd``: the program's kernel is positive semidefinite by construction (``kernels.kernel_is_psd``; a caller who
        passes a raw program asserts it) -- the eigensolver-free kern64 route is right only then, because the reference clamps
        negative eigenvalues of the centred kernel matrix and a polynomial cannot; "auto" takes kern64 for such a float64
        program under KERN64_AUTO_* (one state row, KERN64_AUTO_MIN_K <= k, p_max <= KERN64_AUTO_MAX_P: with more rows or fewer
        members a polynomial kernel gains less than 2x or loses) and runs every other program on the Jacobi kernel, as before."""
        if X.dim() == 2:
            X = X[None]
        X = X.to(self.device).contiguous()
        dtype = X.dtype
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("state must be float32 or float64")
        m, k, G = X.shape
        if rec is None:
            if Yb.dim() != 2 or Yb.shape[0] != k:
                raise ValueError("Yb must be (k, P) with the state's ensemble size")
            rec = self.pack_obs(Yb, d, dtype)
            self._keep_rec = rec      # (a record buffer packed during HIP-graph capture must outlive the capture)
        if rec.dtype != dtype or rec.shape[1] != (k + 1 + 3) // 4 * 4:
            raise ValueError("packed records do not match the state's dtype / ensemble size")
        if method not in self.ANALYSIS_METHODS + self.TILE64_NAMED_METHODS:
            raise ValueError("method must be " + _one_of(self.ANALYSIS_METHODS))
        if method in self.TILE64_MAP_ROUTES and tile_points is None:
            raise ValueError("the %s route needs tile_points (see mesh_tiles)" % method)
        # float64 RBF-kernelised filter on tiles (csrc/lketkf_tile64.hip): 2 <= k <= 40, lists of at most 64 observations, no weights
        can_rbf64 = dtype == torch.float64 and not return_weights and rbf_gamma is not None and kernel_program is None
        if method == "rbf64" and not can_rbf64:
            raise ValueError("the rbf64 route needs float64, rbf_gamma, no kernel_program and cannot return the weights")
        # ... and the same kernel with K from a kernel expression (csrc/lketkf_kern64.hip): positive semidefinite kernels only
        can_kern64 = (dtype == torch.float64 and not return_weights and kernel_program is not None and rbf_gamma is None
                      and bool(kernel_psd))
        if method == "kern64" and not can_kern64:
            raise ValueError("the kern64 route needs float64, a kernel_program with kernel_psd=True and cannot return the weights")
        P = rec.shape[0]
        n = nbrs.g1 - nbrs.g0
        if out is None:
            out = torch.empty((m, k, n), dtype=dtype, device=self.device)
            out_offset = 0
        ldo = out.shape[-1]
        W = torch.empty((n, k, k), dtype=dtype, device=self.device) if return_weights else None
        if flags is None:
            flags = torch.empty(n, dtype=torch.int32, device=self.device)
        elif flags.numel() != n or flags.dtype != torch.int32 or not flags.is_contiguous():
            raise ValueError("flags must be a contiguous int32 tensor with one entry per grid point")
        sfx = "f32" if dtype == torch.float32 else "f64"
        gamma = float(rbf_gamma) if rbf_gamma is not None else 0.0
        args = (_ptr(X), G, m, k, nbrs.g0, nbrs.g1, _ptr(rec), P, _ptr(nbrs.cnt), _ptr(nbrs.idx),
                _ptr(nbrs.w), nbrs.p_cap, nbrs.p_max, float(inf_factor), gamma, _ptr(out), ldo, out_offset)
        alive = (X, rec, out, W, flags, nbrs)      # (args holds addresses: a deferred redo must find the arrays alive)

        flags_out = flags if return_flags else None
        if kernel_program is not None:
            if rbf_gamma is not None:
                raise ValueError("give rbf_gamma or kernel_program, not both")
            nops = len(kernel_program)
            prog = (_cabi.KernelOp * max(nops, 1))()
            for i, (op, val) in enumerate(kernel_program):
                prog[i].op, prog[i].value = int(op), float(val)
            pargs = (*args[:13], float(inf_factor), prog, nops, *args[15:])
            finish = None
            if can_kern64 and n > 0 and (method == "kern64" or (method == "auto" and self._kern64_auto(m, k, nbrs.p_max))):
                if retry is None:
                    retry = torch.zeros(1, dtype=torch.int32, device=self.device)
                rc = self.lib.mia_lketkf_kernel_analysis_matfun_f64(*pargs, _ptr(flags), _ptr(retry), self._stream())
                if rc == -3 and method == "auto":      # shape outside the kernel, tanh / sin, tile = 0: the Jacobi kernel below
                    pass
                else:
                    _cabi.check(rc, "mia_lketkf_kernel_analysis_matfun_f64")
                    finish = self._redo_behind_counter(retry, "mia_lketkf_kernel_analysis_retry_f64",
                                                       lambda: (*pargs, _ptr(flags)), alive)
            if finish is None:
                fn = getattr(self.lib, "mia_lketkf_kernel_analysis_packed_" + sfx)
                _cabi.check(fn(*pargs, _ptr(W), _ptr(flags), self._stream()), "mia_lketkf_kernel_analysis_packed_" + sfx)
            return _result(out, W, flags_out, finish, defer_retry)
        if (return_weights and dtype == torch.float32 and method != "eig" and n > 0):
            # weights without an eigensolver (dual route, order <= 32); -3 = shape outside that kernel
            if retry is None:
                retry = torch.zeros(1, dtype=torch.int32, device=self.device)
            rc = self.lib.mia_letkf_weights_matfun_f32(*args, _ptr(W), _ptr(flags), _ptr(retry), self._stream())
            if rc != -3:
                _cabi.check(rc, "mia_letkf_weights_matfun_f32")
                return _result(out, W, flags_out, self._redo_behind_counter(
                    retry, "mia_letkf_weights_retry_f32", lambda: (*args, _ptr(W), _ptr(flags)), alive), defer_retry)
        can_matfun = dtype == torch.float32 and not return_weights and n > 0
        if method == "matfun" and not can_matfun:
            raise ValueError("the matfun route needs float32 and cannot return the weights")
        # float64 on tiles (csrc/letkf_tile64.hip: p_max <= k <= 64; csrc/letkf_dense64.hip: p_max > k; csrc/letkf_wide64.hip:
        # p_max <= k <= 128; csrc/letkf_stream64.hip: k < p_max <= 256, k <= 128): plain ETKF core, no weights.  "auto" walks
        # TILE64_ROUTES in its order (the dense route up to p_max = 2.4 k, the wide one under WIDE64_AUTO_*, the streamed one
        # under STREAM64_AUTO_*, the one with a map under PATCH64_AUTO_*) and falls back to the Jacobi kernel elsewhere; a
        # route's own name takes that row alone and raises there instead.
        can_matfun64 = dtype == torch.float64 and not return_weights and rbf_gamma is None
        if method in self.TILE64_METHODS + self.TILE64_NAMED_METHODS and not can_matfun64:
            raise ValueError("the %s route needs float64, the plain ETKF core and cannot return the weights" % method)
        use_matfun = can_matfun and (method == "matfun" or (method == "auto" and m <= self.MATFUN_MAX_ROWS))
        # the eigensolver-free entry that is tried, its status, and whether -3 (shape outside the kernel, or tile = 0) hands
        # the shard to the Jacobi kernel below instead of raising
        name, rc, soft = None, -3, method == "auto"
        if can_matfun64 and n > 0 and (method == "auto" or method in self.TILE64_METHODS + self.TILE64_NAMED_METHODS):
            if retry is None:
                retry = torch.zeros(1, dtype=torch.int32, device=self.device)
            name = self.TILE64_ROUTES[0][1]
            for meth, entry, auto in self.TILE64_ROUTES + self.TILE64_NAMED_ROUTES:
                if rc != -3:
                    break
                if method != meth and not (method == "auto" and auto is not None and auto(self, m, k, nbrs.p_max)):
                    continue
                more = ()
                if meth in self.TILE64_MAP_ROUTES:      # the rows with steps of their own: the caller's map, the cover, the census (once per map)
                    if tile_points is None:
                        continue
                    name = entry
                    cover, cap = self.TILE64_MAP_ROUTES[meth]
                    if getattr(self.lib, cover)(m, k, nbrs.p_max, G, ldo, n, P) != 1:
                        continue
                    tp, ub, fits = self._patch64_map(nbrs, tile_points, union_blocks, k, cap)
                    if not fits and method != meth:      # ("auto": a map whose tiles would run in parts is left to the rows below)
                        continue
                    more = (_ptr(tp), tp.shape[0], ub)
                name = entry
                rc = getattr(self.lib, entry)(*args, _ptr(flags), _ptr(retry), *more, self._stream())
        elif can_rbf64 and n > 0 and (method == "rbf64" or (method == "auto" and self._rbf64_auto(m, k, nbrs.p_max))):
            if retry is None:
                retry = torch.zeros(1, dtype=torch.int32, device=self.device)
            name = "mia_lketkf_rbf_analysis_matfun_f64"
            rc = self.lib.mia_lketkf_rbf_analysis_matfun_f64(*args, _ptr(flags), _ptr(retry), self._stream())
        elif use_matfun:
            if retry is None:
                retry = torch.zeros(1, dtype=torch.int32, device=self.device)
            name, soft = "mia_letkf_analysis_matfun_f32", True      # (outside the matfun kernels: eigensolver route)
            rc = self.lib.mia_letkf_analysis_matfun_f32(*args, _ptr(flags), _ptr(retry), self._stream())
        if name is None or (rc == -3 and soft):
            fn = getattr(self.lib, "mia_letkf_analysis_packed_" + sfx)
            _cabi.check(fn(*args, _ptr(W), _ptr(flags), self._stream()), "mia_letkf_analysis_packed_" + sfx)
            return _result(out, W, flags_out, None, defer_retry)
        _cabi.check(rc, name)
        return _result(out, W, flags_out, self._redo_behind_counter(
            retry, "mia_letkf_analysis_retry_" + sfx, lambda: (*args, _ptr(flags)), alive), defer_retry)

    def _weights_tile64(self, entry: str, who: str, Yb, d, nbrs: NeighbourLists, inf_factor, rec, out, return_flags, defer_retry,
                        rbf_gamma, more=None):
        """The body of :meth:`weights64`, :meth:`weights_wide64`, :meth:`weights_stream64` and :meth:`weights_patch64`: the C
        ``entry`` of the route and the public method's name ``who`` for the messages; arguments and answers as documented
        there.  ``more(k)``: the entry's further arguments in front of the stream (weights_patch64's map, number of tiles and
        blocks), asked for once the shapes have been checked and before the launch; None from it: the route does not cover."""
        if rec is None:
            if Yb.dim() != 2 or Yb.dtype != torch.float64:
                return None
            rec = self.pack_obs(Yb, d, torch.float64)
        if rec.dtype != torch.float64 or rec.dim() != 2 or rec.shape[1] < 3:
            return None
        kp = rec.shape[1]
        k = int(Yb.shape[0]) if Yb is not None else (int(out.shape[-1]) if out is not None else None)
        if k is None:
            raise ValueError(who + " from packed records alone needs out= (n, k, k) for the ensemble size")
        if kp != (k + 1 + 3) // 4 * 4:
            raise ValueError("packed records do not match the ensemble size")
        n = nbrs.g1 - nbrs.g0
        if out is None:
            out = torch.empty((n, k, k), dtype=torch.float64, device=self.device)
        elif out.shape != (n, k, k) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 tensor (n, k, k)")
        W = out
        flags = torch.empty(n, dtype=torch.int32, device=self.device)
        retry = torch.zeros(1, dtype=torch.int32, device=self.device)
        gamma = float(rbf_gamma) if rbf_gamma is not None else 0.0

        # the entry and the redo entry take (X, *shard, Xa, *tail): the tile kernel writes W and flags only, X = Xa = NULL
        shard = (nbrs.g1, 1, k, nbrs.g0, nbrs.g1, _ptr(rec), rec.shape[0], _ptr(nbrs.cnt), _ptr(nbrs.idx), _ptr(nbrs.w),
                 nbrs.p_cap, nbrs.p_max, float(inf_factor), gamma)
        tail = (n, 0, _ptr(W), _ptr(flags))
        extra = ()
        if more is not None:
            extra = more(k)
            if extra is None:
                return None
        rc = getattr(self.lib, entry)(None, *shard, None, *tail, _ptr(retry), *extra, self._stream())
        if rc == -3:
            return None
        _cabi.check(rc, entry)

        def redo_args():
            # the Jacobi kernel computes an analysis next to the weights: a one-row zero state and its output, from the
            # workspace, and only now that a point needs them
            x0 = self._workspace("weights64_x0", 8 * k * max(nbrs.g1, 1)).view(torch.float64)[:k * nbrs.g1].zero_()
            xa = self._workspace("weights64_xa", 8 * k * max(n, 1)).view(torch.float64)
            return (_ptr(x0), *shard, _ptr(xa), *tail)
        finish = self._redo_behind_counter(retry, "mia_letkf_weights_retry_f64", redo_args, (rec, nbrs, W, flags))
        return _result(W, None, flags if return_flags else None, finish, defer_retry)

    # LETKF.estimate_weights_arrays hands float64 weights to weights64 by default only from this ensemble size on.  Measured on
    # MI355X (tools/time_weights64.py, profiles/weights64_time.json), 1e5 points, against the Jacobi kernel with W:
    # counter read included: k 40 p 20 3.25x (14.29 / 4.39 ms), k 64 p 31 6.15x (103.0 / 16.7 ms), but k 20 p 10 only 1.64x
    # (3.38 / 2.06 ms; spreads below 1 % in all three).  The default therefore starts at the smallest measured k that passed the
    # factor 2; weights64 itself stays available everywhere the kernel covers
    WEIGHTS64_AUTO_MIN_K = 40

    def weights64(self, Yb: Optional[torch.Tensor], d: Optional[torch.Tensor], nbrs: NeighbourLists, inf_factor: float = 1.0,
                  rec: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, return_flags: bool = False,
                  defer_retry: bool = False, rbf_gamma: Optional[float] = None):
        """The float64 weights W (n, k, k), W[g, i, j] = w_mean_i + W_pert_ij (LETKF.estimate_weights, letkf.py:127-146), of the
        shard described by ``nbrs`` on the matrix cores (mia_letkf_weights_matfun_f64, csrc/letkf_tile64w.hip): float64 Yb (k, P)
        and d (P,) [or their packed records ``rec``], 2 <= k <= 64, p_max <= k, plain ETKF core.  Returns W [, flags (n,)]
        [, finish] -- or None where the entry answers MIA_ERR_UNSUPPORTED (any other shape, float32 input, ``rbf_gamma``,
        option tile = 0): the caller then takes ``analysis(..., return_weights=True)``.  Points the kernel declines are redone
        by the Jacobi kernel (mia_letkf_weights_retry_f64) behind the 8-byte read of the decline counter; with ``defer_retry``
        that read is left to the caller, who must invoke the trailing callable (it returns the number of points redone)."""
        return self._weights_tile64("mia_letkf_weights_matfun_f64", "weights64", Yb, d, nbrs, inf_factor, rec, out, return_flags,
                                    defer_retry, rbf_gamma)

    # LETKF.estimate_weights_arrays hands float64 weights of ensembles above weights64's 64 members to weights_wide64 from this
    # ensemble size on (the project's rule: the smallest MEASURED k from which every measured case is at least 2x the Jacobi
    # kernel with W beyond both spreads, counter read included).  Measured on MI355X (tools/time_wide64w.py,
    # profiles/wide64w_time.json), 1e5 points, Jacobi kernel with W / weights_wide64 with the counter read: k 65 p 53
    # 4.53x (312.8 / 69.1 ms; worst round against best 4.51x), k 80 p 63 5.66x (417.7 / 73.8 ms; 5.65x); spreads at most 0.5 ms.
    # The gate is therefore the route's first ensemble size, 65.  NOT measured against the Jacobi kernel, because it answers
    # MIA_ERR_UNSUPPORTED with W there: k 96 p 81, k 128 p 97 and also k 128 p 62 (206.6 ms per 1e5 points, 116.1 and 107.5 ms per
    # 5e4 points on this route); no shape between 65 and 80 or 80 and 96 members, no list shorter than 53, was measured either.
    # Below 65 members letkf_weights64_kernel keeps the class route (k 64 p 57: 84.9 ms against 59.3 ms here, 1.43x, equal bits
    # -- a factor below the rule's 2); weights_wide64 itself stays available everywhere the kernel covers
    WEIGHTS_WIDE64_AUTO_MIN_K = 65

    def weights_wide64(self, Yb: Optional[torch.Tensor], d: Optional[torch.Tensor], nbrs: NeighbourLists,
                       inf_factor: float = 1.0, rec: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       return_flags: bool = False, defer_retry: bool = False, rbf_gamma: Optional[float] = None):
        """:meth:`weights64` for ensembles of up to 128 members (mia_letkf_weights_wide_f64, csrc/letkf_wide64w.hip): the same
        float64 weights W (n, k, k) with a tile's union split over two or four wavefronts, 2 <= k <= 128, p_max <= k, plain
        ETKF core; the same arguments and the same answers -- W [, flags (n,)] [, finish], or None where the entry answers
        MIA_ERR_UNSUPPORTED (any other shape, float32 input, ``rbf_gamma``, option tile = 0).  Points the kernel declines are
        redone by the Jacobi kernel (mia_letkf_weights_retry_f64) behind the 8-byte read of the decline counter; with
        ``defer_retry`` that read is left to the caller, who must invoke the trailing callable (it returns the number of points
        redone).  The Jacobi kernel holds about 70 local observations: a declined point with more makes the redo raise MiaError
        AFTER every other point has been written -- data-dependent, as ``analysis(method="wide64")`` documents for the analysis."""
        return self._weights_tile64("mia_letkf_weights_wide_f64", "weights_wide64", Yb, d, nbrs, inf_factor, rec, out, return_flags,
                                    defer_retry, rbf_gamma)

    # LETKF.estimate_weights_arrays hands float64 weights of DENSE networks (p_max > k, which weights64 and weights_wide64
    # refuse) to weights_stream64 in two cases.  (1) Wherever the Jacobi kernel cannot hold the shape (_jacobi_primal_fits: from
    # 97 members on; W adds no LDS to its primal form): there is nothing to compare with, the alternative is MiaError.
    # (2) Where the Jacobi kernel runs, from WEIGHTS_STREAM64_AUTO_MIN_K members on while WEIGHTS_STREAM64_AUTO_DEN * p_max <=
    # WEIGHTS_STREAM64_AUTO_NUM * k: the range in which every MEASURED case is at least 2x the Jacobi kernel with W beyond both
    # spreads, counter read included (tools/time_stream64w.py, profiles/stream64w_time.json).
    # Measured on MI355X, 1e5 points, Jacobi kernel with W on a build of the parent commit / this route with the counter read,
    # median ms: k 80 p 93 2.53x (1006.3 / 397.4), but k 65 p 77 1.63x (345.7 / 212.3), k 96 p 107 1.75x (1591.8 / 910.0),
    # k 80 p 173 0.71x (875.0 / 1228.7), k 96 p 173 0.84x (1363.6 / 1623.9); for information k 64 p 153 0.45x (255.1 / 569.4);
    # spreads at most 0.4 %.  The one case that passes the factor 2 lies between two that miss it (65 and 96 members at the same
    # p_max / k), so no range of ensemble sizes can be drawn from it: the constants admit NOTHING where the Jacobi kernel runs,
    # and the class takes the route from 97 members on only (k 128: 1064.8 ms at p 139 and 1714.2 ms at p 203 per 5e4 points,
    # where the parent raises MiaError).  weights_stream64 itself stays available everywhere the kernel covers
    WEIGHTS_STREAM64_AUTO_MIN_K = 129
    WEIGHTS_STREAM64_AUTO_NUM, WEIGHTS_STREAM64_AUTO_DEN = 0, 1

    def _weights_stream64_auto(self, k: int, p_max: int) -> bool:
        if k < 2 or k > 128 or p_max <= k or p_max > 256:
            return False
        if not self._jacobi_primal_fits(k, p_max):
            return True
        return (k >= max(self.WEIGHTS_STREAM64_AUTO_MIN_K, 65)
                and self.WEIGHTS_STREAM64_AUTO_DEN * p_max <= self.WEIGHTS_STREAM64_AUTO_NUM * k)

    def weights_stream64(self, Yb: Optional[torch.Tensor], d: Optional[torch.Tensor], nbrs: NeighbourLists,
                         inf_factor: float = 1.0, rec: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         return_flags: bool = False, defer_retry: bool = False, rbf_gamma: Optional[float] = None):
        """:meth:`weights_wide64` for DENSE local networks (mia_letkf_weights_stream_f64, csrc/letkf_stream64w.hip): the same
        float64 weights W (n, k, k) where a point sees more observations than there are members, 2 <= k <= 128,
        k < p_max <= 256, plain ETKF core, the union's records streamed as by ``analysis(method="stream64")``; the same
        arguments and the same answers -- W [, flags (n,)] [, finish], or None where the entry answers MIA_ERR_UNSUPPORTED (any
        other shape, p_max <= k included, float32 input, ``rbf_gamma``, option tile = 0).  Points the kernel declines are redone
        by the Jacobi kernel (mia_letkf_weights_retry_f64) behind the 8-byte read of the decline counter; with ``defer_retry``
        that read is left to the caller, who must invoke the trailing callable (it returns the number of points redone).  The
        Jacobi kernel cannot hold a dense point from 97 members on: a declined point there makes the redo raise MiaError AFTER
        every other point has been written -- data-dependent, as ``analysis(method="stream64")`` documents for the analysis.
        A point without observations gets sqrt(inf_factor) I exactly and flag 0."""
        return self._weights_tile64("mia_letkf_weights_stream_f64", "weights_stream64", Yb, d, nbrs, inf_factor, rec, out, return_flags,
                                    defer_retry, rbf_gamma)

    # LETKF(..., mesh_shape=...).estimate_weights_arrays hands float64 weights of DENSE networks to weights_patch64 with the
    # map of 4 x 4 patches where the census says every tile fits one pass (largest union <= 256), in two cases.  (a) Wherever
    # _weights_stream64_auto already says yes (from 97 members on): the bits are weights_stream64's, nothing is compared with
    # the Jacobi kernel.  (b) Where the Jacobi kernel runs: WEIGHTS_PATCH64_AUTO_MIN_K <= k <= WEIGHTS_PATCH64_AUTO_MAX_K and
    # WEIGHTS_PATCH64_AUTO_DEN * p_max <= WEIGHTS_PATCH64_AUTO_NUM * k -- the range in which every MEASURED case is at least 2x
    # the Jacobi kernel with W beyond both spreads, counter read included (tools/time_patch64w.py, profiles/patch64w_time.json,
    # DESIGN 9).  Measured on MI355X, 316 x 316 meshes (224 x 224 at k = 128) with an observation at every point, radius 3 (3.5),
    # p_max 101 (145), 4 x 4 patches, census (0.2 - 0.8 ms, first call only) outside, median ms, Jacobi kernel with W /
    # weights_stream64 without a map / this route:
    #   k  40:   80.3 /  853.3 /  226.2   0.35x the Jacobi kernel, LOSES      3.77x the route without a map
    #   k  64:  280.2 / 1977.7 /  403.9   0.69x, LOSES                        4.90x
    #   k  80: 1016.0 / 2630.1 /  770.3   1.32x, misses the factor 2          3.41x
    #   k  96: 1684.0 / 5091.1 / 1040.4   1.62x, misses the factor 2          4.89x
    #   k 128: MiaError / 6251.0 / 2426.7  (no Jacobi kernel)                 2.58x
    # (spreads at most 0.1 % on the tile routes; W and flags bit-identical to the route without a map in all five).  NO case
    # reaches 2x the Jacobi kernel, so the constants admit NOTHING where it runs: the class takes the map under (a) only, where
    # it is 2.58x the route the class ran before (k = 128).  NOT measured: other radii, observations at every second point,
    # ensembles between the measured sizes, 97 - 127 members.  weights_patch64 itself stays available everywhere the kernel covers
    WEIGHTS_PATCH64_AUTO_MIN_K, WEIGHTS_PATCH64_AUTO_MAX_K = 129, 0
    WEIGHTS_PATCH64_AUTO_NUM, WEIGHTS_PATCH64_AUTO_DEN = 0, 1
    WEIGHTS_PATCH64_MAX_BLOCKS = 16        # kPatch64WMaxBlocks (csrc/letkf_patch64w.hip): 256 slots at every ensemble size

    def _weights_patch64_auto(self, k: int, p_max: int) -> bool:
        if k < 2 or k > 128 or p_max <= k or p_max > 256:
            return False
        if self._weights_stream64_auto(k, p_max):
            return True
        return (self.WEIGHTS_PATCH64_AUTO_MIN_K <= k <= self.WEIGHTS_PATCH64_AUTO_MAX_K
                and self.WEIGHTS_PATCH64_AUTO_DEN * p_max <= self.WEIGHTS_PATCH64_AUTO_NUM * k)

    def weights_patch64(self, Yb: Optional[torch.Tensor], d: Optional[torch.Tensor], nbrs: NeighbourLists,
                        tile_points: torch.Tensor, inf_factor: float = 1.0, rec: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None, return_flags: bool = False, defer_retry: bool = False,
                        rbf_gamma: Optional[float] = None, union_blocks: Optional[int] = None):
        """:meth:`weights_stream64` with the sixteen points of a tile taken from ``tile_points`` (mia_letkf_weights_patch_f64,
        csrc/letkf_patch64w.hip): int32 (n_tiles, 16), a point's index relative to the shard's g0 or -1, every point exactly
        once -- :func:`mesh_tiles` builds the 4 x 4 patches of a 2-D mesh, whose unions fit one pass where sixteen consecutive
        points run in parts.  The same float64 weights W (n, k, k), 2 <= k <= 128, k < p_max <= 256, plain ETKF core, bit for
        bit weights_stream64's under any map; the same arguments and the same answers -- W [, flags (n,)] [, finish], or None
        where the route does not cover the shape or the entry answers MIA_ERR_UNSUPPORTED (any other shape, p_max <= k
        included, float32 input, ``rbf_gamma``, option tile = 0).  ``union_blocks``: sixteen-slot blocks of the slot tables, 1
        .. 16; None sizes them for the largest union of a tile, which the census of the map counts (one 8-byte read, kept on
        ``nbrs`` under the map's identity and shared with ``analysis(tile_points=...)``: an analysis and a weights call with
        the same lists and map pay one census); a tile whose union exceeds them runs in halves of its slots.  ValueError for
        a map that is not a partition of the shard's points, a wrong dtype or shape of it and ``union_blocks`` outside 1 ..
        16, before any launch.  Points the kernel declines are redone by the Jacobi kernel (mia_letkf_weights_retry_f64, from
        the lists in natural order) behind the 8-byte read of the decline counter; with ``defer_retry`` that read is left to
        the caller, who must invoke the trailing callable (it returns the number of points redone).  The Jacobi kernel cannot
        hold a dense point from 97 members on: a declined point there makes the redo raise MiaError AFTER every other point
        has been written -- data-dependent, the same raise as weights_stream64's.  A point without observations gets
        sqrt(inf_factor) I exactly and flag 0."""
        n = nbrs.g1 - nbrs.g0
        cap = self.WEIGHTS_PATCH64_MAX_BLOCKS
        if (not isinstance(tile_points, torch.Tensor) or tile_points.dtype != torch.int32 or tile_points.dim() != 2
                or tile_points.shape[1] != 16):
            raise ValueError("tile_points must be an int32 tensor (n_tiles, 16)")
        if union_blocks is not None and not 1 <= int(union_blocks) <= cap:
            raise ValueError("union_blocks must lie in 1 .. %d" % cap)

        def more(k):
            if n <= 0 or self.lib.mia_letkf_weights_patch_f64_cover(k, nbrs.p_max, n, rec.shape[0] if rec is not None else
                                                                    Yb.shape[1]) != 1:
                return None
            tp, ub, _ = self._patch64_map(nbrs, tile_points, union_blocks, k, cap)
            return (_ptr(tp), tp.shape[0], ub)
        return self._weights_tile64("mia_letkf_weights_patch_f64", "weights_patch64", Yb, d, nbrs, inf_factor, rec, out, return_flags,
                                    defer_retry, rbf_gamma, more)

    def weights_patch64_fits(self, nbrs: NeighbourLists, tile_points: torch.Tensor, k: int) -> bool:
        """Whether every tile of the map runs in ONE pass of weights_patch64 (largest union <= 256): the census, once per map."""
        return self._patch64_map(nbrs, tile_points, None, k, self.WEIGHTS_PATCH64_MAX_BLOCKS)[2]

    # ------------------------------------------------------------------- IEnKS
    # ienks_update(method="auto") hands float64 updates with tau = 1 to the tile kernel (csrc/lienks_tile64.hip) only from this
    # ensemble size on: the project's rule for WEIGHTS64_AUTO_MIN_K -- the smallest measured k at which the route, counter read
    # included, is at least 2x the general kernel (ienks_update_kernel<double, 256>) in BOTH variants.  Measured on MI355X
    # (tools/time_ienks64.py, profiles/ienks64_time.json), 1e5 points, bundle (per-point weights) / transform (shared prior):
    # k 40 p 20 3.27x (15.32 / 4.69 ms) / 7.65x (34.23 / 4.48 ms), k 64 p 31 5.60x (103.6 / 18.5 ms) / 12.7x (209.9 / 16.5 ms), but
    # k 20 p 10 only 1.76x (3.89 / 2.21 ms) in the bundle variant (transform 3.00x, 6.27 / 2.09 ms; spreads below 1 % everywhere).
    # The default therefore starts at the smallest measured k that passed in both; method="tile64" names the kernel everywhere it covers
    IENKS64_AUTO_MIN_K = 40
    # Above lienks_update64_kernel's 64 members, ienks_update(method="auto") hands float64 updates with tau = 1 to the wide tile
    # kernel (csrc/lienks_wide64.hip) from this ensemble size on.  The rule is the one above: the smallest MEASURED k >= 65 from
    # which every measured case, counter read included, is at least 2x the general kernel in BOTH variants, beyond both spreads.
    # Measured on MI355X (tools/time_ienks_wide64.py, profiles/ienks_wide64_time.json), 1e5 points, general kernel /
    # route with the counter read, bundle (per-point weights) and transform (shared prior): k 65 p 53 4.27x (287.5 / 67.4 ms) and
    # 6.14x (405.0 / 66.0 ms), k 80 p 63 bundle 5.20x (375.9 / 72.2 ms; the general kernel refuses the transform variant there),
    # k 80 p 20 5.84x (62.3 / 10.7 ms) and 24.9x (244.1 / 9.8 ms); worst round against best round at least 4.26x, spreads at
    # most 0.9 ms.  The gate is therefore the route's first ensemble size, 65.  NOT measured against the general kernel, because it
    # answers MIA_ERR_UNSUPPORTED there in both variants: k 96 p 81 (201.2 / 197.5 ms per 1e5 points on this route), k 128 p 97
    # (114.1 / 111.6 ms per 5e4 points) and k 128 p 62 (106.2 / 103.7 ms per 5e4 points); no shape between 65 and 80 or 80 and 96
    # members, and no list shorter than 20, was measured either.  Where the general kernel refuses a shape the route is taken
    # whatever this gate says.  Below 65 members lienks_update64_kernel keeps "auto" (k 64 p 57: 83.4 / 81.1 ms against 57.9 /
    # 56.6 ms here, 1.44x / 1.43x, equal bits -- a factor below the rule's 2); method="wide64" names the kernel everywhere it covers
    IENKS_WIDE64_AUTO_MIN_K = 65
    # The IEnKS classes (ienks.py) hand float64 updates with tau = 1 of DENSE networks (p_max > k, which the two tile kernels
    # above refuse) to method="stream64" (csrc/lienks_stream64.hip) in two cases.  (a) Wherever the general kernel cannot hold
    # the shape (_ienks_general_fits: with p_max = k + 1 the bundle variant from 80 members on, the transform variant from 69):
    # there is nothing to compare with, the alternative is MiaError.  (b) Where the general kernel runs, from
    # IENKS_STREAM64_AUTO_MIN_K members on while IENKS_STREAM64_AUTO_DEN * p_max <= IENKS_STREAM64_AUTO_NUM * k: the range in
    # which every MEASURED case is at least 2x the general kernel in the variants it holds, beyond both spreads, counter read
    # included (tools/time_ienks_stream64.py, profiles/ienks_stream64_time.json).
    # Measured on MI355X, 1e5 points, general kernel / this route with the counter read, median ms, bundle (per-point weights) and
    # transform (shared prior): k 65 p 77 3.06x (623.8 / 203.6) and 3.66x (743.1 / 202.8), k 72 p 77 bundle 2.74x (777.7 / 283.8;
    # the general kernel refuses the transform variant there); worst round against best round the same figures, spreads at most
    # 1.9 ms.  For information k 40 p 77: bundle 0.95x (95.5 / 100.9), transform 2.20x (221.0 / 100.4) -- below 65 members the
    # bundle variant loses, so the range starts at the smallest measured k from which every measured case passes, 65, and ends at
    # the largest measured p_max / k that passed, 77 / 65 (longer lists cost this kernel more than the general one: 2.19's k 80
    # p 173 was 0.71x the Jacobi kernel).  It is narrow by itself: with p_max = k + 1 the general kernel holds the bundle variant
    # up to 79 members and the transform variant up to 68.  NOT measured: any ensemble size between 65 and 72 or 72 and 79, any
    # p_max other than 77.  Where the general kernel refuses the shape (absolute times, same columns): k 80 p 93 382.6 / 381.6,
    # k 80 p 173 bundle 1178.4, k 96 p 107 bundle 881.9 ms per 1e5 points; k 128 p 139 1010.8 / 1009.0, k 128 p 203 bundle 1623.7 ms
    # per 5e4 points.  method="stream64" names the kernel everywhere it covers.
    # ienks_update(method="auto") itself is unchanged: the hand-over lives in the classes, as for estimate_weights_arrays
    IENKS_STREAM64_AUTO_MIN_K = 65
    IENKS_STREAM64_AUTO_NUM, IENKS_STREAM64_AUTO_DEN = 77, 65

    @staticmethod
    def _ienks_general_lds_bytes(k: int, p_max: int, tau: float, bundle: bool) -> int:
        """Restates the dynamic LDS of ienks_update_kernel<double, 256> as ienks_update_impl sizes it (csrc/ienks.hip)."""
        n, kp = (k + 1) & ~1, (k + 1 + 3) & ~3
        lda = n + 1
        nd = ((max(p_max, 1) + 1) & ~1) if (float(tau) == 1.0 and p_max <= k) else 0
        rows = nd if nd > 0 else max(p_max, 1)
        pl = (p_max + 3) & ~1
        e = 2 * n * lda + (1 if bundle else 2) * rows * kp + 5 * n + pl
        nbk = n // 2
        b = 8 * e + 4 * pl + 16 + 2 * ((nbk * (nbk - 1) // 2 + 7) & ~7) + 4 * ((n + 1) & ~1) + 8 * (256 // 64 * 2)
        return (b + 15) // 16 * 16

    @staticmethod
    def _ienks_general_fits(k: int, p_max: int, tau: float, bundle: bool) -> bool:
        """Whether the general float64 kernel can hold a point of this shape: where it cannot, mia_lienks_update_f64 answers
        MIA_ERR_UNSUPPORTED (k 72 p_max 77: bundle 136 384 bytes fits, transform 183 200 does not)."""
        return LetkfEngine._ienks_general_lds_bytes(k, p_max, tau, bundle) <= LetkfEngine.JACOBI_MAX_LDS

    def _ienks_stream64_auto(self, k: int, p_max: int, bundle: bool, shared: bool) -> bool:
        """Whether the classes name method="stream64" for a float64 update with tau = 1 (checked by the caller, like the
        entry's cover): ``bundle`` = bundle variant, ``shared`` = ONE (k, k) weight matrix for all points."""
        if k < 2 or k > 128 or p_max <= k or p_max > 256:
            return False
        if not (bundle or shared):        # per-point transform weights have Wp != I: the launch would be declined whole
            return False
        if not self._ienks_general_fits(k, p_max, 1.0, bundle):
            return True
        return (k >= self.IENKS_STREAM64_AUTO_MIN_K
                and self.IENKS_STREAM64_AUTO_DEN * p_max <= self.IENKS_STREAM64_AUTO_NUM * k)

    # LocalizedIEnKS*(..., mesh_shape=...).inner_loop_arrays hands float64 updates with tau = 1 of DENSE networks to
    # method="patch64" (csrc/lienks_patch64.hip) with the map of 4 x 4 patches, in two cases.  (a) Wherever
    # _ienks_stream64_auto already says yes: those calls run lienks_stream64_kernel without the map, and the bits are equal
    # under any map.  (b) Where the general kernel runs and is the default: IENKS_PATCH64_AUTO_MIN_K <= k <=
    # IENKS_PATCH64_AUTO_MAX_K and IENKS_PATCH64_AUTO_DEN * p_max <= IENKS_PATCH64_AUTO_NUM * k -- the range in which every
    # MEASURED case is at least 2x the general kernel in the variants it holds, beyond both spreads, counter read included
    # (tools/time_ienks_patch64.py, profiles/ienks_patch64_time.json).
    # Measured on MI355X, 316 x 316 meshes (224 x 224 at k = 128) with an observation at every point, radius 3 (3.5), p_max 101
    # (145), 4 x 4 patches (largest union 176 / 232), census (0.7 - 0.9 ms, first call only) outside, five rounds, the methods
    # alternating, counter read included, median ms; general kernel and method="stream64" on a build of the PARENT commit /
    # method="stream64" on this build / this route; bundle (per-point weights) and transform (shared prior):
    #   k  40 bundle:     97.9 /  823.3 /  822.5 /  216.5   0.45x the general kernel, LOSES     3.80x the route without a map
    #   k  40 transform: 225.7 /  822.6 /  822.4 /  215.8   1.05x, misses the factor 2           3.81x
    #   k  64 bundle:    490.3 / 1899.8 / 1901.2 /  388.4   1.26x, misses the factor 2           4.89x
    #   k  64 transform:    -3 / 1899.6 / 1898.7 /  387.7   (the general kernel refuses)         4.90x
    #   k  80 bundle / transform:  -3 / 2544.4, 2542.7 / 2542.4, 2543.4 /  751.3,  748.3         3.39x, 3.40x
    #   k  96 bundle / transform:  -3 / 4928.7, 4927.1 / 4934.3, 4932.3 / 1004.8, 1002.9         4.91x, 4.91x
    #   k 128 bundle / transform:  -3 / 5995.0, 5992.8 / 6000.4, 5994.9 / 2343.9, 2340.4         2.56x, 2.56x
    # (spreads at most 0.6 % of a median; method="stream64" agrees between the two builds within its spreads in all ten; W and
    # flags bit-identical to the route without a map in all ten; nothing declined).  (a) In every one of the ten cases the slowest
    # round of this route is below the fastest round of the parent's method="stream64", so no shape of that range is excluded.
    # (b) NO case with a baseline reaches 2x the general kernel (0.45x, 1.05x, 1.26x), so the constants admit NOTHING where the
    # general kernel is the default: the classes take the map under (a) only.  NOT measured: other radii, observations at every
    # second point, ensembles between the measured sizes, the range of IENKS_STREAM64_AUTO_* where the general kernel runs (k 65 -
    # 79 with p_max <= 77 / 65 k: taken under (a) on the strength of the cases above).  method="patch64" itself stays available
    # everywhere the kernel covers
    IENKS_PATCH64_AUTO_MIN_K, IENKS_PATCH64_AUTO_MAX_K = 129, 0
    IENKS_PATCH64_AUTO_NUM, IENKS_PATCH64_AUTO_DEN = 0, 1

    def _ienks_patch64_auto(self, k: int, p_max: int, bundle: bool, shared: bool) -> bool:
        """Whether the classes name method="patch64" on a ``mesh_shape`` for a float64 update with tau = 1 (checked by the
        caller, like the entry's cover); arguments as :meth:`_ienks_stream64_auto`."""
        if k < 2 or k > 128 or p_max <= k or p_max > 256:
            return False
        if not (bundle or shared):        # per-point transform weights have Wp != I: the launch would be declined whole
            return False
        if self._ienks_stream64_auto(k, p_max, bundle, shared):
            return True
        return (self.IENKS_PATCH64_AUTO_MIN_K <= k <= self.IENKS_PATCH64_AUTO_MAX_K
                and self.IENKS_PATCH64_AUTO_DEN * p_max <= self.IENKS_PATCH64_AUTO_NUM * k)

    # the float64 tile kernels of ienks_update: method -> (C entry, its cover function, the cover in words, the ensemble size
    # from which "auto" takes it -- None: never at this level).  "auto" tries them in this order
    IENKS_TILE64_ROUTES = {
        "tile64": ("mia_lienks_update_matfun_f64", "mia_lienks_update_f64_cover", "2 <= k <= 64 and p_max <= k",
                   "IENKS64_AUTO_MIN_K"),
        "wide64": ("mia_lienks_update_wide_f64", "mia_lienks_update_wide_f64_cover", "2 <= k <= 128 and p_max <= k",
                   "IENKS_WIDE64_AUTO_MIN_K"),
        "stream64": ("mia_lienks_update_stream_f64", "mia_lienks_update_stream_f64_cover",
                     "2 <= k <= 128 and k < p_max <= 256", None),
        "patch64": ("mia_lienks_update_patch_f64", "mia_lienks_update_patch_f64_cover",
                    "2 <= k <= 128 and k < p_max <= 256", None)}
    IENKS_TILE64_METHODS = tuple(IENKS_TILE64_ROUTES)
    IENKS_METHODS = ("auto", "eig") + IENKS_TILE64_METHODS
    # what the two messages below name: the methods that take no further argument ("patch64" needs tile_points and has a
    # message of its own)
    IENKS_PLAIN_TILE64_METHODS = tuple(m for m in IENKS_TILE64_METHODS if m != "patch64")

    def ienks_update(self, weights: torch.Tensor, Yb: Optional[torch.Tensor], d: Optional[torch.Tensor],
                     nbrs: NeighbourLists, tau: float = 1.0, epsilon: Optional[float] = None,
                     rec: Optional[torch.Tensor] = None, return_flags: bool = False, method: str = "auto",
                     defer_retry: bool = False, out: Optional[torch.Tensor] = None,
                     tile_points: Optional[torch.Tensor] = None, union_blocks: Optional[int] = None):
        """One IEnKS weight update per grid point of the shard ``nbrs`` (core/ienks.py:108-141 on the localised
        block, interface/lienks.py:75-118).  ``weights``: (k, k) shared by all points (e.g. the prior weights) or
        (n, k, k); ``epsilon`` None = transform variant, a positive value = bundle variant.  Returns (n, k, k).
        ``method`` "auto": float32 updates with tau = 1 go through the eigensolver-free weights kernel (bundle variant
        always, transform variant while Wp = I), the general kernel redoing what it declines; float64 updates with tau = 1 go
        through the tile kernel of csrc/lienks_tile64.hip where mia_lienks_update_f64_cover says yes (2 <= k <= 64, p_max <= k),
        k >= IENKS64_AUTO_MIN_K, and the variant is bundle or the weights are ONE shared (k, k) matrix (per-point weights of the
        transform variant have Wp != I everywhere: the launch would be declined whole); above 64 members, under the same
        variant condition, through the wide tile kernel of csrc/lienks_wide64.hip where mia_lienks_update_wide_f64_cover says
        yes (2 <= k <= 128, p_max <= k) and k >= IENKS_WIDE64_AUTO_MIN_K -- and, whatever that gate says, where the general
        kernel answers MIA_ERR_UNSUPPORTED because its LDS cannot hold the shape.  "tile64" / "wide64": those kernels by name
        (ValueError outside float64, tau = 1 and the kernel's cover); "stream64": the tile kernel for DENSE local networks
        (csrc/lienks_stream64.hip, 2 <= k <= 128 and k < p_max <= 256; the same ValueErrors), which "auto" never takes at this
        level -- the IEnKS classes name it where :meth:`_ienks_stream64_auto` says so; "patch64": that kernel with the sixteen
        points of a tile taken from ``tile_points`` (csrc/lienks_patch64.hip, mia_lienks_update_patch_f64; the same cover and
        ValueErrors): int32 (n_tiles, 16), a point's index relative to the shard's g0 or -1, every point exactly once --
        :func:`mesh_tiles` builds the 4 x 4 patches of a 2-D mesh, whose unions fit one pass where sixteen consecutive points
        run in parts.  W and flags are "stream64"'s bit for bit under any map.  ``union_blocks``: sixteen-slot blocks of the
        slot tables, 1 .. 16; None sizes them for the largest union of a tile, which the census of the map counts (one 8-byte
        read, kept on ``nbrs`` under the map's identity and shared with ``analysis(tile_points=...)`` and ``weights_patch64``);
        a tile whose union exceeds them runs in halves of its slots.  ValueError for method="patch64" without ``tile_points``,
        for ``tile_points`` / ``union_blocks`` with any other method, for a map that is not a partition of the shard's points,
        a wrong dtype or shape of it and ``union_blocks`` outside 1 .. 16, before any launch; "auto" never takes the route at
        this level -- the IEnKS classes name it on a ``mesh_shape`` where :meth:`_ienks_patch64_auto` says so; "eig": general
        kernel.  Points a tile kernel declines are
        redone by the general kernel (mia_lienks_update_retry_f64) behind the 8-byte read of the decline counter; where the
        general kernel cannot hold a declined point's shape that redo raises MiaError AFTER every other point has been
        written -- data-dependent, as ``weights_wide64`` documents.  With ``defer_retry`` (the named tile methods only)
        the read is left to the caller, who must invoke the trailing callable of the result (it returns the number of points
        redone).  ``out``: a contiguous (n, k, k) tensor of the weights' dtype to write into."""
        tile_methods = self.IENKS_TILE64_METHODS
        if method not in self.IENKS_METHODS:
            raise ValueError("method must be " + _one_of(("auto", "eig") + self.IENKS_PLAIN_TILE64_METHODS))
        if defer_retry and method not in tile_methods:
            raise ValueError("defer_retry needs method=" + _one_of(self.IENKS_PLAIN_TILE64_METHODS))
        if method == "patch64":
            if tile_points is None:
                raise ValueError("the patch64 route needs tile_points (see mesh_tiles)")
            if (not isinstance(tile_points, torch.Tensor) or tile_points.dtype != torch.int32 or tile_points.dim() != 2
                    or tile_points.shape[1] != 16):
                raise ValueError("tile_points must be an int32 tensor (n_tiles, 16)")
            if union_blocks is not None and not 1 <= int(union_blocks) <= self.WEIGHTS_PATCH64_MAX_BLOCKS:
                raise ValueError("union_blocks must lie in 1 .. %d" % self.WEIGHTS_PATCH64_MAX_BLOCKS)
        elif tile_points is not None or union_blocks is not None:
            raise ValueError("tile_points and union_blocks belong to method='patch64' (method='%s')" % method)
        weights = torch.as_tensor(weights)
        dtype = weights.dtype if weights.dtype in (torch.float32, torch.float64) else torch.float64
        weights = weights.to(device=self.device, dtype=dtype).contiguous()
        k = weights.shape[-1]
        n = nbrs.g1 - nbrs.g0
        if weights.shape[-2] != k or weights.dim() not in (2, 3) or (weights.dim() == 3 and weights.shape[0] != n):
            raise ValueError("weights must be (k, k) or (n, k, k) with n the number of grid points of the shard")
        if rec is None:
            if Yb.dim() != 2 or Yb.shape[0] != k:
                raise ValueError("Yb must be (k, P) with the weights' ensemble size")
            rec = self.pack_obs(Yb, d, dtype)
        if rec.dtype != dtype or rec.shape[1] != (k + 1 + 3) // 4 * 4:
            raise ValueError("packed records do not match the weights' dtype / ensemble size")
        if not 0.0 <= float(tau) <= 1.0:
            raise ValueError("tau must lie in [0, 1]")           # bound_tensor(0, 1), interface/ienks.py:82-86
        if epsilon is not None and not float(epsilon) > 0.0:
            raise ValueError("epsilon must be positive")
        if out is None:
            out = torch.empty((n, k, k), dtype=dtype, device=self.device)
        elif out.shape != (n, k, k) or out.dtype != dtype or not out.is_contiguous() or out.device != weights.device:
            raise ValueError("out must be a contiguous tensor (n, k, k) of the weights' dtype on the engine's device")
        flags = torch.empty(n, dtype=torch.int32, device=self.device)
        sfx = "f32" if dtype == torch.float32 else "f64"
        eps_c = float(epsilon) if epsilon is not None else 0.0
        # every entry's arguments, built once: a tile entry takes (*head, *tail, retry_count, stream), the general kernel and
        # the redo entries (*head, tau, *tail, stream)
        head = (_ptr(weights), k * k if weights.dim() == 3 else 0, k, nbrs.g0, nbrs.g1, _ptr(rec), rec.shape[0], _ptr(nbrs.cnt),
                _ptr(nbrs.idx), _ptr(nbrs.w), nbrs.p_cap, nbrs.p_max)
        tail = (eps_c, _ptr(out), _ptr(flags))
        cover_args = (k, min(nbrs.p_max, nbrs.p_cap), n, rec.shape[0])

        def tile_route(entry, extra=()):
            """The tile kernel behind ``entry`` and the redo of what it declines; None where the entry answers -3.  ``extra``: the
            entry's further arguments in front of the stream (patch64's map, number of tiles and blocks)."""
            retry = torch.zeros(1, dtype=torch.int32, device=self.device)
            rc = getattr(self.lib, entry)(*head, *tail, _ptr(retry), *extra, self._stream())
            if rc == -3:
                return None
            _cabi.check(rc, entry)
            # (the general kernel redoes the declined points)
            finish = self._redo_behind_counter(retry, "mia_lienks_update_retry_" + sfx, lambda: (*head, 1.0, *tail),
                                               (weights, rec, nbrs, out, flags))
            return _result(out, None, flags if return_flags else None, finish, defer_retry)
        f64_tau1 = dtype == torch.float64 and float(tau) == 1.0 and n > 0
        # (per-point weights of the transform variant have Wp != I everywhere: a tile launch would be declined whole)
        variant_ok = epsilon is not None or weights.dim() == 2
        entry, extra = None, ()
        if method in tile_methods:
            if dtype != torch.float64:
                raise ValueError("method='%s' needs float64 weights (float32 has its own route under 'auto')" % method)
            if float(tau) != 1.0:
                raise ValueError("method='%s' needs tau = 1 (tau = %g)" % (method, float(tau)))
            entry, cover, text, _ = self.IENKS_TILE64_ROUTES[method]
            if not getattr(self.lib, cover)(*cover_args):
                raise ValueError("method='%s' covers %s (k = %d, p_max = %d)" % (method, text, k, nbrs.p_max))
            if method == "patch64":
                # the map: validated (ValueError) and sized by the census, once per (lists, map), before any launch
                extra = (None, 0, 1)
                if n > 0:
                    tp, ub, _ = self._patch64_map(nbrs, tile_points, union_blocks, k, self.WEIGHTS_PATCH64_MAX_BLOCKS)
                    extra = (_ptr(tp), tp.shape[0], ub)
        elif dtype == torch.float32 and float(tau) == 1.0 and n > 0 and method != "eig":
            # tau = 1 through the eigensolver-free weights kernel; -3 = shape outside it (primal route, order > 32)
            res = tile_route("mia_lienks_update_matfun_f32")
            if res is not None:
                return res
        elif method == "auto" and f64_tau1 and variant_ok:
            for name, cover, _, min_k in self.IENKS_TILE64_ROUTES.values():
                if min_k is not None and k >= getattr(self, min_k) and getattr(self.lib, cover)(*cover_args):
                    entry = name
                    break
        if entry is not None:
            res = tile_route(entry, extra)
            if res is not None:
                return res
            if method in tile_methods:
                raise ValueError("method='%s': the tile kernel is not available (option tile = 0, or the stream is being "
                                 "captured before the coefficient table exists)" % method)
        rc = getattr(self.lib, "mia_lienks_update_" + sfx)(*head, float(tau), *tail, self._stream())
        wide, wide_cover = self.IENKS_TILE64_ROUTES["wide64"][:2]
        if (rc == -3 and method == "auto" and f64_tau1 and variant_ok and entry != wide
                and getattr(self.lib, wide_cover)(*cover_args)):
            # the general kernel cannot hold the shape (its LDS): the wide tile kernel can, whatever the gate says
            res = tile_route(wide)
            if res is not None:
                return res
        _cabi.check(rc, "mia_lienks_update_" + sfx)
        return (out, flags) if return_flags else out

    def apply_local_weights(self, X: torch.Tensor, W: torch.Tensor, g0: int = 0, g1: Optional[int] = None) -> torch.Tensor:
        """_apply_weights with per-grid-point weights W (g1-g0, k, k) (interface/base.py:257-278)."""
        if X.dim() == 2:
            X = X[None]
        X = X.to(self.device).contiguous()
        m, k, G = X.shape
        g1 = G if g1 is None else g1
        W = W.to(device=self.device, dtype=X.dtype).contiguous()
        if W.shape != (g1 - g0, k, k):
            raise ValueError("weights must be (grid, ensemble, ensemble_new) = (%d, %d, %d)" % (g1 - g0, k, k))
        out = torch.empty((m, k, g1 - g0), dtype=X.dtype, device=self.device)
        sfx = "f32" if X.dtype == torch.float32 else "f64"
        fn = getattr(self.lib, "mia_apply_local_weights_" + sfx)
        _cabi.check(fn(_ptr(X), G, m, k, g0, g1, _ptr(W), _ptr(out), g1 - g0, 0, self._stream()),
                    "mia_apply_local_weights_" + sfx)
        return out

    # ------------------------------------------------------------- global ETKF
    def etkf_weights(self, Yb: torch.Tensor, d: torch.Tensor, inf_factor: float = 1.0, return_flags: bool = False):
        """Global ETKF weights (k, k) (ETKFModule on the full block, core/etkf.py:79-103), 2 <= k <= 256
        (mia_etkf_weights_*).  ``return_flags``: also return the int32 flag word of the solve (one entry on the
        device; MIA_FLAG_NOCONV when the eigensolver reached its sweep cap)."""
        Yb = Yb.to(self.device).contiguous()
        dtype = Yb.dtype
        d = d.to(device=self.device, dtype=dtype).contiguous().reshape(-1)
        k, P = Yb.shape
        if d.shape[0] != P:
            raise ValueError(
                "Observational size between ensemble ({0:d}) and observations ({1:d}) do not match!".format(
                    P, d.shape[0]))
        eb = 4 if dtype == torch.float32 else 8
        nbytes = C.c_size_t(0)
        _cabi.check(self.lib.mia_etkf_workspace_bytes(k, P, eb, C.byref(nbytes)), "etkf_workspace_bytes")
        ws = self._workspace("etkf", nbytes.value)
        W = torch.empty((k, k), dtype=dtype, device=self.device)
        flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        sfx = "f32" if dtype == torch.float32 else "f64"
        fn = getattr(self.lib, "mia_etkf_weights_" + sfx)
        _cabi.check(fn(_ptr(Yb), _ptr(d), k, P, float(inf_factor), _ptr(W), _ptr(flags), _ptr(ws), ws.numel(),
                       self._stream()), "mia_etkf_weights_" + sfx)
        return (W, flags) if return_flags else W

    def ketkf_weights(self, Yb: torch.Tensor, d: torch.Tensor, kernel_program, inf_factor: float = 1.0,
                      return_flags: bool = False):
        """Global kernelised ETKF weights (k, k) for ANY number of observations and 2 <= k <= 256 (KETKFModule on the
        full block, core/ketkf.py:65-94): pair statistics accumulated over observation chunks, then one k x k solve.
        ``return_flags`` as in :meth:`etkf_weights`."""
        Yb = Yb.to(self.device).contiguous()
        dtype = Yb.dtype if Yb.dtype in (torch.float32, torch.float64) else torch.float64
        Yb = Yb.to(dtype)
        d = d.to(device=self.device, dtype=dtype).contiguous().reshape(-1)
        k, P = Yb.shape
        if d.shape[0] != P:
            raise ValueError(
                "Observational size between ensemble ({0:d}) and observations ({1:d}) do not match!".format(
                    P, d.shape[0]))
        nops = len(kernel_program)
        prog = (_cabi.KernelOp * max(nops, 1))()
        for i, (op, val) in enumerate(kernel_program):
            prog[i].op, prog[i].value = int(op), float(val)
        eb = 4 if dtype == torch.float32 else 8
        nbytes = C.c_size_t(0)
        _cabi.check(self.lib.mia_ketkf_workspace_bytes(k, P, eb, C.byref(nbytes)), "ketkf_workspace_bytes")
        ws = self._workspace("ketkf", nbytes.value)
        W = torch.empty((k, k), dtype=dtype, device=self.device)
        flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        sfx = "f32" if dtype == torch.float32 else "f64"
        fn = getattr(self.lib, "mia_ketkf_weights_" + sfx)
        _cabi.check(fn(_ptr(Yb), _ptr(d), k, P, float(inf_factor), prog, nops, _ptr(W), _ptr(flags), _ptr(ws), ws.numel(),
                       self._stream()), "mia_ketkf_weights_" + sfx)
        return (W, flags) if return_flags else W

    def apply_weights(self, X: torch.Tensor, W: torch.Tensor, g0: int = 0, g1: Optional[int] = None) -> torch.Tensor:
        if X.dim() == 2:
            X = X[None]
        X = X.to(self.device).contiguous()
        m, k, G = X.shape
        g1 = G if g1 is None else g1
        W = W.to(device=self.device, dtype=X.dtype).contiguous()
        out = torch.empty((m, k, g1 - g0), dtype=X.dtype, device=self.device)
        sfx = "f32" if X.dtype == torch.float32 else "f64"
        fn = getattr(self.lib, "mia_apply_weights_" + sfx)
        _cabi.check(fn(_ptr(X), G, m, k, g0, g1, _ptr(W), _ptr(out), g1 - g0, 0, self._stream()),
                    "mia_apply_weights_" + sfx)
        return out

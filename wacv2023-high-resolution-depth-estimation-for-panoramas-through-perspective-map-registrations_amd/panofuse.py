"""Python host binding of libpanofuse (include/panofuse.h) over ctypes.

This is the host-side mirror of the reference's DepthNamespace entry points for the fused path
(``Depth.h:286-307``): ``Fuser.register`` ~ SolveDepthToDepth + Depth2DepthTransform,
``Fuser.fuse`` ~ SolveDepthAll, ``Fuser.merge`` ~ MergeDepthMaps' compute core.  Tensors are
torch device tensors (PyTorch is used only for device memory and streams); the compute is the
hand-written HIP in csrc/.  There is no CPU fallback: if lib/libpanofuse.so is missing or no GPU
is present, every call raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# PANOFUSE_LIB selects another build of the same library (A/B tuning runs, tools/gpu_round.sh (ab step))
LIB_PATH = os.environ.get("PANOFUSE_LIB") or os.path.join(HERE, "lib", "libpanofuse.so")

PF_OK, PF_EINVAL, PF_ENOMEM, PF_EHIP, PF_ESTATE, PF_EDEGENERATE = 0, -1, -2, -3, -4, -5
PF_ETIMEOUT = -6  # a resident-kernel hand-off wait timed out: that fusion's output is invalid

# Every symbol declared in include/panofuse.h.
EXPORTS = [
    "pf_create", "pf_destroy", "pf_last_error", "pf_set_stream", "pf_synchronize",
    "pf_version", "pf_set_tiles", "pf_register", "pf_fuse", "pf_merge", "pf_warp_depth",
    "pf_warp_rgb", "pf_level_info", "pf_fuse_partial", "pf_fuse_seed", "pf_fuse_finish_level",
    "pf_probe_taps", "pf_profile_enable", "pf_profile_read", "pf_error_metrics",
    "pf_depth_transform", "pf_register_joint", "pf_set_solver", "pf_fuse_normalize",
    "pf_fuse_border", "pf_fuse_band_plan", "pf_fuse_band_pass", "pf_fuse_multicover",
    "pf_fuse_multicover_patch", "pf_solve_smoothing", "pf_set_metrics_order",
    "pf_jres_errors", "pf_set_jacobi_engine", "pf_stream_wait_level", "pf_debug_jres_fault",
    "pf_probe_warp_coords", "pf_probe_rgb_taps", "pf_debug_smooth_fault",
    "pf_fuse_partial_rows", "pf_fuse_coverage_rows", "pf_fuse_normalize_rows",
    "pf_fuse_tile_rows", "pf_rows_add", "pf_fuse_level", "pf_fuse_targets",
    "pf_rows_add_batch", "pf_set_jacobi_share", "pf_error_laplacian",
    "pf_error_compare", "pf_disp_depth_convert", "pf_register_disparity",
    "pf_disparity_transform", "pf_merge_disparity", "pf_register_global",
    "pf_result_transform", "pf_median_scale", "pf_copy_invalid", "pf_layout_audit",
    "pf_stitch", "pf_laplacian_residual", "pf_fuse_check", "pf_set_tile_validity",
    "pf_tile_valid_counts", "pf_set_register_loss", "pf_register_ex",
    "pf_set_tile_depth", "pf_tile_ray_tables", "pf_tile_ray_factor",
    "pf_overlap_pairs", "pf_overlap_table", "pf_overlap_stats", "pf_register_consistent",
    "pf_tile_tent_weights", "pf_register_weighted", "pf_fuse_weighted", "pf_merge_weighted",
    "pf_tile_range_weights", "pf_register_disparity_weighted", "pf_merge_disparity_weighted",
]
NEW_R4 = {"pf_debug_jres_fault", "pf_probe_warp_coords", "pf_probe_rgb_taps",
          "pf_debug_smooth_fault", "pf_fuse_partial_rows", "pf_fuse_coverage_rows",
          "pf_fuse_normalize_rows", "pf_fuse_tile_rows", "pf_rows_add", "pf_fuse_level",
          "pf_fuse_targets", "pf_rows_add_batch", "pf_set_jacobi_share"}
METRICS_ORDERS = {"tree": 0, "sequential": 1}  # PF_METRICS_*; "sequential" = the reference's
SOLVERS = {"normal": 0, "lm": 1}  # PF_SOLVER_*; "lm" = the reference's Ceres LM (default)
PF_VALID_ALL, PF_VALID_RANGE = 0, 1  # pf_set_tile_validity's modes
LOSSES = {None: 0, "none": 0, "huber": 1, "softl1": 2}  # PF_LOSS_* of pf_set_register_loss
TILE_DEPTHS = {None: 0, "ray": 0, "planar": 1}  # PF_TILE_DEPTH_* of pf_set_tile_depth

STAGES = ["warp", "register", "seed", "targets", "jacobi", "quantize", "metrics"]


class PanofuseError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"panofuse error {code}: {msg}")
        self.code = code


class Window(C.Structure):
    _fields_ = [("az_left", C.c_float), ("az_right", C.c_float),
                ("zen_top", C.c_float), ("zen_down", C.c_float)]


class LevelAudit(C.Structure):
    """pf_level_audit (include/panofuse.h)."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("h0", C.c_int), ("h1", C.c_int),
                ("taps_outside", C.c_longlong), ("taps_clamped", C.c_longlong),
                ("covered", C.c_longlong), ("uncovered_interior", C.c_longlong),
                ("max_cover", C.c_int), ("seam", C.c_int)]


class Response(C.Structure):
    _fields_ = [("alpha", C.c_float), ("kappa", C.c_float), ("beta", C.c_float),
                ("sigma", C.c_float), ("seed", C.c_uint32), ("pad", C.c_uint32)]


_lib = None


def load():
    """Load libpanofuse.so; raises if it was not built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libpanofuse.so not built at {LIB_PATH}: run "
                           f"`python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, fp, ip = C.c_void_p, C.c_float, C.c_int
    L.pf_create.argtypes = [ip, C.POINTER(vp)]
    L.pf_destroy.argtypes = [vp]
    L.pf_destroy.restype = None
    L.pf_last_error.argtypes = [vp]
    L.pf_last_error.restype = C.c_char_p
    L.pf_set_stream.argtypes = [vp, vp]
    L.pf_synchronize.argtypes = [vp]
    L.pf_version.restype = C.c_char_p
    L.pf_set_tiles.argtypes = [vp, C.POINTER(Window), C.POINTER(Window), ip,
                               C.POINTER(C.c_int), C.POINTER(C.c_int), ip, ip]
    L.pf_register.argtypes = [vp, vp, ip, ip, ip, vp, ip, fp, fp, ip, ip, vp, vp]
    L.pf_fuse.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, ip, fp, fp, vp]
    L.pf_merge.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, fp, fp, vp, vp]
    L.pf_warp_depth.argtypes = [vp, vp, ip, ip, ip, vp, vp]
    L.pf_warp_rgb.argtypes = [vp, vp, ip, ip, ip, vp]
    L.pf_solve_smoothing.argtypes = [vp, vp, vp, ip, ip, ip, fp, fp, vp]
    L.pf_stitch.argtypes = [vp, vp, vp, ip, ip, ip, vp]
    L.pf_laplacian_residual.argtypes = [vp, vp, vp, ip, ip, ip, ip, ip, vp]
    L.pf_fuse_check.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, fp, fp, vp, vp]
    L.pf_set_metrics_order.argtypes = [vp, ip]
    L.pf_level_info.argtypes = [ip, ip, fp, fp, ip] + [C.POINTER(C.c_int)] * 6
    L.pf_fuse_partial.argtypes = [vp, vp, vp, ip, ip, ip, ip, fp, fp, ip, vp, vp]
    L.pf_fuse_seed.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, fp, fp, ip, vp]
    L.pf_fuse_finish_level.argtypes = [vp, vp, vp, ip, ip, fp, fp, ip, vp, vp]
    L.pf_probe_taps.argtypes = [vp, ip, ip, fp, fp, ip, vp]
    L.pf_layout_audit.argtypes = [vp, ip, ip, fp, fp, ip, C.POINTER(LevelAudit)]
    L.pf_depth_transform.argtypes = [vp, vp, C.c_longlong, ip, vp]
    L.pf_register_joint.argtypes = [vp, vp, ip, ip, ip, vp, ip, fp, fp, ip, vp, vp, vp]
    L.pf_error_metrics.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, ip, ip, fp, fp, ip, ip,
                                   vp]
    L.pf_error_laplacian.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, ip, ip, vp, vp, vp, vp]
    L.pf_error_compare.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, ip, ip, fp, fp, ip, ip, ip, vp,
                                   vp, vp]
    L.pf_disp_depth_convert.argtypes = [vp, vp, C.c_longlong, ip]
    L.pf_register_disparity.argtypes = [vp, vp, ip, ip, ip, vp, ip, fp, fp, ip, vp, vp, vp]
    L.pf_disparity_transform.argtypes = [vp, vp, C.c_longlong, ip, C.POINTER(C.c_float)]
    L.pf_merge_disparity.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, fp, fp, vp, vp]
    L.pf_register_global.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, ip, fp, fp, ip, vp, vp, vp]
    L.pf_result_transform.argtypes = [vp, vp, ip, ip, ip, fp, fp, vp]
    L.pf_median_scale.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, ip, ip, vp, vp]
    L.pf_copy_invalid.argtypes = [vp, vp, ip, ip, ip, vp, ip, ip, ip, ip]
    L.pf_set_solver.argtypes = [vp, ip]
    L.pf_set_tile_validity.argtypes = [vp, ip, fp, fp]
    L.pf_tile_valid_counts.argtypes = [vp, vp, vp, ip, ip, ip, ip, fp, fp, vp]
    L.pf_set_register_loss.argtypes = [vp, ip, C.c_double]
    L.pf_register_ex.argtypes = [vp, vp, ip, ip, ip, vp, ip, fp, fp, ip, ip, vp, vp, vp]
    L.pf_set_tile_depth.argtypes = [vp, ip]
    L.pf_tile_ray_tables.argtypes = [vp, ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pf_tile_ray_factor.argtypes = [vp, vp]
    L.pf_overlap_pairs.argtypes = [vp, fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    L.pf_overlap_table.argtypes = [vp, fp, fp, vp, vp]
    L.pf_overlap_stats.argtypes = [vp, vp, vp, ip, fp, fp, vp]
    L.pf_register_consistent.argtypes = [vp, vp, ip, ip, ip, vp, ip, fp, fp, C.c_double, ip, vp,
                                         vp, vp]
    L.pf_tile_tent_weights.argtypes = [vp, vp]
    L.pf_register_weighted.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, fp, fp, ip, vp, vp, vp]
    L.pf_fuse_weighted.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, vp, ip, ip, ip, fp, fp, vp]
    L.pf_merge_weighted.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, ip, fp, fp, vp, vp]
    L.pf_tile_range_weights.argtypes = [vp, vp, ip, fp, fp, vp]
    L.pf_register_disparity_weighted.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, fp, fp, ip,
                                                 vp, vp, vp]
    L.pf_merge_disparity_weighted.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, ip, ip, fp, fp, vp,
                                              vp]
    L.pf_fuse_normalize.argtypes = [vp, vp, vp, ip, ip, fp, fp, ip, vp]
    L.pf_fuse_multicover.argtypes = [vp, vp, vp, ip, ip, ip, ip, fp, fp, ip, vp,
                                     C.POINTER(C.c_int)]
    L.pf_fuse_multicover_patch.argtypes = [vp, ip, ip, fp, fp, ip, vp, vp]
    L.pf_fuse_border.argtypes = [vp, vp, ip, ip, fp, fp, ip, vp, vp, vp]
    L.pf_fuse_band_plan.argtypes = [vp, ip, ip, fp, fp, ip, ip, C.POINTER(C.c_int), ip]
    L.pf_fuse_band_pass.argtypes = [vp, vp, ip, ip, ip, vp, vp, ip, vp, vp, vp, ip, ip, fp, fp,
                                    ip, ip, ip, ip]
    L.pf_profile_enable.argtypes = [vp, ip]
    L.pf_jres_errors.argtypes = [vp]
    # (entry points added after round 3: an A/B variant built from older sources may lack them)
    for name, at in (("pf_debug_jres_fault", [vp, ip]), ("pf_debug_smooth_fault", [vp, ip]),
                     ("pf_fuse_partial_rows", [vp, vp, vp, ip, ip, ip, ip, fp, fp, ip, ip, ip,
                                               vp, vp]),
                     ("pf_fuse_coverage_rows", [vp, ip, ip, fp, fp, ip, ip, ip, vp]),
                     ("pf_fuse_normalize_rows", [vp, vp, vp, ip, ip, fp, fp, ip, ip, ip, vp]),
                     ("pf_fuse_tile_rows", [vp, ip, ip, fp, fp, ip, ip, ip,
                                            C.POINTER(C.c_int), C.POINTER(C.c_int)]),
                     ("pf_rows_add", [vp, vp, vp, C.c_longlong]),
                     ("pf_rows_add_batch", [vp, vp, vp, vp, ip]),
                     ("pf_fuse_level", [vp, vp, ip, ip, ip, vp, vp, vp, ip, ip, fp, fp, ip, vp,
                                        vp]),
                     ("pf_fuse_targets", [vp, vp, vp, ip, ip, fp, fp, ip, vp]),
                     ("pf_probe_warp_coords", [C.POINTER(Window), ip, ip, ip, ip, vp, vp]),
                     ("pf_probe_rgb_taps", [C.POINTER(Window), ip, ip, ip, ip, vp])):
        if hasattr(L, name):
            getattr(L, name).argtypes = at
    L.pf_set_jacobi_engine.argtypes = [vp, ip, ip]
    L.pf_set_jacobi_share.argtypes = [vp, C.c_double]
    L.pf_stream_wait_level.argtypes = [vp, ip, vp]
    L.pf_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_longlong)]
    variant = os.environ.get("PANOFUSE_LIB") is not None
    for name in EXPORTS:
        if not hasattr(L, name) and not (variant and name in NEW_R4):
            raise RuntimeError(f"libpanofuse.so lacks {name}")
    _lib = L
    return L


def level_info(out_w, out_h, zr, level):
    """(w, h, h0, h1, iters, nlevels) of a fusion level (Depth.cpp:1420-1437, 1650-1675)."""
    vals = [C.c_int(0) for _ in range(6)]
    rc = load().pf_level_info(out_w, out_h, float(zr[0]), float(zr[1]), level,
                              *[C.byref(v) for v in vals])
    if rc != PF_OK:
        raise PanofuseError(rc, "pf_level_info")
    return tuple(v.value for v in vals)


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("panofuse takes device tensors only")
    if not t.is_contiguous():
        raise ValueError("panofuse takes contiguous tensors")
    return C.c_void_p(t.data_ptr())


def _out_h(out_w, out_h):
    # the level entry points' output height: MergeDepthMaps' out_w / 2 unless the caller gives one
    return out_w // 2 if out_h is None else int(out_h)


def _emap_dims(emap):
    # emap: [B, eh, ew] or [B, eh, ew, ec]
    if emap.dim() == 3:
        return emap.shape[2], emap.shape[1], 1
    return emap.shape[2], emap.shape[1], emap.shape[3]


# pf_metrics field order (include/panofuse.h)
METRIC_KEYS = ("mse", "mae", "mre", "mselog", "delta1", "delta2", "delta3", "median_shift",
               "ls_s", "ls_o", "gt_median", "given_median")
# pf_edge_metrics field order (include/panofuse.h): five doubles, three int64 counts
EDGE_KEYS = ("lap_mse", "lap_mae", "sobelx_mae", "sobely_mae", "lap5_mae")
EDGE_COUNTS = ("n_lap", "n_sobel", "n_lap5")
# pf_compare (include/panofuse.h): a pf_metrics (16 words), four floats, n_nonblack, 3 reserved
COMPARE_WORDS = 24
COMPARE_FLOATS = ("fit_s", "fit_o", "vmin", "vmax")


class Fuser:
    """One context = one device + one stream (pf_ctx)."""

    def __init__(self, device=0, stream=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("panofuse needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.L = load()
        self.device = device
        h = C.c_void_p()
        rc = self.L.pf_create(device, C.byref(h))
        if rc != PF_OK:
            raise PanofuseError(rc, "pf_create failed")
        self.h = h
        self.layout = None
        self.set_stream(stream)

    def set_stream(self, stream=None):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self.stream = stream
        self._check(self.L.pf_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def close(self):
        if getattr(self, "h", None):
            self.L.pf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != PF_OK:
            raise PanofuseError(rc, self.L.pf_last_error(self.h).decode())

    def set_tiles(self, layout, channels=1, cap_ranges=True):
        n = layout.ntiles
        fov = (Window * n)(*[Window(*map(float, layout.fovs[i])) for i in range(n)])
        rng = (Window * n)(*[Window(*map(float, layout.ranges[i])) for i in range(n)])
        tw = (C.c_int * n)(*[int(v) for v in layout.tile_w])
        th = (C.c_int * n)(*[int(v) for v in layout.tile_h])
        self._check(self.L.pf_set_tiles(self.h, fov, rng, n, tw, th, channels,
                                        1 if cap_ranges else 0))
        self.layout = layout
        self.channels = channels
        self.tile_elems = int(sum(int(layout.tile_w[i]) * int(layout.tile_h[i])
                                  for i in range(n))) * channels

    def set_solver(self, solver):
        """Degree-3 registration solver: "lm" (the reference's Ceres LM, default) or "normal"."""
        self._check(self.L.pf_set_solver(self.h, SOLVERS[solver]))

    def set_tile_validity(self, lo=None, hi=None):
        """The tile-pixel validity rule (pf_set_tile_validity).  None, None: every pixel is read,
        as the reference does (the default).  Otherwise a raw tile value v is valid iff
        lo < v < hi in fp32 (NaN never is); a bound left None is infinite, so
        set_tile_validity(float("-inf"), float("inf")) rejects exactly NaN and +-Inf and
        set_tile_validity(lo=0.0) also rejects holes written as 0.  Registration, fusion and
        stitch then skip invalid pixels; the entry points that cannot raise PF_ESTATE."""
        if lo is None and hi is None:
            self._check(self.L.pf_set_tile_validity(self.h, PF_VALID_ALL, 0.0, 0.0))
            return
        lo = float("-inf") if lo is None else float(lo)
        hi = float("inf") if hi is None else float(hi)
        self._check(self.L.pf_set_tile_validity(self.h, PF_VALID_RANGE, lo, hi))

    def tile_valid_counts(self, emap, tiles, zr, counts=None):
        """pf_tile_valid_counts: int64 [B, ntiles, 2] device tensor (made when None) of {valid
        registration samples, valid pixels} per panorama and tile under the context's rule.
        No sync."""
        import torch
        ew, eh, ec = _emap_dims(emap)
        B = emap.shape[0]
        if counts is None:
            counts = torch.zeros((B, self.layout.ntiles, 2), dtype=torch.int64,
                                 device=emap.device)
        self._check(self.L.pf_tile_valid_counts(self.h, _ptr(tiles), _ptr(emap), ew, eh, ec, B,
                                                float(zr[0]), float(zr[1]), _ptr(counts)))
        return counts

    def set_register_loss(self, kind=None, a=0.0):
        """The robust loss of the tile registrations (pf_set_register_loss): None / "none" (least
        squares, the default), "huber" or "softl1" with Ceres' scale a > 0.  With a loss set,
        register / merge fit the cubic sample-wise under it (degree 3, the "lm" solver),
        register_disparity / merge_disparity their model; register_joint and register_global
        raise PF_ESTATE."""
        if kind not in LOSSES:
            raise ValueError(f"unknown loss {kind!r}: one of {sorted(k for k in LOSSES if k)}")
        self._check(self.L.pf_set_register_loss(self.h, LOSSES[kind], float(a)))
        self._loss = LOSSES[kind]

    def set_tile_depth(self, kind=None):
        """What the tiles hold (pf_set_tile_depth): None / "ray" (ray distance, as the reference
        assumes; the default) or "planar" (depth along the optical axis, what perspective depth
        networks predict).  Under "planar" register / register_disparity fit the per-tile model
        times the pixel's ray factor and apply writes clamp01(kf * T(x)); merge / merge_disparity
        apply into a private copy and fuse it; the entry points that fuse a transform into their
        gather raise PF_ESTATE when given coeffs, and register_joint always does."""
        if kind not in TILE_DEPTHS:
            raise ValueError(f"unknown tile depth {kind!r}: \"ray\" or \"planar\"")
        self._check(self.L.pf_set_tile_depth(self.h, TILE_DEPTHS[kind]))

    def tile_ray_tables(self, tile):
        """pf_tile_ray_tables: (cu float64 [tile_w], rv float64 [tile_h]) of one tile of the stored
        layout; the ray factor of pixel (i, j) is float32(sqrt(1.0 + cu[i] + rv[j]))."""
        import numpy as np
        if self.layout is None or not 0 <= tile < self.layout.ntiles:
            raise ValueError(f"tile {tile} outside the stored layout")
        cu = np.zeros(int(self.layout.tile_w[tile]), np.float64)
        rv = np.zeros(int(self.layout.tile_h[tile]), np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self.L.pf_tile_ray_tables(self.h, int(tile), cu.ctypes.data_as(dp),
                                              rv.ctypes.data_as(dp)))
        return cu, rv

    def tile_ray_factor(self, out=None):
        """pf_tile_ray_factor: the ray factor of every tile pixel, float32 [tile pixels] device
        tensor in layout order (made when None).  Works in either mode.  No sync."""
        import torch
        n = self.tile_elems // self.channels
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=f"cuda:{self.device}")
        if out.numel() != n or out.dtype != torch.float32:
            raise ValueError(f"out must hold {n} float32 values")
        self._check(self.L.pf_tile_ray_factor(self.h, _ptr(out)))
        return out

    def overlap_pairs(self, zr):
        """pf_overlap_pairs: (pairs, pair samples) of the stored layout's overlap table for this
        zenith range; builds the table on first use (synchronises then)."""
        n, m = C.c_int(0), C.c_longlong(0)
        self._check(self.L.pf_overlap_pairs(self.h, float(zr[0]), float(zr[1]), C.byref(n),
                                            C.byref(m)))
        return n.value, m.value

    def overlap_table(self, zr):
        """pf_overlap_table: (pairs int32 [npairs, 4] = {p, q, first, count} in ascending (p, q),
        index int32 [nsamples, 2] = {element in tile p, element in tile q}) device tensors."""
        import torch
        n, m = self.overlap_pairs(zr)
        dev = f"cuda:{self.device}"
        pairs = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
        index = torch.zeros((max(m, 1), 2), dtype=torch.int32, device=dev)
        self._check(self.L.pf_overlap_table(self.h, float(zr[0]), float(zr[1]), _ptr(pairs),
                                            _ptr(index)))
        return pairs[:n], index[:m]

    def overlap_stats(self, tiles, zr, coeffs=None, stats=None):
        """pf_overlap_stats: float64 [B, npairs, 5] device tensor (made when None) of {count,
        sum d, sum d^2, max |d|, NaN samples} per panorama and pair, d the difference of the two
        tiles' values at a pair sample under coeffs (float32 [B, ntiles, 4]; None: the raw
        values).  tiles: [B, tile_elems].  No sync once the table exists."""
        import torch
        B = tiles.shape[0]
        n, _ = self.overlap_pairs(zr)
        if stats is None:
            stats = torch.zeros((B, n, 5), dtype=torch.float64, device=tiles.device)
        if stats.numel() != B * n * 5 or stats.dtype != torch.float64:
            raise ValueError(f"stats must hold [B, {n}, 5] float64 values")
        self._check(self.L.pf_overlap_stats(self.h, _ptr(tiles), _ptr(coeffs), B, float(zr[0]),
                                            float(zr[1]), _ptr(stats)))
        return stats

    def register_consistent(self, emap, tiles, zr, lam=1.0, apply=True, coeffs=None,
                            coeffs64=None, summary=None):
        """pf_register_consistent: every tile's cubic fitted to the baseline and to its
        neighbours in the overlaps, one linear least-squares problem per panorama with weight lam
        on the overlap term.  coeffs: float32, coeffs64: float64 [B, ntiles, 4]; summary: float64
        [B, 4] = {data cost, pair cost, pair samples, status (1: singular, NaN coefficients)}
        device tensors.  No sync once the table exists."""
        ew, eh, ec = _emap_dims(emap)
        B = emap.shape[0]
        if summary is not None and summary.numel() != B * 4:
            raise ValueError(f"summary holds {summary.numel()} values, not [B, 4]")
        self._check(self.L.pf_register_consistent(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), B,
                                                  float(zr[0]), float(zr[1]), float(lam),
                                                  1 if apply else 0, _ptr(coeffs),
                                                  _ptr(coeffs64), _ptr(summary)))

    def _summary_ptr(self, summary, B, width):
        if summary is not None and summary.numel() != B * self.layout.ntiles * width:
            raise ValueError(f"summary holds {summary.numel()} values, not [B, ntiles, {width}]")
        return _ptr(summary)

    def register(self, emap, tiles, zr, degree=3, apply=True, coeffs=None, coeffs64=None,
                 summary=None):
        """pf_register; summary (pf_register_ex, only while a loss is set): float64
        [B, ntiles, 6] device tensor of {initial cost, final cost, iterations, termination code,
        samples used, inliers}.  No sync."""
        ew, eh, ec = _emap_dims(emap)
        B = emap.shape[0]
        if summary is not None:
            self._check(self.L.pf_register_ex(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), B,
                                              float(zr[0]), float(zr[1]), degree,
                                              1 if apply else 0, _ptr(coeffs), _ptr(coeffs64),
                                              self._summary_ptr(summary, B, 6)))
            return
        self._check(self.L.pf_register(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), B,
                                       float(zr[0]), float(zr[1]), degree, 1 if apply else 0,
                                       _ptr(coeffs), _ptr(coeffs64)))

    def fuse(self, emap, tiles, out, zr, coeffs=None):
        ew, eh, ec = _emap_dims(emap)
        B, oh, ow = out.shape
        self._check(self.L.pf_fuse(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), _ptr(coeffs),
                                   B, ow, oh, float(zr[0]), float(zr[1]), _ptr(out)))

    def merge(self, emap, tiles, out, zr, coeffs=None):
        ew, eh, ec = _emap_dims(emap)
        B, oh, ow = out.shape
        if oh != ow // 2:
            raise ValueError("MergeDepthMaps output height is out_w/2")
        self._check(self.L.pf_merge(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), B, ow,
                                    float(zr[0]), float(zr[1]), _ptr(coeffs), _ptr(out)))

    # ---- per-pixel tile weights (pf_*_weighted) ----
    def tent_weights(self, out=None):
        """pf_tile_tent_weights: one weight set, float32 [tile_elems] device tensor in the tiles'
        element layout (made when None): the blending tent min(t, m) / m of every tile, 0 in the
        non-zero channels.  No sync."""
        import torch
        if out is None:
            out = torch.empty(self.tile_elems, dtype=torch.float32,
                              device=f"cuda:{self.device}")
        if out.numel() != self.tile_elems or out.dtype != torch.float32:
            raise ValueError(f"out must hold {self.tile_elems} float32 values")
        self._check(self.L.pf_tile_tent_weights(self.h, _ptr(out)))
        return out

    def _wbatch(self, weights, B):
        # weights: None (the library refuses it), [tile_elems] or [wbatch, tile_elems]
        if weights is None:
            return 1
        if weights.numel() % self.tile_elems or weights.shape[-1] != self.tile_elems:
            raise ValueError(f"weights must be [tile_elems] or [B, tile_elems] with tile_elems = "
                             f"{self.tile_elems}")
        return weights.numel() // self.tile_elems

    def register_weighted(self, emap, tiles, weights, zr, apply=True, coeffs=None, coeffs64=None,
                          summary=None):
        """pf_register_weighted: register's degree-3 LM fit as weighted least squares.  weights:
        float32 [tile_elems] (one set for the batch) or [B, tile_elems] in the tiles' element
        layout, channel 0 read; a weight that is not in (0, +inf) switches its pixel off, and
        weights in {0, 1} are the validity rule.  summary: float64 [B, ntiles, 2] device tensor of
        {used samples, sum of w}.  No sync."""
        ew, eh, ec = _emap_dims(emap)
        B = emap.shape[0]
        self._check(self.L.pf_register_weighted(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles),
                                                _ptr(weights), self._wbatch(weights, B), B,
                                                float(zr[0]), float(zr[1]), 1 if apply else 0,
                                                _ptr(coeffs), _ptr(coeffs64),
                                                self._summary_ptr(summary, B, 2)))

    def fuse_weighted(self, emap, tiles, weights, out, zr, coeffs=None):
        """pf_fuse_weighted: fuse with every tile's Laplacian weighted by the smallest weight of
        its five taps; weights as register_weighted's."""
        ew, eh, ec = _emap_dims(emap)
        B, oh, ow = out.shape
        self._check(self.L.pf_fuse_weighted(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles),
                                            _ptr(weights), self._wbatch(weights, B),
                                            _ptr(coeffs), B, ow, oh, float(zr[0]), float(zr[1]),
                                            _ptr(out)))

    def merge_weighted(self, emap, tiles, weights, out, zr, coeffs=None):
        """pf_merge_weighted: register_weighted (tiles untouched) + fuse_weighted."""
        ew, eh, ec = _emap_dims(emap)
        B, oh, ow = out.shape
        if oh != ow // 2:
            raise ValueError("MergeDepthMaps output height is out_w/2")
        self._check(self.L.pf_merge_weighted(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles),
                                             _ptr(weights), self._wbatch(weights, B), B, ow,
                                             float(zr[0]), float(zr[1]), _ptr(coeffs),
                                             _ptr(out)))

    # ---- per-pixel weights for disparity tiles ----
    def range_weights(self, tiles, lo, hi, out=None):
        """pf_tile_range_weights: the validity rule lo < v < hi as one weight set per panorama,
        float32 [B, tile_elems] (made when None): 1.0 at channel 0 of a passing pixel, 0.0
        everywhere else.  tiles: [B, tile_elems].  No sync."""
        import torch
        B = tiles.numel() // self.tile_elems
        if B < 1 or tiles.numel() != B * self.tile_elems or tiles.dtype != torch.float32:
            raise ValueError(f"tiles must hold [B, {self.tile_elems}] float32 values")
        if out is None:
            out = torch.empty((B, self.tile_elems), dtype=torch.float32, device=tiles.device)
        if out.numel() != tiles.numel() or out.dtype != torch.float32:
            raise ValueError(f"out must hold [{B}, {self.tile_elems}] float32 values")
        self._check(self.L.pf_tile_range_weights(self.h, _ptr(tiles), B, float(lo), float(hi),
                                                 _ptr(out)))
        return out

    def register_disparity_weighted(self, emap, tiles, weights, zr, apply=True, coeffs=None,
                                    coeffs64=None, summary=None):
        """pf_register_disparity_weighted: register_disparity's fit as weighted least squares;
        weights as register_weighted's.  summary: float64 [B, ntiles, 6] device tensor of {initial
        cost, final cost, iterations, termination code, used samples, sum of w}.  A tile with
        fewer than 3 used samples gets NaN coefficients and termination 5.  Honours planar-depth
        tiles (set_tile_depth).  No sync."""
        ew, eh, ec = _emap_dims(emap)
        B = emap.shape[0]
        self._check(self.L.pf_register_disparity_weighted(
            self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), _ptr(weights), self._wbatch(weights, B),
            B, float(zr[0]), float(zr[1]), 1 if apply else 0, _ptr(coeffs), _ptr(coeffs64),
            self._summary_ptr(summary, B, 6)))

    def merge_disparity_weighted(self, emap, tiles, weights, out, zr, coeffs=None):
        """pf_merge_disparity_weighted: register_disparity_weighted with apply on a copy of the
        tiles (the caller's stay untouched), then fuse_weighted on the copy with the same
        weights."""
        ew, eh, ec = _emap_dims(emap)
        B, oh, ow = out.shape
        if oh != ow // 2:
            raise ValueError("MergeDepthMaps output height is out_w/2")
        self._check(self.L.pf_merge_disparity_weighted(
            self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), _ptr(weights), self._wbatch(weights, B),
            B, ow, float(zr[0]), float(zr[1]), _ptr(coeffs), _ptr(out)))

    def register_disparity(self, emap, tiles, zr, apply=True, coeffs=None, coeffs64=None,
                           summary=None):
        """The disparity-tile registration (pf_register_disparity): y = 1/(a x + b) + d fitted per
        tile by the reference's LM, abcd = (a, b, 1, d).  coeffs: float32 [B, ntiles, 4], coeffs64 /
        summary: float64 [B, ntiles, 4] device tensors (summary = initial cost, final cost,
        iterations, termination code); apply runs D2DTransform on the tiles.  While a loss is set
        (set_register_loss) the fit runs under it and summary is [B, ntiles, 6], as register's.
        No sync."""
        ew, eh, ec = _emap_dims(emap)
        B = emap.shape[0]
        width = 6 if getattr(self, "_loss", 0) else 4
        self._check(self.L.pf_register_disparity(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), B,
                                                 float(zr[0]), float(zr[1]), 1 if apply else 0,
                                                 _ptr(coeffs), _ptr(coeffs64),
                                                 self._summary_ptr(summary, B, width)))

    def disparity_transform(self, t, abcd, channels=1):
        """D2DTransform (Depth.cpp:214-243) in place on a float32 device tensor: channel 0 of its
        pixels, `channels` interleaved values each, becomes clamp01(c / (a X + b) + d).  No sync."""
        k = (C.c_float * 4)(*[float(v) for v in abcd])
        self._check(self.L.pf_disparity_transform(self.h, _ptr(t), t.numel() // channels,
                                                  int(channels), k))

    def merge_disparity(self, emap, tiles, out, zr, coeffs=None):
        """MergeDepthMaps' core for disparity tiles (pf_merge_disparity); tiles stay untouched."""
        ew, eh, ec = _emap_dims(emap)
        B, oh, ow = out.shape
        if oh != ow // 2:
            raise ValueError("MergeDepthMaps output height is out_w/2")
        self._check(self.L.pf_merge_disparity(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), B, ow,
                                              float(zr[0]), float(zr[1]), _ptr(coeffs),
                                              _ptr(out)))

    def register_global(self, emap, data, zr, apply=False, coeffs=None, coeffs64=None,
                        summary=None):
        """SolveDepthToDepth2 (pf_register_global): one cubic per panorama from the fused result
        data (int16 / uint16 [B, H, W], read as u16) to the baseline emap, by the reference's LM
        from (0, 0, 1, 0).  coeffs: float32 [B, 4], coeffs64 / summary: float64 [B, 4] device
        tensors (summary = initial cost, final cost, iterations, termination code); apply runs
        result_transform with the fitted coefficients.  Needs no tile layout.  No sync."""
        ew, eh, ec = _emap_dims(emap)
        B, oh, ow = data.shape
        self._check(self.L.pf_register_global(self.h, _ptr(emap), ew, eh, ec, _ptr(data), B, ow,
                                              oh, float(zr[0]), float(zr[1]), 1 if apply else 0,
                                              _ptr(coeffs), _ptr(coeffs64), _ptr(summary)))

    def result_transform(self, data, zr, coeffs):
        """The cubic of coeffs (float32 [B, 4] device tensor) on rows h0..h1 of the u16 result
        data [B, H, W], in place (pf_result_transform).  No sync."""
        B, oh, ow = data.shape
        self._check(self.L.pf_result_transform(self.h, _ptr(data), B, ow, oh, float(zr[0]),
                                               float(zr[1]), _ptr(coeffs)))

    def median_scale(self, map0, map1, medians=None, status=None):
        """MedianScaling (pf_median_scale): channel 0 of map0 (float32 [B, h, w] or [B, h, w, c])
        is scaled in place toward map1's median.  medians: float32 [B, 2], status: int32 [B]
        device tensors (1: a map without any valid pixel, nothing written).  No sync."""
        w0, h0, c0 = _emap_dims(map0)
        w1, h1, c1 = _emap_dims(map1)
        self._check(self.L.pf_median_scale(self.h, _ptr(map0), w0, h0, c0, _ptr(map1), w1, h1, c1,
                                           map0.shape[0], _ptr(medians), _ptr(status)))

    def copy_invalid(self, dst, ref):
        """EquirectangularMap::CopyInvalidPixels (pf_copy_invalid): ref's invalid pixels
        (channel 0 < 1e-4 or >= 1 - 1e-4) are copied into channel 0 of dst, in place.  No sync."""
        w, h, c = _emap_dims(dst)
        rw, rh, rc = _emap_dims(ref)
        self._check(self.L.pf_copy_invalid(self.h, _ptr(dst), w, h, c, _ptr(ref), rw, rh, rc,
                                           dst.shape[0]))

    def set_metrics_order(self, order):
        """"tree" (the context's default): fp64 partial sums (fast, means within 1e-5 of exact
        sums); "sequential": the reference's float summation order, bit-exact means (~7.4 ms per
        64-panorama call at C3; the facade and panofuse_main default to it)."""
        self._check(self.L.pf_set_metrics_order(self.h, METRICS_ORDERS[order]))

    def solve_smoothing(self, tiles, out, zr, coeffs=None):
        """SolveDepthBySmoothing (Depth.cpp:1773-1878) into out [B, out_h, out_w] (int16 view
        of u16); coeffs: None or [B, ntiles, 4], applied as Depth2DepthTransform on the fly."""
        B, oh, ow = out.shape
        self._check(self.L.pf_solve_smoothing(self.h, _ptr(tiles), _ptr(coeffs), B, ow, oh,
                                              float(zr[0]), float(zr[1]), _ptr(out)))

    def stitch(self, tiles, out, coeffs=None):
        """The direct tile stitch (pf_stitch, Depth.cpp:817-865) into out [B, out_h, out_w]
        (int16 view of u16): every pixel takes the first tile whose range box contains it, no
        fusion; coeffs: None or [B, ntiles, 4], applied as Depth2DepthTransform on the fly."""
        B, oh, ow = out.shape
        self._check(self.L.pf_stitch(self.h, _ptr(tiles), _ptr(coeffs), B, ow, oh, _ptr(out)))

    def laplacian_residual(self, buf, lnorm, h0, h1, err=None):
        """SolveDepthAll's Laplacian self-check (pf_laplacian_residual, Depth.cpp:1738-1758) of
        the level planes buf against their targets lnorm (float32 [B, h, w] device tensors) over
        rows h0+1 .. h1-1: the reference-order float chain per plane into err (float32 [B]
        device tensor, made when None) -- returned.  Needs no tile layout.  No sync."""
        import torch
        B, h, w = buf.shape
        if tuple(lnorm.shape) != (B, h, w):
            raise ValueError("buf and lnorm differ in shape")
        if err is None:
            err = torch.zeros(B, dtype=torch.float32, device=buf.device)
        self._check(self.L.pf_laplacian_residual(self.h, _ptr(buf), _ptr(lnorm), w, h, int(h0),
                                                 int(h1), B, _ptr(err)))
        return err

    def fuse_check(self, emap, tiles, zr, out_w, out_h=None, coeffs=None, out=None, err=None):
        """pf_fuse_check: the fusion of ONE panorama (emap [1, eh, ew(, ec)], tiles [1, tile_elems],
        coeffs None or [1, ntiles, 4]) with the Laplacian self-check after every level.  Returns
        err, a float32 [nlevels] device tensor (made when None); its last entry is the number the
        reference prints as "check Laplacian err".  out: optional [1, out_h, out_w] or
        [out_h, out_w] (int16 view of u16), equal to fuse()'s.  No sync."""
        import torch
        ew, eh, ec = _emap_dims(emap)
        out_h = _out_h(out_w, out_h)
        if emap.shape[0] != 1:
            raise ValueError("fuse_check takes one panorama")
        if err is None:
            n = level_info(out_w, out_h, zr, 0)[5]
            err = torch.zeros(n, dtype=torch.float32, device=emap.device)
        if out is not None and out.numel() != out_w * out_h:
            raise ValueError("out is not out_h x out_w")
        self._check(self.L.pf_fuse_check(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles),
                                         _ptr(coeffs), out_w, out_h, float(zr[0]), float(zr[1]),
                                         _ptr(err), _ptr(out)))
        return err

    def warp_depth(self, pano, tiles, resp=None):
        B, ph, pw = pano.shape
        self._check(self.L.pf_warp_depth(self.h, _ptr(pano), pw, ph, B, _ptr(resp),
                                         _ptr(tiles)))

    def warp_rgb(self, pano, tiles):
        B, ph, pw, _ = pano.shape
        self._check(self.L.pf_warp_rgb(self.h, _ptr(pano), pw, ph, B, _ptr(tiles)))

    def register_joint(self, emap, tiles, zr, active, degree=3, coeffs=None, coeffs64=None):
        """SolveDepthToDepth with the tiles of `active` (list of tile indices) in one problem;
        coeffs / coeffs64: [B, 4] device tensors."""
        ew, eh, ec = _emap_dims(emap)
        B = emap.shape[0]
        mask = (C.c_int * self.layout.ntiles)(*[1 if i in set(active) else 0
                                                 for i in range(self.layout.ntiles)])
        self._check(self.L.pf_register_joint(self.h, _ptr(emap), ew, eh, ec, _ptr(tiles), B,
                                             float(zr[0]), float(zr[1]), int(degree), mask,
                                             _ptr(coeffs), _ptr(coeffs64)))

    def error_metrics_async(self, gt, given, zr, out, align_way=1, cap_depth=True):
        """pf_error_metrics into out (int32 [B,16] device tensor = B pf_metrics), no sync."""
        import torch
        gw, gh, gc = _emap_dims(gt)
        B, h, w = given.shape[:3]
        if given.dtype in (torch.int16, torch.uint16):
            self._check(self.L.pf_error_metrics(self.h, _ptr(gt), gw, gh, gc, None, _ptr(given),
                                                w, h, 1, B, float(zr[0]), float(zr[1]),
                                                int(align_way), int(cap_depth), _ptr(out)))
        else:
            gvc = given.shape[3] if given.dim() == 4 else 1
            self._check(self.L.pf_error_metrics(self.h, _ptr(gt), gw, gh, gc, _ptr(given), None,
                                                w, h, gvc, B, float(zr[0]), float(zr[1]),
                                                int(align_way), int(cap_depth), _ptr(out)))

    def error_metrics(self, gt, given, zr, align_way=1, cap_depth=True):
        """ErrorData (given: int16/uint16 [B,h,w] result bits) or ErrorEmap (given: float32
        [B,h,w] or [B,h,w,c]) against gt float32 [B,gh,gw] or [B,gh,gw,gc]
        (Depth.cpp:1980-2458).  Returns a list (one per panorama) of dicts of METRIC_KEYS +
        n, nlog."""
        import torch
        B = given.shape[0]
        out = torch.zeros((B, 16), dtype=torch.int32, device=gt.device)
        self.error_metrics_async(gt, given, zr, out, align_way, cap_depth)
        self.synchronize()
        o = out.cpu()
        f = o[:, :12].view(torch.float32)
        res = []
        for b in range(B):
            d = {k: float(f[b, i]) for i, k in enumerate(METRIC_KEYS)}
            d["n"], d["nlog"] = int(o[b, 12]), int(o[b, 13])
            res.append(d)
        return res

    def edge_metrics_async(self, gt, given, out, gt_lap=None, given_lap=None, lap_ae=None):
        """pf_error_laplacian into out (int64 [B,8] device tensor = B pf_edge_metrics), no sync.
        gt_lap / given_lap / lap_ae: optional float64 [B,h,w] device tensors for the maps."""
        import torch
        gw, gh, gc = _emap_dims(gt)
        B, h, w = given.shape[:3]
        if given.dtype in (torch.int16, torch.uint16):
            gf, g16, gvc = None, _ptr(given), 1
        else:
            gf, g16, gvc = _ptr(given), None, (given.shape[3] if given.dim() == 4 else 1)
        self._check(self.L.pf_error_laplacian(self.h, _ptr(gt), gw, gh, gc, gf, g16, w, h, gvc,
                                              B, _ptr(out), _ptr(gt_lap), _ptr(given_lap),
                                              _ptr(lap_ae)))

    def edge_metrics(self, gt, given, maps=False):
        """ErrorLaplacian (Depth.cpp:2636-2953) of given (int16/uint16 [B,h,w] result bits, or
        float32 [B,h,w] / [B,h,w,c]) against gt float32 [B,gh,gw] or [B,gh,gw,gc].  Returns a
        list (one per panorama) of dicts of EDGE_KEYS + EDGE_COUNTS; with maps=True also the
        three float64 [B,h,w] device tensors (gt Laplacian, given Laplacian, absolute error)."""
        import torch
        B, h, w = given.shape[:3]
        out = torch.zeros((B, 8), dtype=torch.int64, device=gt.device)
        planes = [torch.empty((B, h, w), dtype=torch.float64, device=gt.device)
                  for _ in range(3)] if maps else [None, None, None]
        self.edge_metrics_async(gt, given, out, *planes)
        self.synchronize()
        o = out.cpu()
        f = o[:, :5].contiguous().view(torch.float64)
        res = []
        for b in range(B):
            d = {k: float(f[b, i]) for i, k in enumerate(EDGE_KEYS)}
            for i, k in enumerate(EDGE_COUNTS):
                d[k] = int(o[b, 5 + i])
            res.append(d)
        return (res, *planes) if maps else res

    def compare_async(self, gt, given, zr, out, disp_depth, align_way=1, cap_depth=True,
                      depth=None, shifted=None):
        """pf_error_compare into out (int32 [B,24] device tensor = B pf_compare), no sync.
        depth: optional float32 [B,h,w], shifted: optional uint8 [B,h,w] device tensors."""
        gw, gh, gc = _emap_dims(gt)
        B, h, w = given.shape[:3]
        gvc = given.shape[3] if given.dim() == 4 else 1
        self._check(self.L.pf_error_compare(self.h, _ptr(gt), gw, gh, gc, _ptr(given), w, h, gvc,
                                            B, float(zr[0]), float(zr[1]), int(bool(disp_depth)),
                                            int(align_way), int(cap_depth), _ptr(out),
                                            _ptr(depth), _ptr(shifted)))

    def compare(self, gt, given, zr, disp_depth, align_way=1, cap_depth=True, planes=False):
        """ErrorCompare (Depth.cpp:2460-2634) of given (float32 [B,h,w] or [B,h,w,c]: a depth
        map, or with disp_depth a disparity map) against gt float32 [B,gh,gw] or [B,gh,gw,gc].
        Returns a list (one per panorama) of dicts of METRIC_KEYS + n, nlog, fit_s, fit_o, vmin,
        vmax, n_nonblack; with planes=True also the float32 depth plane and the uint8 shifted
        plane, both [B,h,w] device tensors."""
        import torch
        B, h, w = given.shape[:3]
        out = torch.zeros((B, COMPARE_WORDS), dtype=torch.int32, device=gt.device)
        depth = torch.empty((B, h, w), dtype=torch.float32, device=gt.device) if planes else None
        shifted = torch.empty((B, h, w), dtype=torch.uint8, device=gt.device) if planes else None
        self.compare_async(gt, given, zr, out, disp_depth, align_way, cap_depth, depth, shifted)
        self.synchronize()
        o = out.cpu()
        f = o.view(torch.float32)
        res = []
        for b in range(B):
            d = {k: float(f[b, i]) for i, k in enumerate(METRIC_KEYS)}
            d["n"], d["nlog"] = int(o[b, 12]), int(o[b, 13])
            for i, k in enumerate(COMPARE_FLOATS):
                d[k] = float(f[b, 16 + i])
            d["n_nonblack"] = int(o[b, 20])
            res.append(d)
        return (res, depth, shifted) if planes else res

    def disp_depth_convert(self, t, channels=1):
        """DispDepthConversion (Depth.cpp:587-610) in place on a float32 device tensor: channel 0
        of its pixels, `channels` interleaved values each (the last dimension when > 1), is
        inverted `channels` times where (double)|v| >= 1e-5.  No sync."""
        self._check(self.L.pf_disp_depth_convert(self.h, _ptr(t), t.numel() // channels,
                                                 int(channels)))

    def probe_taps(self, out_w, zr, level, out_h=None):
        import torch
        out_h = _out_h(out_w, out_h)
        w, h = level_info(out_w, out_h, zr, level)[:2]
        out = torch.empty((h, w, 5), dtype=torch.int32, device=f"cuda:{self.device}")
        self._check(self.L.pf_probe_taps(self.h, out_w, out_h, float(zr[0]), float(zr[1]),
                                         level, _ptr(out)))
        return out

    def layout_audit(self, out_w, zr, level, out_h=None):
        """pf_layout_audit: what the tiles set by set_tiles do at one level of an out_w x out_h
        fusion, as a dict of pf_level_audit's fields (w, h, h0, h1, taps_outside, taps_clamped,
        covered, uncovered_interior, max_cover, seam).  Counted on the GPU with the fusion's own
        tables; synchronizes the context's stream."""
        a = LevelAudit()
        self._check(self.L.pf_layout_audit(self.h, out_w, _out_h(out_w, out_h), float(zr[0]),
                                           float(zr[1]), level, C.byref(a)))
        return {name: int(getattr(a, name)) for name, _ in LevelAudit._fields_}

    def fuse_partial(self, tiles, coeffs, t0, t1, out_w, zr, level, lsum, cnt, out_h=None):
        self._check(self.L.pf_fuse_partial(self.h, _ptr(tiles), _ptr(coeffs), t0, t1, out_w,
                                           _out_h(out_w, out_h), float(zr[0]), float(zr[1]),
                                           level, _ptr(lsum), _ptr(cnt)))

    def fuse_partial_rows(self, tiles, coeffs, t0, t1, out_w, zr, level, row0, row1, lsum, cnt,
                          out_h=None):
        """pf_fuse_partial on rows [row0, row1) only (zeros on their rows outside the band, nothing
        written elsewhere)."""
        self._check(self.L.pf_fuse_partial_rows(self.h, _ptr(tiles), _ptr(coeffs), t0, t1, out_w,
                                                _out_h(out_w, out_h), float(zr[0]), float(zr[1]),
                                                level, int(row0), int(row1), _ptr(lsum),
                                                _ptr(cnt)))

    def fuse_coverage_rows(self, out_w, zr, level, row0, row1, cnt, out_h=None):
        """Coverage count of every tile on rows [row0, row1) (layout-only)."""
        self._check(self.L.pf_fuse_coverage_rows(self.h, out_w, _out_h(out_w, out_h),
                                                 float(zr[0]), float(zr[1]), level, int(row0),
                                                 int(row1), _ptr(cnt)))

    def fuse_normalize_rows(self, lsum, cnt, out_w, zr, level, row0, row1, lnorm, out_h=None):
        self._check(self.L.pf_fuse_normalize_rows(self.h, _ptr(lsum), _ptr(cnt), out_w,
                                                  _out_h(out_w, out_h), float(zr[0]),
                                                  float(zr[1]), level, int(row0), int(row1),
                                                  _ptr(lnorm)))

    def fuse_tile_rows(self, out_w, zr, level, t0, t1, out_h=None):
        """(ymin, ymax): rows where tiles [t0, t1) have non-zero partial sums (ymin > ymax: none)."""
        lo, hi = C.c_int(), C.c_int()
        self._check(self.L.pf_fuse_tile_rows(self.h, out_w, _out_h(out_w, out_h), float(zr[0]),
                                             float(zr[1]), level, int(t0), int(t1), C.byref(lo),
                                             C.byref(hi)))
        return lo.value, hi.value

    def rows_add(self, dst, src):
        """dst += src (same-size fp32 device tensors), on the context's stream."""
        assert dst.numel() == src.numel()
        self._check(self.L.pf_rows_add(self.h, _ptr(dst), _ptr(src), dst.numel()))

    def rows_add_batch(self, pairs):
        """dst += src for every (dst, src) pair of same-size fp32 device tensors, one launch
        (pf_rows_add_batch); the destinations must not overlap."""
        k = len(pairs)
        if not k:
            return
        dst = (C.c_void_p * k)(*[_ptr(d).value for d, _ in pairs])
        src = (C.c_void_p * k)(*[_ptr(s).value for _, s in pairs])
        n = (C.c_longlong * k)()
        for i, (d, s) in enumerate(pairs):
            assert d.numel() == s.numel()
            n[i] = d.numel()
        self._check(self.L.pf_rows_add_batch(self.h, dst, src, n, k))

    def fuse_seed(self, emap, prev, out_w, zr, level, buf, out_h=None):
        ew, eh, ec = _emap_dims(emap) if emap is not None else (0, 0, 0)
        self._check(self.L.pf_fuse_seed(self.h, _ptr(emap), ew, eh, ec, _ptr(prev), out_w,
                                        _out_h(out_w, out_h), float(zr[0]), float(zr[1]), level,
                                        _ptr(buf)))

    def fuse_finish_level(self, lsum, cnt, out_w, zr, level, buf, out=None, out_h=None):
        self._check(self.L.pf_fuse_finish_level(self.h, _ptr(lsum), _ptr(cnt), out_w,
                                                _out_h(out_w, out_h), float(zr[0]), float(zr[1]),
                                                level, _ptr(buf), _ptr(out)))

    def fuse_level(self, emap, prev, lsum, cnt, out_w, zr, level, buf, out=None, out_h=None):
        """pf_fuse_level: fuse_seed + fuse_finish_level with the seed inside the first pass."""
        ew, eh, ec = _emap_dims(emap) if emap is not None else (0, 0, 0)
        self._check(self.L.pf_fuse_level(self.h, _ptr(emap), ew, eh, ec, _ptr(prev), _ptr(lsum),
                                         _ptr(cnt), out_w, _out_h(out_w, out_h), float(zr[0]),
                                         float(zr[1]), level, _ptr(buf), _ptr(out)))

    def fuse_targets(self, tiles, coeffs, out_w, zr, level, lnorm, out_h=None):
        """pf_fuse_targets: one level's normalised targets of one panorama from every tile."""
        self._check(self.L.pf_fuse_targets(self.h, _ptr(tiles), _ptr(coeffs), out_w,
                                           _out_h(out_w, out_h), float(zr[0]), float(zr[1]),
                                           level, _ptr(lnorm)))

    def multicover_count(self, out_w, zr, level, out_h=None):
        n = C.c_int(0)
        self._check(self.L.pf_fuse_multicover(self.h, None, None, 0, 0, out_w,
                                              _out_h(out_w, out_h), float(zr[0]), float(zr[1]),
                                              level, None, C.byref(n)))
        return n.value

    def multicover(self, tiles, coeffs, t0, t1, out_w, zr, level, contrib, out_h=None):
        n = C.c_int(0)
        self._check(self.L.pf_fuse_multicover(self.h, _ptr(tiles), _ptr(coeffs), t0, t1, out_w,
                                              _out_h(out_w, out_h), float(zr[0]), float(zr[1]),
                                              level, _ptr(contrib), C.byref(n)))

    def multicover_patch(self, out_w, zr, level, contrib, lsum, out_h=None):
        self._check(self.L.pf_fuse_multicover_patch(self.h, out_w, _out_h(out_w, out_h),
                                                    float(zr[0]), float(zr[1]), level,
                                                    _ptr(contrib), _ptr(lsum)))

    # ---- row-band sharding of a level's sweeps (pf_dist.fuse_row_sharded) ----
    def fuse_normalize(self, lsum, cnt, out_w, zr, level, lnorm, out_h=None):
        self._check(self.L.pf_fuse_normalize(self.h, _ptr(lsum), _ptr(cnt), out_w,
                                             _out_h(out_w, out_h), float(zr[0]), float(zr[1]),
                                             level, _ptr(lnorm)))

    def fuse_border(self, prev, out_w, zr, level, a=None, b=None, out=None, out_h=None):
        self._check(self.L.pf_fuse_border(self.h, _ptr(prev), out_w, _out_h(out_w, out_h),
                                          float(zr[0]), float(zr[1]), level, _ptr(a), _ptr(b),
                                          _ptr(out)))

    def band_pass_count(self, out_w, zr, level, nbands=1, out_h=None):
        """How many passes fuse_band_plan gives the level; 0 where it has no band passes (a zenith
        band at rows 1 / h-2, an odd or narrow width: the per-sweep engine of fuse_level), where
        fuse_band_plan raises."""
        n = self.L.pf_fuse_band_plan(self.h, out_w, _out_h(out_w, out_h), float(zr[0]),
                                     float(zr[1]), level, nbands, None, 0)
        if n < 0:
            self._check(n)
        return n

    def fuse_band_plan(self, out_w, zr, level, nbands, out_h=None):
        """Sweep depths of the level's passes (identical on every rank for the same nbands)."""
        T = (C.c_int * 256)()
        n = self.L.pf_fuse_band_plan(self.h, out_w, _out_h(out_w, out_h), float(zr[0]),
                                     float(zr[1]), level, nbands, T, 256)
        if n < 0:
            self._check(n)
        return [T[i] for i in range(n)]

    def fuse_band_pass(self, lnorm, src_mode, out_w, zr, level, T, row0, row1, src=None,
                       dst=None, prev=None, emap=None, out=None, out_h=None):
        ew, eh, ec = _emap_dims(emap) if emap is not None else (0, 0, 0)
        self._check(self.L.pf_fuse_band_pass(self.h, _ptr(emap), ew, eh, ec, _ptr(prev),
                                             _ptr(lnorm), int(src_mode), _ptr(src), _ptr(dst),
                                             _ptr(out), out_w, _out_h(out_w, out_h),
                                             float(zr[0]), float(zr[1]), level, int(T), int(row0),
                                             int(row1)))

    def profile(self, on=True):
        """Enable/disable per-stage hipEvent timing (resets the accumulators)."""
        self._check(self.L.pf_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        """{stage: (ms, algorithmic_bytes, launches)} accumulated since the last read."""
        n = len(STAGES)
        ms, by, ln = (C.c_double * n)(), (C.c_double * n)(), (C.c_longlong * n)()
        self._check(self.L.pf_profile_read(self.h, ms, by, ln))
        return {STAGES[i]: (ms[i], by[i], ln[i]) for i in range(n)}

    def synchronize(self):
        """Wait for the context stream; raises PanofuseError(PF_ETIMEOUT) if a fusion enqueued
        since the last report had a resident-kernel wait time out (its output is invalid)."""
        self._check(self.L.pf_synchronize(self.h))

    def stream_wait_level(self, level, stream):
        """Make torch `stream` wait for level `level` of this context's last enqueued fusion."""
        self._check(self.L.pf_stream_wait_level(self.h, int(level), C.c_void_p(stream.cuda_stream)))

    def set_jacobi_engine(self, resident=True, row_blocks=0):
        """Jacobi engine of the fusion levels: the resident one-launch kernel where it applies
        (default) or the streaming passes; row_blocks forces its blocks per panorama."""
        self._check(self.L.pf_set_jacobi_engine(self.h, 1 if resident else 0, int(row_blocks)))

    def set_jacobi_share(self, share):
        """Fraction of the GPU this context's Jacobi pass plans count on (0 < share <= 1): for
        fusions that run concurrently with others on the same device (pf_set_jacobi_share)."""
        self._check(self.L.pf_set_jacobi_share(self.h, float(share)))

    def jres_errors(self):
        """Timed-out hand-off waits of the resident level kernel so far (0 = every resident
        level result is valid); synchronises."""
        n = self.L.pf_jres_errors(self.h)
        if n < 0:
            self._check(n)
        return n

    def debug_jres_fault(self, spin_log2=10):
        """Test hook: the next resident launch withholds row block 0's hand-off flag with waits
        bounded at 2^spin_log2 polls, so that fusion must report PF_ETIMEOUT."""
        self._check(self.L.pf_debug_jres_fault(self.h, int(spin_log2)))

    def debug_smooth_fault(self, spin_log2=10):
        """Test hook: in the next row-band smoothing, row block 0 never publishes its steps and
        the waits give up after 2^spin_log2 polls, so that call must report PF_ETIMEOUT."""
        self._check(self.L.pf_debug_smooth_fault(self.h, int(spin_log2)))


def warp_coords(fov, tile_w, tile_h, pw, ph):
    """The depth warp's cached map of one tile (host code, no GPU): (wxy uint32 [h*w] =
    x0 | y0 << 16, wfxy float32 [h*w, 2] = (fx, fy))."""
    n = int(tile_w) * int(tile_h)
    wxy = np.zeros(n, np.uint32)
    wf = np.zeros((n, 2), np.float32)
    rc = load().pf_probe_warp_coords(C.byref(Window(*map(float, fov))), int(tile_w), int(tile_h),
                                     int(pw), int(ph), wxy.ctypes.data, wf.ctypes.data)
    if rc != PF_OK:
        raise PanofuseError(rc, "pf_probe_warp_coords")
    return wxy, wf


def rgb_taps(fov, tile_w, tile_h, pw, ph):
    """The RGB warp's cached tap map of one tile (host code, no GPU): uint32 [h*w, 4]."""
    taps = np.zeros((int(tile_w) * int(tile_h), 4), np.uint32)
    rc = load().pf_probe_rgb_taps(C.byref(Window(*map(float, fov))), int(tile_w), int(tile_h),
                                  int(pw), int(ph), taps.ctypes.data)
    if rc != PF_OK:
        raise PanofuseError(rc, "pf_probe_rgb_taps")
    return taps


def make_responses(params, device):
    """[B, ntiles] pf_response array on the device from (alpha, kappa, beta, sigma, seed)."""
    import torch
    p = np.asarray(params, dtype=np.float64).reshape(-1, 5)
    raw = np.zeros((p.shape[0], 6), np.uint32)
    raw[:, 0:4] = p[:, 0:4].astype(np.float32).view(np.uint32)
    raw[:, 4] = p[:, 4].astype(np.uint64).astype(np.uint32)
    return torch.from_numpy(raw.view(np.int32).copy()).to(device)

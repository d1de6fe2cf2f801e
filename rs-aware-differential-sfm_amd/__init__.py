"""rsdsfm -- MI355X-native rolling-shutter differential-SfM solver (Python binding of the C ABI).

The package directory is `rs-aware-differential-sfm_amd/`; import it through the repo-root shim
`import rsdsfm`.  Everything here goes through include/rsdsfm.h (ctypes, plain pointers and sizes): the HIP
library `librsdsfm_hip.so` IS the product.  There is no CPU fallback: if the library is missing or no
gfx950 device is usable, loading / Solver() raises.

Mirrors the reference's function boundary (reference: src/minimal.h:79-161, src/nonlinearRefinement.h:37-113):
    Solver.get_alpha / get_alpha_k / calculate_velocities / ransac
    Solver.estimate_inverse_depths / non_linear_refinement
    Solver.flatten / depth_map / pose_table            (caller glue, rsframe.cc:771-800)
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

from . import dist, pipeline, synth  # noqa: F401  (multi-GPU driver; analytic data generator used by tests and bench)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSDSFM_LIB") or os.path.join(_HERE, "librsdsfm_hip.so")
# opt-in build of the same sources with explicit fused multiply-adds in the per-pixel model (csrc/device_math.hpp)
LIB_PATH_FUSED = os.path.join(_HERE, "librsdsfm_hip_fused.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "rsdsfm.h")

OK = 0
ERR_PENDING = -5
DEPTH_CLOSED_FORM, DEPTH_CERES_LM = 0, 1
K_COMPAT, K_FIXED = 0, 1
FLOW_COMPAT_RANK, FLOW_GATHERED = 0, 1
REFINE_TRACE_COLS = 8  # rsdsfm_get_refine_trace
TRACE_REJECTED, TRACE_ACCEPTED, TRACE_INVALID, TRACE_PARAMETER_TOL, TRACE_FUNCTION_TOL, TRACE_ACCEPTED_GRADIENT_TOL = 0.0, 1.0, 2.0, 3.0, 4.0, 5.0
TERMINATION = {0: "gradient", 1: "parameter", 2: "function", 3: "max_iter", 4: "failure", 5: "min_radius"}

_libs = {}


class RsdsfmError(RuntimeError):
    pass


class LmSummary(C.Structure):
    _fields_ = [
        ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32),
        ("num_unsuccessful_steps", C.c_int32),
        ("termination", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("final_radius", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrameParams(C.Structure):
    _fields_ = [("ransac_trials", C.c_int32), ("use_acceleration_mode", C.c_int32), ("use_refinement", C.c_int32),
                ("depth_mode", C.c_int32), ("k_sign_mode", C.c_int32), ("flow_index_mode", C.c_int32), ("use_global_shutter_mode", C.c_int32),
                ("struct_bytes", C.c_int32), ("ransac_tol", C.c_double),
                ("flow_threshold", C.c_double), ("seed", C.c_uint64)]


class FrameJob(C.Structure):
    _fields_ = [("d_flow_img", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("gamma", C.c_double), ("d_depth_map", C.c_void_p), ("d_R", C.c_void_p), ("d_t", C.c_void_p), ("seed", C.c_uint64)]


class FrameResult(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("num_inliers", C.c_int64), ("best_trial", C.c_int32), ("flipped", C.c_int32),
                ("ransac_w", C.c_double * 3), ("ransac_v", C.c_double * 3), ("ransac_k", C.c_double),
                ("w", C.c_double * 3), ("v", C.c_double * 3), ("k", C.c_double), ("refine_summary", LmSummary),
                ("d_inliers", C.c_void_p), ("d_inlier_idx", C.c_void_p), ("d_scanline", C.c_void_p)]


class TiledInfo(C.Structure):
    _fields_ = [("nranks", C.c_int32), ("rank", C.c_int32), ("col0", C.c_int32), ("slab_cols", C.c_int32), ("shard_points", C.c_int64),
                ("shard_inliers", C.c_int64), ("host_syncs", C.c_int32), ("collectives", C.c_int32), ("ransac_rounds", C.c_int32), ("path_flags", C.c_int32)]


ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
DIST_ID_BYTES = 128


def dist_unique_id():
    """rank 0: the 128-byte RCCL unique id to share with the other ranks (rsdsfm_dist_unique_id)"""
    buf = C.create_string_buffer(DIST_ID_BYTES)
    rc = load_library().rsdsfm_dist_unique_id(buf)
    if rc != OK:
        raise RsdsfmError("rsdsfm_dist_unique_id failed (%d): RCCL not available?" % rc)
    return bytes(buf.raw)


def tiled_slab_bounds(cols, nranks, rank):
    """(col0, slab_cols, stride_cols) of `rank`'s column slab (rsdsfm_tiled_slab_bounds)"""
    c0, sc, per = C.c_int32(), C.c_int32(), C.c_int32()
    rc = load_library().rsdsfm_tiled_slab_bounds(C.c_int32(cols), C.c_int32(nranks), C.c_int32(rank), C.byref(c0), C.byref(sc), C.byref(per))
    if rc != OK:
        raise RsdsfmError("rsdsfm_tiled_slab_bounds failed (%d)" % rc)
    return c0.value, sc.value, per.value


def tiled_shard_bounds(n, nranks, rank):
    """(i0, count, stride) of `rank`'s contiguous shard of an n-point list (rsdsfm_tiled_shard_bounds)"""
    i0, cnt, per = C.c_int64(), C.c_int64(), C.c_int64()
    rc = load_library().rsdsfm_tiled_shard_bounds(C.c_int64(n), C.c_int32(nranks), C.c_int32(rank), C.byref(i0), C.byref(cnt), C.byref(per))
    if rc != OK:
        raise RsdsfmError("rsdsfm_tiled_shard_bounds failed (%d)" % rc)
    return i0.value, cnt.value, per.value


class RansacOut(C.Structure):
    _fields_ = [
        ("num_inliers", C.c_int64),
        ("best_trial", C.c_int32),
        ("_pad", C.c_int32),
        ("w", C.c_double * 3),
        ("v", C.c_double * 3),
        ("k", C.c_double),
        ("inlier_error", C.c_double),
        ("inlier_idx", C.c_void_p),
        ("inliers", C.c_void_p),
        ("alpha", C.c_void_p),
        ("alpha_k", C.c_void_p),
        ("mask", C.c_void_p),
        ("inv_depth", C.c_void_p),
        ("trial_count", C.c_void_p),
        ("trial_err", C.c_void_p),
        ("trial_vel", C.c_void_p),
        ("trial_steps", C.c_void_p),
    ]


def declared_symbols():
    """Names of every function include/rsdsfm.h, include/rsdsfm_retime.h, include/rsdsfm_shutter.h, include/rsdsfm_denoise.h,
    include/rsdsfm_denoise_spatial.h (which rsdsfm_denoise.h includes), include/rsdsfm_superres.h, include/rsdsfm_plate.h,
    include/rsdsfm_plate_medoid.h, include/rsdsfm_erase.h, include/rsdsfm_deblur.h and include/rsdsfm_noise.h declare (used by the CPU symbol-export
    test)."""
    return _declared("rsdsfm.h", "rsdsfm_retime.h", "rsdsfm_shutter.h", "rsdsfm_denoise.h", "rsdsfm_denoise_spatial.h", "rsdsfm_superres.h", "rsdsfm_plate.h",
                     "rsdsfm_plate_medoid.h", "rsdsfm_erase.h", "rsdsfm_deblur.h", "rsdsfm_noise.h")


def load_library(build_if_missing=True, arith="reference"):
    """Loads librsdsfm_hip.so (arith="reference", the default: the reference's unfused arithmetic) or the opt-in
    librsdsfm_hip_fused.so (arith="fused"), building them with hipcc when absent and hipcc exists.  Raises otherwise."""
    if arith in _libs:
        return _libs[arith]
    if arith not in ("reference", "fused"):
        raise RsdsfmError("arith must be 'reference' or 'fused'")
    path = LIB_PATH if arith == "reference" else LIB_PATH_FUSED
    if not os.path.exists(path):
        if not build_if_missing:
            raise RsdsfmError("HIP extension %s is missing (run: python rs-aware-differential-sfm_amd/build.py)" % path)
        from . import build as _build

        _build.build()
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (same soname as /opt/rocm's).  If this
    # library were loaded first it would pull in the system runtime and a later `import torch` would find "No HIP GPUs".
    # Importing torch first (when it is installed) makes both share torch's runtime.
    if "torch" not in sys.modules and os.environ.get("RSDSFM_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(path)
    lib.rsdsfm_version.restype = C.c_char_p
    lib.rsdsfm_last_error.restype = C.c_char_p
    lib.rsdsfm_last_error.argtypes = [C.c_void_p]
    lib.rsdsfm_kernel_name.restype = C.c_char_p
    lib.rsdsfm_kernel_name.argtypes = [C.c_char_p]
    lib.rsdsfm_destroy.restype = None
    lib.rsdsfm_destroy.argtypes = [C.c_void_p]
    if lib.rsdsfm_fused_arithmetic() != (1 if arith == "fused" else 0):
        raise RsdsfmError("%s reports the wrong arithmetic mode (stale build?)" % path)
    _libs[arith] = lib
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _v3(a):
    return (C.c_double * 3)(*[float(x) for x in a])


def _dp(ptr):
    """device pointer (int / torch data_ptr) -> c_void_p"""
    return C.c_void_p(int(ptr))


class Solver:
    """One context = one HIP device + one stream (single owner).  `stream`: a raw hipStream_t handle to adopt,
    e.g. torch.cuda.current_stream().cuda_stream, or None for a private stream."""

    def __init__(self, device=0, stream=None, arith="reference"):
        """arith: "reference" (default) = librsdsfm_hip.so, the reference's unfused arithmetic; "fused" = the opt-in
        librsdsfm_hip_fused.so (same ABI, explicit fmas in the per-pixel model)"""
        self.lib = load_library(arith=arith)
        self.arith = arith
        self._ctx = C.c_void_p()
        rc = self.lib.rsdsfm_create(C.byref(self._ctx), int(device), C.c_void_p(stream) if stream else None)
        if rc != OK:
            self._ctx = None
            raise RsdsfmError("rsdsfm_create(device=%d) failed with %d (no usable gfx950 device? there is no CPU fallback)" % (device, rc))

    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.rsdsfm_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != OK:
            msg = self.lib.rsdsfm_last_error(self._ctx)
            raise RsdsfmError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def set_depth_variant(self, variant):
        """0 = register-staged fused LM kernel (default), 1 = LDS-DMA double-buffered variant"""
        self._check(self.lib.rsdsfm_set_depth_variant(self._ctx, int(variant)), "rsdsfm_set_depth_variant")

    def set_profiling(self, on):
        self._check(self.lib.rsdsfm_set_profiling(self._ctx, int(bool(on))), "rsdsfm_set_profiling")

    def profile_last_ms(self, what="ransac_lm_round0"):
        ms = C.c_double()
        self._check(self.lib.rsdsfm_profile_last_ms(self._ctx, what.encode(), C.byref(ms)), "rsdsfm_profile_last_ms")
        return ms.value

    def set_refine_stage(self, mode):
        """where the refinement's single-workgroup stage runs: 0 (default) = automatic, 1 = in the next pass's prologue, 2 = a launch of its own
        (rsdsfm_set_refine_stage); never a result"""
        self._check(self.lib.rsdsfm_set_refine_stage(self._ctx, int(mode)), "rsdsfm_set_refine_stage")

    def set_ransac_speculation(self, k0):
        """LM iterations speculated by round 0 of RANSAC's batched depth solves: 0 (default) = automatic, follows the context's previous
        solve (2 when none of its hypotheses went beyond one accepted step, else 3); 2 or 3 = fixed.  Scheduling only: never a result."""
        self._check(self.lib.rsdsfm_set_ransac_speculation(self._ctx, int(k0)), "rsdsfm_set_ransac_speculation")

    def set_ransac_math(self, mode):
        """round 0 of RANSAC's batched depth solves: 0 (default) = in-range cores of sqrt / reciprocal with a restart on an argument out
        of range, 1 = always the standard functions (rsdsfm_set_ransac_math); never a result"""
        self._check(self.lib.rsdsfm_set_ransac_math(self._ctx, int(mode)), "rsdsfm_set_ransac_math")

    def set_lm_arithmetic(self, mode):
        """arithmetic of the depth solves inside a RANSAC: 0 = analytic LM trajectory with guards (default), 1 = iterate by iterate
        (rsdsfm_set_lm_arithmetic); integer outputs never depend on it"""
        self._check(self.lib.rsdsfm_set_lm_arithmetic(self._ctx, int(mode)), "rsdsfm_set_lm_arithmetic")

    def set_refine_arithmetic(self, mode):
        """the joint refinement's arithmetic on its own: 0 (default) = radius-factorised while set_lm_arithmetic is 0, 1 = iterate by iterate"""
        self._check(self.lib.rsdsfm_set_refine_arithmetic(self._ctx, int(mode)), "rsdsfm_set_refine_arithmetic")

    def refine_restarts(self):
        """(refinements on the radius-factorised path, those a guard sent back to the iterate-by-iterate kernels, reduced systems solved
        again from stored sums, the guard that tripped last) -- rsdsfm_refine_restarts"""
        n, r, sv, g = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._check(self.lib.rsdsfm_refine_restarts(self._ctx, C.byref(n), C.byref(r), C.byref(sv), C.byref(g)), "rsdsfm_refine_restarts")
        return dict(runs=n.value, restarts=r.value, resolves=sv.value, last_guard=g.value)

    def lma_restarts(self):
        """(RANSAC runs of this context that started over because a guard of the analytic trajectory tripped, bit set of the last guards)"""
        n, g = C.c_int64(0), C.c_int32(0)
        self._check(self.lib.rsdsfm_lma_restarts(self._ctx, C.byref(n), C.byref(g)), "rsdsfm_lma_restarts")
        return int(n.value), int(g.value)

    def lma_count_only(self):
        """(RANSACs of frame solves that ran the count-only form of the analytic pass, those of them that had to fetch error sums)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.rsdsfm_lma_count_only(self._ctx, C.byref(a), C.byref(b)), "rsdsfm_lma_count_only")
        return int(a.value), int(b.value)

    def lma_predict_stats(self):
        """(hypotheses whose pixel pass fused their predicted iterate alone, those of them that ended there) -- rsdsfm_lma_predict_stats"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.rsdsfm_lma_predict_stats(self._ctx, C.byref(a), C.byref(b)), "rsdsfm_lma_predict_stats")
        return int(a.value), int(b.value)

    def ransac_restarts(self):
        """RANSAC runs of this context that started over with the standard functions (rsdsfm_ransac_restarts)"""
        n = C.c_int64()
        self._check(self.lib.rsdsfm_ransac_restarts(self._ctx, C.byref(n)), "rsdsfm_ransac_restarts")
        return n.value

    def depth_restarts(self):
        """dense depth solves of this context that started over with the standard functions (rsdsfm_depth_restarts)"""
        n = C.c_int64()
        self._check(self.lib.rsdsfm_depth_restarts(self._ctx, C.byref(n)), "rsdsfm_depth_restarts")
        return int(n.value)

    def synchronize(self):
        self._check(self.lib.rsdsfm_synchronize(self._ctx), "rsdsfm_synchronize")

    # ---- minimal:: ----
    def get_alpha(self, flow_px, h, gamma):
        flow_px = _f64(flow_px)
        n = flow_px.shape[0]
        out = np.empty(n)
        self._check(self.lib.rsdsfm_get_alpha(self._ctx, _p(flow_px), C.c_int64(n), C.c_double(h), C.c_double(gamma), _p(out)), "rsdsfm_get_alpha")
        return out

    def get_alpha_k(self, q_px, flow_px, h, gamma):
        q_px, flow_px = _f64(q_px), _f64(flow_px)
        n = flow_px.shape[0]
        out = np.empty(n)
        self._check(self.lib.rsdsfm_get_alpha_k(self._ctx, _p(q_px), _p(flow_px), C.c_int64(n), C.c_double(h), C.c_double(gamma), _p(out)), "rsdsfm_get_alpha_k")
        return out

    def calculate_velocities(self, q, u, alpha, alpha_k, use_alpha_k=False, k_sign_mode=K_COMPAT):
        """q, u: (T, 9, 2) or (9, 2); alpha, alpha_k: (T, 9) or (9,).  Returns w (T,3), v (T,3), k (T,)."""
        q, u, alpha, alpha_k = _f64(q), _f64(u), _f64(alpha), _f64(alpha_k)
        single = q.ndim == 2
        T = 1 if single else q.shape[0]
        w, v, k = np.empty((T, 3)), np.empty((T, 3)), np.empty(T)
        self._check(self.lib.rsdsfm_calculate_velocities(self._ctx, _p(q), _p(u), _p(alpha), _p(alpha_k), C.c_int32(T), int(use_alpha_k), int(k_sign_mode), _p(w), _p(v), _p(k)), "rsdsfm_calculate_velocities")
        return (w[0], v[0], float(k[0])) if single else (w, v, k)

    def ransac(self, q, u, alpha, alpha_k, use_alpha_k, iterations, tolerance, samples=None, seed=0, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, outputs=None):
        """outputs: None = fresh arrays, copies returned; a dict (empty at first) = caller-owned output arrays kept in it and REUSED by the
        next call with the same dict -- the returned arrays are then views into them (what a caller that streams frames does: no page faults
        of fresh arrays, no copies, inside the call)"""
        q, u, alpha, alpha_k = _f64(q), _f64(u), _f64(alpha), _f64(alpha_k)
        n, T = q.shape[0], int(iterations)
        smp = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32).reshape(-1)
        reuse = outputs is not None
        if reuse and outputs.get("_shape") == (n, T):
            bufs = outputs["_bufs"]
        else:
            bufs = dict(
                inlier_idx=np.zeros(n, dtype=np.int64), inliers=np.zeros((n, 3)), alpha=np.zeros(n), alpha_k=np.zeros(n),
                mask=np.zeros(n, dtype=np.uint8), inv_depth=np.zeros(n), trial_count=np.zeros(max(T, 1), dtype=np.int64),
                trial_err=np.zeros(max(T, 1)), trial_vel=np.zeros((max(T, 1), 7)), trial_steps=np.zeros(max(T, 1), dtype=np.int32),
            )
            if reuse:
                outputs["_shape"], outputs["_bufs"] = (n, T), bufs
        out = RansacOut()
        for name, arr in bufs.items():
            # (outputs["only"]: the arrays the caller wants filled -- e.g. what the reference's RansacValues holds: inliers, alpha, alpha_k (+ indices);
            # the others stay NULL and are neither computed for the host nor copied)
            if not reuse or "only" not in outputs or name in outputs["only"]:
                setattr(out, name, arr.ctypes.data)
        self._check(self.lib.rsdsfm_ransac(self._ctx, _p(q), _p(u), _p(alpha), _p(alpha_k), C.c_int64(n), int(use_alpha_k), C.c_int32(T), C.c_double(tolerance), _p(smp), C.c_uint64(seed), int(depth_mode), int(k_sign_mode), C.byref(out)), "rsdsfm_ransac")
        m = int(out.num_inliers)
        tag, hits = C.c_uint64(0), C.c_int64(0)
        self._check(self.lib.rsdsfm_last_ransac_tag(self._ctx, C.byref(tag), C.byref(hits)), "rsdsfm_last_ransac_tag")
        return dict(
            tag=int(tag.value),  # names the device-resident copy of this result: non_linear_refinement(..., tag=...) starts from it
            num_inliers=m, best_trial=int(out.best_trial), w=np.array(out.w[:]), v=np.array(out.v[:]), k=float(out.k),
            inlier_error=float(out.inlier_error), inlier_idx=bufs["inlier_idx"][:m] if reuse else bufs["inlier_idx"][:m].copy(),
            inliers=bufs["inliers"][:m] if reuse else bufs["inliers"][:m].copy(), alpha=bufs["alpha"][:m] if reuse else bufs["alpha"][:m].copy(),
            alpha_k=bufs["alpha_k"][:m] if reuse else bufs["alpha_k"][:m].copy(), mask=bufs["mask"], inv_depth=bufs["inv_depth"],
            trial_count=bufs["trial_count"][:T], trial_err=bufs["trial_err"][:T], trial_vel=bufs["trial_vel"][:T],
            trial_steps=bufs["trial_steps"][:T],
        )

    # ---- nonlinear_refinement:: ----
    def estimate_inverse_depths(self, q, u, v, w, k, alpha, alpha_k, mode=DEPTH_CERES_LM):
        q, u, alpha, alpha_k = _f64(q), _f64(u), _f64(alpha), _f64(alpha_k)
        n = q.shape[0]
        rho = np.empty(n)
        sm = LmSummary()
        self._check(self.lib.rsdsfm_estimate_inverse_depths(self._ctx, _p(q), _p(u), C.c_int64(n), _v3(v), _v3(w), C.c_double(k), _p(alpha), _p(alpha_k), int(mode), _p(rho), C.byref(sm)), "rsdsfm_estimate_inverse_depths")
        return rho, sm.as_dict()

    def estimate_inverse_depth(self, q, v, w, flow, k, alpha, alpha_k, mode=DEPTH_CERES_LM):
        """single-pixel variant (nonlinearRefinement.cc:55-106)"""
        rho, _ = self.estimate_inverse_depths(np.asarray(q).reshape(1, 2), np.asarray(flow).reshape(1, 2), v, w, k, [alpha], [alpha_k], mode)
        return float(rho[0])

    def refine_cache_hits(self):
        """refinements of this context that started from the device-resident outputs of a RANSAC (rsdsfm_refine_from_ransac)"""
        tag, hits = C.c_uint64(0), C.c_int64(0)
        self._check(self.lib.rsdsfm_last_ransac_tag(self._ctx, C.byref(tag), C.byref(hits)), "rsdsfm_last_ransac_tag")
        return int(hits.value)

    def non_linear_refinement(self, flow, inliers, alpha, alpha_k, v, w, k, const_acceleration=False, flow_index_mode=FLOW_COMPAT_RANK, inlier_idx=None, tag=0, out=None):
        """tag: `tag` of the ransac() result these arrays are the UNMODIFIED outputs of (0: upload everything) -- rsdsfm_refine_from_ransac;
        out: a caller-owned (m, 3) array for the refined inliers (None: a fresh one)"""
        flow, inliers, alpha, alpha_k = _f64(flow), _f64(inliers), _f64(alpha), _f64(alpha_k)
        m = inliers.shape[0]
        idx = None if inlier_idx is None else np.ascontiguousarray(inlier_idx, dtype=np.int64)
        if out is None or out.shape != (m, 3) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
            out = np.empty((m, 3))
        vo, wo, ko = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double()
        sm = LmSummary()
        if tag:
            self._check(self.lib.rsdsfm_refine_from_ransac(self._ctx, C.c_uint64(int(tag)), _p(flow), C.c_int64(flow.shape[0]), C.c_int64(m), _p(inliers), _p(alpha), _p(alpha_k), _p(idx), _v3(v), _v3(w), C.c_double(k), int(const_acceleration), int(flow_index_mode), _p(out), vo, wo, C.byref(ko), C.byref(sm)), "rsdsfm_refine_from_ransac")
        else:
            self._check(self.lib.rsdsfm_refine(self._ctx, _p(flow), C.c_int64(flow.shape[0]), C.c_int64(m), _p(inliers), _p(alpha), _p(alpha_k), _p(idx), _v3(v), _v3(w), C.c_double(k), int(const_acceleration), int(flow_index_mode), _p(out), vo, wo, C.byref(ko), C.byref(sm)), "rsdsfm_refine")
        return dict(inliers=out, v=np.array(vo[:]), w=np.array(wo[:]), k=ko.value, summary=sm.as_dict())

    def set_refine_trace(self, rows):
        """rows > 0: record the first `rows` LM iterations of every following refinement (rsdsfm_set_refine_trace); 0 = off"""
        self._check(self.lib.rsdsfm_set_refine_trace(self._ctx, C.c_int32(int(rows))), "rsdsfm_set_refine_trace")
        self._refine_trace_rows = int(rows)

    def get_refine_trace(self, rows=None):
        """(rows, 8) array of the last refinement: iteration, cost, candidate cost, model cost change, relative decrease, radius,
        step norm, outcome (TRACE_*); NaN = not computed / no such iteration"""
        rows = getattr(self, "_refine_trace_rows", 0) if rows is None else int(rows)
        out = np.empty((max(rows, 1), REFINE_TRACE_COLS))
        self._check(self.lib.rsdsfm_get_refine_trace(self._ctx, _p(out), C.c_int32(rows)), "rsdsfm_get_refine_trace")
        return out[:rows]

    # ---- caller glue ----
    def flatten(self, flow_img, K, gamma, thr=1e-10):
        flow_img = _f64(flow_img)
        rows, cols = flow_img.shape[:2]
        n = rows * cols
        q, u, a, ak = np.empty((n, 2)), np.empty((n, 2)), np.empty(n), np.empty(n)
        cnt = C.c_int64()
        d = C.c_double
        self._check(self.lib.rsdsfm_flatten(self._ctx, _p(flow_img), C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma), d(thr), _p(q), _p(u), _p(a), _p(ak), C.byref(cnt)),
                "rsdsfm_flatten")
        m = cnt.value
        return q[:m].copy(), u[:m].copy(), a[:m].copy(), ak[:m].copy()

    def depth_map(self, inliers, v, K, rows, cols):
        inl = _f64(inliers).copy()
        m = inl.shape[0]
        vv = _v3(v)
        dm = np.zeros((cols, rows))
        xs, ys = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        flipped = C.c_int()
        self._check(self.lib.rsdsfm_depth_map(self._ctx, _p(inl), C.c_int64(m), vv, *_k4(K), C.c_int32(rows), C.c_int32(cols), _p(dm), _p(xs), _p(ys), C.byref(flipped)), "rsdsfm_depth_map")
        return dict(depth_map=dm.T.copy(), inliers=inl, v=np.array(vv[:]), xs=xs, ys=ys, flipped=bool(flipped.value))

    def pose_table(self, v, w, k, gamma, rows):
        R, t = np.empty((rows, 9)), np.empty((rows, 3))
        self._check(self.lib.rsdsfm_pose_table(self._ctx, _v3(v), _v3(w), C.c_double(k), C.c_double(gamma), C.c_int32(rows), _p(R), _p(t)), "rsdsfm_pose_table")
        return R.reshape(rows, 3, 3), t

    # ---- device API (raw device pointers, asynchronous) ----
    def estimate_inverse_depths_dev(self, d_q, d_u, n, v, w, k, d_alpha, d_alpha_k, d_rho, mode=DEPTH_CERES_LM):
        self._check(self.lib.rsdsfm_estimate_inverse_depths_dev(self._ctx, _dp(d_q), _dp(d_u), C.c_int64(n), _v3(v), _v3(w), C.c_double(k), _dp(d_alpha), _dp(d_alpha_k), int(mode), _dp(d_rho)), "rsdsfm_estimate_inverse_depths_dev")

    def prepared_depth_step(self, d_q, d_u, n, v, w, k, d_alpha, d_alpha_k, d_rho, mode=DEPTH_CERES_LM):
        """Returns a zero-argument callable that enqueues one dense depth solve with pre-marshalled arguments
        (keeps the per-step host cost at one foreign call; used by bench.py)."""
        fn = self.lib.rsdsfm_estimate_inverse_depths_dev
        args = (self._ctx, _dp(d_q), _dp(d_u), C.c_int64(n), _v3(v), _v3(w), C.c_double(k), _dp(d_alpha), _dp(d_alpha_k), C.c_int(int(mode)), _dp(d_rho))
        check = self._check

        def call():
            rc = fn(*args)
            if rc != OK:
                check(rc, "rsdsfm_estimate_inverse_depths_dev")

        return call

    def depth_lm_launch_dev(self, d_q, d_u, n, v, w, k, d_alpha, d_alpha_k, d_rho, launch_id=0):
        self._check(self.lib.rsdsfm_depth_lm_launch_dev(self._ctx, _dp(d_q), _dp(d_u), C.c_int64(n), _v3(v), _v3(w), C.c_double(k), _dp(d_alpha), _dp(d_alpha_k), _dp(d_rho), int(launch_id)), "rsdsfm_depth_lm_launch_dev")

    def flatten_dev(self, d_img, rows, cols, K, gamma, d_q, d_u, d_alpha, d_alpha_k, thr=1e-10):
        cnt = C.c_int64()
        d = C.c_double
        self._check(self.lib.rsdsfm_flatten_dev(self._ctx, _dp(d_img), C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma), d(thr), _dp(d_q), _dp(d_u), _dp(d_alpha),
                _dp(d_alpha_k), C.byref(cnt)), "rsdsfm_flatten_dev")
        return cnt.value

    def ransac_dev(self, d_q, d_u, d_alpha, d_alpha_k, n, use_alpha_k, iterations, tolerance, out_ptrs, samples=None, seed=0, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT):
        """out_ptrs: dict of DEVICE pointers (inlier_idx, inliers, alpha, alpha_k, mask, inv_depth; missing = not wanted)."""
        T = int(iterations)
        smp = None if samples is None else np.ascontiguousarray(samples, dtype=np.int32).reshape(-1)
        out = RansacOut()
        for name in ("inlier_idx", "inliers", "alpha", "alpha_k", "mask", "inv_depth"):
            setattr(out, name, int(out_ptrs[name]) if out_ptrs.get(name) else None)
        tc = np.zeros(max(T, 1), dtype=np.int64)
        ts = np.zeros(max(T, 1), dtype=np.int32)
        out.trial_count, out.trial_steps = tc.ctypes.data, ts.ctypes.data
        self._check(self.lib.rsdsfm_ransac_dev(self._ctx, _dp(d_q), _dp(d_u), _dp(d_alpha), _dp(d_alpha_k), C.c_int64(n), int(use_alpha_k), C.c_int32(T), C.c_double(tolerance), _p(smp), C.c_uint64(seed), int(depth_mode), int(k_sign_mode), C.byref(out)), "rsdsfm_ransac_dev")
        return dict(num_inliers=int(out.num_inliers), best_trial=int(out.best_trial), w=np.array(out.w[:]), v=np.array(out.v[:]), k=float(out.k),
                    inlier_error=float(out.inlier_error), trial_count=tc[:T], trial_steps=ts[:T])

    def refine_dev(self, d_flow, n_flow, m, d_inl, d_alpha, d_alpha_k, d_idx, v, w, k, const_acceleration, flow_index_mode, d_inl_out):
        vo, wo, ko = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double()
        sm = LmSummary()
        self._check(self.lib.rsdsfm_refine_dev(self._ctx, _dp(d_flow), C.c_int64(n_flow), C.c_int64(m), _dp(d_inl), _dp(d_alpha), _dp(d_alpha_k), _dp(d_idx) if d_idx else None, _v3(v), _v3(w), C.c_double(k), int(const_acceleration), int(flow_index_mode), _dp(d_inl_out), vo, wo, C.byref(ko), C.byref(sm)), "rsdsfm_refine_dev")
        return dict(v=np.array(vo[:]), w=np.array(wo[:]), k=ko.value, summary=sm.as_dict())

    def depth_map_dev(self, d_inl, m, v, K, rows, cols, d_depth_map, d_xs=None, d_ys=None):
        vv = _v3(v)
        flipped = C.c_int()
        self._check(self.lib.rsdsfm_depth_map_dev(self._ctx, _dp(d_inl), C.c_int64(m), vv, *_k4(K), C.c_int32(rows), C.c_int32(cols), _dp(d_depth_map),
                _dp(d_xs) if d_xs else None, _dp(d_ys) if d_ys else None, C.byref(flipped)), "rsdsfm_depth_map_dev")
        return np.array(vv[:]), bool(flipped.value)

    def pose_table_dev(self, v, w, k, gamma, rows, d_R, d_t):
        self._check(self.lib.rsdsfm_pose_table_dev(self._ctx, _v3(v), _v3(w), C.c_double(k), C.c_double(gamma), C.c_int32(rows), _dp(d_R), _dp(d_t)), "rsdsfm_pose_table_dev")

    def solve_frame_dev(self, d_flow_img, rows, cols, K, gamma, d_depth_map, d_R=None, d_t=None, trials=50, tol=0.05, seed=1,
                        use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10,
                        flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False):
        """the whole solve of one frame pair in ONE C-ABI call (rsdsfm_solve_frame_dev).  Defaults = evaluateSingleRun: the
        refinement reads the flow by inlier RANK (quirk Q2, main.cc:457); pass flow_index_mode=FLOW_GATHERED for the flow of each
        inlier's own pixel."""
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), int(seed))
        res = FrameResult()
        d = C.c_double
        self._check(self.lib.rsdsfm_solve_frame_dev(self._ctx, _dp(d_flow_img), C.c_int32(rows), C.c_int32(cols), *_k4(K),
                                                    d(gamma), C.byref(prm), _dp(d_depth_map), _dp(d_R) if d_R else None, _dp(d_t) if d_t else None,
                                                    C.byref(res)), "rsdsfm_solve_frame_dev")
        return dict(n=int(res.n_points), num_inliers=int(res.num_inliers), best_trial=int(res.best_trial), flipped=bool(res.flipped),
                    ransac_w=np.array(res.ransac_w[:]), ransac_v=np.array(res.ransac_v[:]), ransac_k=float(res.ransac_k),
                    w=np.array(res.w[:]), v=np.array(res.v[:]), k=float(res.k), refine_summary=res.refine_summary.as_dict(),
                    d_inliers=res.d_inliers, d_inlier_idx=res.d_inlier_idx, d_scanline=res.d_scanline)

    # ---- the column-tiled whole solve driven inside the library (RCCL or caller-provided collectives) ----
    def dist_init(self, nranks, rank, unique_id):
        """collective: creates the RCCL communicator of this context from the shared 128-byte id (rsdsfm_dist_init)"""
        self._check(self.lib.rsdsfm_dist_init(self._ctx, C.c_int32(nranks), C.c_int32(rank), C.c_char_p(bytes(unique_id))), "rsdsfm_dist_init")

    def dist_set_transport(self, nranks, rank, all_gather, all_reduce):
        """caller-provided collectives (Python callables taking (d_send, d_recv, bytes_per_rank, stream) / (d_buf, count, stream) and
        returning 0) instead of RCCL; the ctypes thunks are kept alive on the solver"""
        self._ag = ALL_GATHER_FN(lambda user, s_, r_, b_, st: int(all_gather(s_, r_, b_, st)))
        self._ar = ALL_REDUCE_FN(lambda user, p_, n_, st: int(all_reduce(p_, n_, st)))
        self._check(self.lib.rsdsfm_dist_set_transport(self._ctx, C.c_int32(nranks), C.c_int32(rank), self._ag, self._ar, None), "rsdsfm_dist_set_transport")

    def dist_finalize(self):
        self._check(self.lib.rsdsfm_dist_finalize(self._ctx), "rsdsfm_dist_finalize")

    def solve_frame_tiled_dev(self, d_img_slab, rows, cols, K, gamma, d_depth_map, d_R=None, d_t=None, trials=50, tol=0.05, seed=1,
                              use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT,
                              flow_threshold=1e-10, use_global_shutter_mode=False, flow_index_mode=FLOW_COMPAT_RANK):
        """this rank's part of the column-tiled whole solve (rsdsfm_solve_frame_tiled_dev): d_img_slab = this rank's [rows][slab_cols][2]
        slab, cols = width of the whole image; returns the dict of solve_frame_dev (global counts) plus the slab's info.  Defaults as
        solve_frame_dev: the refinement reads the flow by GLOBAL inlier rank (quirk Q2, main.cc:457) -- the columns a rank needs from
        the slabs in front of it are exchanged inside the call; FLOW_GATHERED = the flow of each inlier's own pixel."""
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), int(seed))
        res, info = FrameResult(), TiledInfo()
        d = C.c_double
        self._check(self.lib.rsdsfm_solve_frame_tiled_dev(self._ctx, _dp(d_img_slab) if d_img_slab else None, C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma), C.byref(prm),
                                                          _dp(d_depth_map), _dp(d_R) if d_R else None,
                                                          _dp(d_t) if d_t else None, C.byref(res), C.byref(info)), "rsdsfm_solve_frame_tiled_dev")
        return dict(n=int(res.n_points), num_inliers=int(res.num_inliers), best_trial=int(res.best_trial), flipped=bool(res.flipped),
                    ransac_w=np.array(res.ransac_w[:]), ransac_v=np.array(res.ransac_v[:]), ransac_k=float(res.ransac_k),
                    w=np.array(res.w[:]), v=np.array(res.v[:]), k=float(res.k), refine_summary=res.refine_summary.as_dict(),
                    d_inliers=res.d_inliers, d_inlier_idx=res.d_inlier_idx, d_scanline=res.d_scanline, flow_index_mode=int(flow_index_mode),
                    info={k2: int(getattr(info, k2)) for k2, _ in TiledInfo._fields_ if k2 != "_pad"})

    def estimate_inverse_depths_tiled_dev(self, d_q_shard, d_u_shard, n_total, v, w, k, d_alpha_shard, d_alpha_k_shard, d_inv_depth,
                                          mode=DEPTH_CERES_LM):
        """this rank's part of the row-tiled dense depth solve (rsdsfm_estimate_inverse_depths_tiled_dev): the shard pointers are
        this rank's tiled_shard_bounds slice; d_inv_depth receives all n_total inverse depths.  Returns (lm summary dict or None, info)"""
        sm, info = LmSummary(), TiledInfo()
        opt = lambda p_: _dp(p_) if p_ else None
        self._check(self.lib.rsdsfm_estimate_inverse_depths_tiled_dev(self._ctx, opt(d_q_shard), opt(d_u_shard), C.c_int64(n_total), _v3(v), _v3(w),
                                                                      C.c_double(k), opt(d_alpha_shard), opt(d_alpha_k_shard), C.c_int(int(mode)),
                                                                      opt(d_inv_depth), C.byref(sm), C.byref(info)),
                    "rsdsfm_estimate_inverse_depths_tiled_dev")
        return (sm.as_dict() if int(mode) == DEPTH_CERES_LM else None,
                {k2: int(getattr(info, k2)) for k2, _ in TiledInfo._fields_ if k2 != "_pad"})

    def prepared_frame_solve(self, d_flow_img, rows, cols, K, gamma, d_depth_map, d_R=None, d_t=None, trials=50, tol=0.05,
                             use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT,
                             flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False):
        """Returns call(seed) -> FrameResult for repeated whole solves with pre-marshalled arguments (one foreign call per solve;
        the host-side cost of building the argument structures and the result dict -- ~30 us in Python, during which the GPU
        idles -- is paid once).  The returned ctypes struct is reused by the next call."""
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 0)
        res = FrameResult()
        d = C.c_double
        fn = self.lib.rsdsfm_solve_frame_dev
        args = (self._ctx, _dp(d_flow_img), C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma), C.byref(prm),
                _dp(d_depth_map), _dp(d_R) if d_R else None, _dp(d_t) if d_t else None, C.byref(res))
        check = self._check

        def call(seed):
            prm.seed = seed
            rc = fn(*args)
            if rc != OK:
                check(rc, "rsdsfm_solve_frame_dev")
            return res

        return call

    def set_sequence_lanes(self, lanes):
        """pairs in flight of solve_frames_dev (rsdsfm_set_sequence_lanes): 1..16, 0 = default (3); scheduling only"""
        self._check(self.lib.rsdsfm_set_sequence_lanes(self._ctx, C.c_int32(int(lanes))), "rsdsfm_set_sequence_lanes")

    def set_frame_side_flatten(self, on):
        """where a dense frame's flatten runs (rsdsfm_set_frame_side_flatten): 3 (default) inside the minimal solver's launch (spare
        workgroups flatten while T waves solve), 2 behind the solver, 1 beside it on a second stream, 0 in front of it; scheduling only"""
        self._check(self.lib.rsdsfm_set_frame_side_flatten(self._ctx, int(on)), "rsdsfm_set_frame_side_flatten")

    def set_frame_tail(self, mode):
        """the launches at the end of a frame solve (rsdsfm_set_frame_tail): 0 (default) the output pass claims the depth-map pixels and one
        kernel decides the sign and writes the map, 1 the stage-by-stage launches; identical results"""
        self._check(self.lib.rsdsfm_set_frame_tail(self._ctx, int(mode)), "rsdsfm_set_frame_tail")

    def set_frame_handoff(self, mode):
        """how a frame solve's refinement gets its inliers (rsdsfm_set_frame_handoff): 0 (default) the first refinement pass gathers them from
        the final stage's block-local lists, 1 the compaction launch; identical results"""
        self._check(self.lib.rsdsfm_set_frame_handoff(self._ctx, int(mode)), "rsdsfm_set_frame_handoff")

    def set_frame_predict(self, mode):
        """the pixel pass of a dense frame's RANSAC (rsdsfm_set_frame_predict): 0 (default) each hypothesis fuses the iterate the solver's launch
        predicted for it, 1 both iterates for every hypothesis, 2 the prediction inverted and the pass's scores discarded (tests); identical outputs of the frame solve"""
        self._check(self.lib.rsdsfm_set_frame_predict(self._ctx, int(mode)), "rsdsfm_set_frame_predict")

    def set_lma_operands(self, mode):
        """where the lanes of the analytic pixel pass take their pixel's operands from (rsdsfm_set_lma_operands): 0 (default) a record one thread
        per pixel leaves in LDS (groups of fewer than 16 hypotheses: as 1), 1 every lane's own global loads, 2 the record for every hypothesis count
        (tests); identical outputs"""
        self._check(self.lib.rsdsfm_set_lma_operands(self._ctx, int(mode)), "rsdsfm_set_lma_operands")

    def prepared_frames_solve(self, jobs, trials=50, tol=0.05, use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM,
                              k_sign_mode=K_COMPAT, flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False):
        """A SEQUENCE of frame pairs in ONE C-ABI call (rsdsfm_solve_frames_dev), pipelined inside the library.  jobs: list of dicts with
        d_flow_img, rows, cols, K, gamma, d_depth_map and optionally d_R, d_t (device pointers).  Returns call(seeds) -> list of
        FrameResult (the ctypes array is reused by the next call); seeds: one sampler seed per pair."""
        n = len(jobs)
        arr = (FrameJob * n)()
        for a, j in zip(arr, jobs):
            K = j["K"]
            a.d_flow_img, a.rows, a.cols = int(j["d_flow_img"]), int(j["rows"]), int(j["cols"])
            a.fx, a.fy, a.cx, a.cy, a.gamma = float(K[0]), float(K[1]), float(K[2]), float(K[3]), float(j["gamma"])
            a.d_depth_map, a.d_R, a.d_t = int(j["d_depth_map"]), int(j.get("d_R") or 0) or None, int(j.get("d_t") or 0) or None
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 0)
        res = (FrameResult * n)()
        fn, ctx, check = self.lib.rsdsfm_solve_frames_dev, self._ctx, self._check

        def call(seeds):
            for a, sd in zip(arr, seeds):
                a.seed = int(sd)
            rc = fn(ctx, arr, C.c_int32(n), C.byref(prm), res)
            if rc != OK:
                check(rc, "rsdsfm_solve_frames_dev")
            return res

        return call

    def solve_frames_dev(self, jobs, seeds, **kw):
        """rsdsfm_solve_frames_dev once; returns one dict per pair (as solve_frame_dev)"""
        res = self.prepared_frames_solve(jobs, **kw)(seeds)
        return [dict(n=int(r.n_points), num_inliers=int(r.num_inliers), best_trial=int(r.best_trial), flipped=bool(r.flipped),
                     ransac_w=np.array(r.ransac_w[:]), ransac_v=np.array(r.ransac_v[:]), ransac_k=float(r.ransac_k),
                     w=np.array(r.w[:]), v=np.array(r.v[:]), k=float(r.k), refine_summary=r.refine_summary.as_dict(),
                     d_inliers=r.d_inliers, d_inlier_idx=r.d_inlier_idx, d_scanline=r.d_scanline) for r in res]

    def depth_lm_reduce_dev(self, n_shard, d_row):
        self._check(self.lib.rsdsfm_depth_lm_reduce_dev(self._ctx, C.c_int64(n_shard), _dp(d_row)), "rsdsfm_depth_lm_reduce_dev")

    def depth_lm_decide_rows_dev(self, d_rows, nrows, n_total, launch_id):
        self._check(self.lib.rsdsfm_depth_lm_decide_rows_dev(self._ctx, _dp(d_rows), C.c_int32(nrows), C.c_int64(n_total), int(launch_id)), "rsdsfm_depth_lm_decide_rows_dev")

    def depth_lm_state(self):
        status, nxt, sm = C.c_int32(), C.c_int32(), LmSummary()
        self._check(self.lib.rsdsfm_depth_lm_state(self._ctx, C.byref(status), C.byref(nxt), C.byref(sm)), "rsdsfm_depth_lm_state")
        return status.value, nxt.value, sm.as_dict()

    def depth_finish_dev(self, d_q, d_u, n, v, w, k, d_alpha, d_alpha_k, d_rho):
        sm = LmSummary()
        extra = C.c_int32()
        self._check(self.lib.rsdsfm_depth_finish_dev(self._ctx, _dp(d_q), _dp(d_u), C.c_int64(n), _v3(v), _v3(w), C.c_double(k), _dp(d_alpha), _dp(d_alpha_k), _dp(d_rho), C.byref(sm), C.byref(extra)), "rsdsfm_depth_finish_dev")
        return sm.as_dict(), extra.value


# ---------------------------------------------------------------------------------------------------
# the marshalling kit: what the stage sections below build their calls from, each idiom once.  A helper returns the numpy and ctypes arrays
# themselves, never a bare address: _p() stays in the call expression, so nothing a call reads can be collected before the call returns.
# ---------------------------------------------------------------------------------------------------
def _header_path(name):
    return os.path.join(os.path.dirname(_HERE), "include", name)


def _declared(*headers):
    """the rsdsfm_* names the given headers of include/ declare"""
    import re

    txt = re.sub(r"/\*.*?\*/", "", "".join(open(_header_path(h)).read() for h in headers), flags=re.S)
    return sorted(set(re.findall(r"\b(rsdsfm_[a-z0-9_]+)\s*\(", txt)))


def _solver_methods(mixin):
    """class decorator of a stage section's mixin: its functions become Solver's methods (a mixin is a namespace, not a base class)"""
    for name, fn in list(vars(mixin).items()):
        if not name.startswith("__"):
            setattr(Solver, name, fn)
    return mixin


def _ref(struct):
    """an optional parameter struct by reference; NULL (the library's defaults) for None"""
    return None if struct is None else C.byref(struct)


def _ptrs(ptrs, n=None):
    """an optional list of device pointers -> a C array of the first n (None: all of them); NULL for None, and for no entries wanted"""
    if ptrs is None or n == 0:
        return None
    return _ptr_array(list(ptrs) if n is None else list(ptrs)[:n])


def _need_all(n, **lists):
    for what, lst in lists.items():
        _need_entries(what, lst, n)


def _need_entries(what, lst, n):
    """a clip wrapper's list must have an entry for every frame the call writes: the library reads exactly n pointers"""
    if lst is not None and len(lst) < n:
        raise RsdsfmError("%s has %d entries, the call needs %d (one per rendered frame; last_frame=True renders every frame of the clip)" % (what, len(lst), n))


def _frame_front(what, d_images, M, m, **lists):
    """the front of a frame call: ns sources, every list with an entry for each, every source with a pose -> (ns, M as (-1, 9), m as (-1, 3))"""
    ns = len(d_images)
    _need_all(ns, **lists)
    Mm, mm = _f64(M).reshape(-1, 9), _f64(m).reshape(-1, 3)
    if Mm.shape[0] < ns or mm.shape[0] < ns:
        raise RsdsfmError("%s: every source needs a pose (M, m)" % what)
    return ns, Mm, mm


def _clip_front(what, d_depth_maps, A, c, A_path, c_path, scales, **lists):
    """the front of a clip call: as many sources as depth maps, every list with an entry for each, every source with a pose on both paths and a
    scale -> (ns, A, c, A_path, c_path as (-1, 9) / (-1, 3), scales as (-1))"""
    ns = len(d_depth_maps)
    _need_all(ns, **lists)
    a, cc, ap, cp, sc = _f64(A).reshape(-1, 9), _f64(c).reshape(-1, 3), _f64(A_path).reshape(-1, 9), _f64(c_path).reshape(-1, 3), _f64(scales).reshape(-1)
    if min(a.shape[0], cc.shape[0], ap.shape[0], cp.shape[0], sc.shape[0]) < ns:
        raise RsdsfmError("%s: every source needs a pose on both paths and a scale" % what)
    return ns, a, cc, ap, cp, sc


def _counts(want, n, *shape, dtype=np.int64, fill=0):
    """a per-frame result buffer the library fills, n (at least one) rows of `shape`; None when it is not wanted"""
    return np.full((max(n, 1),) + shape, fill, dtype=dtype) if want else None


def _wanted(n, **buffers):
    """the first n rows of every buffer that was wanted, by name: what a clip call returns"""
    return {name: buf[:n] for name, buf in buffers.items() if buf is not None}


class _Staging:
    """host arrays onto a device, library calls on them, the results back -- the one place (beside load_library) that imports torch and the one place
    the order is written: up() (torch fills the plane on ITS stream) -> ready(), a device-wide wait: a plane is complete before its pointer is
    handed out, because the library works on another stream -> the library calls -> down(): Solver.synchronize(), then the copies to the host.  A
    convenience with two phases (stabilize_filled) calls wait() and ready() between them itself."""

    def __init__(self, solver, device):
        import torch

        self.torch, self.solver, self.dev = torch, solver, torch.device("cuda", device)
        self._on = torch.cuda.device(self.dev)

    def __enter__(self):
        self._on.__enter__()
        return self

    def __exit__(self, *exc):
        return self._on.__exit__(*exc)

    def up(self, a, dtype=None):
        """a host array, made contiguous (and of dtype), on the device; None stays None"""
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def up64(self, a):
        """uint64 words, which torch does not have: they travel as int64"""
        return self.up(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64))

    def up_frame(self, image, depth_map, R, t):
        """a source as the frame calls take it: the uint8 image, the depth map column-major, the pose table as (rows, 9) and (rows, 3) doubles"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        return self.up(img), self.up(np.asarray(depth_map, dtype=np.float64).T), self.up(_f64(np.asarray(R).reshape(img.shape[0], 9))), self.up(_f64(t))

    def empty(self, shape, dtype="uint8"):
        return self.torch.empty(shape, dtype=getattr(self.torch, dtype), device=self.dev)

    def zeros(self, shape, dtype="uint8"):
        return self.torch.zeros(shape, dtype=getattr(self.torch, dtype), device=self.dev)

    def full(self, shape, value, dtype):
        return self.torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=getattr(self.torch, dtype), device=self.dev)

    def empty_like(self, t):
        return self.torch.empty_like(t)

    def zeros_like(self, t):
        return self.torch.zeros_like(t)

    @staticmethod
    def ptrs(tensors):
        return None if tensors is None else [t.data_ptr() for t in tensors]

    def ready(self):
        self.torch.cuda.synchronize()

    def wait(self):
        self.solver.synchronize()

    @staticmethod
    def host(t):
        return t.cpu().numpy()

    def down(self, *tensors):
        self.wait()
        return tuple(self.host(t) for t in tensors)


def _params(struct, init, lib=None, **words):
    """a parameter struct over the library's defaults: `init` fills it, then every word given a value other than None is set, as the int or the
    float its field holds"""
    p = struct()
    if getattr(lib or load_library(), init)(C.byref(p)) != OK:
        raise RsdsfmError("%s failed" % init)
    for name, value in words.items():
        if value is not None:
            setattr(p, name, type(getattr(p, name))(value))
    return p


def _launches(entry, admits, *sizes):
    """a *_launches entry point: int32 sizes in, the number of kernel launches out; a negative answer is a refusal and `admits` says what is taken"""
    n = getattr(load_library(), entry)(*[C.c_int32(x) for x in sizes])
    if n < 0:
        raise RsdsfmError("%s failed (%d): %s" % (entry, n, admits))
    return n


def _k4(K):
    """K = (fx, fy, cx, cy) as the four doubles every entry point takes: *_k4(K)"""
    return C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3])


# ---------------------------------------------------------------------------------------------------
# stage-level wrappers of the row-tiled whole-frame solve (include/rsdsfm.h "ROW-TILED WHOLE-FRAME"; driver: dist.py)
# ---------------------------------------------------------------------------------------------------
def _np0(ptr):
    return _dp(ptr) if ptr else None


def tile_sizes():
    """(bytes per LM state, bytes of the winner record, doubles per LM row, hypotheses per rows call)"""
    lib = load_library()
    lib.rsdsfm_tile_lm_state_bytes.restype = C.c_size_t
    lib.rsdsfm_tile_best_bytes.restype = C.c_size_t
    return (int(lib.rsdsfm_tile_lm_state_bytes()), int(lib.rsdsfm_tile_best_bytes()), int(lib.rsdsfm_tile_ransac_row_size()),
            int(lib.rsdsfm_tile_ransac_batch()))


def sample_indices(n, iterations, seed):
    """the deterministic sampler of rsdsfm_ransac (host side): [iterations, 9] int32 global indices"""
    lib = load_library()
    out = np.zeros((max(int(iterations), 0), 9), dtype=np.int32)
    rc = lib.rsdsfm_sample_indices(C.c_int64(n), C.c_int32(iterations), C.c_uint64(seed), _p(out))
    if rc != OK:
        raise RsdsfmError("rsdsfm_sample_indices failed (%d): needs 9 <= n < 2^31" % rc)
    return out


@_solver_methods
class _TileMixin:
    def flatten_slab_dev(self, d_img_slab, rows, slab_cols, col0, K, gamma, d_q, d_u, d_alpha, d_alpha_k, thr=1e-10):
        cnt = C.c_int64()
        d = C.c_double
        self._check(self.lib.rsdsfm_flatten_slab_dev(self._ctx, _np0(d_img_slab), C.c_int32(rows), C.c_int32(slab_cols), C.c_int32(col0), *_k4(K), d(gamma), d(thr), _np0(d_q),
                _np0(d_u), _np0(d_alpha), _np0(d_alpha_k), C.byref(cnt)), "rsdsfm_flatten_slab_dev")
        return cnt.value

    def minimal9_probe_dev(self, d_q9, d_u9, d_a9, d_ak9, count, use_alpha_k, k_sign_mode, use_cores, d_hyp, d_probe4):
        """the wave-per-hypothesis minimal solver with per-hypothesis {SVD sweeps, rotations, SVD clocks, total clocks} (rsdsfm_minimal9_probe_dev)"""
        self._check(self.lib.rsdsfm_minimal9_probe_dev(self._ctx, _dp(d_q9), _dp(d_u9), _dp(d_a9), _dp(d_ak9), C.c_int32(count), int(use_alpha_k), int(k_sign_mode),
                                                       int(use_cores), _dp(d_hyp), _dp(d_probe4)), "rsdsfm_minimal9_probe_dev")

    def minimal9_dev(self, d_q9, d_u9, d_a9, d_ak9, count, use_alpha_k, k_sign_mode, d_hyp):
        self._check(self.lib.rsdsfm_minimal9_dev(self._ctx, _np0(d_q9), _np0(d_u9), _np0(d_a9), _np0(d_ak9), C.c_int32(count), int(use_alpha_k), int(k_sign_mode), _np0(d_hyp)), "rsdsfm_minimal9_dev")

    def tile_ransac_lm_rows_dev(self, d_q, d_u, d_a, d_ak, n, d_hyp, count, d_states, rnd, tol, d_rows):
        self._check(self.lib.rsdsfm_tile_ransac_lm_rows_dev(self._ctx, _np0(d_q), _np0(d_u), _np0(d_a), _np0(d_ak), C.c_int64(n), _dp(d_hyp), C.c_int32(count), _dp(d_states), C.c_int32(rnd), C.c_double(tol), _dp(d_rows)), "rsdsfm_tile_ransac_lm_rows_dev")

    def tile_ransac_decide_dev(self, d_rows_all, nranks, count, d_states, n_total, rnd, d_flags, d_scored, d_tcount, d_terr):
        self._check(self.lib.rsdsfm_tile_ransac_decide_dev(self._ctx, _dp(d_rows_all), C.c_int32(nranks), C.c_int32(count), _dp(d_states), C.c_int64(n_total), C.c_int32(rnd), _dp(d_flags), _dp(d_scored), _dp(d_tcount), _dp(d_terr)), "rsdsfm_tile_ransac_decide_dev")

    def tile_ransac_score_rows_dev(self, d_q, d_u, d_a, d_ak, n, d_hyp, count, d_states, depth_mode, tol, d_scored, d_rows):
        self._check(self.lib.rsdsfm_tile_ransac_score_rows_dev(self._ctx, _np0(d_q), _np0(d_u), _np0(d_a), _np0(d_ak), C.c_int64(n), _dp(d_hyp), C.c_int32(count), _dp(d_states), int(depth_mode), C.c_double(tol), _np0(d_scored), _dp(d_rows)), "rsdsfm_tile_ransac_score_rows_dev")

    def tile_ransac_score_merge_dev(self, d_rows_all, nranks, count, d_scored, d_tcount, d_terr):
        self._check(self.lib.rsdsfm_tile_ransac_score_merge_dev(self._ctx, _dp(d_rows_all), C.c_int32(nranks), C.c_int32(count), _np0(d_scored), _dp(d_tcount), _dp(d_terr)), "rsdsfm_tile_ransac_score_merge_dev")

    def tile_ransac_pick_dev(self, d_tcount, d_terr, iterations, d_hyp, d_best):
        self._check(self.lib.rsdsfm_tile_ransac_pick_dev(self._ctx, _np0(d_tcount), _np0(d_terr), C.c_int32(iterations), _np0(d_hyp), _dp(d_best)), "rsdsfm_tile_ransac_pick_dev")

    def tile_ransac_final_dev(self, d_q, d_u, d_a, d_ak, n, d_best, d_states, depth_mode, tol, d_rho, d_mask, d_idx, d_inl, d_oa, d_oak):
        out = RansacOut()
        self._check(self.lib.rsdsfm_tile_ransac_final_dev(self._ctx, _np0(d_q), _np0(d_u), _np0(d_a), _np0(d_ak), C.c_int64(n), _dp(d_best), _dp(d_states), int(depth_mode), C.c_double(tol), _np0(d_rho), _np0(d_mask), _np0(d_idx), _np0(d_inl), _np0(d_oa), _np0(d_oak), C.byref(out)), "rsdsfm_tile_ransac_final_dev")
        return dict(shard_inliers=int(out.num_inliers), best_trial=int(out.best_trial), w=np.array(out.w[:]), v=np.array(out.v[:]), k=float(out.k), inlier_error=float(out.inlier_error))

    def tile_ransac_global_inliers(self, d_best):
        self.lib.rsdsfm_tile_ransac_global_inliers.restype = C.c_int64
        r = int(self.lib.rsdsfm_tile_ransac_global_inliers(self._ctx, _dp(d_best)))
        if r < 0:
            raise RsdsfmError("rsdsfm_tile_ransac_global_inliers failed")
        return r

    def tile_refine_begin_dev(self, d_flow, n_flow, m, d_inl, d_alpha, d_alpha_k, d_idx, v, w, k, const_acceleration, flow_index_mode=FLOW_GATHERED):
        self._check(self.lib.rsdsfm_tile_refine_begin_dev(self._ctx, _np0(d_flow), C.c_int64(n_flow), C.c_int64(m), _np0(d_inl), _np0(d_alpha), _np0(d_alpha_k), _np0(d_idx), _v3(v), _v3(w), C.c_double(k), int(const_acceleration), int(flow_index_mode)), "rsdsfm_tile_refine_begin_dev")

    def tile_refine_row_size(self, const_acceleration, stage):
        return int(self.lib.rsdsfm_tile_refine_row_size(int(const_acceleration), C.c_int32(stage)))

    def tile_refine_rows_dev(self, stage, d_row):
        self._check(self.lib.rsdsfm_tile_refine_rows_dev(self._ctx, C.c_int32(stage), _dp(d_row)), "rsdsfm_tile_refine_rows_dev")

    def tile_refine_apply_dev(self, stage, d_rows_all, nranks, m_total):
        self._check(self.lib.rsdsfm_tile_refine_apply_dev(self._ctx, C.c_int32(stage), _dp(d_rows_all), C.c_int32(nranks), C.c_int64(m_total)), "rsdsfm_tile_refine_apply_dev")

    def tile_refine_poll(self):
        vo, wo, ko = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double()
        sm = LmSummary()
        self._check(self.lib.rsdsfm_tile_refine_poll(self._ctx, vo, wo, C.byref(ko), C.byref(sm)), "rsdsfm_tile_refine_poll")
        return dict(v=np.array(vo[:]), w=np.array(wo[:]), k=ko.value, summary=sm.as_dict(), running=sm.termination < 0)

    def tile_refine_finish_dev(self, d_inl_out):
        self._check(self.lib.rsdsfm_tile_refine_finish_dev(self._ctx, _np0(d_inl_out)), "rsdsfm_tile_refine_finish_dev")

    def tile_zsum_dev(self, d_inl, m, d_zsum):
        self._check(self.lib.rsdsfm_tile_zsum_dev(self._ctx, _np0(d_inl), C.c_int64(m), _dp(d_zsum)), "rsdsfm_tile_zsum_dev")

    def tile_depth_map_dev(self, d_inl, m, d_zsums_all, nranks, m_total, v, K, rows, col0, slab_cols, d_depth_slab, d_xs=None, d_ys=None):
        vv = _v3(v)
        flipped = C.c_int()
        self._check(self.lib.rsdsfm_tile_depth_map_dev(self._ctx, _np0(d_inl), C.c_int64(m), _dp(d_zsums_all), C.c_int32(nranks), C.c_int64(m_total), vv, *_k4(K), C.c_int32(rows),
                C.c_int32(col0), C.c_int32(slab_cols), _np0(d_depth_slab), _np0(d_xs), _np0(d_ys), C.byref(flipped)), "rsdsfm_tile_depth_map_dev")
        return np.array(vv[:]), bool(flipped.value)


# ---------------------------------------------------------------------------------------------------
# consumers of the solve's output: back projection, crack interpolation, 8-bit depth image
# ---------------------------------------------------------------------------------------------------
BACKPROJECT_RS, BACKPROJECT_GS = 0, 1
Q5_COMPAT, Q5_FIXED = 0, 1


@_solver_methods
class _RectifyMixin:
    def back_project(self, image_bgr, depth_map, R, t, K, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, want_coords=True):
        """RsFrame::backProject / backProjectGs.  depth_map: (rows, cols) array; R: (rows, 3, 3) or (rows, 9); t: (rows, 3)."""
        img = np.ascontiguousarray(image_bgr, dtype=np.uint8)
        rows, cols = img.shape[:2]
        dm = np.ascontiguousarray(np.asarray(depth_map, dtype=np.float64).T)  # column-major rows x cols
        Rr, tt = _f64(np.asarray(R).reshape(rows, 9)), _f64(t)
        gs = np.zeros_like(img)
        c3 = np.zeros((rows, cols, 3), dtype=np.float32) if want_coords else None
        self._check(self.lib.rsdsfm_back_project(self._ctx, _p(img), _p(dm), _p(Rr), _p(tt), *_k4(K), C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), _p(gs), _p(c3)),
                "rsdsfm_back_project")
        return gs, c3

    def back_project_dev(self, d_img, d_depth_map, d_R, d_t, K, rows, cols, d_gs, d_coords=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT):
        self._check(self.lib.rsdsfm_back_project_dev(self._ctx, _dp(d_img), _dp(d_depth_map), _dp(d_R), _dp(d_t), *_k4(K), C.c_int32(rows), C.c_int32(cols), int(mode),
                int(q5_mode), _dp(d_gs), _dp(d_coords) if d_coords else None), "rsdsfm_back_project_dev")

    def interpolate_cracky(self, image_bgr, offset=1):
        img = np.ascontiguousarray(image_bgr, dtype=np.uint8)
        rows, cols = img.shape[:2]
        out = np.zeros_like(img)
        self._check(self.lib.rsdsfm_interpolate_cracky(self._ctx, _p(img), C.c_int32(rows), C.c_int32(cols), C.c_int32(offset), _p(out)), "rsdsfm_interpolate_cracky")
        return out

    def interpolate_cracky_dev(self, d_in, rows, cols, d_out, offset=1):
        self._check(self.lib.rsdsfm_interpolate_cracky_dev(self._ctx, _dp(d_in), C.c_int32(rows), C.c_int32(cols), C.c_int32(offset), _dp(d_out)), "rsdsfm_interpolate_cracky_dev")

    def depth_preview(self, inliers, K, rows, cols):
        inl = _f64(inliers).reshape(-1, 3)
        out = np.zeros((rows, cols), dtype=np.uint8)
        self._check(self.lib.rsdsfm_depth_preview(self._ctx, _p(inl), C.c_int64(inl.shape[0]), *_k4(K), C.c_int32(rows), C.c_int32(cols), _p(out)), "rsdsfm_depth_preview")
        return out

    def depth_preview_dev(self, d_inl, m, K, rows, cols, d_out):
        self._check(self.lib.rsdsfm_depth_preview_dev(self._ctx, _np0(d_inl), C.c_int64(m), *_k4(K), C.c_int32(rows), C.c_int32(cols), _dp(d_out)), "rsdsfm_depth_preview_dev")

    def rectify_frame_dev(self, d_inl, m, d_img, d_depth_map, d_R, d_t, K, rows, cols, d_preview, d_gs, d_fixed, d_coords=None, mode=BACKPROJECT_RS,
                          q5_mode=Q5_COMPAT, offset=1):
        """main.cc:480-523 in one call (rsdsfm_rectify_frame_dev): depth image + back projection + crack interpolation, two launches (three when
        the interpolation offset exceeds 2 or cols is not a multiple of 4)"""
        self._check(self.lib.rsdsfm_rectify_frame_dev(self._ctx, _np0(d_inl), C.c_int64(m), _dp(d_img), _dp(d_depth_map), _dp(d_R), _dp(d_t), *_k4(K), C.c_int32(rows),
                                                      C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(offset),
                                                      _dp(d_preview), _dp(d_gs), _np0(d_coords), _dp(d_fixed)), "rsdsfm_rectify_frame_dev")


# ---------------------------------------------------------------------------------------------------
# ground-truth flow between two rolling-shutter frames
# ---------------------------------------------------------------------------------------------------
@_solver_methods
class _TrueFlowMixin:
    def set_true_flow_search(self, mode):
        """0 / False (default): interval-pruned exact search from 96 scanlines on; 1 / True: every scanline for every pixel; 2: pruned
        at any size (rsdsfm_set_true_flow_search).  Identical results."""
        self._check(self.lib.rsdsfm_set_true_flow_search(self._ctx, int(mode)), "rsdsfm_set_true_flow_search")

    def true_flow(self, world_xyz, R2, t2, K, q5_mode=Q5_COMPAT, want_best_row=True):
        """Camera::calculateTrueFlow.  world_xyz: (rows, cols, 3) world point per pixel of frame 1 (zeros = void);
        R2: (rows2, 3, 3) or (rows2, 9); t2: (rows2, 3).  Returns flow (rows, cols, 2) and the winning scanlines."""
        w = np.asarray(world_xyz, dtype=np.float64)
        rows, cols = w.shape[:2]
        maps = [np.ascontiguousarray(w[:, :, c].T) for c in range(3)]  # column-major rows x cols (Eigen MatrixXd)
        tt = _f64(t2)
        rows2 = tt.shape[0]
        Rr = _f64(np.asarray(R2).reshape(rows2, 9))
        flow = np.zeros((rows, cols, 2))
        best = np.zeros((rows, cols), dtype=np.int32) if want_best_row else None
        self._check(self.lib.rsdsfm_true_flow(self._ctx, _p(maps[0]), _p(maps[1]), _p(maps[2]), C.c_int32(rows), C.c_int32(cols), _p(Rr), _p(tt), C.c_int32(rows2), *_k4(K),
                int(q5_mode), _p(flow), _p(best)), "rsdsfm_true_flow")
        return flow, best

    def true_flow_dev(self, d_wx, d_wy, d_wz, rows, cols, d_R2, d_t2, rows2, K, d_flow, d_best_row=None, q5_mode=Q5_COMPAT):
        self._check(self.lib.rsdsfm_true_flow_dev(self._ctx, _dp(d_wx), _dp(d_wy), _dp(d_wz), C.c_int32(rows), C.c_int32(cols), _dp(d_R2), _dp(d_t2), C.c_int32(rows2), *_k4(K),
                int(q5_mode), _dp(d_flow), _dp(d_best_row) if d_best_row else None), "rsdsfm_true_flow_dev")


# ---------------------------------------------------------------------------------------------------
# DeepFlow front end: two 8-bit frames -> dense flow (include/rsdsfm_flow.h; camera.cc:253-277)
# ---------------------------------------------------------------------------------------------------
FLOW_HEADER_PATH = _header_path("rsdsfm_flow.h")


class FlowParams(C.Structure):
    _fields_ = [("sigma", C.c_double), ("min_size", C.c_int32), ("downscale", C.c_double), ("fixed_point_iterations", C.c_int32),
                ("sor_iterations", C.c_int32), ("alpha", C.c_double), ("delta", C.c_double), ("gamma", C.c_double), ("omega", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def flow_declared_symbols():
    """Names of every function include/rsdsfm_flow.h declares"""
    return _declared("rsdsfm_flow.h")


def flow_default_params():
    """createOptFlow_DeepFlow()'s defaults as a dict (rsdsfm_flow_default_params)"""
    p = FlowParams()
    if load_library().rsdsfm_flow_default_params(C.byref(p)) != OK:
        raise RsdsfmError("rsdsfm_flow_default_params failed")
    return p.as_dict()


def _flow_params(params):
    """None -> NULL (defaults); a dict (or FlowParams) -> a FlowParams with the given keys over the defaults"""
    if params is None:
        return None
    if isinstance(params, FlowParams):
        return params
    d = flow_default_params()
    unknown = set(params) - set(d)
    if unknown:
        raise ValueError("unknown flow parameters %s" % sorted(unknown))
    d.update(params)
    return FlowParams(**d)


def flow_levels(rows, cols, params=None):
    """the pyramid DeepFlow builds for a rows x cols pair: list of (rows, cols), level 0 first (host only)"""
    lib = load_library()
    p = _flow_params(params)
    n = C.c_int32(0)
    pp = _ref(p)
    if lib.rsdsfm_flow_levels(C.c_int32(rows), C.c_int32(cols), pp, C.byref(n), None, None) != OK:
        raise RsdsfmError("rsdsfm_flow_levels: bad arguments")
    lr, lc = (C.c_int32 * n.value)(), (C.c_int32 * n.value)()
    if lib.rsdsfm_flow_levels(C.c_int32(rows), C.c_int32(cols), pp, C.byref(n), lr, lc) != OK:
        raise RsdsfmError("rsdsfm_flow_levels failed")
    return [(lr[i], lc[i]) for i in range(n.value)]


@_solver_methods
class _DeepFlowMixin:
    def deep_flow(self, img1, img2, params=None):
        """Camera::calculateDeepFlow: two uint8 images (rows, cols, 3) BGR or (rows, cols[, 1]) gray -> flow (rows, cols, 2) float64"""
        a, b = np.ascontiguousarray(img1, dtype=np.uint8), np.ascontiguousarray(img2, dtype=np.uint8)
        if a.shape != b.shape or a.ndim not in (2, 3):
            raise ValueError("the two images must have the same (rows, cols[, channels]) shape")
        rows, cols = a.shape[:2]
        ch = 1 if a.ndim == 2 else a.shape[2]
        p = _flow_params(params)
        flow = np.empty((rows, cols, 2))
        self._check(self.lib.rsdsfm_deep_flow(self._ctx, _p(a), _p(b), C.c_int32(rows), C.c_int32(cols), C.c_int32(ch),
                                              _ref(p), _p(flow)), "rsdsfm_deep_flow")
        return flow

    def deep_flow_dev(self, d_img1, d_img2, rows, cols, channels, d_flow, params=None):
        """the same on device buffers, enqueued on the context's stream (no host wait)"""
        p = _flow_params(params)
        self._check(self.lib.rsdsfm_deep_flow_dev(self._ctx, _dp(d_img1), _dp(d_img2), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels),
                                                  _ref(p), _dp(d_flow)), "rsdsfm_deep_flow_dev")


# ---------------------------------------------------------------------------------------------------
# whole clips: frames in, the flow of every consecutive pair and its solve out (include/rsdsfm_video.h)
# ---------------------------------------------------------------------------------------------------
VIDEO_HEADER_PATH = _header_path("rsdsfm_video.h")


def video_declared_symbols():
    """Names of every function include/rsdsfm_video.h declares"""
    return _declared("rsdsfm_video.h")


def _ptr_array(ptrs):
    """a list of device pointers (ints / data_ptr(); 0 = NULL) -> a C array of void*"""
    return (C.c_void_p * len(ptrs))(*[int(p) or None for p in ptrs])


def _frame_result_dict(r):
    return dict(n=int(r.n_points), num_inliers=int(r.num_inliers), best_trial=int(r.best_trial), flipped=bool(r.flipped),
                ransac_w=np.array(r.ransac_w[:]), ransac_v=np.array(r.ransac_v[:]), ransac_k=float(r.ransac_k),
                w=np.array(r.w[:]), v=np.array(r.v[:]), k=float(r.k), refine_summary=r.refine_summary.as_dict(),
                d_inliers=r.d_inliers, d_inlier_idx=r.d_inlier_idx, d_scanline=r.d_scanline)


@_solver_methods
class _VideoMixin:
    def set_flow_batch(self, pairs):
        """pairs per batch of the clip calls (rsdsfm_set_flow_batch): 1..32, 0 = the default (8); scheduling only (it sizes the
        context's sequence workspace, about (120 B + 41 (B + 1)) bytes per pixel)"""
        self._check(self.lib.rsdsfm_set_flow_batch(self._ctx, C.c_int32(int(pairs))), "rsdsfm_set_flow_batch")

    def deep_flow_seq(self, frames, params=None):
        """DeepFlow of every consecutive pair of a clip: uint8 (F, rows, cols, 3) BGR or (F, rows, cols) gray -> (F - 1, rows, cols, 2)
        float64; flows[p] is deep_flow(frames[p], frames[p + 1]) bit for bit"""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.ndim not in (3, 4) or f.shape[0] < 2:
            raise ValueError("frames must be (F >= 2, rows, cols[, channels])")
        nf, rows, cols = f.shape[:3]
        ch = 1 if f.ndim == 3 else f.shape[3]
        p = _flow_params(params)
        flows = np.empty((nf - 1, rows, cols, 2))
        self._check(self.lib.rsdsfm_deep_flow_seq(self._ctx, _ptr_array([f[i].ctypes.data for i in range(nf)]), C.c_int32(nf), C.c_int32(rows),
                                                  C.c_int32(cols), C.c_int32(ch), _ref(p),
                                                  _ptr_array([flows[i].ctypes.data for i in range(nf - 1)])), "rsdsfm_deep_flow_seq")
        return flows

    def deep_flow_seq_dev(self, d_frames, rows, cols, channels, d_flows, params=None):
        """the same on device buffers (lists of F frame and F - 1 field pointers), enqueued on the context's stream (no host wait)"""
        p = _flow_params(params)
        self._check(self.lib.rsdsfm_deep_flow_seq_dev(self._ctx, _ptr_array(d_frames), C.c_int32(len(d_frames)), C.c_int32(rows), C.c_int32(cols),
                                                      C.c_int32(channels), _ref(p), _ptr_array(d_flows)),
                    "rsdsfm_deep_flow_seq_dev")

    def solve_video_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, seeds=None, d_flows=None, d_R=None, d_t=None, flow_params=None,
                        trials=50, tol=0.05, use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT,
                        flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False):
        """a whole clip in ONE call (rsdsfm_solve_video_dev): the flow of each batch of pairs, then solve_frames_dev over that batch.
        d_frames: F device frames; d_depth_maps (and optionally d_flows, d_R, d_t): F - 1 device buffers each (d_flows=None: a ring
        owned by the library); seeds: one per pair (None: 1).  Returns one dict per pair, as solve_frames_dev."""
        n = len(d_frames) - 1
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 1)
        res = (FrameResult * max(n, 1))()
        sd = (C.c_uint64 * n)(*[int(s) for s in seeds]) if seeds is not None else None
        p = _flow_params(flow_params)
        d = C.c_double
        self._check(self.lib.rsdsfm_solve_video_dev(self._ctx, _ptr_array(d_frames), C.c_int32(len(d_frames)), C.c_int32(rows), C.c_int32(cols),
                                                    C.c_int32(channels), *_k4(K), d(gamma), _ref(p),
                                                    C.byref(prm), sd, _ptrs(d_flows), _ptr_array(d_depth_maps), _ptrs(d_R), _ptrs(d_t), res),
                    "rsdsfm_solve_video_dev")
        return [_frame_result_dict(r) for r in res[:n]]


# ---------------------------------------------------------------------------------------------------
# rectified products of whole clips, gray frames included (include/rsdsfm_rectify_video.h)
# ---------------------------------------------------------------------------------------------------
RECTIFY_VIDEO_HEADER_PATH = _header_path("rsdsfm_rectify_video.h")


def rectify_video_declared_symbols():
    """Names of every function include/rsdsfm_rectify_video.h declares"""
    return _declared("rsdsfm_rectify_video.h")


@_solver_methods
class _RectifyVideoMixin:
    def rectify_gray_frame_dev(self, d_inl, m, d_img, d_depth_map, d_R, d_t, K, rows, cols, d_preview, d_gs, d_fixed, d_coords=None, mode=BACKPROJECT_RS,
                               q5_mode=Q5_COMPAT, offset=1):
        """rectify_frame_dev on a one-channel image (rsdsfm_rectify_gray_frame_dev): d_img, d_gs, d_fixed are rows x cols bytes; the outputs are
        channel 0 of rectify_frame_dev's for the image (g, g, g), the depth image and the world points are its bit for bit"""
        self._check(self.lib.rsdsfm_rectify_gray_frame_dev(self._ctx, _np0(d_inl), C.c_int64(m), _dp(d_img), _dp(d_depth_map), _dp(d_R), _dp(d_t), *_k4(K), C.c_int32(rows),
                                                           C.c_int32(cols), int(mode), int(q5_mode),
                                                           C.c_int32(offset), _dp(d_preview), _dp(d_gs), _np0(d_coords), _dp(d_fixed)),
                    "rsdsfm_rectify_gray_frame_dev")

    def rectify_video_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_depth_est, d_gs, d_fixed, d_coords=None, seeds=None,
                          d_flows=None, d_R=None, d_t=None, flow_params=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, offset=1, trials=50, tol=0.05,
                          use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10,
                          flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False):
        """solve_video_dev plus, per pair p, the rectification of frame p with pair p's solve, in ONE call (rsdsfm_rectify_video_dev).
        d_depth_est, d_gs, d_fixed (and optionally d_coords): F - 1 device buffers each -- rows x cols bytes, rows x cols x channels bytes
        (twice), rows x cols x 3 floats; channels 1 = gray frames and gray images.  All outputs are complete on return.  Returns one dict
        per pair, as solve_video_dev."""
        n = len(d_frames) - 1
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 1)
        res = (FrameResult * max(n, 1))()
        sd = (C.c_uint64 * n)(*[int(s) for s in seeds]) if seeds is not None else None
        p = _flow_params(flow_params)
        d = C.c_double
        self._check(self.lib.rsdsfm_rectify_video_dev(self._ctx, _ptr_array(d_frames), C.c_int32(len(d_frames)), C.c_int32(rows), C.c_int32(cols),
                                                      C.c_int32(channels), *_k4(K), d(gamma),
                                                      _ref(p), C.byref(prm), sd, _ptrs(d_flows), _ptr_array(d_depth_maps),
                                                      _ptrs(d_R), _ptrs(d_t), res, int(mode), int(q5_mode), C.c_int32(offset), _ptr_array(d_depth_est),
                                                      _ptr_array(d_gs), _ptr_array(d_fixed), _ptrs(d_coords)), "rsdsfm_rectify_video_dev")
        return [_frame_result_dict(r) for r in res[:n]]


# ---------------------------------------------------------------------------------------------------
# the dense global-shutter frame: depth fill + backward warp (include/rsdsfm_rectify_dense.h)
# ---------------------------------------------------------------------------------------------------
RECTIFY_DENSE_HEADER_PATH = _header_path("rsdsfm_rectify_dense.h")


def rectify_dense_declared_symbols():
    """Names of every function include/rsdsfm_rectify_dense.h declares"""
    return _declared("rsdsfm_rectify_dense.h")


def rectify_dense_launches(rows, cols):
    """kernel launches of one rectify_dense_frame_dev call at this size (rsdsfm_rectify_dense_launches; host only)"""
    return _launches("rsdsfm_rectify_dense_launches", "rows and cols must be in [2, 16384]", rows, cols)


@_solver_methods
class _RectifyDenseMixin:
    def rectify_dense_frame_dev(self, d_img, channels, d_depth_map, d_R, d_t, K, rows, cols, d_dense, d_mask=None, d_filled=None, d_disp=None,
                                mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """the hole-free, sub-pixel global-shutter frame (rsdsfm_rectify_dense_frame_dev): push-pull fill of the inverse depth, the splat's
        chain per pixel as a displacement plane, and its fixed-point inverse sampled bilinearly.  d_img / d_dense rows x cols x channels
        bytes; optional d_mask rows x cols bytes, d_filled rows x cols doubles (column-major, like d_depth_map), d_disp rows x cols x 2
        floats; iterations 1..16, 0 = the default (3).  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_rectify_dense_frame_dev(self._ctx, _dp(d_img), C.c_int32(channels), _dp(d_depth_map), _dp(d_R), _dp(d_t), *_k4(K), C.c_int32(rows),
                                                            C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations),
                                                            _dp(d_dense), _np0(d_mask), _np0(d_filled), _np0(d_disp)), "rsdsfm_rectify_dense_frame_dev")

    def rectify_dense(self, image, depth_map, R, t, K, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, device=0):
        """host convenience around rectify_dense_frame_dev: image (rows, cols) or (rows, cols, 3) uint8, depth_map (rows, cols) (0 where
        unknown), R (rows, 3, 3) / (rows, 9), t (rows, 3).  Returns (dense image, mask)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = img.shape[:2]
        with _Staging(self, device) as st:
            d_img, d_dm, d_R, d_t = st.up_frame(img, depth_map, R, t)
            d_out, d_mask = st.empty_like(d_img), st.empty((rows, cols))
            st.ready()
            self.rectify_dense_frame_dev(d_img.data_ptr(), 1 if img.ndim == 2 else img.shape[2], d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols,
                                         d_out.data_ptr(), d_mask.data_ptr(), mode=mode, q5_mode=q5_mode, iterations=iterations)
            return st.down(d_out, d_mask)
    def rectify_dense_video_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_dense, d_masks=None, d_filled=None, seeds=None,
                                d_flows=None, d_R=None, d_t=None, flow_params=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, trials=50,
                                tol=0.05, use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT,
                                flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False):
        """solve_video_dev plus, per pair p and on that pair's lane, rectify_dense_frame_dev of frame p with pair p's depth map and pose
        table, in ONE call (rsdsfm_rectify_dense_video_dev).  d_dense (and optionally d_masks, d_filled): F - 1 device buffers each.  All
        outputs are complete on return.  Returns one dict per pair, as solve_video_dev."""
        n = len(d_frames) - 1
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 1)
        res = (FrameResult * max(n, 1))()
        sd = (C.c_uint64 * n)(*[int(s) for s in seeds]) if seeds is not None else None
        p = _flow_params(flow_params)
        d = C.c_double
        self._check(self.lib.rsdsfm_rectify_dense_video_dev(self._ctx, _ptr_array(d_frames), C.c_int32(len(d_frames)), C.c_int32(rows), C.c_int32(cols),
                                                            C.c_int32(channels), *_k4(K), d(gamma),
                                                            _ref(p), C.byref(prm), sd, _ptrs(d_flows), _ptr_array(d_depth_maps),
                                                            _ptrs(d_R), _ptrs(d_t), res, int(mode), int(q5_mode), C.c_int32(iterations), _ptr_array(d_dense),
                                                            _ptrs(d_masks), _ptrs(d_filled)), "rsdsfm_rectify_dense_video_dev")
        return [_frame_result_dict(r) for r in res[:n]]


# ---------------------------------------------------------------------------------------------------
# the forward-backward flow check: an occlusion mask that gates the solve (include/rsdsfm_flow_check.h)
# ---------------------------------------------------------------------------------------------------
FLOW_CHECK_HEADER_PATH = _header_path("rsdsfm_flow_check.h")


class FlowCheckParams(C.Structure):
    _fields_ = [("a1", C.c_double), ("a2", C.c_double)]


def flow_check_declared_symbols():
    """Names of every function include/rsdsfm_flow_check.h declares"""
    return _declared("rsdsfm_flow_check.h")


def flow_check_default_params():
    """the check's defaults as a dict: a1 = 0.01, a2 = 0.5 (rsdsfm_flow_check_default_params)"""
    p = FlowCheckParams()
    if load_library().rsdsfm_flow_check_default_params(C.byref(p)) != OK:
        raise RsdsfmError("rsdsfm_flow_check_default_params failed")
    return dict(a1=p.a1, a2=p.a2)


def _flow_check_params(a1, a2):
    """(None, None) -> NULL (the defaults); otherwise a FlowCheckParams with the given values over the defaults"""
    if a1 is None and a2 is None:
        return None
    d = flow_check_default_params()
    return FlowCheckParams(float(d["a1"] if a1 is None else a1), float(d["a2"] if a2 is None else a2))


@_solver_methods
class _FlowCheckMixin:
    def flow_consistency_dev(self, d_fwd, d_bwd, rows, cols, d_mask, d_masked=None, d_resid=None, d_count=None, a1=None, a2=None):
        """the forward-backward check on device fields (rsdsfm_flow_consistency_dev; tests/flow_check_spec_numpy.py): d_fwd / d_bwd
        rows x cols x 2 doubles, d_mask rows x cols bytes (4-byte aligned); optional d_masked rows x cols x 2 doubles (may be d_fwd),
        d_resid rows x cols doubles, d_count one int64.  One launch, enqueued on the context's stream."""
        k = _flow_check_params(a1, a2)
        self._check(self.lib.rsdsfm_flow_consistency_dev(self._ctx, _dp(d_fwd), _dp(d_bwd), C.c_int32(rows), C.c_int32(cols),
                                                         _ref(k), _dp(d_mask), _np0(d_masked), _np0(d_resid), _np0(d_count)),
                    "rsdsfm_flow_consistency_dev")

    def flow_consistency(self, fwd, bwd, a1=None, a2=None, device=0):
        """host convenience around flow_consistency_dev: two (rows, cols, 2) float64 fields in, dict(mask (rows, cols) uint8, masked
        (rows, cols, 2), resid (rows, cols), count) out"""
        f, b = _f64(fwd), _f64(bwd)
        if f.ndim != 3 or f.shape[2] != 2 or b.shape != f.shape:
            raise ValueError("the two fields must have the same (rows, cols, 2) shape")
        rows, cols = f.shape[:2]
        with _Staging(self, device) as st:
            d_f, d_b = st.up(f), st.up(b)
            d_mask, d_masked, d_resid, d_count = st.empty((rows, cols)), st.empty_like(d_f), st.empty((rows, cols), "float64"), st.empty(1, "int64")
            st.ready()
            self.flow_consistency_dev(d_f.data_ptr(), d_b.data_ptr(), rows, cols, d_mask.data_ptr(), d_masked.data_ptr(), d_resid.data_ptr(),
                                      d_count.data_ptr(), a1=a1, a2=a2)
            mask, masked, resid, count = st.down(d_mask, d_masked, d_resid, d_count)
            return dict(mask=mask, masked=masked, resid=resid, count=int(count[0]))
    def deep_flow_checked_dev(self, d_img1, d_img2, rows, cols, channels, d_flow, d_mask, d_bwd=None, d_count=None, params=None, a1=None, a2=None):
        """DeepFlow both ways and the check (rsdsfm_deep_flow_checked_dev): d_flow receives the MASKED forward field (solve_frame_dev can
        follow on the same stream), d_mask the mask, optionally d_bwd the backward field and d_count the number of consistent pixels"""
        p, k = _flow_params(params), _flow_check_params(a1, a2)
        self._check(self.lib.rsdsfm_deep_flow_checked_dev(self._ctx, _dp(d_img1), _dp(d_img2), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels),
                                                          _ref(p), _ref(k), _dp(d_flow),
                                                          _np0(d_bwd), _dp(d_mask), _np0(d_count)), "rsdsfm_deep_flow_checked_dev")

    def deep_flow_checked(self, img1, img2, params=None, a1=None, a2=None, device=0):
        """host convenience around deep_flow_checked_dev: two uint8 images as deep_flow takes them -> dict(flow (rows, cols, 2): the
        masked forward field, bwd (rows, cols, 2), mask (rows, cols) uint8, count)"""
        a, b = np.ascontiguousarray(img1, dtype=np.uint8), np.ascontiguousarray(img2, dtype=np.uint8)
        if a.shape != b.shape or a.ndim not in (2, 3):
            raise ValueError("the two images must have the same (rows, cols[, channels]) shape")
        rows, cols = a.shape[:2]
        with _Staging(self, device) as st:
            d_a, d_b = st.up(a), st.up(b)
            d_flow, d_bwd = (st.empty((rows, cols, 2), "float64") for _ in range(2))
            d_mask, d_count = st.empty((rows, cols)), st.empty(1, "int64")
            st.ready()
            self.deep_flow_checked_dev(d_a.data_ptr(), d_b.data_ptr(), rows, cols, 1 if a.ndim == 2 else a.shape[2], d_flow.data_ptr(), d_mask.data_ptr(),
                                       d_bwd=d_bwd.data_ptr(), d_count=d_count.data_ptr(), params=params, a1=a1, a2=a2)
            flow, bwd, mask, count = st.down(d_flow, d_bwd, d_mask, d_count)
            return dict(flow=flow, bwd=bwd, mask=mask, count=int(count[0]))
    def solve_video_checked_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_masks, seeds=None, d_flows=None, d_bwd_flows=None,
                                d_R=None, d_t=None, flow_params=None, a1=None, a2=None, trials=50, tol=0.05, use_acceleration_mode=False,
                                use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10,
                                flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False):
        """solve_video_dev with the forward-backward check between every batch's flow and its solve (rsdsfm_solve_video_checked_dev):
        d_masks: F - 1 device masks; d_flows (or the library's ring) hold the MASKED fields; d_bwd_flows: F - 1 buffers for the backward
        fields (None: a ring owned by the library).  Returns one dict per pair, as solve_video_dev, each with "consistent" (the pair's
        count of consistent pixels)."""
        n = len(d_frames) - 1
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 1)
        res = (FrameResult * max(n, 1))()
        cnt = (C.c_int64 * max(n, 1))()
        sd = (C.c_uint64 * n)(*[int(s) for s in seeds]) if seeds is not None else None
        p, k = _flow_params(flow_params), _flow_check_params(a1, a2)
        d = C.c_double
        self._check(self.lib.rsdsfm_solve_video_checked_dev(self._ctx, _ptr_array(d_frames), C.c_int32(len(d_frames)), C.c_int32(rows), C.c_int32(cols),
                                                            C.c_int32(channels), *_k4(K), d(gamma),
                                                            _ref(p), C.byref(prm), sd, _ptrs(d_flows), _ptr_array(d_depth_maps),
                                                            _ptrs(d_R), _ptrs(d_t), res, _ref(k), _ptr_array(d_masks),
                                                            _ptrs(d_bwd_flows), cnt), "rsdsfm_solve_video_checked_dev")
        return [dict(_frame_result_dict(r), consistent=int(cnt[i])) for i, r in enumerate(res[:n])]


# ---------------------------------------------------------------------------------------------------
# a clip's trajectory: the links between consecutive pairs, the chain of scales and poses, the clip's points (include/rsdsfm_trajectory.h)
# ---------------------------------------------------------------------------------------------------
TRAJECTORY_HEADER_PATH = _header_path("rsdsfm_trajectory.h")


class LinkParams(C.Structure):
    _fields_ = [("tol", C.c_double), ("min_links", C.c_int32), ("radix_bits", C.c_int32), ("struct_bytes", C.c_int32), ("reserved", C.c_int32)]


class LinkRecord(C.Structure):
    _fields_ = [("n", C.c_int64), ("ratio", C.c_double), ("agree", C.c_int64), ("valid", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(n=int(self.n), ratio=float(self.ratio), agree=int(self.agree), valid=bool(self.valid))


def trajectory_declared_symbols():
    """Names of every function include/rsdsfm_trajectory.h declares"""
    return _declared("rsdsfm_trajectory.h")


def link_default_params():
    """the link's defaults as a dict: tol = 0.1, min_links = 16, radix_bits = 0 (rsdsfm_link_params_init)"""
    p = _params(LinkParams, "rsdsfm_link_params_init")
    return dict(tol=p.tol, min_links=p.min_links, radix_bits=p.radix_bits)


def _link_params(tol, min_links, radix_bits):
    """(None, None, None) -> NULL (the defaults); otherwise a LinkParams with the given values over the defaults"""
    if tol is None and min_links is None and radix_bits is None:
        return None
    return _params(LinkParams, "rsdsfm_link_params_init", tol=tol, min_links=min_links, radix_bits=radix_bits)


def _records_in(records):
    rec = (LinkRecord * max(len(records), 1))()
    for i, r in enumerate(records):
        rec[i].n, rec[i].ratio, rec[i].agree, rec[i].valid = int(r["n"]), float(r["ratio"]), int(r["agree"]), int(bool(r["valid"]))
    return rec


def chain_clip(records, vs, ws, gamma):
    """the clip's scales and poses from its links and motions (rsdsfm_chain_clip; host arithmetic, no GPU).  records: the F - 2 link records
    (dicts with n, ratio, agree, valid); vs / ws: (F - 1, 3).  -> dict(scales (F - 1), A (F, 3, 3), c (F, 3), broken (F - 2) uint8):
    S_0 = 1, S_{q+1} = S_q / ratio_q (carried over a link that is not valid: broken[q] = 1); frame q's first scanline in frame 0's
    coordinates is X_0 = A_q X_q + c_q."""
    v, w = _f64(vs).reshape(-1, 3), _f64(ws).reshape(-1, 3)
    n = v.shape[0]
    if w.shape[0] != n or len(records) != max(n - 1, 0):
        raise ValueError("F - 1 motions need F - 2 link records")
    scales, A, c = np.empty(max(n, 1)), np.empty((n + 1, 3, 3)), np.empty((n + 1, 3))
    broken = np.zeros(max(n - 1, 1), dtype=np.uint8)
    rc = load_library().rsdsfm_chain_clip(_records_in(records), _p(v), _p(w), C.c_int32(n), C.c_double(gamma), _p(scales), _p(A), _p(c), _p(broken))
    if rc != OK:
        raise RsdsfmError("rsdsfm_chain_clip failed (%d): at least one pair, gamma finite and > 0" % rc)
    return dict(scales=scales[:n], A=A, c=c, broken=broken[:max(n - 1, 0)])


@_solver_methods
class _TrajectoryMixin:
    def link_pairs_dev(self, d_fields, d_depth_maps, vs, ws, ks, rows, cols, K, gamma, global_shutter=False, d_planes=None, tol=None, min_links=None,
                       radix_bits=None):
        """the links of n solved pairs on the device (rsdsfm_link_pairs_dev; tests/link_spec_numpy.py): d_fields / d_depth_maps: n device
        pointers each (the last field is not read: 0 will do), vs / ws (n, 3) and ks (n): the pairs' final motions; d_planes: n - 1
        buffers of rows x cols uint64 for the ratio planes (None: the context's workspace).  Returns the n - 1 records as dicts
        (n, ratio, agree, valid).  Waits for the one copy of the scalars."""
        n = len(d_depth_maps)
        v, w, k = _f64(vs).reshape(-1, 3), _f64(ws).reshape(-1, 3), _f64(ks).reshape(-1)
        if not (v.shape[0] == w.shape[0] == k.shape[0] == n) or len(d_fields) not in (n - 1, n):
            raise ValueError("n depth maps need n motions and n (or n - 1) fields")
        p = _link_params(tol, min_links, radix_bits)
        rec = (LinkRecord * max(n - 1, 1))()
        d = C.c_double
        self._check(self.lib.rsdsfm_link_pairs_dev(self._ctx, _ptr_array(list(d_fields) + [0] * (n - len(d_fields))), _ptr_array(d_depth_maps), _p(v), _p(w),
                                                   _p(k), C.c_int32(n), C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma),
                                                   C.c_int32(int(bool(global_shutter))), _ref(p),
                                                   _ptrs(d_planes), rec), "rsdsfm_link_pairs_dev")
        return [r.as_dict() for r in rec[:max(n - 1, 0)]]

    def link_pairs(self, fields, depth_maps, vs, ws, ks, K, gamma, global_shutter=False, tol=None, min_links=None, radix_bits=None, want_planes=False,
                   device=0):
        """host convenience around link_pairs_dev: fields (n or n - 1, rows, cols, 2) float64, depth_maps (n, rows, cols) float64 (row-major
        here; uploaded column-major, as the solve writes them) -> the n - 1 records, each with "plane" ((rows, cols) uint64) when
        want_planes"""
        maps = [_f64(m) for m in depth_maps]
        rows, cols = maps[0].shape
        with _Staging(self, device) as st:
            d_f = [st.up(_f64(f)) for f in fields]
            d_z = [st.up(m.T) for m in maps]  # column-major, as the solve writes them
            d_pl = [st.zeros((rows, cols), "int64") for _ in range(len(maps) - 1)] if want_planes else None
            st.ready()
            rec = self.link_pairs_dev(st.ptrs(d_f), st.ptrs(d_z), vs, ws, ks, rows, cols, K, gamma, global_shutter, st.ptrs(d_pl), tol, min_links, radix_bits)
            if want_planes:  # (link_pairs_dev has waited for the records)
                for r, t in zip(rec, d_pl):
                    r["plane"] = st.host(t).view(np.uint64)
        return rec
    def clip_points_dev(self, d_points_in, d_points_out, rows, cols, scales, A, c):
        """the clip's points (rsdsfm_clip_points_dev): pair q's world points (rows x cols x 3 floats, in frame q's coordinates) ->
        A_q (S_q X) + c_q, float64 rounded once to float; d_points_out[q] may be d_points_in[q]; (0, 0, 0) stays (0, 0, 0).  Enqueued on
        the context's stream."""
        n = len(d_points_in)
        s, a, cc = _f64(scales).reshape(-1), _f64(A).reshape(-1, 9), _f64(c).reshape(-1, 3)
        if len(d_points_out) != n or s.shape[0] < n or a.shape[0] < n or cc.shape[0] < n:
            raise ValueError("every pair needs an output, a scale and a pose")
        self._check(self.lib.rsdsfm_clip_points_dev(self._ctx, _ptr_array(d_points_in), _ptr_array(d_points_out), C.c_int32(n), C.c_int32(rows),
                                                    C.c_int32(cols), _p(s), _p(a), _p(cc)), "rsdsfm_clip_points_dev")

    def solve_video_linked_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_flows, d_masks=None, seeds=None, d_R=None, d_t=None,
                               d_points=None, flow_params=None, a1=None, a2=None, link_tol=None, min_links=None, radix_bits=None, trials=50, tol=0.05,
                               use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10,
                               flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False, d_fused=None, d_flags=None, fuse_tol=None):
        """solve_video_dev (solve_video_checked_dev when d_masks is passed), then the links, the chain and -- when d_points is passed (F - 1
        buffers holding each pair's world points) -- the clip's points in place (rsdsfm_solve_video_linked_dev).  d_flows is required.
        Returns dict(pairs: one dict per pair as solve_video_dev, links: the F - 2 records, scales, A, c, broken).
        d_fused (F - 1 buffers of rows x cols doubles; d_flags: as many of rows x cols bytes, optional): behind the links, the fusion of
        the pairs' depth maps (fuse_depths_dev on the call's own fields, maps, motions and records); the result then carries "fuse", the
        F - 1 fusion records.  Without d_fused the call is unchanged."""
        if d_fused is None and d_flags is not None:
            raise ValueError("d_flags needs d_fused")
        n = len(d_frames) - 1
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 1)
        res = (FrameResult * max(n, 1))()
        rec = (LinkRecord * max(n - 1, 1))()
        scales, A, c = np.empty(max(n, 1)), np.empty((max(n, 1) + 1, 3, 3)), np.empty((max(n, 1) + 1, 3))
        broken = np.zeros(max(n - 1, 1), dtype=np.uint8)
        sd = (C.c_uint64 * n)(*[int(s) for s in seeds]) if seeds is not None else None
        p, k, lp = _flow_params(flow_params), _flow_check_params(a1, a2), _link_params(link_tol, min_links, radix_bits)
        d = C.c_double
        self._check(self.lib.rsdsfm_solve_video_linked_dev(self._ctx, _ptr_array(d_frames), C.c_int32(len(d_frames)), C.c_int32(rows), C.c_int32(cols),
                                                           C.c_int32(channels), *_k4(K), d(gamma),
                                                           _ref(p), C.byref(prm), sd, _ptrs(d_flows), _ptr_array(d_depth_maps),
                                                           _ptrs(d_R), _ptrs(d_t), res, _ref(k), _ptrs(d_masks),
                                                           _ref(lp), rec, _p(scales), _p(A), _p(c), _p(broken), _ptrs(d_points)),
                    "rsdsfm_solve_video_linked_dev")
        out = dict(pairs=[_frame_result_dict(r) for r in res[:n]], links=[r.as_dict() for r in rec[:max(n - 1, 0)]], scales=scales[:n], A=A[:n + 1],
                   c=c[:n + 1], broken=broken[:max(n - 1, 0)])
        if d_fused is not None:
            out["fuse"] = self.fuse_depths_dev(d_flows, d_depth_maps, [r["v"] for r in out["pairs"]], [r["w"] for r in out["pairs"]],
                                               [r["k"] for r in out["pairs"]], rows, cols, K, gamma, out["links"], d_fused, use_global_shutter_mode,
                                               d_flags, None, fuse_tol)
        return out


# ---------------------------------------------------------------------------------------------------
# the fusion of a clip's depth maps: every pair's holes filled from what its neighbours measured there (include/rsdsfm_fuse.h)
# ---------------------------------------------------------------------------------------------------
FUSE_HEADER_PATH = _header_path("rsdsfm_fuse.h")
FUSE_OWN, FUSE_PREV, FUSE_NEXT, FUSE_PREV_AGREES, FUSE_NEXT_AGREES = 1, 2, 4, 8, 16


class FuseParams(C.Structure):
    _fields_ = [("tol", C.c_double), ("struct_bytes", C.c_int32), ("reserved", C.c_int32)]


class FuseRecord(C.Structure):
    _fields_ = [("own", C.c_int64), ("filled_prev", C.c_int64), ("filled_next", C.c_int64), ("confirmed", C.c_int64), ("contradicted", C.c_int64),
                ("left", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def fuse_declared_symbols():
    """Names of every function include/rsdsfm_fuse.h declares"""
    return _declared("rsdsfm_fuse.h")


def fuse_default_params():
    """the fusion's defaults as a dict: tol = 0.1 (rsdsfm_fuse_params_init)"""
    return dict(tol=_params(FuseParams, "rsdsfm_fuse_params_init").tol)


def _fuse_records_in(records):
    """link records as the fusion reads them: ratio and valid (n and agree are carried along where present)"""
    rec = (LinkRecord * max(len(records), 1))()
    for i, r in enumerate(records):
        rec[i].n, rec[i].ratio, rec[i].agree, rec[i].valid = int(r.get("n", 0)), float(r["ratio"]), int(r.get("agree", 0)), int(bool(r["valid"]))
    return rec


@_solver_methods
class _FuseMixin:
    def fuse_depths_dev(self, d_fields, d_depth_maps, vs, ws, ks, rows, cols, K, gamma, records, d_fused, global_shutter=False, d_flags=None, d_planes=None,
                        tol=None, want_records=True):
        """the fused depth maps of n solved pairs on the device (rsdsfm_fuse_depths_dev; tests/fuse_spec_numpy.py): d_fields / d_depth_maps
        / vs / ws / ks as link_pairs_dev's, records: its n - 1 link records (dicts); d_fused: n buffers of rows x cols doubles
        (column-major, none of them an input); d_flags: n buffers of rows x cols bytes (None: no flags); d_planes: n - 1 buffers of
        rows x cols uint64 for the splat planes (None: the context's workspace).  Returns the n records as dicts (own, filled_prev,
        filled_next, confirmed, contradicted, left) and waits for their one copy; want_records=False only enqueues and returns None."""
        n = len(d_depth_maps)
        v, w, k = _f64(vs).reshape(-1, 3), _f64(ws).reshape(-1, 3), _f64(ks).reshape(-1)
        if not (v.shape[0] == w.shape[0] == k.shape[0] == n) or len(d_fields) not in (n - 1, n) or len(records) != max(n - 1, 0) or len(d_fused) != n:
            raise ValueError("n depth maps need n motions, n (or n - 1) fields, n - 1 link records and n outputs")
        p = _params(FuseParams, "rsdsfm_fuse_params_init", self.lib, tol=tol) if tol is not None else None
        rec = (FuseRecord * max(n, 1))() if want_records else None
        d = C.c_double
        self._check(self.lib.rsdsfm_fuse_depths_dev(self._ctx, _ptr_array(list(d_fields) + [0] * (n - len(d_fields))), _ptr_array(d_depth_maps), _p(v), _p(w),
                                                    _p(k), C.c_int32(n), C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma),
                                                    C.c_int32(int(bool(global_shutter))), _fuse_records_in(records) if n > 1 else None,
                                                    _ref(p), _ptr_array(d_fused),
                                                    _ptrs(d_flags),
                                                    _ptrs(d_planes), rec), "rsdsfm_fuse_depths_dev")
        return [r.as_dict() for r in rec[:n]] if want_records else None

    def fuse_depths(self, fields, depth_maps, vs, ws, ks, records, K, gamma, global_shutter=False, tol=None, want_flags=False, want_planes=False, device=0):
        """host convenience around fuse_depths_dev: fields (n or n - 1, rows, cols, 2) float64, depth_maps (n, rows, cols) float64
        (row-major here; uploaded column-major, as the solve writes them), records: the n - 1 link records -> dict(fused: n (rows, cols)
        float64, records: n dicts, flags: n (rows, cols) uint8 when want_flags, planes: n - 1 (rows, cols) uint64 when want_planes)"""
        maps = [_f64(m) for m in depth_maps]
        n = len(maps)
        rows, cols = maps[0].shape
        with _Staging(self, device) as st:
            d_f = [st.up(_f64(f)) for f in fields]
            d_z = [st.up(m.T) for m in maps]  # column-major, as the solve writes them
            d_out = [st.empty((cols, rows), "float64") for _ in range(n)]
            d_fl = [st.empty((rows, cols)) for _ in range(n)] if want_flags else None
            d_pl = [st.empty((rows, cols), "int64") for _ in range(n - 1)] if want_planes else None
            st.ready()
            rec = self.fuse_depths_dev(st.ptrs(d_f), st.ptrs(d_z), vs, ws, ks, rows, cols, K, gamma, records, st.ptrs(d_out), global_shutter, st.ptrs(d_fl), st.ptrs(d_pl), tol)
            out = dict(fused=[st.host(t).T.copy() for t in d_out], records=rec)  # (fuse_depths_dev has waited for the records)
            if want_flags:
                out["flags"] = [st.host(t) for t in d_fl]
            if want_planes:
                out["planes"] = [st.host(t).view(np.uint64) for t in d_pl]
        return out


# ---------------------------------------------------------------------------------------------------
# the stabiliser: a smoothed camera path and every frame rendered from its virtual camera on it (include/rsdsfm_stabilize.h)
# ---------------------------------------------------------------------------------------------------
STABILIZE_HEADER_PATH = _header_path("rsdsfm_stabilize.h")


class StabilizeParams(C.Structure):
    _fields_ = [("sigma", C.c_double), ("radius", C.c_int32), ("translation", C.c_int32), ("struct_bytes", C.c_int32), ("last_frame", C.c_int32)]
    reserved = property(lambda self: self.last_frame)  # the word's name before it meant anything


def stabilize_declared_symbols():
    """Names of every function include/rsdsfm_stabilize.h declares"""
    return _declared("rsdsfm_stabilize.h")


def stabilize_default_params():
    """the stabiliser's defaults as a dict: sigma = 4.0 frames, radius = 0 (ceil(3 sigma)), translation = 1 (rsdsfm_stabilize_params_init)"""
    p = _params(StabilizeParams, "rsdsfm_stabilize_params_init")
    return dict(sigma=p.sigma, radius=p.radius, translation=p.translation)


def _stabilize_params(sigma, radius, translation, last_frame=False):
    """a StabilizeParams with the given values over the defaults (sigma None: the default)"""
    return _params(StabilizeParams, "rsdsfm_stabilize_params_init", sigma=sigma, radius=radius, translation=bool(translation), last_frame=last_frame)


def smooth_path(A, c, sigma=None, radius=0, translation=True):
    """the smoothed camera path (rsdsfm_smooth_path; host arithmetic, no GPU; tests/stabilize_spec_numpy.py): A (F, 3, 3), c (F, 3) from
    chain_clip -> (A_s, c_s), one tangent-space mean step about every frame's pose with Gaussian weights of width sigma frames (None: the
    default, 4) over |j| <= radius (0: ceil(3 sigma)); translation=False smooths the rotation only (c_s = c)."""
    a, cc = _f64(A).reshape(-1, 9), _f64(c).reshape(-1, 3)
    n = a.shape[0]
    if cc.shape[0] != n:
        raise ValueError("every frame needs a rotation and a centre")
    p = _stabilize_params(sigma, radius, translation)
    A_s, c_s = np.empty((max(n, 1), 9)), np.empty((max(n, 1), 3))
    rc = load_library().rsdsfm_smooth_path(_p(a), _p(cc), C.c_int32(n), C.byref(p), _p(A_s), _p(c_s))
    if rc != OK:
        raise RsdsfmError("rsdsfm_smooth_path failed (%d): at least one frame, sigma finite and > 0, radius in [0, 1024]" % rc)
    return A_s[:n].reshape(n, 3, 3), c_s[:n]


def virtual_poses(A, c, A_s, c_s, scales, translation=True, last_frame=False):
    """every pair's virtual pose (rsdsfm_virtual_poses; host): M_q = A_s_q^T A_q, m_q = A_s_q^T (c_q - c_s_q) / S_q for q < F - 1 -- a point X in
    frame q's first-scanline coordinates is M_q X + m_q in the virtual camera's.  translation=False: m = 0 and scales (may be None) is not read.
    -> (M (F - 1, 3, 3), m (F - 1, 3)).  last_frame=True: the clip's last frame has a pose too (its scale is scales[F - 1], the last pair's
    carried over): F entries."""
    a, cc, a_s, cc_s = _f64(A).reshape(-1, 9), _f64(c).reshape(-1, 3), _f64(A_s).reshape(-1, 9), _f64(c_s).reshape(-1, 3)
    n = a.shape[0] - (0 if last_frame else 1)
    if not (cc.shape[0] == a_s.shape[0] == cc_s.shape[0] == a.shape[0]):
        raise ValueError("the path and the smoothed path need the same number of frames")
    sc = None
    if translation:
        sc = _f64(scales).reshape(-1)
        if sc.shape[0] < n:
            raise ValueError("every pair needs a scale")
    M, m = np.empty((max(n, 1), 9)), np.empty((max(n, 1), 3))
    rc = load_library().rsdsfm_virtual_poses(_p(a), _p(cc), _p(a_s), _p(cc_s), _p(sc), C.c_int32(n), C.c_int32(int(bool(translation))), _p(M), _p(m))
    if rc != OK:
        raise RsdsfmError("rsdsfm_virtual_poses failed (%d): at least one pair, every scale finite and positive" % rc)
    return M[:n].reshape(n, 3, 3), m[:n]


def stabilize_launches(rows, cols, count=False):
    """kernel launches of one stabilize_frame_dev call at this size: rectify_dense_launches, plus one with a valid count
    (rsdsfm_stabilize_launches; host only)"""
    return _launches("rsdsfm_stabilize_launches", "rows and cols must be in [2, 16384]", rows, cols, int(bool(count)))


@_solver_methods
class _StabilizeMixin:
    def stabilize_frame_dev(self, d_img, channels, d_depth_map, d_R, d_t, K, rows, cols, M, m, d_out, d_mask=None, d_filled=None, d_disp=None, d_valid=None,
                            mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """rectify_dense_frame_dev seen from the virtual camera (M (3, 3), m (3): host arrays; rsdsfm_stabilize_frame_dev): one more rigid
        transform inside the dense rectifier's stage B.  d_valid: a device int64 that receives the number of mask pixels that are 1.
        Enqueued on the context's stream."""
        Mh = None if M is None else _f64(M).reshape(9)
        mh = None if m is None else _f64(m).reshape(3)
        self._check(self.lib.rsdsfm_stabilize_frame_dev(self._ctx, _dp(d_img), C.c_int32(channels), _dp(d_depth_map), _dp(d_R), _dp(d_t), *_k4(K), C.c_int32(rows),
                                                        C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), _p(Mh), _p(mh),
                                                        _dp(d_out), _np0(d_mask), _np0(d_filled), _np0(d_disp), _np0(d_valid)), "rsdsfm_stabilize_frame_dev")

    def stabilize(self, image, depth_map, R, t, K, M, m, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, device=0):
        """host convenience around stabilize_frame_dev: image (rows, cols) or (rows, cols, 3) uint8, depth_map (rows, cols) (0 where unknown),
        R (rows, 3, 3) / (rows, 9), t (rows, 3), M (3, 3), m (3).  Returns (stabilised image, mask, valid)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = img.shape[:2]
        with _Staging(self, device) as st:
            d_img, d_dm, d_R, d_t = st.up_frame(img, depth_map, R, t)
            d_out, d_mask, d_valid = st.empty_like(d_img), st.empty((rows, cols)), st.zeros(1, "int64")
            st.ready()
            self.stabilize_frame_dev(d_img.data_ptr(), 1 if img.ndim == 2 else img.shape[2], d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, M, m,
                                     d_out.data_ptr(), d_mask.data_ptr(), d_valid=d_valid.data_ptr(), mode=mode, q5_mode=q5_mode, iterations=iterations)
            out, mask, valid = st.down(d_out, d_mask, d_valid)
            return out, mask, int(valid[0])
    def stabilize_video_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_flows, d_R, d_t, d_stab, d_masks_out=None, d_fused=None,
                            want_valid=True, sigma=None, radius=0, translation=True, fuse_tol=None, d_masks=None, seeds=None, flow_params=None, a1=None,
                            a2=None, link_tol=None, min_links=None, radix_bits=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, trials=50, tol=0.05,
                            use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10,
                            flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False, last_frame=False):
        """the stabilised clip in ONE call (rsdsfm_stabilize_video_dev): solve_video_linked_dev (d_flows, d_depth_maps, d_R, d_t all required), the
        fusion of the maps when d_fused (F - 1 buffers) is passed, smooth_path, virtual_poses and stabilize_frame_dev of frames 0 .. F - 2 into
        d_stab (and d_masks_out).  Returns solve_video_linked_dev's dict plus A_s, c_s, M, m and, with want_valid, valid (F - 1 counts; the
        call then waits for the frames).  last_frame=True also renders frame F - 1, from the last pair's map moved onto it (last_frame_dev):
        d_depth_maps, d_R, d_t, d_stab, d_masks_out and d_fused then need F entries, and scales, M, m and valid have F."""
        return self._stabilize_video("rsdsfm_stabilize_video_dev", (), **_stabilize_video_args())

    def _stabilize_video(self, entry, tail, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_flows, d_R, d_t, d_stab, d_masks_out, d_fused, want_valid,
                         sigma, radius, translation, fuse_tol, d_masks, seeds, flow_params, a1, a2, link_tol, min_links, radix_bits, mode, q5_mode, iterations,
                         trials, tol, use_acceleration_mode, use_refinement, depth_mode, k_sign_mode, flow_threshold, flow_index_mode, use_global_shutter_mode,
                         last_frame=False):
        """stabilize_video_dev's marshalling, for it and for the entry points that take its arguments and then a `tail` of their own
        (stabilize_video_filled_dev)"""
        n = len(d_frames) - 1
        nr = n + (1 if last_frame else 0)  # rendered frames
        for what, lst, need in (("d_depth_maps", d_depth_maps, nr), ("d_R", d_R, nr), ("d_t", d_t, nr), ("d_stab", d_stab, nr), ("d_masks_out", d_masks_out, nr),
                                ("d_fused", d_fused, nr), ("d_flows", d_flows, n), ("d_masks", d_masks, n), ("seeds", seeds, n)):
            _need_entries(what, lst, need)
        prm = FrameParams(int(trials), int(use_acceleration_mode), int(use_refinement), int(depth_mode), int(k_sign_mode),
                          int(flow_index_mode), int(use_global_shutter_mode), 0, float(tol), float(flow_threshold), 1)
        res = (FrameResult * max(n, 1))()
        rec = (LinkRecord * max(n - 1, 1))()
        nn = max(n, 1)
        scales, A, c = np.empty(nn + 1), np.empty((nn + 1, 3, 3)), np.empty((nn + 1, 3))
        A_s, c_s, M, m = np.empty((nn + 1, 3, 3)), np.empty((nn + 1, 3)), np.empty((nn + 1, 3, 3)), np.empty((nn + 1, 3))
        valid = _counts(want_valid, nn + 1)
        broken = np.zeros(max(n - 1, 1), dtype=np.uint8)
        sd = (C.c_uint64 * n)(*[int(s) for s in seeds]) if seeds is not None else None
        p, k, lp = _flow_params(flow_params), _flow_check_params(a1, a2), _link_params(link_tol, min_links, radix_bits)
        sp = _stabilize_params(sigma, radius, translation, last_frame)
        fp = _params(FuseParams, "rsdsfm_fuse_params_init", self.lib, tol=fuse_tol) if fuse_tol is not None else None
        d = C.c_double
        self._check(getattr(self.lib, entry)(self._ctx, _ptr_array(d_frames), C.c_int32(len(d_frames)), C.c_int32(rows), C.c_int32(cols),
                                             C.c_int32(channels), *_k4(K), d(gamma), _ref(p), C.byref(prm), sd, _ptrs(d_flows),
                                             _ptrs(d_depth_maps), _ptrs(d_R), _ptrs(d_t), res, _ref(k), _ptrs(d_masks), _ref(lp), rec, _p(scales), _p(A), _p(c),
                                             _p(broken), _ref(fp), _ptrs(d_fused), C.byref(sp), int(mode), int(q5_mode), C.c_int32(iterations), _p(A_s),
                                             _p(c_s), _p(M), _p(m), _ptrs(d_stab), _ptrs(d_masks_out), _p(valid), *tail), entry)
        out = dict(pairs=[_frame_result_dict(r) for r in res[:n]], links=[r.as_dict() for r in rec[:max(n - 1, 0)]], scales=scales[:nr], A=A[:n + 1], c=c[:n + 1],
                   broken=broken[:max(n - 1, 0)], A_s=A_s[:n + 1], c_s=c_s[:n + 1], M=M[:nr], m=m[:nr])
        out.update(_wanted(nr, valid=valid))
        return out


def _stabilize_video_args():
    """the arguments of the calling stabilize_video_* wrapper that _stabilize_video itself takes, selected by ITS parameter names (behind self, entry
    and tail): a local or a keyword of the wrapper's own cannot leak into the call"""
    code = Solver._stabilize_video.__code__
    scope = sys._getframe(1).f_locals
    return {name: scope[name] for name in code.co_varnames[3:code.co_argcount]}


# ---------------------------------------------------------------------------------------------------
# the stabiliser's border fill: the band its own frame leaves empty, from the neighbouring frames (include/rsdsfm_stabilize_fill.h)
# ---------------------------------------------------------------------------------------------------
STABILIZE_FILL_HEADER_PATH = _header_path("rsdsfm_stabilize_fill.h")


class StabilizeFillParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("struct_bytes", C.c_int32), ("occlusion", C.c_int32), ("occlusion_tol_q16", C.c_int32)]
    reserved = property(lambda self: [self.occlusion, self.occlusion_tol_q16])  # the two words' name before they meant anything


def stabilize_fill_declared_symbols():
    """Names of every function include/rsdsfm_stabilize_fill.h declares"""
    return _declared("rsdsfm_stabilize_fill.h")


def stabilize_fill_default_params():
    """the border fill's defaults as a dict: radius = 2 neighbours on each side (rsdsfm_stabilize_fill_params_init)"""
    return dict(radius=_params(StabilizeFillParams, "rsdsfm_stabilize_fill_params_init").radius)


def _occlusion_tol_q16(tol):
    """a tolerance as a fraction of the depth -> units of 1 / 65536; outside (0, 1] a value the library refuses"""
    q = int(round(float(tol) * 65536.0))
    return q if 1 <= q <= 65536 else -1


def _stabilize_fill_params(radius, occlusion=False, occlusion_tol=None):
    """a StabilizeFillParams with the given radius (0: the default); occlusion: the neighbour candidates go through the occlusion test
    (stabilize_visible_frame_dev), occlusion_tol its tolerance as a fraction of the depth in (0, 1] (None: the default, about 0.05)"""
    return _params(StabilizeFillParams, "rsdsfm_stabilize_fill_params_init", radius=radius or None, occlusion=occlusion,  # (occlusion: anything but 0 and 1 is refused by the library)
                   occlusion_tol_q16=0 if occlusion_tol is None else _occlusion_tol_q16(occlusion_tol))


def neighbour_poses(A, c, A_s, c_s, scales, q, radius=2):
    """the candidates of frame q and their poses (rsdsfm_neighbour_poses; host arithmetic, no GPU; tests/stabilize_fill_spec_numpy.py): the
    frames n = q - 1, q + 1, ..., q - radius, q + radius that have a pair, their source ids (2 |j| for a previous, 2 |j| + 1 for a next frame)
    and M = A_s_q^T A_n, m = A_s_q^T (c_n - c_s_q) / S_n -- a point X in frame n's first-scanline coordinates is M X + m in virtual camera q's.
    scales: one per pair (their number is the number of pairs), always read.  -> (frames (k,), source_ids (k,), M (k, 3, 3), m (k, 3)),
    k <= 2 radius"""
    a, cc, a_s, cc_s, sc = _f64(A).reshape(-1, 9), _f64(c).reshape(-1, 3), _f64(A_s).reshape(-1, 9), _f64(c_s).reshape(-1, 3), _f64(scales).reshape(-1)
    n = sc.shape[0]
    if not (a.shape[0] == cc.shape[0] and a_s.shape[0] == cc_s.shape[0] and a.shape[0] >= n and a_s.shape[0] >= n):
        raise ValueError("the path and the smoothed path need an entry for every pair")
    room = 2 * max(int(radius), 1)
    frames, ids = np.zeros(room, dtype=np.int32), np.zeros(room, dtype=np.int32)
    M, m = np.empty((room, 9)), np.empty((room, 3))
    k = C.c_int32(0)
    rc = load_library().rsdsfm_neighbour_poses(_p(a), _p(cc), _p(a_s), _p(cc_s), _p(sc), C.c_int32(n), C.c_int32(q), C.c_int32(radius), _p(frames), _p(ids), _p(M),
                                               _p(m), C.byref(k))
    if rc != OK:
        raise RsdsfmError("rsdsfm_neighbour_poses failed (%d): q in [0, pairs - 1], radius in [1, 16], every listed neighbour's scale finite and positive" % rc)
    return frames[:k.value], ids[:k.value], M[:k.value].reshape(-1, 3, 3), m[:k.value]


def stabilize_fill_launches(rows, cols):
    """kernel launches of one stabilize_fill_frame_dev call at this size: rectify_dense_launches -- the fill-warp kernel counts by itself
    (rsdsfm_stabilize_fill_launches; host only)"""
    return _launches("rsdsfm_stabilize_fill_launches", "rows and cols must be in [2, 16384]", rows, cols)


@_solver_methods
class _StabilizeFillMixin:
    def stabilize_fill_frame_dev(self, d_img_n, channels, d_depth_map_n, d_R_n, d_t_n, K, rows, cols, M, m, source_id, d_image, d_mask, d_source=None,
                                 d_filled=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """one candidate of the border fill (rsdsfm_stabilize_fill_frame_dev): the neighbour's frame, depth map and pose table seen from the
        virtual camera (M (3, 3), m (3): host arrays, neighbour_poses') and taken where d_mask is 0 and the candidate is valid: d_image gets the
        pixel, d_mask 1, d_source (a device plane of bytes) source_id.  d_filled: a device int64 that receives the number of pixels taken.
        Enqueued on the context's stream."""
        Mh = None if M is None else _f64(M).reshape(9)
        mh = None if m is None else _f64(m).reshape(3)
        self._check(self.lib.rsdsfm_stabilize_fill_frame_dev(self._ctx, _dp(d_img_n), C.c_int32(channels), _dp(d_depth_map_n), _dp(d_R_n), _dp(d_t_n), *_k4(K), C.c_int32(rows),
                                                             C.c_int32(cols), int(mode), int(q5_mode),
                                                             C.c_int32(iterations), _p(Mh), _p(mh), C.c_int32(source_id), _dp(d_image), _dp(d_mask), _np0(d_source),
                                                             _np0(d_filled)), "rsdsfm_stabilize_fill_frame_dev")

    def stabilize_filled(self, images, depth_maps, Rs, ts, K, A, c, A_s, c_s, scales, q, M, m, radius=2, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0,
                         device=0):
        """host convenience: frame q of a clip rendered from its virtual camera (M, m: virtual_poses' entry q) and its empty band filled from
        its neighbours (neighbour_poses, then one stabilize_fill_frame_dev each).  images / depth_maps / Rs / ts are indexed by frame and entry
        q and its candidates' are read: images (rows, cols[, 3]) uint8, depth maps (rows, cols) (0 where unknown), R (rows, 3, 3) / (rows, 9),
        t (rows, 3).  Returns (image, mask, source (rows, cols) uint8, counts (2 + 2 radius,) int64: [none, own, -1, +1, -2, +2, ...])."""
        frames, ids, nM, nm = neighbour_poses(A, c, A_s, c_s, scales, q, radius)
        rows, cols = np.asarray(images[q]).shape[:2]
        with _Staging(self, device) as st:
            frame = lambda n: st.up_frame(images[n], depth_maps[n], Rs[n], ts[n])
            d_img, d_dm, d_R, d_t = frame(q)
            channels = 1 if d_img.ndim == 2 else d_img.shape[2]
            d_out, d_mask, d_cnt = st.empty_like(d_img), st.empty((rows, cols)), st.zeros(2 + 2 * radius, "int64")
            cand = [frame(int(n)) for n in frames]
            st.ready()
            self.stabilize_frame_dev(d_img.data_ptr(), channels, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, M, m, d_out.data_ptr(),
                                     d_mask.data_ptr(), d_valid=d_cnt[1:].data_ptr(), mode=mode, q5_mode=q5_mode, iterations=iterations)
            st.wait()  # two phases: the own frame's mask is complete before torch copies it, and the copy before the fill passes write it
            d_source = d_mask.clone()
            st.ready()
            for (n_img, n_dm, n_R, n_t), sid, Mn, mn in zip(cand, ids, nM, nm):
                self.stabilize_fill_frame_dev(n_img.data_ptr(), channels, n_dm.data_ptr(), n_R.data_ptr(), n_t.data_ptr(), K, rows, cols, Mn, mn, int(sid),
                                              d_out.data_ptr(), d_mask.data_ptr(), d_source.data_ptr(), d_cnt[int(sid):].data_ptr(), mode=mode, q5_mode=q5_mode,
                                              iterations=iterations)
            out, mask, source, counts = st.down(d_out, d_mask, d_source, d_cnt)
            counts[0] = rows * cols - int(counts[1:].sum())
            return out, mask, source, counts
    def stabilize_video_filled_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_flows, d_R, d_t, d_stab, d_masks_out, d_sources=None,
                                   fill_radius=0, want_counts=True, d_fused=None, want_valid=True, sigma=None, radius=0, translation=True, fuse_tol=None,
                                   d_masks=None, seeds=None, flow_params=None, a1=None, a2=None, link_tol=None, min_links=None, radix_bits=None,
                                   mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, trials=50, tol=0.05, use_acceleration_mode=False, use_refinement=True,
                                   depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK,
                                   use_global_shutter_mode=False, last_frame=False, occlusion=False, occlusion_tol=None, occlusion_search=False):
        """the stabilised clip with its borders filled in ONE call (rsdsfm_stabilize_video_filled_dev): stabilize_video_dev with these arguments
        (d_masks_out required), then for every frame its mask copied to d_sources (F - 1 device planes of bytes, optional), neighbour_poses with
        fill_radius neighbours on each side (0: the default, 2) and one stabilize_fill_frame_dev per candidate -- on the fused maps when d_fused
        is passed.  Returns stabilize_video_dev's dict plus, with want_counts, counts ((F - 1, 2 + 2 fill_radius) int64: [none, own, -1, +1,
        ...] per frame; the call then waits for the passes).
        last_frame=True (see stabilize_video_dev): the clip's last frame too; every per-frame list and array then has F entries.
        occlusion=True: the neighbour candidates go through the occlusion test (stabilize_visible_frame_dev; occlusion_tol: its tolerance as a
        fraction of the depth, None: the default) -- a rejected pixel shows up under a later offset or under none.
        occlusion_search=True (needs occlusion): set_occlusion_search(1) for this call -- a rejected pixel whose visible pre-image is found is
        recovered (stabilize_search_frame_dev) and counts under its offset; the knob is put back afterwards."""
        n = len(d_frames) - 1 + (1 if last_frame else 0)  # rendered frames
        _need_all(n, d_sources=d_sources)
        fp = _stabilize_fill_params(fill_radius, occlusion, occlusion_tol)
        counts = _counts(want_counts, n, 2 + 2 * fp.radius)
        args = _stabilize_video_args()
        with _occlusion_search_for(self, occlusion_search, occlusion):
            out = self._stabilize_video("rsdsfm_stabilize_video_filled_dev", (C.byref(fp), _ptrs(d_sources), _p(counts)), **args)
        out.update(_wanted(n, counts=counts))
        return out


# ---------------------------------------------------------------------------------------------------
# the stabiliser's crop and zoom: one window for the clip, every frame rendered through it (include/rsdsfm_stabilize_crop.h)
# ---------------------------------------------------------------------------------------------------
STABILIZE_CROP_HEADER_PATH = _header_path("rsdsfm_stabilize_crop.h")


class StabilizeCropParams(C.Structure):
    _fields_ = [("max_empty", C.c_int64), ("margin", C.c_int32), ("struct_bytes", C.c_int32), ("reserved", C.c_int32 * 4)]


def stabilize_crop_declared_symbols():
    """Names of every function include/rsdsfm_stabilize_crop.h declares"""
    return _declared("rsdsfm_stabilize_crop.h")


def stabilize_crop_default_params():
    """the crop's defaults as a dict: max_empty = 0, margin = 1 (rsdsfm_stabilize_crop_params_init)"""
    p = _params(StabilizeCropParams, "rsdsfm_stabilize_crop_params_init")
    return dict(max_empty=p.max_empty, margin=p.margin)


def _stabilize_crop_params(max_empty, margin):
    """a StabilizeCropParams with the given values over the defaults (margin None: the default)"""
    return _params(StabilizeCropParams, "rsdsfm_stabilize_crop_params_init", max_empty=max_empty, margin=margin)


def crop_window_launches(rows, cols):
    """kernel launches of one crop_window_dev call: 3 (rsdsfm_crop_window_launches; host only)"""
    return _launches("rsdsfm_crop_window_launches", "rows and cols must be in [2, 16384]", rows, cols)


def stabilize_window_launches(rows, cols):
    """kernel launches of one stabilize_window_frame_dev call at this size: stabilize_fill_launches (rsdsfm_stabilize_window_launches; host
    only)"""
    return _launches("rsdsfm_stabilize_window_launches", "rows and cols must be in [2, 16384]", rows, cols)


def _window4(window):
    return None if window is None else (C.c_int32 * 4)(*[int(x) for x in window])


@_solver_methods
class _StabilizeCropMixin:
    def crop_window_dev(self, d_masks, rows, cols, max_empty=0, margin=None):
        """the clip's window (rsdsfm_crop_window_dev; tests/stabilize_crop_spec_numpy.py): d_masks, a list of device planes of rows x cols bytes
        (0 = empty) -> (r0, c0, h, w): the largest rectangle of the frame's aspect ratio whose surroundings within `margin` pixels (None: the
        default, 1) hold at most max_empty pixels empty in any plane, nearest the centre; (0, 0, 0, 0) when nothing fits.  Waits for the result."""
        p = _stabilize_crop_params(max_empty, margin)
        w = (C.c_int32 * 4)()
        self._check(self.lib.rsdsfm_crop_window_dev(self._ctx, _ptr_array(d_masks), C.c_int32(len(d_masks)), C.c_int32(rows), C.c_int32(cols), C.byref(p), w),
                    "rsdsfm_crop_window_dev")
        return tuple(int(x) for x in w)

    def crop_window(self, masks, max_empty=0, margin=None, device=0):
        """host convenience around crop_window_dev: masks (planes, rows, cols) or a list of (rows, cols) uint8 arrays"""
        m = np.ascontiguousarray(masks, dtype=np.uint8)
        if m.ndim == 2:
            m = m[None]
        with _Staging(self, device) as st:
            planes = [st.up(x) for x in m]
            st.ready()
            return self.crop_window_dev(st.ptrs(planes), m.shape[1], m.shape[2], max_empty, margin)
    def stabilize_window_frame_dev(self, d_img_n, channels, d_depth_map_n, d_R_n, d_t_n, K, rows, cols, M, m, source_id, window, d_image, d_mask, d_source=None,
                                   d_filled=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """one frame through a window (rsdsfm_stabilize_window_frame_dev): stabilize_fill_frame_dev with output pixel g mapped into
        window = (r0, c0, h, w) before stage C's fixed point, so that the full-size output shows the window, zoomed.  source_id 1 .. 255 (1: the
        own frame, onto a zeroed mask).  Enqueued on the context's stream."""
        Mh = None if M is None else _f64(M).reshape(9)
        mh = None if m is None else _f64(m).reshape(3)
        self._check(self.lib.rsdsfm_stabilize_window_frame_dev(self._ctx, _dp(d_img_n), C.c_int32(channels), _dp(d_depth_map_n), _dp(d_R_n), _dp(d_t_n), *_k4(K), C.c_int32(rows),
                                                               C.c_int32(cols), int(mode), int(q5_mode),
                                                               C.c_int32(iterations), _p(Mh), _p(mh), C.c_int32(source_id), _window4(window), _dp(d_image),
                                                               _dp(d_mask), _np0(d_source), _np0(d_filled)), "rsdsfm_stabilize_window_frame_dev")

    def stabilize_cropped(self, images, depth_maps, Rs, ts, K, A, c, A_s, c_s, scales, q, M, m, window, radius=2, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT,
                          iterations=0, device=0):
        """host convenience: frame q of a clip rendered through `window` from its virtual camera (M, m: virtual_poses' entry q) onto zeroed
        planes, then its neighbours (neighbour_poses with `radius`; 0: none), one stabilize_window_frame_dev each.  Arguments as
        stabilize_filled.  Returns (image, mask, source (rows, cols) uint8, counts (2 + 2 radius,) int64: [none, own, -1, +1, -2, +2, ...])."""
        frames, ids, nM, nm = neighbour_poses(A, c, A_s, c_s, scales, q, radius) if radius else ((), (), (), ())
        rows, cols = np.asarray(images[q]).shape[:2]
        with _Staging(self, device) as st:
            frame = lambda n: st.up_frame(images[n], depth_maps[n], Rs[n], ts[n])
            own = frame(q)
            channels = 1 if own[0].ndim == 2 else own[0].shape[2]
            d_out = st.zeros_like(own[0])
            d_mask, d_source = (st.zeros((rows, cols)) for _ in range(2))
            d_cnt = st.zeros(2 + 2 * radius, "int64")
            cand = [frame(int(n)) for n in frames]
            st.ready()
            for (n_img, n_dm, n_R, n_t), sid, Mn, mn in zip([own] + cand, [1] + list(ids), [M] + list(nM), [m] + list(nm)):
                self.stabilize_window_frame_dev(n_img.data_ptr(), channels, n_dm.data_ptr(), n_R.data_ptr(), n_t.data_ptr(), K, rows, cols, Mn, mn, int(sid), window,
                                                d_out.data_ptr(), d_mask.data_ptr(), d_source.data_ptr(), d_cnt[int(sid):].data_ptr(), mode=mode, q5_mode=q5_mode,
                                                iterations=iterations)
            out, mask, source, counts = st.down(d_out, d_mask, d_source, d_cnt)
            counts[0] = rows * cols - int(counts[1:].sum())
            return out, mask, source, counts
    def stabilize_video_cropped_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_flows, d_R, d_t, d_stab, d_masks_out, d_crop, d_crop_masks,
                                    d_crop_sources=None, window_in=None, max_empty=0, margin=None, want_crop_counts=True, d_sources=None, fill_radius=2,
                                    want_counts=True, d_fused=None, want_valid=True, sigma=None, radius=0, translation=True, fuse_tol=None, d_masks=None,
                                    seeds=None, flow_params=None, a1=None, a2=None, link_tol=None, min_links=None, radix_bits=None, mode=BACKPROJECT_RS,
                                    q5_mode=Q5_COMPAT, iterations=0, trials=50, tol=0.05, use_acceleration_mode=False, use_refinement=True,
                                    depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK,
                                    use_global_shutter_mode=False, last_frame=False, occlusion=False, occlusion_tol=None, occlusion_search=False):
        """the stabilised clip, cropped and zoomed, in ONE call (rsdsfm_stabilize_video_cropped_dev): stabilize_video_filled_dev with these
        arguments (fill_radius 0 .. 16 HERE: 0 means no fill, the inner call is then stabilize_video_dev), the window of its output masks
        (crop_window_dev with max_empty / margin; window_in = (r0, c0, h, w) skips the search) and, for every frame, the own frame and its
        neighbours through that window (stabilize_window_frame_dev) into d_crop, d_crop_masks and d_crop_sources (F - 1 device buffers each,
        zeroed first).  Returns the inner call's dict plus window and, with want_crop_counts, crop_counts ((F - 1, 2 + 2 fill_radius) int64:
        [none, own, -1, +1, ...] per frame; the call then waits for the passes).
        last_frame=True (see stabilize_video_dev): the clip's last frame too; every per-frame list and array then has F entries.
        occlusion=True: the neighbour candidates go through the occlusion test (stabilize_visible_frame_dev; occlusion_tol: its tolerance as a
        fraction of the depth, None: the default) -- a rejected pixel shows up under a later offset or under none.
        occlusion_search=True (needs occlusion): set_occlusion_search(1) for this call -- a rejected pixel whose visible pre-image is found is
        recovered (stabilize_search_frame_dev) and counts under its offset; the knob is put back afterwards."""
        n = len(d_frames) - 1 + (1 if last_frame else 0)  # rendered frames
        _need_all(n, d_sources=d_sources, d_crop=d_crop, d_crop_masks=d_crop_masks, d_crop_sources=d_crop_sources)
        fp = _stabilize_fill_params(fill_radius, occlusion, occlusion_tol)
        fp.radius = int(fill_radius)  # 0 stays 0 here
        cp = _stabilize_crop_params(max_empty, margin)
        width = 2 + 2 * int(fill_radius)
        counts = _counts(want_counts, n, width)
        crop_counts = _counts(want_crop_counts, n, width)
        window = (C.c_int32 * 4)()
        args = _stabilize_video_args()
        with _occlusion_search_for(self, occlusion_search, occlusion):
            out = self._stabilize_video("rsdsfm_stabilize_video_cropped_dev",
                                        (C.byref(fp), _ptrs(d_sources), _p(counts), C.byref(cp), _window4(window_in), _ptrs(d_crop), _ptrs(d_crop_masks), _ptrs(d_crop_sources),
                                         window, _p(crop_counts)), **args)
        out["window"] = tuple(int(x) for x in window)
        out.update(_wanted(n, counts=counts, crop_counts=crop_counts))
        return out


# ---------------------------------------------------------------------------------------------------
# the stabiliser's occlusion test: a neighbour offers a pixel only where it is the nearest surface there (include/rsdsfm_stabilize_visible.h)
# ---------------------------------------------------------------------------------------------------
STABILIZE_VISIBLE_HEADER_PATH = _header_path("rsdsfm_stabilize_visible.h")
OCCLUSION_TOL_Q16_DEFAULT = 3277  # RSDSFM_OCCLUSION_TOL_Q16_DEFAULT: about 0.05, a choice, not a measurement


def stabilize_visible_declared_symbols():
    """Names of every function include/rsdsfm_stabilize_visible.h declares"""
    return _declared("rsdsfm_stabilize_visible.h")


def stabilize_visible_launches(rows, cols):
    """kernel launches of one stabilize_visible_frame_dev call at this size: stabilize_window_launches -- the map kernel splats and the warp
    kernel tests and counts by themselves (rsdsfm_stabilize_visible_launches; host only)"""
    return _launches("rsdsfm_stabilize_visible_launches", "rows and cols must be in [2, 16384]", rows, cols)


@_solver_methods
class _StabilizeVisibleMixin:
    def stabilize_visible_frame_dev(self, d_img_n, channels, d_depth_map_n, d_R_n, d_t_n, K, rows, cols, M, m, source_id, window, d_image, d_mask, d_source=None,
                                    d_counts2=None, tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """one frame through a window and the occlusion test (rsdsfm_stabilize_visible_frame_dev; tests/stabilize_visible_spec_numpy.py):
        stabilize_window_frame_dev, but a valid pixel whose source is not the nearest surface that lands there (within tol_q16 / 65536 of
        the depth; 0: the default, 3277) is rejected and not taken.  d_counts2: two device int64 that receive [taken, rejected].  Enqueued on
        the context's stream."""
        Mh = None if M is None else _f64(M).reshape(9)
        mh = None if m is None else _f64(m).reshape(3)
        self._check(self.lib.rsdsfm_stabilize_visible_frame_dev(self._ctx, _dp(d_img_n), C.c_int32(channels), _dp(d_depth_map_n), _dp(d_R_n), _dp(d_t_n), *_k4(K), C.c_int32(rows),
                                                                C.c_int32(cols), int(mode), int(q5_mode),
                                                                C.c_int32(iterations), _p(Mh), _p(mh), C.c_int32(source_id), _window4(window), _dp(d_image),
                                                                _dp(d_mask), _np0(d_source), C.c_int32(tol_q16), _np0(d_counts2)),
                    "rsdsfm_stabilize_visible_frame_dev")

    def stabilize_visible(self, image_n, depth_map_n, R_n, t_n, K, M, m, source_id=2, window=None, image=None, mask=None, source=None, tol_q16=0, mode=BACKPROJECT_RS,
                          q5_mode=Q5_COMPAT, iterations=0, device=0):
        """host convenience around stabilize_visible_frame_dev: one candidate -- image_n (rows, cols[, 3]) uint8, depth_map_n (rows, cols) (0
        where unknown), R_n (rows, 3, 3) / (rows, 9), t_n (rows, 3), seen with (M, m) -- onto the planes image / mask / source (None: zeroed;
        the arrays passed are not changed).  window None: the full frame.  Returns (image, mask, source (rows, cols) uint8, taken, rejected)."""
        img = np.ascontiguousarray(image_n, dtype=np.uint8)
        rows, cols = img.shape[:2]
        channels = 1 if img.ndim == 2 else img.shape[2]
        with _Staging(self, device) as st:
            plane = lambda a, like: st.up(np.zeros_like(like) if a is None else np.asarray(a, dtype=np.uint8))
            zero = np.zeros((rows, cols), dtype=np.uint8)
            d_n, d_dm, d_R, d_t = st.up_frame(img, depth_map_n, R_n, t_n)
            d_out, d_mask, d_source = plane(image, img), plane(mask, zero), plane(source, zero)
            d_cnt = st.zeros(2, "int64")
            st.ready()
            self.stabilize_visible_frame_dev(d_n.data_ptr(), channels, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, M, m, int(source_id),
                                         (0, 0, rows, cols) if window is None else window, d_out.data_ptr(), d_mask.data_ptr(), d_source.data_ptr(),
                                         d_cnt.data_ptr(), tol_q16=tol_q16, mode=mode, q5_mode=q5_mode, iterations=iterations)
            out, mask, source, cnt = st.down(d_out, d_mask, d_source, d_cnt)
            return (out, mask, source) + tuple(int(x) for x in cnt)


# ---------------------------------------------------------------------------------------------------
# the search for the visible pre-image: a pixel the occlusion test rejects is looked for again from the source pixel that landed nearest the
# camera (include/rsdsfm_stabilize_search.h)
# ---------------------------------------------------------------------------------------------------
STABILIZE_SEARCH_HEADER_PATH = _header_path("rsdsfm_stabilize_search.h")


def stabilize_search_declared_symbols():
    """Names of every function include/rsdsfm_stabilize_search.h declares"""
    return _declared("rsdsfm_stabilize_search.h")


def stabilize_search_launches(rows, cols):
    """kernel launches of one stabilize_search_frame_dev call at this size: stabilize_window_launches -- the map kernel splats the keys and the
    warp kernel tests, searches and counts by themselves (rsdsfm_stabilize_search_launches; host only)"""
    return _launches("rsdsfm_stabilize_search_launches", "rows and cols must be in [2, 16384]", rows, cols)


@contextlib.contextmanager
def _occlusion_search_for(solver, search, occlusion):
    """a clip call's occlusion_search keyword: True = the context's knob at 1 for the call and put back afterwards (it needs occlusion), False =
    the knob stays where set_occlusion_search left it"""
    if not search:
        yield
        return
    if not occlusion:
        raise RsdsfmError("occlusion_search=True needs occlusion=True: the search runs where the occlusion test rejects")
    before = getattr(solver, "_occlusion_search", 0)
    solver.set_occlusion_search(1)
    try:
        yield
    finally:
        solver.set_occlusion_search(before)


@_solver_methods
class _StabilizeSearchMixin:
    def set_occlusion_search(self, on):
        """the clip calls' knob (rsdsfm_set_occlusion_search): 0 (the default) = a neighbour candidate that goes through the occlusion test goes
        through stabilize_visible_frame_dev, 1 = through stabilize_search_frame_dev; anything else is refused.  It takes effect only in calls
        with occlusion=True."""
        self._check(self.lib.rsdsfm_set_occlusion_search(self._ctx, C.c_int32(int(on))), "rsdsfm_set_occlusion_search")
        self._occlusion_search = int(on)

    def stabilize_search_frame_dev(self, d_img_n, channels, d_depth_map_n, d_R_n, d_t_n, K, rows, cols, M, m, source_id, window, d_image, d_mask, d_source=None,
                                   d_counts3=None, tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """one frame through a window, the occlusion test and the search (rsdsfm_stabilize_search_frame_dev; tests/stabilize_search_spec_numpy.py):
        stabilize_visible_frame_dev, but a pixel the test rejects is looked for again from the source pixel that landed nearest the camera on
        its cell and, where that ends on the visible surface, recovered.  d_counts3: three device int64 that receive [taken, rejected,
        recovered].  Enqueued on the context's stream."""
        Mh = None if M is None else _f64(M).reshape(9)
        mh = None if m is None else _f64(m).reshape(3)
        self._check(self.lib.rsdsfm_stabilize_search_frame_dev(self._ctx, _dp(d_img_n), C.c_int32(channels), _dp(d_depth_map_n), _dp(d_R_n), _dp(d_t_n), *_k4(K), C.c_int32(rows),
                                                               C.c_int32(cols), int(mode), int(q5_mode),
                                                               C.c_int32(iterations), _p(Mh), _p(mh), C.c_int32(source_id), _window4(window), _dp(d_image),
                                                               _dp(d_mask), _np0(d_source), C.c_int32(tol_q16), _np0(d_counts3)),
                    "rsdsfm_stabilize_search_frame_dev")

    def stabilize_search(self, image_n, depth_map_n, R_n, t_n, K, M, m, source_id=2, window=None, image=None, mask=None, source=None, tol_q16=0, mode=BACKPROJECT_RS,
                         q5_mode=Q5_COMPAT, iterations=0, device=0):
        """host convenience around stabilize_search_frame_dev: stabilize_visible's arguments.  Returns (image, mask, source (rows, cols) uint8,
        taken, rejected, recovered)."""
        img = np.ascontiguousarray(image_n, dtype=np.uint8)
        rows, cols = img.shape[:2]
        channels = 1 if img.ndim == 2 else img.shape[2]
        with _Staging(self, device) as st:
            plane = lambda a, like: st.up(np.zeros_like(like) if a is None else np.asarray(a, dtype=np.uint8))
            zero = np.zeros((rows, cols), dtype=np.uint8)
            d_n, d_dm, d_R, d_t = st.up_frame(img, depth_map_n, R_n, t_n)
            d_out, d_mask, d_source = plane(image, img), plane(mask, zero), plane(source, zero)
            d_cnt = st.zeros(3, "int64")
            st.ready()
            self.stabilize_search_frame_dev(d_n.data_ptr(), channels, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, M, m, int(source_id),
                                        (0, 0, rows, cols) if window is None else window, d_out.data_ptr(), d_mask.data_ptr(), d_source.data_ptr(),
                                        d_cnt.data_ptr(), tol_q16=tol_q16, mode=mode, q5_mode=q5_mode, iterations=iterations)
            out, mask, source, cnt = st.down(d_out, d_mask, d_source, d_cnt)
            return (out, mask, source) + tuple(int(x) for x in cnt)


# ---------------------------------------------------------------------------------------------------
# the stabiliser's seam blend: a gain per candidate and a feather next to the own frame's empty band (include/rsdsfm_stabilize_blend.h)
# ---------------------------------------------------------------------------------------------------
STABILIZE_BLEND_HEADER_PATH = _header_path("rsdsfm_stabilize_blend.h")
GAIN_ONE = 65536


class StabilizeBlendParams(C.Structure):
    _fields_ = [("min_overlap", C.c_int64), ("feather", C.c_int32), ("gain_mode", C.c_int32), ("struct_bytes", C.c_int32), ("reserved", C.c_int32 * 3)]


def stabilize_blend_declared_symbols():
    """Names of every function include/rsdsfm_stabilize_blend.h declares"""
    return _declared("rsdsfm_stabilize_blend.h")


def stabilize_blend_default_params():
    """the blend's defaults as a dict: feather = 16, gain_mode = 0, min_overlap = 1024 (rsdsfm_stabilize_blend_params_init)"""
    p = _params(StabilizeBlendParams, "rsdsfm_stabilize_blend_params_init")
    return dict(feather=p.feather, gain_mode=p.gain_mode, min_overlap=p.min_overlap)


def _stabilize_blend_params(feather, gain, min_overlap):
    """a StabilizeBlendParams with the given values over the defaults (feather / min_overlap None or 0: the default; gain False: off)"""
    return _params(StabilizeBlendParams, "rsdsfm_stabilize_blend_params_init", feather=feather or None, min_overlap=min_overlap or None, gain_mode=0 if gain else 1)


def seam_gains(sums, channels, min_overlap=0, gain_mode=0):
    """the gains of one 8-word record of seam_blend_layer_dev, with the kernel's integer arithmetic (rsdsfm_seam_gains; host only): (3,)
    uint32 in 1 / 65536, 65536 for a channel >= channels.  min_overlap 0: the default, 1024."""
    s = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1)
    if s.shape[0] != 8:
        raise ValueError("a record has 8 values")
    g = np.zeros(3, dtype=np.uint32)
    rc = load_library().rsdsfm_seam_gains(_p(s), C.c_int32(channels), C.c_int64(min_overlap), C.c_int32(gain_mode), _p(g))
    if rc != OK:
        raise RsdsfmError("rsdsfm_seam_gains failed (%d): channels 1 or 3, min_overlap >= 0, gain_mode 0 or 1" % rc)
    return g


def seam_distance_launches(rows, cols):
    """kernel launches of one seam_distance_dev call: 2 (rsdsfm_seam_distance_launches; host only)"""
    return _launches("rsdsfm_seam_distance_launches", "rows and cols must be in [2, 16384]", rows, cols)


def seam_blend_layer_launches(rows, cols):
    """kernel launches of one seam_blend_layer_dev call: 2 (rsdsfm_seam_blend_layer_launches; host only)"""
    return _launches("rsdsfm_seam_blend_layer_launches", "rows and cols must be in [2, 16384]", rows, cols)


@_solver_methods
class _StabilizeBlendMixin:
    def seam_distance_dev(self, d_mask, rows, cols, feather, d_dist):
        """the seam distance of a device mask into a device plane of bytes (rsdsfm_seam_distance_dev; tests/stabilize_blend_spec_numpy.py): 0 on
        an empty pixel, else min(feather, chessboard distance to the nearest empty pixel of the frame); feather 1 .. 64 (0: 16).  Enqueued on
        the context's stream."""
        self._check(self.lib.rsdsfm_seam_distance_dev(self._ctx, _dp(d_mask), C.c_int32(rows), C.c_int32(cols), C.c_int32(feather), _dp(d_dist)),
                    "rsdsfm_seam_distance_dev")

    def seam_distance(self, mask, feather=0, device=0):
        """host convenience around seam_distance_dev: mask (rows, cols) uint8 -> the distance plane (rows, cols) uint8"""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        with _Staging(self, device) as st:
            d_m = st.up(m)
            d_d = st.empty_like(d_m)
            st.ready()
            self.seam_distance_dev(d_m.data_ptr(), m.shape[0], m.shape[1], feather, d_d.data_ptr())
            return st.down(d_d)[0]
    def seam_blend_layer_dev(self, d_layer_image, d_layer_mask, channels, rows, cols, d_dist, source_id, d_image, d_mask, d_source, d_sums, d_counts=None, feather=None,
                             gain=True, min_overlap=None):
        """one candidate's layer onto the in-out planes (rsdsfm_seam_blend_layer_dev): the sums over the pixels the layer shares with the own
        frame (source 1) into d_sums (8 device uint64), one gain per channel from them (gain=False: none), then every pixel of the layer
        copied where source is 0 and mixed where source is 1 and d_dist (seam_distance_dev's plane for the same feather) is below feather.
        d_counts: 2 device int64 that receive [filled, blended].  source_id 2 .. 255.  Enqueued on the context's stream."""
        p = _stabilize_blend_params(feather, gain, min_overlap)
        self._check(self.lib.rsdsfm_seam_blend_layer_dev(self._ctx, _dp(d_layer_image), _dp(d_layer_mask), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols),
                                                         _dp(d_dist), C.byref(p), C.c_int32(source_id), _dp(d_image), _dp(d_mask), _dp(d_source), _dp(d_sums),
                                                         _np0(d_counts)), "rsdsfm_seam_blend_layer_dev")

    def stabilize_video_blended_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_flows, d_R, d_t, d_stab, d_masks_out, d_crop, d_crop_masks,
                                    d_blend, d_blend_masks, d_blend_sources, blend_feather=None, blend_gain=True, blend_min_overlap=None, want_gains=True,
                                    want_blend_counts=True, d_crop_sources=None, window_in=None, max_empty=0, margin=None, want_crop_counts=True, d_sources=None,
                                    fill_radius=2, want_counts=True, d_fused=None, want_valid=True, sigma=None, radius=0, translation=True, fuse_tol=None,
                                    d_masks=None, seeds=None, flow_params=None, a1=None, a2=None, link_tol=None, min_links=None, radix_bits=None,
                                    mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, trials=50, tol=0.05, use_acceleration_mode=False, use_refinement=True,
                                    depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT, flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK,
                                    use_global_shutter_mode=False, last_frame=False, occlusion=False, occlusion_tol=None, occlusion_search=False):
        """the stabilised clip, cropped, zoomed and blended, in ONE call (rsdsfm_stabilize_video_blended_dev): stabilize_video_cropped_dev with
        these arguments, then for every frame the own frame through the window into d_blend, d_blend_masks and d_blend_sources (F - 1 device
        buffers each, zeroed first), seam_distance_dev of its mask and, per neighbour, the neighbour alone on the context's layer and
        seam_blend_layer_dev (blend_feather None: 16; blend_gain False: no gain; blend_min_overlap None: 1024).  To blend without cropping pass
        window_in = (0, 0, rows, cols).  Returns stabilize_video_cropped_dev's dict plus, with want_gains, gains ((F - 1, 2 fill_radius, 3)
        uint32 in 1 / 65536, per offset -1, +1, -2, +2, ...) and, with want_blend_counts, blend_counts ((F - 1, 2 + 4 fill_radius) int64:
        [none, own_untouched, (filled, blended) per offset]); with either the call waits for the passes.
        last_frame=True (see stabilize_video_dev): the clip's last frame too; every per-frame list and array then has F entries.
        occlusion=True: the neighbour candidates go through the occlusion test (stabilize_visible_frame_dev; occlusion_tol: its tolerance as a
        fraction of the depth, None: the default) -- a rejected pixel shows up under a later offset or under none.
        occlusion_search=True (needs occlusion): set_occlusion_search(1) for this call -- a rejected pixel whose visible pre-image is found is
        recovered (stabilize_search_frame_dev) and counts under its offset; the knob is put back afterwards."""
        n = len(d_frames) - 1 + (1 if last_frame else 0)  # rendered frames
        _need_all(n, d_sources=d_sources, d_crop=d_crop, d_crop_masks=d_crop_masks, d_crop_sources=d_crop_sources, d_blend=d_blend, d_blend_masks=d_blend_masks, d_blend_sources=d_blend_sources)
        fp = _stabilize_fill_params(fill_radius, occlusion, occlusion_tol)
        fp.radius = int(fill_radius)  # 0 stays 0 here
        cp = _stabilize_crop_params(max_empty, margin)
        bp = _stabilize_blend_params(blend_feather, blend_gain, blend_min_overlap)
        width = 2 + 2 * int(fill_radius)
        counts = _counts(want_counts, n, width)
        crop_counts = _counts(want_crop_counts, n, width)
        gains = _counts(want_gains, n, max(2 * int(fill_radius), 1), 3, dtype=np.uint32)
        blend_counts = _counts(want_blend_counts, n, 2 + 4 * int(fill_radius))
        window = (C.c_int32 * 4)()
        args = _stabilize_video_args()
        with _occlusion_search_for(self, occlusion_search, occlusion):
            out = self._stabilize_video("rsdsfm_stabilize_video_blended_dev",
                                        (C.byref(fp), _ptrs(d_sources), _p(counts), C.byref(cp), _window4(window_in), _ptrs(d_crop), _ptrs(d_crop_masks), _ptrs(d_crop_sources),
                                         window, _p(crop_counts), C.byref(bp), _ptrs(d_blend), _ptrs(d_blend_masks), _ptrs(d_blend_sources), _p(gains), _p(blend_counts)),
                                        **args)
        out["window"] = tuple(int(x) for x in window)
        out.update(_wanted(n, counts=counts, crop_counts=crop_counts, blend_counts=blend_counts))
        if want_gains:
            out["gains"] = gains[:n, :2 * int(fill_radius)]
        return out


# ---------------------------------------------------------------------------------------------------
# the stabiliser's inpainting: the pixels no frame saw, from an integer pull-push pyramid (include/rsdsfm_stabilize_inpaint.h)
# ---------------------------------------------------------------------------------------------------
STABILIZE_INPAINT_HEADER_PATH = _header_path("rsdsfm_stabilize_inpaint.h")
INPAINT_SOURCE = 255  # RSDSFM_SOURCE_INPAINTED


def stabilize_inpaint_declared_symbols():
    """Names of every function include/rsdsfm_stabilize_inpaint.h declares"""
    return _declared("rsdsfm_stabilize_inpaint.h")


def inpaint_launches(rows, cols):
    """kernel launches of one inpaint_frame_dev call: 3 for a small frame, 8 at 1280 x 720 (rsdsfm_inpaint_launches; host only)"""
    return _launches("rsdsfm_inpaint_launches", "rows and cols must be in [2, 16384]", rows, cols)


@_solver_methods
class _StabilizeInpaintMixin:
    def inpaint_frame_dev(self, d_image, d_mask, channels, rows, cols, d_source=None, d_count=None):
        """the empty pixels (d_mask byte 0; only read) of the device image filled from an integer pull-push pyramid of the set ones
        (rsdsfm_inpaint_frame_dev; tests/stabilize_inpaint_spec_numpy.py).  d_source: a device plane of rows x cols bytes that receives
        INPAINT_SOURCE where a pixel was written; d_count: one device int64 that receives their number.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_inpaint_frame_dev(self._ctx, _dp(d_image), _dp(d_mask), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols), _np0(d_source),
                                                      _np0(d_count)), "rsdsfm_inpaint_frame_dev")

    def inpaint(self, image, mask, device=0):
        """host convenience around inpaint_frame_dev: image (rows, cols) or (rows, cols, 3) uint8 and mask (rows, cols) uint8 (0 = empty) ->
        (image, source (rows, cols) uint8: INPAINT_SOURCE where a pixel was written and 0 elsewhere, count)"""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if img.shape[:2] != m.shape or m.ndim != 2:
            raise ValueError("image (rows, cols[, channels]) and mask (rows, cols)")
        with _Staging(self, device) as st:
            d_img, d_m = st.up(img), st.up(m)
            d_src, d_cnt = st.zeros_like(d_m), st.zeros(1, "int64")
            st.ready()
            self.inpaint_frame_dev(d_img.data_ptr(), d_m.data_ptr(), 1 if img.ndim == 2 else img.shape[2], m.shape[0], m.shape[1], d_src.data_ptr(), d_cnt.data_ptr())
            out, src, cnt = st.down(d_img, d_src, d_cnt)
            return out, src, int(cnt[0])
    def stabilize_video_inpainted_dev(self, d_frames, rows, cols, channels, K, gamma, d_depth_maps, d_flows, d_R, d_t, d_stab, d_masks_out, d_crop, d_crop_masks,
                                      d_blend, d_blend_masks, d_blend_sources, d_inpaint, d_inpaint_sources=None, want_inpaint_counts=True, blend_feather=None,
                                      blend_gain=True, blend_min_overlap=None, want_gains=True, want_blend_counts=True, d_crop_sources=None, window_in=None,
                                      max_empty=0, margin=None, want_crop_counts=True, d_sources=None, fill_radius=2, want_counts=True, d_fused=None,
                                      want_valid=True, sigma=None, radius=0, translation=True, fuse_tol=None, d_masks=None, seeds=None, flow_params=None, a1=None,
                                      a2=None, link_tol=None, min_links=None, radix_bits=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, trials=50,
                                      tol=0.05, use_acceleration_mode=False, use_refinement=True, depth_mode=DEPTH_CERES_LM, k_sign_mode=K_COMPAT,
                                      flow_threshold=1e-10, flow_index_mode=FLOW_COMPAT_RANK, use_global_shutter_mode=False, last_frame=False, occlusion=False, occlusion_tol=None, occlusion_search=False):
        """the stabilised clip, cropped, zoomed, blended and inpainted, in ONE call (rsdsfm_stabilize_video_inpainted_dev):
        stabilize_video_blended_dev with these arguments, then for every frame d_blend copied to d_inpaint (and d_blend_sources to
        d_inpaint_sources when passed; F - 1 device buffers each) and inpaint_frame_dev on the copy with the frame's blend mask.  Returns
        stabilize_video_blended_dev's dict plus, with want_inpaint_counts, inpaint_counts ((F - 1,) int64: the pixels written per frame; the
        call then waits for the passes).
        last_frame=True (see stabilize_video_dev): the clip's last frame too; every per-frame list and array then has F entries.
        occlusion=True: the neighbour candidates go through the occlusion test (stabilize_visible_frame_dev; occlusion_tol: its tolerance as a
        fraction of the depth, None: the default) -- a rejected pixel shows up under a later offset or under none.
        occlusion_search=True (needs occlusion): set_occlusion_search(1) for this call -- a rejected pixel whose visible pre-image is found is
        recovered (stabilize_search_frame_dev) and counts under its offset; the knob is put back afterwards."""
        n = len(d_frames) - 1 + (1 if last_frame else 0)  # rendered frames
        _need_all(n, d_sources=d_sources, d_crop=d_crop, d_crop_masks=d_crop_masks, d_crop_sources=d_crop_sources, d_blend=d_blend, d_blend_masks=d_blend_masks, d_blend_sources=d_blend_sources, d_inpaint=d_inpaint, d_inpaint_sources=d_inpaint_sources)
        fp = _stabilize_fill_params(fill_radius, occlusion, occlusion_tol)
        fp.radius = int(fill_radius)  # 0 stays 0 here
        cp = _stabilize_crop_params(max_empty, margin)
        bp = _stabilize_blend_params(blend_feather, blend_gain, blend_min_overlap)
        width = 2 + 2 * int(fill_radius)
        counts = _counts(want_counts, n, width)
        crop_counts = _counts(want_crop_counts, n, width)
        gains = _counts(want_gains, n, max(2 * int(fill_radius), 1), 3, dtype=np.uint32)
        blend_counts = _counts(want_blend_counts, n, 2 + 4 * int(fill_radius))
        inpaint_counts = _counts(want_inpaint_counts, n)
        window = (C.c_int32 * 4)()
        args = _stabilize_video_args()
        with _occlusion_search_for(self, occlusion_search, occlusion):
            out = self._stabilize_video("rsdsfm_stabilize_video_inpainted_dev",
                                        (C.byref(fp), _ptrs(d_sources), _p(counts), C.byref(cp), _window4(window_in), _ptrs(d_crop), _ptrs(d_crop_masks), _ptrs(d_crop_sources),
                                         window, _p(crop_counts), C.byref(bp), _ptrs(d_blend), _ptrs(d_blend_masks), _ptrs(d_blend_sources), _p(gains), _p(blend_counts),
                                         _ptrs(d_inpaint), _ptrs(d_inpaint_sources), _p(inpaint_counts)), **args)
        out["window"] = tuple(int(x) for x in window)
        out.update(_wanted(n, counts=counts, crop_counts=crop_counts, blend_counts=blend_counts, inpaint_counts=inpaint_counts))
        if want_gains:
            out["gains"] = gains[:n, :2 * int(fill_radius)]
        return out


# ---------------------------------------------------------------------------------------------------
# the clip's last frame: the last pair's depth map moved onto it, and its pose table (include/rsdsfm_last_frame.h)
# ---------------------------------------------------------------------------------------------------
LAST_FRAME_HEADER_PATH = _header_path("rsdsfm_last_frame.h")


def last_frame_declared_symbols():
    """Names of every function include/rsdsfm_last_frame.h declares"""
    return _declared("rsdsfm_last_frame.h")


def last_frame_motion(v, w, k):
    """the motion that puts a pair's SECOND frame into pose_table's form (rsdsfm_last_frame_motion; host arithmetic, no GPU;
    tests/last_frame_spec_numpy.py): v' = v (2 + 3 k) / (2 + k), w' likewise, k' = k / (1 + k); the identity bit for bit at k = 0.
    -> (v' (3,), w' (3,), k')"""
    vo, wo, ko = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double()
    rc = load_library().rsdsfm_last_frame_motion(_v3(v), _v3(w), C.c_double(k), vo, wo, C.byref(ko))
    if rc != OK:
        raise RsdsfmError("rsdsfm_last_frame_motion failed (%d): the motion must be finite with 1 + k > 0" % rc)
    return np.array(vo[:]), np.array(wo[:]), ko.value


def advance_depth_launches(rows, cols):
    """kernel launches of one advance_depth_dev call: 3 (rsdsfm_advance_depth_launches; host only)"""
    return _launches("rsdsfm_advance_depth_launches", "rows and cols must be in [2, 16384]", rows, cols)


@_solver_methods
class _LastFrameMixin:
    def advance_depth_dev(self, d_field, d_depth_map, v, w, k, rows, cols, K, gamma, d_out, global_shutter=False, d_plane=None, d_count=None):
        """a pair's depth map moved to its second capture, as a depth map of the second frame (rsdsfm_advance_depth_dev;
        tests/last_frame_spec_numpy.py): d_field the pair's field (rows x cols x 2, row-major), d_depth_map / d_out column-major maps, (v, w, k)
        the pair's final motion (host).  d_plane: a device plane of rows x cols uint64 that receives the winners' bit patterns; d_count: one
        device int64 that receives the number of pixels with a value.  Enqueued on the context's stream."""
        d = C.c_double
        self._check(self.lib.rsdsfm_advance_depth_dev(self._ctx, _dp(d_field), _dp(d_depth_map), _v3(v), _v3(w), d(k), C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma),
                                                      C.c_int32(int(bool(global_shutter))), _dp(d_out), _np0(d_plane),
                                                      _np0(d_count)), "rsdsfm_advance_depth_dev")

    def advance_depth(self, field, depth_map, v, w, k, K, gamma, global_shutter=False, want_plane=False, device=0):
        """host convenience around advance_depth_dev: field (rows, cols, 2), depth_map (rows, cols) (0 where unknown) -> (map (rows, cols),
        count[, plane (rows, cols) uint64])"""
        F, Z = _f64(field), _f64(depth_map)
        rows, cols = Z.shape
        if F.shape != (rows, cols, 2):
            raise ValueError("field (rows, cols, 2) and depth_map (rows, cols)")
        with _Staging(self, device) as st:
            d_F, d_Z = st.up(F), st.up(Z.T)  # column-major rows x cols
            d_out = st.empty((cols, rows), "float64")
            d_plane = st.empty((rows, cols), "int64") if want_plane else None
            d_cnt = st.zeros(1, "int64")
            st.ready()
            self.advance_depth_dev(d_F.data_ptr(), d_Z.data_ptr(), v, w, k, rows, cols, K, gamma, d_out.data_ptr(), global_shutter,
                                   d_plane.data_ptr() if want_plane else None, d_cnt.data_ptr())
            moved, cnt = st.down(d_out, d_cnt)
            out = (np.ascontiguousarray(moved.T), int(cnt[0]))
            return out + (st.host(d_plane).view(np.uint64),) if want_plane else out
    def last_frame_dev(self, d_field, d_depth_map, v, w, k, rows, cols, K, gamma, d_out, d_R, d_t, global_shutter=False, d_plane=None, d_count=None):
        """the last frame's depth map and pose table from the last pair (rsdsfm_last_frame_dev): advance_depth_dev, last_frame_motion and
        pose_table_dev of the moved motion into d_R (rows x 9) / d_t (rows x 3), one after another.  Enqueued on the context's stream."""
        d = C.c_double
        self._check(self.lib.rsdsfm_last_frame_dev(self._ctx, _dp(d_field), _dp(d_depth_map), _v3(v), _v3(w), d(k), C.c_int32(rows), C.c_int32(cols), *_k4(K), d(gamma),
                                                   C.c_int32(int(bool(global_shutter))), _dp(d_out), _dp(d_R), _dp(d_t),
                                                   _np0(d_plane), _np0(d_count)), "rsdsfm_last_frame_dev")


# ---------------------------------------------------------------------------------------------------
# the retimer: a frame at any instant along the camera path, from the two input frames next to it in time (include/rsdsfm_retime.h)
# ---------------------------------------------------------------------------------------------------
RETIME_HEADER_PATH = _header_path("rsdsfm_retime.h")
RETIME_NONE, RETIME_FROM_A, RETIME_FROM_B, RETIME_DISSOLVED, RETIME_CONFLICT_A, RETIME_CONFLICT_B = range(6)


class RetimeParams(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("occlusion", C.c_int32), ("occlusion_tol_q16", C.c_int32), ("struct_bytes", C.c_int32), ("reserved", C.c_int32 * 4)]


def retime_declared_symbols():
    """Names of every function include/rsdsfm_retime.h declares"""
    return _declared("rsdsfm_retime.h")


def retime_default_params():
    """the retimer's defaults as a dict: threshold = 24, occlusion = 0, occlusion_tol_q16 = 0 (rsdsfm_retime_params_init)"""
    p = _params(RetimeParams, "rsdsfm_retime_params_init")
    return dict(threshold=p.threshold, occlusion=p.occlusion, occlusion_tol_q16=p.occlusion_tol_q16)


def _retime_params(threshold, occlusion, occlusion_tol_q16):
    """a RetimeParams with the given values over the defaults (threshold None: the default)"""
    return _params(RetimeParams, "rsdsfm_retime_params_init", threshold=threshold, occlusion=occlusion, occlusion_tol_q16=occlusion_tol_q16)


def path_at(A_path, c_path, t):
    """the pose at time t on a path (rsdsfm_path_at; host arithmetic, no GPU; tests/retime_spec_numpy.py): A_path (F, 3, 3), c_path (F, 3),
    t in [0, F - 1] -> (A_t (3, 3), c_t (3,)).  An integer t returns the entry's bytes; between two poses the rotation moves along the
    geodesic and the centre along the segment."""
    a, cc = _f64(A_path).reshape(-1, 9), _f64(c_path).reshape(-1, 3)
    if cc.shape[0] != a.shape[0]:
        raise ValueError("every pose needs a rotation and a centre")
    A_t, c_t = np.empty(9), np.empty(3)
    rc = load_library().rsdsfm_path_at(_p(a), _p(cc), C.c_int32(a.shape[0]), C.c_double(t), _p(A_t), _p(c_t))
    if rc != OK:
        raise RsdsfmError("rsdsfm_path_at failed (%d): at least one pose, t finite and in [0, nposes - 1]" % rc)
    return A_t.reshape(3, 3), c_t


def retime_poses(A, c, A_path, c_path, scales, t, nsources=None):
    """the sources of the frame at time t and their poses (rsdsfm_retime_poses; host): A, c the chain's, A_path, c_path the path to ride,
    nsources the frames that have a depth map (None: len(scales)) -> (sources (n0,) or (n0, n0 + 1), weight_q16, M (nsrc, 3, 3), m (nsrc, 3),
    A_t (3, 3), c_t (3,))"""
    a, cc, ap, cp = _f64(A).reshape(-1, 9), _f64(c).reshape(-1, 3), _f64(A_path).reshape(-1, 9), _f64(c_path).reshape(-1, 3)
    sc = _f64(scales).reshape(-1)
    ns = sc.shape[0] if nsources is None else int(nsources)
    if min(a.shape[0], cc.shape[0], ap.shape[0], cp.shape[0], sc.shape[0]) < ns:
        raise ValueError("every source needs a pose on both paths and a scale")
    src, nsrc, w = (C.c_int32 * 2)(), C.c_int32(), C.c_int32()
    M, m, A_t, c_t = np.empty((2, 9)), np.empty((2, 3)), np.empty(9), np.empty(3)
    rc = load_library().rsdsfm_retime_poses(_p(a), _p(cc), _p(ap), _p(cp), _p(sc), C.c_int32(ns), C.c_double(t), src, C.byref(nsrc), C.byref(w), _p(M), _p(m), _p(A_t),
                                            _p(c_t))
    if rc != OK:
        raise RsdsfmError("rsdsfm_retime_poses failed (%d): t finite and in [0, nsources - 1], the sources' scales finite and positive" % rc)
    n = nsrc.value
    return tuple(int(x) for x in src[:n]), int(w.value), M[:n].reshape(n, 3, 3), m[:n], A_t.reshape(3, 3), c_t


def retime_times(nsources, factor):
    """the instants of a clip slowed down by an integer `factor`: i / factor for i = 0 .. (nsources - 1) factor"""
    nsources, factor = int(nsources), int(factor)
    if nsources < 1 or factor < 1:
        raise ValueError("nsources >= 1 and factor >= 1")
    return np.arange((nsources - 1) * factor + 1, dtype=np.float64) / np.float64(factor)


def retime_launches(rows, cols, nsrc=2):
    """kernel launches of one retime_frame_dev call: nsrc stabilize_window_launches + 1 (rsdsfm_retime_launches; host only)"""
    return _launches("rsdsfm_retime_launches", "rows and cols must be in [2, 16384], nsrc 1 or 2", rows, cols, nsrc)


def retime_merge_launches():
    """kernel launches of one retime_merge_dev call: 1 (rsdsfm_retime_merge_launches; host only)"""
    return int(load_library().rsdsfm_retime_merge_launches())


@_solver_methods
class _RetimeMixin:
    def retime_merge_dev(self, d_image_a, d_mask_a, d_image_b, d_mask_b, channels, rows, cols, weight_q16, d_image, d_mask, d_source=None, d_counts5=None,
                         threshold=24):
        """two layers merged by how near each is in time (rsdsfm_retime_merge_dev; tests/retime_spec_numpy.py): where only one layer is set its
        bytes, where both are a cross-dissolve with weight_q16 / 65536 on b, or the nearer layer's bytes where they differ by more than
        `threshold`.  d_image_b = d_mask_b = None: b absent (weight 0).  d_source receives the RETIME_* byte per pixel, d_counts5 (five device
        int64) [none, a only, b only, dissolved, conflict].  Every output byte is written.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_retime_merge_dev(self._ctx, _dp(d_image_a), _dp(d_mask_a), _np0(d_image_b), _np0(d_mask_b), C.c_int32(channels), C.c_int32(rows),
                                                     C.c_int32(cols), C.c_int32(weight_q16), C.c_int32(threshold), _dp(d_image), _dp(d_mask), _np0(d_source),
                                                     _np0(d_counts5)), "rsdsfm_retime_merge_dev")

    def retime_merge(self, image_a, mask_a, image_b=None, mask_b=None, weight_q16=0, threshold=24, device=0):
        """host convenience around retime_merge_dev -> (image, mask, source (rows, cols) uint8, counts (5,) int64)"""
        ia, ma = np.ascontiguousarray(image_a, dtype=np.uint8), np.ascontiguousarray(mask_a, dtype=np.uint8)
        rows, cols = ma.shape
        with _Staging(self, device) as st:
            d_ia, d_ma, d_ib, d_mb = st.up(ia), st.up(ma), st.up(image_b, np.uint8), st.up(mask_b, np.uint8)
            d_out, d_mask, d_src = st.empty_like(d_ia), st.empty_like(d_ma), st.empty_like(d_ma)
            d_cnt = st.zeros(5, "int64")
            st.ready()
            ptr = lambda x: None if x is None else x.data_ptr()
            self.retime_merge_dev(d_ia.data_ptr(), d_ma.data_ptr(), ptr(d_ib), ptr(d_mb), 1 if ia.ndim == 2 else ia.shape[2], rows, cols, int(weight_q16),
                                  d_out.data_ptr(), d_mask.data_ptr(), d_src.data_ptr(), d_cnt.data_ptr(), threshold=threshold)
            return st.down(d_out, d_mask, d_src, d_cnt)
    def retime_frame_dev(self, d_images, channels, d_depth_maps, d_Rs, d_ts, K, rows, cols, M, m, weight_q16, d_image, d_mask, d_source=None, d_counts5=None,
                         window=None, threshold=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, params=None):
        """one frame at one instant (rsdsfm_retime_frame_dev): d_images, d_depth_maps, d_Rs, d_ts are lists of one or two device pointers (the
        sources of retime_poses), M (nsrc, 3, 3), m (nsrc, 3) and weight_q16 its results.  Every source is rendered alone onto a layer of the
        context (stabilize_window_frame_dev; occlusion=True: stabilize_visible_frame_dev, or stabilize_search_frame_dev with
        set_occlusion_search(1)) and the layers are merged (retime_merge_dev) into d_image, d_mask, d_source, d_counts5.  window None: the full
        frame.  params: a RetimeParams passed as it is, instead of threshold / occlusion / occlusion_tol_q16.  Enqueued on the context's stream."""
        nsrc = len(d_images)
        Mh = None if M is None else _f64(M).reshape(-1)
        mh = None if m is None else _f64(m).reshape(-1)
        if (Mh is not None and Mh.size < 9 * min(nsrc, 2)) or (mh is not None and mh.size < 3 * min(nsrc, 2)) or min(len(d_depth_maps), len(d_Rs), len(d_ts)) < min(nsrc, 2):
            raise RsdsfmError("retime_frame_dev: every source needs an image, a depth map, a pose table and a pose (M, m)")
        p = params if params is not None else _retime_params(threshold, occlusion, occlusion_tol_q16)
        self._check(self.lib.rsdsfm_retime_frame_dev(self._ctx, _ptrs(d_images, min(len(d_images), 2)), C.c_int32(channels), _ptrs(d_depth_maps, min(len(d_depth_maps), 2)),
                                                     _ptrs(d_Rs, min(len(d_Rs), 2)), _ptrs(d_ts, min(len(d_ts),
                                                     2)), *_k4(K), C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(nsrc), _p(Mh),
                                                     _p(mh), C.c_int32(weight_q16), C.byref(p), _window4(window), _dp(d_image), _dp(d_mask), _np0(d_source),
                                                     _np0(d_counts5)), "rsdsfm_retime_frame_dev")

    def retime(self, images, depth_maps, Rs, ts, K, M, m, weight_q16, window=None, threshold=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS,
               q5_mode=Q5_COMPAT, iterations=0, device=0):
        """host convenience around retime_frame_dev: images, depth_maps (rows, cols), Rs, ts: lists of one or two sources' host arrays
        -> (image, mask, source (rows, cols) uint8, counts (5,) int64)"""
        imgs = [np.ascontiguousarray(i, dtype=np.uint8) for i in images]
        rows, cols = imgs[0].shape[:2]
        with _Staging(self, device) as st:
            d_i, d_dm, d_R, d_t = ([st.up(x) for x in xs] for xs in (imgs, [np.asarray(z, dtype=np.float64).T for z in depth_maps],
                                                                     [_f64(np.asarray(R).reshape(rows, 9)) for R in Rs], [_f64(t) for t in ts]))
            d_out, d_mask = st.empty_like(d_i[0]), st.empty((rows, cols))
            d_src, d_cnt = st.empty_like(d_mask), st.zeros(5, "int64")
            st.ready()
            self.retime_frame_dev(st.ptrs(d_i), 1 if imgs[0].ndim == 2 else imgs[0].shape[2], st.ptrs(d_dm), st.ptrs(d_R), st.ptrs(d_t), K, rows, cols, M, m, int(weight_q16),
                                  d_out.data_ptr(), d_mask.data_ptr(), d_src.data_ptr(), d_cnt.data_ptr(), window=window, threshold=threshold, occlusion=occlusion,
                                  occlusion_tol_q16=occlusion_tol_q16, mode=mode, q5_mode=q5_mode, iterations=iterations)
            return st.down(d_out, d_mask, d_src, d_cnt)
    def retime_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, times, d_out, d_out_masks, d_out_sources=None,
                         want_counts=True, window=None, threshold=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """a solved clip retimed (rsdsfm_retime_video_dev): d_depth_maps, d_R, d_t (their length is the number of sources; d_frames has at least
        as many) and the host arrays A, c, scales as a stabilise clip call left them, A_path, c_path the path to ride (its A_s, c_s, or A, c);
        for every t of `times` retime_poses and retime_frame_dev into d_out[i], d_out_masks[i], d_out_sources[i].  Returns dict(sources
        (ntimes, 2) int32, -1 for absent; weights (ntimes,) int32; with want_counts counts (ntimes, 5) int64 -- the call then waits)."""
        ns, a, cc, ap, cp, sc = _clip_front("retime_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t)
        tm = _f64(times).reshape(-1)
        nt = tm.shape[0]
        _need_all(nt, d_out=d_out, d_out_masks=d_out_masks, d_out_sources=d_out_sources)
        p = _retime_params(threshold, occlusion, occlusion_tol_q16)
        sources, weights = _counts(True, nt, 2, dtype=np.int32, fill=-1), _counts(True, nt, dtype=np.int32)
        counts = _counts(want_counts, nt, 5)
        self._check(self.lib.rsdsfm_retime_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                     _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode),
                                                     int(q5_mode), C.c_int32(iterations), _p(tm), C.c_int32(nt), C.byref(p), _window4(window), _ptrs(d_out, nt),
                                                     _ptrs(d_out_masks, nt), _ptrs(d_out_sources, nt), _p(sources), _p(weights), _p(counts)), "rsdsfm_retime_video_dev")
        return _wanted(nt, sources=sources, weights=weights, counts=counts)


# ---------------------------------------------------------------------------------------------------
# the synthetic shutter: a frame exposed over a window of time, the mean of sub-instant renders (include/rsdsfm_shutter.h)
# ---------------------------------------------------------------------------------------------------
SHUTTER_HEADER_PATH = _header_path("rsdsfm_shutter.h")
SHUTTER_SAMPLES_MAX = 64


class ShutterParams(C.Structure):
    _fields_ = [("shutter", C.c_double), ("samples", C.c_int32), ("min_samples", C.c_int32), ("struct_bytes", C.c_int32), ("reserved", C.c_int32 * 3)]


def shutter_declared_symbols():
    """Names of every function include/rsdsfm_shutter.h declares"""
    return _declared("rsdsfm_shutter.h")


def _shutter_params(shutter=None, samples=None, min_samples=None):
    """a ShutterParams with the given values over the defaults (None: the default)"""
    return _params(ShutterParams, "rsdsfm_shutter_params_init", shutter=shutter, samples=samples, min_samples=min_samples)


def shutter_default_params():
    """the shutter's defaults as a dict: shutter = 0.5, samples = 8, min_samples = 1 (rsdsfm_shutter_params_init); choices, not measurements"""
    p = _shutter_params()
    return dict(shutter=p.shutter, samples=p.samples, min_samples=p.min_samples)


def shutter_times(t, shutter, samples, nsources):
    """the kept sub-instants of the exposure about t (rsdsfm_shutter_times; host arithmetic, no GPU; tests/shutter_spec_numpy.py):
    t_j = t + shutter ((j + 0.5) / samples - 0.5) for j = 0 .. samples - 1, those inside [0, nsources - 1], in order -> (kept,) float64"""
    n = int(samples)
    out, kept = np.zeros(max(min(n, SHUTTER_SAMPLES_MAX), 1)), C.c_int32()
    rc = load_library().rsdsfm_shutter_times(C.c_double(t), C.c_double(shutter), C.c_int32(n), C.c_int32(nsources), _p(out), C.byref(kept))
    if rc != OK:
        raise RsdsfmError("rsdsfm_shutter_times failed (%d): samples in [1, 64], shutter finite and in [0, nsources - 1], t finite and in [0, nsources - 1]" % rc)
    return out[:kept.value].copy()


def shutter_from_angle(angle_deg, factor):
    """the shutter width, in input-frame intervals, of a shutter angle on a clip retimed by `factor` (output frames per input frame; 1 / 2
    halves the frame rate): angle / 360 of the output frame's interval 1 / factor"""
    return float(angle_deg) / 360.0 / float(factor)


def shutter_launches(rows, cols, n_one_source, n_two_sources):
    """kernel launches of one shutter_frame_dev call whose kept sub-instants are n_one_source integer instants and n_two_sources others: their
    retime_launches plus one accumulate each (rsdsfm_shutter_launches; host only)"""
    return _launches("rsdsfm_shutter_launches", "rows and cols in [2, 16384], counts >= 0 with a sum in [1, 64]", rows, cols, n_one_source, n_two_sources)


def shutter_accumulate_launches():
    """kernel launches of one shutter_accumulate_dev call: 1 (rsdsfm_shutter_accumulate_launches; host only)"""
    return int(load_library().rsdsfm_shutter_accumulate_launches())


@_solver_methods
class _ShutterMixin:
    def shutter_accumulate_dev(self, d_image, d_mask, channels, rows, cols, d_cells, first, last, nsamples, min_samples=1, d_image_out=None, d_mask_out=None,
                               d_coverage=None, d_counts3=None):
        """one sample accumulated (rsdsfm_shutter_accumulate_dev; tests/shutter_spec_numpy.py): d_cells holds rows x cols cells of channels + 1
        uint16 [sums, n] (None only with first and last).  first: the cells are set from the sample; otherwise the sample is added where its mask
        is not 0.  last: the cells are not written; the mean (round half up) goes to d_image_out and 1 to d_mask_out where n >= min_samples, n to
        d_coverage, [unset, partial, full] to d_counts3 (three device int64).  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_shutter_accumulate_dev(self._ctx, _dp(d_image), _dp(d_mask), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols), _np0(d_cells),
                                                           C.c_int32(int(first)), C.c_int32(int(last)), C.c_int32(nsamples), C.c_int32(min_samples), _np0(d_image_out),
                                                           _np0(d_mask_out), _np0(d_coverage), _np0(d_counts3)), "rsdsfm_shutter_accumulate_dev")

    def shutter_accumulate(self, samples, min_samples=1, device=0):
        """host convenience around shutter_accumulate_dev: samples, a list of 1 .. 64 (image, mask) pairs of host arrays
        -> (image, mask, coverage (rows, cols) uint8, counts (3,) int64 [unset, partial, full])"""
        S = len(samples)
        first = np.ascontiguousarray(samples[0][0], dtype=np.uint8)
        rows, cols = first.shape[:2]
        ch = 1 if first.ndim == 2 else first.shape[2]
        with _Staging(self, device) as st:
            d_s = [(st.up(i, np.uint8), st.up(m, np.uint8)) for i, m in samples]
            d_cells = st.empty((rows, cols, ch + 1), "int16")
            d_out, d_mask = st.empty_like(d_s[0][0]), st.empty((rows, cols))
            d_cov, d_cnt = st.empty_like(d_mask), st.zeros(3, "int64")
            st.ready()
            for j, (d_i, d_m) in enumerate(d_s):
                self.shutter_accumulate_dev(d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == S - 1, S, min_samples, d_out.data_ptr(),
                                            d_mask.data_ptr(), d_cov.data_ptr(), d_cnt.data_ptr())
            return st.down(d_out, d_mask, d_cov, d_cnt)
    def shutter_frame_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, t, d_image, d_mask, d_coverage=None,
                          d_counts3=None, shutter=None, samples=None, min_samples=None, window=None, threshold=None, occlusion=False, occlusion_tol_q16=0,
                          mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, shutter_params=None, retime_params=None):
        """one exposed frame of a solved clip (rsdsfm_shutter_frame_dev): the clip as retime_video_dev takes it; for every kept sub-instant of
        shutter_times(t, shutter, samples, len(d_depth_maps)) retime_poses, retime_frame_dev onto the context's sample planes and
        shutter_accumulate_dev, the mean into d_image, d_mask, d_coverage, d_counts3.  shutter, samples, min_samples None: the defaults (0.5, 8,
        1); shutter_params / retime_params: structs passed as they are instead.  Returns the kept count.  Enqueued on the context's stream."""
        ns, a, cc, ap, cp, sc = _clip_front("shutter_frame_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t)
        sp = shutter_params if shutter_params is not None else _shutter_params(shutter, samples, min_samples)
        rp = retime_params if retime_params is not None else _retime_params(threshold, occlusion, occlusion_tol_q16)
        d = C.c_double
        kept = C.c_int32()
        self._check(self.lib.rsdsfm_shutter_frame_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                      _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode),
                                                      int(q5_mode), C.c_int32(iterations), d(t), C.byref(sp), C.byref(rp), _window4(window), _dp(d_image), _dp(d_mask),
                                                      _np0(d_coverage), _np0(d_counts3), C.byref(kept)), "rsdsfm_shutter_frame_dev")
        return int(kept.value)

    def shutter_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, times, d_out, d_out_masks, d_out_coverage=None,
                          want_counts=True, shutter=None, samples=None, min_samples=None, window=None, threshold=None, occlusion=False, occlusion_tol_q16=0,
                          mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """a solved clip exposed at every t of `times` (rsdsfm_shutter_video_dev): one shutter_frame_dev per instant into d_out[i],
        d_out_masks[i], d_out_coverage[i].  Returns dict(kept (ntimes,) int32; with want_counts counts (ntimes, 3) int64 [unset, partial, full]
        -- the call then waits)."""
        ns, a, cc, ap, cp, sc = _clip_front("shutter_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t)
        tm = _f64(times).reshape(-1)
        nt = tm.shape[0]
        _need_all(nt, d_out=d_out, d_out_masks=d_out_masks, d_out_coverage=d_out_coverage)
        sp, rp = _shutter_params(shutter, samples, min_samples), _retime_params(threshold, occlusion, occlusion_tol_q16)
        kept = _counts(True, nt, dtype=np.int32)
        counts = _counts(want_counts, nt, 3)
        self._check(self.lib.rsdsfm_shutter_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                      _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode),
                                                      int(q5_mode), C.c_int32(iterations), _p(tm), C.c_int32(nt), C.byref(sp), C.byref(rp), _window4(window),
                                                      _ptrs(d_out, nt), _ptrs(d_out_masks, nt), _ptrs(d_out_coverage, nt), _p(kept), _p(counts)), "rsdsfm_shutter_video_dev")
        return _wanted(nt, kept=kept, counts=counts)


# ---------------------------------------------------------------------------------------------------
# the temporal denoise: a frame averaged with its registered neighbours, patch-weighted (include/rsdsfm_denoise.h)
# ---------------------------------------------------------------------------------------------------
DENOISE_HEADER_PATH = _header_path("rsdsfm_denoise.h")
DENOISE_RADIUS_MAX = 7
DENOISE_LAYERS_MAX = 14


class DenoiseParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("strength", C.c_int32), ("gain_mode", C.c_int32), ("occlusion", C.c_int32), ("occlusion_tol_q16", C.c_int32),
                ("struct_bytes", C.c_int32), ("min_overlap", C.c_int64), ("reserved", C.c_int32 * 4)]


def denoise_declared_symbols():
    """Names of every function include/rsdsfm_denoise.h declares"""
    return _declared("rsdsfm_denoise.h")


def _denoise_params(radius=None, strength=None, gain=True, occlusion=False, occlusion_tol_q16=0, min_overlap=None):
    """a DenoiseParams with the given values over the defaults (None: the default)"""
    return _params(DenoiseParams, "rsdsfm_denoise_params_init", radius=radius, strength=strength, min_overlap=min_overlap, gain_mode=0 if gain else 1, occlusion=occlusion,
                   occlusion_tol_q16=occlusion_tol_q16)


def denoise_default_params():
    """the denoise's defaults as a dict: radius = 2, strength = 12, min_overlap = 1024 (rsdsfm_denoise_params_init); choices, not measurements"""
    p = _denoise_params()
    return dict(radius=p.radius, strength=p.strength, min_overlap=p.min_overlap, gain_mode=p.gain_mode, occlusion=p.occlusion)


def denoise_launches(rows, cols, nsrc):
    """kernel launches of one denoise_frame_dev call on nsrc sources: nsrc stabilize_window_launches + 2 (nsrc - 1), or + 1 with one source
    (rsdsfm_denoise_launches; host only)"""
    return _launches("rsdsfm_denoise_launches", "rows and cols in [2, 16384], nsrc in [1, 15]", rows, cols, nsrc)


def denoise_accumulate_launches():
    """kernel launches of one denoise_accumulate_dev call: 1 (rsdsfm_denoise_accumulate_launches; host only)"""
    return int(load_library().rsdsfm_denoise_accumulate_launches())


@_solver_methods
class _DenoiseMixin:
    def seam_overlap_sums_dev(self, d_image, d_source, d_layer, d_layer_mask, channels, rows, cols, d_sums8):
        """the seam blend's record as a call of its own (rsdsfm_seam_overlap_sums_dev; tests/stabilize_blend_spec_numpy.py's overlap_sums):
        d_sums8 (8 device uint64) = [count, sum image_c, sum layer_c, 0 ...] over d_source == 1 under a set layer mask.  Enqueued on the context's
        stream."""
        self._check(self.lib.rsdsfm_seam_overlap_sums_dev(self._ctx, _dp(d_image), _dp(d_source), _dp(d_layer), _dp(d_layer_mask), C.c_int32(channels), C.c_int32(rows),
                                                          C.c_int32(cols), _dp(d_sums8)), "rsdsfm_seam_overlap_sums_dev")

    def denoise_accumulate_dev(self, d_ref, d_ref_mask, d_layer, d_layer_mask, channels, rows, cols, d_cells, first, last, d_sums8=None, min_overlap=0, gain_mode=0,
                               strength=0, d_image_out=None, d_mask_out=None, d_weight=None, d_counts3=None):
        """one layer accumulated onto the cells (rsdsfm_denoise_accumulate_dev; tests/denoise_spec_numpy.py): the weight of a layer's pixel falls
        with the mean absolute difference to the reference over its 3 x 3 patch, 16 at none, 0 at `strength` per channel.  d_layer = d_layer_mask
        = None: no layer (first and last).  d_sums8: the layer's record (seam_overlap_sums_dev), None: no gain.  first: the cells are set from
        the reference; last: the cells are not written, the mean goes to d_image_out, 1 to d_mask_out where anything counted, the summed weight
        to d_weight and [unset, own only, averaged] to d_counts3 (three device int64).  At most 14 layers.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_denoise_accumulate_dev(self._ctx, _dp(d_ref), _dp(d_ref_mask), _np0(d_layer), _np0(d_layer_mask), C.c_int32(channels), C.c_int32(rows),
                                                           C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode), C.c_int32(strength), _np0(d_cells),
                                                           C.c_int32(int(first)), C.c_int32(int(last)), _np0(d_image_out), _np0(d_mask_out), _np0(d_weight),
                                                           _np0(d_counts3)), "rsdsfm_denoise_accumulate_dev")

    def denoise_accumulate(self, ref, ref_mask, layers, records=None, min_overlap=0, gain_mode=0, strength=0, device=0):
        """host convenience around denoise_accumulate_dev: the reference (image, mask), layers a list of 0 .. 14 (image, mask) pairs of host
        arrays, records None or one 8-word record (or None) per layer
        -> (image, mask, weight (rows, cols) uint8, counts (3,) int64 [unset, own only, averaged])"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        ch = 1 if ref.ndim == 2 else ref.shape[2]
        with _Staging(self, device) as st:
            d_ref, d_rm = st.up(ref), st.up(ref_mask, np.uint8)
            d_l = [(st.up(i, np.uint8), st.up(m, np.uint8)) for i, m in layers]
            d_rec = [None if records is None or records[j] is None else st.up64(records[j]) for j in range(len(layers))]
            d_cells = st.empty((rows, cols, ch + 1), "int16")
            d_out, d_mask = st.empty_like(d_ref), st.empty((rows, cols))
            d_w, d_cnt = st.empty_like(d_mask), st.zeros(3, "int64")
            st.ready()
            outs = dict(d_image_out=d_out.data_ptr(), d_mask_out=d_mask.data_ptr(), d_weight=d_w.data_ptr(), d_counts3=d_cnt.data_ptr())
            if not d_l:
                self.denoise_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), None, None, ch, rows, cols, None, True, True, None, min_overlap, gain_mode, strength, **outs)
            for j, (d_i, d_m) in enumerate(d_l):
                self.denoise_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == len(d_l) - 1,
                                            d_rec[j].data_ptr() if d_rec[j] is not None else None, min_overlap, gain_mode, strength, **outs)
            return st.down(d_out, d_mask, d_w, d_cnt)
    def denoise_frame_dev(self, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_weight=None, d_counts3=None, strength=None, gain=True,
                          min_overlap=None, window=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, params=None):
        """one denoised frame (rsdsfm_denoise_frame_dev): d_images, d_depth_maps, d_R, d_t lists of 1 .. 15 device pointers, source 0 the own
        frame and the others its neighbours; M (nsrc, 3, 3), m (nsrc, 3) every source's pose in the target camera.  The own frame through
        stabilize_window_frame_dev, every neighbour alone on the context's layer, seam_overlap_sums_dev and denoise_accumulate_dev per neighbour;
        the mean into d_image, d_mask, d_weight, d_counts3.  params: a DenoiseParams passed as it is instead of the keywords.  Enqueued on the
        context's stream."""
        ns, Mm, mm = _frame_front("denoise_frame_dev", d_images, M, m, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
        dp = params if params is not None else _denoise_params(None, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
        self._check(self.lib.rsdsfm_denoise_frame_dev(self._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), *_k4(K),
                                                      C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns), _p(Mm), _p(mm),
                                                      C.byref(dp), _window4(window), _dp(d_image), _dp(d_mask), _np0(d_weight), _np0(d_counts3)), "rsdsfm_denoise_frame_dev")

    def denoise_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_weights=None,
                          want_counts=True, radius=None, strength=None, gain=True, min_overlap=None, window=None, occlusion=False, occlusion_tol_q16=0,
                          mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """a solved clip denoised (rsdsfm_denoise_video_dev): the clip as retime_video_dev takes it; for every frame q the own pose by
        retime_poses(t = q), the neighbours within `radius` (None: 2) by neighbour_poses on the same path, and denoise_frame_dev into d_out[q],
        d_out_masks[q], d_out_weights[q].  A_path = A, c_path = c denoises the rectified frames in place.  Returns dict(); with want_counts
        counts (nsources, 3) int64 [unset, own only, averaged] -- the call then waits."""
        ns, a, cc, ap, cp, sc = _clip_front("denoise_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out,
                d_out_masks=d_out_masks, d_out_weights=d_out_weights)
        dp = _denoise_params(radius, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
        counts = _counts(want_counts, ns, 3)
        self._check(self.lib.rsdsfm_denoise_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                      _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode), int(q5_mode),
                                                      C.c_int32(iterations), C.byref(dp), _window4(window), _ptrs(d_out, ns), _ptrs(d_out_masks, ns), _ptrs(d_out_weights, ns), _p(counts)),
                    "rsdsfm_denoise_video_dev")
        return _wanted(ns, counts=counts)


# ---------------------------------------------------------------------------------------------------
# the spatial top-up: a single-frame patch-weighted mean in proportion to what the temporal denoise did not give (include/rsdsfm_denoise_spatial.h)
# ---------------------------------------------------------------------------------------------------
DENOISE_SPATIAL_HEADER_PATH = _header_path("rsdsfm_denoise_spatial.h")
DENOISE_SPATIAL_SEARCH_MAX = 3


def denoise_spatial_declared_symbols():
    """Names of every function include/rsdsfm_denoise_spatial.h declares"""
    return _declared("rsdsfm_denoise_spatial.h")


class DenoiseSpatialParams(C.Structure):
    _fields_ = [("strength", C.c_int32), ("target", C.c_int32), ("search", C.c_int32), ("struct_bytes", C.c_int32), ("reserved", C.c_int32 * 4)]


def _denoise_spatial_params(strength=None, target=None, search=None):
    """a DenoiseSpatialParams with the given values over the defaults (None: the default)"""
    return _params(DenoiseSpatialParams, "rsdsfm_denoise_spatial_params_init", strength=strength, target=target, search=search)


def denoise_spatial_default_params():
    """the top-up's defaults as a dict: strength = 12, target = 80, search = 2 (rsdsfm_denoise_spatial_params_init); choices, not measurements"""
    p = _denoise_spatial_params()
    return dict(strength=p.strength, target=p.target, search=p.search)


def denoise_spatial_launches():
    """kernel launches of one denoise_spatial_dev call: 1 (rsdsfm_denoise_spatial_launches; host only)"""
    return int(load_library().rsdsfm_denoise_spatial_launches())


def denoise_spatial_frame_launches(rows, cols, nsrc):
    """kernel launches of one denoise_spatial_frame_dev call: denoise_launches + 1 (rsdsfm_denoise_spatial_frame_launches; host only)"""
    return _launches("rsdsfm_denoise_spatial_frame_launches", "rows and cols in [2, 16384], nsrc in [1, 15]", rows, cols, nsrc)


@_solver_methods
class _DenoiseSpatialMixin:
    def denoise_spatial_dev(self, d_image, d_mask, d_weight, channels, rows, cols, d_image_out, d_support=None, d_counts3=None, strength=0, target=0, search=0):
        """the spatial top-up (rsdsfm_denoise_spatial_dev; tests/denoise_spatial_spec_numpy.py): every set pixel whose weight n (d_weight; None: 16)
        is below `target` is mixed with the patch-weighted mean of its set neighbours within [-search, search]^2 of its own frame, in
        proportion to target - n; a pixel at or above the target keeps its bytes.  The support to d_support, [unset, kept, smoothed] to d_counts3
        (three device int64).  0: the default (strength 12, target 80, search 2).  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_denoise_spatial_dev(self._ctx, _dp(d_image), _dp(d_mask), _np0(d_weight), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols),
                                                        C.c_int32(strength), C.c_int32(target), C.c_int32(search), _dp(d_image_out), _np0(d_support), _np0(d_counts3)),
                    "rsdsfm_denoise_spatial_dev")

    def denoise_spatial(self, image, mask, weight=None, strength=0, target=0, search=0, device=0):
        """host convenience around denoise_spatial_dev: image (rows, cols[, 3]) uint8, mask and weight (or None) (rows, cols) uint8
        -> (image, support (rows, cols) uint8, counts (3,) int64 [unset, kept, smoothed])"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        with _Staging(self, device) as st:
            d_i, d_m, d_w = st.up(image), st.up(mask, np.uint8), st.up(weight, np.uint8)
            d_out, d_sup, d_cnt = st.empty_like(d_i), st.empty((rows, cols)), st.zeros(3, "int64")
            st.ready()
            self.denoise_spatial_dev(d_i.data_ptr(), d_m.data_ptr(), d_w.data_ptr() if d_w is not None else None, ch, rows, cols, d_out.data_ptr(), d_sup.data_ptr(),
                                     d_cnt.data_ptr(), strength, target, search)
            return st.down(d_out, d_sup, d_cnt)
    def denoise_spatial_frame_dev(self, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_weight=None, d_support=None, d_counts6=None,
                                  strength=None, gain=True, min_overlap=None, window=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT,
                                  iterations=0, params=None, spatial_strength=None, target=None, search=None, spatial_params=None):
        """one frame through the temporal denoise and the top-up (rsdsfm_denoise_spatial_frame_dev): denoise_frame_dev's arguments; the temporal
        result stays in the context's workspace (its weight in d_weight when given, its mask in d_mask, its counters in d_counts6[0 .. 2]) and
        denoise_spatial_dev reads it into d_image, d_support and d_counts6[3 .. 5].  params / spatial_params: a DenoiseParams / DenoiseSpatialParams
        passed as it is instead of the keywords.  Enqueued on the context's stream."""
        ns, Mm, mm = _frame_front("denoise_spatial_frame_dev", d_images, M, m, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
        dp = params if params is not None else _denoise_params(None, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
        sp = spatial_params if spatial_params is not None else _denoise_spatial_params(spatial_strength, target, search)
        self._check(self.lib.rsdsfm_denoise_spatial_frame_dev(self._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns),
                                                              *_k4(K), C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns), _p(Mm),
                                                              _p(mm), C.byref(dp), C.byref(sp), _window4(window), _dp(d_image), _dp(d_mask), _np0(d_weight), _np0(d_support),
                                                              _np0(d_counts6)), "rsdsfm_denoise_spatial_frame_dev")

    def denoise_spatial_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_weights=None,
                                  d_out_supports=None, want_counts=True, radius=None, strength=None, gain=True, min_overlap=None, window=None, occlusion=False,
                                  occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, spatial_strength=None, target=None, search=None):
        """a solved clip through the temporal denoise and the top-up (rsdsfm_denoise_spatial_video_dev): denoise_video_dev's clip and walk,
        denoise_spatial_frame_dev per frame into d_out[q], d_out_masks[q], d_out_weights[q], d_out_supports[q].  Returns dict(); with want_counts
        counts (nsources, 6) int64 [unset, own only, averaged, unset, kept, smoothed] -- the call then waits."""
        ns, a, cc, ap, cp, sc = _clip_front("denoise_spatial_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out,
                d_out_masks=d_out_masks, d_out_weights=d_out_weights, d_out_supports=d_out_supports)
        dp = _denoise_params(radius, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
        sp = _denoise_spatial_params(spatial_strength, target, search)
        counts = _counts(want_counts, ns, 6)
        self._check(self.lib.rsdsfm_denoise_spatial_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                              _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode),
                                                              int(q5_mode), C.c_int32(iterations), C.byref(dp), C.byref(sp), _window4(window), _ptrs(d_out, ns), _ptrs(d_out_masks, ns),
                                                              _ptrs(d_out_weights, ns), _ptrs(d_out_supports, ns), _p(counts)), "rsdsfm_denoise_spatial_video_dev")
        return _wanted(ns, counts=counts)


# ---------------------------------------------------------------------------------------------------
# the noise level: a frame's noise measured from the frame, and the two denoisers at the strength it asks for (include/rsdsfm_noise.h)
# ---------------------------------------------------------------------------------------------------
NOISE_HEADER_PATH = _header_path("rsdsfm_noise.h")
NOISE_BINS = 1024


def noise_declared_symbols():
    """Names of every function include/rsdsfm_noise.h declares"""
    return _declared("rsdsfm_noise.h")


class NoiseParams(C.Structure):
    _fields_ = [("quantile_q8", C.c_int32), ("scale", C.c_int32), ("struct_bytes", C.c_int32), ("reserved0", C.c_int32), ("min_samples", C.c_int64),
                ("reserved", C.c_int32 * 4)]


def _noise_params(quantile_q8=None, scale=None, min_samples=None):
    """a NoiseParams with the given values over the defaults (None: the default)"""
    return _params(NoiseParams, "rsdsfm_noise_params_init", quantile_q8=quantile_q8, scale=scale, min_samples=min_samples)


def noise_default_params():
    """the noise level's defaults as a dict: quantile_q8 = 128 (the median; a choice, not a measurement), scale = 12, min_samples = 1024
    (rsdsfm_noise_params_init)"""
    p = _noise_params()
    return dict(quantile_q8=p.quantile_q8, scale=p.scale, min_samples=p.min_samples)


def noise_level_launches():
    """kernel launches of one noise_level_dev call: 2 (rsdsfm_noise_level_launches; host only)"""
    return int(load_library().rsdsfm_noise_level_launches())


def noise_strength(n, m, scale=0, fallback=0, min_samples=0):
    """the strength h a record [n, m, ...] asks for (rsdsfm_noise_strength; tests/noise_spec_numpy.py; host only): fallback (0: 12) where
    n < min_samples (0: 1024), else clamp((scale m + 8) >> 4, 1, 255) (scale 0: 12)"""
    h = load_library().rsdsfm_noise_strength(C.c_int64(int(n)), C.c_int64(int(m)), C.c_int32(scale), C.c_int32(fallback), C.c_int64(min_samples))
    if h < 0:
        raise RsdsfmError("rsdsfm_noise_strength failed (%d): n, m >= 0, scale in [0, 255], fallback in [0, 255], min_samples >= 0" % h)
    return int(h)


def denoise_auto_frame_launches(rows, cols, nsrc, with_spatial=False):
    """kernel launches of one denoise_auto_frame_dev call: denoise_launches + 2, + 1 with the top-up (rsdsfm_denoise_auto_frame_launches; host only)"""
    return _launches("rsdsfm_denoise_auto_frame_launches", "rows and cols in [2, 16384], nsrc in [1, 15]", rows, cols, nsrc, 1 if with_spatial else 0)


@_solver_methods
class _NoiseMixin:
    def noise_level_dev(self, d_image, d_mask, channels, rows, cols, d_hist1024, d_record4, quantile_q8=0):
        """a frame's noise level (rsdsfm_noise_level_dev; tests/noise_spec_numpy.py): the histogram of |K * I| over the unclipped samples under
        the mask into d_hist1024 (1024 device uint32) and [n, m, sigma_q8, 0] into d_record4 (four device uint64), m the quantile_q8 / 256
        quantile (0: 128, the median).  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_noise_level_dev(self._ctx, _dp(d_image), _dp(d_mask), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols), C.c_int32(quantile_q8),
                                                    _dp(d_hist1024), _dp(d_record4)), "rsdsfm_noise_level_dev")

    def noise_level(self, image, mask, quantile_q8=0, device=0):
        """host convenience around noise_level_dev: image (rows, cols[, 3]) uint8, mask (rows, cols) uint8
        -> dict(hist (1024,) uint32, record (4,) uint64 [n, m, sigma_q8, 0], sigma: the record's sigma in grey levels)"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        with _Staging(self, device) as st:
            d_i, d_m = st.up(image), st.up(mask, np.uint8)
            d_h, d_r = st.empty(NOISE_BINS, "int32"), st.empty(4, "int64")
            st.ready()
            self.noise_level_dev(d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_h.data_ptr(), d_r.data_ptr(), quantile_q8)
            hist, record = st.down(d_h, d_r)
            record = record.view(np.uint64)
            return dict(hist=hist.view(np.uint32), record=record, sigma=int(record[2]) / 256.0)
    def denoise_accumulate_auto_dev(self, d_ref, d_ref_mask, d_layer, d_layer_mask, channels, rows, cols, d_cells, first, last, d_noise4, d_sums8=None, min_overlap=0,
                                    gain_mode=0, strength=0, scale=0, min_samples=0, d_image_out=None, d_mask_out=None, d_weight=None, d_counts3=None):
        """denoise_accumulate_dev at the strength the record d_noise4 (four device uint64, noise_level_dev's) asks for, formed on the device
        (rsdsfm_denoise_accumulate_auto_dev): `strength` is the fallback where the record has fewer than min_samples samples.  Enqueued on the
        context's stream."""
        self._check(self.lib.rsdsfm_denoise_accumulate_auto_dev(self._ctx, _dp(d_ref), _dp(d_ref_mask), _np0(d_layer), _np0(d_layer_mask), C.c_int32(channels), C.c_int32(rows),
                                                                C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode), C.c_int32(strength), _np0(d_noise4),
                                                                C.c_int32(scale), C.c_int64(min_samples), _np0(d_cells), C.c_int32(int(first)), C.c_int32(int(last)),
                                                                _np0(d_image_out), _np0(d_mask_out), _np0(d_weight), _np0(d_counts3)), "rsdsfm_denoise_accumulate_auto_dev")

    def denoise_accumulate_auto(self, ref, ref_mask, layers, record4, records=None, min_overlap=0, gain_mode=0, strength=0, scale=0, min_samples=0, device=0):
        """host convenience around denoise_accumulate_auto_dev: denoise_accumulate's arguments with record4, a noise record (4,) uint64
        -> (image, mask, weight (rows, cols) uint8, counts (3,) int64 [unset, own only, averaged])"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        ch = 1 if ref.ndim == 2 else ref.shape[2]
        with _Staging(self, device) as st:
            d_ref, d_rm, d_n = st.up(ref), st.up(ref_mask, np.uint8), st.up64(record4)
            d_l = [(st.up(i, np.uint8), st.up(m, np.uint8)) for i, m in layers]
            d_rec = [None if records is None or records[j] is None else st.up64(records[j]) for j in range(len(layers))]
            d_cells = st.empty((rows, cols, ch + 1), "int16")
            d_out, d_mask = st.empty_like(d_ref), st.empty((rows, cols))
            d_w, d_cnt = st.empty_like(d_mask), st.zeros(3, "int64")
            st.ready()
            kw = dict(min_overlap=min_overlap, gain_mode=gain_mode, strength=strength, scale=scale, min_samples=min_samples, d_image_out=d_out.data_ptr(),
                      d_mask_out=d_mask.data_ptr(), d_weight=d_w.data_ptr(), d_counts3=d_cnt.data_ptr())
            if not d_l:
                self.denoise_accumulate_auto_dev(d_ref.data_ptr(), d_rm.data_ptr(), None, None, ch, rows, cols, None, True, True, d_n.data_ptr(), None, **kw)
            for j, (d_i, d_m) in enumerate(d_l):
                self.denoise_accumulate_auto_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == len(d_l) - 1,
                                                 d_n.data_ptr(), d_rec[j].data_ptr() if d_rec[j] is not None else None, **kw)
            return st.down(d_out, d_mask, d_w, d_cnt)
    def denoise_spatial_auto_dev(self, d_image, d_mask, d_weight, channels, rows, cols, d_noise4, d_image_out, d_support=None, d_counts3=None, strength=0, scale=0,
                                 min_samples=0, target=0, search=0):
        """denoise_spatial_dev at the strength the record d_noise4 asks for, formed on the device (rsdsfm_denoise_spatial_auto_dev): `strength` is
        the fallback.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_denoise_spatial_auto_dev(self._ctx, _dp(d_image), _dp(d_mask), _np0(d_weight), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols),
                                                             C.c_int32(strength), _np0(d_noise4), C.c_int32(scale), C.c_int64(min_samples), C.c_int32(target), C.c_int32(search),
                                                             _dp(d_image_out), _np0(d_support), _np0(d_counts3)), "rsdsfm_denoise_spatial_auto_dev")

    def denoise_spatial_auto(self, image, mask, record4, weight=None, strength=0, scale=0, min_samples=0, target=0, search=0, device=0):
        """host convenience around denoise_spatial_auto_dev: denoise_spatial's arguments with record4, a noise record (4,) uint64
        -> (image, support (rows, cols) uint8, counts (3,) int64 [unset, kept, smoothed])"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        with _Staging(self, device) as st:
            d_i, d_m, d_w, d_n = st.up(image), st.up(mask, np.uint8), st.up(weight, np.uint8), st.up64(record4)
            d_out, d_sup, d_cnt = st.empty_like(d_i), st.empty((rows, cols)), st.zeros(3, "int64")
            st.ready()
            self.denoise_spatial_auto_dev(d_i.data_ptr(), d_m.data_ptr(), d_w.data_ptr() if d_w is not None else None, ch, rows, cols, d_n.data_ptr(), d_out.data_ptr(),
                                          d_sup.data_ptr(), d_cnt.data_ptr(), strength, scale, min_samples, target, search)
            return st.down(d_out, d_sup, d_cnt)
    def denoise_auto_frame_dev(self, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_weight=None, d_support=None, d_counts6=None,
                               d_noise4=None, strength=None, gain=True, min_overlap=None, window=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS,
                               q5_mode=Q5_COMPAT, iterations=0, params=None, quantile_q8=None, scale=None, min_samples=None, noise_params=None, spatial=False,
                               spatial_strength=None, target=None, search=None, spatial_params=None):
        """one frame denoised at the strength its own noise asks for (rsdsfm_denoise_auto_frame_dev): denoise_frame_dev's arguments; the rendered
        own frame is measured (noise_level_dev), every neighbour goes through denoise_accumulate_auto_dev, and with spatial (or spatial_params)
        denoise_spatial_auto_dev follows on the same record.  `strength` and `spatial_strength` are the fallbacks.  d_counts6: six device int64
        [unset, own only, averaged, unset, kept, smoothed]; d_noise4: four device uint64 for the record.  Enqueued on the context's stream."""
        ns, Mm, mm = _frame_front("denoise_auto_frame_dev", d_images, M, m, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
        dp = params if params is not None else _denoise_params(None, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
        npar = noise_params if noise_params is not None else _noise_params(quantile_q8, scale, min_samples)
        sp = spatial_params if spatial_params is not None else (_denoise_spatial_params(spatial_strength, target, search) if spatial else None)
        self._check(self.lib.rsdsfm_denoise_auto_frame_dev(self._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), *_k4(K),
                                                           C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns), _p(Mm),
                                                           _p(mm), C.byref(dp), C.byref(npar), _ref(sp), _window4(window), _dp(d_image),
                                                           _dp(d_mask), _np0(d_weight), _np0(d_support), _np0(d_counts6), _np0(d_noise4)), "rsdsfm_denoise_auto_frame_dev")

    def denoise_auto_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_weights=None,
                               d_out_supports=None, want_counts=True, want_noise=True, radius=None, strength=None, gain=True, min_overlap=None, window=None,
                               occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, quantile_q8=None, scale=None, min_samples=None,
                               spatial=False, spatial_strength=None, target=None, search=None):
        """a solved clip denoised at every frame's own strength (rsdsfm_denoise_auto_video_dev): denoise_video_dev's clip and walk,
        denoise_auto_frame_dev per frame.  Returns dict(); with want_counts counts (nsources, 6) int64, with want_noise noise (nsources, 4)
        uint64 [n, m, sigma_q8, 0] -- with either the call waits."""
        ns, a, cc, ap, cp, sc = _clip_front("denoise_auto_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out,
                d_out_masks=d_out_masks, d_out_weights=d_out_weights, d_out_supports=d_out_supports)
        dp = _denoise_params(radius, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
        npar = _noise_params(quantile_q8, scale, min_samples)
        sp = _denoise_spatial_params(spatial_strength, target, search) if spatial else None
        counts = _counts(want_counts, ns, 6)
        noise = _counts(want_noise, ns, 4, dtype=np.uint64)
        self._check(self.lib.rsdsfm_denoise_auto_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                           _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode), int(q5_mode),
                                                           C.c_int32(iterations), C.byref(dp), C.byref(npar), _ref(sp), _window4(window),
                                                           _ptrs(d_out, ns), _ptrs(d_out_masks, ns), _ptrs(d_out_weights, ns), _ptrs(d_out_supports, ns), _p(counts), _p(noise)),
                    "rsdsfm_denoise_auto_video_dev")
        return _wanted(ns, counts=counts, noise=noise)


# ---------------------------------------------------------------------------------------------------
# the multi-frame super-resolution: a frame on a grid S times finer, merged from its registered neighbours (include/rsdsfm_superres.h)
# ---------------------------------------------------------------------------------------------------
SUPERRES_HEADER_PATH = _header_path("rsdsfm_superres.h")
SUPERRES_SCALE_MAX = 4
SUPERRES_RADIUS_MAX = 7
SUPERRES_LAYERS_MAX = 14
SUPERRES_PROX_MAX = 16


class SuperresParams(C.Structure):
    _fields_ = [("scale", C.c_int32), ("radius", C.c_int32), ("strength", C.c_int32), ("gain_mode", C.c_int32), ("min_overlap", C.c_int64), ("struct_bytes", C.c_int32),
                ("reserved", C.c_int32 * 5)]


def superres_declared_symbols():
    """Names of every function include/rsdsfm_superres.h declares"""
    return _declared("rsdsfm_superres.h")


def _superres_params(scale=None, radius=None, strength=None, gain=True, min_overlap=None):
    """a SuperresParams with the given values over the defaults (None: the default)"""
    return _params(SuperresParams, "rsdsfm_superres_params_init", scale=scale, radius=radius, strength=strength, min_overlap=min_overlap, gain_mode=0 if gain else 1)


def superres_default_params():
    """the super-resolution's defaults as a dict: scale = 2, radius = 2, strength = 12, min_overlap = 1024 (rsdsfm_superres_params_init); choices,
    not measurements"""
    p = _superres_params()
    return dict(scale=p.scale, radius=p.radius, strength=p.strength, min_overlap=p.min_overlap, gain_mode=p.gain_mode)


def superres_render_launches(rows, cols, scale):
    """kernel launches of one superres_render_dev call: stabilize_window_launches(rows, cols) (rsdsfm_superres_render_launches; host only)"""
    return _launches("rsdsfm_superres_render_launches", "rows and cols in [2, 16384], scale in [1, 4], scale * size at most 16384", rows, cols, scale)


def superres_accumulate_launches():
    """kernel launches of one superres_accumulate_dev call: 1 (rsdsfm_superres_accumulate_launches; host only)"""
    return int(load_library().rsdsfm_superres_accumulate_launches())


def superres_launches(rows, cols, scale, nsrc):
    """kernel launches of one superres_frame_dev call on nsrc sources of rows x cols: nsrc superres_render_launches + 2 (nsrc - 1), or + 1 with one
    source (rsdsfm_superres_launches; host only)"""
    return _launches("rsdsfm_superres_launches", "rows and cols in [2, 16384], scale in [1, 4], scale * size at most 16384, nsrc in [1, 15]", rows, cols, scale, nsrc)


@_solver_methods
class _SuperresMixin:
    def superres_render_dev(self, d_image, channels, d_depth_map, d_R, d_t, K, rows, cols, M, m, scale, d_bil, d_near, d_prox, d_valid=None, window=None,
                            mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """one source rendered alone onto a grid `scale` times finer (rsdsfm_superres_render_dev; tests/superres_spec_numpy.py): d_bil and d_near
        (scale rows x scale cols x channels) the bilinear and the nearest source sample of every fine pixel, d_prox (scale rows x scale cols) how
        near the nearest fell, 1 .. 16, 0 where the pixel is not valid; d_valid (optional) 1 where d_prox is not 0.  Every byte is written.
        Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_superres_render_dev(self._ctx, _dp(d_image), C.c_int32(channels), _dp(d_depth_map), _dp(d_R), _dp(d_t), *_k4(K), C.c_int32(rows),
                                                        C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), _p(_f64(M).reshape(-1)),
                                                        _p(_f64(m).reshape(-1)), C.c_int32(scale), _window4(window), _np0(d_bil), _np0(d_near), _np0(d_prox), _np0(d_valid)),
                    "rsdsfm_superres_render_dev")

    def superres_render(self, image, depth, R, t, K, M, m, scale=2, window=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, device=0):
        """host convenience around superres_render_dev: image (rows, cols[, 3]) uint8, depth (rows, cols), R (rows, 9 or 3, 3), t (rows, 3)
        -> dict(bil, near, prox, valid) of host arrays on the fine grid"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        rows, cols = image.shape[:2]
        ch = 1 if image.ndim == 2 else image.shape[2]
        with _Staging(self, device) as st:
            d_i, d_z, d_R, d_t = st.up_frame(image, depth, R, t)
            fine = (scale * rows, scale * cols)
            d_b = st.empty(fine + image.shape[2:])
            d_n, d_q, d_v = st.empty_like(d_b), st.empty(fine), st.empty(fine)
            st.ready()
            self.superres_render_dev(d_i.data_ptr(), ch, d_z.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, M, m, scale, d_b.data_ptr(), d_n.data_ptr(),
                                     d_q.data_ptr(), d_v.data_ptr(), window, mode, q5_mode, iterations)
            return dict(zip(("bil", "near", "prox", "valid"), st.down(d_b, d_n, d_q, d_v)))
    def superres_accumulate_dev(self, d_ref, d_ref_near, d_ref_prox, d_layer, d_layer_near, d_layer_prox, channels, rows, cols, d_cells, first, last, d_sums8=None,
                                min_overlap=0, gain_mode=0, strength=0, d_image_out=None, d_mask_out=None, d_weight=None, d_counts3=None):
        """one layer accumulated onto the cells (rsdsfm_superres_accumulate_dev; tests/superres_spec_numpy.py) on FINE planes of rows x cols: the
        layer's nearest samples weighted by the denoise's 3 x 3 patch weight (taken on the bilinear planes) times the layer's proximity.  The
        three layer pointers None: no layer (first and last).  d_sums8: the layer's record (seam_overlap_sums_dev), None: no gain.  first: the
        cells are set from the reference's nearest samples and proximity; last: the cells are not written, the merged pixel goes to d_image_out
        (the reference's bilinear sample where no layer contributed), 1 to d_mask_out where anything counted, the summed weight to d_weight and
        [unset, own only, merged] to d_counts3 (three device int64).  At most 14 layers.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_superres_accumulate_dev(self._ctx, _dp(d_ref), _dp(d_ref_near), _dp(d_ref_prox), _np0(d_layer), _np0(d_layer_near), _np0(d_layer_prox),
                                                            C.c_int32(channels), C.c_int32(rows), C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode),
                                                            C.c_int32(strength), _np0(d_cells), C.c_int32(int(first)), C.c_int32(int(last)), _np0(d_image_out),
                                                            _np0(d_mask_out), _np0(d_weight), _np0(d_counts3)), "rsdsfm_superres_accumulate_dev")

    def superres_accumulate(self, ref, ref_near, ref_prox, layers, records=None, min_overlap=0, gain_mode=0, strength=0, device=0):
        """host convenience around superres_accumulate_dev: the reference's (bil, near, prox), layers a list of 0 .. 14 (bil, near, prox) triples of
        host arrays on the fine grid, records None or one 8-word record (or None) per layer
        -> (image, mask, weight (rows, cols) uint8, counts (3,) int64 [unset, own only, merged])"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        ch = 1 if ref.ndim == 2 else ref.shape[2]
        with _Staging(self, device) as st:
            d_ref, d_rn, d_rq = st.up(ref), st.up(ref_near, np.uint8), st.up(ref_prox, np.uint8)
            d_l = [(st.up(b, np.uint8), st.up(n, np.uint8), st.up(q, np.uint8)) for b, n, q in layers]
            d_rec = [None if records is None or records[j] is None else st.up64(records[j]) for j in range(len(layers))]
            d_cells = st.empty((rows, cols, ch + 1), "int16")
            d_out, d_mask = st.empty_like(d_ref), st.empty((rows, cols))
            d_w, d_cnt = st.empty_like(d_mask), st.zeros(3, "int64")
            st.ready()
            outs = dict(d_image_out=d_out.data_ptr(), d_mask_out=d_mask.data_ptr(), d_weight=d_w.data_ptr(), d_counts3=d_cnt.data_ptr())
            ref_ptrs = (d_ref.data_ptr(), d_rn.data_ptr(), d_rq.data_ptr())
            if not d_l:
                self.superres_accumulate_dev(*ref_ptrs, None, None, None, ch, rows, cols, None, True, True, None, min_overlap, gain_mode, strength, **outs)
            for j, (d_b, d_n, d_q) in enumerate(d_l):
                self.superres_accumulate_dev(*ref_ptrs, d_b.data_ptr(), d_n.data_ptr(), d_q.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == len(d_l) - 1,
                                             d_rec[j].data_ptr() if d_rec[j] is not None else None, min_overlap, gain_mode, strength, **outs)
            return st.down(d_out, d_mask, d_w, d_cnt)
    def superres_frame_dev(self, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_weight=None, d_counts3=None, scale=None, strength=None,
                           gain=True, min_overlap=None, window=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, params=None):
        """one super-resolved frame (rsdsfm_superres_frame_dev): d_images, d_depth_maps, d_R, d_t lists of 1 .. 15 device pointers of rows x cols
        sources, source 0 the own frame and the others its neighbours; M (nsrc, 3, 3), m (nsrc, 3) every source's pose in the target camera.
        Every source through superres_render_dev, per neighbour seam_overlap_sums_dev and superres_accumulate_dev; the merged frame into d_image
        (scale rows x scale cols x channels), d_mask, d_weight (scale rows x scale cols), d_counts3.  params: a SuperresParams passed as it is
        instead of the keywords.  Enqueued on the context's stream."""
        ns, Mm, mm = _frame_front("superres_frame_dev", d_images, M, m, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
        sp = params if params is not None else _superres_params(scale, None, strength, gain, min_overlap)
        self._check(self.lib.rsdsfm_superres_frame_dev(self._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), *_k4(K),
                                                       C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns), _p(Mm), _p(mm),
                                                       C.byref(sp), _window4(window), _dp(d_image), _dp(d_mask), _np0(d_weight), _np0(d_counts3)), "rsdsfm_superres_frame_dev")

    def superres_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_weights=None,
                           want_counts=True, scale=None, radius=None, strength=None, gain=True, min_overlap=None, window=None, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT,
                           iterations=0):
        """a solved clip super-resolved (rsdsfm_superres_video_dev): the clip as denoise_video_dev takes it and walks it; for every frame q the
        own pose by retime_poses(t = q), the neighbours within `radius` (None: 2) by neighbour_poses on the same path, and superres_frame_dev
        into d_out[q], d_out_masks[q], d_out_weights[q] (planes `scale` (None: 2) times finer than the frames).  Returns dict(); with want_counts
        counts (nsources, 3) int64 [unset, own only, merged] -- the call then waits."""
        ns, a, cc, ap, cp, sc = _clip_front("superres_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out,
                d_out_masks=d_out_masks, d_out_weights=d_out_weights)
        sp = _superres_params(scale, radius, strength, gain, min_overlap)
        counts = _counts(want_counts, ns, 3)
        self._check(self.lib.rsdsfm_superres_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                       _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode), int(q5_mode),
                                                       C.c_int32(iterations), C.byref(sp), _window4(window), _ptrs(d_out, ns), _ptrs(d_out_masks, ns), _ptrs(d_out_weights, ns), _p(counts)),
                    "rsdsfm_superres_video_dev")
        return _wanted(ns, counts=counts)


# ---------------------------------------------------------------------------------------------------
# the clean plate: the per-pixel median of a frame and its registered neighbours, and a moving flag (include/rsdsfm_plate.h)
# ---------------------------------------------------------------------------------------------------
PLATE_HEADER_PATH = _header_path("rsdsfm_plate.h")
PLATE_RADIUS_MAX = 7
PLATE_LAYERS_MAX = 14
PLATE_UNSET, PLATE_STATIC, PLATE_MOVING, PLATE_UNDECIDED = 0, 1, 2, 3  # the flag plane's bytes and the counters' order


class PlateParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("threshold", C.c_int32), ("min_votes", C.c_int32), ("gain_mode", C.c_int32), ("occlusion", C.c_int32),
                ("occlusion_tol_q16", C.c_int32), ("struct_bytes", C.c_int32), ("reserved0", C.c_int32), ("min_overlap", C.c_int64), ("reserved", C.c_int32 * 4)]


def plate_declared_symbols():
    """Names of every function include/rsdsfm_plate.h declares"""
    return _declared("rsdsfm_plate.h")


def _plate_params(radius=None, threshold=None, min_votes=None, gain=True, occlusion=False, occlusion_tol_q16=0, min_overlap=None):
    """a PlateParams with the given values over the defaults (None: the default)"""
    return _params(PlateParams, "rsdsfm_plate_params_init", radius=radius, threshold=threshold, min_votes=min_votes, min_overlap=min_overlap, gain_mode=0 if gain else 1,
                   occlusion=occlusion, occlusion_tol_q16=occlusion_tol_q16)


def plate_default_params():
    """the plate's defaults as a dict: radius = 2, threshold = 24, min_votes = 3, min_overlap = 1024 (rsdsfm_plate_params_init); choices, not
    measurements"""
    p = _plate_params()
    return dict(radius=p.radius, threshold=p.threshold, min_votes=p.min_votes, min_overlap=p.min_overlap, gain_mode=p.gain_mode, occlusion=p.occlusion)


def plate_launches(rows, cols, nsrc):
    """kernel launches of one plate_frame_dev call on nsrc sources: nsrc stabilize_window_launches + (nsrc - 1) + 1 (rsdsfm_plate_launches; host
    only)"""
    return _launches("rsdsfm_plate_launches", "rows and cols in [2, 16384], nsrc in [1, 15]", rows, cols, nsrc)


def plate_median_launches():
    """kernel launches of one plate_median_dev call: 1 (rsdsfm_plate_median_launches; host only)"""
    return int(load_library().rsdsfm_plate_median_launches())


@_solver_methods
class _PlateMixin:
    def plate_median_dev(self, d_ref, d_ref_mask, d_layers, d_layer_masks, channels, rows, cols, d_image_out, d_mask_out, d_votes=None, d_moving=None, d_counts4=None,
                         d_sums8=None, min_overlap=0, gain_mode=0, threshold=0, min_votes=0, nlayers=None):
        """the per-pixel, per-channel lower median of the reference and 0 .. 14 layers (rsdsfm_plate_median_dev; tests/plate_spec_numpy.py):
        d_layers, d_layer_masks lists of device pointers (None: no layers), d_sums8 the layers' records, nlayers x 8 device uint64 (None: no
        gain).  The plate into d_image_out, 1 into d_mask_out where anything voted, the number of candidates into d_votes, the flag 0 unset /
        1 static / 2 moving / 3 undecided into d_moving and the four counts into d_counts4 (four device int64).  One launch, enqueued on the
        context's stream."""
        self._plate_estimator_dev("rsdsfm_plate_median_dev", d_ref, d_ref_mask, d_layers, d_layer_masks, channels, rows, cols, d_image_out, d_mask_out, d_votes, d_moving,
                                  d_counts4, d_sums8, min_overlap, gain_mode, threshold, min_votes, nlayers)

    def _plate_estimator_dev(self, name, d_ref, d_ref_mask, d_layers, d_layer_masks, channels, rows, cols, d_image_out, d_mask_out, d_votes, d_moving, d_counts4, d_sums8,
                             min_overlap, gain_mode, threshold, min_votes, nlayers):
        """rsdsfm_plate_median_dev or rsdsfm_plate_medoid_dev: one signature"""
        n = (len(d_layers) if d_layers is not None else 0) if nlayers is None else int(nlayers)
        self._check(getattr(self.lib, name)(self._ctx, _dp(d_ref), _dp(d_ref_mask), _ptrs(d_layers or None), _ptrs(d_layer_masks or None), C.c_int32(n), C.c_int32(channels), C.c_int32(rows),
                                            C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode), C.c_int32(threshold), C.c_int32(min_votes),
                                            _np0(d_image_out), _np0(d_mask_out), _np0(d_votes), _np0(d_moving), _np0(d_counts4)), name)

    def plate_median(self, ref, ref_mask, layers, records=None, min_overlap=0, gain_mode=0, threshold=0, min_votes=0, device=0):
        """host convenience around plate_median_dev: the reference (image, mask), layers a list of 0 .. 14 (image, mask) pairs of host arrays,
        records None or (nlayers, 8) uint64
        -> (image, mask, votes, moving (rows, cols) uint8, counts (4,) int64 [unset, static, moving, undecided])"""
        return self._plate_estimator(self.plate_median_dev, ref, ref_mask, layers, records, min_overlap, gain_mode, threshold, min_votes, device)

    def _plate_estimator(self, call_dev, ref, ref_mask, layers, records, min_overlap, gain_mode, threshold, min_votes, device):
        """plate_median's and plate_medoid's upload, call and download"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        ch = 1 if ref.ndim == 2 else ref.shape[2]
        with _Staging(self, device) as st:
            d_ref, d_rm = st.up(ref), st.up(ref_mask, np.uint8)
            d_l = [(st.up(i, np.uint8), st.up(m, np.uint8)) for i, m in layers]
            d_rec = None
            if records is not None and len(layers):
                d_rec = st.up64(np.ascontiguousarray(records, dtype=np.uint64).reshape(len(layers), 8))
            d_out, d_mask = st.empty_like(d_ref), st.empty((rows, cols))
            d_v, d_f, d_cnt = st.empty_like(d_mask), st.empty_like(d_mask), st.zeros(4, "int64")
            st.ready()
            call_dev(d_ref.data_ptr(), d_rm.data_ptr(), [i.data_ptr() for i, _ in d_l], [m.data_ptr() for _, m in d_l], ch, rows, cols, d_out.data_ptr(), d_mask.data_ptr(),
                     d_v.data_ptr(), d_f.data_ptr(), d_cnt.data_ptr(), d_rec.data_ptr() if d_rec is not None else None, min_overlap, gain_mode, threshold, min_votes)
            return st.down(d_out, d_mask, d_v, d_f, d_cnt)
    def plate_frame_dev(self, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_votes=None, d_moving=None, d_counts4=None, threshold=None,
                        min_votes=None, gain=True, min_overlap=None, window=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0,
                        params=None):
        """one clean plate (rsdsfm_plate_frame_dev): d_images, d_depth_maps, d_R, d_t lists of 1 .. 15 device pointers, source 0 the own frame
        and the others its neighbours; M (nsrc, 3, 3), m (nsrc, 3) every source's pose in the target camera.  The own frame through
        stabilize_window_frame_dev, every neighbour alone on its own layer of the context's stack with its record by seam_overlap_sums_dev, one
        plate_median_dev into d_image, d_mask, d_votes, d_moving, d_counts4.  params: a PlateParams passed as it is instead of the keywords.
        Enqueued on the context's stream."""
        ns, Mm, mm = _frame_front("plate_frame_dev", d_images, M, m, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
        pp = params if params is not None else _plate_params(None, threshold, min_votes, gain, occlusion, occlusion_tol_q16, min_overlap)
        self._check(self.lib.rsdsfm_plate_frame_dev(self._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), *_k4(K),
                                                    C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns), _p(Mm), _p(mm),
                                                    C.byref(pp), _window4(window), _dp(d_image), _dp(d_mask), _np0(d_votes), _np0(d_moving), _np0(d_counts4)),
                    "rsdsfm_plate_frame_dev")

    def plate_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_votes=None,
                        d_out_moving=None, want_counts=True, radius=None, threshold=None, min_votes=None, gain=True, min_overlap=None, window=None, occlusion=False,
                        occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """a solved clip's plates (rsdsfm_plate_video_dev): the clip as denoise_video_dev takes it and walks it; for every frame q the own pose
        by retime_poses(t = q), the neighbours within `radius` (None: 2) by neighbour_poses on the same path, and plate_frame_dev into d_out[q],
        d_out_masks[q], d_out_votes[q], d_out_moving[q].  Returns dict(); with want_counts counts (nsources, 4) int64 [unset, static, moving,
        undecided] -- the call then waits."""
        ns, a, cc, ap, cp, sc = _clip_front("plate_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out,
                d_out_masks=d_out_masks, d_out_votes=d_out_votes, d_out_moving=d_out_moving)
        pp = _plate_params(radius, threshold, min_votes, gain, occlusion, occlusion_tol_q16, min_overlap)
        counts = _counts(want_counts, ns, 4)
        self._check(self.lib.rsdsfm_plate_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                    _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode), int(q5_mode),
                                                    C.c_int32(iterations), C.byref(pp), _window4(window), _ptrs(d_out, ns), _ptrs(d_out_masks, ns), _ptrs(d_out_votes,
                                                            ns), _ptrs(d_out_moving, ns),
                                                    _p(counts)), "rsdsfm_plate_video_dev")
        return _wanted(ns, counts=counts)


# ---------------------------------------------------------------------------------------------------
# the colour-consistent plate: the L1 medoid in the median's place, and the context's knob between them (include/rsdsfm_plate_medoid.h)
# ---------------------------------------------------------------------------------------------------
PLATE_MEDOID_HEADER_PATH = _header_path("rsdsfm_plate_medoid.h")
PLATE_MEDIAN, PLATE_MEDOID = 0, 1  # rsdsfm_set_plate_estimator
_PLATE_ESTIMATORS = {"median": PLATE_MEDIAN, "medoid": PLATE_MEDOID}


def plate_medoid_declared_symbols():
    """Names of every function include/rsdsfm_plate_medoid.h declares"""
    return _declared("rsdsfm_plate_medoid.h")


def plate_medoid_launches():
    """kernel launches of one plate_medoid_dev call: 1 (rsdsfm_plate_medoid_launches; host only)"""
    return int(load_library().rsdsfm_plate_medoid_launches())


@_solver_methods
class _PlateMedoidMixin:
    def plate_medoid_dev(self, d_ref, d_ref_mask, d_layers, d_layer_masks, channels, rows, cols, d_image_out, d_mask_out, d_votes=None, d_moving=None, d_counts4=None,
                         d_sums8=None, min_overlap=0, gain_mode=0, threshold=0, min_votes=0, nlayers=None):
        """the per-pixel L1 medoid of the reference and 0 .. 14 layers (rsdsfm_plate_medoid_dev; tests/plate_medoid_spec_numpy.py): a whole
        candidate, the one whose summed L1 distance to the others is smallest, where plate_median_dev selects every channel on its own.  Every
        argument and output is plate_median_dev's; with channels == 1 so is every byte.  One launch, enqueued on the context's stream."""
        self._plate_estimator_dev("rsdsfm_plate_medoid_dev", d_ref, d_ref_mask, d_layers, d_layer_masks, channels, rows, cols, d_image_out, d_mask_out, d_votes, d_moving,
                                  d_counts4, d_sums8, min_overlap, gain_mode, threshold, min_votes, nlayers)

    def plate_medoid(self, ref, ref_mask, layers, records=None, min_overlap=0, gain_mode=0, threshold=0, min_votes=0, device=0):
        """host convenience around plate_medoid_dev, as plate_median is around plate_median_dev
        -> (image, mask, votes, moving (rows, cols) uint8, counts (4,) int64 [unset, static, moving, undecided])"""
        return self._plate_estimator(self.plate_medoid_dev, ref, ref_mask, layers, records, min_overlap, gain_mode, threshold, min_votes, device)

    def set_plate_estimator(self, estimator):
        """the context's knob (rsdsfm_set_plate_estimator): "median" or 0 (the default) = plate_frame_dev ends with plate_median_dev, "medoid" or
        1 = with plate_medoid_dev; plate_video_dev, erase_frame_dev and erase_video_dev follow it.  Anything else is refused.  Holds until set
        again; Solver.plate_estimator is the value in force."""
        value = _PLATE_ESTIMATORS.get(estimator, estimator) if isinstance(estimator, str) else estimator
        if isinstance(value, str):
            raise RsdsfmError("set_plate_estimator: 'median', 'medoid', 0 or 1, not %r" % (estimator,))
        self._check(self.lib.rsdsfm_set_plate_estimator(self._ctx, C.c_int32(int(value))), "rsdsfm_set_plate_estimator")
        self._plate_estimator_knob = int(value)

    @property
    def plate_estimator(self):
        """the knob set_plate_estimator left: 0 (median) or 1 (medoid)"""
        return getattr(self, "_plate_estimator_knob", PLATE_MEDIAN)


# ---------------------------------------------------------------------------------------------------
# the mover removal: the plate's flag as a cleaned, feathered matte and the plate under it (include/rsdsfm_erase.h)
# ---------------------------------------------------------------------------------------------------
ERASE_HEADER_PATH = _header_path("rsdsfm_erase.h")
ERASE_OPEN_MAX, ERASE_GROW_MAX, ERASE_FEATHER_MAX = 3, 8, 16
ERASE_COUNTS = ("unset", "kept", "replaced", "feathered", "unresolved")  # the counters' order


class EraseParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("threshold", C.c_int32), ("min_votes", C.c_int32), ("gain_mode", C.c_int32), ("occlusion", C.c_int32),
                ("occlusion_tol_q16", C.c_int32), ("struct_bytes", C.c_int32), ("open", C.c_int32), ("min_overlap", C.c_int64), ("grow", C.c_int32),
                ("feather", C.c_int32), ("include_undecided", C.c_int32), ("reserved", C.c_int32 * 5)]


def erase_declared_symbols():
    """Names of every function include/rsdsfm_erase.h declares"""
    return _declared("rsdsfm_erase.h")


def _erase_params(radius=None, open=None, grow=None, feather=None, include_undecided=False, threshold=None, min_votes=None, gain=True, occlusion=False,
                  occlusion_tol_q16=0, min_overlap=None):
    """an EraseParams with the given values over the defaults (None: the default).  open and grow are literal here: 0 means none (the struct's -1)"""
    literal = lambda x: None if x is None else (int(x) or -1)
    return _params(EraseParams, "rsdsfm_erase_params_init", radius=radius, threshold=threshold, min_votes=min_votes, min_overlap=min_overlap, open=literal(open),
                   grow=literal(grow), feather=feather, gain_mode=0 if gain else 1, occlusion=occlusion, occlusion_tol_q16=occlusion_tol_q16,
                   include_undecided=include_undecided)


def erase_default_params():
    """the mover removal's defaults as a dict: the plate's and open = 2, grow = 2, feather = 4, include_undecided = 0 (rsdsfm_erase_params_init);
    choices, not measurements"""
    p = _erase_params()
    return dict(radius=p.radius, threshold=p.threshold, min_votes=p.min_votes, min_overlap=p.min_overlap, gain_mode=p.gain_mode, occlusion=p.occlusion, open=p.open, grow=p.grow,
                feather=p.feather, include_undecided=p.include_undecided)


def mover_matte_launches(rows, cols):
    """kernel launches of one mover_matte_dev call: 3 (rsdsfm_mover_matte_launches; host only)"""
    return _launches("rsdsfm_mover_matte_launches", "rows and cols in [2, 16384]", rows, cols)


def erase_composite_launches():
    """kernel launches of one erase_composite_dev call: 1 (rsdsfm_erase_composite_launches; host only)"""
    return int(load_library().rsdsfm_erase_composite_launches())


def erase_launches(rows, cols, nsrc):
    """kernel launches of one erase_frame_dev call on nsrc sources: plate_launches + 3 + 1 (rsdsfm_erase_launches; host only)"""
    return _launches("rsdsfm_erase_launches", "rows and cols in [2, 16384], nsrc in [1, 15]", rows, cols, nsrc)


@_solver_methods
class _EraseMixin:
    def mover_matte_dev(self, d_flag, rows, cols, d_matte, open=2, grow=2, feather=4, include_undecided=False):
        """the plate's flag plane as a matte (rsdsfm_mover_matte_dev; tests/erase_spec_numpy.py): the seeds (flag 2, with include_undecided 3 too)
        eroded by the (2 open + 1)^2 window inside the frame, then feather within open + grow of what is left, one less per pixel beyond.
        Literal values.  Three launches, enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_mover_matte_dev(self._ctx, _np0(d_flag), C.c_int32(rows), C.c_int32(cols), C.c_int32(open), C.c_int32(grow), C.c_int32(feather),
                                                    C.c_int32(int(include_undecided)), _np0(d_matte)), "rsdsfm_mover_matte_dev")

    def mover_matte(self, flag, open=2, grow=2, feather=4, include_undecided=False, device=0):
        """host convenience around mover_matte_dev: flag (rows, cols) uint8 -> the matte (rows, cols) uint8"""
        flag = np.ascontiguousarray(flag, dtype=np.uint8)
        rows, cols = flag.shape
        with _Staging(self, device) as st:
            d_f = st.up(flag)
            d_a = st.empty_like(d_f)
            st.ready()
            self.mover_matte_dev(d_f.data_ptr(), rows, cols, d_a.data_ptr(), open, grow, feather, include_undecided)
            return st.down(d_a)[0]
    def erase_composite_dev(self, d_ref, d_ref_mask, d_plate, d_plate_mask, d_matte, channels, rows, cols, d_image_out, d_mask_out, d_counts5=None, feather=4):
        """the plate under the matte, the own frame's bytes everywhere else (rsdsfm_erase_composite_dev; tests/erase_spec_numpy.py); the counts
        [unset, kept, replaced, feathered, unresolved] into d_counts5 (five device int64).  One launch, enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_erase_composite_dev(self._ctx, _np0(d_ref), _np0(d_ref_mask), _np0(d_plate), _np0(d_plate_mask), _np0(d_matte), C.c_int32(channels),
                                                        C.c_int32(rows), C.c_int32(cols), C.c_int32(feather), _np0(d_image_out), _np0(d_mask_out), _np0(d_counts5)),
                    "rsdsfm_erase_composite_dev")

    def erase_composite(self, ref, ref_mask, plate, plate_mask, matte, feather=4, device=0):
        """host convenience around erase_composite_dev -> (image, mask (rows, cols) uint8, counts (5,) int64)"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        ch = 1 if ref.ndim == 2 else ref.shape[2]
        with _Staging(self, device) as st:
            d_ref, d_rm, d_p, d_pm, d_a = (st.up(x, np.uint8) for x in (ref, ref_mask, plate, plate_mask, matte))
            d_out, d_mask, d_cnt = st.empty_like(d_ref), st.empty((rows, cols)), st.zeros(5, "int64")
            st.ready()
            self.erase_composite_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_p.data_ptr(), d_pm.data_ptr(), d_a.data_ptr(), ch, rows, cols, d_out.data_ptr(), d_mask.data_ptr(),
                                     d_cnt.data_ptr(), feather)
            return st.down(d_out, d_mask, d_cnt)
    def erase_frame_dev(self, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_matte=None, d_moving=None, d_counts5=None, open=None,
                        grow=None, feather=None, include_undecided=False, threshold=None, min_votes=None, gain=True, min_overlap=None, window=None, occlusion=False,
                        occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, params=None):
        """one frame without its movers (rsdsfm_erase_frame_dev): the sources and poses as plate_frame_dev takes them; plate_frame_dev into the
        context's workspace, the matte of its flag (open, grow, feather literal; None: the defaults 2, 2, 4), the plate under the matte and the
        own frame everywhere else into d_image, d_mask; the matte into d_matte, the plate's flag into d_moving, [unset, kept, replaced,
        feathered, unresolved] into d_counts5.  params: an EraseParams passed as it is instead of the keywords.  Enqueued on the context's stream."""
        ns, Mm, mm = _frame_front("erase_frame_dev", d_images, M, m, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
        ep = params if params is not None else _erase_params(None, open, grow, feather, include_undecided, threshold, min_votes, gain, occlusion, occlusion_tol_q16, min_overlap)
        self._check(self.lib.rsdsfm_erase_frame_dev(self._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), *_k4(K),
                                                    C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns), _p(Mm), _p(mm),
                                                    C.byref(ep), _window4(window), _dp(d_image), _dp(d_mask), _np0(d_matte), _np0(d_moving), _np0(d_counts5)),
                    "rsdsfm_erase_frame_dev")

    def erase_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_mattes=None,
                        d_out_moving=None, want_counts=True, radius=None, open=None, grow=None, feather=None, include_undecided=False, threshold=None, min_votes=None,
                        gain=True, min_overlap=None, window=None, occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0):
        """a solved clip without its movers (rsdsfm_erase_video_dev): the clip as plate_video_dev takes it and walks it, erase_frame_dev into
        d_out[q], d_out_masks[q], d_out_mattes[q], d_out_moving[q].  Returns dict(); with want_counts counts (nsources, 5) int64 [unset, kept,
        replaced, feathered, unresolved] -- the call then waits."""
        ns, a, cc, ap, cp, sc = _clip_front("erase_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out,
                d_out_masks=d_out_masks, d_out_mattes=d_out_mattes, d_out_moving=d_out_moving)
        ep = _erase_params(radius, open, grow, feather, include_undecided, threshold, min_votes, gain, occlusion, occlusion_tol_q16, min_overlap)
        counts = _counts(want_counts, ns, 5)
        self._check(self.lib.rsdsfm_erase_video_dev(self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                    _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode), int(q5_mode),
                                                    C.c_int32(iterations), C.byref(ep), _window4(window), _ptrs(d_out, ns), _ptrs(d_out_masks, ns), _ptrs(d_out_mattes,
                                                            ns), _ptrs(d_out_moving, ns),
                                                    _p(counts)), "rsdsfm_erase_video_dev")
        return _wanted(ns, counts=counts)


# ---------------------------------------------------------------------------------------------------
# the sharpness transfer: a blurred frame takes pixels from its sharper registered neighbours (include/rsdsfm_deblur.h)
# ---------------------------------------------------------------------------------------------------
DEBLUR_HEADER_PATH = _header_path("rsdsfm_deblur.h")
DEBLUR_RADIUS_MAX = 3
DEBLUR_LAYERS_MAX = 7
DEBLUR_TAU_MAX = 32
DEBLUR_TAUS_PER_FRAME = 2 * DEBLUR_RADIUS_MAX
DEBLUR_BANDS_MAX = 64


class DeblurParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("strength", C.c_int32), ("margin", C.c_int32), ("gate_mode", C.c_int32), ("gain_mode", C.c_int32), ("occlusion", C.c_int32),
                ("occlusion_tol_q16", C.c_int32), ("struct_bytes", C.c_int32), ("min_overlap", C.c_int64), ("min_pairs", C.c_int64), ("band_rows", C.c_int32), ("reserved3", C.c_int32 * 3)]
    reserved = property(lambda self: [self.band_rows] + list(self.reserved3))  # the four words' name before the first meant anything


def _deblur_params(radius=None, strength=None, margin=None, gate=True, gain=True, occlusion=False, occlusion_tol_q16=0, min_overlap=None, min_pairs=None, band_rows=None):
    """a DeblurParams with the given values over the defaults (None: the default; margin -1: none; band_rows None or 0: one tau per neighbour)"""
    return _params(DeblurParams, "rsdsfm_deblur_params_init", radius=radius, strength=strength, margin=margin, min_overlap=min_overlap, min_pairs=min_pairs,
                   band_rows=band_rows, gate_mode=0 if gate else 1, gain_mode=0 if gain else 1, occlusion=occlusion, occlusion_tol_q16=occlusion_tol_q16)


def deblur_default_params():
    """the sharpness transfer's defaults as a dict: radius = 2, strength = 24, margin = 4, min_overlap = 1024, min_pairs = 1024, band_rows = 0
    (off) (rsdsfm_deblur_params_init); choices, not measurements"""
    p = _deblur_params()
    return dict(radius=p.radius, strength=p.strength, margin=p.margin, gate_mode=p.gate_mode, gain_mode=p.gain_mode, occlusion=p.occlusion, min_overlap=p.min_overlap,
                min_pairs=p.min_pairs, band_rows=p.band_rows)


def deblur_tau(sharp4, margin=0, min_pairs=0):
    """a layer's factor 0 .. 32 from its sharpness record [pairs, A_R, A_L, 0] (rsdsfm_deblur_tau; host only).  margin: -1 none, 0 the default
    (4 sixteenths), 1 .. 64; min_pairs: 0 the default (1024)"""
    rec = np.ascontiguousarray(sharp4, dtype=np.uint64).reshape(4)
    out = C.c_int32(-1)
    rc = load_library().rsdsfm_deblur_tau(_p(rec), C.c_int32(margin), C.c_int64(min_pairs), C.byref(out))
    if rc != OK:
        raise RsdsfmError("rsdsfm_deblur_tau failed (%d): margin in [-1, 64], min_pairs >= 0" % rc)
    return int(out.value)


def deblur_band_taus(records, margin=0, min_pairs=0):
    """the factors 0 .. 32 of a layer's band records (NB, 4) [pairs, A_R, A_L, 0] (rsdsfm_deblur_band_taus; host only): deblur_tau per band
    -> (NB,) int32"""
    rec = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 4)
    out = np.full(max(rec.shape[0], 1), -1, dtype=np.int32)
    rc = load_library().rsdsfm_deblur_band_taus(_p(rec), C.c_int32(rec.shape[0]), C.c_int32(margin), C.c_int64(min_pairs), _p(out))
    if rc != OK:
        raise RsdsfmError("rsdsfm_deblur_band_taus failed (%d): 1 .. 64 bands, margin in [-1, 64], min_pairs >= 0" % rc)
    return out[:rec.shape[0]]


def deblur_row_taus(taus, band_rows, rows):
    """every row's factor from the band factors, interpolated between the band centres (rsdsfm_deblur_row_taus; host only;
    tests/deblur_bands_spec_numpy.py's row_taus) -> (rows,) int32"""
    t = np.ascontiguousarray(taus, dtype=np.int32).reshape(-1)
    out = np.full(max(int(rows), 1), -1, dtype=np.int32)
    rc = load_library().rsdsfm_deblur_row_taus(_p(t), C.c_int32(t.shape[0]), C.c_int32(band_rows), C.c_int32(rows), _p(out))
    if rc != OK:
        raise RsdsfmError("rsdsfm_deblur_row_taus failed (%d): band_rows a multiple of 16 in [16, 16384], rows in [2, 16384], ceil(rows / band_rows) <= 64 taus "
                          "in [0, 32]" % rc)
    return out[:int(rows)]


def deblur_launches(rows, cols, nsrc):
    """kernel launches of one deblur_frame_dev call on nsrc sources: nsrc stabilize_window_launches + 3 (nsrc - 1), or + 1 with one source
    (rsdsfm_deblur_launches; host only)"""
    return _launches("rsdsfm_deblur_launches", "rows and cols in [2, 16384], nsrc in [1, 8]", rows, cols, nsrc)


@_solver_methods
class _DeblurMixin:
    def deblur_sharpness_dev(self, d_ref, d_ref_mask, d_layer, d_layer_mask, channels, rows, cols, d_sharp4, d_sums8=None, min_overlap=0, gain_mode=0):
        """a layer's sharpness record against the reference (rsdsfm_deblur_sharpness_dev; tests/deblur_spec_numpy.py's sharpness): d_sharp4
        (4 device uint64) = [pairs, A_R, A_L, 0], the squared luma differences of every adjacent pixel pair both images see.  d_sums8: the
        layer's overlap record (seam_overlap_sums_dev), None: no gain.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_deblur_sharpness_dev(self._ctx, _np0(d_ref), _np0(d_ref_mask), _np0(d_layer), _np0(d_layer_mask), C.c_int32(channels), C.c_int32(rows),
                                                         C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode), _np0(d_sharp4)),
                    "rsdsfm_deblur_sharpness_dev")

    def deblur_sharpness(self, ref, ref_mask, layer, layer_mask, record=None, min_overlap=0, gain_mode=0, device=0):
        """host convenience around deblur_sharpness_dev -> (4,) uint64"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        with _Staging(self, device) as st:
            d = [st.up(x, np.uint8) for x in (ref, ref_mask, layer, layer_mask)]
            d_rec = None if record is None else st.up64(record)
            d_T = st.full(4, -1, "int64")
            st.ready()
            self.deblur_sharpness_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 1 if ref.ndim == 2 else ref.shape[2], rows, cols, d_T.data_ptr(),
                                      d_rec.data_ptr() if d_rec is not None else None, min_overlap, gain_mode)
            return st.down(d_T)[0].view(np.uint64)
    def deblur_accumulate_dev(self, d_ref, d_ref_mask, d_layer, d_layer_mask, channels, rows, cols, d_cells, first, last, d_sharp4=None, d_sums8=None, min_overlap=0,
                              gain_mode=0, strength=0, margin=0, min_pairs=0, gate_mode=0, d_image_out=None, d_mask_out=None, d_weight=None, d_counts3=None):
        """one layer accumulated onto the cells (rsdsfm_deblur_accumulate_dev; tests/deblur_spec_numpy.py): the layer's pixel counts
        u = (w tau + 8) >> 4, tau from the layer's sharpness record d_sharp4 (deblur_sharpness_dev; required with a layer), w the gate on the
        3 x 3 signed patch sum of the luma difference.  d_layer = d_layer_mask = None: no layer (first and last).  first / last, the outputs and
        [unset, own only, transferred] in d_counts3 as denoise_accumulate_dev.  At most 7 layers.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_deblur_accumulate_dev(self._ctx, _np0(d_ref), _np0(d_ref_mask), _np0(d_layer), _np0(d_layer_mask), C.c_int32(channels), C.c_int32(rows),
                                                          C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode), C.c_int32(strength), _np0(d_sharp4),
                                                          C.c_int32(margin), C.c_int64(min_pairs), C.c_int32(gate_mode), _np0(d_cells), C.c_int32(int(first)),
                                                          C.c_int32(int(last)), _np0(d_image_out), _np0(d_mask_out), _np0(d_weight), _np0(d_counts3)),
                    "rsdsfm_deblur_accumulate_dev")

    def deblur_accumulate(self, ref, ref_mask, layers, records=None, sharps=None, min_overlap=0, gain_mode=0, strength=0, margin=0, min_pairs=0, gate_mode=0, device=0):
        """host convenience around deblur_sharpness_dev and deblur_accumulate_dev: the reference (image, mask), layers a list of 0 .. 7 (image,
        mask) pairs of host arrays, records None or one 8-word overlap record (or None) per layer, sharps None (every layer's sharpness record
        is computed on the device) or one 4-word record per layer
        -> (image, mask, weight (rows, cols) uint8, counts (3,) int64 [unset, own only, transferred], sharps (n, 4) uint64)"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        ch = 1 if ref.ndim == 2 else ref.shape[2]
        with _Staging(self, device) as st:
            d_ref, d_rm = st.up(ref), st.up(ref_mask, np.uint8)
            d_l = [(st.up(i, np.uint8), st.up(m, np.uint8)) for i, m in layers]
            d_rec = [None if records is None or records[j] is None else st.up64(records[j]) for j in range(len(layers))]
            d_T = st.full((max(len(layers), 1), 4), -1, "int64") if sharps is None else st.up64(np.asarray(sharps, dtype=np.uint64).reshape(-1, 4))
            d_cells = st.empty((rows, cols, ch + 1), "int16")
            d_out, d_mask = st.empty_like(d_ref), st.empty((rows, cols))
            d_w, d_cnt = st.empty_like(d_mask), st.zeros(3, "int64")
            st.ready()
            outs = dict(d_image_out=d_out.data_ptr(), d_mask_out=d_mask.data_ptr(), d_weight=d_w.data_ptr(), d_counts3=d_cnt.data_ptr())
            knobs = dict(min_overlap=min_overlap, gain_mode=gain_mode, strength=strength, margin=margin, min_pairs=min_pairs, gate_mode=gate_mode)
            if not d_l:
                self.deblur_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), None, None, ch, rows, cols, None, True, True, **knobs, **outs)
            for j, (d_i, d_m) in enumerate(d_l):
                rec = d_rec[j].data_ptr() if d_rec[j] is not None else None
                if sharps is None:
                    self.deblur_sharpness_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_T[j].data_ptr(), rec, min_overlap, gain_mode)
                self.deblur_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == len(d_l) - 1,
                                           d_T[j].data_ptr(), rec, **knobs, **outs)
            out, mask, weight, counts, T = st.down(d_out, d_mask, d_w, d_cnt, d_T)
            return out, mask, weight, counts, T.view(np.uint64)[:len(layers)]
    def deblur_band_sharpness_dev(self, d_ref, d_ref_mask, d_layer, d_layer_mask, channels, rows, cols, band_rows, d_band_records, d_sums8=None, min_overlap=0,
                                  gain_mode=0):
        """a layer's sharpness records per band of band_rows rows (rsdsfm_deblur_band_sharpness_dev; tests/deblur_bands_spec_numpy.py's
        band_sharpness): d_band_records (ceil(rows / band_rows) x 4 device uint64), a pair in the band of its left or upper pixel.  Enqueued on
        the context's stream."""
        self._check(self.lib.rsdsfm_deblur_band_sharpness_dev(self._ctx, _np0(d_ref), _np0(d_ref_mask), _np0(d_layer), _np0(d_layer_mask), C.c_int32(channels),
                                                              C.c_int32(rows), C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode),
                                                              C.c_int32(band_rows), _np0(d_band_records)), "rsdsfm_deblur_band_sharpness_dev")

    def deblur_band_sharpness(self, ref, ref_mask, layer, layer_mask, band_rows, record=None, min_overlap=0, gain_mode=0, device=0):
        """host convenience around deblur_band_sharpness_dev -> (NB, 4) uint64"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        nb = max(1, -(-rows // max(int(band_rows), 1)))
        with _Staging(self, device) as st:
            d = [st.up(x, np.uint8) for x in (ref, ref_mask, layer, layer_mask)]
            d_rec = None if record is None else st.up64(record)
            d_T = st.full((nb, 4), -1, "int64")
            st.ready()
            self.deblur_band_sharpness_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 1 if ref.ndim == 2 else ref.shape[2], rows, cols, band_rows,
                                           d_T.data_ptr(), d_rec.data_ptr() if d_rec is not None else None, min_overlap, gain_mode)
            return st.down(d_T)[0].view(np.uint64)
    def deblur_band_accumulate_dev(self, d_ref, d_ref_mask, d_layer, d_layer_mask, channels, rows, cols, band_rows, d_cells, first, last, d_band_records=None, d_sums8=None,
                                   min_overlap=0, gain_mode=0, strength=0, margin=0, min_pairs=0, gate_mode=0, d_image_out=None, d_mask_out=None, d_weight=None,
                                   d_counts3=None):
        """deblur_accumulate_dev with a factor per row (rsdsfm_deblur_band_accumulate_dev; tests/deblur_bands_spec_numpy.py): d_band_records the
        layer's band records (deblur_band_sharpness_dev; required with a layer), every band's tau by the frame-wide rule, a row's tau
        interpolated between the band centres.  Enqueued on the context's stream."""
        self._check(self.lib.rsdsfm_deblur_band_accumulate_dev(self._ctx, _np0(d_ref), _np0(d_ref_mask), _np0(d_layer), _np0(d_layer_mask), C.c_int32(channels),
                                                               C.c_int32(rows), C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode),
                                                               C.c_int32(strength), _np0(d_band_records), C.c_int32(band_rows), C.c_int32(margin), C.c_int64(min_pairs),
                                                               C.c_int32(gate_mode), _np0(d_cells), C.c_int32(int(first)), C.c_int32(int(last)), _np0(d_image_out),
                                                               _np0(d_mask_out), _np0(d_weight), _np0(d_counts3)), "rsdsfm_deblur_band_accumulate_dev")

    def deblur_band_accumulate(self, ref, ref_mask, layers, band_rows, records=None, band_records=None, min_overlap=0, gain_mode=0, strength=0, margin=0, min_pairs=0,
                               gate_mode=0, device=0):
        """host convenience around deblur_band_sharpness_dev and deblur_band_accumulate_dev, as deblur_accumulate: band_records None (computed
        on the device) or one (NB, 4) array per layer
        -> (image, mask, weight, counts (3,) int64, band records (n, NB, 4) uint64, cells (rows, cols, CH + 1) uint16 after the last step)"""
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        rows, cols = ref.shape[:2]
        ch = 1 if ref.ndim == 2 else ref.shape[2]
        nb = max(1, -(-rows // max(int(band_rows), 1)))
        with _Staging(self, device) as st:
            d_ref, d_rm = st.up(ref), st.up(ref_mask, np.uint8)
            d_l = [(st.up(i, np.uint8), st.up(m, np.uint8)) for i, m in layers]
            d_rec = [None if records is None or records[j] is None else st.up64(records[j]) for j in range(len(layers))]
            d_T = (st.full((max(len(layers), 1), nb, 4), -1, "int64") if band_records is None
                   else st.up64(np.asarray(band_records, dtype=np.uint64).reshape(-1, nb, 4)))
            d_cells = st.zeros((rows, cols, ch + 1), "int16")
            d_out, d_mask = st.empty_like(d_ref), st.empty((rows, cols))
            d_w, d_cnt = st.empty_like(d_mask), st.zeros(3, "int64")
            st.ready()
            outs = dict(d_image_out=d_out.data_ptr(), d_mask_out=d_mask.data_ptr(), d_weight=d_w.data_ptr(), d_counts3=d_cnt.data_ptr())
            knobs = dict(min_overlap=min_overlap, gain_mode=gain_mode, strength=strength, margin=margin, min_pairs=min_pairs, gate_mode=gate_mode)
            if not d_l:
                self.deblur_band_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), None, None, ch, rows, cols, band_rows, None, True, True, **knobs, **outs)
            for j, (d_i, d_m) in enumerate(d_l):
                rec = d_rec[j].data_ptr() if d_rec[j] is not None else None
                if band_records is None:
                    self.deblur_band_sharpness_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, band_rows, d_T[j].data_ptr(), rec,
                                                   min_overlap, gain_mode)
                self.deblur_band_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, band_rows, d_cells.data_ptr(), j == 0,
                                                j == len(d_l) - 1, d_T[j].data_ptr(), rec, **knobs, **outs)
            out, mask, weight, counts, T, cells = st.down(d_out, d_mask, d_w, d_cnt, d_T, d_cells)
            return out, mask, weight, counts, T.view(np.uint64)[:len(layers)], cells.view(np.uint16)
    def deblur_frame_dev(self, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_weight=None, d_counts3=None, d_sharp_records=None,
                         strength=None, margin=None, gate=True, gain=True, min_overlap=None, min_pairs=None, window=None, occlusion=False, occlusion_tol_q16=0,
                         mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, params=None, band_rows=None):
        """one frame (rsdsfm_deblur_frame_dev): d_images, d_depth_maps, d_R, d_t lists of 1 .. 8 device pointers, source 0 the own frame and the
        others its neighbours; M (nsrc, 3, 3), m (nsrc, 3) every source's pose in the target camera.  The own frame through
        stabilize_window_frame_dev, every neighbour alone on the context's layer, then seam_overlap_sums_dev, deblur_sharpness_dev and
        deblur_accumulate_dev per neighbour; the result into d_image, d_mask, d_weight, d_counts3, the neighbours' sharpness records into
        d_sharp_records ((nsrc - 1) x 4 device uint64).  band_rows (a multiple of 16; None or 0: off): a tau per band of rows through
        deblur_band_sharpness_dev and deblur_band_accumulate_dev, d_sharp_records then (nsrc - 1) x NB x 4.  params: a DeblurParams passed as it
        is instead of the keywords.  Enqueued on the context's stream."""
        ns, Mm, mm = _frame_front("deblur_frame_dev", d_images, M, m, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
        dp = params if params is not None else _deblur_params(None, strength, margin, gate, gain, occlusion, occlusion_tol_q16, min_overlap, min_pairs, band_rows)
        self._check(self.lib.rsdsfm_deblur_frame_dev(self._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), *_k4(K),
                                                     C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns), _p(Mm), _p(mm),
                                                     C.byref(dp), _window4(window), _np0(d_image), _np0(d_mask), _np0(d_weight), _np0(d_counts3), _np0(d_sharp_records)),
                    "rsdsfm_deblur_frame_dev")

    def deblur_video_dev(self, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_weights=None,
                         want_counts=True, want_taus=True, radius=None, strength=None, margin=None, gate=True, gain=True, min_overlap=None, min_pairs=None, window=None,
                         occlusion=False, occlusion_tol_q16=0, mode=BACKPROJECT_RS, q5_mode=Q5_COMPAT, iterations=0, band_rows=None):
        """a solved clip through the sharpness transfer (rsdsfm_deblur_video_dev; with band_rows rsdsfm_deblur_video_banded_dev): the clip as denoise_video_dev takes it and walks it, with
        `radius` 1 .. 3 (None: 2).  Returns dict(); with want_counts counts (nsources, 3) int64 [unset, own only, transferred], with want_taus
        taus (nsources, 6) int32, entry j the factor of the j-th neighbour neighbour_poses lists, -1 behind them -- the call then waits.
        band_rows (a multiple of 16; None: off): a tau per band of rows; taus is then the largest of a neighbour's band taus and, with
        want_taus, band_taus (nsources, 6, NB) int32 rides along.  band_rows 0: rsdsfm_deblur_video_banded_dev with the bands off, band_taus
        (nsources, 6, 1).  Without band_rows every key and byte is what it was."""
        ns, a, cc, ap, cp, sc = _clip_front("deblur_video_dev", d_depth_maps, A, c, A_path, c_path, scales, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out,
                d_out_masks=d_out_masks, d_out_weights=d_out_weights)
        dp = _deblur_params(radius, strength, margin, gate, gain, occlusion, occlusion_tol_q16, min_overlap, min_pairs, band_rows)
        counts = _counts(want_counts, ns, 3)
        taus = _counts(want_taus, ns, DEBLUR_TAUS_PER_FRAME, dtype=np.int32, fill=-1)
        banded = band_rows is not None  # 0: the banded entry point with band_rows off, one band
        nb = max(1, -(-int(rows) // int(band_rows))) if banded and int(band_rows) > 0 else 1
        band_taus = _counts(want_taus and banded, ns, DEBLUR_TAUS_PER_FRAME, min(nb, DEBLUR_BANDS_MAX), dtype=np.int32, fill=-1)
        args = (self._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K), _ptrs(d_depth_maps, ns),
                _ptrs(d_R, ns), _ptrs(d_t, ns), _p(a), _p(cc), _p(ap), _p(cp), _p(sc), int(mode), int(q5_mode), C.c_int32(iterations), C.byref(dp), _window4(window), _ptrs(d_out, ns),
                _ptrs(d_out_masks, ns), _ptrs(d_out_weights, ns), _p(counts), _p(taus))
        if banded:
            self._check(self.lib.rsdsfm_deblur_video_banded_dev(*args, _p(band_taus)), "rsdsfm_deblur_video_banded_dev")
        else:
            self._check(self.lib.rsdsfm_deblur_video_dev(*args), "rsdsfm_deblur_video_dev")
        return _wanted(ns, band_taus=band_taus, counts=counts, taus=taus)


# ---------------------------------------------------------------------------------------------------
# accuracy metrics
# ---------------------------------------------------------------------------------------------------
class ReprojectionStats(C.Structure):
    _fields_ = [("scale", C.c_double), ("mean_error", C.c_double), ("sum_error", C.c_double), ("number_outliers", C.c_int64),
                ("scale_inliers", C.c_int64), ("error_inliers", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def velocity_errors(w_est, v_est, w_true, v_true):
    """(rotation error, translation angle) of errorMeasure.cpp:178-186 -- host-only scalar math through the C ABI"""
    lib = load_library()
    we, ve = C.c_double(), C.c_double()
    rc = lib.rsdsfm_velocity_errors(_v3(w_est), _v3(v_est), _v3(w_true), _v3(v_true), C.byref(we), C.byref(ve))
    if rc != OK:
        raise RsdsfmError("rsdsfm_velocity_errors failed (%d)" % rc)
    return we.value, ve.value


@_solver_methods
class _MetricsMixin:
    def reprojection_error(self, est_coords, gt_depth, est_depth, R_abs, t_abs, K, max_norm=10.0, want_image=True):
        """Camera::meanReprojectionError (+ createErrorImage).  est_coords: (rows, cols, 3) float32; depth maps (rows, cols)."""
        est = np.ascontiguousarray(est_coords, dtype=np.float32)
        rows, cols = est.shape[:2]
        gd = np.ascontiguousarray(np.asarray(gt_depth, dtype=np.float64).T)
        ed = np.ascontiguousarray(np.asarray(est_depth, dtype=np.float64).T)
        Rr, tt = _f64(np.asarray(R_abs).reshape(rows, 9)), _f64(t_abs)
        st = ReprojectionStats()
        img = np.zeros((rows, cols), dtype=np.uint8) if want_image else None
        d = C.c_double
        self._check(self.lib.rsdsfm_reprojection_error(self._ctx, _p(est), _p(gd), _p(ed), _p(Rr), _p(tt), *_k4(K), C.c_int32(rows), C.c_int32(cols), d(max_norm), C.byref(st),
                _p(img)), "rsdsfm_reprojection_error")
        return st.as_dict(), img

    def reprojection_error_dev(self, d_est, d_gt_depth, d_est_depth, d_R, d_t, K, rows, cols, max_norm=10.0, d_error_image=None):
        st = ReprojectionStats()
        d = C.c_double
        self._check(self.lib.rsdsfm_reprojection_error_dev(self._ctx, _dp(d_est), _dp(d_gt_depth), _dp(d_est_depth), _dp(d_R), _dp(d_t), *_k4(K), C.c_int32(rows), C.c_int32(cols),
                d(max_norm), C.byref(st), _dp(d_error_image) if d_error_image else None), "rsdsfm_reprojection_error_dev")
        return st.as_dict()


from . import evaluate, formats  # noqa: E402,F401  (on-disk formats + archive runner)


# ---------------------------------------------------------------------------------------------------
# batched fast path of the dense depth solve: several independent solves per launch (one context each, one shared stream)
# ---------------------------------------------------------------------------------------------------
def prepared_depth_batch(solvers, problems, launch0_only=False):
    """solvers: list of Solver (<= 8, all created on the SAME stream); problems: list of dicts with device pointers
    d_q, d_u, d_alpha, d_alpha_k, d_rho and n, v, w, k.  Returns a zero-argument callable that enqueues the whole batch with
    pre-marshalled arguments (rsdsfm_estimate_inverse_depths_batch_dev; launch0_only: only the streaming launch, for profiling);
    finish each solve with solvers[i].depth_finish_dev."""
    lib = solvers[0].lib
    cnt = len(solvers)
    assert cnt == len(problems) and 1 <= cnt <= 8
    VP = C.c_void_p * cnt
    ctxs = VP(*[s._ctx for s in solvers])
    ptrs = {k2: VP(*[int(p[k2]) for p in problems]) for k2 in ("d_q", "d_u", "d_alpha", "d_alpha_k", "d_rho")}
    ns = (C.c_int64 * cnt)(*[int(p["n"]) for p in problems])
    v3 = (C.c_double * (3 * cnt))(*[float(x) for p in problems for x in p["v"]])
    w3 = (C.c_double * (3 * cnt))(*[float(x) for p in problems for x in p["w"]])
    ks = (C.c_double * cnt)(*[float(p["k"]) for p in problems])
    fn = lib.rsdsfm_depth_lm_batch_launch_dev if launch0_only else lib.rsdsfm_estimate_inverse_depths_batch_dev
    args = (ctxs, C.c_int32(cnt), ptrs["d_q"], ptrs["d_u"], ns, v3, w3, ks, ptrs["d_alpha"], ptrs["d_alpha_k"], ptrs["d_rho"])
    s0 = solvers[0]

    def call():
        rc = fn(*args)
        if rc != OK:
            s0._check(rc, "rsdsfm_estimate_inverse_depths_batch_dev")

    return call

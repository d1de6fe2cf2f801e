"""The temporal noise curve's Python interface (include/rsdsfm_noise_temporal.h; tests/noise_temporal_spec_numpy.py is the definition): a frame's
noise measured from the differences to its registered neighbours, in the noise curve's format, and the temporal denoise and the spatial top-up
at the strength per pixel that curve asks for.

A top-level module beside the import shim rsdsfm.py, NOT part of the package, as rsdsfm_noise_curve.py and rsdsfm_sharpen.py are and for their
reason: the package's public surface and Solver's attributes are pinned (tests/test_binding_marshalling_cpu.py), so every function here takes a
Solver as its first argument in place of being its method.  Argument order and keyword names follow rsdsfm_noise_curve.py's frame and clip
calls.  The library is called without argtypes: every argument is wrapped here, device pointers as c_void_p, sizes as c_int32 / c_int64, doubles
as c_double.  Of the package's private names only _dp, _p, _ptr_array and _libs are reached.
"""
import ctypes as C
import os

import numpy as np

import rsdsfm
from rsdsfm_noise_curve import NOISE_CURVE_BANDS, NOISE_CURVE_ROWS, NOISE_CURVE_WORDS, NoiseCurveParams, noise_curve_strengths

NOISE_TEMPORAL_HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "include", "rsdsfm_noise_temporal.h")
NOISE_PAIR_BIN_NUM, NOISE_PAIR_BIN_DEN = 918, 256  # 3.586 = 4.047 / 1.128: derived, not tuned (the header)


# ---------------------------------------------------------------------------------------------------
# marshalling: what the package's kit does, on the names this module may reach
# ---------------------------------------------------------------------------------------------------
def _np0(ptr):
    """an optional device pointer: NULL for None and 0"""
    return rsdsfm._dp(ptr) if ptr else None


def _ptrs(ptrs, n):
    """an optional list of device pointers -> a C array of the first n; NULL for None, and for no entries wanted"""
    return None if ptrs is None or n == 0 else rsdsfm._ptr_array(list(ptrs)[:n])


def _ref(struct):
    return None if struct is None else C.byref(struct)


def _k4(K):
    return C.c_double(K[0]), C.c_double(K[1]), C.c_double(K[2]), C.c_double(K[3])


def _window4(window):
    return None if window is None else (C.c_int32 * 4)(*[int(x) for x in window])


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _need_all(what, n, **lists):
    for name, lst in lists.items():
        if lst is not None and len(lst) < n:
            raise rsdsfm.RsdsfmError("%s: %s has %d entries, the call needs %d" % (what, name, len(lst), n))


def _params(struct, init, **words):
    """a parameter struct over the library's defaults: `init` fills it, then every word given a value other than None is set"""
    p = struct()
    if getattr(rsdsfm.load_library(), init)(C.byref(p)) != rsdsfm.OK:
        raise rsdsfm.RsdsfmError("%s failed" % init)
    for name, value in words.items():
        if value is not None:
            setattr(p, name, type(getattr(p, name))(value))
    return p


def _curve_params(quantile_q8=None, scale=None, min_samples=None, band_min_samples=None):
    return _params(NoiseCurveParams, "rsdsfm_noise_curve_params_init", quantile_q8=quantile_q8, scale=scale, min_samples=min_samples, band_min_samples=band_min_samples)


def _denoise_params(radius, strength, gain, occlusion, occlusion_tol_q16, min_overlap):
    return _params(rsdsfm.DenoiseParams, "rsdsfm_denoise_params_init", radius=radius, strength=strength, min_overlap=min_overlap, gain_mode=0 if gain else 1,
                   occlusion=occlusion, occlusion_tol_q16=occlusion_tol_q16)


def _spatial_params(strength, target, search):
    return _params(rsdsfm.DenoiseSpatialParams, "rsdsfm_denoise_spatial_params_init", strength=strength, target=target, search=search)


# ---------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------
def noise_pair_hist_launches():
    """kernel launches of one noise_pair_hist_dev call: 1 (rsdsfm_noise_pair_hist_launches; host only)"""
    return int(rsdsfm.load_library().rsdsfm_noise_pair_hist_launches())


def noise_curve_resolve_launches():
    """kernel launches of one noise_curve_resolve_dev call: 1 (rsdsfm_noise_curve_resolve_launches; host only)"""
    return int(rsdsfm.load_library().rsdsfm_noise_curve_resolve_launches())


def denoise_temporal_frame_launches(rows, cols, nsrc, with_spatial=False):
    """kernel launches of one denoise_temporal_frame_dev call: denoise_launches + (nsrc - 1) + 1, + 1 with the top-up
    (rsdsfm_denoise_temporal_frame_launches; host only)"""
    n = rsdsfm.load_library().rsdsfm_denoise_temporal_frame_launches(C.c_int32(rows), C.c_int32(cols), C.c_int32(nsrc), C.c_int32(1 if with_spatial else 0))
    if n < 0:
        raise rsdsfm.RsdsfmError("rsdsfm_denoise_temporal_frame_launches failed (%d): rows and cols in [2, 16384], nsrc in [1, 15]" % n)
    return n


# ---------------------------------------------------------------------------------------------------
# the device calls
# ---------------------------------------------------------------------------------------------------
def noise_pair_hist_dev(solver, d_ref, d_ref_mask, d_layer, d_layer_mask, channels, rows, cols, d_hist8192, first=True, d_sums8=None, min_overlap=0, gain_mode=0):
    """one registered neighbour's pair histogram (rsdsfm_noise_pair_hist_dev): the 3 x 3 patch means of |R - k(L)| over the full, unsaturated
    windows, scaled by 918 / 256 onto the noise curve's m, per band of the reference pixel's level, into d_hist8192 (8 x 1024 device uint32).
    first: the histogram is zeroed in front of the launch; else the launch adds to it.  d_sums8: the overlap record (None: no gain).  Enqueued
    on the context's stream."""
    solver._check(solver.lib.rsdsfm_noise_pair_hist_dev(solver._ctx, rsdsfm._dp(d_ref), rsdsfm._dp(d_ref_mask), _np0(d_layer), _np0(d_layer_mask), C.c_int32(channels),
                                                        C.c_int32(rows), C.c_int32(cols), _np0(d_sums8), C.c_int64(min_overlap), C.c_int32(gain_mode), C.c_int32(int(first)),
                                                        _np0(d_hist8192)), "rsdsfm_noise_pair_hist_dev")


def noise_curve_resolve_dev(solver, d_hist8192, d_curve36, quantile_q8=0):
    """the curve of a banded histogram (rsdsfm_noise_curve_resolve_dev): noise_curve_dev's second launch alone, nine rows [n, m, sigma_q8, 0] into
    d_curve36 (36 device uint64).  Enqueued on the context's stream."""
    solver._check(solver.lib.rsdsfm_noise_curve_resolve_dev(solver._ctx, _np0(d_hist8192), C.c_int32(quantile_q8), _np0(d_curve36)), "rsdsfm_noise_curve_resolve_dev")


def denoise_temporal_frame_dev(solver, d_images, channels, d_depth_maps, d_R, d_t, K, rows, cols, M, m, d_image, d_mask, d_weight=None, d_support=None, d_counts6=None,
                               d_curve36=None, strength=None, gain=True, min_overlap=None, window=None, occlusion=False, occlusion_tol_q16=0, mode=rsdsfm.BACKPROJECT_RS,
                               q5_mode=rsdsfm.Q5_COMPAT, iterations=0, params=None, quantile_q8=None, scale=None, min_samples=None, band_min_samples=None, curve_params=None,
                               spatial=False, spatial_strength=None, target=None, search=None, spatial_params=None):
    """one frame denoised at the strength per pixel the differences to its registered neighbours ask for (rsdsfm_denoise_temporal_frame_dev):
    rsdsfm_noise_curve.denoise_curve_frame_dev's arguments; every neighbour is rendered onto a stack and measured (noise_pair_hist_dev), the
    curve is resolved once, then every neighbour goes through denoise_accumulate_curve_dev, and with spatial (or spatial_params)
    denoise_spatial_curve_dev follows on the same curve.  `strength` and `spatial_strength` are the fallbacks.  d_counts6: six device int64
    [unset, own only, averaged, unset, kept, smoothed]; d_curve36: 36 device uint64 for the curve.  Enqueued on the context's stream."""
    ns = len(d_images)
    _need_all("denoise_temporal_frame_dev", ns, d_depth_maps=d_depth_maps, d_R=d_R, d_t=d_t)
    Mm, mm = _f64(M).reshape(-1, 9), _f64(m).reshape(-1, 3)
    if Mm.shape[0] < ns or mm.shape[0] < ns:
        raise rsdsfm.RsdsfmError("denoise_temporal_frame_dev: every source needs a pose (M, m)")
    dp = params if params is not None else _denoise_params(None, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
    cp = curve_params if curve_params is not None else _curve_params(quantile_q8, scale, min_samples, band_min_samples)
    sp = spatial_params if spatial_params is not None else (_spatial_params(spatial_strength, target, search) if spatial else None)
    solver._check(solver.lib.rsdsfm_denoise_temporal_frame_dev(solver._ctx, _ptrs(d_images, ns), C.c_int32(channels), _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns),
                                                               *_k4(K), C.c_int32(rows), C.c_int32(cols), int(mode), int(q5_mode), C.c_int32(iterations), C.c_int32(ns),
                                                               rsdsfm._p(Mm), rsdsfm._p(mm), C.byref(dp), C.byref(cp), _ref(sp), _window4(window), rsdsfm._dp(d_image),
                                                               rsdsfm._dp(d_mask), _np0(d_weight), _np0(d_support), _np0(d_counts6), _np0(d_curve36)),
                  "rsdsfm_denoise_temporal_frame_dev")


def denoise_temporal_video_dev(solver, d_frames, rows, cols, channels, K, d_depth_maps, d_R, d_t, A, c, A_path, c_path, scales, d_out, d_out_masks, d_out_weights=None,
                               d_out_supports=None, want_counts=True, want_curves=True, radius=None, strength=None, gain=True, min_overlap=None, window=None, occlusion=False,
                               occlusion_tol_q16=0, mode=rsdsfm.BACKPROJECT_RS, q5_mode=rsdsfm.Q5_COMPAT, iterations=0, quantile_q8=None, scale=None, min_samples=None,
                               band_min_samples=None, spatial=False, spatial_strength=None, target=None, search=None):
    """a solved clip denoised at every frame's temporal noise curve (rsdsfm_denoise_temporal_video_dev): rsdsfm_noise_curve.denoise_curve_video_dev's
    clip and walk, denoise_temporal_frame_dev per frame.  Returns dict(); with want_counts counts (nsources, 6) int64, with want_curves curves
    (nsources, 9, 4) uint64 -- with either the call waits."""
    ns = len(d_depth_maps)
    _need_all("denoise_temporal_video_dev", ns, d_frames=d_frames, d_R=d_R, d_t=d_t, d_out=d_out, d_out_masks=d_out_masks, d_out_weights=d_out_weights,
              d_out_supports=d_out_supports)
    a, cc, ap, cp_, sc = _f64(A).reshape(-1, 9), _f64(c).reshape(-1, 3), _f64(A_path).reshape(-1, 9), _f64(c_path).reshape(-1, 3), _f64(scales).reshape(-1)
    if min(a.shape[0], cc.shape[0], ap.shape[0], cp_.shape[0], sc.shape[0]) < ns:
        raise rsdsfm.RsdsfmError("denoise_temporal_video_dev: every source needs a pose on both paths and a scale")
    dp = _denoise_params(radius, strength, gain, occlusion, occlusion_tol_q16, min_overlap)
    cpar = _curve_params(quantile_q8, scale, min_samples, band_min_samples)
    sp = _spatial_params(spatial_strength, target, search) if spatial else None
    counts = np.zeros((max(ns, 1), 6), dtype=np.int64) if want_counts else None
    curves = np.zeros((max(ns, 1), NOISE_CURVE_ROWS, 4), dtype=np.uint64) if want_curves else None
    solver._check(solver.lib.rsdsfm_denoise_temporal_video_dev(solver._ctx, _ptrs(d_frames, ns), C.c_int32(ns), C.c_int32(rows), C.c_int32(cols), C.c_int32(channels), *_k4(K),
                                                               _ptrs(d_depth_maps, ns), _ptrs(d_R, ns), _ptrs(d_t, ns), rsdsfm._p(a), rsdsfm._p(cc), rsdsfm._p(ap),
                                                               rsdsfm._p(cp_), rsdsfm._p(sc), int(mode), int(q5_mode), C.c_int32(iterations), C.byref(dp), C.byref(cpar), _ref(sp),
                                                               _window4(window), _ptrs(d_out, ns), _ptrs(d_out_masks, ns), _ptrs(d_out_weights, ns), _ptrs(d_out_supports, ns),
                                                               rsdsfm._p(counts), rsdsfm._p(curves)), "rsdsfm_denoise_temporal_video_dev")
    out = {}
    if counts is not None:
        out["counts"] = counts[:ns]
    if curves is not None:
        out["curves"] = curves[:ns]
    return out


def noise_temporal(solver, ref, ref_mask, layers, records=None, min_overlap=0, gain_mode=0, quantile_q8=0, scale=0, fallback=0, min_samples=0, band_min_samples=0, device=0):
    """host convenience around noise_pair_hist_dev and noise_curve_resolve_dev: ref (rows, cols[, 3]) uint8 with its mask, layers a list of
    registered (image, mask), records None or one (8,) uint64 (or None) per layer
    -> dict(hist (8, 1024) uint32, curve (9, 4) uint64, sigmas (9,) in grey levels, lut (256,) uint8: noise_curve_strengths of the curve)"""
    import torch

    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    rows, cols = ref.shape[:2]
    ch = 1 if ref.ndim == 2 else ref.shape[2]
    dev = torch.device("cuda", device)
    up = lambda a, dt=np.uint8: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    d_r, d_m = up(ref), up(ref_mask)
    d_l = [(up(i), up(k)) for i, k in layers]
    d_s = [None if records is None or records[j] is None else up(np.asarray(records[j], dtype=np.uint64).view(np.int64), np.int64) for j in range(len(d_l))]
    d_h, d_c = torch.zeros(NOISE_CURVE_BANDS * 1024, dtype=torch.int32, device=dev), torch.empty(NOISE_CURVE_WORDS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # torch fills the planes on its stream, the library works on the context's
    for j, (d_i, d_k) in enumerate(d_l):
        noise_pair_hist_dev(solver, d_r.data_ptr(), d_m.data_ptr(), d_i.data_ptr(), d_k.data_ptr(), ch, rows, cols, d_h.data_ptr(), j == 0,
                            d_s[j].data_ptr() if d_s[j] is not None else None, min_overlap, gain_mode)
    noise_curve_resolve_dev(solver, d_h.data_ptr(), d_c.data_ptr(), quantile_q8)
    solver.synchronize()
    hist = d_h.cpu().numpy().view(np.uint32).reshape(NOISE_CURVE_BANDS, 1024)
    curve = d_c.cpu().numpy().view(np.uint64).reshape(NOISE_CURVE_ROWS, 4)
    return dict(hist=hist, curve=curve, sigmas=curve[:, 2].astype(np.float64) / 256.0, lut=noise_curve_strengths(curve, scale, fallback, min_samples, band_min_samples))

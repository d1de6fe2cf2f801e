"""The sharpen stage's Python interface (include/rsdsfm_sharpen.h; tests/sharpen_spec_numpy.py is the definition): a noise-gated unsharp mask
whose coring threshold follows the noise curve, for the end of a stabilise / super-resolve / denoise chain.

A top-level module beside the import shim rsdsfm.py, NOT part of the package, as rsdsfm_noise_curve.py is and for its reason: the package's
public surface and Solver's attributes are pinned (tests/test_binding_marshalling_cpu.py), so every function here takes a Solver as its first
argument in place of being its method.  The library is called without argtypes: every argument is wrapped here, device pointers as c_void_p,
sizes as c_int32 / c_int64.  Of the package's private names only _dp, _p, _ptr_array and _libs are reached.

amount_q4, coring_q4 and overshoot have NO "0 means the default": 0 is the identity, no coring, no overshoot.  Their defaults (16, 8, 0: choices,
not measurements) are the keyword defaults here and what rsdsfm_sharpen_params_init sets.  strength, scale, min_samples, band_min_samples and
quantile_q8 keep "0: the default".
"""
import ctypes as C
import os

import numpy as np

import rsdsfm
from rsdsfm_noise_curve import NOISE_CURVE_ROWS, NOISE_CURVE_WORDS, NoiseCurveParams

SHARPEN_HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "include", "rsdsfm_sharpen.h")
SHARPEN_AMOUNT_DEFAULT, SHARPEN_CORING_DEFAULT, SHARPEN_OVERSHOOT_DEFAULT = 16, 8, 0  # choices, not measurements
SHARPEN_AMOUNT_MAX, SHARPEN_CORING_MAX, SHARPEN_OVERSHOOT_MAX = 64, 64, 255
SHARPEN_COUNTS = ("unset", "kept", "sharpened", "limited")  # the counters' order


class SharpenParams(C.Structure):
    _fields_ = [("amount_q4", C.c_int32), ("coring_q4", C.c_int32), ("overshoot", C.c_int32), ("strength", C.c_int32), ("struct_bytes", C.c_int32),
                ("reserved", C.c_int32 * 3)]


# ---------------------------------------------------------------------------------------------------
# marshalling: what the package's kit does, on the names this module may reach
# ---------------------------------------------------------------------------------------------------
def _np0(ptr):
    """an optional device pointer: NULL for None and 0"""
    return rsdsfm._dp(ptr) if ptr else None


def _ptrs(ptrs, n):
    return rsdsfm._ptr_array(list(ptrs)[:n])


def _params(struct, init, **words):
    """a parameter struct over the library's defaults: `init` fills it, then every word given a value other than None is set"""
    p = struct()
    if getattr(rsdsfm.load_library(), init)(C.byref(p)) != rsdsfm.OK:
        raise rsdsfm.RsdsfmError("%s failed" % init)
    for name, value in words.items():
        if value is not None:
            setattr(p, name, type(getattr(p, name))(value))
    return p


def _sharpen_params(amount_q4=None, coring_q4=None, overshoot=None, strength=None):
    return _params(SharpenParams, "rsdsfm_sharpen_params_init", amount_q4=amount_q4, coring_q4=coring_q4, overshoot=overshoot, strength=strength)


def _curve_params(quantile_q8=None, scale=None, min_samples=None, band_min_samples=None):
    return _params(NoiseCurveParams, "rsdsfm_noise_curve_params_init", quantile_q8=quantile_q8, scale=scale, min_samples=min_samples, band_min_samples=band_min_samples)


# ---------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------
def sharpen_default_params():
    """the sharpen stage's defaults as a dict: amount_q4 = 16, coring_q4 = 8, overshoot = 0, strength = 12 -- choices, not measurements
    (rsdsfm_sharpen_params_init)"""
    p = _sharpen_params()
    return dict(amount_q4=p.amount_q4, coring_q4=p.coring_q4, overshoot=p.overshoot, strength=p.strength)


def sharpen_launches():
    """kernel launches of one sharpen_dev or sharpen_curve_dev call: 1 (rsdsfm_sharpen_launches; host only)"""
    return int(rsdsfm.load_library().rsdsfm_sharpen_launches())


def sharpen_frame_launches():
    """kernel launches of one sharpen_frame_dev call: 3, the noise curve's two and the sharpen's one (rsdsfm_sharpen_frame_launches; host only)"""
    return int(rsdsfm.load_library().rsdsfm_sharpen_frame_launches())


# ---------------------------------------------------------------------------------------------------
# the device calls
# ---------------------------------------------------------------------------------------------------
def sharpen_dev(solver, d_image, d_mask, channels, rows, cols, d_image_out, d_counts4=None, amount_q4=SHARPEN_AMOUNT_DEFAULT, coring_q4=SHARPEN_CORING_DEFAULT,
                overshoot=SHARPEN_OVERSHOOT_DEFAULT, strength=0):
    """an image sharpened at one strength (rsdsfm_sharpen_dev): a 5 x 5 binomial unsharp mask whose detail is cored below (coring_q4 strength + 8)
    >> 4 and whose result is limited to the local 3 x 3 range widened by overshoot.  d_counts4: four device int64 [unset, kept, sharpened,
    limited].  In-place is refused.  Enqueued on the context's stream."""
    solver._check(solver.lib.rsdsfm_sharpen_dev(solver._ctx, rsdsfm._dp(d_image), rsdsfm._dp(d_mask), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols),
                                                C.c_int32(amount_q4), C.c_int32(coring_q4), C.c_int32(overshoot), C.c_int32(strength), rsdsfm._dp(d_image_out),
                                                _np0(d_counts4)), "rsdsfm_sharpen_dev")


def sharpen_curve_dev(solver, d_image, d_mask, channels, rows, cols, d_curve36, d_image_out, d_counts4=None, amount_q4=SHARPEN_AMOUNT_DEFAULT,
                      coring_q4=SHARPEN_CORING_DEFAULT, overshoot=SHARPEN_OVERSHOOT_DEFAULT, strength=0, scale=0, min_samples=0, band_min_samples=0):
    """sharpen_dev with the strength per pixel from the curve d_curve36 (36 device uint64, noise_curve_dev's), formed on the device
    (rsdsfm_sharpen_curve_dev): the table's entry at the pixel's own level; `strength` is the fallback where the curve's last row has fewer than
    min_samples samples.  Enqueued on the context's stream."""
    solver._check(solver.lib.rsdsfm_sharpen_curve_dev(solver._ctx, rsdsfm._dp(d_image), rsdsfm._dp(d_mask), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols),
                                                      C.c_int32(amount_q4), C.c_int32(coring_q4), C.c_int32(overshoot), C.c_int32(strength), _np0(d_curve36), C.c_int32(scale),
                                                      C.c_int64(min_samples), C.c_int64(band_min_samples), rsdsfm._dp(d_image_out), _np0(d_counts4)),
                  "rsdsfm_sharpen_curve_dev")


def sharpen_frame_dev(solver, d_image, d_mask, channels, rows, cols, d_image_out, d_counts4=None, d_curve36=None, amount_q4=None, coring_q4=None, overshoot=None,
                      strength=None, params=None, quantile_q8=None, scale=None, min_samples=None, band_min_samples=None, curve_params=None):
    """any 8-bit image under a mask measured and sharpened (rsdsfm_sharpen_frame_dev): noise_curve_dev on the input, then sharpen_curve_dev on
    that curve.  A word left None keeps the library's default; params / curve_params pass a struct through as it is.  d_curve36: 36 device uint64
    for the curve, else it stays in the workspace.  Enqueued on the context's stream."""
    sp = params if params is not None else _sharpen_params(amount_q4, coring_q4, overshoot, strength)
    cp = curve_params if curve_params is not None else _curve_params(quantile_q8, scale, min_samples, band_min_samples)
    solver._check(solver.lib.rsdsfm_sharpen_frame_dev(solver._ctx, rsdsfm._dp(d_image), rsdsfm._dp(d_mask), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols), C.byref(sp),
                                                      C.byref(cp), rsdsfm._dp(d_image_out), _np0(d_counts4), _np0(d_curve36)), "rsdsfm_sharpen_frame_dev")


def sharpen_video_dev(solver, d_images, d_masks, channels, rows, cols, d_out, want_counts=True, want_curves=True, amount_q4=None, coring_q4=None, overshoot=None,
                      strength=None, params=None, quantile_q8=None, scale=None, min_samples=None, band_min_samples=None, curve_params=None):
    """a clip of images sharpened frame by frame at every frame's own noise curve (rsdsfm_sharpen_video_dev): sharpen_frame_dev per frame; no
    solved clip is needed.  Returns dict(); with want_counts counts (nframes, 4) int64, with want_curves curves (nframes, 9, 4) uint64 -- with
    either the call waits."""
    n = len(d_images)
    for name, lst in (("d_masks", d_masks), ("d_out", d_out)):
        if len(lst) < n:
            raise rsdsfm.RsdsfmError("sharpen_video_dev: %s has %d entries, the call needs %d" % (name, len(lst), n))
    if n == 0:
        raise rsdsfm.RsdsfmError("sharpen_video_dev: no frames")
    sp = params if params is not None else _sharpen_params(amount_q4, coring_q4, overshoot, strength)
    cp = curve_params if curve_params is not None else _curve_params(quantile_q8, scale, min_samples, band_min_samples)
    counts = np.zeros((n, 4), dtype=np.int64) if want_counts else None
    curves = np.zeros((n, NOISE_CURVE_ROWS, 4), dtype=np.uint64) if want_curves else None
    solver._check(solver.lib.rsdsfm_sharpen_video_dev(solver._ctx, _ptrs(d_images, n), _ptrs(d_masks, n), C.c_int32(n), C.c_int32(channels), C.c_int32(rows), C.c_int32(cols),
                                                      C.byref(sp), C.byref(cp), _ptrs(d_out, n), rsdsfm._p(counts), rsdsfm._p(curves)), "rsdsfm_sharpen_video_dev")
    out = {}
    if counts is not None:
        out["counts"] = counts
    if curves is not None:
        out["curves"] = curves
    return out


def sharpen(solver, image, mask=None, amount_q4=SHARPEN_AMOUNT_DEFAULT, coring_q4=SHARPEN_CORING_DEFAULT, overshoot=SHARPEN_OVERSHOOT_DEFAULT, strength=0, quantile_q8=0,
            scale=0, min_samples=0, band_min_samples=0, device=0):
    """host convenience around sharpen_frame_dev: image (rows, cols[, 3]) uint8, mask (rows, cols) uint8 or None for a full one
    -> dict(image, counts [unset, kept, sharpened, limited], curve (9, 4) uint64, lut (256,) uint8: the strength table the kernel formed)"""
    import torch

    import rsdsfm_noise_curve

    image = np.ascontiguousarray(image, dtype=np.uint8)
    rows, cols = image.shape[:2]
    mask = np.full((rows, cols), 255, dtype=np.uint8) if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    ch = 1 if image.ndim == 2 else image.shape[2]
    dev = torch.device("cuda", device)
    d_i, d_m = torch.from_numpy(image).to(dev), torch.from_numpy(mask).to(dev)
    d_o = torch.empty_like(d_i)
    d_n, d_c = torch.empty(4, dtype=torch.int64, device=dev), torch.empty(NOISE_CURVE_WORDS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # torch fills the planes on its stream, the library works on the context's
    sharpen_frame_dev(solver, d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_o.data_ptr(), d_n.data_ptr(), d_c.data_ptr(), amount_q4, coring_q4, overshoot, strength, None,
                      quantile_q8, scale, min_samples, band_min_samples)
    solver.synchronize()
    curve = d_c.cpu().numpy().view(np.uint64).reshape(NOISE_CURVE_ROWS, 4)
    return dict(image=d_o.cpu().numpy(), counts=d_n.cpu().numpy().tolist(), curve=curve,
                lut=rsdsfm_noise_curve.noise_curve_strengths(curve, scale, strength, min_samples, band_min_samples))

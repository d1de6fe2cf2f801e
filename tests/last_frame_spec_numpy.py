"""The clip's last frame (include/rsdsfm_last_frame.h), defined in float64 numpy: the kernels of csrc/last_frame_kernels.hip reproduce the
advance bit for bit, csrc/last_frame_host.hip the motion to rounding.  Every operation is rounded once and none is fused (the library is
built with -ffp-contract=off).  Nothing here is new arithmetic: the prediction is tests/link_spec_numpy.py's (predict, steps 1 - 4), the
z-buffer tests/fuse_spec_numpy.py's (splat_plane), both imported unchanged.

ADVANCE.  A pair's depth map Z ((rows, cols) here; column-major on the device), the field F it was solved on and its final motion (v, w, k)
give the pair's depth map AS A DEPTH MAP OF THE SECOND FRAME:
    plane = splat_plane(F, Z, v, w, k, 1.0, K, gamma, global_shutter)
every pixel with a valid depth and a usable vector whose landing pixel is inside offers zf = z_pred * 1.0 -- a ratio of exactly 1.0 makes
the product exact, so this is the link's steps 1 - 4 and the fusion's z-buffer with nothing else added -- and the smallest offer per pixel
wins.  The output map is the plane's bit patterns as doubles, +0.0 where the plane is NOTHING; the count is the number of pixels that
received a value.  The map is in the pair's own unit, like the pair's own map.

MOTION.  rsdsfm_pose_table_dev writes, for scanline i of a frame, R_i = I + beta_1 [w]x and t_i = beta_1 v with
    beta_1(tau) = (tau + k tau^2 / 2) * 2 / (2 + k),   tau = gamma i / rows,
the integral of the flow model's velocity profile (1 + k tau) 2 / (2 + k) from the frame's first scanline: tau = 1 is one frame period, where
the pair's second frame starts.  The model holds (v, w, k) constant over both frames of the pair, so scanline s of the SECOND frame, seen
from that frame's first scanline, has moved by
    beta_1(1 + s) - beta_1(1) = ((1 + s) + k (1 + s)^2 / 2 - 1 - k / 2) * 2 / (2 + k)
                              = ((1 + k) s + k s^2 / 2) * 2 / (2 + k)
                              = (1 + k) (s + k' s^2 / 2) * 2 / (2 + k),              k' = k / (1 + k).
The table's own law for a motion (v', w', k') is (s + k' s^2 / 2) * 2 / (2 + k'), and 2 + k' = (2 + 3 k) / (1 + k), so the second frame's
scanlines are the table of
    v' = v (2 + 3 k) / (2 + k),   w' = w (2 + 3 k) / (2 + k),   k' = k / (1 + k)
(to first order in the rotation, which is the table's own approximation).  With k = 0 the factor is 2 / 2 = 1 exactly and k' = 0 / 1: the
outputs are the inputs bit for bit.  1 + k <= 0 would mean the camera stops before the second frame starts and is refused.
"""
import numpy as np

from fuse_spec_numpy import NOTHING, splat_plane
from link_spec_numpy import valid_depth  # noqa: F401  (the validity rule, for the tests)


def advance_depth(F, Z, v, w, k, K, gamma, global_shutter=False):
    """-> (map (rows, cols) float64, plane (rows, cols) uint64, count)"""
    plane = splat_plane(F, Z, v, w, k, 1.0, K, gamma, global_shutter)
    got = plane != NOTHING
    return np.where(got, plane, np.uint64(0)).view(np.float64), plane, int(got.sum())


def last_frame_motion(v, w, k):
    """-> (v', w', k'); ValueError where the library returns RSDSFM_ERR_INVALID"""
    v, w, k = np.asarray(v, dtype=np.float64).reshape(3), np.asarray(w, dtype=np.float64).reshape(3), np.float64(k)
    if not (np.isfinite(v).all() and np.isfinite(w).all() and np.isfinite(k) and 1.0 + k > 0.0):
        raise ValueError("the motion must be finite with 1 + k > 0")
    f = (2.0 + 3.0 * k) / (2.0 + k)
    return v * f, w * f, float(k / (1.0 + k))


def beta_1(tau, k):
    """the pose table's law (csrc/glue_kernels.hip: pose_table_row, with tau = gamma i / rows)"""
    return (tau + 0.5 * k * tau * tau) * (2.0 / (2.0 + k))

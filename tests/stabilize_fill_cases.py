"""Inputs of the border fill's tests (tests/test_stabilize_fill_cpu.py, tests/test_gpu_stabilize_fill.py) and of its golden fixture
(tests/golden/make_golden_stabilize_fill.py): the stabiliser's shift case with a neighbour, a small clip on a jittering path built from
the dense rectifier's images and thinned depth maps (tests/rectify_dense_cases.py), and the two frames of one static scene the accuracy
test is made of."""
import numpy as np

import link_spec_numpy as link
import stabilize_cases as stab_cases
import stabilize_spec_numpy as stab
from stabilize_cases import POSE, golden_path, inputs, shift_case  # noqa: F401  (reused as they are)

# tests/test_stabilize_fill_cpu.py::test_accuracy_against_the_analytic_truth, measured on the CPU (the spec on the neighbour's holed map, 3
# iterations): the filled pixels' position error in pixels and their mean absolute error, and the bounds the GPU-free test asserts, the
# measured values plus half of them
ACC_MEASURED = 0.072328
ACC_BOUND = 1.5 * ACC_MEASURED
ACC_MAE_MEASURED = 0.373208
ACC_MAE_BOUND = 1.5 * ACC_MAE_MEASURED


def shift_fill_case():
    """stabilize_cases.shift_case() (24 x 40, constant depth 4, identity tables, own m = (1, -0.5, 0): 640 of 960 pixels covered) with a
    neighbour of other bytes on the same depth and tables, seen twice:
      full     M = I, m = 0: the neighbour's frame as it is, valid everywhere -- it fills exactly the 320 pixels the own frame leaves, with its
               own bytes: counts (0, 640, 320)
      partial  m = (-1, 0.5, 0): D = (-8, 4), valid in rows 4 .. 23, columns 0 .. 31 -- it fills columns 0 .. 7 of rows 4 .. 19 and columns
               0 .. 31 of rows 20 .. 23, 256 pixels, with the neighbour shifted by (-8, 4), and leaves 64: counts (64, 640, 256)"""
    s = shift_case()
    rows, cols = s["depth"].shape
    rng = np.random.default_rng(2441)
    neighbour = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
    empty = s["mask"] == 0
    full_take = empty.copy()
    full_want = s["want"].copy()
    full_want[full_take] = neighbour[full_take]
    cand = np.zeros_like(neighbour)
    cand_mask = np.zeros((rows, cols), dtype=bool)
    cand[4:, :cols - 8] = neighbour[:rows - 4, 8:]  # output g samples the neighbour at p = g - (-8, 4)
    cand_mask[4:, :cols - 8] = True
    part_take = empty & cand_mask
    part_want = s["want"].copy()
    part_want[part_take] = cand[part_take]
    region = np.zeros((rows, cols), dtype=bool)
    region[4:20, 0:8] = True
    region[20:24, 0:32] = True
    assert np.array_equal(part_take, region)
    return dict(s, neighbour=neighbour, full=dict(M=np.eye(3), m=np.zeros(3), take=full_take, want=full_want, counts=(0, 640, 320)),
                partial=dict(M=np.eye(3), m=np.array([-1.0, 0.5, 0.0]), take=part_take, want=part_want, counts=(64, 640, 256)))


def clip_case(pose_table, rows, cols, channels=3, nframes=5, sigma=1.0, holes=0.4):
    """a clip of nframes frames (nframes - 1 pairs) for stabilize_filled_frame: frame n is the dense rectifier's image and thinned depth map
    rolled by 3 n columns and n rows (other bytes, other holes), every pair has the dense tests' pose table (pose_table: oracle_py's) and
    the frames sit on a jittering path (stabilize_cases.jitter_path, a tenth of its walk so that the frames overlap) with scales 0.8 .. 1.25;
    the path is smoothed with `sigma`.  -> dict(K, images, depths, Rs, ts (lists over the pairs), A, c, As, cs, scales, M, m)"""
    K, image, depth = inputs(rows, cols, channels=channels, holes=holes)
    R, t = pose_table(POSE["v"], POSE["w"], POSE["k"], POSE["gamma"], rows)
    R = np.ascontiguousarray(R).reshape(rows, 9)
    npairs = nframes - 1
    images = [np.ascontiguousarray(np.roll(image, (n, 3 * n), axis=(0, 1))) for n in range(npairs)]
    depths = [np.ascontiguousarray(np.roll(depth, (n, 3 * n), axis=(0, 1))) for n in range(npairs)]
    _, _, A, c = stab_cases.jitter_path(nframes, rot=0.02, pos=0.03)
    c = c * 0.1 + (c - stab_cases.uniform_path(nframes)[1]) * 0.9  # a tenth of the walk, the whole jitter
    scales = np.linspace(0.8, 1.25, npairs)
    As, cs = stab.smooth_path(A, c, sigma)
    M, m = stab.virtual_poses(A, c, As, cs, scales)
    return dict(K=K, images=images, depths=depths, Rs=[R] * npairs, ts=[t] * npairs, A=A, c=c, As=As, cs=cs, scales=scales, M=M, m=m)


def static_scene(synth, pose_table, rows=96, cols=128, seed=0x5EED0000):
    """two frames of ONE static scene from two known poses (tests/test_stabilize_cpu.py's accuracy case made into a clip of two pairs):
      frame n = 1  the rolling-shutter frame of that test: the analytic texture at its pixels, the depth synth.scene_depth with 30 % of it and a
                   block zeroed, that test's pose table; A_1 = I, c_1 = 0, S_1 = 1: its first scanline is the world
      frame q = 0  a GLOBAL-shutter frame (identity tables) of the same scene from A_0 = exp([0.01, -0.02, 0.005]x), c_0 = (0.04, -0.03, 0.02),
                   S_0 = 1: the texture at the positions the world's points have in it (the forward map of frame 1 on the TRUE depth into camera 0,
                   inverted by 50 fixed-point iterations), constant depth 1
      the virtual camera of q: the same centre (c~_0 = c_0), turned by 0.05 rad about y and -0.03 about x: a pure rotation, so the own frame's
      rendering does not depend on its depth and leaves a band of about 5 x 3 pixels empty.
    truth: what the virtual camera sees, from frame 1's TRUE depth: image (rows, cols, 3) float64 and the positions (px, py) in frame 1."""
    K = (0.8 * cols, 0.8 * cols, cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    R, t = pose_table(np.array([0.03, 0.03, 0.0]), np.array([0.02, -0.03, 0.125]), 0.1, 0.8, rows)
    R = np.ascontiguousarray(R).reshape(rows, 9)
    depth = synth.scene_depth(rows, cols)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    frame1 = np.rint(synth._texture(xx, yy, seed)).astype(np.uint8)
    rng = np.random.default_rng(7)  # tests/test_rectify_dense_cpu.py::_holed(depth, 0.30, (40, 50, 12, 20))
    holed = depth.copy()
    holed[rng.random(holed.shape) < 0.30] = 0.0
    holed[40:52, 50:70] = 0.0
    A = np.stack([link.rodrigues(np.array([0.01, -0.02, 0.005])), np.eye(3), np.eye(3)])
    c = np.array([[0.04, -0.03, 0.02], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    As = np.stack([A[0] @ link.rodrigues(np.array([-0.03, 0.05, 0.0])), np.eye(3), np.eye(3)])
    cs = c.copy()
    scales = np.ones(2)

    def seen_from(M, m):  # frame 1's true depth through (M, m): the positions in frame 1 of every pixel of that camera
        gx, gy, _ = stab.forward_map(depth, R, t, *K, M, m)
        F = np.stack([gx - xx, gy - yy], axis=-1)
        px, py = xx.copy(), yy.copy()
        for _ in range(50):
            d = synth._bilinear(F, px, py)
            px, py = xx - d[..., 0], yy - d[..., 1]
        return px, py

    px0, py0 = seen_from(A[0].T, -(A[0].T @ c[0]))  # X_0 = A_0^T (X - c_0)
    frame0 = np.rint(synth._texture(px0, py0, seed)).astype(np.uint8)
    eye_R, zero_t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    M_own, m_own = stab.virtual_poses(A, c, As, cs, scales)
    px, py = seen_from(As[0].T @ A[1], As[0].T @ (c[1] - cs[0]))
    return dict(K=K, images=[frame0, frame1], depths=[np.ones((rows, cols)), holed], Rs=[eye_R, R], ts=[zero_t, t], A=A, c=c, As=As, cs=cs, scales=scales,
                M=M_own[0], m=m_own[0], truth=synth._texture(px, py, seed), px=px, py=py)

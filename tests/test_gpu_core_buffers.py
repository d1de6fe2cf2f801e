"""GPU: the core device entry points of include/rsdsfm.h under the discipline of the later stages' tests.  Every device plane goes through
tests/guarded_planes.py: an input sits at the MINIMUM alignment the header admits for it and not at the next power of two (a double2 array
16 bytes into its buffer, a plain double array 8, an image or a float / int32 array 4, the 8-bit depth and error images at offsets 1, 2 and
3), with guard bytes on both sides; an output is never preset (every byte is the guard value, so a hole that must be WRITTEN as zero is
seen); after every call the guards are intact and the inputs unchanged.  Expected values are the oracle's, with the tolerances of the
existing parity tests of each entry point (bytes, indices and bit patterns exact).  For every pointer with an alignment need, a call with
that pointer one step below the need is refused with RsdsfmError and enqueues nothing: every output is still all guard bytes, every input
unchanged, and the same call without the fault goes through and equals the oracle.

Shapes are the smallest at which each path of the kernels exists (rectify_kernels.hip: 4 pixels per thread with a byte tail, 64 x 16 claim
and write tiles, 32 x 32 depth-image tiles, two launches iff offset <= 2 and cols % 4 == 0; gtflow_kernels.hip / metrics_kernels.hip: 16 x 16
tiles, scanline blocks of 32; glue_kernels.hip: 8-column x 64-row flatten tiles; depth_kernels.hip: double2 pairs, 256-thread blocks,
128-point LDS-DMA tiles)."""
import functools

import numpy as np
import pytest

from guarded_planes import ADMITTED, BELOW, Plane, fresh

pytestmark = pytest.mark.gpu

ARITH = ["reference", "fused"]


class Args:
    """the device planes of ONE call: inputs placed, outputs fresh, each at the admitted minimum of its kind -- except the plane named `bad`,
    which sits at `bad_place` (an (offset, modulus) one step below its need)"""

    def __init__(self, bad=None, bad_place=None):
        import torch

        self.dev = torch.device("cuda", 0)
        self.bad, self.bad_place = bad, bad_place
        self.ins, self.outs, self.inouts, self.kinds = {}, {}, set(), {}

    def _place(self, name, kind):
        self.kinds[name] = kind
        return self.bad_place if name == self.bad else ADMITTED[kind]

    def inp(self, name, a, kind, inout=False):
        self.ins[name] = Plane(a, *self._place(name, kind), device=self.dev)
        if inout:
            self.inouts.add(name)
        return self.ins[name].ptr

    def out(self, name, shape, dtype, kind):
        self.outs[name] = fresh(shape, dtype, *self._place(name, kind), device=self.dev)
        return self.outs[name].ptr

    def inputs_unchanged(self):
        return all(p.unchanged() for n, p in self.ins.items() if n not in self.inouts)

    def nothing_happened(self):
        """after a refused call: every output still all guard bytes, every input (in/out ones too) and every guard as placed"""
        return all(p.unchanged() for p in self.outs.values()) and all(p.unchanged() for p in self.ins.values())

    def get(self, name):
        return (self.outs[name] if name in self.outs else self.ins[name]).get()


def _refusals(rsdsfm, s, run, pointers):
    """run(A) makes the call with its planes allocated through A.  For every (name, kind) of `pointers` whose kind has an alignment need, and
    every placement one step below it: the call raises, and nothing was enqueued.  Returns how many refusals were seen."""
    seen = 0
    for name, kind in pointers:
        for place in BELOW.get(kind, ()):
            A = Args(bad=name, bad_place=place)
            with pytest.raises(rsdsfm.RsdsfmError):
                run(A)
            s.synchronize()
            assert name in A.kinds, name  # the call did allocate a plane of that name
            assert A.nothing_happened(), (name, place)
            seen += 1
    return seen


def _arith(oracle, arith):
    return oracle.arithmetic(arith)


# =====================================================================================================
# rectifier family
# =====================================================================================================
RECT_SIZES = [(1, 1), (1, 7), (7, 1), (4, 4), (3, 5), (5, 6), (9, 5), (33, 68), (33, 70), (2, 8),
              (16, 64), (17, 65), (32, 32), (33, 33)]  # + both sides of the 16-row / 64-column tiles and of the depth image's 32 x 32 tile
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (mode, q5_mode)
BYTE_KINDS = ("byte1", "byte2", "byte3")


@functools.lru_cache(maxsize=None)
def _rect_scene(rsdsfm, oracle, rows, cols):
    """test_back_project_collisions_last_writer_wins's forward-motion construction at rows x cols: holes, collisions, marker pixels; a BGR
    image and a gray one; three inlier lists (none, one, more than pixels: collisions, points outside the image, negative depths)"""
    d = rsdsfm.synth.make_config(1, rows=rows, cols=cols)
    rng = np.random.default_rng(rows * 1000 + cols)
    img = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
    img[rng.random((rows, cols)) < 0.05] = (2, 3, 1)
    marker = rng.random((rows, cols)) < 0.03
    marker[0, 0] = True
    img[marker] = (1, 1, 1)
    gray = rng.integers(16, 256, size=(rows, cols), dtype=np.uint8)
    dark = rng.random((rows, cols)) < 0.05
    gray[dark] = rng.integers(0, 9, size=int(dark.sum()), dtype=np.uint8)
    gray[marker] = 1
    depth = np.array(d["truth"]["Z"])
    depth[rng.random((rows, cols)) < 0.07] = 0.0
    depth = np.abs(depth) + 1.0
    K = tuple(float(x) for x in d["K"])
    R, t = oracle.pose_table(np.array([0.0, 0.0, -3.0]), np.array([0.2, 0.1, 0.3]), 0.0, d["gamma"], rows)
    R = np.ascontiguousarray(R).reshape(rows, 9)
    inls = []
    for m in (0, 1, 2 * rows * cols + 3):
        x, y = rng.uniform(-1.5, cols + 1.5, m), rng.uniform(-1.5, rows + 1.5, m)
        inls.append(np.ascontiguousarray(np.column_stack([(x - K[2]) / K[0], (y - K[3]) / K[1], rng.normal(2.0, 1.5, m)]).reshape(m, 3)))
    e = dict(K=K, img=img, gray=gray, depth_cm=np.ascontiguousarray(depth.T), R=R, t=np.ascontiguousarray(t), inls=inls, bgr={}, g={}, fixed={}, gfixed={})
    gray3 = np.repeat(gray[:, :, None], 3, axis=2)
    for mode, q5 in MODES:
        gs, c3 = oracle.back_project(img, depth, R, t, *K, mode=mode, q5_mode=q5)
        e["bgr"][mode, q5] = (gs, c3)
        gs3, c3g = oracle.back_project(gray3, depth, R, t, *K, mode=mode, q5_mode=q5)
        e["g"][mode, q5] = (gs3, c3g)  # the gray outputs are channel 0 of these, as the header defines them
        for off in (0, 1, 2, 3):
            e["fixed"][mode, q5, off] = oracle.interpolate_cracky(gs, off)
            e["gfixed"][mode, q5, off] = np.ascontiguousarray(oracle.interpolate_cracky(gs3, off)[:, :, 0])
        # the zeros that must be WRITTEN over the guard value are there: a target nobody claims, a marker pixel whose world point is 0
        assert (gs.reshape(-1, 3).max(axis=1) == 0).any() and (gs3.reshape(-1, 3).max(axis=1) == 0).any(), (rows, cols, mode, q5)
        assert marker.any() and (c3[marker] == 0).all() and (c3g[marker] == 0).all()
    e["prev"] = [oracle.depth_preview(inl, *K, rows, cols) for inl in inls]
    assert (e["prev"][0] == 0).all() and ((e["prev"][2] != 0).any() or rows * cols < 16)  # no inlier: every pixel a written zero; many: something lands
    return e


def _frame_inputs(A, e, gray, m_i):
    img = e["gray"] if gray else e["img"]
    inl = e["inls"][m_i]
    return (A.inp("inl", inl if len(inl) else np.zeros((1, 3)), "double"), len(inl), A.inp("img", img, "word"), A.inp("depth", e["depth_cm"], "double"),
            A.inp("R", e["R"], "double"), A.inp("t", e["t"], "double"))


def _run_back_project(s, A, e, mode, q5, coords):
    rows, cols = e["img"].shape[:2]
    s.back_project_dev(A.inp("img", e["img"], "word"), A.inp("depth", e["depth_cm"], "double"), A.inp("R", e["R"], "double"), A.inp("t", e["t"], "double"), e["K"],
                       rows, cols, A.out("gs", (rows, cols, 3), np.uint8, "word"), A.out("c3", (rows, cols, 3), np.float32, "word") if coords else None,
                       mode=mode, q5_mode=q5)


def _check_back_project(A, e, mode, q5, coords):
    gs_o, c3_o = e["bgr"][mode, q5]
    assert A.inputs_unchanged()
    assert np.array_equal(A.get("gs"), gs_o), (mode, q5)
    if coords:
        assert np.array_equal(A.get("c3").view(np.uint32), c3_o.view(np.uint32)), (mode, q5)


def _run_interpolate(s, A, e, src, off):
    rows, cols = src.shape[:2]
    s.interpolate_cracky_dev(A.inp("in", src, "word"), rows, cols, A.out("out", src.shape, np.uint8, "word"), offset=off)


def _run_preview(s, A, e, m_i, kind):
    rows, cols = e["img"].shape[:2]
    inl = e["inls"][m_i]
    s.depth_preview_dev(A.inp("inl", inl if len(inl) else np.zeros((1, 3)), "double"), len(inl), e["K"], rows, cols, A.out("prev", (rows, cols), np.uint8, kind))


def _run_frame(s, A, e, gray, mode, q5, off, m_i, coords, kind):
    rows, cols = e["img"].shape[:2]
    d_inl, m, d_img, d_dm, d_R, d_t = _frame_inputs(A, e, gray, m_i)
    shape = (rows, cols) if gray else (rows, cols, 3)
    (s.rectify_gray_frame_dev if gray else s.rectify_frame_dev)(
        d_inl, m, d_img, d_dm, d_R, d_t, e["K"], rows, cols, A.out("prev", (rows, cols), np.uint8, kind), A.out("gs", shape, np.uint8, "word"),
        A.out("fixed", shape, np.uint8, "word"), A.out("c3", (rows, cols, 3), np.float32, "word") if coords else None, mode=mode, q5_mode=q5, offset=off)


def _check_frame(A, e, gray, mode, q5, off, m_i, coords):
    gs_o, c3_o = e["g" if gray else "bgr"][mode, q5]
    assert A.inputs_unchanged()
    assert np.array_equal(A.get("gs"), gs_o[:, :, 0] if gray else gs_o), (gray, mode, q5, off)
    assert np.array_equal(A.get("fixed"), e["gfixed" if gray else "fixed"][mode, q5, off]), (gray, mode, q5, off)
    assert np.array_equal(A.get("prev"), e["prev"][m_i]), (gray, m_i)
    if coords:
        assert np.array_equal(A.get("c3").view(np.uint32), c3_o.view(np.uint32)), (gray, mode, q5)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("rows,cols", RECT_SIZES)
def test_rectifier_stages_equal_the_oracle(oracle, rsdsfm, rows, cols, arith):
    """back_project_dev in both modes and q5 modes with and without the world points; interpolate_cracky_dev at offsets 0 .. 3 on an image
    with holes; depth_preview_dev with no inlier, one, and more inliers than pixels, the depth image at byte offsets 1, 2, 3"""
    e = _rect_scene(rsdsfm, oracle, rows, cols)
    with rsdsfm.Solver(0, arith=arith) as s:
        for mode, q5 in MODES:
            for coords in (True, False):
                A = Args()
                _run_back_project(s, A, e, mode, q5, coords)
                s.synchronize()
                _check_back_project(A, e, mode, q5, coords)
        src = e["bgr"][0, 0][0]
        for off in (0, 1, 2, 3):
            A = Args()
            _run_interpolate(s, A, e, src, off)
            s.synchronize()
            assert A.inputs_unchanged() and np.array_equal(A.get("out"), e["fixed"][0, 0, off]), off
        for m_i in range(3):
            for kind in BYTE_KINDS:
                A = Args()
                _run_preview(s, A, e, m_i, kind)
                s.synchronize()
                assert A.inputs_unchanged() and np.array_equal(A.get("prev"), e["prev"][m_i]), (m_i, kind)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("rows,cols", RECT_SIZES)
def test_rectify_frame_one_call_equals_the_stages_and_the_oracle(oracle, rsdsfm, rows, cols, gray, arith):
    """rsdsfm_rectify_frame_dev / rsdsfm_rectify_gray_frame_dev at every offset 0 .. 3 (3: three launches also where cols % 4 == 0) in every
    mode; the inlier list, the world points and the depth image's byte offset take turns; the BGR call at offset 1 is also compared with the
    three separate device calls on the same context"""
    e = _rect_scene(rsdsfm, oracle, rows, cols)
    with rsdsfm.Solver(0, arith=arith) as s:
        turn = 0
        for off in (0, 1, 2, 3):
            for mode, q5 in MODES:
                # three counters of different period, so that over the 16 calls every mode and every offset meets both settings of the world
                # points, every inlier list meets every byte offset of the depth image, and neither follows the mode index's parity
                m_i, coords, kind = turn % 3, (turn // 4 + turn) % 2 == 0, BYTE_KINDS[(turn // 3) % 3]
                turn += 1
                A = Args()
                _run_frame(s, A, e, gray, mode, q5, off, m_i, coords, kind)
                s.synchronize()
                _check_frame(A, e, gray, mode, q5, off, m_i, coords)
        if not gray:
            for mode, q5 in MODES:
                A, B, C_, D = Args(), Args(), Args(), Args()
                _run_frame(s, A, e, False, mode, q5, 1, 2, True, "byte1")
                _run_back_project(s, B, e, mode, q5, True)
                s.synchronize()
                _run_interpolate(s, C_, e, B.get("gs"), 1)
                _run_preview(s, D, e, 2, "byte3")
                s.synchronize()
                assert np.array_equal(A.get("gs"), B.get("gs")) and np.array_equal(A.get("c3").view(np.uint32), B.get("c3").view(np.uint32))
                assert np.array_equal(A.get("fixed"), C_.get("out")) and np.array_equal(A.get("prev"), D.get("prev"))


def test_rectifier_refuses_misaligned_pointers(oracle, rsdsfm):
    """every pointer of the five entry points one step below its need (images and world points +1 and +2, double arrays +4); the depth image
    has no need.  (5, 6) takes the byte tail and three launches, (4, 4) the packed path and two"""
    for rows, cols in ((5, 6), (4, 4)):
        e = _rect_scene(rsdsfm, oracle, rows, cols)
        with rsdsfm.Solver(0) as s:
            n = _refusals(rsdsfm, s, lambda A: _run_back_project(s, A, e, 0, 0, True), [("img", "word"), ("depth", "double"), ("R", "double"), ("t", "double"), ("gs", "word"), ("c3", "word")])
            assert n == 3 * 2 + 3
            n = _refusals(rsdsfm, s, lambda A: _run_interpolate(s, A, e, e["bgr"][0, 0][0], 1), [("in", "word"), ("out", "word")])
            assert n == 4
            assert _refusals(rsdsfm, s, lambda A: _run_preview(s, A, e, 2, "byte1"), [("inl", "double"), ("prev", "byte1")]) == 1
            frame = [("inl", "double"), ("img", "word"), ("depth", "double"), ("R", "double"), ("t", "double"), ("prev", "byte2"), ("gs", "word"), ("fixed", "word"), ("c3", "word")]
            for gray in (False, True):
                assert _refusals(rsdsfm, s, lambda A: _run_frame(s, A, e, gray, 0, 0, 1, 2, True, "byte2"), frame) == 4 * 1 + 4 * 2
            # the same calls without the fault
            A = Args()
            _run_back_project(s, A, e, 0, 0, True)
            s.synchronize()
            _check_back_project(A, e, 0, 0, True)
            A = Args()
            _run_interpolate(s, A, e, e["bgr"][0, 0][0], 1)
            s.synchronize()
            assert np.array_equal(A.get("out"), e["fixed"][0, 0, 1])
            A = Args()
            _run_preview(s, A, e, 2, "byte1")
            s.synchronize()
            assert np.array_equal(A.get("prev"), e["prev"][2])
            for gray in (False, True):
                A = Args()
                _run_frame(s, A, e, gray, 0, 0, 1, 2, True, "byte2")
                s.synchronize()
                _check_frame(A, e, gray, 0, 0, 1, 2, True)


# =====================================================================================================
# ground-truth flow
# =====================================================================================================
FLOW_SHAPES = [(1, 1, 1), (15, 17, 33), (17, 15, 97), (16, 16, 32), (17, 17, 31)]  # + exactly one 16 x 16 tile and one scanline block, one over / one under


@functools.lru_cache(maxsize=None)
def _flow_scene(rsdsfm, oracle, rows, cols, rows2, arith, live=True):
    """tests/test_gpu_rectify.py::_flow_scene with void pixels forced in; a single pixel is void or live"""
    d = rsdsfm.synth.make_config(1, rows=rows, cols=cols)
    fx, fy, cx, cy = d["K"]
    rng = np.random.default_rng(rows + cols + rows2)
    yy, xx = np.mgrid[0:rows, 0:cols]
    Z = np.array(d["truth"]["Z"])
    world = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones((rows, cols))], axis=2) * Z[:, :, None]
    world[rng.random((rows, cols)) < 0.1] = 0.0
    if rows * cols > 1:
        world[rows - 1, cols - 1] = 0.0
    elif not live:
        world[0, 0] = 0.0
    R2, t2 = oracle.pose_table(np.array([0.12, 0.10, 0.05]), np.array([0.03, -0.02, 0.06]), 0.3, d["gamma"], rows2)
    t2 = t2 + np.array([0.04, 0.02, 0.01])
    K = tuple(float(x) for x in d["K"])
    want = {}
    with _arith(oracle, arith):
        for q5 in (0, 1):
            want[q5] = oracle.true_flow(world, R2, t2, *K, q5_mode=q5)
    void = (world == 0).all(axis=2)
    assert void.any() or (rows * cols == 1 and live)
    assert (want[0][1][void] == -1).all() and ((want[0][1] >= 0) == ~void).all()
    maps = [np.ascontiguousarray(world[:, :, c].T) for c in range(3)]  # column-major rows x cols
    return dict(K=K, maps=maps, R2=np.ascontiguousarray(R2).reshape(rows2, 9), t2=np.ascontiguousarray(t2), want=want, shape=(rows, cols, rows2))


def _run_true_flow(s, A, e, q5, with_best):
    rows, cols, rows2 = e["shape"]
    s.true_flow_dev(A.inp("wx", e["maps"][0], "double"), A.inp("wy", e["maps"][1], "double"), A.inp("wz", e["maps"][2], "double"), rows, cols,
                    A.inp("R2", e["R2"], "double"), A.inp("t2", e["t2"], "double"), rows2, e["K"], A.out("flow", (rows, cols, 2), np.float64, "double2"),
                    A.out("best", (rows, cols), np.int32, "word") if with_best else None, q5_mode=q5)


def _check_true_flow(A, e, q5, with_best):
    flow_o, best_o = e["want"][q5]
    assert A.inputs_unchanged()
    assert np.array_equal(A.get("flow").view(np.uint64), flow_o.view(np.uint64)), q5
    if with_best:
        assert np.array_equal(A.get("best"), best_o), q5


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("rows,cols,rows2", FLOW_SHAPES)
def test_true_flow_dev_equals_the_oracle(oracle, rsdsfm, rows, cols, rows2, arith):
    """the exhaustive loop (1) and the pruned search at any size (2), both q5 modes, with the winning scanlines and without: flows and winners
    bit for bit; nothing but the two outputs is written"""
    scenes = [_flow_scene(rsdsfm, oracle, rows, cols, rows2, arith)] + ([_flow_scene(rsdsfm, oracle, rows, cols, rows2, arith, live=False)] if rows * cols == 1 else [])
    with rsdsfm.Solver(0, arith=arith) as s:
        for e in scenes:
            for search in (1, 2):
                s.set_true_flow_search(search)
                for q5 in (0, 1):
                    for with_best in (True, False):
                        A = Args()
                        _run_true_flow(s, A, e, q5, with_best)
                        s.synchronize()
                        _check_true_flow(A, e, q5, with_best)


def test_true_flow_dev_refuses_misaligned_pointers(oracle, rsdsfm):
    e = _flow_scene(rsdsfm, oracle, 15, 17, 33, "reference")
    with rsdsfm.Solver(0) as s:
        n = _refusals(rsdsfm, s, lambda A: _run_true_flow(s, A, e, 0, True),
                      [("wx", "double"), ("wy", "double"), ("wz", "double"), ("R2", "double"), ("t2", "double"), ("flow", "double2"), ("best", "word")])
        assert n == 5 + 2 + 2
        A = Args()
        _run_true_flow(s, A, e, 0, True)
        s.synchronize()
        _check_true_flow(A, e, 0, True)


# =====================================================================================================
# reprojection error
# =====================================================================================================
def _close_stats(a, b):  # tests/test_gpu_rectify.py
    assert (a["number_outliers"], a["scale_inliers"], a["error_inliers"]) == (b["number_outliers"], b["scale_inliers"], b["error_inliers"])
    for key in ("scale", "mean_error", "sum_error"):  # global sums: summation order only
        assert np.isclose(a[key], b[key], rtol=1e-11, equal_nan=True), key


@functools.lru_cache(maxsize=None)
def _metrics_scene(rsdsfm, oracle, rows, cols):
    """tests/test_gpu_rectify.py::test_metrics_equal_oracle's scene"""
    d = rsdsfm.synth.make_config(1, rows=rows, cols=cols)
    rng = np.random.default_rng(rows + 3 * cols)
    img = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
    depth = np.array(d["truth"]["Z"])
    depth[rng.random((rows, cols)) < 0.07] = 0.0
    K = tuple(float(x) for x in d["K"])
    R, t = oracle.pose_table(np.array([0.12, 0.10, 0.05]), np.array([0.03, -0.02, 0.06]), 0.0, d["gamma"], rows)
    _, c3 = oracle.back_project(img, depth, R, t, *K)
    est = (c3.astype(np.float64) * 1.3).astype(np.float32)
    est += (rng.normal(0, 0.02, est.shape) * (rng.random(est.shape) < 0.5)).astype(np.float32)
    est[rng.random((rows, cols)) < 0.02] *= 40.0
    gt = np.array(d["truth"]["Z"])
    gt[rng.random((rows, cols)) < 0.03] = 0.0
    Ra, ta = oracle.pose_table(np.array([0.11, 0.10, 0.06]), np.array([0.03, -0.02, 0.05]), 0.0, d["gamma"], rows)
    st_o, eimg_o = oracle.reprojection_error(est, gt, depth, Ra, ta, *K, max_norm=4.0)
    return dict(K=K, est=np.ascontiguousarray(est), gt_cm=np.ascontiguousarray(gt.T), depth_cm=np.ascontiguousarray(depth.T), Ra=np.ascontiguousarray(Ra).reshape(rows, 9),
                ta=np.ascontiguousarray(ta), st=st_o, eimg=eimg_o, shape=(rows, cols))


def _run_metrics(s, A, e, kind):
    rows, cols = e["shape"]
    return s.reprojection_error_dev(A.inp("est", e["est"], "word"), A.inp("gt", e["gt_cm"], "double"), A.inp("depth", e["depth_cm"], "double"), A.inp("R", e["Ra"], "double"),
                                    A.inp("t", e["ta"], "double"), e["K"], rows, cols, max_norm=4.0, d_error_image=A.out("eimg", (rows, cols), np.uint8, kind) if kind else None)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("rows,cols", [(1, 1), (15, 17), (33, 31), (16, 16), (17, 16)])
def test_reprojection_error_dev_equals_the_oracle(oracle, rsdsfm, rows, cols, arith):
    e = _metrics_scene(rsdsfm, oracle, rows, cols)
    with rsdsfm.Solver(0, arith=arith) as s:
        for kind in BYTE_KINDS + (None,):
            A = Args()
            st = _run_metrics(s, A, e, kind)
            assert A.inputs_unchanged()
            _close_stats(st, e["st"])
            if kind:
                # the image depends on the scale, whose last bits depend on the summation order (tests/test_gpu_rectify.py::test_metrics_equal_oracle)
                assert (A.get("eimg") != e["eimg"]).mean() < 1e-5


def test_reprojection_error_dev_refuses_misaligned_pointers(oracle, rsdsfm):
    e = _metrics_scene(rsdsfm, oracle, 15, 17)
    with rsdsfm.Solver(0) as s:
        assert _refusals(rsdsfm, s, lambda A: _run_metrics(s, A, e, "byte1"), [("est", "word"), ("gt", "double"), ("depth", "double"), ("R", "double"), ("t", "double"), ("eimg", "byte1")]) == 2 + 4
        A = Args()
        _close_stats(_run_metrics(s, A, e, "byte1"), e["st"])
        assert (A.get("eimg") != e["eimg"]).mean() < 1e-5


# =====================================================================================================
# solve-side glue: flatten, pose table, depth map
# =====================================================================================================
@functools.lru_cache(maxsize=None)
def _flatten_scene(oracle, rows, cols, col0, zero):
    """a slab of `cols` columns whose first is image column col0; some exactly-zero vectors (n < rows * cols), or all of them"""
    rng = np.random.default_rng(rows * 7 + cols + col0)
    total = col0 + cols + 2
    full = rng.normal(0, 1.0, (rows, total, 2))
    full[rng.random((rows, total)) < 0.3] = 0.0
    full[0, col0] = 0.0
    if zero:
        full[:] = 0.0
    K, gamma = (300.0, 310.0, total / 2.0 + 0.3, rows / 2.0 - 0.2), 0.9
    only = np.zeros_like(full)
    only[:, col0:col0 + cols] = full[:, col0:col0 + cols]  # the reference's scan is column-major: the slab's points are these columns' points
    q, u, qpx, fpx = oracle.flatten(only, *K, gamma)
    assert len(q) < rows * cols and (len(q) == 0) == zero
    return dict(K=K, gamma=gamma, slab=np.ascontiguousarray(full[:, col0:col0 + cols]), q=q, u=u, a=oracle.get_alpha(fpx, rows, gamma), ak=oracle.get_alpha_k(qpx, fpx, rows, gamma),
                shape=(rows, cols, col0))


def _run_flatten(s, A, e, slab_call):
    rows, cols, col0 = e["shape"]
    N = rows * cols
    ptrs = (A.out("q", (N, 2), np.float64, "double2"), A.out("u", (N, 2), np.float64, "double2"), A.out("alpha", (N,), np.float64, "double"), A.out("alpha_k", (N,), np.float64, "double"))
    if slab_call:
        return s.flatten_slab_dev(A.inp("img", e["slab"], "double2"), rows, cols, col0, e["K"], e["gamma"], *ptrs)
    assert col0 == 0
    return s.flatten_dev(A.inp("img", e["slab"], "double2"), rows, cols, e["K"], e["gamma"], *ptrs)


def _check_flatten(A, e, n):
    assert n == len(e["q"]) and A.inputs_unchanged()
    assert np.array_equal(A.get("q")[:n], e["q"]) and np.array_equal(A.get("u")[:n], e["u"])
    assert np.array_equal(A.get("alpha")[:n], e["a"]) and np.array_equal(A.get("alpha_k")[:n], e["ak"])


@pytest.mark.parametrize("arith", ARITH)
def test_flatten_dev_equals_the_oracle(oracle, rsdsfm, arith):
    """one tile and ragged tiles (8 columns x 64 rows), both sides of the tile borders, an all-zero field, slabs with col0 > 0: elements [0, n) bit
    for bit, the guards around the rows x cols capacity intact"""
    with rsdsfm.Solver(0, arith=arith) as s:
        for rows, cols in ((5, 7), (33, 65), (64, 8), (65, 9), (63, 7)):
            for zero in (False, True):
                for col0, slab_call in ((0, False), (0, True), (3, True)):
                    e = _flatten_scene(oracle, rows, cols, col0, zero)
                    A = Args()
                    n = _run_flatten(s, A, e, slab_call)
                    s.synchronize()
                    _check_flatten(A, e, n)


def _run_pose_table(s, A, rows, v, w, k, gamma):
    s.pose_table_dev(v, w, k, gamma, rows, A.out("R", (rows, 9), np.float64, "double"), A.out("t", (rows, 3), np.float64, "double"))


@pytest.mark.parametrize("arith", ARITH)
def test_pose_table_dev_equals_the_oracle(oracle, rsdsfm, arith):
    v, w = np.array([0.03, 0.02, 0.01]), np.array([0.002, -0.003, 0.0087])
    with rsdsfm.Solver(0, arith=arith) as s:
        for rows in (1, 2, 63, 64, 65, 255, 256, 257):  # (the kernel's blocks are 256 scanlines)
            for k in (0.0, 0.4):
                A = Args()
                _run_pose_table(s, A, rows, v, w, k, 0.8)
                s.synchronize()
                Ro, to = oracle.pose_table(v, w, k, 0.8, rows)
                assert np.array_equal(A.get("R"), Ro.reshape(rows, 9)) and np.array_equal(A.get("t"), to), (rows, k)


@functools.lru_cache(maxsize=None)
def _depth_map_scene(oracle, rows, cols, kind, sign):
    rng = np.random.default_rng(rows + cols)
    K = (0.9 * cols, 0.8 * cols, cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    m = {"none": 0, "few": 3, "colliding": 3 * rows * cols, "outside": 40}[kind]
    lo, hi = (-1.5, 1.5) if kind != "outside" else (-40.0, 40.0)
    x, y = rng.uniform(lo, cols + hi, m), rng.uniform(lo, rows + hi, m)
    inl = np.ascontiguousarray(np.column_stack([(x - K[2]) / K[0], (y - K[3]) / K[1], sign * np.abs(rng.normal(2.0, 1.0, m)) - 0.1 * sign]).reshape(m, 3))
    v = np.array([0.3, -0.2, 0.1])
    inl_o, v_o, flipped = oracle.canonicalize_sign(inl, v)
    dm_o, xs_o, ys_o = oracle.scatter_depth(inl_o, *K, rows, cols)
    assert flipped == (sign < 0 and m > 0)
    if kind == "colliding":
        assert len(set(zip(xs_o.tolist(), ys_o.tolist()))) < m
    if kind == "outside":
        assert ((xs_o < 0) | (xs_o >= cols) | (ys_o < 0) | (ys_o >= rows)).any()
    return dict(K=K, inl=inl, v=v, inl_o=inl_o, v_o=v_o, flipped=flipped, dm_cm=np.ascontiguousarray(dm_o.T), xs=xs_o, ys=ys_o, shape=(rows, cols), m=m)


def _run_depth_map(s, A, e, with_xy):
    rows, cols = e["shape"]
    m = e["m"]
    return s.depth_map_dev(A.inp("inl", e["inl"] if m else np.zeros((1, 3)), "double", inout=True), m, e["v"], e["K"], rows, cols, A.out("dm", (cols, rows), np.float64, "double"),
                           A.out("xs", (max(m, 1),), np.int32, "word") if with_xy else None, A.out("ys", (max(m, 1),), np.int32, "word") if with_xy else None)


def _check_depth_map(A, e, got, with_xy):
    m = e["m"]
    v, flipped = got
    assert flipped == e["flipped"] and np.array_equal(v, e["v_o"]) and A.inputs_unchanged()
    assert np.array_equal(A.get("dm"), e["dm_cm"])  # every element written: the zeros too
    assert np.array_equal(A.get("inl")[:m], e["inl_o"]) if m else A.ins["inl"].unchanged()
    if with_xy and m:
        assert np.array_equal(A.get("xs"), e["xs"]) and np.array_equal(A.get("ys"), e["ys"])
    elif with_xy:
        assert A.outs["xs"].unchanged() and A.outs["ys"].unchanged()


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("rows,cols", [(7, 5), (33, 65), (16, 16)])
def test_depth_map_dev_equals_the_oracle(oracle, rsdsfm, rows, cols, arith):
    """no inlier, a few, colliding ones (the last writer wins), ones outside the image; both signs of the mean depth (the in-place flip); with
    and without the pixel indices; the map (exactly 256 pixels at 16 x 16: one block) is written in every element"""
    with rsdsfm.Solver(0, arith=arith) as s:
        for kind in ("none", "few", "colliding", "outside"):
            for sign in (1.0, -1.0):
                e = _depth_map_scene(oracle, rows, cols, kind, sign)
                for with_xy in (True, False):
                    A = Args()
                    got = _run_depth_map(s, A, e, with_xy)
                    _check_depth_map(A, e, got, with_xy)


def test_glue_refuses_misaligned_pointers(oracle, rsdsfm):
    v, w = np.array([0.03, 0.02, 0.01]), np.array([0.002, -0.003, 0.0087])
    with rsdsfm.Solver(0) as s:
        e = _flatten_scene(oracle, 5, 7, 0, False)
        names = [("img", "double2"), ("q", "double2"), ("u", "double2"), ("alpha", "double"), ("alpha_k", "double")]
        for slab_call in (False, True):
            assert _refusals(rsdsfm, s, lambda A: _run_flatten(s, A, e, slab_call), names) == 3 * 2 + 2
            A = Args()
            _check_flatten(A, e, _run_flatten(s, A, e, slab_call))
        assert _refusals(rsdsfm, s, lambda A: _run_pose_table(s, A, 65, v, w, 0.4, 0.8), [("R", "double"), ("t", "double")]) == 2
        A = Args()
        _run_pose_table(s, A, 65, v, w, 0.4, 0.8)
        s.synchronize()
        Ro, to = oracle.pose_table(v, w, 0.4, 0.8, 65)
        assert np.array_equal(A.get("R"), Ro.reshape(65, 9)) and np.array_equal(A.get("t"), to)
        e = _depth_map_scene(oracle, 7, 5, "colliding", -1.0)
        assert _refusals(rsdsfm, s, lambda A: _run_depth_map(s, A, e, True), [("inl", "double"), ("dm", "double"), ("xs", "word"), ("ys", "word")]) == 2 + 2 * 2
        A = Args()
        _check_depth_map(A, e, _run_depth_map(s, A, e, True), True)


# =====================================================================================================
# dense depth solve
# =====================================================================================================
def _check_summary(sm, ref):  # tests/test_gpu_depth.py
    for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "termination"):
        assert sm[k] == ref[k], (k, sm, ref)
    assert np.isclose(sm["initial_cost"], ref["initial_cost"], rtol=1e-12)
    assert np.isclose(sm["final_cost"], ref["final_cost"], rtol=1e-9, atol=1e-25)
    assert np.isclose(sm["final_radius"], ref["final_radius"], rtol=1e-15)


DEPTH_POSE = (np.array([0.6, 0.7, 0.3]), np.array([0.01, -0.02, 0.008]), 0.1)


@functools.lru_cache(maxsize=None)
def _depth_scene(rsdsfm, oracle, n, arith):
    """tests/test_gpu_depth.py::test_ragged_sizes's data"""
    d = rsdsfm.synth.make_config(1, rows=72, cols=96)
    q, u, a, ak = (np.ascontiguousarray(d[k][:n]) for k in ("q", "u", "alpha", "alpha_k"))
    v, w, k = DEPTH_POSE
    with _arith(oracle, arith):
        want = {mode: oracle.estimate_inverse_depths(q, u, v, w, k, a, ak, mode=mode) for mode in (0, 1)}
    return dict(q=q, u=u, a=a, ak=ak, n=n, want=want)


def _run_depth(s, A, e, mode):
    """all five arrays are moved as double2 (the LDS-DMA variant: 16 bytes per lane, each lane's address a multiple of 16 from a 16-byte base)"""
    v, w, k = DEPTH_POSE
    ptrs = (A.inp("q", e["q"], "double2"), A.inp("u", e["u"], "double2"), e["n"], v, w, k, A.inp("alpha", e["a"], "double2"), A.inp("alpha_k", e["ak"], "double2"),
            A.out("rho", (e["n"],), np.float64, "double2"))
    s.estimate_inverse_depths_dev(*ptrs, mode=mode)
    return s.depth_finish_dev(*ptrs)[0] if mode == 1 else s.synchronize()


def _check_depth(A, e, mode, sm):
    rho_o, sm_o = e["want"][mode]
    assert A.inputs_unchanged()
    assert np.allclose(A.get("rho"), rho_o, rtol=1e-9, atol=1e-13)
    if mode == 1:
        _check_summary(sm, sm_o)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_estimate_inverse_depths_dev_equals_the_oracle(oracle, rsdsfm, variant, arith):
    """both depth modes at one pair, odd counts and both sides of the 256-thread block; around one 128-point tile of the LDS-DMA variant (1),
    whose loads need no more than the 16 bytes the entry point demands"""
    with rsdsfm.Solver(0, arith=arith) as s:
        s.set_depth_variant(variant)
        for n in (1, 2, 3, 255, 256, 257) + ((127, 128, 129) if variant == 1 else ()):
            e = _depth_scene(rsdsfm, oracle, n, arith)
            for mode in (0, 1):
                A = Args()
                sm = _run_depth(s, A, e, mode)
                _check_depth(A, e, mode, sm)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_estimate_inverse_depths_dev_refuses_misaligned_pointers(oracle, rsdsfm, variant):
    """the 16-byte check of the depth launches, every variant, both modes: +8 and +4"""
    e = _depth_scene(rsdsfm, oracle, 257, "reference")
    with rsdsfm.Solver(0) as s:
        s.set_depth_variant(variant)
        for mode in (0, 1):
            n = _refusals(rsdsfm, s, lambda A: _run_depth(s, A, e, mode), [(k, "double2") for k in ("q", "u", "alpha", "alpha_k", "rho")])
            assert n == 10
            A = Args()
            _check_depth(A, e, mode, _run_depth(s, A, e, mode))


def _depth_problem(A, e, tag):
    v, w, k = DEPTH_POSE
    names = ("q", "u", "alpha", "alpha_k")
    p = {"d_" + name: A.inp(name + tag, e[key], "double2") for name, key in zip(names, ("q", "u", "a", "ak"))}
    return dict(p, d_rho=A.out("rho" + tag, (e["n"],), np.float64, "double2"), n=e["n"], v=v, w=w, k=k)


def _finish_depth(s, p):
    return s.depth_finish_dev(p["d_q"], p["d_u"], p["n"], p["v"], p["w"], p["k"], p["d_alpha"], p["d_alpha_k"], p["d_rho"])[0]


def test_depth_batch_and_stage_launches_refuse_misaligned_pointers(oracle, rsdsfm):
    """the same 16-byte check in the batched launch (rsdsfm_estimate_inverse_depths_batch_dev and its streaming-launch-only twin: a pointer of
    the SECOND problem, so nothing of the first is enqueued either) and in the stage launch rsdsfm_depth_lm_launch_dev (refusal only: it is
    launch 1 of the solve that test_estimate_inverse_depths_dev_equals_the_oracle runs at this alignment).  The batch without the fault equals
    the oracle on both problems."""
    import torch

    es = [_depth_scene(rsdsfm, oracle, n, "reference") for n in (257, 3)]
    five = ("q", "u", "alpha", "alpha_k", "rho")
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    solvers = [rsdsfm.Solver(0, stream=stream.cuda_stream) for _ in es]  # (a batch's contexts share one stream)
    try:
        for launch0_only in (False, True):
            run = lambda A: rsdsfm.prepared_depth_batch(solvers, [_depth_problem(A, e, str(i)) for i, e in enumerate(es)], launch0_only=launch0_only)()
            assert _refusals(rsdsfm, solvers[0], run, [(k + "1", "double2") for k in five] + [("q0", "double2")]) == 12
        A = Args()
        probs = [_depth_problem(A, e, str(i)) for i, e in enumerate(es)]
        rsdsfm.prepared_depth_batch(solvers, probs)()
        sms = [_finish_depth(s, p) for s, p in zip(solvers, probs)]
        assert A.inputs_unchanged()
        for i, e in enumerate(es):
            rho_o, sm_o = e["want"][1]
            # (tests/test_gpu_depth.py::test_batched_fast_path_equals_single_solves)
            assert sms[i]["num_iterations"] == sm_o["num_iterations"] and np.allclose(A.get("rho%d" % i), rho_o, rtol=1e-9, atol=1e-13)

        def stage(A):
            p = _depth_problem(A, es[0], "")
            solvers[0].depth_lm_launch_dev(p["d_q"], p["d_u"], p["n"], p["v"], p["w"], p["k"], p["d_alpha"], p["d_alpha_k"], p["d_rho"], launch_id=0)

        assert _refusals(rsdsfm, solvers[0], stage, [(k, "double2") for k in five]) == 10
    finally:
        for s in solvers:
            s.close()


# =====================================================================================================
# RANSAC and refinement on device buffers
# =====================================================================================================
RANSAC_OUT = [("inlier_idx", np.int64, 1, "double"), ("inliers", np.float64, 3, "double"), ("alpha", np.float64, 1, "double"), ("alpha_k", np.float64, 1, "double"),
              ("mask", np.uint8, 1, "byte3"), ("inv_depth", np.float64, 1, "double")]


@functools.lru_cache(maxsize=None)
def _ransac_scene(rsdsfm, oracle):
    """the smallest frame of tests/test_gpu_ransac.py::test_ransac_hypothesis_groups_on_small_frames"""
    d = rsdsfm.synth.make_config(3, rows=24, cols=32)
    q, u, a, ak = (np.ascontiguousarray(d[k]) for k in ("q", "u", "alpha", "alpha_k"))
    T, tol = 50, 0.004
    samples = oracle.sample_indices(len(q), T, 99)
    ro = oracle.ransac(q, u, a, ak, False, T, tol, samples, depth_mode=1)
    assert 0 < ro["num_inliers"] < len(q)
    return dict(q=q, u=u, a=a, ak=ak, T=T, tol=tol, samples=samples, want=ro)


def _run_ransac(s, A, e):
    n = len(e["a"])
    outs = {name: A.out(name, (n, w_) if w_ > 1 else (n,), dtype, kind) for name, dtype, w_, kind in RANSAC_OUT}
    return s.ransac_dev(A.inp("q", e["q"], "double2"), A.inp("u", e["u"], "double2"), A.inp("a", e["a"], "double"), A.inp("ak", e["ak"], "double"), n, False, e["T"], e["tol"],
                        outs, samples=e["samples"], depth_mode=1)


def _ransac_result(A, r):
    m = r["num_inliers"]
    out = dict(r)
    for name, _, _, _ in RANSAC_OUT:
        out[name] = A.get(name) if name in ("mask", "inv_depth") else A.get(name)[:m]
    return out


def _check_ransac(A, e, r, plain=None):
    ro = e["want"]
    g = _ransac_result(A, r)
    assert A.inputs_unchanged()
    # tests/test_gpu_ransac.py::_compare_ransac, for what the device call returns
    assert np.array_equal(g["trial_count"], ro["trial_count"]) and np.array_equal(g["trial_steps"], ro["trial_steps"])
    assert g["best_trial"] == ro["best_trial"] and g["num_inliers"] == ro["num_inliers"]
    assert np.array_equal(g["mask"], ro["mask"]) and np.array_equal(g["inlier_idx"], ro["inlier_idx"])
    assert np.allclose(g["inv_depth"], ro["inv_depth"], rtol=1e-9, atol=1e-13) and np.allclose(g["inliers"], ro["inliers"], rtol=1e-9, atol=1e-13)
    assert np.array_equal(g["alpha"], ro["alpha"]) and np.array_equal(g["alpha_k"], ro["alpha_k"])
    assert np.allclose(g["w"], ro["w"], atol=1e-10) and np.allclose(g["v"], ro["v"], atol=1e-10) and abs(g["k"] - ro["k"]) <= 1e-9 * max(1.0, abs(ro["k"]))
    if plain is not None:  # the run on ordinary buffers: the same bits
        for key in g:
            if key != "inlier_error":  # (a diagnostic whose last bits depend on which form scored the winner: include/rsdsfm.h)
                assert np.array_equal(np.asarray(g[key]), np.asarray(plain[key])), key


def _plain_ransac(torch, s, e):
    dev = torch.device("cuda", 0)
    n = len(e["a"])
    tt = lambda a: torch.from_numpy(a).to(dev)
    d_q, d_u, d_a, d_ak = tt(e["q"]), tt(e["u"]), tt(e["a"]), tt(e["ak"])
    bufs = {name: torch.zeros((n, w_) if w_ > 1 else (n,), dtype=getattr(torch, np.dtype(dtype).name), device=dev) for name, dtype, w_, _ in RANSAC_OUT}
    torch.cuda.synchronize()  # torch filled these on its own stream; the library works on the context's
    r = s.ransac_dev(d_q.data_ptr(), d_u.data_ptr(), d_a.data_ptr(), d_ak.data_ptr(), n, False, e["T"], e["tol"], {k: b.data_ptr() for k, b in bufs.items()},
                     samples=e["samples"], depth_mode=1)
    m = r["num_inliers"]
    out = dict(r)
    for name in bufs:
        out[name] = bufs[name].cpu().numpy() if name in ("mask", "inv_depth") else bufs[name].cpu().numpy()[:m]
    return out


def test_ransac_dev_on_guarded_planes_equals_ordinary_buffers_and_the_oracle(oracle, rsdsfm):
    import torch

    e = _ransac_scene(rsdsfm, oracle)
    pointers = [("q", "double2"), ("u", "double2"), ("a", "double"), ("ak", "double")] + [(name, kind) for name, _, _, kind in RANSAC_OUT]
    with rsdsfm.Solver(0) as s:
        assert _refusals(rsdsfm, s, lambda A: _run_ransac(s, A, e), pointers) == 2 * 2 + 2 + 5
        plain = _plain_ransac(torch, s, e)
        A = Args()
        r = _run_ransac(s, A, e)
        _check_ransac(A, e, r, plain)


@functools.lru_cache(maxsize=None)
def _refine_scene(oracle, mode):
    """tests/test_gpu_refine_glue.py::test_refine_golden_cases on its first noisy case, both ways of indexing the flow"""
    import os

    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v1.npz"))
    g = lambda k: golden["noisy_k0/" + k]
    q, u, a, ak = g("q"), g("u"), g("alpha"), g("alpha_k")
    use_k = bool(g("use_k"))
    b = int(g("best"))
    v, w, k = g("hyp_v")[b], g("hyp_w")[b], float(g("hyp_k")[b])
    mask = g("best_mask").astype(bool)
    rho, _ = oracle.estimate_inverse_depths(q, u, v, w, k, a, ak, mode=1)
    inl = np.ascontiguousarray(np.stack([q[mask, 0], q[mask, 1], 1.0 / rho[mask]], axis=1))
    idx = np.ascontiguousarray(np.nonzero(mask)[0].astype(np.int64))
    ref = oracle.refine(u, inl, a[mask], ak[mask], v, w, k, use_k, flow_index_mode=mode, inlier_idx=idx)
    return dict(u=np.ascontiguousarray(u), inl=inl, a=np.ascontiguousarray(a[mask]), ak=np.ascontiguousarray(ak[mask]), idx=idx, v=v, w=w, k=k, use_k=use_k, mode=mode, want=ref)


def _run_refine(s, A, e):
    m = len(e["inl"])
    return s.refine_dev(A.inp("flow", e["u"], "double2"), len(e["u"]), m, A.inp("inl", e["inl"], "double"), A.inp("a", e["a"], "double"), A.inp("ak", e["ak"], "double"),
                        A.inp("idx", e["idx"], "double") if e["mode"] == 1 else None, e["v"], e["w"], e["k"], e["use_k"], e["mode"], A.out("out", (m, 3), np.float64, "double"))


def _check_refine(A, e, out, plain=None):  # tests/test_gpu_refine_glue.py::_check_refine
    ref, rtol = e["want"], 1e-6
    sm, smo = out["summary"], ref["summary"]
    inl = A.get("out")
    assert A.inputs_unchanged()
    for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "termination"):
        assert sm[k] == smo[k], (k, sm, smo)
    assert np.isclose(sm["initial_cost"], smo["initial_cost"], rtol=1e-11)
    assert np.isclose(sm["final_cost"], smo["final_cost"], rtol=1e-7, atol=1e-25)
    assert np.allclose(out["v"], ref["v"], rtol=rtol, atol=1e-10) and np.allclose(out["w"], ref["w"], rtol=rtol, atol=1e-10)
    assert np.isclose(out["k"], ref["k"], rtol=rtol, atol=1e-10)
    assert np.array_equal(inl[:, :2], ref["inliers"][:, :2]) and np.allclose(inl[:, 2], ref["inliers"][:, 2], rtol=rtol)
    if plain is not None:
        p_out, p_inl = plain
        assert np.array_equal(inl, p_inl) and np.array_equal(out["v"], p_out["v"]) and np.array_equal(out["w"], p_out["w"]) and out["k"] == p_out["k"] and sm == p_out["summary"]


@pytest.mark.parametrize("mode", [0, 1])
def test_refine_dev_on_guarded_planes_equals_ordinary_buffers_and_the_oracle(oracle, rsdsfm, mode):
    import torch

    dev = torch.device("cuda", 0)
    e = _refine_scene(oracle, mode)
    m = len(e["inl"])
    pointers = [("flow", "double2"), ("inl", "double"), ("a", "double"), ("ak", "double"), ("out", "double")] + ([("idx", "double")] if mode == 1 else [])
    with rsdsfm.Solver(0) as s:
        assert _refusals(rsdsfm, s, lambda A: _run_refine(s, A, e), pointers) == 2 + 4 + mode
        tt = lambda a: torch.from_numpy(a).to(dev)
        t_ = {k: tt(e[k]) for k in ("u", "inl", "a", "ak", "idx")}
        t_out = torch.zeros((m, 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()  # torch filled these on its own stream; the library works on the context's
        p_out = s.refine_dev(t_["u"].data_ptr(), len(e["u"]), m, t_["inl"].data_ptr(), t_["a"].data_ptr(), t_["ak"].data_ptr(), t_["idx"].data_ptr() if mode == 1 else None,
                             e["v"], e["w"], e["k"], e["use_k"], mode, t_out.data_ptr())
        s.synchronize()
        A = Args()
        out = _run_refine(s, A, e)
        s.synchronize()
        _check_refine(A, e, out, (p_out, t_out.cpu().numpy()))


# =====================================================================================================
# the frame solve
# =====================================================================================================
@functools.lru_cache(maxsize=None)
def _frame_scene(rsdsfm):
    """the smallest parity case tests/test_gpu_frame.py solves"""
    d = rsdsfm.synth.make_config(3, rows=144, cols=256)
    return dict(rows=d["rows"], cols=d["cols"], K=d["K"], gamma=d["gamma"], flow=np.ascontiguousarray(d["flow_img"]), T=12, tol=0.002, seed=99)


def _frame_planes(A, e, tag=""):
    rows, cols = e["rows"], e["cols"]
    return (A.inp("img" + tag, e["flow"], "double2"), A.out("dm" + tag, (cols, rows), np.float64, "double"), A.out("R" + tag, (rows, 9), np.float64, "double"),
            A.out("t" + tag, (rows, 3), np.float64, "double"))


def _run_solve_frame(s, A, e, rsdsfm, seed=None):
    d_img, d_dm, d_R, d_t = _frame_planes(A, e)
    return s.solve_frame_dev(d_img, e["rows"], e["cols"], e["K"], e["gamma"], d_dm, d_R, d_t, trials=e["T"], tol=e["tol"], seed=e["seed"] if seed is None else seed,
                             flow_index_mode=rsdsfm.FLOW_GATHERED)


def _run_solve_frames(s, A, e, rsdsfm, seeds):
    jobs = []
    for i in range(len(seeds)):
        d_img, d_dm, d_R, d_t = _frame_planes(A, e, str(i))
        jobs.append(dict(d_flow_img=d_img, rows=e["rows"], cols=e["cols"], K=e["K"], gamma=e["gamma"], d_depth_map=d_dm, d_R=d_R, d_t=d_t))
    return s.solve_frames_dev(jobs, seeds, trials=e["T"], tol=e["tol"], flow_index_mode=rsdsfm.FLOW_GATHERED)


SCALARS = ("n", "num_inliers", "best_trial", "flipped", "k", "ransac_k", "refine_summary")


def _same_solve(A, tag, r, plain):
    p, dm, R, t = plain
    for key in SCALARS:
        assert r[key] == p[key], key
    for key in ("w", "v", "ransac_w", "ransac_v"):
        assert np.array_equal(r[key], p[key]), key
    assert np.array_equal(A.get("dm" + tag), dm) and np.array_equal(A.get("R" + tag), R) and np.array_equal(A.get("t" + tag), t)


def _plain_solve(torch, s, e, rsdsfm, seed):
    dev = torch.device("cuda", 0)
    rows, cols = e["rows"], e["cols"]
    img = torch.from_numpy(e["flow"]).to(dev)
    dm, R, t = (torch.zeros(shape, dtype=torch.float64, device=dev) for shape in ((cols, rows), (rows, 9), (rows, 3)))
    torch.cuda.synchronize()  # torch filled these on its own stream; the library works on the context's
    r = s.solve_frame_dev(img.data_ptr(), rows, cols, e["K"], e["gamma"], dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=e["T"], tol=e["tol"], seed=seed,
                          flow_index_mode=rsdsfm.FLOW_GATHERED)
    s.synchronize()
    return r, dm.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()


def test_solve_frame_dev_on_guarded_planes(oracle, rsdsfm):
    """tests/test_gpu_frame.py::test_solve_frame_dev_matches_stages_and_oracle (gathered flow) with the depth map and the pose table guarded, at 8
    bytes and never preset, the flow image at 16: the stage-by-stage path bit for bit, the oracle chain to that test's bars, the run on ordinary
    buffers bit for bit; every pointer one step below its need is refused"""
    import torch

    e = _frame_scene(rsdsfm)
    rows, cols, K, gamma, T, tol, seed = e["rows"], e["cols"], e["K"], e["gamma"], e["T"], e["tol"], e["seed"]
    with rsdsfm.Solver(0) as s:
        assert _refusals(rsdsfm, s, lambda A: _run_solve_frame(s, A, e, rsdsfm), [("img", "double2"), ("dm", "double"), ("R", "double"), ("t", "double")]) == 2 + 3
        A = Args()
        r = _run_solve_frame(s, A, e, rsdsfm)
        s.synchronize()
        assert A.inputs_unchanged()
        _same_solve(A, "", r, _plain_solve(torch, s, e, rsdsfm, seed))
        q, u, a, ak = s.flatten(e["flow"], K, gamma)
        rr = s.ransac(q, u, a, ak, False, T, tol, samples=None, seed=seed, depth_mode=1)
        ref = s.non_linear_refinement(u, rr["inliers"], rr["alpha"], rr["alpha_k"], rr["v"], rr["w"], rr["k"], False, flow_index_mode=1, inlier_idx=rr["inlier_idx"])
        dmap = s.depth_map(ref["inliers"], ref["v"], K, rows, cols)
        Rr, tr = s.pose_table(dmap["v"], ref["w"], ref["k"], gamma, rows)
    got = A.get("dm").T
    assert r["n"] == len(q) and r["num_inliers"] == rr["num_inliers"] and r["best_trial"] == rr["best_trial"]
    assert np.array_equal(r["ransac_w"], rr["w"]) and np.array_equal(r["ransac_v"], rr["v"])
    assert np.array_equal(r["w"], ref["w"]) and np.array_equal(r["v"], dmap["v"]) and r["k"] == ref["k"]
    assert r["refine_summary"] == ref["summary"]
    assert np.array_equal(got, dmap["depth_map"]) and (got == 0).any()  # pixels without an inlier: zeros that were written
    assert np.array_equal(A.get("R").reshape(rows, 3, 3), Rr) and np.array_equal(A.get("t"), tr)
    ro = oracle.ransac(q, u, a, ak, False, T, tol, oracle.sample_indices(len(q), T, seed), depth_mode=1)
    assert ro["num_inliers"] == r["num_inliers"] and ro["best_trial"] == r["best_trial"] and 0 < ro["num_inliers"] < len(q)
    refo = oracle.refine(u, ro["inliers"], ro["alpha"], ro["alpha_k"], ro["v"], ro["w"], ro["k"], False, 1, ro["inlier_idx"])
    for key in ("num_iterations", "num_successful_steps", "termination"):
        assert r["refine_summary"][key] == refo["summary"][key], key
    inl_o, v_o, _ = oracle.canonicalize_sign(refo["inliers"], refo["v"])
    assert np.allclose(r["v"], v_o, rtol=1e-6, atol=1e-10) and np.allclose(r["w"], refo["w"], rtol=1e-6, atol=1e-10)
    dm_o, _, _ = oracle.scatter_depth(inl_o, *K, rows, cols)
    assert np.array_equal(got != 0, dm_o != 0) and np.allclose(got, dm_o, rtol=1e-6)


def test_solve_frames_dev_on_guarded_planes(rsdsfm):
    """two jobs in one call: each equals rsdsfm_solve_frame_dev with the job's seed on ordinary buffers, bit for bit; a misaligned pointer in
    the SECOND job is refused before the first is enqueued"""
    import torch

    e = _frame_scene(rsdsfm)
    seeds = [99, 100]
    with rsdsfm.Solver(0) as s:
        plains = [_plain_solve(torch, s, e, rsdsfm, sd) for sd in seeds]
        names = [("img1", "double2"), ("dm1", "double"), ("R1", "double"), ("t1", "double"), ("dm0", "double")]
        assert _refusals(rsdsfm, s, lambda A: _run_solve_frames(s, A, e, rsdsfm, seeds), names) == 2 + 4
        A = Args()
        res = _run_solve_frames(s, A, e, rsdsfm, seeds)
        s.synchronize()
        assert A.inputs_unchanged()
        for i in range(2):
            _same_solve(A, str(i), res[i], plains[i])


# =====================================================================================================
# the clip calls' buffers (include/rsdsfm_rectify_video.h: "must be 4-byte aligned"; what becomes a pair's frame job as the frame solve's)
# =====================================================================================================
CLIP = dict(rows=5, cols=6, K=(4.5, 4.5, 3.0, 2.5), gamma=0.8, seeds=[3, 8])
CLIP_SOLVE = [("flow", np.float64, "double2"), ("dm", np.float64, "double"), ("R", np.float64, "double"), ("t", np.float64, "double")]
CLIP_IMAGES = [("gs", np.uint8, "word"), ("fixed", np.uint8, "word"), ("c3", np.float32, "word")]


def _clip_planes(A, rectify):
    """three frames, and per pair every buffer of the clip calls (caller-owned flows and pose tables too), guarded, at its minimum, never preset"""
    rows, cols = CLIP["rows"], CLIP["cols"]
    rng = np.random.default_rng(5)
    d_frames = [A.inp("frame%d" % i, rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8), "word") for i in range(3)]
    shapes = dict(flow=(rows, cols, 2), dm=(cols, rows), R=(rows, 9), t=(rows, 3), prev=(rows, cols), gs=(rows, cols, 3), fixed=(rows, cols, 3), c3=(rows, cols, 3))
    kinds = CLIP_SOLVE + (CLIP_IMAGES if rectify else [])
    outs = {name: [A.out("%s%d" % (name, p), shapes[name], dtype, kind) for p in range(2)] for name, dtype, kind in kinds}
    if rectify:
        outs["prev"] = [A.out("prev%d" % p, shapes["prev"], np.uint8, BYTE_KINDS[p]) for p in range(2)]
    return d_frames, outs


def _run_solve_video(s, A):
    d_frames, o = _clip_planes(A, False)
    return s.solve_video_dev(d_frames, CLIP["rows"], CLIP["cols"], 3, CLIP["K"], CLIP["gamma"], o["dm"], seeds=CLIP["seeds"], d_flows=o["flow"], d_R=o["R"], d_t=o["t"], trials=20)


def _run_rectify_video(s, A):
    d_frames, o = _clip_planes(A, True)
    return s.rectify_video_dev(d_frames, CLIP["rows"], CLIP["cols"], 3, CLIP["K"], CLIP["gamma"], o["dm"], o["prev"], o["gs"], o["fixed"], d_coords=o["c3"], seeds=CLIP["seeds"],
                               d_flows=o["flow"], d_R=o["R"], d_t=o["t"], trials=20, offset=1)


def test_clip_calls_refuse_misaligned_buffers(rsdsfm):
    """rsdsfm_solve_video_dev and rsdsfm_rectify_video_dev on a three-frame clip: a caller-supplied flow field one step below 16 bytes, a depth
    map or a pose table one step below 8, and for the rectifier a frame, an output image or the world points one step below 4, in the first pair
    or the second, is refused before the first pair's flow is enqueued: every buffer of BOTH pairs is still all guard bytes.  Refusals only: what
    the calls compute on buffers at these alignments is the frame solve's and the frame rectifier's above, and the clip pipeline itself is
    tests/test_gpu_video.py's and tests/test_gpu_rectify_video.py's."""
    solve = [("flow0", "double2"), ("flow1", "double2"), ("dm0", "double"), ("dm1", "double"), ("R1", "double"), ("t0", "double")]
    images = [("frame0", "word"), ("frame2", "word"), ("gs1", "word"), ("fixed0", "word"), ("c31", "word")]
    with rsdsfm.Solver(0) as s:
        assert _refusals(rsdsfm, s, lambda A: _run_solve_video(s, A), solve) == 2 * 2 + 4
        assert _refusals(rsdsfm, s, lambda A: _run_rectify_video(s, A), solve + images) == 2 * 2 + 4 + 5 * 2

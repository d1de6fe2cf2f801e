"""CPU: the last frame's definition (tests/last_frame_spec_numpy.py) -- the advance against a second formulation in plain loops over pixels,
its properties (an integer shift moves the map exactly, the smallest of many offers wins whatever their order), the motion against the pose
table's law, the coverage of a model pair, the golden fixture -- and the ABI (include/rsdsfm_last_frame.h): exported by both library
builds, the host-only entry points, the params word, every kernel without a private segment or spills."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import last_frame_cases as cases
import last_frame_spec_numpy as spec
import link_spec_numpy as link_spec
from conftest import ROOT

NEW_SYMBOLS = {"rsdsfm_advance_depth_dev", "rsdsfm_advance_depth_launches", "rsdsfm_last_frame_motion", "rsdsfm_last_frame_dev"}
KERNELS = {"advance_preset_kernel", "advance_splat_kernel", "advance_resolve_kernel"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_last_frame_v1.npz")
ERR_INVALID = -1  # RSDSFM_ERR_INVALID (include/rsdsfm.h)


@pytest.mark.parametrize("shape", cases.CPU_SHAPES)
def test_spec_equals_the_loops_over_pixels(shape):
    rows, cols = shape
    for name in cases.FAMILIES:
        for k, gs in ((0.2, False), (-0.3, True)):
            d = cases.family(name, rows, cols, k)
            got, plane, count = spec.advance_depth(d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"], gs)
            want, n = cases.loop_advance(d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"], gs)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and count == n, (shape, name, k, gs)
            assert count == int((plane != spec.NOTHING).sum()) == int((got != 0).sum())
            assert not np.signbit(got).any() and (spec.valid_depth(got) == (got != 0)).all()
            if name == "empty":
                assert count == 0
    d = cases.family("leaving", rows, cols)
    got = spec.advance_depth(d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"])[0]
    # the first pixel's (-0.5, -0.5) lands on itself, the last pixel's (0.49, 0.49) stays inside
    assert got[0, 0] > 0 and got[rows - 1, cols - 1] > 0


def test_zero_motion_and_an_integer_shift_move_the_map_exactly():
    rows, cols = 17, 33
    d = cases.family("model", rows, cols)
    for dy, dx in ((2, -3), (-1, 4), (0, 1)):
        F = np.empty((rows, cols, 2))
        F[..., 0], F[..., 1] = float(dx), float(dy)
        got, _, count = spec.advance_depth(F, d["Z"], np.zeros(3), np.zeros(3), 0.0, d["K"], d["gamma"])
        want = np.zeros((rows, cols))
        src = d["Z"][max(0, -dy):rows - max(0, dy), max(0, -dx):cols - max(0, dx)]
        want[max(0, dy):rows - max(0, -dy), max(0, dx):cols - max(0, -dx)] = src
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and count == int((want != 0).sum()) > 0


def test_many_offers_to_one_pixel_keep_the_smallest_in_any_order():
    rows, cols = 16, 64
    d = cases.family("one_pixel", rows, cols)
    args = (d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"])
    got, _, count = spec.advance_depth(*args)
    z_pred, r2, c2, inside = link_spec.predict(*args)
    ok = spec.valid_depth(d["Z"]) & inside & spec.valid_depth(z_pred)
    ti, tj = rows // 2, cols // 3
    at = ok & (r2 == ti) & (c2 == tj)
    assert at.sum() > 100 and got[ti, tj] == z_pred[at].min()
    rng = np.random.default_rng(3)
    for _ in range(3):
        want, n = cases.loop_advance(*args, order=rng.permutation(rows * cols))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and n == count


def test_last_frame_motion(rsdsfm):
    v, w = np.array([0.03, -0.02, 0.011]), np.array([0.004, -0.006, 0.009])
    for fn in (spec.last_frame_motion, rsdsfm.last_frame_motion):
        for k in (0.0, -0.0):
            v2, w2, k2 = fn(v, w, k)
            assert np.array_equal(v2.view(np.uint64), v.view(np.uint64)) and np.array_equal(w2.view(np.uint64), w.view(np.uint64))
            assert k2 == 0.0 and np.signbit(k2) == np.signbit(k)
        for k in (0.3, -0.3, 0.05, 1.5, -0.9):
            v2, w2, k2 = fn(v, w, k)
            for s in (0.0, 0.1, 0.37, 0.8, 1.0):  # tau = gamma i / rows of the second frame's scanlines
                second = spec.beta_1(1.0 + s, k) - spec.beta_1(1.0, k)
                assert np.allclose(spec.beta_1(s, k2) * v2, second * v, rtol=0, atol=1e-12), (k, s)
                assert np.allclose(spec.beta_1(s, k2) * w2, second * w, rtol=0, atol=1e-12), (k, s)
    for k in (0.3, -0.3, 1.5):  # the library against the spec, to rounding
        a, b = rsdsfm.last_frame_motion(v, w, k), spec.last_frame_motion(v, w, k)
        assert np.allclose(a[0], b[0], rtol=1e-15, atol=0) and np.allclose(a[1], b[1], rtol=1e-15, atol=0) and abs(a[2] - b[2]) <= 1e-16
    for bad in ((v, w, -1.0), (v, w, -1.5), (v, w, np.nan), (v * np.inf, w, 0.1), (v, w * np.nan, 0.1)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.last_frame_motion(*bad)
        with pytest.raises(ValueError):
            spec.last_frame_motion(*bad)
    lib = rsdsfm.load_library()
    v3, k_out = (ctypes.c_double * 3)(1.0, 2.0, 3.0), ctypes.c_double()
    assert lib.rsdsfm_last_frame_motion(None, v3, ctypes.c_double(0.0), v3, v3, ctypes.byref(k_out)) == ERR_INVALID
    assert lib.rsdsfm_last_frame_motion(v3, v3, ctypes.c_double(0.0), v3, v3, None) == ERR_INVALID


def test_coverage_of_a_model_pair(rsdsfm):
    """the advance of the true depth of a model pair with 3 px of flow covers 95.1 % of the frame (the rest: the band the second frame sees
    and the first did not, and the cracks where the field stretches); of a map with 30 % holes (this file's draw of them), 95.6 % as many pixels as the map holds"""
    d = cases.coverage_scene(rsdsfm.synth)
    rows, cols = d["Z"].shape
    _, _, full = spec.advance_depth(d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"])
    _, _, holed = spec.advance_depth(d["F"], d["Z_holed"], d["v"], d["w"], d["k"], d["K"], d["gamma"])
    held = int((d["Z_holed"] != 0).sum())
    print("coverage: %.4f of the frame; %.4f of the %d pixels the holed map holds" % (full / (rows * cols), holed / held, held))
    assert full >= cases.COVERAGE_BOUND * rows * cols
    assert holed >= cases.COVERAGE_BOUND * held


def test_golden_fixture():
    g = np.load(GOLDEN)
    keys = [k[:-len("params")] for k in g.files if k.endswith("/params")]
    assert len(keys) == 3
    for key in keys:
        name, size = key.split("/")[:2]
        rows, cols = (int(x) for x in size.split("x"))
        k, gs = g[key + "params"]
        d = cases.family(name, rows, cols, float(k))
        got, _, count = spec.advance_depth(d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"], bool(gs))
        assert np.array_equal(got.view(np.uint64), g[key + "map"].view(np.uint64)) and count == int(g[key + "count"]) > 0, key
    for k in (0.0, 0.3, -0.3):
        v, w, kk = spec.last_frame_motion([0.03, -0.02, 0.01], [0.004, -0.006, 0.009], k)
        assert np.array_equal(np.concatenate([v, w, [kk]]), g["motion/%r" % k])
    assert os.path.getsize(GOLDEN) <= 32 * 1024


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_last_frame_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.last_frame_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols(),
                  rsdsfm.fuse_declared_symbols(), rsdsfm.stabilize_declared_symbols(), rsdsfm.stabilize_fill_declared_symbols(),
                  rsdsfm.stabilize_crop_declared_symbols(), rsdsfm.stabilize_blend_declared_symbols(), rsdsfm.stabilize_inpaint_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    for name in ("advance_depth", "advance_depth_dev", "last_frame_dev"):
        assert callable(getattr(rsdsfm.Solver, name))


def test_params_word_and_host_entry_points(rsdsfm):
    """`last_frame` is the word that was `reserved`: same offset, same size, still answered under the old name, 0 from the init call"""
    P = rsdsfm.StabilizeParams
    assert ctypes.sizeof(P) == 24 and P.last_frame.offset == 20 and P.last_frame.size == 4
    p = P()
    assert rsdsfm.load_library().rsdsfm_stabilize_params_init(ctypes.byref(p)) == 0
    assert p.last_frame == 0 and p.reserved == 0 and p.struct_bytes == 24
    p.last_frame = 1
    assert p.reserved == 1
    hdr = open(rsdsfm.STABILIZE_HEADER_PATH).read()
    assert re.search(r"int32_t\s+last_frame;", hdr) and not re.search(r"int32_t\s+reserved;", hdr)
    # a value other than 0 and 1 is refused wherever the params are checked (the path smoother is host only)
    A, c = np.tile(np.eye(3).reshape(1, 9), (3, 1)), np.zeros((3, 3))
    out_A, out_c = np.empty_like(A), np.empty_like(c)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib = rsdsfm.load_library()
    for value, rc in ((0, 0), (1, 0), (2, ERR_INVALID), (-1, ERR_INVALID)):
        p.last_frame = value
        assert lib.rsdsfm_smooth_path(ptr(A), ptr(c), ctypes.c_int32(3), ctypes.byref(p), ptr(out_A), ptr(out_c)) == rc
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.advance_depth_launches(r, c_)
    for r, c_ in ((2, 2), (96, 128), (720, 1280), (16384, 16384)):
        assert rsdsfm.advance_depth_launches(r, c_) == 3
    v3 = (ctypes.c_double * 3)()
    i32, f64 = ctypes.c_int32, ctypes.c_double
    assert lib.rsdsfm_advance_depth_dev(None, None, None, v3, v3, f64(0), i32(8), i32(8), f64(1), f64(1), f64(0), f64(0), f64(0.8), i32(0), None, None, None) == ERR_INVALID
    assert lib.rsdsfm_last_frame_dev(None, None, None, v3, v3, f64(0), i32(8), i32(8), f64(1), f64(1), f64(0), f64(0), f64(0.8), i32(0), None, None, None, None,
                                     None) == ERR_INVALID  # no context


def test_last_frame_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of last_frame_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_inpaint_cpu.py reads the inpaint's): a
    zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "last_frame_kernels.hip")
    out = tmp_path / "last_frame_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    entries = re.split(r"\n  - (?=\.)", txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")])[1:]  # one YAML list item per kernel
    field = lambda e, k: re.search(r"^\s*\.%s:\s+(\S+)\s*$" % k, e, flags=re.M).group(1)
    kernels = {field(e, "name"): tuple(int(field(e, k)) for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
               for e in entries}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert names == KERNELS and len(kernels) == 3, (sorted(kernels), sorted(names))
    for k in KERNELS:
        assert any(k in n for n in kernels), k
    bad = {n: m for n, m in kernels.items() if m[1:] != (0, 0, 0) or m[0] > 65536}
    assert not bad, bad
    print({n: (m, field(e, "vgpr_count"), field(e, "sgpr_count")) for (n, m), e in zip(kernels.items(), entries)})

"""CPU: the inpainting's definition (tests/stabilize_inpaint_spec_numpy.py) -- the vectorised spec against a second formulation in plain
loops over cells, its properties (set pixels kept, every output inside the set pixels' range, a constant stays the constant, one set pixel
floods the frame, channels independent, any non-zero mask byte is "set"), its accuracy against the mean of the set pixels on four holes in a
smooth texture, the golden fixture -- and the ABI (include/rsdsfm_stabilize_inpaint.h): exported by both library builds, the host-only entry
point, every kernel without a private segment or spills."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stabilize_inpaint_cases as cases
import stabilize_inpaint_spec_numpy as spec
from conftest import ROOT

NEW_SYMBOLS = {"rsdsfm_inpaint_frame_dev", "rsdsfm_inpaint_launches", "rsdsfm_stabilize_video_inpainted_dev"}
KERNELS = {"inpaint_pull0_kernel", "inpaint_pull_kernel", "inpaint_small_kernel", "inpaint_push_kernel", "inpaint_write_kernel"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_stabilize_inpaint_v1.npz")
ERR_INVALID = -1  # RSDSFM_ERR_INVALID (include/rsdsfm.h)


def _run(image, mask, fn=spec.inpaint):
    out, source = image.copy(), np.zeros(mask.shape, dtype=np.uint8)
    keep = mask.copy()
    count = fn(out, mask, source)
    assert np.array_equal(mask, keep)  # only read
    return out, source, count


def test_constants():
    assert spec.SOURCE_INPAINTED == 255


@pytest.mark.parametrize("shape", cases.CPU_SIZES)
def test_spec_equals_the_loops_over_cells(shape):
    rows, cols = shape
    for ch in (1, 3):
        image = cases.image_of(rows, cols, ch, 10 * rows + cols + ch)
        for name, mask in cases.masks(rows, cols, rows + cols):
            got, want = _run(image, mask), _run(image, mask, cases.loop_inpaint)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (shape, ch, name)
            empty = mask == 0
            assert got[2] == (int(empty.sum()) if (mask != 0).any() else 0)
            assert np.array_equal(got[1], np.where(empty & (got[2] > 0), spec.SOURCE_INPAINTED, 0))


@pytest.mark.parametrize("shape", cases.CPU_SIZES + [(2, 4099), (67, 130), (720, 1280)])
def test_properties(shape):
    """set pixels byte-identical; every output channel within [min, max] of that channel over the set pixels; a full mask is the identity
    with count 0; an empty mask changes nothing with count 0; a constant image inpaints to the constant; one set pixel floods the frame"""
    rows, cols = shape
    for ch in (1, 3):
        image = cases.image_of(rows, cols, ch, rows + 7 * cols + ch)
        flat = image.reshape(rows, cols, ch)
        for name, mask in cases.masks(rows, cols, 3 * rows + cols):
            out, source, count = _run(image, mask)
            seen = mask != 0
            assert np.array_equal(out[seen], image[seen]), (shape, ch, name)
            if name == "set" or not seen.any():  # nothing to fill, or nothing to fill from
                assert count == 0 and np.array_equal(out, image) and not source.any()
                continue
            else:
                assert count == rows * cols - int(seen.sum()) and (source[~seen] == spec.SOURCE_INPAINTED).all() and not source[seen].any()
                o = out.reshape(rows, cols, ch)
                for c in range(ch):
                    assert flat[seen][:, c].min() <= o[..., c].min() and o[..., c].max() <= flat[seen][:, c].max(), (shape, ch, name, c)
            if name == "last":
                assert count == rows * cols - 1 and (o == flat[rows - 1, cols - 1]).all()
            if name in ("bands", "random-255"):
                const = np.empty_like(image)
                const.reshape(rows, cols, ch)[:] = np.array([7, 130, 255])[:ch]
                got = _run(const, mask)
                assert np.array_equal(got[0], const) and got[2] == count


def test_three_channels_are_three_gray_images():
    for shape in ((7, 5), (33, 70)):
        image = cases.image_of(*shape, 3, 5)
        for name, mask in cases.masks(*shape, 9):
            out, _, count = _run(image, mask)
            for c in range(3):
                g = _run(np.ascontiguousarray(image[..., c]), mask)
                assert np.array_equal(g[0], out[..., c]) and g[2] == count, (shape, name, c)


def test_any_non_zero_mask_byte_is_set():
    image = cases.image_of(33, 70, 3, 2)
    mask = cases.masks(33, 70, 4)[3][1]
    a, b = _run(image, mask), _run(image, (mask * 255).astype(np.uint8))
    assert mask.max() == 1 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] > 0


@pytest.mark.parametrize("name,hole", cases.ACC_HOLES)
def test_accuracy_against_the_mean_fill(name, hole):
    """the blend's exposure texture (smooth, in [6, 200]) at 96 x 128 with one hole: the mean absolute error of the inpainted pixels against
    the texture must be below that of the hole filled with the rounded mean of the set pixels, a baseline that shares nothing with the code
    under test.  The spec's values ("Inpaint"): 12.7 / 20.2, 5.9 / 81.5, 14.3 / 30.9, 5.2 / 19.6."""
    texture, image, mask = cases.accuracy_case(hole)
    out, _, count = _run(image, mask)
    empty = mask == 0
    base = float(np.rint(image[~empty].astype(np.float64).mean()))
    err = np.abs(out[empty].astype(np.float64) - texture[empty]).mean()
    err_base = np.abs(base - texture[empty]).mean()
    print("%s: %d pixels, inpaint %.2f, mean fill %.2f" % (name, count, err, err_base))
    assert count == int(empty.sum()) > 0
    assert err < err_base


def test_golden_fixture():
    g = np.load(GOLDEN)
    keys = [k[:-len("params")] for k in g.files if k.endswith("/params")]
    assert len(keys) == 3
    for key in keys:
        rows, cols, ch = (int(x) for x in key[:-1].split("x"))
        seed, family = (int(x) for x in g[key + "params"])
        image, mask = cases.image_of(rows, cols, ch, seed), cases.masks(rows, cols, seed)[family][1]
        assert np.array_equal(np.packbits(mask != 0), g[key + "mask"]), key
        out, source, count = _run(image, mask)
        assert np.array_equal(out, g[key + "out_image"]) and np.array_equal(np.packbits(source != 0), g[key + "out_source"]) and count == int(g[key + "out_count"]) > 0, key
    assert os.path.getsize(GOLDEN) <= 22 * 1024


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_stabilize_inpaint_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.stabilize_inpaint_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols(),
                  rsdsfm.fuse_declared_symbols(), rsdsfm.stabilize_declared_symbols(), rsdsfm.stabilize_fill_declared_symbols(),
                  rsdsfm.stabilize_crop_declared_symbols(), rsdsfm.stabilize_blend_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    assert rsdsfm.INPAINT_SOURCE == spec.SOURCE_INPAINTED == 255
    assert re.search(r"#define\s+RSDSFM_SOURCE_INPAINTED\s+255\b", open(rsdsfm.STABILIZE_INPAINT_HEADER_PATH).read())
    for name in ("inpaint", "inpaint_frame_dev", "stabilize_video_inpainted_dev"):
        assert callable(getattr(rsdsfm.Solver, name))


def _launches(rows, cols, capacity=8160):
    """level 0 -> 1, the large pulls, ONE workgroup from the first level S >= 1 from which everything up to 1 x 1 is at most `capacity` cells,
    the large pushes, the output"""
    cells, h, w = [], rows, cols
    while h > 1 or w > 1:
        h, w = (h + 1) // 2, (w + 1) // 2
        cells.append(h * w)
    small = min(i for i in range(len(cells)) if sum(cells[i:]) <= capacity)
    return 3 if small == 0 else 1 + (small - 1) + 1 + small + 1


def test_host_entry_points(rsdsfm):
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.inpaint_launches(r, c_)
    # level 0 -> 1, the large pulls, the single-workgroup launch (everything from its level up is at most 8160 cells), the large pushes, the output
    for (r, c_), n in (((2, 2), 3), ((129, 67), 3), ((2, 4099), 3), ((401, 603), 6), ((720, 1280), 8), ((16384, 16384), 16)):
        assert rsdsfm.inpaint_launches(r, c_) == n == _launches(r, c_), (r, c_)
    for r, c_ in ((127, 128), (129, 128), (180, 181), (181, 181), (300, 400), (1080, 1920), (2, 16384)):
        assert rsdsfm.inpaint_launches(r, c_) == _launches(r, c_), (r, c_)
    assert rsdsfm.inpaint_launches(720, 1280) == rsdsfm.rectify_dense_launches(720, 1280) - 1  # stage A's structure: the dense call's map and warp against one output launch
    lib = rsdsfm.load_library()
    assert lib.rsdsfm_inpaint_frame_dev(None, None, None, ctypes.c_int32(1), ctypes.c_int32(8), ctypes.c_int32(8), None, None) == ERR_INVALID  # no context


def test_stabilize_inpaint_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of stabilize_inpaint_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_blend_cpu.py reads the blend's):
    the three plain kernels and both instances of the two templates, a zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "stabilize_inpaint_kernels.hip")
    out = tmp_path / "stabilize_inpaint_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    entries = re.split(r"\n  - (?=\.)", txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")])[1:]  # one YAML list item per kernel
    field = lambda e, k: re.search(r"^\s*\.%s:\s+(\S+)\s*$" % k, e, flags=re.M).group(1)
    kernels = {field(e, "name"): tuple(int(field(e, k)) for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
               for e in entries}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert names == KERNELS and len(kernels) == 7, (sorted(kernels), sorted(names))
    for k in KERNELS:
        assert any(k in n for n in kernels), k
    bad = {n: m for n, m in kernels.items() if m[1:] != (0, 0, 0) or m[0] > 65536}
    assert not bad, bad
    print({n: (m, field(e, "vgpr_count"), field(e, "sgpr_count")) for (n, m), e in zip(kernels.items(), entries)})

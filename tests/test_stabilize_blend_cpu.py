"""CPU: the seam blend's definition (tests/stabilize_blend_spec_numpy.py) -- the separable distance against the brute-force definition, the
layer call's properties (feather 1 with the gain off is the hard fill, a pixel a nearer candidate has never changes, the gains' clamps and
their overlap threshold), its accuracy on an exposure step, the golden fixture -- synth.render_sequence's exposure factors, and the ABI
(include/rsdsfm_stabilize_blend.h): exported by both library builds, the host-only entry points, every kernel without a private segment or
spills."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stabilize_blend_cases as cases
import stabilize_blend_spec_numpy as spec
import stabilize_crop_spec_numpy as crop
from conftest import ROOT

NEW_SYMBOLS = {"rsdsfm_stabilize_blend_params_init", "rsdsfm_seam_distance_dev", "rsdsfm_seam_distance_launches", "rsdsfm_seam_blend_layer_dev",
               "rsdsfm_seam_blend_layer_launches", "rsdsfm_seam_gains", "rsdsfm_stabilize_video_blended_dev"}
KERNELS = {"seam_distance_rows_kernel", "seam_distance_cols_kernel", "seam_overlap_sums_kernel", "seam_blend_kernel"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_stabilize_blend_v1.npz")
ERR_INVALID = -1  # RSDSFM_ERR_INVALID (include/rsdsfm.h)


def test_constants():
    assert (spec.FEATHER_DEFAULT, spec.MIN_OVERLAP_DEFAULT, spec.GAIN_MIN, spec.GAIN_ONE, spec.GAIN_MAX) == (16, 1024, 16384, 65536, 262144)


# ---------------------------------------------------------------------------------------------------
# the distance
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 5), (20, 33), (5, 40), (12, 12), (9, 9)])
def test_separable_distance_equals_the_brute_force_definition(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    masks = [np.ones(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)]
    masks += [np.where(rng.random(shape) < e, 0, v).astype(np.uint8) for e, v in ((0.02, 1), (0.1, 255), (0.5, 1))]
    one = np.ones(shape, dtype=np.uint8)
    one[shape[0] - 1, 0] = 0
    masks.append(one)
    for T in (1, 3, 4, 16, 64):
        for m in masks:
            d = spec.seam_distance(m, T)
            assert d.dtype == np.uint8 and np.array_equal(d, cases.brute_distance(m, T)), (shape, T)
            assert not d[m == 0].any() and (d[m != 0] >= 1).all() and d.max() <= T
    assert (spec.seam_distance(masks[0], 16) == 16).all() and not spec.seam_distance(masks[1], 16).any()  # the frame's edge is not a hole


# ---------------------------------------------------------------------------------------------------
# one layer
# ---------------------------------------------------------------------------------------------------
def test_feather_one_without_gain_is_the_hard_fill(oracle):
    """T = 1, gain off: blend_layer of a candidate rendered alone equals fill_from_window of the candidate on the same planes"""
    cc = cases.clip_case(oracle.pose_table, 33, 70, channels=3)
    window = (0, 0, 33, 70)
    q, n = 1, 0
    out = np.zeros_like(cc["images"][q])
    mask, source = np.zeros((33, 70), dtype=np.uint8), np.zeros((33, 70), dtype=np.uint8)
    crop.fill_from_window(out, mask, source, cc["images"][q], cc["depths"][q], cc["Rs"][q], cc["ts"][q], cc["K"], cc["M"][q], cc["m"][q], 1, window)
    M, m = crop.fill.neighbour_pose(cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, n)
    want = [a.copy() for a in (out, mask, source)]
    taken = crop.fill_from_window(*want, cc["images"][n], cc["depths"][n], cc["Rs"][n], cc["ts"][n], cc["K"], M, m, 2, window)
    layer, lmask = np.zeros_like(out), np.zeros_like(mask)
    crop.fill_from_window(layer, lmask, np.zeros_like(mask), cc["images"][n], cc["depths"][n], cc["Rs"][n], cc["ts"][n], cc["K"], M, m, 2, window)
    dist = spec.seam_distance(mask, 1)
    G = spec.gains(spec.overlap_sums(out, source, layer, lmask), 3, 1, gain_mode=1)
    assert G == [spec.GAIN_ONE] * 3
    got = [a.copy() for a in (out, mask, source)]
    assert spec.blend_layer(*got, dist, 1, layer, lmask, 2, G) == (taken, 0) and taken > 0
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_layer_properties():
    """a pixel with source >= 2 never changes; source 1 with dist >= T never changes; a pixel under an empty layer mask never changes; a
    blended pixel gets the id and keeps its mask; the counters are the changes"""
    for ch, T in ((1, 16), (3, 4)):
        e = cases.layer_case(33, 70, ch, 7 + ch, T)
        image, mask, source = e["image"].copy(), e["mask"].copy(), e["source"].copy()
        G = spec.gains(spec.overlap_sums(image, source, e["layer"], e["lmask"]), ch, 1)
        filled, blended = spec.blend_layer(image, mask, source, e["dist"], T, e["layer"], e["lmask"], 9, G)
        keep = (e["source"] >= 2) | (e["lmask"] == 0) | ((e["source"] == 1) & (e["dist"] >= T))
        assert np.array_equal(image[keep], e["image"][keep]) and np.array_equal(source[keep], e["source"][keep]) and np.array_equal(mask[keep], e["mask"][keep])
        assert filled == ((e["source"] == 0) & (e["lmask"] != 0)).sum() > 0 and blended == ((e["source"] == 1) & (e["dist"] < T) & (e["lmask"] != 0)).sum() > 0
        assert (source == 9).sum() == filled + blended and mask.sum() == e["mask"].sum() + filled and keep.sum() > 0


def test_gains_clamp_and_need_an_overlap():
    s = lambda count, si, sl: np.array([count, si, sl, 0, 0, 0, 0, 0], dtype=np.uint64)
    assert spec.gains(s(2000, 2000 * 255, 2000), 1) == [spec.GAIN_MAX]         # a layer of 1s under 255s
    assert spec.gains(s(2000, 2000, 2000 * 255), 1) == [spec.GAIN_MIN]         # the reverse
    assert spec.gains(s(2000, 3000, 2000), 1) == [98304]                       # 1.5
    assert spec.gains(s(2000, 1000, 3000), 1) == [(1000 * 65536 + 1500) // 3000]
    assert spec.gains(s(1023, 3000, 2000), 1) == [spec.GAIN_ONE]               # under min_overlap
    assert spec.gains(s(1024, 3000, 2000), 1) == [98304]
    assert spec.gains(s(2000, 3000, 0), 1) == [spec.GAIN_ONE]                  # nothing to divide by
    assert spec.gains(s(2000, 3000, 2000), 1, gain_mode=1) == [spec.GAIN_ONE]  # off
    three = np.array([5000, 100, 200, 300, 100, 100, 100, 0], dtype=np.uint64)
    assert spec.gains(three, 3) == [65536, 131072, 196608]
    big = s(1 << 28, 255 << 28, 1 << 28)  # 16384 x 16384 of 255 over 1: 64 bits hold it
    assert spec.gains(big, 1) == [spec.GAIN_MAX]


@pytest.mark.parametrize("g", cases.ACC_GAINS)
def test_accuracy_on_an_exposure_step(g):
    """a smooth texture in [6, 200] as the own frame, empty in a band, and the texture times g, rounded, as the layer; 96 x 128, T = 16.
    Every output pixel within 2 grey levels of the texture -- derived, not tuned: the layer's rounding (0.5) times G / 65536 <= 1.25, plus the
    two roundings of 0.5 each -- and the gain within 0.1 % of 65536 / g.  The hard fill's step at the seam on the same inputs is printed."""
    e = cases.exposure_case(g)
    image, mask, source = e["image"].copy(), e["mask"].copy(), e["source"].copy()
    sums = spec.overlap_sums(image, source, e["layer"], e["lmask"])
    G = spec.gains(sums, 1)
    assert int(sums[0]) == int(e["mask"].sum()) >= spec.MIN_OVERLAP_DEFAULT
    filled, blended = spec.blend_layer(image, mask, source, e["dist"], e["T"], e["layer"], e["lmask"], 2, G)
    err = np.abs(image.astype(np.float64) - e["texture"]).max()
    hard = np.where(e["mask"] == 1, e["image"], e["layer"]).astype(np.float64)
    step = np.abs(hard[:, 39] - hard[:, 40]).max()
    print("g %.1f: G %d (65536 / g = %.1f), filled %d, blended %d, max error %.3f, the hard fill's step %.0f" % (g, G[0], 65536 / g, filled, blended, err, step))
    assert mask.all() and filled == 96 * 24 and blended == 96 * 2 * 15
    assert abs(G[0] - 65536 / g) <= 0.001 * 65536 / g
    assert err <= 2.0


def test_golden_fixture():
    g = np.load(GOLDEN)
    import oracle_py

    for key in [k[:-len("params")] for k in g.files if k.endswith("/params") and k.startswith("mask")]:
        rows, cols = (int(x) for x in key[4:-1].split("x"))
        seed, T = (int(x) for x in g[key + "params"])
        m = cases.random_masks(rows, cols, 1, float(g[key + "empty"]), seed)[0]
        assert np.array_equal(np.packbits(m != 0), g[key + "mask"]) and np.array_equal(spec.seam_distance(m, T), g[key + "dist"]), key
    n = 0
    for key in [k[:-len("modes")] for k in g.files if k.endswith("/modes")]:
        rows, cols, _ = (int(x) for x in key[:-1].split("x"))
        ch, q, radius, mode, q5, it, T, min_overlap, gain_mode = (int(x) for x in g[key + "modes"])
        cc = cases.clip_case(oracle_py.pose_table, rows, cols, channels=ch)
        r = spec.blend_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q], cc["m"][q],
                             tuple(int(x) for x in g[key + "window"]), radius=radius, T=T, min_overlap=min_overlap, gain_mode=gain_mode, mode=mode, q5_mode=q5,
                             iterations=it)
        for name in ("image", "mask", "source", "dist", "gains", "sums"):
            assert np.array_equal(r[name], g[key + "out_" + name]), (key, name)
        assert r["counts"] == g[key + "out_counts"].tolist() and sum(r["counts"]) == rows * cols
        n += sum(r["counts"][3::2])
    assert n > 1000  # pixels were blended


# ---------------------------------------------------------------------------------------------------
# the synthetic clip's exposure
# ---------------------------------------------------------------------------------------------------
def test_render_sequence_gains(rsdsfm):
    rows, cols = 24, 32
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    plain = rsdsfm.synth.render_sequence(3, rows, cols, K, v, w, k, 0.8, seed=21)
    none = rsdsfm.synth.render_sequence(3, rows, cols, K, v, w, k, 0.8, seed=21, gains=None)
    ones = rsdsfm.synth.render_sequence(3, rows, cols, K, v, w, k, 0.8, seed=21, gains=[1.0, 1.0, 1.0])
    got = rsdsfm.synth.render_sequence(3, rows, cols, K, v, w, k, 0.8, seed=21, gains=[1.0, 1.1, 3.0])
    sp = rsdsfm.synth.render_sequence(3, rows, cols, K, v, w, k, 0.8, seed=21, speeds=(1.0, 1.4), gains=[0.9, 1.0, 1.0])
    sp0 = rsdsfm.synth.render_sequence(3, rows, cols, K, v, w, k, 0.8, seed=21, speeds=(1.0, 1.4))
    for a, b in zip(plain, none):
        assert np.array_equal(a, b)
    assert np.array_equal(ones[0], plain[0]) and np.array_equal(got[0][0], plain[0][0]) and np.array_equal(got[1], plain[1])
    assert np.abs(got[0][1].astype(np.float64) - 1.1 * plain[0][1]).max() <= 1.05 + 1e-9 or (got[0][1] == 255).any()  # the factor before the rounding
    assert got[0][2].max() == 255 and got[0].dtype == np.uint8                                                       # clipped, not wrapped
    assert np.array_equal(sp[0][1:], sp0[0][1:]) and not np.array_equal(sp[0][0], sp0[0][0])
    with pytest.raises(ValueError):
        rsdsfm.synth.render_sequence(3, rows, cols, K, v, w, k, 0.8, gains=[1.0, 1.0])


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_stabilize_blend_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.stabilize_blend_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols(),
                  rsdsfm.fuse_declared_symbols(), rsdsfm.stabilize_declared_symbols(), rsdsfm.stabilize_fill_declared_symbols(),
                  rsdsfm.stabilize_crop_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    assert rsdsfm.stabilize_blend_default_params() == dict(feather=spec.FEATHER_DEFAULT, gain_mode=0, min_overlap=spec.MIN_OVERLAP_DEFAULT)
    assert ctypes.sizeof(rsdsfm.StabilizeBlendParams) == 32 and rsdsfm.GAIN_ONE == spec.GAIN_ONE
    p = rsdsfm.StabilizeBlendParams()
    assert lib.rsdsfm_stabilize_blend_params_init(None) != rsdsfm.OK
    assert lib.rsdsfm_stabilize_blend_params_init(ctypes.byref(p)) == rsdsfm.OK
    assert (p.min_overlap, p.feather, p.gain_mode, p.struct_bytes, list(p.reserved)) == (1024, 16, 0, 32, [0, 0, 0])
    assert os.path.exists(rsdsfm.STABILIZE_BLEND_HEADER_PATH)
    for name in ("seam_distance_dev", "seam_distance", "seam_blend_layer_dev", "stabilize_video_blended_dev"):
        assert callable(getattr(rsdsfm.Solver, name))


def test_host_entry_points(rsdsfm):
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.seam_distance_launches(r, c_)
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.seam_blend_layer_launches(r, c_)
    for r, c_ in ((2, 2), (300, 400), (720, 1280), (16384, 16384)):
        assert rsdsfm.seam_distance_launches(r, c_) == 2 and rsdsfm.seam_blend_layer_launches(r, c_) == 2
    rng = np.random.default_rng(3)
    for ch in (1, 3):
        for _ in range(50):  # the host's gains are the spec's, whatever the record
            rec = np.zeros(8, dtype=np.uint64)
            rec[0] = rng.integers(0, 4000)
            rec[1:1 + 2 * ch] = rng.integers(0, 1 << int(rng.integers(1, 36)), size=2 * ch)
            for min_overlap, mode in ((0, 0), (1, 0), (3000, 0), (0, 1)):
                want = spec.gains(rec, ch, min_overlap or spec.MIN_OVERLAP_DEFAULT, mode) + [spec.GAIN_ONE] * (3 - ch)
                assert rsdsfm.seam_gains(rec, ch, min_overlap, mode).tolist() == want
    big = np.array([1 << 28, 255 << 28, 1 << 28, 0, 0, 0, 0, 0], dtype=np.uint64)
    assert rsdsfm.seam_gains(big, 1).tolist() == [spec.GAIN_MAX, spec.GAIN_ONE, spec.GAIN_ONE]
    for bad in (dict(channels=2), dict(min_overlap=-1), dict(gain_mode=2)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.seam_gains(big, **dict(dict(channels=1, min_overlap=0, gain_mode=0), **bad))
    lib = rsdsfm.load_library()
    assert lib.rsdsfm_seam_gains(None, 1, ctypes.c_int64(0), 0, None) == ERR_INVALID
    assert lib.rsdsfm_seam_distance_dev(None, None, ctypes.c_int32(8), ctypes.c_int32(8), ctypes.c_int32(16), None) == ERR_INVALID  # no context
    assert lib.rsdsfm_seam_blend_layer_dev(None, None, None, ctypes.c_int32(1), ctypes.c_int32(8), ctypes.c_int32(8), None, None, ctypes.c_int32(2), None, None, None,
                                           None, None) == ERR_INVALID


def test_stabilize_blend_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of stabilize_blend_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_crop_cpu.py reads the crop's): the
    two distance kernels and both instances of the two templates, a zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "stabilize_blend_kernels.hip")
    out = tmp_path / "stabilize_blend_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    entries = re.split(r"\n  - (?=\.)", txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")])[1:]  # one YAML list item per kernel
    field = lambda e, k: re.search(r"^\s*\.%s:\s+(\S+)\s*$" % k, e, flags=re.M).group(1)
    kernels = {field(e, "name"): tuple(int(field(e, k)) for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
               for e in entries}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert names == KERNELS and len(kernels) == 6, (sorted(kernels), sorted(names))
    for k in KERNELS:
        assert any(k in n for n in kernels), k
    bad = {n: m for n, m in kernels.items() if m[1:] != (0, 0, 0) or m[0] > 65536}
    assert not bad, bad
    print({n: (m, field(e, "vgpr_count"), field(e, "sgpr_count")) for (n, m), e in zip(kernels.items(), entries)})

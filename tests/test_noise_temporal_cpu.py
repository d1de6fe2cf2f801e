"""GPU-free tests of the temporal noise curve (include/rsdsfm_noise_temporal.h): the definition (tests/noise_temporal_spec_numpy.py) against the
golden fixture, against a loop per pixel and against the properties that follow from it; the estimator on denoise_cases' noisy shift clip --
it follows the noise where the frame's own spatial curve measures the texture --, the denoise at its strength, and the plate's mover; the
kernel's resources from hipcc's metadata; the exported symbols, the launch counts and the host-side refusals; and the no-argtypes marshalling
of rsdsfm_noise_temporal.py on the recording library."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import binding_recorder as rec  # noqa: E402
import noise_curve_spec_numpy as cspec  # noqa: E402
import noise_temporal_binding_cases as bcases  # noqa: E402
import noise_temporal_cases as cases  # noqa: E402
import noise_temporal_spec_numpy as spec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_noise_temporal_v1.npz")
GOLDEN_CALLS = os.path.join(ROOT, "tests", "golden", "noise_temporal_calls_v1.json.gz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_noise_temporal.h")).read()
NEW_SYMBOLS = {"rsdsfm_noise_pair_hist_dev", "rsdsfm_noise_pair_hist_launches", "rsdsfm_noise_curve_resolve_dev", "rsdsfm_noise_curve_resolve_launches",
               "rsdsfm_denoise_temporal_frame_dev", "rsdsfm_denoise_temporal_frame_launches", "rsdsfm_denoise_temporal_video_dev"}
ERR_INVALID = -1


@pytest.fixture(scope="module")
def nt(rsdsfm):
    import rsdsfm_noise_temporal

    return rsdsfm_noise_temporal


def _dense(pairs):
    hist = np.zeros(spec.BANDS * spec.BINS, dtype=np.uint32)
    hist[pairs[:, 0]] = pairs[:, 1]
    return hist.reshape(spec.BANDS, spec.BINS)


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture():
    g = np.load(GOLDEN)
    golden = cases.golden_cases()
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in golden} | {"frame"}
    assert {c["kind"] for c in golden} == set(cases.PAIR_KINDS)
    for case in golden:
        n = case["name"] + "/"
        for k in ("ref", "rmask", "layer", "lmask"):
            assert np.array_equal(g[n + k], case[k]), n + k
        assert np.array_equal(spec.pair_histogram(g[n + "ref"], g[n + "rmask"], g[n + "layer"], g[n + "lmask"]), _dense(g[n + "hist"])), n
    m = cases.shift_measure(3, 6, 0)
    ref, rmask, _ = m["run"]["ref"]
    assert np.array_equal(g["frame/ref"], ref) and np.array_equal(g["frame/rmask"], rmask) and np.array_equal(g["frame/records"], m["run"]["records"])
    layers = [(g["frame/layer%d" % j], g["frame/lmask%d" % j]) for j in range(4)]
    r = spec.noise_temporal(g["frame/ref"], g["frame/rmask"], layers, list(g["frame/records"]))
    assert np.array_equal(r["hist"], _dense(g["frame/hist"])) and r["curve"].tolist() == g["frame/curve"].tolist() and int(r["curve"][8, 0]) > 1024
    assert os.path.getsize(GOLDEN) <= 128 * 1024


def _loop(ref, rmask, layer, lmask, G):
    """the definition once more, a literal loop per pixel"""
    R, L = spec.temporal._planes(ref).astype(np.int64), spec.temporal._planes(layer).astype(np.int64)
    rows, cols, ch = R.shape
    hist = np.zeros((spec.BANDS, spec.BINS), dtype=np.uint32)
    for y in range(1, rows - 1):
        for x in range(1, cols - 1):
            D, ok = 0, True
            for yy in range(y - 1, y + 2):
                for xx in range(x - 1, x + 2):
                    ok = ok and rmask[yy, xx] != 0 and lmask[yy, xx] != 0
                    for c in range(ch):
                        r, l = int(R[yy, xx, c]), int(L[yy, xx, c])
                        ok = ok and r not in (0, 255) and l not in (0, 255)
                        D += abs(r - min(255, (G[c] * l + 32768) >> 16))
            if ok:
                level = int(R[y, x, 0]) if ch == 1 else (int(R[y, x].sum()) + 1) // 3
                hist[level >> 5, (918 * D + 128 * 9 * ch) // (256 * 9 * ch)] += 1
    return hist


def test_the_definition_equals_a_loop_per_pixel():
    small = [c for c in cases.pair_cases() if c["ref"].shape[0] * c["ref"].shape[1] <= 17 * 65]
    assert {c["kind"] for c in small} == set(cases.PAIR_KINDS)
    for k, case in enumerate(small):
        ch = 1 if case["ref"].ndim == 2 else 3
        record = None
        if k % 3 == 1:  # a gain other than 1: [count, sums of the image, sums of the layer]
            record = np.zeros(8, dtype=np.uint64)
            record[0], record[1:1 + ch], record[1 + ch:1 + 2 * ch] = 5000, [1100, 900, 1000][:ch], [1000, 1000, 1001][:ch]
        G = spec.temporal.gains(record, ch)
        assert (record is None) == (G == [65536] * ch)
        want = _loop(case["ref"], case["rmask"], case["layer"], case["lmask"], G)
        assert np.array_equal(spec.pair_histogram(case["ref"], case["rmask"], case["layer"], case["lmask"], record), want), case["name"]


def test_the_properties_that_follow_from_the_definition():
    for case in cases.pair_cases():
        ref, rmask, layer, lmask = case["ref"], case["rmask"], case["layer"], case["lmask"]
        t = spec.pair_terms(ref, rmask, layer, lmask)
        hist = spec.pair_histogram(ref, rmask, layer, lmask)
        assert int(hist.sum()) == int(t["sample"].sum()), case["name"]  # the total is the number of sample pixels
        assert not t["sample"][0].any() and not t["sample"][-1].any() and not t["sample"][:, 0].any() and not t["sample"][:, -1].any()  # interior only
        if case["kind"] == "empty":
            assert hist.sum() == 0  # a layer with no overlap adds nothing
        # a layer identical to the reference: every sample in bin 0, m = 0 and the strength clamps to 1
        same = spec.pair_histogram(ref, rmask, ref, rmask)
        assert same[:, 1:].sum() == 0
        curve = spec.resolve(same)
        assert int(curve[8, 1]) == 0 and (int(curve[8, 0]) == 0 or set(cspec.strengths(curve, min_samples=1, band_min_samples=1).tolist()) == {1})
    # the histogram's total over three layers, and any order of them gives the same histogram
    ref, rmask, _, _ = cases.pair(17, 65, 3, "holes", seed=5)
    layers = [cases.pair(17, 65, 3, "holes", seed=5, amp=a)[2:] for a in (2, 7, 15)]
    total = spec.frame_histogram(ref, rmask, layers)
    assert int(total.sum()) == sum(int(spec.pair_terms(ref, rmask, i, m)["sample"].sum()) for i, m in layers) > 0
    for order in itertools.permutations(range(3)):
        assert np.array_equal(spec.frame_histogram(ref, rmask, [layers[j] for j in order]), total)
    assert not np.array_equal(spec.pair_histogram(ref, rmask, *layers[0]), spec.pair_histogram(ref, rmask, *layers[2]))
    # one source: the empty histogram, row 8 with n = 0, every strength the fallback
    none = spec.noise_temporal(ref, rmask, [])
    assert none["hist"].sum() == 0 and none["curve"][:, :2].sum() == 0 and set(cspec.strengths(none["curve"], fallback=33).tolist()) == {33}


def test_each_exclusion_removes_exactly_the_windows_that_contain_it():
    for channels in (1, 3):
        ref, rmask, layer, lmask = cases.pair(17, 65, channels, "full", seed=9)
        base = spec.pair_terms(ref, rmask, layer, lmask)["sample"]
        assert base[1:-1, 1:-1].all() and int(base.sum()) == 15 * 63
        y, x = 8, 30
        near = np.zeros_like(base)
        near[y - 1:y + 2, x - 1:x + 2] = True
        edits = []
        for value in (0, 255):  # one saturated byte, in R and in L
            for which in (0, 2):
                planes = [ref.copy(), rmask, layer.copy(), lmask]
                planes[which][(y, x, channels - 1) if channels == 3 else (y, x)] = value
                edits.append(planes)
        for which in (1, 3):  # one unset pixel, in either mask
            planes = [ref, rmask.copy(), layer, lmask.copy()]
            planes[which][y, x] = 0
            edits.append(planes)
        for planes in edits:
            got = spec.pair_terms(*planes)["sample"]
            assert np.array_equal(got, base & ~near) and int(got.sum()) == 15 * 63 - 9
    for rows, cols in ((2, 2), (2, 9), (9, 2)):  # no full window
        ref, rmask, layer, lmask = cases.pair(rows, cols, 3, "full")
        assert spec.pair_histogram(ref, rmask, layer, lmask).sum() == 0
    ref, rmask, layer, lmask = cases.pair(3, 3, 1, "full")
    assert spec.pair_histogram(ref, rmask, layer, lmask).sum() == 1


def test_the_bounds_the_definition_states():
    for ch in (1, 3):
        N, D = 9 * ch, 9 * ch * 255
        assert 918 * D + 128 * N < 2 ** 32 and (918 * D + 128 * N) // (256 * N) == 914 < spec.BINS
    # the half-up rounding: D / N = 1 -> 918 / 256 = 3.586 -> 4; D = 0 -> 0
    assert (918 * 9 + 128 * 9) // (256 * 9) == 4 and (128 * 27) // (256 * 27) == 0
    assert abs(918 / 256 - (0.6745 * 6) / (2 / np.sqrt(np.pi))) < 0.002


# ---------------------------------------------------------------------------------------------------
# the estimator, the denoise at its strength and the mover: measured on the definition
# ---------------------------------------------------------------------------------------------------
# Measured on denoise_cases.shift_clip (24 x 40, five frames, the middle one at radius 2, uniform noise +-a, seeds 0 .. 3, BGR and gray):
#   sigma-hat / sigma-true    0.991 .. 1.057 over all 32 runs: the largest deviation is 0.057
#   strength at +-6           11 or 12
#   the own spatial curve     sigma-hat / sigma-true 39.7 .. 40.5 at +-2, 14.9 .. 15.3 at +-6, 7.7 .. 8.1 at +-12, 4.8 .. 5.0 at +-20
#   error ratio at +-20       0.400 .. 0.440 at the temporal strength against 0.907 .. 0.963 at the fixed 12: the smallest per-seed gap is 0.468
#   error ratio at +-6        0.395 .. 0.441 against 0.395 .. 0.445: at most 0.014 apart
SIGMA_LARGEST_DEVIATION = 0.057
DENOISE_SMALLEST_GAP = 0.468


@pytest.fixture(scope="module")
def measured():
    return {(ch, a, seed): cases.shift_measure(ch, a, seed) for ch in (3, 1) for a in cases.AMPS for seed in cases.SEEDS}


def test_the_estimate_follows_the_noise_where_the_spatial_curve_measures_the_texture(measured):
    """sigma-hat / sigma-true within twice the largest measured deviation (0.057) of 1 on every run; the strength at +-6 is the project's default
    12 or next to it; the frame's own spatial curve is at least 4 sigma-true at +-2, +-6 and +-12 (measured: 7.7 x and more) -- the defect.
    Measured, BGR and gray, seeds 0 .. 3: sigma-hat / sigma-true 1.050 at +-2, 0.991 .. 1.057 at +-6, 0.993 .. 1.028 at +-12, 1.002 .. 1.044 at
    +-20; h 5, 11 .. 12, 22 .. 23, 36 .. 38; the spatial curve's ratio 39.7 .. 40.5, 14.9 .. 15.3, 7.7 .. 8.1, 4.8 .. 5.0"""
    assert len(cases.SEEDS) >= 4
    for ch in (3, 1):
        for a in cases.AMPS:
            runs = [measured[ch, a, seed] for seed in cases.SEEDS]
            st = cases.sigma_true(a)
            ratios = [cases.sigma_hat(m["temporal"]["curve"]) / st for m in runs]
            spatial = [cases.sigma_hat(m["spatial"]["curve"]) / st for m in runs]
            hs = [cases.strength_of(m["temporal"]["curve"]) for m in runs]
            print("%s +-%d: sigma_true %.2f, sigma-hat / sigma-true %s, h %s; spatial %s" % ("BGR" if ch == 3 else "gray", a, st, ["%.3f" % x for x in ratios], hs,
                                                                                           ["%.1f" % x for x in spatial]))
            assert all(int(m["temporal"]["curve"][8, 0]) >= 1024 for m in runs)
            assert all(abs(x - 1) <= 2 * SIGMA_LARGEST_DEVIATION for x in ratios), (ch, a, ratios)
            if a == 6:
                assert all(h in (11, 12, 13) for h in hs), hs
            if a in (2, 6, 12):
                assert all(x >= 4 for x in spatial), (ch, a, spatial)


def test_the_denoise_at_the_temporal_strength(measured):
    """at +-20 the temporal strength beats the fixed 12 by more than half the smallest measured per-seed gap (0.468); at +-6, where the fixed 12
    is right, the two are within that same margin of each other (measured: 0.014).  Measured error ratios, temporal / fixed 12, BGR and gray,
    seeds 0 .. 3: +-2 0.352 .. 0.418 / 0.328 .. 0.408; +-6 0.395 .. 0.441 / 0.395 .. 0.445; +-12 0.400 .. 0.442 / 0.509 .. 0.578; +-20
    0.400 .. 0.440 / 0.907 .. 0.963"""
    margin = DENOISE_SMALLEST_GAP / 2
    for ch in (3, 1):
        for a in cases.AMPS:
            pairs = [cases.denoise_ratios(measured[ch, a, seed]) for seed in cases.SEEDS]
            print("%s +-%d: temporal %s, fixed 12 %s" % ("BGR" if ch == 3 else "gray", a, ["%.3f" % t for t, _ in pairs], ["%.3f" % f for _, f in pairs]))
            if a == 20:
                assert all(t < f - margin for t, f in pairs), (ch, pairs)
            if a == 6:
                assert all(abs(t - f) <= margin for t, f in pairs), (ch, pairs)


# Measured (the plate's mover, a block of 255 that sits elsewhere in every frame, on the shift texture of 96 columns at +-2, seeds 0 .. 3): the
# mean absolute error against the clean texture where the NEIGHBOURS' blocks fall in frame q is 0.50 .. 0.56 at the temporal curve (h = 5) and
# 11.84 .. 11.93 at the frame's own spatial curve (h = 171 .. 172, the gate fully open: the blocks ghost).  Smallest gap 11.32.
MOVER_SMALLEST_GAP = 11.32


def test_a_mover_does_not_ghost_at_the_temporal_strength():
    """the temporal curve is better on every seed (0.498 .. 0.556 against 11.844 .. 11.934 grey levels), so the direction is asserted, at half
    the smallest per-seed gap (11.32)"""
    for seed in cases.SEEDS:
        r = cases.mover_measure(seed)
        print("mover seed %d: temporal %.3f (h %d), spatial %.3f (h %d)" % (seed, r["temporal"], r["h_temporal"], r["spatial"], r["h_spatial"]))
        assert r["temporal"] < r["spatial"] - MOVER_SMALLEST_GAP / 2, r


# ---------------------------------------------------------------------------------------------------
# the kernel's resources
# ---------------------------------------------------------------------------------------------------
PATTERN = r"\S*noise_pair_hist_kernelILi[13]EE\S*"


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(flags):
        key = tuple(flags)
        if key not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("noise_temporal") / ("noise_temporal_kernels%d.s" % len(cache))
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "noise_temporal_kernels.hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")] +
                               list(flags) + [src, "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[key] = out.read_text()
        return cache[key]

    return get


@pytest.mark.parametrize("flags", [[], ["-DRSDSFM_FUSED=1"]])
def test_the_pair_histogram_kernels_have_no_private_segment(assembly, flags):
    """exactly two instances and no kernel beside them (the resolve is the noise curve's, only declared here), no private segment, no spills,
    at most 40 KB of LDS each: four workgroups in a CU's 160 KB"""
    txt = assembly(flags)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % PATTERN, txt)
    assert len(kernels) == 2 and len({n for n, _, _, _ in kernels}) == 2, kernels
    assert not [(n, ps, sp) for n, ps, vg, sp in kernels if int(ps) != 0 or int(sp) != 0], kernels
    assert all(int(vg) <= 128 for n, ps, vg, sp in kernels), kernels
    assert len(re.findall(r"\.name:\s+\S*kernel\S*\n", txt)) == 2
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\s+\.name:).*\n)*?\s+\.name:\s+\S*noise_pair_hist_kernel\S*\n", txt)
    assert len(lds) == 2 and all(32 * 1024 < int(x) <= 40 * 1024 for x in lds), lds
    print("pair histogram kernels (name, private, vgprs, spills):", kernels, "LDS bytes:", lds)


# ---------------------------------------------------------------------------------------------------
# the header, the symbols, the host-only entry points
# ---------------------------------------------------------------------------------------------------
def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/noise_temporal_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_noise_curve.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "NOT here" in HEADER_TEXT and "918" in HEADER_TEXT and "3.586" in HEADER_TEXT
    for prefix in ('"noise pair: ', '"noise resolve: ', '"denoise temporal frame: ', '"denoise temporal video: '):
        assert prefix in HEADER_TEXT, prefix


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_symbols_are_exported_by_both_builds(rsdsfm, nt, arith):
    lib = rsdsfm.load_library(arith=arith)
    txt = re.sub(r"/\*.*?\*/", "", open(nt.NOISE_TEMPORAL_HEADER_PATH).read(), flags=re.S)
    names = set(re.findall(r"\b(rsdsfm_[a-z0-9_]+)\s*\(", txt))
    assert names == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    assert not NEW_SYMBOLS & set(rsdsfm.declared_symbols())  # the package's surface is as it was


def test_launch_counts_and_host_errors(rsdsfm, nt):
    assert nt.noise_pair_hist_launches() == 1 and nt.noise_curve_resolve_launches() == 1
    for rows, cols, nsrc in ((24, 40, 1), (24, 40, 2), (37, 67, 5), (720, 1280, 15)):
        for top_up in (False, True):
            assert nt.denoise_temporal_frame_launches(rows, cols, nsrc, top_up) == rsdsfm.denoise_launches(rows, cols, nsrc) + (nsrc - 1) + 1 + int(top_up)
    for bad in ((1, 40, 3), (24, 16385, 3), (24, 40, 0), (24, 40, 16)):
        with pytest.raises(rsdsfm.RsdsfmError):
            nt.denoise_temporal_frame_launches(*bad)
    lib = rsdsfm.load_library()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    # no context: refused before anything is read
    assert lib.rsdsfm_noise_pair_hist_dev(None, None, None, None, None, i32(3), i32(8), i32(8), None, i64(0), i32(0), i32(1), None) == ERR_INVALID
    assert lib.rsdsfm_noise_curve_resolve_dev(None, None, i32(0), None) == ERR_INVALID
    assert lib.rsdsfm_denoise_temporal_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), i32(1), None, None, None, None,
                                                 None, None, None, None, None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_temporal_video_dev(None, None, i32(1), i32(8), i32(8), i32(3), f64(1), f64(1), f64(0), f64(0), None, None, None, None, None, None, None, None, 0, 0,
                                                 i32(0), None, None, None, None, None, None, None, None, None, None) == ERR_INVALID


# ---------------------------------------------------------------------------------------------------
# the marshalling of rsdsfm_noise_temporal.py: no argtypes, so every argument's type and value is compared with the golden
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_calls():
    return rec.read_gz(GOLDEN_CALLS)


def test_the_table_covers_every_dev_function_and_the_golden_lists_the_same_cases(nt, golden_calls):
    names = [name for name, _ in bcases.CASES]
    assert len(set(names)) == len(names) and sorted(names) == sorted(golden_calls["cases"])
    dev = sorted(n for n in vars(nt) if n.endswith("_dev") and callable(getattr(nt, n)))
    assert dev == sorted(bcases.DEV_FUNCTIONS) and set(dev) <= {n.split("/")[0] for n in names}
    public = {"NOISE_TEMPORAL_HEADER_PATH", "noise_pair_hist_launches", "noise_curve_resolve_launches", "denoise_temporal_frame_launches", "noise_pair_hist_dev",
              "noise_curve_resolve_dev", "denoise_temporal_frame_dev", "denoise_temporal_video_dev", "noise_temporal"}
    assert public <= set(vars(nt))
    # of the package's private names the module reaches only what rsdsfm_sharpen.py reaches
    reach = lambda path: set(re.findall(r"\brsdsfm\.(_[a-z][a-zA-Z0-9_]*)", open(os.path.join(ROOT, path)).read()))
    txt = open(os.path.join(ROOT, "rsdsfm_noise_temporal.py")).read()
    assert reach("rsdsfm_noise_temporal.py") <= reach("rsdsfm_sharpen.py") and "argtypes" not in txt.split('"""', 2)[2]
    for fn in dev:  # a refusal and at least one call that goes through
        assert fn + "/refused" in names


@pytest.mark.parametrize("name,fn", bcases.CASES, ids=[name for name, _ in bcases.CASES])
def test_case_hands_the_library_the_golden_arguments(rsdsfm, nt, golden_calls, name, fn):
    want = golden_calls["cases"][name]
    got = rec.loads(rec.dumps(rec.run_case(rsdsfm, lambda e: fn(e, nt))))
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert len(g[1]) == len(w[1]), g[0]
        for i, (ga, wa) in enumerate(zip(g[1], w[1])):
            assert ga == wa, "%s argument %d" % (g[0], i)
    assert got.get("raises") == want.get("raises")
    assert got.get("returns") == want.get("returns")


def test_the_recorded_calls_have_the_headers_argument_counts_and_wrapped_types(golden_calls):
    """independent of the golden's history: every recorded call has as many arguments as the header declares, every device pointer went out as
    a c_void_p (or NULL) and every word by value as the type of the prototype"""
    txt = re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"\bint\s+(rsdsfm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}
    seen = set()
    for case in golden_calls["cases"].values():
        for name, args in case["calls"]:
            if name not in NEW_SYMBOLS:
                continue
            seen.add(name)
            params = [] if protos[name] == ["void"] else protos[name]
            assert len(args) == len(params), name
            for a, p in zip(args, params):
                if re.match(r"(const )?(uint8_t|uint32_t|uint64_t|int64_t)\* d_", p) or p.startswith("rsdsfm_ctx"):  # one device plane, or the context
                    assert a is None or list(a) == ["c_void_p"], (name, p, a)
                elif p.startswith("int32_t "):
                    assert list(a) == [ctypes.c_int32.__name__], (name, p, a)
                elif p.startswith("int64_t "):
                    assert list(a) == [ctypes.c_int64.__name__], (name, p, a)
                elif p.startswith("double "):
                    assert list(a) == [ctypes.c_double.__name__], (name, p, a)
    assert seen == NEW_SYMBOLS

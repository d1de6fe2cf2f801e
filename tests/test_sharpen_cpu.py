"""GPU-free tests of the sharpen stage (include/rsdsfm_sharpen.h): the definition (tests/sharpen_spec_numpy.py) against the properties that
follow from it, against a loop per pixel and against the golden fixture, the curve form against the fixed form under a flat curve and under too
few samples, the kernel's exact division, the exported symbols, params_init and the launch counts, the no-argtypes marshalling of
rsdsfm_sharpen.py on the recording library, and two quality scenes on the definition: a blurred edge texture beside a flat third under noise,
and the noise curve's ramp whose noise grows with brightness."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import binding_recorder as rec  # noqa: E402
import noise_curve_cases as ccases  # noqa: E402
import noise_curve_spec_numpy as cspec  # noqa: E402
import noise_spec_numpy as nspec  # noqa: E402
import sharpen_binding_cases as bcases  # noqa: E402
import sharpen_cases as cases  # noqa: E402
import sharpen_spec_numpy as spec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_sharpen_v1.npz")
GOLDEN_CALLS = os.path.join(ROOT, "tests", "golden", "sharpen_calls_v1.json.gz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_sharpen.h")).read()
NEW_SYMBOLS = {"rsdsfm_sharpen_params_init", "rsdsfm_sharpen_dev", "rsdsfm_sharpen_curve_dev", "rsdsfm_sharpen_launches", "rsdsfm_sharpen_frame_dev",
               "rsdsfm_sharpen_frame_launches", "rsdsfm_sharpen_video_dev"}
ERR_INVALID = -1


@pytest.fixture(scope="module")
def sh(rsdsfm):
    import rsdsfm_sharpen

    return rsdsfm_sharpen


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture():
    g = np.load(GOLDEN)
    golden = cases.golden_cases()
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in golden} | {"curve"}
    assert {c["kind"] for c in golden} == set(cases.KINDS) and {(c["amount_q4"], c["coring_q4"], c["overshoot"]) for c in golden} == set(cases.PARAMS)
    for case in golden:
        n = case["name"] + "/"
        assert np.array_equal(g[n + "in_image"], case["image"]) and np.array_equal(g[n + "in_mask"], case["mask"])
        assert g[n + "params"].tolist() == [case["amount_q4"], case["coring_q4"], case["overshoot"], case["strength"]]
        r = spec.sharpen(g[n + "in_image"], g[n + "in_mask"], *[int(x) for x in g[n + "params"]])
        assert np.array_equal(r["image"], g[n + "image"]) and r["counts"] == g[n + "counts"].tolist(), n
    image, mask, lut = cases.golden_curve_case()
    assert np.array_equal(g["curve/in_image"], image) and np.array_equal(g["curve/in_mask"], mask) and np.array_equal(g["curve/lut"], lut)
    r = spec.sharpen(image, mask, lut=lut)
    assert np.array_equal(r["image"], g["curve/image"]) and r["counts"] == g["curve/counts"].tolist() and len(set(lut.tolist())) > 1
    assert os.path.getsize(GOLDEN) <= 64 * 1024


def _loop(image, mask, amount, coring, overshoot, h_of):
    """the definition once more, a literal loop per pixel"""
    I = spec._planes(image).astype(np.int64)
    rows, cols, ch = I.shape
    out = np.zeros_like(I)
    counts = [0, 0, 0, 0]
    k1 = (1, 4, 6, 4, 1)
    for y in range(rows):
        for x in range(cols):
            if not mask[y, x]:
                counts[0] += 1
                continue
            S, K = [0] * ch, 0
            for oy in range(-2, 3):
                for ox in range(-2, 3):
                    yy, xx = y + oy, x + ox
                    if 0 <= yy < rows and 0 <= xx < cols and mask[yy, xx]:
                        k = k1[oy + 2] * k1[ox + 2]
                        K += k
                        for c in range(ch):
                            S[c] += k * int(I[yy, xx, c])
            level = int(I[y, x, 0]) if ch == 1 else (int(I[y, x].sum()) + 1) // 3
            T = (coring * h_of(level) + 8) >> 4
            block = [I[yy, xx] for yy in range(max(y - 1, 0), min(y + 2, rows)) for xx in range(max(x - 1, 0), min(x + 2, cols)) if mask[yy, xx]]
            changed = limited = False
            for c in range(ch):
                d = K * int(I[y, x, c]) - S[c]
                e = max(0, abs(d) - T * K)
                r = (2 * amount * e + 16 * K) // (32 * K)
                o = int(I[y, x, c]) + (r if d > 0 else -r if d < 0 else 0)
                lo, hi = min(int(b[c]) for b in block), max(int(b[c]) for b in block)
                res = min(max(o, max(0, lo - overshoot)), min(255, hi + overshoot))
                out[y, x, c] = res
                changed |= res != I[y, x, c]
                limited |= res != o
            counts[1 if not changed else 3 if limited else 2] += 1
    return out[..., 0] if np.asarray(image).ndim == 2 else out, counts


def test_the_definition_equals_a_loop_per_pixel():
    every = [c for c in cases.primitive_cases() if c["image"].shape[0] * c["image"].shape[1] <= 17 * 65]
    assert {c["kind"] for c in every} == set(cases.KINDS)
    lut = cspec.strengths(ccases.RISING)
    for k, case in enumerate(every[::3]):
        with_lut = k % 2 == 1
        want, counts = _loop(case["image"], case["mask"], case["amount_q4"], case["coring_q4"], case["overshoot"],
                             (lambda L: int(lut[L])) if with_lut else (lambda L, h=case["strength"]: h))
        got = cases.run_spec(case, lut if with_lut else None)
        assert np.array_equal(got["image"], want) and got["counts"] == counts, case["name"]


def test_the_properties_that_follow_from_the_definition():
    for case in cases.primitive_cases():
        image, mask = case["image"], case["mask"]
        v = mask != 0
        I = spec._planes(image)
        masked = np.where(v[..., None], I, 0)
        n = image.shape[0] * image.shape[1]
        r = cases.run_spec(case)
        assert sum(r["counts"]) == n and r["counts"][0] == int((~v).sum()), case["name"]
        # amount_q4 = 0 copies I under the mask
        r0 = spec.sharpen(image, mask, 0, case["coring_q4"], case["overshoot"], case["strength"])
        assert np.array_equal(spec._planes(r0["image"]), masked) and r0["counts"][2:] == [0, 0]
        # T >= 255 copies: coring_q4 h >= 4072
        rt = spec.sharpen(image, mask, 64, 64, 255, 64)
        assert (64 * 64 + 8) >> 4 >= 255 and np.array_equal(spec._planes(rt["image"]), masked) and rt["counts"][2:] == [0, 0]
        # with overshoot = 0 every output byte lies within the 3 x 3 set range of its input
        rl = spec.sharpen(image, mask, 64, 0, 0, case["strength"])
        lo, hi = spec.local_range(image, mask)
        out = spec._planes(rl["image"]).astype(np.int64)
        assert ((out >= lo) & (out <= hi))[v].all(), case["name"]
        if case["kind"] == "flat":  # a constant image is all kept
            assert spec.sharpen(image, mask, 64, 0, 255, 1)["counts"][2:] == [0, 0]
        if case["kind"] == "isolated":  # a set pixel whose 5 x 5 block holds no other set pixel is kept
            _, K = spec.blur_sums(image, mask)
            alone = v & (K == 36)
            rs = spec.sharpen(image, mask, 64, 0, 255, 1)
            assert np.array_equal(spec._planes(rs["image"])[alone], I[alone])
            assert alone.any() or min(image.shape[:2]) < 3
    # an affine image is kept at least 2 from the border and from any hole: the kernel is symmetric, so the blur of a ramp is the ramp
    y, x = np.mgrid[0:40, 0:70]
    ramp = (3 * x + y).astype(np.uint8)
    assert (3 * x + y).max() <= 255
    mask = np.full(ramp.shape, 255, dtype=np.uint8)
    mask[20, 30] = 0
    far = np.ones(ramp.shape, dtype=bool)
    far[:2], far[-2:], far[:, :2], far[:, -2:] = False, False, False, False
    far[18:23, 28:33] = False
    out = spec.sharpen(ramp, mask, 64, 0, 255, 1)["image"]
    assert np.array_equal(out[far], ramp[far]) and not np.array_equal(out[~far & (mask != 0)], ramp[~far & (mask != 0)])
    bgr = np.stack([ramp, ramp // 2, 255 - ramp], axis=-1)
    assert np.array_equal(spec.sharpen(bgr, mask, 64, 0, 255, 1)["image"][far][:, [0, 2]], bgr[far][:, [0, 2]])


def test_the_bounds_the_header_states():
    """K >= 36 under the mask and >= 121 on a full mask, |d| <= 255 (K - 36), and the checker reaches the largest detail"""
    for case in cases.primitive_cases():
        S, K = spec.blur_sums(case["image"], case["mask"])
        v = case["mask"] != 0
        d = np.abs(K[..., None] * spec._planes(case["image"]).astype(np.int64) - S)
        assert K.max() <= 256 and (not v.any() or K[v].min() >= 36) and (d[v] <= 255 * (K[v] - 36)[..., None]).all()
        if v.all():
            assert K.min() >= (121 if min(v.shape) >= 3 else 36)
    assert (64 * 255 + 8) >> 4 == 1020 and 2 * 64 * 255 * 220 + 16 * 256 < 2 ** 24 and "2^24" in HEADER_TEXT


def test_the_kernels_division_is_exact():
    """div_u24 (csrc/sharpen.hpp): q = trunc(float(num) * rcp(float(den))) corrected once by its remainder.  Here with a reciprocal that is off by
    up to 2 ulp either way (the hardware's is within 1): the estimate stays within one of the quotient for every K and the extreme and random
    numerators, so one correction step is enough"""
    rng = np.random.default_rng(5)
    for K in range(36, 257):
        den = 16 * K
        num = np.concatenate([np.arange(0, 4 * den), rng.integers(0, 64 * 255 * 220 + 8 * 256, size=400), [64 * 255 * (K - 36) + 8 * K]]).astype(np.int64)
        for ulps in (-2, 0, 2):
            rcp = np.float32(1.0) / np.float32(den)
            for _ in range(abs(ulps)):
                rcp = np.nextafter(rcp, np.float32(np.inf if ulps > 0 else -np.inf), dtype=np.float32)
            q = (num.astype(np.float32) * rcp).astype(np.int64)
            rem = num - q * den
            q = np.where(rem < 0, q - 1, np.where(rem >= den, q + 1, q))
            assert np.array_equal(q, num // den), (K, ulps)
    assert ((np.arange(767) * 21846) >> 16).tolist() == (np.arange(767) // 3).tolist()  # sharpen_third


# ---------------------------------------------------------------------------------------------------
# the curve form
# ---------------------------------------------------------------------------------------------------
def test_a_flat_curve_and_too_few_samples_give_the_fixed_form():
    flat = [(ccases.flat_curve(700, 16), 0, 0, 0, 0), (ccases.flat_curve(20, 9), 200, 40, 64, 16), (ccases.TOO_FEW, 33, 0, ccases.MIN_SAMPLES, ccases.BAND_MIN_SAMPLES)]
    for k, (curve, fallback, scale, ms, bms) in enumerate(flat):
        lut = cspec.strengths(curve, scale, fallback or 12, ms, bms)
        h = nspec.noise_strength(int(curve[8, 0]), int(curve[8, 1]), scale, fallback or 12, ms)
        assert set(lut.tolist()) == {h}
        for ch in (1, 3):
            image, mask = ccases.ramp_reference(17, 65, ch, seed=k)
            a, b = spec.sharpen(image, mask, 32, 8, 8, fallback or 12, lut), spec.sharpen(image, mask, 32, 8, 8, h)
            assert np.array_equal(a["image"], b["image"]) and a["counts"] == b["counts"]
    image, mask = ccases.ramp_reference(17, 65, 3, seed=3)
    assert not np.array_equal(spec.sharpen(image, mask, lut=cspec.strengths(ccases.RISING))["image"], spec.sharpen(image, mask)["image"])  # a real curve matters


# ---------------------------------------------------------------------------------------------------
# the header, the symbols, the host-only entry points
# ---------------------------------------------------------------------------------------------------
def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/sharpen_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_noise_curve.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "choices, not measurements" in HEADER_TEXT and "NOT here" in HEADER_TEXT and "0 IS A VALUE" in HEADER_TEXT
    for prefix in ('"sharpen: ', '"sharpen curve: ', '"sharpen frame: ', '"sharpen video: '):
        assert prefix in HEADER_TEXT, prefix


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_symbols_are_exported_by_both_builds(rsdsfm, sh, arith):
    lib = rsdsfm.load_library(arith=arith)
    txt = re.sub(r"/\*.*?\*/", "", open(sh.SHARPEN_HEADER_PATH).read(), flags=re.S)
    names = set(re.findall(r"\b(rsdsfm_[a-z0-9_]+)\s*\(", txt))
    assert names == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    assert not NEW_SYMBOLS & set(rsdsfm.declared_symbols())  # the package's surface is as it was
    assert sh.sharpen_default_params() == dict(amount_q4=spec.AMOUNT_DEFAULT, coring_q4=spec.CORING_DEFAULT, overshoot=spec.OVERSHOOT_DEFAULT, strength=spec.STRENGTH_DEFAULT)
    assert ctypes.sizeof(sh.SharpenParams) == 32
    p = sh.SharpenParams()
    assert lib.rsdsfm_sharpen_params_init(ctypes.byref(p)) == 0 and p.struct_bytes == 32 and list(p.reserved) == [0, 0, 0]
    assert (p.amount_q4, p.coring_q4, p.overshoot, p.strength) == (16, 8, 0, 12)
    assert lib.rsdsfm_sharpen_params_init(None) == ERR_INVALID


def test_launch_counts_and_host_errors(rsdsfm, sh):
    assert sh.sharpen_launches() == 1 and sh.sharpen_frame_launches() == 3
    lib = rsdsfm.load_library()
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    # no context: refused before anything is read
    assert lib.rsdsfm_sharpen_dev(None, None, None, i32(3), i32(8), i32(8), i32(16), i32(8), i32(0), i32(0), None, None) == ERR_INVALID
    assert lib.rsdsfm_sharpen_curve_dev(None, None, None, i32(3), i32(8), i32(8), i32(16), i32(8), i32(0), i32(0), None, i32(0), i64(0), i64(0), None, None) == ERR_INVALID
    assert lib.rsdsfm_sharpen_frame_dev(None, None, None, i32(3), i32(8), i32(8), None, None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_sharpen_video_dev(None, None, None, i32(1), i32(3), i32(8), i32(8), None, None, None, None, None) == ERR_INVALID


# ---------------------------------------------------------------------------------------------------
# the marshalling of rsdsfm_sharpen.py: no argtypes, so every argument's type and value is compared with the golden
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_calls():
    return rec.read_gz(GOLDEN_CALLS)


def test_the_table_covers_every_dev_function_and_the_golden_lists_the_same_cases(sh, golden_calls):
    names = [name for name, _ in bcases.CASES]
    assert len(set(names)) == len(names) and sorted(names) == sorted(golden_calls["cases"])
    dev = sorted(n for n in vars(sh) if n.endswith("_dev") and callable(getattr(sh, n)))
    assert dev == sorted(bcases.DEV_FUNCTIONS) and set(dev) <= {n.split("/")[0] for n in names}
    public = {"SHARPEN_HEADER_PATH", "SharpenParams", "sharpen_default_params", "sharpen_launches", "sharpen_frame_launches", "sharpen_dev", "sharpen_curve_dev",
              "sharpen_frame_dev", "sharpen_video_dev", "sharpen"}
    assert public <= set(vars(sh))
    # of the package's private names the module reaches only what tests/binding_cases.py's PRIVATE_SURFACE lists
    import binding_cases

    txt = open(os.path.join(ROOT, "rsdsfm_sharpen.py")).read()
    assert set(re.findall(r"\brsdsfm\.(_[a-z][a-zA-Z0-9_]*)", txt)) <= set(binding_cases.PRIVATE_SURFACE) and "argtypes" not in txt.split('"""', 2)[2]
    for fn in dev:  # a refusal and at least one call that goes through
        assert fn + "/refused" in names


@pytest.mark.parametrize("name,fn", bcases.CASES, ids=[name for name, _ in bcases.CASES])
def test_case_hands_the_library_the_golden_arguments(rsdsfm, sh, golden_calls, name, fn):
    want = golden_calls["cases"][name]
    got = rec.loads(rec.dumps(rec.run_case(rsdsfm, lambda e: fn(e, sh))))
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
                if re.match(r"(const )?(uint8_t|uint64_t|int64_t)\* d_", p) or p.startswith("rsdsfm_ctx"):  # one device plane, or the context
                    assert a is None or list(a) == ["c_void_p"], (name, p, a)
                elif p.startswith("int32_t "):
                    assert list(a) == [ctypes.c_int32.__name__], (name, p, a)
                elif p.startswith("int64_t "):
                    assert list(a) == [ctypes.c_int64.__name__], (name, p, a)
    assert seen == NEW_SYMBOLS


# ---------------------------------------------------------------------------------------------------
# the quality scenes, on the definition
# ---------------------------------------------------------------------------------------------------
# Measured on this file's scene (sharpen_cases.quality_frame: a flat third at 120 beside bars and blocks of 70 / 180, blurred by the 3 x 3
# binomial, uniform noise +-a, fixed h = 2 a, eight seeds; mean absolute error against the unblurred clean frame, output / input).  Per a:
# (textured defaults max, textured no coring max, flat defaults farthest from 1, flat no coring min)
QUALITY_MEASURED = {2: (0.6989, 0.6354, 1.0000, 1.2429), 6: (0.8386, 0.6679, 1.0000, 1.2726), 12: (0.9418, 0.7267, 1.0000, 1.2753)}


def _quality(a):
    tex, flat = cases.quality_regions()
    rows = []
    for seed in range(cases.QUALITY_SEEDS):
        clean, obs = cases.quality_frame(seed, a)
        e_in = np.abs(obs.astype(np.int64) - clean)
        r = []
        for coring in (spec.CORING_DEFAULT, 0):
            e = np.abs(spec.sharpen(obs, None, spec.AMOUNT_DEFAULT, coring, 0, 2 * a)["image"].astype(np.int64) - clean)
            r += [e[tex].mean() / e_in[tex].mean(), e[flat].mean() / e_in[flat].mean()]
        rows.append(r)
    return np.array(rows)  # (seeds, [textured defaults, flat defaults, textured no coring, flat no coring])


@pytest.mark.parametrize("a", cases.QUALITY_AMPS)
def test_sharpening_helps_the_texture_and_coring_spares_the_flat(a):
    """the bounds are half the smallest measured gap to 1 over the seeds (QUALITY_MEASURED): the textured part's error falls with the defaults,
    the flat part's error rises without coring, and with the defaults it stays within that same margin of 1"""
    r = _quality(a)
    print("a = %d: textured defaults %.4f - %.4f, no coring %.4f - %.4f; flat defaults %.4f - %.4f, no coring %.4f - %.4f" % (
        a, r[:, 0].min(), r[:, 0].max(), r[:, 2].min(), r[:, 2].max(), r[:, 1].min(), r[:, 1].max(), r[:, 3].min(), r[:, 3].max()))
    tex_max, _, _, flat_raw_min = QUALITY_MEASURED[a]
    assert (r[:, 0] < 1 - (1 - tex_max) / 2).all()
    margin = (flat_raw_min - 1) / 2
    assert (r[:, 3] > 1 + margin).all()
    assert (np.abs(r[:, 1] - 1) < margin).all()


# Measured on noise_curve_cases.ramp_clip (levels 20 .. 235 across the columns, noise +-2 at 0 to +-20 at 255, eight seeds, the first frame of
# each clip): the share of pixels the defaults change, per third of the columns, with the frame's own curve against the one global strength
# rsdsfm_noise_strength forms from the curve's last row.  Gray: dark 0.0203 - 0.0346 against 0.0000 - 0.0015, middle 0.0065 - 0.0124 against
# 0.0157 - 0.0293, bright 0.0038 - 0.0085 against 0.0893 - 0.1345; BGR: dark 0.0598 - 0.1003 against 0.0010 - 0.0065, middle 0.0235 - 0.0303 against
# 0.0484 - 0.0942, bright 0.0125 - 0.0218 against 0.2491 - 0.3641.  Per channels: the smallest per-seed gap (dark: curve - global; middle and
# bright: global - curve)
RAMP_MEASURED_GAPS = {1: (0.0199, 0.0048, 0.0852), 3: (0.0552, 0.0225, 0.2327)}


def _ramp_shares(channels):
    x = np.arange(ccases.QUALITY_COLS)
    thirds = [x < ccases.QUALITY_COLS // 3, (x >= ccases.QUALITY_COLS // 3) & (x < 2 * ccases.QUALITY_COLS // 3), x >= 2 * ccases.QUALITY_COLS // 3]
    rows = []
    for seed in range(ccases.QUALITY_SEEDS):
        _, frames = ccases.ramp_clip(channels, seed, *ccases.QUALITY_AMPS)
        f = frames[0]
        r = spec.sharpen_frame(f)
        g = nspec.noise_strength(int(r["curve"][8, 0]), int(r["curve"][8, 1]))
        changed_c = (spec._planes(r["image"]) != spec._planes(f)).any(axis=-1)
        changed_g = (spec._planes(spec.sharpen(f, None, strength=g)["image"]) != spec._planes(f)).any(axis=-1)
        rows.append([[changed_c[:, t].mean(), changed_g[:, t].mean()] for t in thirds])
    return np.array(rows)  # (seeds, thirds, [curve, global])


@pytest.mark.parametrize("channels", [1, 3])
def test_the_curve_moves_the_sharpening_from_the_noisy_highlights_to_the_clean_shadows(channels):
    """with the frame's own curve the defaults sharpen MORE pixels in the dark third, where the noise is weak, and FEWER in the bright third,
    and in the middle third, where it is strong, than with the one global strength: each direction held over every seed when measured and is
    asserted at half its smallest measured gap"""
    s = _ramp_shares(channels)
    for t, name in enumerate(("dark", "middle", "bright")):
        print("channels %d, %s third: curve %.4f - %.4f, global %.4f - %.4f, per-seed gap (curve - global) %.4f - %.4f" % (
            channels, name, s[:, t, 0].min(), s[:, t, 0].max(), s[:, t, 1].min(), s[:, t, 1].max(), (s[:, t, 0] - s[:, t, 1]).min(), (s[:, t, 0] - s[:, t, 1]).max()))
    dark, middle, bright = RAMP_MEASURED_GAPS[channels]
    assert dark > 0 and middle > 0 and bright > 0
    assert (s[:, 0, 0] - s[:, 0, 1] > dark / 2).all()
    assert (s[:, 1, 1] - s[:, 1, 0] > middle / 2).all()
    assert (s[:, 2, 1] - s[:, 2, 0] > bright / 2).all()

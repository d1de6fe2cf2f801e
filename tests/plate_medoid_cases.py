"""Inputs of the colour-consistent plate's tests (tests/test_plate_medoid_cpu.py, tests/test_gpu_plate_medoid.py): tests/plate_cases.py's
constructed cases with the answers an L1 medoid has by hand -- they differ from the median's wherever the candidates disagree channel by channel
--, the triple without a majority that the estimator was built for, and the seeded campaigns by channel count.  plate_cases itself is imported
and unchanged."""
import numpy as np

import plate_cases as cases
import plate_medoid_spec_numpy as spec

GREY, RED, BLUE = (100, 100, 100), (0, 0, 255), (255, 0, 0)  # BGR
PURPLE = (100, 0, 100)  # the per-channel median of the three: a colour none of them has


def packed(image):
    """b | g << 8 | r << 16 per pixel (the gray value for one channel): the order two candidates of equal cost are ranked by"""
    a = np.asarray(image).astype(np.int64)
    return a if a.ndim == 2 else a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16)


def smaller_colour(a, b):
    """per pixel the whole pixel of a or b with the smaller packed colour"""
    pick = packed(a) <= packed(b)
    return np.where(pick if np.asarray(a).ndim == 2 else pick[..., None], a, b)


def no_majority(rows=19, cols=70):
    """the own frame grey, one layer red, one blue: cost(grey) = 355 + 355 = 710, cost(red) = cost(blue) = 355 + 510 = 865 -- the medoid is the
    grey candidate, the median (100, 0, 100).  e = 0 everywhere: static"""
    px = lambda c: np.broadcast_to(np.array(c, dtype=np.uint8), (rows, cols, 3)).copy()
    full, ones = np.full((rows, cols), 255, dtype=np.uint8), np.ones((rows, cols), dtype=np.uint8)
    return cases._case("no-majority", px(GREY), full, [(px(RED), full), (px(BLUE), full)],
                       dict(image=px(GREY), mask=ones, votes=3 * ones, moving=ones, counts=[0, rows * cols, 0, 0]))


def constructed(channels, **kw):
    """plate_cases.constructed with the medoid's hand answers: with one channel the list as it is (consequence (a)); with three, two candidates
    give the one with the smaller packed colour (equal costs), three random layers give no hand answer for the image, everything else -- all
    equal, one outlier among fifteen, ties (costs 12, 14, 14, 12; of the two at 12 (5, 2, 7) packs below (9, 3, 7)), the impulses -- keeps its
    answer; plus the triple without a majority"""
    out = []
    for case in cases.constructed(channels, **kw):
        want = dict(case["want"])
        if channels == 3 and case["name"] == "two-candidates":
            want["image"] = smaller_colour(case["ref"], case["layers"][0][0])
        elif channels == 3 and case["name"] == "two-layers-no-own":
            want["image"] = smaller_colour(case["layers"][0][0], case["layers"][1][0])
        elif channels == 3 and case["name"] == "own-mask-empty":
            del want["image"]
        out.append(dict(case, want=want))
    if channels == 3:
        out.append(no_majority())
    return out


def random_cases(seed, count, channels):
    """the first `count` cases of plate_cases.random_case's stream with that many channels"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        case = cases.random_case(rng)
        if (1 if case["ref"].ndim == 2 else 3) == channels:
            out.append(case)
    return out


def shuffled(case, perm):
    """the case with its layers and their records in another order"""
    return dict(case, layers=[case["layers"][i] for i in perm], records=None if case["records"] is None else np.asarray(case["records"])[list(perm)])


spec_of = spec.spec_of

"""The table of calls tests/test_sharpen_cpu.py replays on the recording library (tests/binding_recorder.py) for rsdsfm_sharpen.py: one entry or
more per function that reaches the library, both sides of every optional argument, params= and curve_params= pass-through, want_counts= and
want_curves=, and refusals with their text.  A case is (name, function of the recorder's Env and the module); tests/binding_cases.py's helpers
are imported unchanged.  The golden is tests/golden/sharpen_calls_v1.json.gz (tests/golden/make_golden_sharpen.py)."""
from binding_cases import CH, COLS, ROWS


def _fails2(name, rc, fn):
    def run(e, sh):
        e.lib.returns[name] = rc
        return fn(e, sh)
    return run


def _curve_params(sh):
    return sh.NoiseCurveParams(quantile_q8=77, scale=9, struct_bytes=48, min_samples=2 ** 33, band_min_samples=19)


CASES = [
    ("sharpen_default_params", lambda e, sh: sh.sharpen_default_params()),
    ("sharpen_params_init/refused", _fails2("rsdsfm_sharpen_params_init", -1, lambda e, sh: sh.sharpen_default_params())),
    ("sharpen_launches", lambda e, sh: [sh.sharpen_launches(), sh.sharpen_frame_launches()]),
    ("sharpen_dev", lambda e, sh: [sh.sharpen_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p()), sh.sharpen_dev(e.s, e.p(), e.p(), 1, ROWS, COLS, e.p(), e.p(), 0, 0, 0, 0),
                                   sh.sharpen_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p(), e.p(), 64, 63, 255, 40)]),
    ("sharpen_dev/refused", _fails2("rsdsfm_sharpen_dev", -1, lambda e, sh: sh.sharpen_dev(e.s, e.p(), e.p(), 2, ROWS, COLS, e.p()))),
    ("sharpen_curve_dev", lambda e, sh: [sh.sharpen_curve_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p(), e.p()),
                                         sh.sharpen_curve_dev(e.s, e.p(), e.p(), 1, ROWS, COLS, e.p(), e.p(), e.p(), 0, 0, 0, 40, 24, 2 ** 34, 2 ** 35)]),
    ("sharpen_curve_dev/refused", _fails2("rsdsfm_sharpen_curve_dev", -1, lambda e, sh: sh.sharpen_curve_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, None, e.p()))),
    ("sharpen_frame_dev", lambda e, sh: [sh.sharpen_frame_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p()),
                                         sh.sharpen_frame_dev(e.s, e.p(), e.p(), 1, ROWS, COLS, e.p(), e.p(), e.p(), 0, 0, 0, 40, None, 200, 24, 2 ** 34, 2 ** 35),
                                         sh.sharpen_frame_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p(), d_curve36=e.p(), amount_q4=64, overshoot=9)]),
    ("sharpen_frame_dev/params", lambda e, sh: sh.sharpen_frame_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p(), params=sh.SharpenParams(3, 5, 7, 41, 32),
                                                                   curve_params=_curve_params(sh))),
    ("sharpen_frame_dev/refused", _fails2("rsdsfm_sharpen_frame_dev", -1, lambda e, sh: sh.sharpen_frame_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p()))),
    ("sharpen_video_dev", lambda e, sh: sh.sharpen_video_dev(e.s, e.P(3), e.P(3), CH, ROWS, COLS, e.P(3))),
    ("sharpen_video_dev/everything", lambda e, sh: sh.sharpen_video_dev(e.s, e.P(2), e.P(3), 1, ROWS, COLS, e.P(4), True, False, 0, 0, 0, 40, None, 200, 24, 2 ** 34, 2 ** 35)),
    ("sharpen_video_dev/params", lambda e, sh: sh.sharpen_video_dev(e.s, e.P(2), e.P(2), CH, ROWS, COLS, e.P(2), False, True, params=sh.SharpenParams(3, 5, 7, 41, 32),
                                                                   curve_params=_curve_params(sh))),
    ("sharpen_video_dev/no host arrays", lambda e, sh: sh.sharpen_video_dev(e.s, e.P(2), e.P(2), CH, ROWS, COLS, e.P(2), want_counts=False, want_curves=False)),
    ("sharpen_video_dev/out one short", lambda e, sh: sh.sharpen_video_dev(e.s, e.P(3), e.P(3), CH, ROWS, COLS, e.P(2))),
    ("sharpen_video_dev/no frames", lambda e, sh: sh.sharpen_video_dev(e.s, [], [], CH, ROWS, COLS, [])),
    ("sharpen_video_dev/refused", _fails2("rsdsfm_sharpen_video_dev", -1, lambda e, sh: sh.sharpen_video_dev(e.s, e.P(2), e.P(2), CH, ROWS, COLS, e.P(2)))),
]

# the *_dev functions of the module: each needs a case above
DEV_FUNCTIONS = ("sharpen_dev", "sharpen_curve_dev", "sharpen_frame_dev", "sharpen_video_dev")

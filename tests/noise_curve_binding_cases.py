"""The table of calls tests/test_noise_curve_cpu.py replays on the recording library (tests/binding_recorder.py) for rsdsfm_noise_curve.py: one
entry or more per function that reaches the library, both sides of every optional argument, params= pass-through, window=, want_counts= and
want_curves=, and refusals with their text.  A case is (name, function of the recorder's Env and the module); tests/binding_cases.py's helpers
are imported unchanged.  The golden is tests/golden/noise_curve_calls_v1.json.gz (tests/golden/make_golden_noise_curve.py)."""
import numpy as np

from binding_cases import CH, COLS, K, ROWS, accumulate_outs, ar, clip, frame

CURVE = (np.arange(36, dtype=np.uint64) * 37 + 5).reshape(9, 4)


def _fails2(name, rc, fn):
    def run(e, nc):
        e.lib.returns[name] = rc
        return fn(e, nc)
    return run


CASES = [
    ("noise_curve_default_params", lambda e, nc: nc.noise_curve_default_params()),
    ("noise_curve_params_init/refused", _fails2("rsdsfm_noise_curve_params_init", -1, lambda e, nc: nc.noise_curve_default_params())),
    ("noise_curve_launches", lambda e, nc: nc.noise_curve_launches()),
    ("noise_curve_strengths", lambda e, nc: [nc.noise_curve_strengths(CURVE), nc.noise_curve_strengths(CURVE.reshape(-1), 24, 40, 2 ** 33, 17)]),
    ("noise_curve_strengths/35 words", lambda e, nc: nc.noise_curve_strengths(np.arange(35))),
    ("noise_curve_strengths/refused", _fails2("rsdsfm_noise_curve_strengths", -1, lambda e, nc: nc.noise_curve_strengths(CURVE, 256))),
    ("denoise_curve_frame_launches", lambda e, nc: [nc.denoise_curve_frame_launches(ROWS, COLS, 3), nc.denoise_curve_frame_launches(ROWS, COLS, 3, True)]),
    ("denoise_curve_frame_launches/refused", _fails2("rsdsfm_denoise_curve_frame_launches", -1, lambda e, nc: nc.denoise_curve_frame_launches(1, COLS, 3))),
    ("noise_curve_dev", lambda e, nc: [nc.noise_curve_dev(e.s, e.p(), e.p(), CH, ROWS, COLS, e.p(), e.p()), nc.noise_curve_dev(e.s, e.p(), e.p(), 1, ROWS, COLS, e.p(), e.p(), 200)]),
    ("noise_curve_dev/refused", _fails2("rsdsfm_noise_curve_dev", -1, lambda e, nc: nc.noise_curve_dev(e.s, e.p(), e.p(), 2, ROWS, COLS, e.p(), e.p()))),
    ("denoise_accumulate_curve_dev", lambda e, nc: [nc.denoise_accumulate_curve_dev(e.s, e.p(), e.p(), e.p(), e.p(), CH, ROWS, COLS, e.p(), True, False, e.p()),
                                                   nc.denoise_accumulate_curve_dev(e.s, e.p(), e.p(), None, None, 1, ROWS, COLS, None, True, True, e.p(), None, 0, 0, 0, 0, 0, 0,
                                                                                   **accumulate_outs(e)),
                                                   nc.denoise_accumulate_curve_dev(e.s, e.p(), e.p(), e.p(), e.p(), CH, ROWS, COLS, e.p(), False, True, e.p(), e.p(), 2 ** 33, 1, 40, 24,
                                                                                   2 ** 34, 2 ** 35, **accumulate_outs(e))]),
    ("denoise_accumulate_curve_dev/refused", _fails2("rsdsfm_denoise_accumulate_curve_dev", -1, lambda e, nc: nc.denoise_accumulate_curve_dev(
        e.s, e.p(), e.p(), e.p(), e.p(), CH, ROWS, COLS, e.p(), True, True, None))),
    ("denoise_spatial_curve_dev", lambda e, nc: [nc.denoise_spatial_curve_dev(e.s, e.p(), e.p(), None, CH, ROWS, COLS, e.p(), e.p()),
                                                nc.denoise_spatial_curve_dev(e.s, e.p(), e.p(), e.p(), 1, ROWS, COLS, e.p(), e.p(), e.p(), e.p(), 40, 24, 2 ** 34, 2 ** 35, 70, 3)]),
    ("denoise_spatial_curve_dev/refused", _fails2("rsdsfm_denoise_spatial_curve_dev", -1, lambda e, nc: nc.denoise_spatial_curve_dev(e.s, e.p(), e.p(), None, CH, ROWS, COLS, None,
                                                                                                                                   e.p()))),
    ("denoise_curve_frame_dev", lambda e, nc: [nc.denoise_curve_frame_dev(e.s, *frame(e, 3)),
                                              nc.denoise_curve_frame_dev(e.s, *frame(e, 2, 1), e.p(), e.p(), e.p(), e.p(), 40, False, 2 ** 33, (1, 2, 30, 40), True, 5000, 1, 1, 5, None, 200,
                                                                         24, 2 ** 34, 2 ** 35, None, True, 120, 60, 3),
                                              nc.denoise_curve_frame_dev(e.s, *frame(e, 1), d_curve36=e.p(), spatial=True)]),
    ("denoise_curve_frame_dev/params", lambda e, nc: nc.denoise_curve_frame_dev(
        e.s, *frame(e, 2), params=e.m.DenoiseParams(radius=3, strength=41, struct_bytes=48), curve_params=nc.NoiseCurveParams(quantile_q8=77, scale=9, struct_bytes=48,
                                                                                                                              min_samples=2 ** 33, band_min_samples=19),
        spatial_params=e.m.DenoiseSpatialParams(strength=7, target=90, search=1, struct_bytes=32))),
    ("denoise_curve_frame_dev/pose missing", lambda e, nc: nc.denoise_curve_frame_dev(e.s, e.P(3), CH, e.P(3), e.P(3), e.P(3), K, ROWS, COLS, ar(2, 3, 3), ar(3, 3), e.p(), e.p())),
    ("denoise_curve_frame_dev/pose table missing", lambda e, nc: nc.denoise_curve_frame_dev(e.s, e.P(2), CH, e.P(2), e.P(1), e.P(2), K, ROWS, COLS, ar(2, 3, 3), ar(2, 3, off=1), e.p(),
                                                                                          e.p())),
    ("denoise_curve_frame_dev/refused", _fails2("rsdsfm_denoise_curve_frame_dev", -1, lambda e, nc: nc.denoise_curve_frame_dev(e.s, *frame(e, 2)))),
    ("denoise_curve_video_dev", lambda e, nc: nc.denoise_curve_video_dev(e.s, *clip(e, 3), e.P(3), e.P(3))),
    ("denoise_curve_video_dev/everything", lambda e, nc: nc.denoise_curve_video_dev(e.s, *clip(e, 3), e.P(4), e.P(3), e.P(3), e.P(3), False, True, 3, 40, False, 2 ** 33, (1, 2, 30, 40),
                                                                                    True, 5000, 1, 1, 5, 200, 24, 2 ** 34, 2 ** 35, True, 120, 60, 3)),
    ("denoise_curve_video_dev/no host arrays", lambda e, nc: nc.denoise_curve_video_dev(e.s, *clip(e, 2), e.P(2), e.P(2), want_counts=False, want_curves=False)),
    ("denoise_curve_video_dev/counts only", lambda e, nc: nc.denoise_curve_video_dev(e.s, *clip(e, 2), e.P(2), e.P(2), None, None, True, False)),
    ("denoise_curve_video_dev/out one short", lambda e, nc: nc.denoise_curve_video_dev(e.s, *clip(e, 3), e.P(3), e.P(2))),
    ("denoise_curve_video_dev/too few scales", lambda e, nc: nc.denoise_curve_video_dev(e.s, *clip(e, 3)[:12], ar(2), e.P(3), e.P(3))),
    ("denoise_curve_video_dev/refused", _fails2("rsdsfm_denoise_curve_video_dev", -1, lambda e, nc: nc.denoise_curve_video_dev(e.s, *clip(e, 2), e.P(2), e.P(2)))),
]

# the *_dev functions of the module: each needs a case above
DEV_FUNCTIONS = ("noise_curve_dev", "denoise_accumulate_curve_dev", "denoise_spatial_curve_dev", "denoise_curve_frame_dev", "denoise_curve_video_dev")

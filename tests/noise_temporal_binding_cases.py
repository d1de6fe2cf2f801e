"""The table of calls tests/test_noise_temporal_cpu.py replays on the recording library (tests/binding_recorder.py) for rsdsfm_noise_temporal.py:
one entry or more per function that reaches the library, both sides of every optional argument, params= pass-through, window=, want_counts= and
want_curves=, and refusals with their text.  A case is (name, function of the recorder's Env and the module); tests/binding_cases.py's helpers
are imported unchanged.  The golden is tests/golden/noise_temporal_calls_v1.json.gz (tests/golden/make_golden_noise_temporal.py)."""
from binding_cases import CH, COLS, K, ROWS, ar, clip, frame


def _fails2(name, rc, fn):
    def run(e, nt):
        e.lib.returns[name] = rc
        return fn(e, nt)
    return run


CASES = [
    ("noise_temporal_launches", lambda e, nt: [nt.noise_pair_hist_launches(), nt.noise_curve_resolve_launches()]),
    ("denoise_temporal_frame_launches", lambda e, nt: [nt.denoise_temporal_frame_launches(ROWS, COLS, 3), nt.denoise_temporal_frame_launches(ROWS, COLS, 5, True)]),
    ("denoise_temporal_frame_launches/refused", _fails2("rsdsfm_denoise_temporal_frame_launches", -1, lambda e, nt: nt.denoise_temporal_frame_launches(1, COLS, 3))),
    ("noise_pair_hist_dev", lambda e, nt: [nt.noise_pair_hist_dev(e.s, e.p(), e.p(), e.p(), e.p(), CH, ROWS, COLS, e.p()),
                                           nt.noise_pair_hist_dev(e.s, e.p(), e.p(), e.p(), e.p(), 1, ROWS, COLS, e.p(), False, e.p(), 2 ** 33, 1),
                                           nt.noise_pair_hist_dev(e.s, e.p(), e.p(), e.p(), e.p(), CH, ROWS, COLS, e.p(), first=True, d_sums8=None, min_overlap=5000)]),
    ("noise_pair_hist_dev/refused", _fails2("rsdsfm_noise_pair_hist_dev", -1, lambda e, nt: nt.noise_pair_hist_dev(e.s, e.p(), e.p(), None, None, 2, ROWS, COLS, e.p()))),
    ("noise_curve_resolve_dev", lambda e, nt: [nt.noise_curve_resolve_dev(e.s, e.p(), e.p()), nt.noise_curve_resolve_dev(e.s, e.p(), e.p(), 200)]),
    ("noise_curve_resolve_dev/refused", _fails2("rsdsfm_noise_curve_resolve_dev", -1, lambda e, nt: nt.noise_curve_resolve_dev(e.s, None, e.p(), 257))),
    ("denoise_temporal_frame_dev", lambda e, nt: [nt.denoise_temporal_frame_dev(e.s, *frame(e, 3)),
                                                  nt.denoise_temporal_frame_dev(e.s, *frame(e, 2, 1), e.p(), e.p(), e.p(), e.p(), 40, False, 2 ** 33, (1, 2, 30, 40), True, 5000, 1, 1, 5,
                                                                                None, 200, 24, 2 ** 34, 2 ** 35, None, True, 120, 60, 3),
                                                  nt.denoise_temporal_frame_dev(e.s, *frame(e, 1), d_curve36=e.p(), spatial=True)]),
    ("denoise_temporal_frame_dev/params", lambda e, nt: nt.denoise_temporal_frame_dev(
        e.s, *frame(e, 2), params=e.m.DenoiseParams(radius=3, strength=41, struct_bytes=48), curve_params=nt.NoiseCurveParams(quantile_q8=77, scale=9, struct_bytes=48,
                                                                                                                              min_samples=2 ** 33, band_min_samples=19),
        spatial_params=e.m.DenoiseSpatialParams(strength=7, target=90, search=1, struct_bytes=32))),
    ("denoise_temporal_frame_dev/pose missing", lambda e, nt: nt.denoise_temporal_frame_dev(e.s, e.P(3), CH, e.P(3), e.P(3), e.P(3), K, ROWS, COLS, ar(2, 3, 3), ar(3, 3), e.p(),
                                                                                            e.p())),
    ("denoise_temporal_frame_dev/pose table missing", lambda e, nt: nt.denoise_temporal_frame_dev(e.s, e.P(2), CH, e.P(2), e.P(1), e.P(2), K, ROWS, COLS, ar(2, 3, 3),
                                                                                                  ar(2, 3, off=1), e.p(), e.p())),
    ("denoise_temporal_frame_dev/refused", _fails2("rsdsfm_denoise_temporal_frame_dev", -1, lambda e, nt: nt.denoise_temporal_frame_dev(e.s, *frame(e, 2)))),
    ("denoise_temporal_video_dev", lambda e, nt: nt.denoise_temporal_video_dev(e.s, *clip(e, 3), e.P(3), e.P(3))),
    ("denoise_temporal_video_dev/everything", lambda e, nt: nt.denoise_temporal_video_dev(e.s, *clip(e, 3), e.P(4), e.P(3), e.P(3), e.P(3), False, True, 3, 40, False, 2 ** 33,
                                                                                          (1, 2, 30, 40), True, 5000, 1, 1, 5, 200, 24, 2 ** 34, 2 ** 35, True, 120, 60, 3)),
    ("denoise_temporal_video_dev/no host arrays", lambda e, nt: nt.denoise_temporal_video_dev(e.s, *clip(e, 2), e.P(2), e.P(2), want_counts=False, want_curves=False)),
    ("denoise_temporal_video_dev/counts only", lambda e, nt: nt.denoise_temporal_video_dev(e.s, *clip(e, 2), e.P(2), e.P(2), None, None, True, False)),
    ("denoise_temporal_video_dev/out one short", lambda e, nt: nt.denoise_temporal_video_dev(e.s, *clip(e, 3), e.P(3), e.P(2))),
    ("denoise_temporal_video_dev/too few scales", lambda e, nt: nt.denoise_temporal_video_dev(e.s, *clip(e, 3)[:12], ar(2), e.P(3), e.P(3))),
    ("denoise_temporal_video_dev/refused", _fails2("rsdsfm_denoise_temporal_video_dev", -1, lambda e, nt: nt.denoise_temporal_video_dev(e.s, *clip(e, 2), e.P(2), e.P(2)))),
]

# the *_dev functions of the module: each needs a case above
DEV_FUNCTIONS = ("noise_pair_hist_dev", "noise_curve_resolve_dev", "denoise_temporal_frame_dev", "denoise_temporal_video_dev")

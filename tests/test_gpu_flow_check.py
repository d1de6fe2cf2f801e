"""GPU: the forward-backward flow check (rsdsfm_flow_consistency_dev) bit for bit against its definition (tests/flow_check_spec_numpy.py):
mask bytes, masked field, residual (+inf included) and count, on the fields of tests/flow_check_cases.py -- a consistent majority, a block of
inconsistent vectors, vectors leaving the frame on all four sides, NaN / inf, landing points on and one ulp past the last column and row --
in place, with each optional output missing, at other parameters, in both library builds; and the arguments it refuses."""
import numpy as np
import pytest

import flow_check_cases as cases
import flow_check_spec_numpy as spec

pytestmark = pytest.mark.gpu

_expected = {}


def _case(shape, a1=None, a2=None):
    """inputs and the spec's outputs, computed once per case and shared"""
    key = (shape, a1, a2)
    if key not in _expected:
        fwd, bwd, _ = cases.fields(*shape)
        kw = {k: v for k, v in (("a1", a1), ("a2", a2)) if v is not None}
        _expected[key] = dict(fwd=fwd, bwd=bwd, out=spec.flow_check(fwd, bwd, **kw))
    return _expected[key]


def _run(torch, s, e, a1=None, a2=None, in_place=False, without=()):
    """one call; the output buffers start as 77 / NaN, so an element that is not written shows"""
    dev = torch.device("cuda", 0)
    rows, cols = e["fwd"].shape[:2]
    d_fwd, d_bwd = torch.from_numpy(e["fwd"]).to(dev), torch.from_numpy(e["bwd"]).to(dev)
    mask = torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
    masked = d_fwd if in_place else torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev)
    resid = torch.full((rows, cols), np.nan, dtype=torch.float64, device=dev)
    count = torch.full((1,), 77, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptr = lambda name, t: None if name in without else t.data_ptr()
    s.flow_consistency_dev(d_fwd.data_ptr(), d_bwd.data_ptr(), rows, cols, mask.data_ptr(), ptr("masked", masked), ptr("resid", resid), ptr("count", count),
                           a1=a1, a2=a2)
    s.synchronize()
    return dict(mask=mask.cpu().numpy(), masked=masked.cpu().numpy(), resid=resid.cpu().numpy(), count=int(count.cpu()[0]), bwd=d_bwd.cpu().numpy())


def _check(got, want, without=()):
    assert np.array_equal(got["mask"], want["mask"])  # (1 or 0: no 77 left)
    if "masked" in without:
        assert np.isnan(got["masked"]).all()
    else:
        assert np.array_equal(got["masked"].view(np.uint64), want["masked"].view(np.uint64))
    if "resid" in without:
        assert np.isnan(got["resid"]).all()
    else:
        assert np.array_equal(got["resid"].view(np.uint64), want["resid"].view(np.uint64))
    assert got["count"] == (77 if "count" in without else want["count"])


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_flow_check_equals_the_spec(rsdsfm, shape):
    import torch

    e = _case(shape)
    with rsdsfm.Solver(0) as s:
        _check(_run(torch, s, e), e["out"])
        got = _run(torch, s, e, in_place=True)  # d_masked == d_fwd
        _check(got, e["out"])
        assert np.array_equal(got["bwd"].view(np.uint64), e["bwd"].view(np.uint64))
    if min(shape) >= 16:
        assert 0 < e["out"]["count"] < shape[0] * shape[1] and np.isinf(e["out"]["resid"]).any()


@pytest.mark.parametrize("without", ["masked", "resid", "count"])
def test_each_optional_output_may_be_missing(rsdsfm, without):
    import torch

    e = _case((33, 70))
    with rsdsfm.Solver(0) as s:
        _check(_run(torch, s, e, without=(without,)), e["out"], without=(without,))
        _check(_run(torch, s, e, without=("masked", "resid", "count")), e["out"], without=("masked", "resid", "count"))


@pytest.mark.parametrize("a1,a2", [(0.05, 0.02), (0.0, 0.0), (0.0, 20.0)])
def test_other_parameters(rsdsfm, a1, a2):
    import torch

    for shape in ((33, 70), (150, 200)):
        e = _case(shape, a1, a2)
        assert e["out"]["count"] != _case(shape)["out"]["count"]
        with rsdsfm.Solver(0) as s:
            _check(_run(torch, s, e, a1=a1, a2=a2), e["out"])


def test_both_library_builds_give_the_same_bytes(rsdsfm):
    import torch

    e = _case((150, 200))
    with rsdsfm.Solver(0, arith="fused") as s:
        _check(_run(torch, s, e), e["out"])


def test_host_convenience_call(rsdsfm):
    e = _case((33, 68))
    with rsdsfm.Solver(0) as s:
        got = s.flow_consistency(e["fwd"], e["bwd"])
    _check(got, e["out"])


def test_refused_arguments(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 8, 12
    f, b = (torch.zeros((rows, cols, 2), dtype=torch.float64, device=dev) for _ in range(2))
    spare = torch.zeros((rows, cols, 2), dtype=torch.float64, device=dev)
    mask = torch.zeros(rows * cols + 4, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        call = lambda *a, **kw: s.flow_consistency_dev(*a, **kw)
        fp, bp, mp = f.data_ptr(), b.data_ptr(), mask.data_ptr()
        call(fp, bp, rows, cols, mp, fp, spare.data_ptr(), count.data_ptr())  # (the accepted form, in place)
        for bad in (lambda: call(fp, bp, 1, cols, mp),                      # a side of 1
                    lambda: call(fp, bp, rows, 1, mp),
                    lambda: call(fp, bp, rows, 16385, mp),
                    lambda: call(fp, bp, rows, cols, mp + 1),               # a misaligned mask
                    lambda: call(fp, bp, rows, cols, mp, bp),               # the masked field over the backward field
                    lambda: call(fp, bp, rows, cols, mp, None, fp),         # the residual over the forward field
                    lambda: call(fp, bp, rows, cols, mp, spare.data_ptr(), spare.data_ptr()),  # two outputs in one buffer
                    lambda: call(fp, bp, rows, cols, fp),                   # the mask over an input
                    lambda: call(0, bp, rows, cols, mp),
                    lambda: call(fp, bp, rows, cols, mp, a1=-0.01),         # a negative a1
                    lambda: call(fp, bp, rows, cols, mp, a2=float("nan")),
                    lambda: call(fp, bp, rows, cols, mp, a1=float("inf"))):
            with pytest.raises(rsdsfm.RsdsfmError):
                bad()
        s.synchronize()
    assert not mask.cpu().numpy()[rows * cols:].any()

"""GPU: the link kernels (rsdsfm_link_pairs_dev) against tests/link_spec_numpy.py bit for bit -- the ratio plane as written, n, the lower
median, agree and valid -- on the cases of tests/link_cases.py at sizes around the LDS tile and the wave, with both digit widths of the
selection and both library builds; several links in one call; the context's planes; the argument checks."""
import numpy as np
import pytest

import link_cases as cases
import link_spec_numpy as spec

pytestmark = pytest.mark.gpu

_SPEC = {}


def _shape_cases(rows, cols):
    """(name, inputs, the spec's outputs) of one shape, computed once and shared by the tests (which do not modify them)"""
    if (rows, cols) not in _SPEC:
        out = [("holes %g" % h, cases.base_case(rows, cols, h)) for h in cases.HOLES]
        out += [("specials", cases.special_case(rows, cols)[0]), ("empty", cases.empty_case(rows, cols)), ("negative z_pred", cases.negative_prediction_case(rows, cols)),
                ("wide ratios", cases.wide_ratios(rows, cols)), ("all equal", cases.planted_case(rows, cols, [0.8125], share=1.0)),
                ("two values", cases.two_values_on_the_boundary(rows, cols))]
        gs = cases.base_case(rows, cols, 0.3, salt=29)
        gs["global_shutter"] = True
        out.append(("global shutter", gs))
        _SPEC[(rows, cols)] = [(name, d, spec.link(d["F"], d["Zp"], d["v"], d["w"], d["k"], d["Zn"], d["K"], d["gamma"], d.get("global_shutter", False)))
                               for name, d in out]
    return _SPEC[(rows, cols)]


def _same_record(got, want, what):
    assert got["n"] == want["n"] and got["agree"] == want["agree"] and got["valid"] == want["valid"], (what, got, {k: want[k] for k in ("n", "ratio", "agree", "valid")})
    if want["n"] == 0:
        assert np.isnan(got["ratio"]), what
    else:
        assert np.float64(got["ratio"]).view(np.uint64) == np.float64(want["ratio"]).view(np.uint64), (what, got["ratio"], want["ratio"])


@pytest.fixture(scope="module")
def solvers(rsdsfm):
    made = {}

    def get(arith):
        if arith not in made:
            made[arith] = rsdsfm.Solver(0, arith=arith)
        return made[arith]

    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_single_links_equal_the_spec(solvers, shape, arith):
    s = solvers(arith)
    for name, d, want in _shape_cases(*shape):
        for bits in (None, 8):
            got = s.link_pairs([d["F"]], [d["Zp"], d["Zn"]], [d["v"]] * 2, [d["w"]] * 2, [d["k"]] * 2, d["K"], d["gamma"], d.get("global_shutter", False),
                               radix_bits=bits, want_planes=True)[0]
            assert np.array_equal(got["plane"], want["plane"]), (name, bits, int((got["plane"] != want["plane"]).sum()))
            _same_record(got, want, (name, bits))


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("shape", [(17, 70), (65, 129), (150, 200)])
def test_several_links_in_one_call(solvers, shape, arith):
    """six pairs chained from maps with different hole shares, a map without a valid pixel and a planted one: five links with different n
    in the same launches (a link must not see another's histogram), with the caller's planes and with the context's"""
    rows, cols = shape
    s = solvers(arith)
    parts = [cases.base_case(rows, cols, h, salt=31 + i) for i, h in enumerate((0.0, 0.3, 0.97, 0.5))]
    maps = [parts[0]["Zp"], parts[1]["Zn"], parts[2]["Zp"], cases.empty_case(rows, cols)["Zp"], parts[3]["Zn"], cases.wide_ratios(rows, cols)["Zn"]]
    fields = [p["F"] for p in parts] + [np.zeros((rows, cols, 2))]
    vs = [p["v"] * (1 + 0.1 * i) for i, p in enumerate(parts)] + [np.zeros(3)] * 2
    ws = [p["w"] * (1 - 0.1 * i) for i, p in enumerate(parts)] + [np.zeros(3)] * 2
    ks = [0.0, 0.2, -0.1, 0.3, 0.0, 0.0]
    K, gamma = parts[0]["K"], parts[0]["gamma"]
    want = [spec.link(fields[q], maps[q], vs[q], ws[q], ks[q], maps[q + 1], K, gamma, tol=0.05, min_links=100) for q in range(5)]
    assert len({w["n"] for w in want}) >= 4 and want[2]["n"] == 0 == want[3]["n"] and want[0]["n"] > want[1]["n"] > 0
    for bits in (None, 8):
        got = s.link_pairs(fields, maps, vs, ws, ks, K, gamma, tol=0.05, min_links=100, radix_bits=bits, want_planes=True)
        ws_only = s.link_pairs(fields, maps, vs, ws, ks, K, gamma, tol=0.05, min_links=100, radix_bits=bits)
        for q in range(5):
            assert np.array_equal(got[q]["plane"], want[q]["plane"]), (q, bits)
            _same_record(got[q], want[q], (q, bits))
            _same_record(ws_only[q], want[q], (q, bits, "context planes"))
    assert [w["valid"] for w in want] != [True] * 5  # min_links = 100 makes the thin links invalid


def test_arguments_are_checked(rsdsfm, solvers):
    import torch

    s = solvers("reference")
    dev = torch.device("cuda", 0)
    rows, cols = 17, 70
    d = cases.base_case(rows, cols, 0.3)
    f = torch.from_numpy(d["F"]).to(dev)
    zp, zn = (torch.from_numpy(np.ascontiguousarray(z.T)).to(dev) for z in (d["Zp"], d["Zn"]))
    plane = torch.zeros((rows, cols), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    args = lambda **kw: dict(dict(d_fields=[f.data_ptr()], d_depth_maps=[zp.data_ptr(), zn.data_ptr()], vs=[d["v"]] * 2, ws=[d["w"]] * 2, ks=[d["k"]] * 2, rows=rows,
                                  cols=cols, K=d["K"], gamma=d["gamma"]), **kw)
    good = s.link_pairs_dev(**args(d_planes=[plane.data_ptr()]))
    assert good[0]["n"] > 0
    for bad in (dict(radix_bits=7), dict(tol=-0.1), dict(tol=float("nan")), dict(min_links=-1), dict(gamma=0.0), dict(rows=1), dict(cols=20000),
                dict(d_fields=[0]), dict(d_depth_maps=[zp.data_ptr(), 0]), dict(d_planes=[0]), dict(d_planes=[zn.data_ptr()]), dict(d_planes=[f.data_ptr()])):
        with pytest.raises(rsdsfm.RsdsfmError):
            s.link_pairs_dev(**args(**bad))
    with pytest.raises(rsdsfm.RsdsfmError):  # one pair has no link
        s.link_pairs_dev([f.data_ptr()], [zp.data_ptr()], [d["v"]], [d["w"]], [d["k"]], rows, cols, d["K"], d["gamma"])
    import ctypes as C

    p = rsdsfm.LinkParams(0.1, 16, 0, 20, 0)  # a struct of another layout
    rec = (rsdsfm.LinkRecord * 1)()
    rc = s.lib.rsdsfm_link_pairs_dev(s._ctx, rsdsfm._ptr_array([f.data_ptr(), 0]), rsdsfm._ptr_array([zp.data_ptr(), zn.data_ptr()]), rsdsfm._p(np.zeros(6)),
                                     rsdsfm._p(np.zeros(6)), rsdsfm._p(np.zeros(2)), C.c_int32(2), C.c_int32(rows), C.c_int32(cols), C.c_double(50.0), C.c_double(50.0),
                                     C.c_double(35.0), C.c_double(8.0), C.c_double(0.8), C.c_int32(0), C.byref(p), None, rec)
    assert rc == -1 and b"struct_bytes" in s.lib.rsdsfm_last_error(s._ctx)
    # the context still works
    again = s.link_pairs_dev(**args())
    assert again[0] == good[0]

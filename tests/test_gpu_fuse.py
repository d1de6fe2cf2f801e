"""GPU: the fusion kernels (rsdsfm_fuse_depths_dev) against tests/fuse_spec_numpy.py bit for bit -- fused maps, flags, splat planes and
records, no pixel excluded, over output buffers prefilled with 0xCD -- on the chains of tests/fuse_cases.py at sizes around the LDS tile and
the wave, with both library builds; the special chain; 34 pairs across the 32-plane chunk; the workspace's planes; optional outputs; the
enqueue-only form; the argument checks; the dense rectifier on a fused map; the clip form behind rsdsfm_solve_video_linked_dev; and the
accuracy of the filled depths through the library's solve."""
import ctypes as C

import numpy as np
import pytest

import fuse_cases as cases
import fuse_spec_numpy as spec
import link_cases
import link_spec_numpy as link_spec
from test_gpu_video import _buffers, _record, _scaled_motion

pytestmark = pytest.mark.gpu

TRIALS = 20
_SPEC = {}


def _expected(key, make):
    """a chain and the spec's outputs, computed once per key and shared by the tests (which do not modify them)"""
    if key not in _SPEC:
        ch = make()
        _SPEC[key] = (ch, spec.fuse(ch["fields"], ch["maps"], ch["vs"], ch["ws"], ch["ks"], ch["records"], ch["K"], ch["gamma"], ch.get("global_shutter", False),
                                    ch.get("tol", link_spec.TOL_DEFAULT)))
    return _SPEC[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _Device:
    """a chain's inputs on the device and output buffers prefilled with 0xCD"""

    def __init__(self, torch, ch, flags=True, planes=True):
        self.torch, self.ch = torch, ch
        dev = torch.device("cuda", 0)
        self.n = n = len(ch["maps"])
        self.rows, self.cols = rows, cols = ch["maps"][0].shape
        self.d_f = [torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).to(dev) for f in ch["fields"][:n - 1]]
        self.d_z = [torch.from_numpy(np.ascontiguousarray(np.asarray(m, dtype=np.float64).T)).to(dev) for m in ch["maps"]]
        cd = lambda nbytes: torch.full((nbytes,), 0xCD, dtype=torch.uint8, device=dev)
        self.d_out = [cd(8 * rows * cols) for _ in range(n)]
        self.d_fl = [cd(rows * cols) for _ in range(n)] if flags else None
        self.d_pl = [cd(8 * rows * cols) for _ in range(n - 1)] if planes else None
        torch.cuda.synchronize()

    def args(self, **kw):
        ch, p = self.ch, lambda ts: [t.data_ptr() for t in ts] if ts is not None else None
        a = dict(d_fields=p(self.d_f), d_depth_maps=p(self.d_z), vs=ch["vs"], ws=ch["ws"], ks=ch["ks"], rows=self.rows, cols=self.cols, K=ch["K"], gamma=ch["gamma"],
                 records=ch["records"], d_fused=p(self.d_out), global_shutter=ch.get("global_shutter", False), d_flags=p(self.d_fl), d_planes=p(self.d_pl),
                 tol=ch.get("tol"))
        a.update(kw)
        return a

    def run(self, s, **kw):
        rec = s.fuse_depths_dev(**self.args(**kw))
        s.synchronize()
        return self.download(rec)

    def download(self, rec=None):
        rows, cols = self.rows, self.cols
        out = dict(records=rec, fused=[t.cpu().numpy().view(np.uint64).reshape(cols, rows).T for t in self.d_out])
        if self.d_fl is not None:
            out["flags"] = [t.cpu().numpy().reshape(rows, cols) for t in self.d_fl]
        if self.d_pl is not None:
            out["planes"] = [t.cpu().numpy().view(np.uint64).reshape(rows, cols) for t in self.d_pl]
        return out


def _same(got, want, what=""):
    for p, f in enumerate(want["fused"]):
        assert np.array_equal(got["fused"][p], _bits(f)), (what, "fused", p, int((got["fused"][p] != _bits(f)).sum()))
        if "flags" in got:
            assert np.array_equal(got["flags"][p], want["flags"][p]), (what, "flags", p, int((got["flags"][p] != want["flags"][p]).sum()))
    if "planes" in got:
        for l, pl in enumerate(want["splat"]):
            assert np.array_equal(got["planes"][l], pl), (what, "plane", l, int((got["planes"][l] != pl).sum()))
    if got["records"] is not None:
        assert got["records"] == want["records"], (what, got["records"], want["records"])


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
@pytest.mark.parametrize("holes", cases.HOLES)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_three_pair_chains_equal_the_spec(solvers, shape, holes, arith):
    import torch

    ch, want = _expected(("chain", shape, holes), lambda: cases.chain_case(*shape, 3, holes))
    _same(_Device(torch, ch).run(solvers(arith)), want, (shape, holes))


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("shape", cases.SPECIAL_SHAPES)
def test_special_chain_equals_the_spec(solvers, shape, arith):
    """NaN / inf / negative depths in every map, NaN / inf / (0, 0) vectors, vectors leaving every border and landing on the last row and
    column, negative z_pred and zc, collisions, a map without a valid pixel, each kind of broken link, global-shutter mode, tol = 0.01;
    and the first pair alone"""
    import torch

    s = solvers(arith)
    for broken in sorted(cases.BROKEN):
        ch, want = _expected(("special", shape, broken), lambda: cases.special_chain(*shape, broken))
        _same(_Device(torch, ch).run(s), want, (shape, broken))
    ch, want = _expected(("special gs", shape), lambda: dict(cases.special_chain(*shape), global_shutter=True, tol=0.01))
    _same(_Device(torch, ch).run(s), want, (shape, "global shutter, tol 0.01"))

    def one():
        c = cases.special_chain(*shape)
        return dict(c, fields=[], maps=c["maps"][:1], vs=c["vs"][:1], ws=c["ws"][:1], ks=c["ks"][:1], records=[])

    ch, want = _expected(("one pair", shape), one)
    got = _Device(torch, ch).run(s)
    _same(got, want, (shape, "one pair"))
    own = link_spec.valid_depth(ch["maps"][0])
    assert np.array_equal(got["fused"][0], np.where(own, _bits(ch["maps"][0]), np.uint64(0))) and np.array_equal(got["flags"][0], own.astype(np.uint8))


def test_34_pairs_cross_the_chunk_boundary(solvers):
    """pairs 0 .. 31 and 32 .. 33 run in two chunks; link 31's plane belongs to the second; caller's planes and the workspace's"""
    import torch

    ch, want = _expected(("long",), lambda: cases.chain_case(17, 70, 34, 0.3, salt=5))
    assert want["records"][32]["filled_prev"] > 0 and want["records"][31]["filled_next"] > 0
    s = solvers("reference")
    _same(_Device(torch, ch).run(s), want, "34 pairs")
    _same(_Device(torch, ch, planes=False).run(s), want, "34 pairs, workspace planes")


def test_workspace_planes_optional_outputs_and_the_enqueue_only_form(rsdsfm, solvers):
    import torch

    ch, want = _expected(("special", (65, 129), "invalid"), lambda: cases.special_chain(65, 129, "invalid"))
    s = solvers("reference")
    full = _Device(torch, ch).run(s)
    _same(full, want)
    for flags, planes in ((True, False), (False, True), (False, False)):
        got = _Device(torch, ch, flags=flags, planes=planes).run(s)
        _same(got, want, (flags, planes))
        assert all(np.array_equal(a, b) for a, b in zip(got["fused"], full["fused"]))
    # without the records the call only enqueues: the same bytes after a wait
    d = _Device(torch, ch)
    assert s.fuse_depths_dev(**d.args(want_records=False)) is None
    s.synchronize()
    _same(d.download(), want, "enqueue only")
    # the host convenience
    host = s.fuse_depths(ch["fields"][:5], ch["maps"], ch["vs"], ch["ws"], ch["ks"], ch["records"], ch["K"], ch["gamma"], want_flags=True, want_planes=True)
    _same(dict(fused=[_bits(f) for f in host["fused"]], flags=host["flags"], planes=host["planes"], records=host["records"]), want, "fuse_depths")


def test_arguments_are_checked(rsdsfm, solvers):
    import torch

    ch, want = _expected(("chain", (17, 70), 0.3), lambda: cases.chain_case(17, 70, 3, 0.3))
    s = solvers("reference")
    d = _Device(torch, ch)
    a = d.args()
    spare = torch.full((8 * 17 * 70,), 0xCD, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    swap = lambda lst, i, v: lst[:i] + [v] + lst[i + 1:]
    bad = [dict(rows=1), dict(cols=20000), dict(rows=16385), dict(tol=-0.1), dict(tol=float("nan")), dict(tol=float("inf")), dict(gamma=0.0),
           dict(d_fields=swap(a["d_fields"], 0, 0)), dict(d_depth_maps=swap(a["d_depth_maps"], 2, 0)), dict(d_fused=swap(a["d_fused"], 1, 0)),
           dict(d_flags=swap(a["d_flags"], 1, 0)), dict(d_planes=swap(a["d_planes"], 1, 0)),
           dict(d_fused=swap(a["d_fused"], 0, a["d_depth_maps"][1])), dict(d_fused=swap(a["d_fused"], 2, a["d_fields"][0])),
           dict(d_fused=swap(a["d_fused"], 0, a["d_fused"][1])), dict(d_planes=swap(a["d_planes"], 0, a["d_depth_maps"][2])),
           dict(d_flags=swap(a["d_flags"], 0, a["d_fused"][2])), dict(d_planes=swap(a["d_planes"], 1, a["d_flags"][0]))]
    for kw in bad:
        with pytest.raises(rsdsfm.RsdsfmError):
            s.fuse_depths_dev(**d.args(**kw))
    # npairs < 1, NULL host pointers, NULL records with two pairs, a struct of another layout: the C entry point itself
    P = rsdsfm._ptr_array
    zeros = np.zeros(9)

    def call(npairs, v=zeros, records=True, params=None, fused=a["d_fused"]):
        rec = (rsdsfm.LinkRecord * 2)()
        rec[0].ratio = rec[1].ratio = 1.5
        rec[0].valid = rec[1].valid = 1
        return s.lib.rsdsfm_fuse_depths_dev(s._ctx, P(a["d_fields"] + [0]), P(a["d_depth_maps"]), rsdsfm._p(v) if v is not None else None, rsdsfm._p(zeros),
                                            rsdsfm._p(zeros), C.c_int32(npairs), C.c_int32(17), C.c_int32(70), C.c_double(50.0), C.c_double(50.0), C.c_double(35.0),
                                            C.c_double(8.0), C.c_double(0.8), C.c_int32(0), rec if records else None, C.byref(params) if params is not None else None,
                                            P(fused) if fused is not None else None, P(a["d_flags"]), P(a["d_planes"] + [0]), None)

    assert call(0) == -1 and call(-3) == -1 and call(3, v=None) == -1 and call(3, records=False) == -1 and call(3, fused=None) == -1
    assert call(3, params=rsdsfm.FuseParams(0.1, 20, 0)) == -1 and b"struct_bytes" in s.lib.rsdsfm_last_error(s._ctx)
    s.synchronize()
    # no refused call touched an output
    got = d.download()
    for t in got["fused"] + got["planes"]:
        assert np.all(t == np.uint64(0xCDCDCDCDCDCDCDCD))
    assert all(np.all(t == 0xCD) for t in got["flags"]) and bool(torch.all(spare == 0xCD))
    # a zero-initialised struct is the caller's tol; the context still works
    assert call(3, params=rsdsfm.FuseParams(0.1, 0, 0)) == 0 and call(1, records=False) == 0
    _same(d.run(s), want, "after the refused calls")


def test_dense_rectifier_reads_a_fused_map(oracle, rsdsfm):
    """rsdsfm_rectify_dense_frame_dev on the device's fused map of the middle pair of a (65, 129) chain equals its definition
    (tests/rectify_dense_spec_numpy.py) on the spec's fused map"""
    import torch

    import rectify_dense_cases as dense_cases
    import rectify_dense_spec_numpy as dense_spec

    rows, cols = 65, 129
    ch, want = _expected(("chain", (rows, cols), 0.3), lambda: cases.chain_case(rows, cols, 3, 0.3))
    assert want["records"][1]["filled_prev"] > 0 and want["records"][1]["left"] > 0
    K, image, _ = dense_cases.inputs(rows, cols, channels=3)
    R, t = oracle.pose_table(dense_cases.POSE["v"], dense_cases.POSE["w"], dense_cases.POSE["k"], dense_cases.POSE["gamma"], rows)
    R = np.ascontiguousarray(R).reshape(rows, 9)
    exp = dense_spec.rectify_dense(image, want["fused"][1], R, t, *K)
    own = dense_spec.rectify_dense(image, ch["maps"][1], R, t, *K)
    assert not np.array_equal(exp["image"], own["image"])  # the fill matters
    dev = torch.device("cuda", 0)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_img, d_R, d_t = tt(image), tt(R), tt(t)
    out, mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
    with rsdsfm.Solver(0) as s:
        d = _Device(torch, ch)
        s.fuse_depths_dev(**d.args(want_records=False))
        s.rectify_dense_frame_dev(d_img.data_ptr(), 3, d.d_out[1].data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, out.data_ptr(), mask.data_ptr())
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), exp["image"]) and np.array_equal(mask.cpu().numpy(), exp["mask"])


# ---- the clip form --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip_runs(rsdsfm):
    """the rendered sequence of tests/test_gpu_video_linked.py (96 x 128, five frames) through solve_video_linked_dev with and without
    d_fused, each followed by a plain clip call on the same context: run once, read by the tests below"""
    import torch

    rows, cols, gamma = 96, 128, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v, w, k, gamma, seed=21, speeds=(1.0, 1.4, 0.8, 1.0))
    seeds, n = [3 + 5 * i for i in range(4)], 4
    dev = torch.device("cuda", 0)
    ptrs = lambda a: [t.data_ptr() for t in a]
    runs = {}
    for fused in (True, False):
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
        dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
        cd = lambda nbytes: torch.full((nbytes,), 0xCD, dtype=torch.uint8, device=dev)
        d_fu, d_fl = [cd(8 * rows * cols) for _ in range(n)], [cd(rows * cols) for _ in range(n)]
        d_fu2, d_fl2 = [cd(8 * rows * cols) for _ in range(n)], [cd(rows * cols) for _ in range(n)]
        torch.cuda.synchronize()
        with rsdsfm.Solver(0) as s:
            s.set_flow_batch(8)
            r = s.solve_video_linked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), seeds=seeds, d_R=ptrs(Rs), d_t=ptrs(ts), trials=TRIALS,
                                         **(dict(d_fused=ptrs(d_fu), d_flags=ptrs(d_fl)) if fused else {}))
            s.synchronize()
            out = dict(r=r, records=[_record(x, dms[i], Rs[i], ts[i]) for i, x in enumerate(r["pairs"])], flows=[f.cpu().numpy() for f in d_flows],
                       maps=[m.cpu().numpy().reshape(cols, rows).T.copy() for m in dms])
            view = lambda a, shape: [t.cpu().numpy().view(np.uint64 if shape == "map" else np.uint8) for t in a]
            if fused:
                out["fused"] = [x.reshape(cols, rows).T for x in view(d_fu, "map")]
                out["flags"] = [x.reshape(rows, cols) for x in view(d_fl, "flags")]
                vs, ws, ks = ([x[key] for x in r["pairs"]] for key in ("v", "w", "k"))
                out["again"] = s.fuse_depths_dev(ptrs(d_flows), ptrs(dms), vs, ws, ks, rows, cols, K, gamma, r["links"], ptrs(d_fu2), d_flags=ptrs(d_fl2))
                s.synchronize()
                out["fused_again"] = [x.reshape(cols, rows).T for x in view(d_fu2, "map")]
                out["flags_again"] = [x.reshape(rows, cols) for x in view(d_fl2, "flags")]
            dms2, Rs2, ts2 = _buffers(torch, dev, n, rows, cols)
            torch.cuda.synchronize()
            res2 = s.solve_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms2), seeds=seeds, d_R=ptrs(Rs2), d_t=ptrs(ts2), trials=TRIALS)
            s.synchronize()
            out["plain_after"] = [_record(x, dms2[i], Rs2[i], ts2[i]) for i, x in enumerate(res2)]
        runs[fused] = out
    return dict(runs, K=K, gamma=gamma)


def test_linked_clip_with_fusion_equals_its_parts_and_the_spec(clip_runs):
    a, K, gamma = clip_runs[True], clip_runs["K"], clip_runs["gamma"]
    r = a["r"]
    assert a["again"] == r["fuse"] and len(r["fuse"]) == 4
    for p in range(4):
        assert np.array_equal(a["fused"][p], a["fused_again"][p]) and np.array_equal(a["flags"][p], a["flags_again"][p]), p
    vs, ws, ks = ([x[key] for x in r["pairs"]] for key in ("v", "w", "k"))
    want = spec.fuse(a["flows"], a["maps"], vs, ws, ks, r["links"], K, gamma)
    _same(dict(fused=a["fused"], flags=a["flags"], records=r["fuse"]), want, "clip")
    # (this clip's solve keeps every pixel, so here the fusion confirms and contradicts; the chains above and the accuracy case below fill)
    assert all(l["valid"] for l in r["links"]) and all(x["confirmed"] > 0.9 * x["own"] for x in r["fuse"]) and sum(x["contradicted"] for x in r["fuse"]) > 0
    assert all(x["own"] + x["filled_prev"] + x["filled_next"] + x["left"] == 96 * 128 for x in r["fuse"])


def test_fusion_changes_nothing_else_of_the_linked_clip(clip_runs):
    a, b = clip_runs[True], clip_runs[False]
    assert "fuse" not in b["r"] and a["records"] == b["records"] and a["plain_after"] == b["plain_after"]
    for p in range(4):
        assert np.array_equal(a["flows"][p].view(np.uint64), b["flows"][p].view(np.uint64)) and np.array_equal(_bits(a["maps"][p]), _bits(b["maps"][p])), p
    for x, y in zip(a["r"]["links"], b["r"]["links"]):
        assert (x["n"], x["agree"], x["valid"]) == (y["n"], y["agree"], y["valid"]) and np.float64(x["ratio"]).view(np.uint64) == np.float64(y["ratio"]).view(np.uint64)
    for name in ("scales", "A", "c", "broken"):
        assert np.asarray(a["r"][name]).tobytes() == np.asarray(b["r"][name]).tobytes(), name


def test_fill_accuracy_through_the_gpu_solve(rsdsfm):
    """tests/test_fuse_cpu.py's accuracy case (link_cases' three-pair scene, 96 x 128) with the pairs solved by rsdsfm_solve_frame_dev, linked
    by rsdsfm_link_pairs_dev and fused by rsdsfm_fuse_depths_dev, under the bounds recorded from the CPU: the largest 95th-percentile error
    of PREV-filled pixels 0.131457 there, bound 0.197186 (plus half of it); the smallest share of holes filled 0.730083 there, bound
    0.680083 (less 5 points)."""
    import torch

    sc = link_cases.accuracy_scene(rsdsfm.synth)
    rows, cols, K, gamma = link_cases.ACC_ROWS, link_cases.ACC_COLS, sc["K"], sc["gamma"]
    dev = torch.device("cuda", 0)
    d_f = [torch.from_numpy(f).to(dev) for f in sc["fields"]]
    dms, _, _ = _buffers(torch, dev, 3, rows, cols)
    d_fu = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(3)]
    d_fl = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a]
    with rsdsfm.Solver(0) as s:
        res = []
        for q in range(3):
            res.append(s.solve_frame_dev(d_f[q].data_ptr(), rows, cols, K, gamma, dms[q].data_ptr(), trials=link_cases.ACC_TRIALS, tol=link_cases.ACC_TOL,
                                         seed=link_cases.ACC_SOLVE_SEED, flow_index_mode=rsdsfm.FLOW_GATHERED))
            s.synchronize()
        vs, ws, ks = ([r[key] for r in res] for key in ("v", "w", "k"))
        links = s.link_pairs_dev(ptrs(d_f), ptrs(dms), vs, ws, ks, rows, cols, K, gamma)
        recs = s.fuse_depths_dev(ptrs(d_f), ptrs(dms), vs, ws, ks, rows, cols, K, gamma, links, ptrs(d_fu), d_flags=ptrs(d_fl))
        s.synchronize()
    maps = [m.cpu().numpy().reshape(cols, rows).T for m in dms]
    out = dict(fused=[m.cpu().numpy().reshape(cols, rows).T for m in d_fu], flags=[m.cpu().numpy() for m in d_fl])
    stats = cases.fill_statistics(out, maps, rsdsfm.synth.scene_depth(rows, cols))
    prev_p95, filled = max(x["prev"][1] for x in stats[1:]), min(x["filled"] for x in stats)
    print("records", recs, "PREV-filled p95 per pair", [x["prev"][1] for x in stats], "filled share per pair", [x["filled"] for x in stats])
    assert all(l["valid"] for l in links)
    assert prev_p95 <= cases.ACC_PREV_P95_BOUND and filled >= cases.ACC_FILLED_BOUND


def test_evaluate_real_sequence_with_fusion(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., trajectory=True, fuse=True, dense=True): per pair the fused map, flags and record of Solver.fuse_depths on
    the pairs it returns, the dense frame of the FUSED map, depth_fused.png and fusion.csv; everything else as without fuse"""
    import torch

    rows, cols, gamma = 96, 128, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(4, rows, cols, K, v, w, k, gamma, seed=21, speeds=(1.0, 1.4, 0.8))
    seeds = [3, 8, 13]
    with rsdsfm.Solver(0) as s:
        out = rsdsfm.evaluate.evaluate_real_sequence(s, frames, camera=K, gamma=gamma, out_dir=str(tmp_path / "f"), trials=TRIALS, seeds=seeds, trajectory=True,
                                                     fuse=True, dense=True)
        base = rsdsfm.evaluate.evaluate_real_sequence(s, frames, camera=K, gamma=gamma, out_dir=str(tmp_path / "b"), trials=TRIALS, seeds=seeds, trajectory=True,
                                                      dense=True)
        pairs = out["pairs"]
        again = s.fuse_depths([p["flow"] for p in pairs], [p["depth_map"] for p in pairs], [p["v"] for p in pairs], [p["w"] for p in pairs],
                              [p["k"] for p in pairs], out["links"], K, gamma, want_flags=True)
        # the dense frame of pair 1 is the dense rectifier's on the FUSED map
        dev = torch.device("cuda", 0)
        tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        d_img, d_z, d_R, d_t = tt(frames[1]), tt(pairs[1]["fused_depth"].T), tt(pairs[1]["R"].reshape(rows, 9)), tt(pairs[1]["t"])
        d_out, d_mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s.rectify_dense_frame_dev(d_img.data_ptr(), 3, d_z.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, d_out.data_ptr(), d_mask.data_ptr(),
                                  mode=rsdsfm.BACKPROJECT_RS)
        s.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), pairs[1]["dense_image"]) and np.array_equal(d_mask.cpu().numpy(), pairs[1]["dense_mask"])
    for q, p in enumerate(pairs):
        assert np.array_equal(_bits(p["fused_depth"]), _bits(again["fused"][q])) and np.array_equal(p["fuse_flags"], again["flags"][q]) and p["fuse_record"] == again["records"][q]
        assert np.array_equal(_bits(p["depth_map"]), _bits(base["pairs"][q]["depth_map"])) and "fused_depth" not in base["pairs"][q]
        if np.array_equal(_bits(p["fused_depth"]), _bits(p["depth_map"])):  # (this clip's solve leaves few holes or none)
            assert np.array_equal(p["dense_image"], base["pairs"][q]["dense_image"])
        img = rsdsfm.formats.read_png(str(tmp_path / "f" / str(q) / "depth_fused.png"))
        img = img[..., 0] if img.ndim == 3 else img
        assert np.array_equal(img != 0, p["fused_depth"] > 0) and img[p["fused_depth"] > 0].min() >= 10
        assert not (tmp_path / "b" / str(q) / "depth_fused.png").exists()
    assert not (tmp_path / "b" / "fusion.csv").exists()
    lines = (tmp_path / "f" / "fusion.csv").read_text().strip().split("\n")
    assert lines[0] == "pair,own,filled_prev,filled_next,confirmed,contradicted,left" and len(lines) == 4
    assert lines[1] == ",".join(["0"] + [str(pairs[0]["fuse_record"][k_]) for k_ in spec.RECORD_FIELDS])
    assert (tmp_path / "f" / "poses.csv").read_text() == (tmp_path / "b" / "poses.csv").read_text()

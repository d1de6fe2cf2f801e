"""GPU: whole clips through the linked solve (rsdsfm_solve_video_linked_dev): per pair the results, fields and depth maps of
rsdsfm_solve_video_dev (of rsdsfm_solve_video_checked_dev when masks are passed) byte for byte, the records of rsdsfm_link_pairs_dev on those
outputs, the scales and poses of rsdsfm_chain_clip, the clip's points against the spec in place and out of place -- at every batch size and
lane count; the plain clip call on the same context returns what it returns alone; the accuracy of the scale through the GPU solve."""
import numpy as np
import pytest

import link_cases as cases
import link_spec_numpy as spec
from test_gpu_video import _buffers, _record, _scaled_motion

pytestmark = pytest.mark.gpu

TRIALS = 20


@pytest.fixture(scope="module")
def clip(rsdsfm):
    rows, cols, gamma = 96, 128, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v, w, k, gamma, seed=21, speeds=(1.0, 1.4, 0.8, 1.0))
    return frames, rows, cols, K, gamma, [3 + 5 * i for i in range(4)]


def _run(rsdsfm, torch, clip, batch, lanes, masks, linked, points=None, then_plain=False):
    """one clip call on a fresh context: the plain / checked call, or the linked one"""
    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    d_masks = [torch.full((rows, cols), 77, dtype=torch.uint8, device=dev) for _ in range(n)] if masks else None
    d_points = [torch.from_numpy(p.copy()).to(dev) for p in points] if points is not None else None
    dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    out = {}
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(batch)
        s.set_sequence_lanes(lanes)
        if linked:
            r = s.solve_video_linked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), d_masks=ptrs(d_masks), seeds=seeds, d_R=ptrs(Rs),
                                         d_t=ptrs(ts), d_points=ptrs(d_points), trials=TRIALS)
            res = r["pairs"]
            out.update(links=r["links"], scales=r["scales"], A=r["A"], c=r["c"], broken=r["broken"])
        elif masks:
            res = s.solve_video_checked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_masks), seeds=seeds, d_flows=ptrs(d_flows), d_R=ptrs(Rs),
                                            d_t=ptrs(ts), trials=TRIALS)
        else:
            res = s.solve_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), seeds=seeds, d_flows=ptrs(d_flows), d_R=ptrs(Rs), d_t=ptrs(ts), trials=TRIALS)
        s.synchronize()
        out.update(records=[_record(x, dms[i], Rs[i], ts[i]) for i, x in enumerate(res)], flows=[f.cpu().numpy() for f in d_flows],
                   masks=[m.cpu().numpy() for m in d_masks] if masks else None, v=[x["v"] for x in res], w=[x["w"] for x in res], k=[x["k"] for x in res],
                   points=[p.cpu().numpy() for p in d_points] if d_points is not None else None)
        if linked:
            # the links of rsdsfm_link_pairs_dev on the call's own outputs, on the same context
            out["links_again"] = s.link_pairs_dev(ptrs(d_flows), ptrs(dms), out["v"], out["w"], out["k"], rows, cols, K, gamma)
        if then_plain:
            dms2, Rs2, ts2 = _buffers(torch, dev, n, rows, cols)
            torch.cuda.synchronize()
            res2 = s.solve_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms2), seeds=seeds, d_R=ptrs(Rs2), d_t=ptrs(ts2), trials=TRIALS)
            s.synchronize()
            out["plain_after"] = [_record(x, dms2[i], Rs2[i], ts2[i]) for i, x in enumerate(res2)]
        out["maps"] = [m.cpu().numpy().reshape(cols, rows).T.copy() for m in dms]
    return out


def _same_links(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x["n"], x["agree"], x["valid"]) == (y["n"], y["agree"], y["valid"])
        assert np.float64(x["ratio"]).view(np.uint64) == np.float64(y["ratio"]).view(np.uint64)


@pytest.mark.parametrize("batch,lanes,masks", [(1, 1, False), (2, 0, False), (8, 0, False), (8, 1, False), (1, 0, True), (2, 1, True), (8, 0, True)])
def test_linked_clip_equals_its_parts(rsdsfm, clip, batch, lanes, masks):
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    want = _run(rsdsfm, torch, clip, batch, lanes, masks, linked=False)
    got = _run(rsdsfm, torch, clip, batch, lanes, masks, linked=True)
    assert got["records"] == want["records"]
    for p in range(4):
        assert np.array_equal(got["flows"][p].view(np.uint64), want["flows"][p].view(np.uint64)), p
        if masks:
            assert np.array_equal(got["masks"][p], want["masks"][p]), p
    _same_links(got["links"], got["links_again"])
    # ... which are the spec's on those outputs
    for q in range(3):
        rec = spec.link(got["flows"][q], got["maps"][q], got["v"][q], got["w"][q], got["k"][q], got["maps"][q + 1], K, gamma)
        _same_links([got["links"][q]], [rec])
        assert rec["valid"]
    ch = rsdsfm.chain_clip(got["links"], got["v"], got["w"], gamma)
    for name in ("scales", "A", "c", "broken"):
        assert np.array_equal(np.asarray(got[name]), np.asarray(ch[name])), name
    assert not got["broken"].any() and got["scales"][0] == 1.0 and np.all(got["scales"] > 0)


def test_plain_clip_call_after_a_linked_one(rsdsfm, clip):
    """solve_video_dev behind a linked call on ONE context (the library's ring) returns what it returns alone on a context with that history"""
    import torch

    linked = _run(rsdsfm, torch, clip, 2, 0, False, linked=True, then_plain=True)
    plain = _run(rsdsfm, torch, clip, 2, 0, False, linked=False, then_plain=True)
    assert linked["records"] == plain["records"] and linked["plain_after"] == plain["plain_after"]


def test_clip_points_in_place_and_out_of_place(rsdsfm, clip):
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    r = np.random.default_rng(4)
    pts = [r.normal(size=(rows, cols, 3)).astype(np.float32) * 3 for _ in range(4)]
    for p in pts:
        p[r.uniform(size=(rows, cols)) < 0.3] = 0.0  # pixels the rectifier skipped
        p[5, 7] = (0.0, -0.0, 0.0)
        p[6, 7] = (0.0, 0.0, 1e-30)  # not a zero point
    got = _run(rsdsfm, torch, clip, 8, 0, False, linked=True, points=pts)
    want = [spec.clip_points(pts[q], got["scales"][q], got["A"][q], got["c"][q]) for q in range(4)]
    for q in range(4):
        assert np.array_equal(got["points"][q].view(np.uint32), want[q].view(np.uint32)), q
        assert not got["points"][q][5, 7].any() and got["points"][q][6, 7].any()
    # the call on its own: out of place (the input stays), then in place
    d_in = [torch.from_numpy(p).to(dev) for p in pts]
    d_out = [torch.full((rows, cols, 3), np.nan, dtype=torch.float32, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a]
    with rsdsfm.Solver(0) as s:
        s.clip_points_dev(ptrs(d_in), ptrs(d_out), rows, cols, got["scales"], got["A"], got["c"])
        s.synchronize()
        for q in range(4):
            assert np.array_equal(d_out[q].cpu().numpy().view(np.uint32), want[q].view(np.uint32)), q
            assert np.array_equal(d_in[q].cpu().numpy().view(np.uint32), pts[q].view(np.uint32)), q
        s.clip_points_dev(ptrs(d_in), ptrs(d_in), rows, cols, got["scales"], got["A"], got["c"])
        s.synchronize()
        for q in range(4):
            assert np.array_equal(d_in[q].cpu().numpy().view(np.uint32), want[q].view(np.uint32)), q
        with pytest.raises(rsdsfm.RsdsfmError):  # two pairs share an output
            s.clip_points_dev(ptrs(d_in), [d_out[0].data_ptr()] * 4, rows, cols, got["scales"], got["A"], got["c"])


def test_the_field_buffers_are_required(rsdsfm, clip):
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    dms, _, _ = _buffers(torch, dev, 4, rows, cols)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        with pytest.raises(rsdsfm.RsdsfmError, match="d_flows is required"):
            s.solve_video_linked_dev([f.data_ptr() for f in d_frames], rows, cols, 3, K, gamma, [m.data_ptr() for m in dms], None, trials=TRIALS)


def test_scale_accuracy_through_the_gpu_solve(rsdsfm):
    """tests/test_link_cpu.py's accuracy case (three pairs whose translations are 1, 1.5 and 1 times the default motion's, 96 x 128, 0.05 px noise,
    10 % outliers) with the pairs solved by rsdsfm_solve_frame_dev and linked by rsdsfm_link_pairs_dev, under the bound recorded from the CPU:
    relative errors 0.030781 and 0.004472 there, bound 0.046173 (the larger error plus half of it)."""
    import torch

    sc = cases.accuracy_scene(rsdsfm.synth)
    rows, cols, K, gamma = cases.ACC_ROWS, cases.ACC_COLS, sc["K"], sc["gamma"]
    dev = torch.device("cuda", 0)
    d_f = [torch.from_numpy(f).to(dev) for f in sc["fields"]]
    dms, _, _ = _buffers(torch, dev, 3, rows, cols)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        res = []
        for q in range(3):
            res.append(s.solve_frame_dev(d_f[q].data_ptr(), rows, cols, K, gamma, dms[q].data_ptr(), trials=cases.ACC_TRIALS, tol=cases.ACC_TOL,
                                         seed=cases.ACC_SOLVE_SEED, flow_index_mode=rsdsfm.FLOW_GATHERED))
            s.synchronize()
        links = s.link_pairs_dev([f.data_ptr() for f in d_f], [m.data_ptr() for m in dms], [r["v"] for r in res], [r["w"] for r in res], [r["k"] for r in res],
                                 rows, cols, K, gamma)
    ch = rsdsfm.chain_clip(links, [r["v"] for r in res], [r["w"] for r in res], gamma)
    errs = cases.speed_ratio_errors(ch["scales"], [r["v"] for r in res])
    print("links", [(r["n"], r["agree"]) for r in links], "scales", ch["scales"], "relative errors %.6f %.6f" % tuple(errs))
    assert all(r["valid"] for r in links) and not ch["broken"].any()
    assert max(errs) <= cases.ACC_BOUND


def test_evaluate_real_sequence_with_trajectory(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., trajectory=True): the pairs it returned before, the links of Solver.link_pairs on their fields, maps and
    motions, chain_clip's scales and poses, the spec's points, and one PLY with the points of every pixel that carries a depth"""
    frames, rows, cols, K, gamma, seeds = clip
    with rsdsfm.Solver(0) as s:
        out = rsdsfm.evaluate.evaluate_real_sequence(s, frames, camera=K, gamma=gamma, out_dir=str(tmp_path), trials=TRIALS, seeds=seeds, trajectory=True)
        pairs = out["pairs"]
        again = s.link_pairs([p["flow"] for p in pairs], [p["depth_map"] for p in pairs], [p["v"] for p in pairs], [p["w"] for p in pairs], [p["k"] for p in pairs], K, gamma)
    assert len(pairs) == 4 and len(out["links"]) == 3
    _same_links(out["links"], again)
    ch = rsdsfm.chain_clip(out["links"], [p["v"] for p in pairs], [p["w"] for p in pairs], gamma)
    for name in ("scales", "A", "c", "broken"):
        assert np.array_equal(np.asarray(out[name]), np.asarray(ch[name])), name
    for q in range(4):
        want = spec.clip_points(pairs[q]["coords"], out["scales"][q], out["A"][q], out["c"][q])
        assert np.array_equal(out["points"][q].view(np.uint32), want.view(np.uint32)), q
    coords, colours = rsdsfm.formats.read_ply(str(tmp_path / "clip.ply"))
    keep = [p["depth_map"] > 0 for p in pairs]
    assert len(coords) == sum(int(k_.sum()) for k_ in keep) > 0
    assert np.allclose(coords[: int(keep[0].sum())], out["points"][0][keep[0]], rtol=1e-6, atol=1e-30)
    assert np.array_equal(colours[: int(keep[0].sum())], frames[0][keep[0]])
    lines = (tmp_path / "trajectory.csv").read_text().strip().split("\n")
    assert len(lines) == 1 + 5 and lines[0].startswith("frame,c_x") and lines[1].startswith("0,0,0,0,1,0,0,0,1,0,0,0,1,1")

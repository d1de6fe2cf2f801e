"""evaluateSingleRun for a synthetic example archive (reference main.cc:364-560) on the HIP path: ground-truth flow ->
flatten + alpha -> ransac -> nonLinearRefinement -> sign fix + depth map + 8-bit depth image -> setRelativePose ->
backProject -> interpolateCrackyImage -> point cloud, images and (synthetic data) error image / mean reprojection error.

Host-side orchestration over the C-ABI wrappers (Solver); file formats in formats.py.  Image decoding / encoding and the
CSV parsing are host work like in the reference; everything per-pixel runs in the HIP kernels.
"""
import contextlib
import os

import numpy as np

from . import formats


def gt_depth_map(world, R_abs, t_abs):
    """RsFrame::getGroundtruthDepthMap (rsframe.cc:416-436): z of the world point in the camera frame of ITS scanline"""
    z = (R_abs[:, 2, :][:, None, :] * world).sum(axis=2) + t_abs[:, 2][:, None]
    return np.where(np.sqrt((world * world).sum(axis=2)) > 0, z, 0.0)


def relocate_pose(R_abs, t_abs):
    """RsFrame::relocatePose (rsframe.cc:951-967): scanline 0 becomes the origin (scanline 0 itself is left untouched)"""
    R, t = np.array(R_abs, dtype=np.float64), np.array(t_abs, dtype=np.float64)
    inv0 = np.linalg.inv(R[0])
    R[1:] = inv0 @ R[1:]
    t[1:] = t[1:] - t[0]
    return R, t


def evaluate_single_run(solver, task_dir, out_dir, trials=50, tol=0.05, seed=1, use_acceleration_mode=False, use_refinement=True,
                        use_global_shutter_mode=False, flow_threshold=1e-10, write_outputs=True, flow_index_mode=0):
    """evaluateSingleRun (main.cc:302-559) on a synthetic example archive.  flow_index_mode 0 (default) = the reference: the
    refinement reads the flow by inlier RANK (main.cc:457, quirk Q2); 1 = each inlier's own pixel."""
    from . import BACKPROJECT_GS, BACKPROJECT_RS, velocity_errors

    a = formats.load_example_archive(task_dir)
    K, truth = a["K"], a["truth"]
    gamma = truth["gamma"]
    f1, f2 = a["frames"]
    rows, cols = f1["rs_image"].shape[:2]
    # main.cc:383 calculateTrueFlow(1, 2)
    flow, _ = solver.true_flow(f1["world"], f2["R"], f2["t"], K, want_best_row=False)
    # main.cc:398-457
    q, u, alpha, alpha_k = solver.flatten(flow, K, gamma, thr=flow_threshold)
    if use_global_shutter_mode:  # main.cc:441-444
        alpha = alpha * 0.0 + 1.0
    rr = solver.ransac(q, u, alpha, alpha_k, use_acceleration_mode, trials, tol, samples=None, seed=seed)
    res = dict(v=rr["v"], w=rr["w"], k=rr["k"], inliers=rr["inliers"])
    if use_refinement:
        ref = solver.non_linear_refinement(u, rr["inliers"], rr["alpha"], rr["alpha_k"], rr["v"], rr["w"], rr["k"], use_acceleration_mode,
                                           flow_index_mode=flow_index_mode, inlier_idx=rr["inlier_idx"] if flow_index_mode else None)
        res = dict(v=ref["v"], w=ref["w"], k=ref["k"], inliers=ref["inliers"], refine_summary=ref["summary"])
    # main.cc:466-509
    dm = solver.depth_map(res["inliers"], res["v"], K, rows, cols)
    depth_est = solver.depth_preview(dm["inliers"], K, rows, cols)
    # main.cc:515-523
    R_rel, t_rel = solver.pose_table(dm["v"], res["w"], res["k"], gamma, rows)
    gs, coords = solver.back_project(f1["rs_image"], dm["depth_map"], R_rel, t_rel, K, mode=BACKPROJECT_GS if use_global_shutter_mode else BACKPROJECT_RS)
    backprojection = solver.interpolate_cracky(gs, 1)
    # synthetic data only (main.cc:533-556): error image + mean reprojection error against the archive's ground truth
    gt_depth = gt_depth_map(f1["world"], f1["R"], f1["t"])
    R_abs, t_abs = relocate_pose(f1["R"], f1["t"])
    stats, error_image = solver.reprojection_error(coords, gt_depth, dm["depth_map"], R_abs, t_abs, K, max_norm=10.0)
    w_err, v_err = velocity_errors(res["w"], dm["v"], truth["w"], truth["v"])
    out = dict(n=len(q), num_inliers=rr["num_inliers"], v=dm["v"], w=res["w"], k=res["k"], flipped=dm["flipped"], w_error=w_err, v_error=v_err,
               mean_reprojection_error=stats["mean_error"], reprojection=stats, flow=flow, depth_map=dm["depth_map"], depth_est=depth_est,
               gs_image=gs, backprojection=backprojection, coords=coords, error_image=error_image, truth=truth)
    if write_outputs:
        os.makedirs(out_dir, exist_ok=True)
        formats.write_png(out_dir + "/MinimalDepth.png", depth_est)
        formats.write_png(out_dir + "/rs_image.png", f1["rs_image"])
        formats.write_png(out_dir + "/backprojection.png", backprojection)
        formats.write_png(out_dir + "/error_image.png", error_image)
        formats.write_png(out_dir + "/optical_flow.png", formats.flow_to_bgr(flow))  # main.cc:390-392
        if f1.get("gs_image") is not None:  # main.cc:535-554: comparisons against the archive's global-shutter image
            original_gs, original_rs = f1["gs_image"], f1["rs_image"]
            difference = formats.abs_diff(backprojection, original_gs)
            formats.write_png(out_dir + "/gs_image.png", original_gs)
            formats.write_png(out_dir + "/difference.png", difference)
            formats.write_png(out_dir + "/remainder.png", formats.abs_diff(original_gs, difference))
            base = formats.shift_channel_bgr(original_gs, 1, 1, 1)
            formats.write_png(out_dir + "/overlay_gs_rs.png", formats.create_overlay_image(
                base, formats.shift_channel_bgr(formats.abs_diff(original_rs, original_gs), 2, 0.5, 0.5)))
            formats.write_png(out_dir + "/overlay_gs_bp.png", formats.create_overlay_image(base, formats.shift_channel_bgr(difference, 2, 0.5, 0.5)))
        formats.write_ply(out_dir + "/point_cloud.ply", coords, f1["rs_image"])
        formats.write_sweep_results(out_dir, [os.path.basename(task_dir.rstrip("/"))], [[w_err]], [[v_err]], [[stats["mean_error"]]],
                                    w=[res["w"]], v=[dm["v"]], k=[[res["k"]]])
    return out


def evaluate_real_run(solver, data_prefix, flow=None, camera="galaxy", gamma=0.95, out_dir=None, trials=5, tol=0.05, seed=1,
                      use_acceleration_mode=False, use_refinement=True, use_global_shutter_mode=False, flow_threshold=1e-10,
                      flow_index_mode=0, device=0, frame2=None, flow_params=None, dense=False, check_flow=False):
    """The real-world branch of evaluateSingleRun (main.cc:341-361, 364-531; setupCameraReal main.cc:675-690): <data_prefix>frame1.png,
    one of the hard-coded phone calibrations (or a (f_x, f_y, c_x, c_y) tuple), gamma 0.95 -- and the optical flow from frame 1 to
    frame 2: passed in (an array, a .npy or a Middlebury .flo file, formats.load_flow), or, with flow=None, computed on the device
    by the DeepFlow front end (Solver.deep_flow_dev; camera.cc:253-277, main.cc:380-384) from <data_prefix>frame2.png or the
    `frame2` array (flow_params: its parameters, None = OpenCV's defaults); that flow goes into the solve without leaving the device
    and is returned as out["flow"].  Runs the whole solve in ONE device-resident call, then the consumers (8-bit depth image, back
    projection, crack interpolation, point cloud) and writes what the reference writes (optical_flow.png too when the flow was
    computed here, main.cc:386-392).  Defaults as in main.cc:304-311 (5 trials, tolerance 0.05, refinement on).  A 2-D (gray) frame 1 goes
    through the one-channel rectifier (Solver.rectify_gray_frame_dev): gs_image / backprojection come back (rows, cols), equal to channel 0
    of the run on the replicated BGR frame, and the point cloud takes the replicated gray as its colour.  dense=True additionally
    returns the hole-free global-shutter frame and its mask (Solver.rectify_dense_frame_dev: out["dense_image"], out["dense_mask"]) and, with
    out_dir, writes rectified_dense.png and rectified_dense_mask.png (mask x 255); the default returns and writes exactly what it did.
    check_flow=True (only with a flow computed here: ValueError with a passed-in flow) puts the forward-backward check between the flow and
    the solve (Solver.deep_flow_checked_dev, include/rsdsfm_flow_check.h): the solve sees the MASKED field, which is also out["flow"];
    out["flow_mask"] is the mask (rows, cols) uint8, out["flow_consistent"] its count, and with out_dir flow_mask.png (mask x 255) is written."""
    import torch

    from . import BACKPROJECT_GS, BACKPROJECT_RS

    if check_flow and flow is not None:
        raise ValueError("check_flow=True needs the flow to be computed here (flow=None): the check reads the backward field too")
    image = formats.read_png(data_prefix + "frame1.png") if isinstance(data_prefix, str) else np.ascontiguousarray(data_prefix, dtype=np.uint8)
    K = formats.CAMERA_INTRINSICS[camera] if isinstance(camera, str) else tuple(float(x) for x in camera)
    rows, cols = image.shape[:2]
    image2 = None
    if flow is None:
        if frame2 is None:
            if not isinstance(data_prefix, str):
                raise ValueError("flow=None needs frame 2: a data prefix with frame2.png or the frame2 array")
            frame2 = formats.read_png(data_prefix + "frame2.png")
        image2 = np.ascontiguousarray(frame2, dtype=np.uint8)
        if image2.shape != image.shape:
            raise ValueError("frame2 is %s, frame1 is %s" % (image2.shape, image.shape))
    else:
        flow = formats.load_flow(flow)
        if flow.shape[:2] != (rows, cols):
            raise ValueError("flow is %dx%d, frame1 is %dx%d" % (flow.shape[0], flow.shape[1], rows, cols))
    dev = torch.device("cuda", device)
    mode = BACKPROJECT_GS if use_global_shutter_mode else BACKPROJECT_RS
    with torch.cuda.device(dev):  # everything stays on the device until the products are copied out
        d_img = torch.from_numpy(image).to(dev)
        if image2 is None:
            d_flow = torch.from_numpy(flow).to(dev)
        else:
            d_img2 = torch.from_numpy(image2).to(dev)
            d_flow = torch.empty((rows, cols, 2), dtype=torch.float64, device=dev)
        d_map = torch.empty(rows * cols, dtype=torch.float64, device=dev)
        d_R = torch.empty(rows * 9, dtype=torch.float64, device=dev)
        d_t = torch.empty(rows * 3, dtype=torch.float64, device=dev)
        d_depth_est = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
        d_gs, d_back = torch.empty_like(d_img), torch.empty_like(d_img)
        d_coords = torch.empty((rows, cols, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if check_flow:  # both fields and the check on the solver's stream, ahead of the solve that reads the masked field
            d_fmask, d_fcount = torch.empty((rows, cols), dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            solver.deep_flow_checked_dev(d_img.data_ptr(), d_img2.data_ptr(), rows, cols, 1 if image.ndim == 2 else image.shape[2], d_flow.data_ptr(),
                                         d_fmask.data_ptr(), d_count=d_fcount.data_ptr(), params=flow_params)
        elif image2 is not None:  # the flow is computed on the solver's stream, ahead of the solve that reads it
            solver.deep_flow_dev(d_img.data_ptr(), d_img2.data_ptr(), rows, cols, 1 if image.ndim == 2 else image.shape[2], d_flow.data_ptr(),
                                 params=flow_params)
        r = solver.solve_frame_dev(d_flow.data_ptr(), rows, cols, K, gamma, d_map.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), trials=trials, tol=tol,
                                   seed=seed, use_acceleration_mode=use_acceleration_mode, use_refinement=use_refinement,
                                   flow_threshold=flow_threshold, flow_index_mode=flow_index_mode, use_global_shutter_mode=use_global_shutter_mode)
        m = r["num_inliers"]
        # main.cc:480-523 -- 8-bit depth image, back projection, crack interpolation -- in ONE call of two launches
        rectify = solver.rectify_gray_frame_dev if image.ndim == 2 else solver.rectify_frame_dev
        rectify(r["d_inliers"], m, d_img.data_ptr(), d_map.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, d_depth_est.data_ptr(),
                d_gs.data_ptr(), d_back.data_ptr(), d_coords=d_coords.data_ptr(), mode=mode, offset=1)
        if dense:
            d_dense, d_dmask = torch.empty_like(d_img), torch.empty((rows, cols), dtype=torch.uint8, device=dev)
            solver.rectify_dense_frame_dev(d_img.data_ptr(), 1 if image.ndim == 2 else image.shape[2], d_map.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K,
                                           rows, cols, d_dense.data_ptr(), d_dmask.data_ptr(), mode=mode)
        solver.synchronize()
        depth_map = d_map.cpu().numpy().reshape(cols, rows).T.copy()  # the device map is column-major (Eigen MatrixXd)
        R_rel, t_rel = d_R.cpu().numpy().reshape(rows, 3, 3), d_t.cpu().numpy().reshape(rows, 3)
        depth_est, gs, backprojection, coords = d_depth_est.cpu().numpy(), d_gs.cpu().numpy(), d_back.cpu().numpy(), d_coords.cpu().numpy()
        if image2 is not None:
            flow = d_flow.cpu().numpy()
    out = dict(n=r["n"], num_inliers=m, v=r["v"], w=r["w"], k=r["k"], flipped=r["flipped"], refine_summary=r["refine_summary"],
               depth_map=depth_map, depth_est=depth_est, gs_image=gs, backprojection=backprojection, coords=coords, R=R_rel, t=t_rel)
    if image2 is not None:
        out["flow"] = flow
    if dense:
        out["dense_image"], out["dense_mask"] = d_dense.cpu().numpy(), d_dmask.cpu().numpy()
    if check_flow:
        out["flow_mask"], out["flow_consistent"] = d_fmask.cpu().numpy(), int(d_fcount.cpu()[0])
    if out_dir:
        _write_real_outputs(out_dir, image, flow if image2 is not None else None, depth_est, backprojection, coords)
        if dense:
            _write_dense_outputs(out_dir, out["dense_image"], out["dense_mask"])
        if check_flow:
            formats.write_png(out_dir + "/flow_mask.png", (out["flow_mask"] * 255).astype(np.uint8))
    return out


def _write_dense_outputs(out_dir, dense_image, dense_mask):
    """the dense rectifier's two files beside _write_real_outputs'"""
    formats.write_png(out_dir + "/rectified_dense.png", dense_image)
    formats.write_png(out_dir + "/rectified_dense_mask.png", (dense_mask * 255).astype(np.uint8))


def _write_real_outputs(out_dir, image, flow, depth_est, backprojection, coords):
    """what the real-world branch writes (main.cc:386-392 and :480-523); optical_flow.png only for a flow computed here"""
    os.makedirs(out_dir, exist_ok=True)
    if flow is not None:
        formats.write_png(out_dir + "/optical_flow.png", formats.flow_to_bgr(flow))  # main.cc:386-392
    formats.write_png(out_dir + "/MinimalDepth.png", depth_est)
    formats.write_png(out_dir + "/rs_image.png", image)
    formats.write_png(out_dir + "/backprojection.png", backprojection)
    formats.write_ply(out_dir + "/point_cloud.ply", coords, image if image.ndim == 3 else np.repeat(image[:, :, None], 3, axis=2))


@contextlib.contextmanager
def _plate_estimator_for(solver, estimator):
    """evaluate_real_sequence's plate_estimator keyword: the solver's knob (Solver.set_plate_estimator) at `estimator` inside the block and back
    where it was behind it, whatever happens inside; None: the knob stays where the caller left it"""
    if estimator is None:
        yield
        return
    before = solver.plate_estimator
    solver.set_plate_estimator(estimator)
    try:
        yield
    finally:
        solver.set_plate_estimator(before)


def evaluate_real_sequence(solver, frames, camera="galaxy", gamma=0.95, out_dir=None, trials=5, seeds=None, tol=0.05, use_acceleration_mode=False,
                           use_refinement=True, use_global_shutter_mode=False, flow_threshold=1e-10, flow_index_mode=0, device=0, flow_params=None, dense=False,
                           check_flow=False, trajectory=False, link_tol=None, min_links=None, fuse=False, fuse_tol=None, stabilize=False, smooth_sigma=None,
                           smooth_translation=True, fill=0, crop=False, crop_margin=None, crop_max_empty=0, blend=False, blend_feather=None,
                           blend_gain=True, inpaint=False, last_frame=False, occlusion=False, occlusion_tol=None, occlusion_search=False, retime=None,
                           shutter=None, denoise=None, superres=None, plate=None, erase=None, plate_estimator=None, deblur=None, sharpen=None):
    """evaluate_real_run's real-world branch (main.cc:341-361, 364-531) for a clip: `frames` is <prefix>frame1.png ... frameN.png (the
    prefix, or a list of paths), or the frames themselves (an (N, rows, cols[, 3]) uint8 array or a list of arrays; 2-D frames are gray).
    By default ONE call does the clip (Solver.rectify_video_dev): the batched DeepFlow of every consecutive pair, the pipelined solve of every pair p
    (frames p, p + 1; seed seeds[p], default 1 as in evaluate_real_run) and, behind it on the pair's lane, the rectification of frame p.
    Returns one dict per pair with evaluate_real_run's keys and "flow"; each is bit for bit evaluate_real_run(frames[p], None,
    frame2=frames[p + 1]).  With out_dir: evaluate_real_run's files (optical_flow.png included) under out_dir/<pair>/, and
    out_dir/poses.csv (pair, v, w, k, inliers).  dense=True: per pair also evaluate_real_run's dense_image / dense_mask (behind the clip call,
    from the pair's depth map and pose table) and its two files rectified_dense.png / rectified_dense_mask.png; the default writes exactly
    what it did.  check_flow=True: every pair goes through evaluate_real_run's checked chain instead (Solver.deep_flow_checked_dev, the solve on
    the masked field, the rectifier; pair after pair on the solver's stream, one wait at the end) -- per pair evaluate_real_run(...,
    check_flow=True) bit for bit, with its flow_mask / flow_consistent and flow_mask.png.
    trajectory=True: behind the clip, the links between consecutive pairs (Solver.link_pairs_dev on the pairs' fields, depth maps and motions), the
    chain (chain_clip) and the clip's points (Solver.clip_points_dev on the pairs' world points); the return value is then
    dict(pairs: the list above, links, scales, A, c, broken, points: per pair (rows, cols, 3) float32 in frame 0's coordinates and unit), and
    out_dir receives trajectory.csv (frame, position, rotation row by row, the scale of the pair that starts there) and clip.ply: the points
    of every pair's pixels that carry a depth, with frame p's colours, written by formats.write_ply.
    fuse=True (needs trajectory=True: ValueError otherwise): behind the links, the fusion of the pairs' depth maps (Solver.fuse_depths_dev:
    every pair's holes filled from what its neighbours measured there); each pair's dict gets fused_depth ((rows, cols) float64, 0 = no value),
    fuse_flags ((rows, cols) uint8: FUSE_OWN ...) and fuse_record; with dense=True the dense rectifier reads the FUSED map; out_dir receives
    depth_fused.png per pair (Solver.depth_preview's 8-bit depth image of the fused map) and fusion.csv (pair and the six counts).  The clip's
    points and clip.ply keep selecting by the solve's map.  The default writes exactly what it did.
    stabilize=True (implies trajectory=True): behind the chain (and the fusion), the smoothed camera path (smooth_path with smooth_sigma frames,
    None = the default; smooth_translation=False smooths the rotation only), every pair's virtual pose (virtual_poses) and frame p rendered from
    its virtual camera (Solver.stabilize_frame_dev on the pair's map -- the FUSED one with fuse=True -- and pose table).  The returned dict then
    also has stabilized and stab_masks (per pair, the frame's shape / (rows, cols) uint8), stab_valid (per pair, the mask's count) and
    path_smoothed = dict(A_s, c_s, M, m); out_dir receives stabilized_<p>.png per pair and path_smoothed.csv (frame, smoothed position, smoothed
    rotation row by row).  The last frame has no pair and is not rendered unless last_frame=True.  With stabilize=False every output is unchanged.
    fill=K (needs stabilize=True: ValueError otherwise; K = 1 .. 16 neighbours on each side): behind the stabilised frames, the band each leaves
    empty filled from its neighbours (neighbour_poses, then one Solver.stabilize_fill_frame_dev per candidate on COPIES of the frame and its
    mask, on the neighbour's map -- the FUSED one with fuse=True).  The returned dict then also has stab_filled (per pair, the frame's shape),
    stab_sources (per pair, (rows, cols) uint8: 0 nobody, 1 the own frame, 2 |j| / 2 |j| + 1 the frame j before / after) and fill_counts
    ((pairs, 2 + 2 K) int64: [none, own, -1, +1, -2, +2, ...]); out_dir receives stabilized_filled_<p>.png per pair and fill.csv (pair and the
    counts).  Without fill every output is what it was.
    crop=True (needs stabilize=True: ValueError otherwise; with or without fill=K): ONE window for the clip (Solver.crop_window_dev with
    crop_margin -- None: the default, 1 -- and crop_max_empty on the filled masks, or the stabilised ones without fill) and every frame rendered
    through it at full size (Solver.stabilize_window_frame_dev: the own frame onto zeroed planes, then the K neighbours on each side).  The
    returned dict then also has stab_cropped (per pair, the frame's shape), crop_window ((r0, c0, h, w); all 0: nothing fits, the frames are
    then black) and crop_counts ((pairs, 2 + 2 K) int64, fill_counts' layout); out_dir receives stabilized_cropped_<p>.png per pair and crop.csv
    (the window, then pair and the counts).  Without crop every output is what it was.
    blend=True (needs stabilize=True and fill >= 1: ValueError otherwise): every frame once more through the crop's window (crop=True) or the
    full frame, with its seams blended (tests/stabilize_blend_spec_numpy.py): the own frame onto zeroed planes, Solver.seam_distance_dev of its
    mask with blend_feather pixels (None: the default, 16), then every neighbour rendered alone onto a layer and Solver.seam_blend_layer_dev
    (a gain per channel from the overlap unless blend_gain=False, the layer copied where nobody is and mixed over the feather).  The returned
    dict then also has stab_blended (per pair, the frame's shape), blend_gains ((pairs, 2 K, 3) uint32 in 1 / 65536, per offset -1, +1, -2,
    +2, ...; 65536 for a skipped offset or an unused channel) and blend_counts ((pairs, 2 + 4 K) int64: [none, own_untouched, (filled,
    blended) per offset]); out_dir receives stabilized_blended_<p>.png per pair and blend.csv (pair, the counts, the gains).  Without blend
    every output is what it was.
    inpaint=True (needs stabilize=True: ValueError otherwise): the pixels the last stage produced -- blended, else cropped, else filled, else
    stabilised -- leaves empty, invented from what surrounds them (Solver.inpaint_frame_dev on a COPY of the stage's frames, with its masks;
    tests/stabilize_inpaint_spec_numpy.py).  The returned dict then also has stab_inpainted (per pair, the frame's shape), inpaint_sources (per
    pair, (rows, cols) uint8: INPAINT_SOURCE = 255 where a pixel was invented, elsewhere the stage's source plane -- the blend's and the fill's
    -- or its mask) and inpaint_counts ((pairs,) int64); out_dir receives stabilized_inpainted_<p>.png per pair and inpaint.csv (pair, stage,
    the count).  Without inpaint every output is what it was.
    last_frame=True (needs stabilize=True: ValueError otherwise): the clip's last frame is rendered too, from the last pair's depth map moved onto
    it and that pair's motion (Solver.last_frame_dev; the fused map by Solver.advance_depth_dev with fuse=True; the last pair's scale): every
    stage above then has one more frame -- one more entry in its lists and arrays, the N-th stabilized*_<p>.png and one more row in fill.csv,
    crop.csv, blend.csv and inpaint.csv -- and the last frame is a candidate for the frames before it.  The solve's outputs, the trajectory and
    path_smoothed's A_s and c_s are unchanged (M and m gain the last frame's entry).  Without last_frame every output is what it was.
    occlusion=True (needs stabilize=True and fill >= 1: ValueError otherwise): every NEIGHBOUR candidate of the fill, the crop and the blend is
    rendered by Solver.stabilize_visible_frame_dev (tests/stabilize_visible_spec_numpy.py; the fill through the full-frame window): a pixel whose
    source is not the nearest surface that lands there -- a fold of the neighbour's map, a parallax ghost -- is rejected and left to the next
    candidate or the inpainter.  occlusion_tol: the test's tolerance as a fraction of the depth in (0, 1] (None: the default, about 0.05).  The
    outputs keep their keys, shapes and files; a rejected pixel shows up under a later offset or under none.  Without occlusion every output
    is what it was.
    occlusion_search=True (needs occlusion=True: ValueError otherwise): those candidates are rendered by Solver.stabilize_search_frame_dev instead
    (tests/stabilize_search_spec_numpy.py): a pixel the test rejects is looked for again from the source pixel that landed nearest the camera on
    its cell and, where that ends on the visible surface, recovered; it counts under its offset.  The returned dict then also has fill_recovered
    and, with crop=True, crop_recovered ((frames,) int64: the recovered pixels per frame, summed over its candidates, from the calls' own
    counters); out_dir receives occlusion_search.csv (frame and the sums).  Without occlusion_search every output is what it was.
    retime=factor or a list of times (needs stabilize=True: ValueError otherwise): behind everything else, the solved clip rendered once more at
    the instants retime_times(frames with a depth map, factor), or at the given times, along the SMOOTHED path (Solver.retime_video_dev,
    tests/retime_spec_numpy.py; the fused maps with fuse=True, the layers through the occlusion test with occlusion=True): the returned dict
    also has retimed, retime_masks, retime_sources (lists of frames), retime_counts ((times, 5) int64: [none, a only, b only, dissolved,
    conflict]) and retime_times; out_dir receives retimed_<i>.png and retime.csv.  Without the keyword every key and file is what it was.
    shutter=width or (width, samples) (needs retime: ValueError otherwise): behind the retimed frames, the same instants once more EXPOSED over a
    window of `width` input-frame intervals (shutter_from_angle turns a shutter angle into one), the mean of `samples` (default 8) sub-instant
    renders each (Solver.shutter_video_dev, tests/shutter_spec_numpy.py; the retimed frames' maps, path and occlusion settings): the returned dict
    also has shuttered, shutter_masks, shutter_coverage (lists of frames; the coverage is the number of sub-instants that saw the pixel),
    shutter_counts ((times, 3) int64: [unset, partial, full]) and shutter_kept ((times,) int32: the sub-instants inside the clip); out_dir
    receives shuttered_<i>.png and shutter.csv.  The retimed keys and files stay as they are; without the keyword every key and file is what it was.
    denoise=K or (K, strength) (needs stabilize=True: ValueError otherwise): behind everything else, every stabilised frame once more as the
    patch-weighted mean of itself and its K neighbours on either side (1 .. 7), each rendered alone into the frame's camera on the SMOOTHED path
    (Solver.denoise_video_dev, tests/denoise_spec_numpy.py; strength None: the default, 12; the fused maps with fuse=True, the neighbours through
    the occlusion test with occlusion=True): the returned dict also has stab_denoised, denoise_masks, denoise_weights (lists of frames; the weight
    is 16 for the own frame plus up to 16 per neighbour) and denoise_counts ((frames, 3) int64: [unset, own only, averaged]); out_dir receives
    stabilized_denoised_<p>.png and denoise.csv.  Without the keyword every key and file is what it was.
    denoise=(K, strength, spatial) with spatial True or (target, search): the spatial top-up behind the temporal stage of every frame
    (Solver.denoise_spatial_video_dev, tests/denoise_spatial_spec_numpy.py; the strength is both stages', True: target 80, search 2): stab_denoised is
    then the topped-up clip, the returned dict also has denoise_support (a list of planes) and denoise_spatial_counts ((frames, 3) int64:
    [unset, kept, smoothed]), and denoise.csv three more columns (kept, smoothed, mean_support).  Without the third element every key, file and
    byte is what it was.
    denoise=(K, "auto") or (K, "auto", spatial): the strength of both stages from every frame's own noise, measured on the device behind the
    frame's own render (Solver.denoise_auto_video_dev, tests/noise_spec_numpy.py): the returned dict also has denoise_noise ((frames, 4) int64:
    [n, m, sigma_q8, h]) and denoise.csv three more columns (noise_m, sigma, strength).  With an integer or None strength every key, file and
    byte is what it was.
    denoise=(K, "curve") or (K, "curve", spatial): the strength of both stages PER PIXEL from every frame's own noise curve, measured per
    brightness band on the device behind the frame's own render (rsdsfm_noise_curve.denoise_curve_video_dev, tests/noise_curve_spec_numpy.py): the
    returned dict also has denoise_curve ((frames, 9, 4) int64: [n, m, sigma_q8, 0] of the eight bands, then of all samples), and
    denoise.csv eleven more columns (noise_m0 .. noise_m7, noise_m, and strength_min, strength_max: the ends of the frame's strength table).
    denoise=(K, "temporal") or (K, "temporal", spatial): as "curve", with the curve measured from the differences to the frame's registered
    neighbours in place of the frame's own render, so that a textured frame is not taken for a noisy one
    (rsdsfm_noise_temporal.denoise_temporal_video_dev, tests/noise_temporal_spec_numpy.py): the same keys and the same columns.  Any other
    string is a ValueError.
    superres=scale or (scale, K) (needs stabilize=True: ValueError otherwise): behind everything else, every stabilised frame once more on a grid
    `scale` times finer (1 .. 4), merged from itself and its K neighbours on either side (1 .. 7, default 2), each rendered alone into the frame's
    camera on the SMOOTHED path (Solver.superres_video_dev, tests/superres_spec_numpy.py; the fused maps with fuse=True): the returned dict also
    has superres, superres_masks (lists of scale rows x scale cols frames) and superres_counts ((frames, 3) int64: [unset, own only, merged]);
    out_dir receives superres_<p>.png and superres.csv.  Without the keyword every key and file is what it was.
    plate=K or (K, threshold) (needs stabilize=True: ValueError otherwise): behind everything else, every stabilised frame once more as its clean
    plate -- the per-pixel, per-channel median of the frame and its up to K neighbours on each side, each rendered alone into the frame's camera on
    the SMOOTHED path -- and where the frame differs from it (Solver.plate_video_dev, tests/plate_spec_numpy.py; threshold None: the default, 24;
    the fused maps with fuse=True, the neighbours through the occlusion test with occlusion=True): the returned dict also has plate,
    plate_moving (lists of frames; the flag is 0 unset, 1 static, 2 moving, 3 undecided) and plate_counts ((frames, 4) int64: [unset, static,
    moving, undecided]); out_dir receives plate_<p>.png, moving_<p>.png (255 where the flag is 2) and plate.csv.  Without the keyword every key
    and file is what it was.
    erase=True, K or (K, open, grow, feather) (needs stabilize=True: ValueError otherwise): behind everything else, every stabilised frame once
    more WITHOUT what moved through it -- the plate of the frame and its up to K neighbours on each side (True: the default, 2) under the cleaned,
    grown and feathered matte of the plate's flag, the frame's own bytes everywhere else (Solver.erase_video_dev, tests/erase_spec_numpy.py; open,
    grow, feather literal, default 2, 2, 4; the fused maps with fuse=True, the neighbours through the occlusion test with occlusion=True): the
    returned dict also has erased, erase_matte (lists of frames; the matte is 0 .. feather) and erase_counts ((frames, 5) int64: [unset, kept,
    replaced, feathered, unresolved]); out_dir receives erased_<p>.png, matte_<p>.png (the matte scaled to 0 .. 255) and erase.csv.  Without the
    keyword every key and file is what it was.
    plate_estimator="median" or "medoid" (needs plate= or erase=: ValueError otherwise): the solver's knob (Solver.set_plate_estimator) is set to
    it around the plate= and erase= stages and put back afterwards -- "medoid": every plate pixel is a whole candidate, the L1 medoid
    (tests/plate_medoid_spec_numpy.py), not a per-channel median.  The keys and files are plate='s and erase='s.  None: the knob stays where the
    caller left it, and every key and file is what it was.
    deblur=True, K or (K, strength) (needs stabilize=True: ValueError otherwise): behind everything else, every stabilised frame once more with the
    pixels of its sharper neighbours -- the frame and its up to K neighbours on each side (1 .. 3; True: the default, 2), each rendered alone into
    the frame's camera on the SMOOTHED path, a neighbour counting by how much sharper than the frame it is on their overlap
    (Solver.deblur_video_dev, tests/deblur_spec_numpy.py; strength None: the default, 24; the fused maps with fuse=True, the neighbours through
    the occlusion test with occlusion=True): the returned dict also has deblurred (a list of frames), deblur_counts ((frames, 3) int64: [unset,
    own only, transferred]) and deblur_taus ((frames, 6) int32: the factor 0 .. 32 of every listed neighbour, -1 behind them); out_dir receives
    deblurred_<p>.png and deblur.csv.  deblur=(K, strength, band_rows): a factor per band of band_rows rows (a multiple of 16) and not per frame,
    for frames whose blur varies down the rows (tests/deblur_bands_spec_numpy.py); deblur_taus is then the largest of a neighbour's band factors,
    the dict also has deblur_band_taus ((frames, 6, NB) int32) and deblur.csv one column per neighbour and band behind the existing ones.  Without
    the third element, and without the keyword, every key and file is what it was.
    sharpen=True, amount_q4 or (amount_q4, coring_q4[, overshoot]) (needs stabilize=True: ValueError otherwise): behind EVERYTHING else, one stream of
    frames once more through the noise-gated unsharp mask (rsdsfm_sharpen.sharpen_video_dev, tests/sharpen_spec_numpy.py: every frame's own noise
    curve measured, the detail cored below the strength it asks for per pixel, the result limited to the local range; True: amount 16, coring 8,
    overshoot 0).  The stream is chosen by fixed priority: the super-resolved frames if superres was given, else the deblurred, else the denoised,
    else the most complete stabilised frames the run produced (inpainted, blended, cropped, filled, stabilized), under that stream's masks.  The
    returned dict also has sharpened (a list of frames), sharpen_counts ((frames, 4) int64: [unset, kept, sharpened, limited]), sharpen_curves
    ((frames, 9, 4) int64) and sharpen_source (the key it read); out_dir receives sharpened_<p>.png and sharpen.csv (pair, the counts, noise_m,
    strength_min, strength_max).  Without the keyword every key, file and byte is what it was."""
    if sharpen is False:
        sharpen = None
    if sharpen is not None and not stabilize:
        raise ValueError("sharpen needs stabilize=True: it sharpens the frames the stages behind the stabiliser produced")
    if sharpen is not None:
        sh_amount, sh_coring, sh_overshoot = (None, None, None) if sharpen is True else (int(sharpen), None, None) if np.ndim(sharpen) == 0 else \
            (int(sharpen[0]), int(sharpen[1]), int(sharpen[2]) if len(sharpen) > 2 else None)
    if plate_estimator is not None and plate_estimator not in ("median", "medoid"):
        raise ValueError("plate_estimator is None, 'median' or 'medoid'")
    if plate_estimator is not None and plate is None and erase in (None, False):
        raise ValueError("plate_estimator needs plate= or erase=: it chooses what their plate is made with")
    if erase is not None and erase is not False and not stabilize:
        raise ValueError("erase needs stabilize=True: it takes the movers out of the frames of the stabilised clip")
    if erase is False:
        erase = None
    if erase is not None:
        er_radius, er_open, er_grow, er_feather = (None, None, None, None) if erase is True else (int(erase), None, None, None) if np.ndim(erase) == 0 else \
            tuple(int(x) for x in erase)
        erase_feather = er_feather or 4  # the matte's largest byte (None or 0: the default), for matte_<p>.png
    if deblur is not None and deblur is not False and not stabilize:
        raise ValueError("deblur needs stabilize=True: it transfers sharpness between the frames of the stabilised clip")
    if deblur is False:
        deblur = None
    if deblur is not None:
        db_radius, db_strength = (None, None) if deblur is True else (int(deblur), None) if np.ndim(deblur) == 0 else (int(deblur[0]), int(deblur[1]))
        db_band_rows = (int(deblur[2]) or None) if deblur is not True and np.ndim(deblur) != 0 and len(deblur) > 2 else None  # 0: off, as without it
    if plate is not None and not stabilize:
        raise ValueError("plate needs stabilize=True: it takes the median of the frames of the stabilised clip")
    if superres is not None and not stabilize:
        raise ValueError("superres needs stabilize=True: it merges the frames of the stabilised clip")
    if denoise is not None and not stabilize:
        raise ValueError("denoise needs stabilize=True: it averages the frames of the stabilised clip")
    if shutter is not None and retime is None:
        raise ValueError("shutter needs retime=factor or times: it exposes the retimed clip's instants")
    if retime is not None and not stabilize:
        raise ValueError("retime needs stabilize=True: it rides the smoothed path of the stabilised clip")
    if occlusion_search and not occlusion:
        raise ValueError("occlusion_search needs occlusion=True: the search runs where the occlusion test rejects")
    if occlusion and not (stabilize and fill >= 1):
        raise ValueError("occlusion needs stabilize=True and fill >= 1: it tests the neighbour candidates of the stabilised frames")
    if last_frame and not stabilize:
        raise ValueError("last_frame needs stabilize=True: it renders the clip's last frame")
    if inpaint and not stabilize:
        raise ValueError("inpaint needs stabilize=True: it inpaints what the stabilised frames leave empty")
    if blend and not (stabilize and fill >= 1):
        raise ValueError("blend needs stabilize=True and fill >= 1: it blends the seams between a stabilised frame and its neighbours")
    if fill and not stabilize:
        raise ValueError("fill needs stabilize=True: it fills the stabilised frames' borders")
    if crop and not stabilize:
        raise ValueError("crop needs stabilize=True: it crops the stabilised frames")
    if stabilize:
        trajectory = True
    if fuse and not trajectory:
        raise ValueError("fuse=True needs trajectory=True: the fusion converts between the pairs' units with the links' ratios")
    import torch

    from . import BACKPROJECT_GS, BACKPROJECT_RS

    if isinstance(frames, str):
        paths, i = [], 1
        while os.path.exists(frames + "frame%d.png" % i):
            paths.append(frames + "frame%d.png" % i)
            i += 1
        frames = paths
    images = [formats.read_png(f) if isinstance(f, str) else np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
    if len(images) < 2 or any(im.shape != images[0].shape for im in images):
        raise ValueError("a clip needs at least two frames of one shape")
    npairs = len(images) - 1
    seeds = [1] * npairs if seeds is None else [int(s) for s in seeds]
    if len(seeds) != npairs:
        raise ValueError("one seed per pair")
    K = formats.CAMERA_INTRINSICS[camera] if isinstance(camera, str) else tuple(float(x) for x in camera)
    rows, cols = images[0].shape[:2]
    channels = 1 if images[0].ndim == 2 else images[0].shape[2]
    dev = torch.device("cuda", device)
    mode = BACKPROJECT_GS if use_global_shutter_mode else BACKPROJECT_RS
    outs = []
    with torch.cuda.device(dev):
        d_imgs = [torch.from_numpy(im).to(dev) for im in images]
        d_flows = [torch.empty((rows, cols, 2), dtype=torch.float64, device=dev) for _ in range(npairs)]
        d_maps = [torch.empty(rows * cols, dtype=torch.float64, device=dev) for _ in range(npairs)]
        d_Rs = [torch.empty(rows * 9, dtype=torch.float64, device=dev) for _ in range(npairs)]
        d_ts = [torch.empty(rows * 3, dtype=torch.float64, device=dev) for _ in range(npairs)]
        d_depth_ests = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(npairs)]
        d_gss = [torch.empty_like(d_imgs[0]) for _ in range(npairs)]
        d_backs = [torch.empty_like(d_imgs[0]) for _ in range(npairs)]
        d_coordss = [torch.empty((rows, cols, 3), dtype=torch.float32, device=dev) for _ in range(npairs)]
        torch.cuda.synchronize()
        ptrs = lambda ts: [t.data_ptr() for t in ts]
        if check_flow:
            d_fmasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(npairs)]
            d_fcounts = torch.empty(npairs, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            rectify = solver.rectify_gray_frame_dev if channels == 1 else solver.rectify_frame_dev
            res = []
            for p in range(npairs):  # (a pair's rectifier is enqueued in front of the next pair's solve, which overwrites the inlier list)
                solver.deep_flow_checked_dev(d_imgs[p].data_ptr(), d_imgs[p + 1].data_ptr(), rows, cols, channels, d_flows[p].data_ptr(),
                                             d_fmasks[p].data_ptr(), d_count=d_fcounts[p:].data_ptr(), params=flow_params)
                r = solver.solve_frame_dev(d_flows[p].data_ptr(), rows, cols, K, gamma, d_maps[p].data_ptr(), d_Rs[p].data_ptr(), d_ts[p].data_ptr(),
                                           trials=trials, tol=tol, seed=seeds[p], use_acceleration_mode=use_acceleration_mode, use_refinement=use_refinement,
                                           flow_threshold=flow_threshold, flow_index_mode=flow_index_mode, use_global_shutter_mode=use_global_shutter_mode)
                rectify(r["d_inliers"], r["num_inliers"], d_imgs[p].data_ptr(), d_maps[p].data_ptr(), d_Rs[p].data_ptr(), d_ts[p].data_ptr(), K, rows, cols,
                        d_depth_ests[p].data_ptr(), d_gss[p].data_ptr(), d_backs[p].data_ptr(), d_coords=d_coordss[p].data_ptr(), mode=mode, offset=1)
                res.append(r)
            solver.synchronize()
        else:
            res = solver.rectify_video_dev(ptrs(d_imgs), rows, cols, channels, K, gamma, ptrs(d_maps), ptrs(d_depth_ests), ptrs(d_gss), ptrs(d_backs),
                                           d_coords=ptrs(d_coordss), seeds=seeds, d_flows=ptrs(d_flows), d_R=ptrs(d_Rs), d_t=ptrs(d_ts), flow_params=flow_params,
                                           mode=mode, offset=1, trials=trials, tol=tol, use_acceleration_mode=use_acceleration_mode,
                                           use_refinement=use_refinement, flow_threshold=flow_threshold, flow_index_mode=flow_index_mode,
                                           use_global_shutter_mode=use_global_shutter_mode)  # (every output is complete when it returns)
        for p, r in enumerate(res):
            outs.append(dict(n=r["n"], num_inliers=r["num_inliers"], v=r["v"], w=r["w"], k=r["k"], flipped=r["flipped"], refine_summary=r["refine_summary"],
                             depth_map=d_maps[p].cpu().numpy().reshape(cols, rows).T.copy(), depth_est=d_depth_ests[p].cpu().numpy(),
                             gs_image=d_gss[p].cpu().numpy(), backprojection=d_backs[p].cpu().numpy(), coords=d_coordss[p].cpu().numpy(),
                             R=d_Rs[p].cpu().numpy().reshape(rows, 3, 3), t=d_ts[p].cpu().numpy().reshape(rows, 3), flow=d_flows[p].cpu().numpy()))
            if check_flow:
                outs[p]["flow_mask"], outs[p]["flow_consistent"] = d_fmasks[p].cpu().numpy(), int(d_fcounts[p].cpu())
        def run_dense(d_depths):  # every pair enqueued behind the clip call, one wait for all of them
            d_denses = [torch.empty_like(d_imgs[0]) for _ in range(npairs)]
            d_dmasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(npairs)]
            torch.cuda.synchronize()
            for p in range(npairs):
                solver.rectify_dense_frame_dev(d_imgs[p].data_ptr(), channels, d_depths[p].data_ptr(), d_Rs[p].data_ptr(), d_ts[p].data_ptr(), K, rows, cols,
                                               d_denses[p].data_ptr(), d_dmasks[p].data_ptr(), mode=mode)
            solver.synchronize()
            for p in range(npairs):
                outs[p]["dense_image"], outs[p]["dense_mask"] = d_denses[p].cpu().numpy(), d_dmasks[p].cpu().numpy()

        if dense and not fuse:
            run_dense(d_maps)
        if trajectory:
            from . import chain_clip

            d_clip = [torch.empty_like(t) for t in d_coordss]
            torch.cuda.synchronize()
            vs, ws, ks = [o["v"] for o in outs], [o["w"] for o in outs], [o["k"] for o in outs]
            links = solver.link_pairs_dev(ptrs(d_flows), ptrs(d_maps), vs, ws, ks, rows, cols, K, gamma, use_global_shutter_mode, tol=link_tol,
                                          min_links=min_links) if npairs >= 2 else []
            traj = chain_clip(links, vs, ws, gamma)
            solver.clip_points_dev(ptrs(d_coordss), ptrs(d_clip), rows, cols, traj["scales"], traj["A"], traj["c"])
            solver.synchronize()
            traj.update(links=links, points=[t.cpu().numpy() for t in d_clip])
            if fuse:
                d_fused = [torch.empty(rows * cols, dtype=torch.float64, device=dev) for _ in range(npairs)]
                d_fflags = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(npairs)]
                torch.cuda.synchronize()
                frecs = solver.fuse_depths_dev(ptrs(d_flows), ptrs(d_maps), vs, ws, ks, rows, cols, K, gamma, links, ptrs(d_fused), use_global_shutter_mode,
                                               ptrs(d_fflags), tol=fuse_tol)
                for p in range(npairs):
                    outs[p]["fused_depth"], outs[p]["fuse_flags"] = d_fused[p].cpu().numpy().reshape(cols, rows).T.copy(), d_fflags[p].cpu().numpy()
                    outs[p]["fuse_record"] = frecs[p]
                if dense:
                    run_dense(d_fused)
            if stabilize:
                from . import smooth_path, virtual_poses
                nst, st_scales = npairs, traj["scales"]  # rendered frames and their units
                if last_frame:  # the last frame: its pair's map moved onto it, its table from its pair's motion, its pair's unit
                    d_maps.append(torch.empty(rows * cols, dtype=torch.float64, device=dev))
                    d_Rs.append(torch.empty(rows * 9, dtype=torch.float64, device=dev))
                    d_ts.append(torch.empty(rows * 3, dtype=torch.float64, device=dev))
                    torch.cuda.synchronize()
                    lo = outs[npairs - 1]
                    solver.last_frame_dev(d_flows[npairs - 1].data_ptr(), d_maps[npairs - 1].data_ptr(), lo["v"], lo["w"], lo["k"], rows, cols, K, gamma,
                                          d_maps[npairs].data_ptr(), d_Rs[npairs].data_ptr(), d_ts[npairs].data_ptr(), use_global_shutter_mode)
                    if fuse:
                        d_fused.append(torch.empty(rows * cols, dtype=torch.float64, device=dev))
                        torch.cuda.synchronize()
                        solver.advance_depth_dev(d_flows[npairs - 1].data_ptr(), d_fused[npairs - 1].data_ptr(), lo["v"], lo["w"], lo["k"], rows, cols, K, gamma,
                                                 d_fused[npairs].data_ptr(), use_global_shutter_mode)
                    nst, st_scales = npairs + 1, np.append(traj["scales"], traj["scales"][npairs - 1])

                A_s, c_s = smooth_path(traj["A"], traj["c"], smooth_sigma, 0, smooth_translation)
                vM, vm = virtual_poses(traj["A"], traj["c"], A_s, c_s, st_scales, smooth_translation, last_frame)
                d_stabs = [torch.empty_like(d_imgs[0]) for _ in range(nst)]
                d_smasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                d_svalid = torch.zeros(nst, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                d_src = d_fused if fuse else d_maps
                for p in range(nst):  # every frame enqueued behind the clip, one wait for all of them
                    solver.stabilize_frame_dev(d_imgs[p].data_ptr(), channels, d_src[p].data_ptr(), d_Rs[p].data_ptr(), d_ts[p].data_ptr(), K, rows, cols, vM[p],
                                               vm[p], d_stabs[p].data_ptr(), d_smasks[p].data_ptr(), d_valid=d_svalid[p:].data_ptr(), mode=mode)
                solver.synchronize()
                traj.update(stabilized=[t.cpu().numpy() for t in d_stabs], stab_masks=[t.cpu().numpy() for t in d_smasks],
                            stab_valid=[int(x) for x in d_svalid.cpu().numpy()], path_smoothed=dict(A_s=A_s, c_s=c_s, M=vM, m=vm))
                if occlusion:
                    from . import _occlusion_tol_q16

                    occ_q16 = 0 if occlusion_tol is None else _occlusion_tol_q16(occlusion_tol)
                    # [taken, rejected] of the call in flight, or with the search [taken, rejected, recovered]
                    d_occ = torch.zeros((nst, 2 + 2 * fill, 3 if occlusion_search else 2), dtype=torch.int64, device=dev)

                def occ_counts():
                    """-> (what every neighbour put into its frame (frames, 2 fill), the recovered pixels per frame or None)"""
                    got = d_occ.cpu().numpy()[:, 2:]
                    return (got[:, :, 0] + got[:, :, 2], got[:, :, 2].sum(axis=1)) if occlusion_search else (got[:, :, 0], None)

                def neighbour_dev(n, sid, nM, nm, window, d_image, d_mask, d_source, d_count, p):
                    """one neighbour candidate: the window call (the fill call without a window), or with occlusion the visible call, whose first
                    counter is copied behind it"""
                    head = (d_imgs[n].data_ptr(), channels, d_src[n].data_ptr(), d_Rs[n].data_ptr(), d_ts[n].data_ptr(), K, rows, cols, nM, nm, int(sid))
                    tail = (d_image.data_ptr(), d_mask.data_ptr(), None if d_source is None else d_source.data_ptr())
                    if occlusion:
                        call = solver.stabilize_search_frame_dev if occlusion_search else solver.stabilize_visible_frame_dev
                        call(*head, window or (0, 0, rows, cols), *tail, None if d_count is None else d_occ[p, int(sid)].data_ptr(), tol_q16=occ_q16, mode=mode)
                    elif window is None:
                        solver.stabilize_fill_frame_dev(*head, *tail, None if d_count is None else d_count.data_ptr(), mode=mode)
                    else:
                        solver.stabilize_window_frame_dev(*head, window, *tail, None if d_count is None else d_count.data_ptr(), mode=mode)

                if fill:
                    from . import neighbour_poses

                    d_fills, d_fmasks2, d_sources = [t.clone() for t in d_stabs], [t.clone() for t in d_smasks], [t.clone() for t in d_smasks]
                    d_fcnt = torch.zeros((nst, 2 + 2 * fill), dtype=torch.int64, device=dev)
                    d_fcnt[:, 1] = d_svalid
                    torch.cuda.synchronize()
                    for p in range(nst):  # every pass enqueued, one wait for all of them
                        for n, sid, nM, nm in zip(*neighbour_poses(traj["A"], traj["c"], A_s, c_s, st_scales, p, fill)):
                            neighbour_dev(n, sid, nM, nm, None, d_fills[p], d_fmasks2[p], d_sources[p], d_fcnt[p, int(sid):], p)
                    solver.synchronize()
                    counts = d_fcnt.cpu().numpy()
                    if occlusion:
                        counts[:, 2:], recovered = occ_counts()
                        if occlusion_search:
                            traj.update(fill_recovered=recovered)
                    counts[:, 0] = rows * cols - counts[:, 1:].sum(axis=1)
                    traj.update(stab_filled=[t.cpu().numpy() for t in d_fills], stab_sources=[t.cpu().numpy() for t in d_sources], fill_counts=counts)
                if crop:
                    from . import neighbour_poses

                    window = solver.crop_window_dev(ptrs(d_fmasks2 if fill else d_smasks), rows, cols, crop_max_empty, crop_margin)
                    d_crops = [torch.zeros_like(t) for t in d_stabs]
                    d_cmasks = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    d_ccnt = torch.zeros((nst, 2 + 2 * fill), dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    for p in range(nst if window[2] else 0):  # every pass enqueued, one wait for all of them
                        cand = [(p, 1, vM[p], vm[p])] + (list(zip(*neighbour_poses(traj["A"], traj["c"], A_s, c_s, st_scales, p, fill))) if fill else [])
                        for n, sid, nM, nm in cand:
                            if int(sid) == 1:  # the own frame keeps its call
                                solver.stabilize_window_frame_dev(d_imgs[n].data_ptr(), channels, d_src[n].data_ptr(), d_Rs[n].data_ptr(), d_ts[n].data_ptr(), K,
                                                                  rows, cols, nM, nm, 1, window, d_crops[p].data_ptr(), d_cmasks[p].data_ptr(), None,
                                                                  d_ccnt[p, 1:].data_ptr(), mode=mode)
                            else:
                                neighbour_dev(n, sid, nM, nm, window, d_crops[p], d_cmasks[p], None, d_ccnt[p, int(sid):], p)
                    solver.synchronize()
                    counts = d_ccnt.cpu().numpy()
                    if occlusion and window[2]:
                        counts[:, 2:], recovered = occ_counts()
                    if occlusion_search:
                        traj.update(crop_recovered=recovered if window[2] else np.zeros(nst, dtype=np.int64))
                    counts[:, 0] = rows * cols - counts[:, 1:].sum(axis=1)
                    traj.update(stab_cropped=[t.cpu().numpy() for t in d_crops], crop_window=window, crop_counts=counts)
                if blend:
                    from . import GAIN_ONE, neighbour_poses, seam_gains

                    bwindow = traj["crop_window"] if crop else (0, 0, rows, cols)
                    d_blends = [torch.zeros_like(t) for t in d_stabs]
                    d_bmasks = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    d_bsources = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    d_dist = torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
                    d_layers = [torch.zeros_like(d_stabs[0]) for _ in range(2 * fill)]  # one per candidate of a frame, zeroed again per frame
                    d_lmasks = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(2 * fill)]
                    d_sums = torch.zeros((nst, 2 * fill, 8), dtype=torch.int64, device=dev)  # (the records' 64-bit words)
                    d_bcnt = torch.zeros((nst, 2 * fill, 2), dtype=torch.int64, device=dev)
                    d_own = torch.zeros(nst, dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    for p in range(nst if bwindow[2] else 0):  # a frame's passes enqueued on the solver's stream, one wait per frame
                        if p:
                            for t in d_layers + d_lmasks:
                                t.zero_()
                            torch.cuda.synchronize()
                        solver.stabilize_window_frame_dev(d_imgs[p].data_ptr(), channels, d_src[p].data_ptr(), d_Rs[p].data_ptr(), d_ts[p].data_ptr(), K, rows, cols,
                                                          vM[p], vm[p], 1, bwindow, d_blends[p].data_ptr(), d_bmasks[p].data_ptr(), d_bsources[p].data_ptr(),
                                                          d_own[p:].data_ptr(), mode=mode)
                        solver.seam_distance_dev(d_bmasks[p].data_ptr(), rows, cols, blend_feather or 0, d_dist.data_ptr())
                        for n, sid, nM, nm in zip(*neighbour_poses(traj["A"], traj["c"], A_s, c_s, st_scales, p, fill)):
                            d_layer, d_lmask = d_layers[int(sid) - 2], d_lmasks[int(sid) - 2]
                            neighbour_dev(n, sid, nM, nm, bwindow, d_layer, d_lmask, None, None, p)
                            solver.seam_blend_layer_dev(d_layer.data_ptr(), d_lmask.data_ptr(), channels, rows, cols, d_dist.data_ptr(), int(sid),
                                                        d_blends[p].data_ptr(), d_bmasks[p].data_ptr(), d_bsources[p].data_ptr(), d_sums[p, int(sid) - 2].data_ptr(),
                                                        d_bcnt[p, int(sid) - 2].data_ptr(), feather=blend_feather, gain=blend_gain)
                        solver.synchronize()
                    sums, per, own = d_sums.cpu().numpy().view(np.uint64), d_bcnt.cpu().numpy(), d_own.cpu().numpy()
                    gains = np.full((nst, 2 * fill, 3), GAIN_ONE, dtype=np.uint32)
                    for p in range(nst):
                        for k_ in range(2 * fill):
                            gains[p, k_] = seam_gains(sums[p, k_], channels, 0, 0 if blend_gain else 1)
                    counts = np.concatenate([(rows * cols - own - per[:, :, 0].sum(axis=1))[:, None], (own - per[:, :, 1].sum(axis=1))[:, None],
                                             per.reshape(nst, -1)], axis=1)
                    traj.update(stab_blended=[t.cpu().numpy() for t in d_blends], blend_gains=gains, blend_counts=counts)
                if inpaint:
                    if blend:
                        stage, d_last, d_lmask, d_lsrc = "blended", d_blends, d_bmasks, d_bsources
                    elif crop:
                        stage, d_last, d_lmask, d_lsrc = "cropped", d_crops, d_cmasks, d_cmasks
                    elif fill:
                        stage, d_last, d_lmask, d_lsrc = "filled", d_fills, d_fmasks2, d_sources
                    else:
                        stage, d_last, d_lmask, d_lsrc = "stabilized", d_stabs, d_smasks, d_smasks
                    d_inps, d_isrcs = [t.clone() for t in d_last], [t.clone() for t in d_lsrc]
                    d_icnt = torch.zeros(nst, dtype=torch.int64, device=dev)
                    torch.cuda.synchronize()
                    for p in range(nst):  # every frame enqueued, one wait for all of them
                        solver.inpaint_frame_dev(d_inps[p].data_ptr(), d_lmask[p].data_ptr(), channels, rows, cols, d_isrcs[p].data_ptr(), d_icnt[p:].data_ptr())
                    solver.synchronize()
                    traj.update(stab_inpainted=[t.cpu().numpy() for t in d_inps], inpaint_sources=[t.cpu().numpy() for t in d_isrcs],
                                inpaint_counts=d_icnt.cpu().numpy())
                if retime is not None:  # the solved clip once more, at the asked instants along the smoothed path
                    from . import retime_times

                    times = retime_times(nst, retime) if np.ndim(retime) == 0 else np.asarray(retime, dtype=np.float64).reshape(-1)
                    d_rts = [torch.empty_like(d_imgs[0]) for _ in times]
                    d_rmasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in times]
                    d_rsrcs = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in times]
                    torch.cuda.synchronize()
                    rt = solver.retime_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s,
                                                 c_s, st_scales, times, ptrs(d_rts), ptrs(d_rmasks), ptrs(d_rsrcs), occlusion=occlusion,
                                                 occlusion_tol_q16=occ_q16 if occlusion else 0, mode=mode)
                    traj.update(retimed=[t.cpu().numpy() for t in d_rts], retime_masks=[t.cpu().numpy() for t in d_rmasks],
                                retime_sources=[t.cpu().numpy() for t in d_rsrcs], retime_counts=rt["counts"], retime_times=times)
                    if shutter is not None:  # the same instants once more, exposed
                        width, nsamp = (shutter, None) if np.ndim(shutter) == 0 else (shutter[0], int(shutter[1]))
                        d_sh = [torch.empty_like(d_imgs[0]) for _ in times]
                        d_shmasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in times]
                        d_shcov = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in times]
                        torch.cuda.synchronize()
                        sh = solver.shutter_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"],
                                                      A_s, c_s, st_scales, times, ptrs(d_sh), ptrs(d_shmasks), ptrs(d_shcov), shutter=float(width), samples=nsamp,
                                                      occlusion=occlusion, occlusion_tol_q16=occ_q16 if occlusion else 0, mode=mode)
                        traj.update(shuttered=[t.cpu().numpy() for t in d_sh], shutter_masks=[t.cpu().numpy() for t in d_shmasks],
                                    shutter_coverage=[t.cpu().numpy() for t in d_shcov], shutter_counts=sh["counts"], shutter_kept=sh["kept"])
                if denoise is not None:  # every stabilised frame once more, averaged with its neighbours
                    dn_one = not isinstance(denoise, (tuple, list, np.ndarray))  # K alone; (K, strength, (target, search)) is ragged: no np.ndim
                    dn_auto = not dn_one and isinstance(denoise[1], str)  # (K, "auto"[, spatial]): the strength from every frame's own noise
                    dn_temporal = dn_auto and denoise[1] == "temporal"  # (K, "temporal"[, spatial]): the curve measured from the registered neighbours
                    dn_curve = dn_auto and (denoise[1] == "curve" or dn_temporal)  # (K, "curve"[, spatial]): a strength per pixel from every frame's own noise curve
                    dn_auto = dn_auto and not dn_curve
                    if dn_auto and denoise[1] != "auto":
                        raise ValueError("denoise: the strength is an integer, None or \"auto\"")
                    dn_radius, dn_strength = (int(denoise), None) if dn_one else (int(denoise[0]), None if denoise[1] is None or dn_auto or dn_curve else int(denoise[1]))
                    dn_spatial = None if dn_one or len(denoise) < 3 or denoise[2] is None or denoise[2] is False else denoise[2]
                    d_dn = [torch.empty_like(d_imgs[0]) for _ in range(nst)]
                    d_dnmasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    d_dnw = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    dn_kw = dict(radius=dn_radius, strength=dn_strength, occlusion=occlusion, occlusion_tol_q16=occ_q16 if occlusion else 0, mode=mode)
                    if dn_auto:  # the frame's noise measured behind its own render, both stages at the strength it asks for
                        sp_target, sp_search = (None, None) if dn_spatial is None or dn_spatial is True else (int(dn_spatial[0]), int(dn_spatial[1]))
                        d_dns = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)] if dn_spatial is not None else None
                        torch.cuda.synchronize()
                        dn = solver.denoise_auto_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s,
                                                           c_s, st_scales, ptrs(d_dn), ptrs(d_dnmasks), ptrs(d_dnw), ptrs(d_dns) if d_dns else None,
                                                           spatial=dn_spatial is not None, target=sp_target, search=sp_search, **dn_kw)
                        from . import noise_strength

                        noise = dn["noise"].astype(np.int64)
                        noise[:, 3] = [noise_strength(int(r[0]), int(r[1])) for r in noise]  # [n, m, sigma_q8, h]
                        traj.update(stab_denoised=[t.cpu().numpy() for t in d_dn], denoise_masks=[t.cpu().numpy() for t in d_dnmasks],
                                    denoise_weights=[t.cpu().numpy() for t in d_dnw], denoise_counts=dn["counts"][:, :3].copy(), denoise_noise=noise)
                        if d_dns:
                            traj.update(denoise_support=[t.cpu().numpy() for t in d_dns], denoise_spatial_counts=dn["counts"][:, 3:].copy())
                    elif dn_curve:  # the frame's noise curve measured behind its own render, both stages at a strength per pixel
                        import rsdsfm_noise_curve as nc  # a module beside the import shim: the package's surface is pinned

                        sp_target, sp_search = (None, None) if dn_spatial is None or dn_spatial is True else (int(dn_spatial[0]), int(dn_spatial[1]))
                        d_dns = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)] if dn_spatial is not None else None
                        torch.cuda.synchronize()
                        dn_call = nc.denoise_curve_video_dev
                        if dn_temporal:  # the same arguments, keys and files; the curve comes from the differences to the registered neighbours
                            import rsdsfm_noise_temporal as nt

                            dn_call = nt.denoise_temporal_video_dev
                        dn = dn_call(solver, ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s, c_s, st_scales,
                                     ptrs(d_dn), ptrs(d_dnmasks), ptrs(d_dnw), ptrs(d_dns) if d_dns else None, spatial=dn_spatial is not None, target=sp_target, search=sp_search,
                                     **dn_kw)
                        curves = dn["curves"].astype(np.int64)  # (frames, 9, 4): [n, m, sigma_q8, 0] per band, then of all samples
                        traj.update(stab_denoised=[t.cpu().numpy() for t in d_dn], denoise_masks=[t.cpu().numpy() for t in d_dnmasks],
                                    denoise_weights=[t.cpu().numpy() for t in d_dnw], denoise_counts=dn["counts"][:, :3].copy(), denoise_curve=curves)
                        if d_dns:
                            traj.update(denoise_support=[t.cpu().numpy() for t in d_dns], denoise_spatial_counts=dn["counts"][:, 3:].copy())
                    elif dn_spatial is None:
                        torch.cuda.synchronize()
                        dn = solver.denoise_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s,
                                                      c_s, st_scales, ptrs(d_dn), ptrs(d_dnmasks), ptrs(d_dnw), **dn_kw)
                        traj.update(stab_denoised=[t.cpu().numpy() for t in d_dn], denoise_masks=[t.cpu().numpy() for t in d_dnmasks],
                                    denoise_weights=[t.cpu().numpy() for t in d_dnw], denoise_counts=dn["counts"])
                    else:  # the top-up behind the temporal stage of every frame: True, or (target, search)
                        sp_target, sp_search = (None, None) if dn_spatial is True else (int(dn_spatial[0]), int(dn_spatial[1]))
                        d_dns = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                        torch.cuda.synchronize()
                        dn = solver.denoise_spatial_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"],
                                                              A_s, c_s, st_scales, ptrs(d_dn), ptrs(d_dnmasks), ptrs(d_dnw), ptrs(d_dns), spatial_strength=dn_strength,
                                                              target=sp_target, search=sp_search, **dn_kw)
                        traj.update(stab_denoised=[t.cpu().numpy() for t in d_dn], denoise_masks=[t.cpu().numpy() for t in d_dnmasks],
                                    denoise_weights=[t.cpu().numpy() for t in d_dnw], denoise_counts=dn["counts"][:, :3].copy(),
                                    denoise_support=[t.cpu().numpy() for t in d_dns], denoise_spatial_counts=dn["counts"][:, 3:].copy())
                if superres is not None:  # every stabilised frame once more, on a finer grid, merged with its neighbours
                    sr_scale, sr_radius = (int(superres), None) if np.ndim(superres) == 0 else (int(superres[0]), int(superres[1]))
                    fine = (sr_scale * rows, sr_scale * cols)
                    d_sr = [torch.empty(fine + tuple(d_imgs[0].shape[2:]), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    d_srmasks = [torch.empty(fine, dtype=torch.uint8, device=dev) for _ in range(nst)]
                    torch.cuda.synchronize()
                    sr = solver.superres_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s,
                                                   c_s, st_scales, ptrs(d_sr), ptrs(d_srmasks), None, scale=sr_scale, radius=sr_radius, mode=mode)
                    traj.update(superres=[t.cpu().numpy() for t in d_sr], superres_masks=[t.cpu().numpy() for t in d_srmasks], superres_counts=sr["counts"])
                if plate is not None:  # every stabilised frame once more, as the median of itself and its neighbours, and where it moved
                    pl_radius, pl_threshold = (int(plate), None) if np.ndim(plate) == 0 else (int(plate[0]), int(plate[1]))
                    d_pl = [torch.empty_like(d_imgs[0]) for _ in range(nst)]
                    d_plmasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    d_plmov = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    torch.cuda.synchronize()
                    with _plate_estimator_for(solver, plate_estimator):
                        pl = solver.plate_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s,
                                                    c_s, st_scales, ptrs(d_pl), ptrs(d_plmasks), None, ptrs(d_plmov), radius=pl_radius, threshold=pl_threshold,
                                                    occlusion=occlusion, occlusion_tol_q16=occ_q16 if occlusion else 0, mode=mode)
                    traj.update(plate=[t.cpu().numpy() for t in d_pl], plate_moving=[t.cpu().numpy() for t in d_plmov], plate_counts=pl["counts"])
                if erase is not None:  # every stabilised frame once more, without what moved through it
                    d_er = [torch.empty_like(d_imgs[0]) for _ in range(nst)]
                    d_ermasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    d_ermatte = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    torch.cuda.synchronize()
                    with _plate_estimator_for(solver, plate_estimator):
                        er = solver.erase_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s,
                                                    c_s, st_scales, ptrs(d_er), ptrs(d_ermasks), ptrs(d_ermatte), None, radius=er_radius, open=er_open, grow=er_grow,
                                                    feather=er_feather, occlusion=occlusion, occlusion_tol_q16=occ_q16 if occlusion else 0, mode=mode)
                    traj.update(erased=[t.cpu().numpy() for t in d_er], erase_matte=[t.cpu().numpy() for t in d_ermatte], erase_counts=er["counts"])
                if deblur is not None:  # every stabilised frame once more, with what its sharper neighbours show
                    d_db = [torch.empty_like(d_imgs[0]) for _ in range(nst)]
                    d_dbmasks = [torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(nst)]
                    torch.cuda.synchronize()
                    db = solver.deblur_video_dev(ptrs(d_imgs), rows, cols, channels, K, ptrs(d_src[:nst]), ptrs(d_Rs[:nst]), ptrs(d_ts[:nst]), traj["A"], traj["c"], A_s,
                                                 c_s, st_scales, ptrs(d_db), ptrs(d_dbmasks), None, radius=db_radius, strength=db_strength, occlusion=occlusion,
                                                 occlusion_tol_q16=occ_q16 if occlusion else 0, mode=mode, band_rows=db_band_rows)
                    traj.update(deblurred=[t.cpu().numpy() for t in d_db], deblur_counts=db["counts"], deblur_taus=db["taus"])
                    if db_band_rows:
                        traj.update(deblur_band_taus=db["band_taus"])
                if sharpen is not None:  # one stream of frames once more, sharpened at every frame's own noise curve: behind everything else
                    import rsdsfm_sharpen as shp  # a module beside the import shim: the package's surface is pinned

                    if superres is not None:
                        sh_source, d_shin, d_shmask = "superres", d_sr, d_srmasks
                    elif deblur is not None:
                        sh_source, d_shin, d_shmask = "deblurred", d_db, d_dbmasks
                    elif denoise is not None:
                        sh_source, d_shin, d_shmask = "stab_denoised", d_dn, d_dnmasks
                    elif inpaint:
                        sh_source, d_shin, d_shmask = "stab_inpainted", d_inps, d_isrcs  # a source id is 0 exactly where nothing is
                    elif blend:
                        sh_source, d_shin, d_shmask = "stab_blended", d_blends, d_bmasks
                    elif crop:
                        sh_source, d_shin, d_shmask = "stab_cropped", d_crops, d_cmasks
                    elif fill:
                        sh_source, d_shin, d_shmask = "stab_filled", d_fills, d_fmasks2
                    else:
                        sh_source, d_shin, d_shmask = "stabilized", d_stabs, d_smasks
                    d_shout = [torch.empty_like(t) for t in d_shin]
                    torch.cuda.synchronize()
                    shr = shp.sharpen_video_dev(solver, ptrs(d_shin), ptrs(d_shmask), channels, int(d_shin[0].shape[0]), int(d_shin[0].shape[1]), ptrs(d_shout),
                                                amount_q4=sh_amount, coring_q4=sh_coring, overshoot=sh_overshoot)
                    traj.update(sharpened=[t.cpu().numpy() for t in d_shout], sharpen_counts=shr["counts"], sharpen_curves=shr["curves"].astype(np.int64),
                                sharpen_source=sh_source)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        lines = ["pair,v_x,v_y,v_z,w_x,w_y,w_z,k,inliers"]
        for p, o in enumerate(outs):
            _write_real_outputs(os.path.join(out_dir, str(p)), images[p], o["flow"], o["depth_est"], o["backprojection"], o["coords"])
            if dense:
                _write_dense_outputs(os.path.join(out_dir, str(p)), o["dense_image"], o["dense_mask"])
            if check_flow:
                formats.write_png(os.path.join(out_dir, str(p), "flow_mask.png"), (o["flow_mask"] * 255).astype(np.uint8))
            lines.append(",".join([str(p)] + ["%.17g" % x for x in list(o["v"]) + list(o["w"]) + [o["k"]]] + [str(o["num_inliers"])]))
        with open(os.path.join(out_dir, "poses.csv"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        if fuse:
            names = ["own", "filled_prev", "filled_next", "confirmed", "contradicted", "left"]
            flines = ["pair," + ",".join(names)]
            ii, jj = np.mgrid[0:rows, 0:cols].astype(np.float64)
            for p, o in enumerate(outs):
                z = o["fused_depth"]
                has = z > 0
                pts = np.stack([(jj[has] - K[2]) / K[0], (ii[has] - K[3]) / K[1], z[has]], axis=-1)  # the depth image's input: (x, y, z) per pixel with a value
                formats.write_png(os.path.join(out_dir, str(p), "depth_fused.png"), solver.depth_preview(pts, K, rows, cols))
                flines.append(",".join([str(p)] + [str(o["fuse_record"][k_]) for k_ in names]))
            with open(os.path.join(out_dir, "fusion.csv"), "w") as fh:
                fh.write("\n".join(flines) + "\n")
        if trajectory:
            rows_ = ["frame,c_x,c_y,c_z," + ",".join("a_%d%d" % (i, j) for i in range(3) for j in range(3)) + ",scale"]
            for f in range(npairs + 1):
                rows_.append(",".join([str(f)] + ["%.17g" % x for x in list(traj["c"][f]) + list(traj["A"][f].reshape(-1))] +
                                      ["%.17g" % traj["scales"][f] if f < npairs else ""]))
            with open(os.path.join(out_dir, "trajectory.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
            keep = [o["depth_map"] > 0 for o in outs]
            colour = [im if im.ndim == 3 else np.repeat(im[..., None], 3, axis=2) for im in images[:npairs]]
            formats.write_ply(os.path.join(out_dir, "clip.ply"), np.concatenate([traj["points"][p][keep[p]] for p in range(npairs)]),
                              np.concatenate([colour[p][keep[p]] for p in range(npairs)]))
        if stabilize:
            nst = npairs + (1 if last_frame else 0)
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "stabilized_%d.png" % p), traj["stabilized"][p])
            ps = traj["path_smoothed"]
            rows_ = ["frame,c_x,c_y,c_z," + ",".join("a_%d%d" % (i, j) for i in range(3) for j in range(3))]
            for f in range(npairs + 1):
                rows_.append(",".join([str(f)] + ["%.17g" % x for x in list(ps["c_s"][f]) + list(ps["A_s"][f].reshape(-1))]))
            with open(os.path.join(out_dir, "path_smoothed.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if fill:
            names = ["none", "own"] + ["%s%d" % (sg, j) for j in range(1, fill + 1) for sg in ("prev", "next")]
            rows_ = ["pair," + ",".join(names)]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "stabilized_filled_%d.png" % p), traj["stab_filled"][p])
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["fill_counts"][p]]))
            with open(os.path.join(out_dir, "fill.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if crop:
            names = ["none", "own"] + ["%s%d" % (sg, j) for j in range(1, fill + 1) for sg in ("prev", "next")]
            rows_ = ["window," + ",".join(str(x) for x in traj["crop_window"]), "pair," + ",".join(names)]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "stabilized_cropped_%d.png" % p), traj["stab_cropped"][p])
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["crop_counts"][p]]))
            with open(os.path.join(out_dir, "crop.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if occlusion_search:
            names = ["fill_recovered"] + (["crop_recovered"] if crop else [])
            rows_ = ["pair," + ",".join(names)] + [",".join([str(p)] + [str(int(traj[k_][p])) for k_ in names]) for p in range(nst)]
            with open(os.path.join(out_dir, "occlusion_search.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if blend:
            offs = ["%s%d" % (sg, j) for j in range(1, fill + 1) for sg in ("prev", "next")]
            names = ["none", "own_untouched"] + [o + "_" + w for o in offs for w in ("filled", "blended")] + ["gain_%s_%d" % (o, c_) for o in offs for c_ in range(3)]
            rows_ = ["pair," + ",".join(names)]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "stabilized_blended_%d.png" % p), traj["stab_blended"][p])
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["blend_counts"][p]] + [str(int(x)) for x in traj["blend_gains"][p].reshape(-1)]))
            with open(os.path.join(out_dir, "blend.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if retime is not None:
            rows_ = ["index,time,source_a,source_b,weight_q16,none,a_only,b_only,dissolved,conflict"]
            for i, t_ in enumerate(traj["retime_times"]):
                formats.write_png(os.path.join(out_dir, "retimed_%d.png" % i), traj["retimed"][i])
                rows_.append(",".join([str(i), "%.17g" % t_] + [str(int(x)) for x in list(rt["sources"][i]) + [rt["weights"][i]] + list(traj["retime_counts"][i])]))
            with open(os.path.join(out_dir, "retime.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if shutter is not None:
            rows_ = ["index,time,kept,unset,partial,full"]
            for i, t_ in enumerate(traj["retime_times"]):
                formats.write_png(os.path.join(out_dir, "shuttered_%d.png" % i), traj["shuttered"][i])
                rows_.append(",".join([str(i), "%.17g" % t_, str(int(traj["shutter_kept"][i]))] + [str(int(x)) for x in traj["shutter_counts"][i]]))
            with open(os.path.join(out_dir, "shutter.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if denoise is not None:
            topped = "denoise_spatial_counts" in traj  # three more columns: kept, smoothed, mean_support
            measured = "denoise_noise" in traj  # three more columns: noise_m, sigma, strength
            curved = "denoise_curve" in traj  # eleven more columns: noise_m0 .. noise_m7, noise_m, strength_min, strength_max
            rows_ = ["pair,unset,own_only,averaged,mean_weight" + (",kept,smoothed,mean_support" if topped else "") + (",noise_m,sigma,strength" if measured else "") +
                     ("," + ",".join("noise_m%d" % b for b in range(8)) + ",noise_m,strength_min,strength_max" if curved else "")]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "stabilized_denoised_%d.png" % p), traj["stab_denoised"][p])
                more = [str(int(x)) for x in traj["denoise_spatial_counts"][p][1:]] + ["%.4f" % float(traj["denoise_support"][p].mean())] if topped else []
                if measured:
                    nz = traj["denoise_noise"][p]
                    more = more + [str(int(nz[1])), "%.4f" % (int(nz[2]) / 256.0), str(int(nz[3]))]
                if curved:  # the band medians, the median of all samples, and the ends of the strength table the consumers formed (the defaults)
                    import rsdsfm_noise_curve as nc

                    lut = nc.noise_curve_strengths(traj["denoise_curve"][p].astype(np.uint64))
                    more = more + [str(int(m_)) for m_ in traj["denoise_curve"][p][:, 1]] + [str(int(lut.min())), str(int(lut.max()))]
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["denoise_counts"][p]] + ["%.4f" % float(traj["denoise_weights"][p].mean())] + more))
            with open(os.path.join(out_dir, "denoise.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if superres is not None:
            rows_ = ["pair,unset,own_only,merged"]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "superres_%d.png" % p), traj["superres"][p])
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["superres_counts"][p]]))
            with open(os.path.join(out_dir, "superres.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if plate is not None:
            rows_ = ["pair,unset,static,moving,undecided"]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "plate_%d.png" % p), traj["plate"][p])
                formats.write_png(os.path.join(out_dir, "moving_%d.png" % p), np.where(traj["plate_moving"][p] == 2, 255, 0).astype(np.uint8))
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["plate_counts"][p]]))
            with open(os.path.join(out_dir, "plate.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if erase is not None:
            rows_ = ["pair,unset,kept,replaced,feathered,unresolved"]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "erased_%d.png" % p), traj["erased"][p])
                formats.write_png(os.path.join(out_dir, "matte_%d.png" % p), (traj["erase_matte"][p].astype(np.int64) * 255 // erase_feather).astype(np.uint8))
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["erase_counts"][p]]))
            with open(os.path.join(out_dir, "erase.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if deblur is not None:
            rows_ = ["pair,unset,own_only,transferred," + ",".join("tau_%d" % j for j in range(traj["deblur_taus"].shape[1]))]
            bt = traj.get("deblur_band_taus")  # (frames, 6, NB): one column per neighbour and band behind the existing ones
            if bt is not None:
                rows_[0] += "," + ",".join("tau_%d_band_%d" % (j, b) for j in range(bt.shape[1]) for b in range(bt.shape[2]))
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "deblurred_%d.png" % p), traj["deblurred"][p])
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["deblur_counts"][p]] + [str(int(x)) for x in traj["deblur_taus"][p]] +
                                      ([str(int(x)) for x in bt[p].reshape(-1)] if bt is not None else [])))
            with open(os.path.join(out_dir, "deblur.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if sharpen is not None:
            import rsdsfm_noise_curve as nc

            rows_ = ["pair,unset,kept,sharpened,limited,noise_m,strength_min,strength_max"]
            for p in range(len(traj["sharpened"])):
                formats.write_png(os.path.join(out_dir, "sharpened_%d.png" % p), traj["sharpened"][p])
                lut = nc.noise_curve_strengths(traj["sharpen_curves"][p].astype(np.uint64))  # the table the kernel formed (the defaults)
                rows_.append(",".join([str(p)] + [str(int(x)) for x in traj["sharpen_counts"][p]] + [str(int(traj["sharpen_curves"][p][8, 1])), str(int(lut.min())),
                                                                                                      str(int(lut.max()))]))
            with open(os.path.join(out_dir, "sharpen.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
        if inpaint:
            rows_ = ["pair,stage,inpainted"]
            for p in range(nst):
                formats.write_png(os.path.join(out_dir, "stabilized_inpainted_%d.png" % p), traj["stab_inpainted"][p])
                rows_.append("%d,%s,%d" % (p, stage, int(traj["inpaint_counts"][p])))
            with open(os.path.join(out_dir, "inpaint.csv"), "w") as fh:
                fh.write("\n".join(rows_) + "\n")
    if trajectory:
        return dict(traj, pairs=outs)
    return outs


# ---------------------------------------------------------------------------------------------------
# parameter sweep (reference main.cc:148-299 -> error_measure::evaluateVelocities, errorMeasure.cpp:41-254)
# ---------------------------------------------------------------------------------------------------
def evaluate_velocities(solvers, archive, gamma, ransac_trials=50, num_evaluations=5, constant_acceleration=False, global_shutter=False,
                        optimize_results=True, tol=0.05, flow_threshold=1e-10, base_seed=1, image_path=None, flow_index_mode=0):
    """errorMeasure.cpp:41-254 for one task: ground-truth flow once, then `num_evaluations` independent solves (the reference
    reseeds rand() per trial; here evaluation e uses the sampler seed base_seed + e) with their rotation / translation /
    reprojection errors.  `solvers`: one Solver or a list -- the evaluations are independent and are spread over the
    contexts, one host thread each (sequence-throughput mode).  flow_index_mode 0 (default) = the reference's rank-indexed flow
    (errorMeasure.cpp:152 -> nonlinearRefinement.cc:209-212, quirk Q2), 1 = gathered."""
    from concurrent.futures import ThreadPoolExecutor

    from . import BACKPROJECT_GS, BACKPROJECT_RS, Solver, velocity_errors

    if isinstance(solvers, Solver):
        solvers = [solvers]
    K, truth = archive["K"], archive["truth"]
    f1, f2 = archive["frames"]
    rows, cols = f1["rs_image"].shape[:2]
    s0 = solvers[0]
    flow, _ = s0.true_flow(f1["world"], f2["R"], f2["t"], K, want_best_row=False)
    q, u, alpha, alpha_k = s0.flatten(flow, K, gamma, thr=flow_threshold)
    if global_shutter:  # errorMeasure.cpp:107-112
        alpha = alpha * 0.0 + 1.0
        constant_acceleration = False
    gt_depth = gt_depth_map(f1["world"], f1["R"], f1["t"])
    R_abs, t_abs = relocate_pose(f1["R"], f1["t"])

    def one(e):
        s = solvers[e % len(solvers)]
        rr = s.ransac(q, u, alpha, alpha_k, constant_acceleration, ransac_trials, tol, samples=None, seed=base_seed + e)
        res = dict(v=rr["v"], w=rr["w"], k=rr["k"], inliers=rr["inliers"])
        if optimize_results:
            ref = s.non_linear_refinement(u, rr["inliers"], rr["alpha"], rr["alpha_k"], rr["v"], rr["w"], rr["k"], constant_acceleration,
                                          flow_index_mode=flow_index_mode, inlier_idx=rr["inlier_idx"] if flow_index_mode else None)
            res = dict(v=ref["v"], w=ref["w"], k=ref["k"], inliers=ref["inliers"])
        dm = s.depth_map(res["inliers"], res["v"], K, rows, cols)
        w_err, v_err = velocity_errors(res["w"], dm["v"], truth["w"], truth["v"])
        R_rel, t_rel = s.pose_table(dm["v"], res["w"], res["k"], gamma, rows)
        _, coords = s.back_project(f1["rs_image"], dm["depth_map"], R_rel, t_rel, K, mode=BACKPROJECT_GS if global_shutter else BACKPROJECT_RS)
        stats, _ = s.reprojection_error(coords, gt_depth, dm["depth_map"], R_abs, t_abs, K, want_image=False)
        if image_path:
            formats.write_png("%s%d.png" % (image_path, e), s.depth_preview(dm["inliers"], K, rows, cols))
            formats.write_ply("%s%d.ply" % (image_path, e), coords, f1["rs_image"])
        return dict(w=res["w"], v=dm["v"], k=res["k"], w_error=w_err, v_error=v_err, reproject_error=stats["mean_error"], num_inliers=rr["num_inliers"])

    if len(solvers) == 1:
        runs = [one(e) for e in range(num_evaluations)]
    else:
        with ThreadPoolExecutor(max_workers=len(solvers)) as pool:
            # evaluation e always runs on context e % S: one thread per context at a time
            chunks = [list(range(j, num_evaluations, len(solvers))) for j in range(len(solvers))]
            parts = list(pool.map(lambda ch: [(e, one(e)) for e in ch], chunks))
        runs = [r for _, r in sorted((er for p in parts for er in p), key=lambda er: er[0])]
    col = lambda key: np.array([r[key] for r in runs])
    return dict(w=col("w"), v=col("v"), k=col("k"), error_w_vec=col("w_error"), error_v_vec=col("v_error"), error_reproject_vec=col("reproject_error"),
                error_w=float(col("w_error").mean()), error_v=float(col("v_error").mean()), error_reproject=float(col("reproject_error").mean()),
                num_inliers=col("num_inliers"))


def evaluate_parameter_sweep(solvers, path, result_dir, tasks=None, **kw):
    """main.cc:148-299: every task directory listed in <path>/tasks.txt (or `tasks`) -> errors.csv, w.csv, v.csv, k.csv,
    reproject_errors.csv, error_v.csv, error_w.csv and depthMaps/<task index>/<evaluation>.{png,ply} under result_dir"""
    if tasks is None:
        tasks = [ln.strip() for ln in open(os.path.join(path, "tasks.txt")) if ln.strip()]
    os.makedirs(result_dir, exist_ok=True)
    results = []
    for i, task in enumerate(tasks):
        archive = formats.load_example_archive(os.path.join(path, task))
        image_path = os.path.join(result_dir, "depthMaps", str(i)) + "/"
        os.makedirs(image_path, exist_ok=True)
        results.append(evaluate_velocities(solvers, archive, archive["truth"]["gamma"], image_path=image_path, **kw))
    formats.write_sweep_results(result_dir, tasks, [r["error_w_vec"] for r in results], [r["error_v_vec"] for r in results],
                                [r["error_reproject_vec"] for r in results], w=[r["w"] for r in results], v=[r["v"] for r in results],
                                k=[r["k"] for r in results])
    return dict(zip(tasks, results))

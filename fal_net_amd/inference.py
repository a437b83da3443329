"""Inference post-processing of Test_KITTI.py (ms_pp :287-300, flip post-process :200-203) around the HIP model.
The resampling of the 1- and 3-channel maps (bilinear x2/3, nearest back) goes through falnet_resize_planar; only the
host-side 95th percentile stays in numpy exactly as in the reference (opt-in: the exact device-side percentile of dumps.py); the two
network forwards are the HIP plan.  `evaluate(writer=...)` also writes every frame's outputs to disk (dumps.FrameWriter), `evaluate(sweep_writer=...)` its views along the
baseline (dumps.SweepWriter), `evaluate(freeview_writer=...)` its free-viewpoint views (freeview.FreeviewWriter), `evaluate(stats_writer=...)` the statistics of its disparity distribution and its confidence-filtered point cloud
(confidence.StatsWriter), `evaluate(lidar_writer=...)` its disparity back-projected into a Velodyne-format scan (pseudo_lidar.PseudoLidarWriter), `evaluate(mesh_writer=...)` its disparity as a triangle mesh cut at its depth edges (mesh.MeshWriter);
`evaluate(sparsification=...)` the sparsification curves of its confidence scores against its depth errors (sparsification.SparsificationTable);
`evaluate(disparity="peak")` evaluates the peak disparity of the same forward instead of the expectation."""
import math

import numpy as np
import torch

from . import _lib as L
from .train import hflip


def resize_planar(x, size, bilinear, scale=1.0):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) / mode='nearest' on planar f32 (B, C, H, W), times `scale`."""
    B, C, H, W = x.shape
    x = x.contiguous().float()
    out = torch.empty(B, C, size[0], size[1], device=x.device)
    L.check(L.lib().falnet_resize_planar(L.ptr(x), L.ptr(out), B * C, H, W, size[0], size[1], int(bilinear), float(scale), L.stream_ptr()),
            "resize_planar")
    return out


def ms_pp(input_view, pan_model, disp, min_disp, max_pix, device_percentile=False):
    """Test_KITTI.py:287-300: second forward on the flipped, x2/3-downscaled view; blend by normalised disparity.
    device_percentile: the 95th percentile comes from dumps.percentile (exact, on the device, per sample) instead of the copy to the host and
    np.percentile over the whole batch; the reference's loop runs at batch size 1, where the two are the same number."""
    B, C, H, W = input_view.shape
    up_fac = 2 / 3
    # F.interpolate(scale_factor=2/3) sizes the output as floor(in * scale) and (align_corners=True) samples at dst (in-1)/(out-1)
    upscaled = resize_planar(hflip(input_view), (int(math.floor(H * up_fac)), int(math.floor(W * up_fac))), bilinear=True)
    dwn_flip_disp = pan_model(upscaled, min_disp, max_pix, ret_disp=True, ret_pan=False, ret_subocc=False)
    dwn_flip_disp = resize_planar(dwn_flip_disp, (H, W), bilinear=False, scale=1 / up_fac)
    dwn_flip_disp = hflip(dwn_flip_disp)
    if device_percentile:
        from . import dumps
        norm = disp / (dumps.percentile(disp, 95.0).view(-1, 1, 1, 1) + 1e-6)
    else:
        norm = disp / (np.percentile(disp.detach().cpu().numpy(), 95) + 1e-6)
    norm[norm > 1] = 1
    return (1 - norm) * disp + norm * dwn_flip_disp


def flip_post_process(input_view, pan_model, disp, min_disp, max_pix):
    """Test_KITTI.py:200-203."""
    flip_disp = pan_model(hflip(input_view), min_disp, max_pix, ret_disp=True, ret_pan=False, ret_subocc=False)
    return (disp + hflip(flip_disp)) / 2


def dump_frame(writer, i, pan_model, left, disp, min_disp, max_pix):
    """Frame `i` to disk through a dumps.FrameWriter (Test_KITTI.py:189-194,211-253).  The synthesised view and the occlusion masks come
    from one more forward with ret_pan / ret_subocc, only where the writer wants them; the feature maps are the reference's
    [local_normalization(input), maskL, maskRL] (its `dispr / 100` is not an output of this model's forward)."""
    from . import dumps
    pan = feats = None
    if writer.needs_views:
        pan, _, mask_l, mask_rl = pan_model(left, min_disp, max_pix, ret_disp=True, ret_subocc=True, ret_pan=True)
        feats = [dumps.local_normalization(left), mask_l, mask_rl]
    writer.write(i, left, disp, pan=pan, feats=feats)


def sweep_frame(sweep_writer, i, pan_model, left, min_disp, max_pix, fractions):
    """Frame `i` through a dumps.SweepWriter: the views at the baseline `fractions` and the disparity in the right view's own frame (t = 1),
    all from the logits of one more disparity-only forward (views.render)."""
    from . import views as V
    ts = list(fractions)
    if 1.0 not in ts:
        ts.append(1.0)  # rendered for its disparity only
    imgs, disps, _ = V.render(pan_model, left, min_disp, max_pix, ts)
    sweep_writer.write(i, imgs[:, :len(fractions)], right_disp=disps[:, ts.index(1.0)])


def freeview_frame(freeview_writer, i, pan_model, left, min_disp, max_pix, pose_kwargs, fill_beta=None):
    """Frame `i` through a freeview.FreeviewWriter: the views and cover maps of the target cameras `pose_kwargs` (freeview.pose keyword sets, as
    freeview.paths returns them) around the nominal camera of the frame's size, from the logits of one more disparity-only forward
    (freeview.render).  fill_beta: also the hole-filled views (freeview.fill_views with that bias) as ..._filled.png."""
    from . import freeview as FV
    K = FV.camera(left.shape[-2], left.shape[-1])
    out, _ = FV.render(pan_model, left, min_disp, max_pix, [FV.pose(K, **kw) for kw in pose_kwargs], want=("view", "cover"), fill=fill_beta)
    freeview_writer.write(i, out["view"], out["cover"])
    if fill_beta is not None:
        freeview_writer.write_filled(i, out["view_filled"])


def stats_frame(stats_writer, i, pan_model, left, disp, min_disp, max_pix):
    """Frame `i` through a confidence.StatsWriter: the statistics of the logits of one more disparity-only forward (confidence.from_model);
    the filtered point cloud is made of `disp`, the disparity the run evaluates."""
    from . import confidence
    st, _ = confidence.from_model(pan_model, left, min_disp, max_pix, stats_writer.which)
    B, _, H, W = left.shape
    stats_writer.write(i, left, disp, st, pan_model._plan(B, H, W, left.device).buf["dlog0"].shape[1])


def lidar_frame(lidar_writer, i, pan_model, left, disp, min_disp, max_pix):
    """Frame `i` through a pseudo_lidar.PseudoLidarWriter: `disp`, the disparity the run evaluates, back-projected with the calibration the
    writer has for the frame.  The confidence map comes from one more disparity-only forward (confidence.from_model), only when the writer
    filters by it."""
    conf = None
    if lidar_writer.min_conf is not None:
        from . import confidence
        conf = confidence.from_model(pan_model, left, min_disp, max_pix, ("conf",))[0]["conf"]
    P, fb = lidar_writer.calibration(i, disp.shape[-2], disp.shape[-1])
    lidar_writer.write(i, disp, P, fb, conf=conf)


def mesh_frame(mesh_writer, i, pan_model, left, disp, min_disp, max_pix):
    """Frame `i` through a mesh.MeshWriter: `disp`, the disparity the run evaluates, as a triangle mesh cut at its depth edges.  The confidence
    map comes from one more disparity-only forward (confidence.from_model), only when the writer filters by it."""
    conf = None
    if mesh_writer.min_conf is not None:
        from . import confidence
        conf = confidence.from_model(pan_model, left, min_disp, max_pix, ("conf",))[0]["conf"]
    mesh_writer.write(i, left, disp, conf=conf)


def sparsify_frame(table, pan_model, left, disp, target, mode, use_median, min_disp, max_pix):
    """One frame with ground truth into the next row of a sparsification.SparsificationTable.  The errors are those of `disp`, the disparity the
    run evaluates AFTER post-processing; the scores (table.names, from sparsification.SCORES) are statistics of the logits of one more
    disparity-only forward of the plain view (confidence.from_model), as in stats_frame: with ms_pp or the flip post-processing the scores
    describe the first of the two blended forwards."""
    from . import confidence
    from . import sparsification as S
    st, _ = confidence.from_model(pan_model, left, min_disp, max_pix, S.stats_needed(table.names))
    S.curves(disp, target, mode, S.score_maps(st, table.names), use_median=use_median, steps=table.steps, out=table.row(table.n))


def view_frame(table, pan_model, left, right, min_disp, max_pix):
    """One frame's synthesised right view against the real one into the next row of `table` (a metrics.MetricTable of the view's own): RMSE, MAE
    and PSNR (metrics.view_errors) and SSIM (metrics.ssim), from one more forward with ret_pan=True."""
    from . import metrics as M
    p_im, _ = pan_model(left, min_disp, max_pix, ret_disp=True, ret_subocc=False, ret_pan=True)
    row = table.row(table.n)
    M.view_errors(p_im, right, out=row)
    M.ssim(p_im, right, out=row)


def view_result(table):
    """{'rmse', 'mea', 'psnr', 'ssim': means over the frames, 'n'} of a view_frame table -- the one read of it."""
    res = table.result()
    return {"rmse": res["rmse_mean"], "mea": res["mea_mean"], "psnr": res["psnr_mean"], "ssim": res["ssim_mean"], "n": int(len(res["view"]))}


def peak_disparity(pan_model, left, min_disp, max_pix):
    """The forward with the peak disparity (confidence.py: the expectation over the arg-max plane and its two neighbours) in the place of
    the expectation over all planes: one disparity-only forward and one statistics launch over its logits."""
    from . import confidence
    return confidence.from_model(pan_model, left, min_disp, max_pix, ("peak",))[0]["peak"]


def evaluate(pan_model, loader, data_name="Kitti2015", max_disp=300.0, min_disp=2.0, rel_baseline=1.0, post="ms_pp", use_median=False,
             print_freq=10, log=print, with_metrics=True, writer=None, device_percentile=False, device_metrics=False, sweep_writer=None,
             sweep_fractions=None, stats_writer=None, disparity="mean", lidar_writer=None, sparsification=None, view_metrics=False,
             freeview_writer=None, freeview_poses=None, freeview_fill=None, mesh_writer=None):
    """The evaluation loop of Test_KITTI.py:163-208,255-280 over a loader of full-size frames (batch size 1: KITTI mixes image
    sizes, :113): forward (+ flip or multi-scale post-processing, :196-205), then per image the KITTI depth errors and -- for
    KITTI 2015 -- the end-point error (:257-271).  `loader` yields lists of (left_u8, right_u8, gt) from
    datasets.StereoValDataset; gt is a disparity map (Kitti2015) or a depth map (Eigen split, listdataset_test.py:43-46 reads both
    as uint16 / 256); with datasets.StereoEvalDataset it may also be the depth map of a '.npy' file or a datasets.VeloScan (a raw Velodyne
    scan and its projection matrix: the depth map is then velodyne.project of it on the device) -- the original Eigen split.
    Returns {'epe', 'kitti': {name: value}, 'n', 'sec_per_image'} (and 'sparsification' with `sparsification`).
    writer: a dumps.FrameWriter -- every frame's outputs are also written to disk (:211-253), after the timed region and after the metrics;
    where it wants the synthesised view or the occlusion masks the model runs once more with ret_pan / ret_subocc.  device_percentile: ms_pp.
    device_metrics: the depth errors (median scaling included) and the EPE come from the kernels behind fal_net_amd/metrics.py -- no map and no
    metric is copied to the host per frame; the results table is read after the last frame (and on the iterations that print, for the running a1).
    sweep_writer / sweep_fractions: a dumps.SweepWriter and baseline fractions -- every frame's views along the baseline are written too (sweep_frame).
    freeview_writer / freeview_poses: a freeview.FreeviewWriter and freeview.pose keyword sets -- every frame's free-viewpoint views are written too (freeview_frame);
    freeview_fill: a bias beta -- their hole-filled versions as well (freeview.fill_views).
    stats_writer: a confidence.StatsWriter -- every frame's distribution statistics and its confidence-filtered point cloud are written too (stats_frame).
    lidar_writer: a pseudo_lidar.PseudoLidarWriter -- every frame's disparity is also written as a Velodyne-format scan (lidar_frame).
    mesh_writer: a mesh.MeshWriter -- every frame's disparity is also written as a triangle mesh cut at its depth edges (mesh_frame).
    sparsification: a sparsification.SparsificationTable built with the score names -- every frame with ground truth also leaves its sparsification
    curves in the table's next row (sparsify_frame: the errors of `disp` after post-processing, the scores from one more disparity-only forward), with
    and without device_metrics; the table is read once after the last frame and its result() is returned under 'sparsification'.
    view_metrics: every frame with a right image also runs one more forward with ret_pan=True after the timed region, and the synthesised view's
    RMSE / MAE / PSNR and SSIM against the loader's right image go into a device table of their own (view_frame), read once after the last frame; the
    result gains 'view': {'rmse', 'mea', 'psnr', 'ssim', 'n'}.
    disparity: "mean" (the forward's expectation) or "peak" (peak_disparity; only with post == "none": ms_pp and the flip blend two expectations)."""
    if disparity not in ("mean", "peak"):
        raise ValueError("disparity must be 'mean' or 'peak', got {!r}".format(disparity))
    if disparity == "peak" and post != "none":
        raise ValueError("disparity='peak' needs post='none': ms_pp and the flip post-processing blend two expectation maps")
    import time
    from . import datasets as DS
    from . import myUtils as utils
    from .loss_functions import realEPE
    dev = next(pan_model.parameters()).device
    pan_model.eval()
    epes, kitti, batch_time = utils.AverageMeter(), utils.multiAverageMeter(utils.kitti_error_names), utils.AverageMeter()
    n = 0
    table = None
    if device_metrics and with_metrics:
        from . import metrics as M
        table = M.MetricTable(len(loader.dataset) if hasattr(loader, "dataset") else 1, dev)
    view_table = None
    if view_metrics:
        from . import metrics as M
        view_table = M.MetricTable(len(loader.dataset) if hasattr(loader, "dataset") else 1, dev)
    with torch.no_grad():
        for i, batch in enumerate(loader):
            for left_u8, right_u8, gt in batch:
                left = DS.to_model_input(left_u8, dev)
                mx = torch.full((1, 1, 1), float(max_disp) * rel_baseline, device=dev)  # :181-182
                mn = mx * min_disp / max_disp
                torch.cuda.synchronize()
                t0 = time.time()
                if disparity == "peak":
                    disp = peak_disparity(pan_model, left, mn, mx)
                else:
                    disp = pan_model(left, mn, mx, ret_disp=True, ret_subocc=False, ret_pan=False)  # :196
                if post == "flip":
                    disp = flip_post_process(left, pan_model, disp, mn, mx)
                elif post == "ms_pp":
                    disp = ms_pp(left, pan_model, disp, mn, mx, device_percentile)
                torch.cuda.synchronize()
                batch_time.update(time.time() - t0, 1)
                if gt is not None and with_metrics:  # `-eval False`: forward and timing only (:255)
                    if isinstance(gt, DS.VeloScan):  # original Eigen split from a raw scan: the ground truth is projected here, at the left image's size
                        from . import velodyne
                        gt = velodyne.project(gt.points.to(dev), gt.P, left_u8.shape[0], left_u8.shape[1])
                    target = gt.to(dev).view(1, 1, *gt.shape)
                    if table is not None:
                        row = table.row(table.n)
                        if data_name == "Kitti2015":
                            M.epe(disp, target, sparse=True, out=row)
                        M.depth_errors(disp, target, "kitti2015" if data_name == "Kitti2015" else "eigen", use_median=use_median, out=row)
                    else:
                        t_np, p_np = target.squeeze(1).cpu().numpy(), disp.float().squeeze(1).cpu().numpy()
                        if data_name == "Kitti2015":  # :265-271
                            epes.update(float(realEPE(disp, target, sparse=True)), 1)
                            gt_depth, pred_depth = utils.disps_to_depths_kitti2015(t_np, p_np)
                        else:  # Eigen split: :258-263
                            gt_depth, pred_depth = utils.disps_to_depths_kitti(t_np, p_np)
                        kitti.update(utils.compute_kitti_errors(gt_depth[0], pred_depth[0], use_median=use_median), 1)
                    if sparsification is not None:
                        sparsify_frame(sparsification, pan_model, left, disp, target, "kitti2015" if data_name == "Kitti2015" else "eigen", use_median, mn, mx)
                if view_table is not None and right_u8 is not None:
                    view_frame(view_table, pan_model, left, DS.to_model_input(right_u8, dev), mn, mx)
                if writer is not None:
                    dump_frame(writer, n, pan_model, left, disp, mn, mx)
                if sweep_writer is not None:
                    sweep_frame(sweep_writer, n, pan_model, left, mn, mx, sweep_fractions)
                if freeview_writer is not None:
                    freeview_frame(freeview_writer, n, pan_model, left, mn, mx, freeview_poses, fill_beta=freeview_fill)
                if stats_writer is not None:
                    stats_frame(stats_writer, n, pan_model, left, disp, mn, mx)
                if lidar_writer is not None:
                    lidar_frame(lidar_writer, n, pan_model, left, disp, mn, mx)
                if mesh_writer is not None:
                    mesh_frame(mesh_writer, n, pan_model, left, disp, mn, mx)
                n += 1
            if log is not None and i % print_freq == 0:
                a1 = kitti.avg[4] if table is None else table.running_mean("a1")
                log('Test: [{0}/{1}]\t Time {2}\t a1 {3:.4f}'.format(i, len(loader), batch_time, a1))  # :273-275
    if table is not None:  # the one read of the table: the meters are filled frame by frame, as the host path fills them
        res = table.result()
        for e in res["epe"]:
            epes.update(float(e), 1)
        for errs in res["depth"]:
            kitti.update(errs, 1)
    out = {"epe": epes.avg, "kitti": dict(zip(utils.kitti_error_names, [float(a) for a in kitti.avg])), "kitti_table": repr(kitti), "n": n,
           "sec_per_image": batch_time.avg}
    if sparsification is not None:
        out["sparsification"] = sparsification.result()
    if view_table is not None:
        out["view"] = view_result(view_table)
    return out

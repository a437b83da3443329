"""Inference post-processing of Test_KITTI.py (ms_pp :287-300, flip post-process :200-203) around the HIP model.
The resampling of the 1- and 3-channel maps (bilinear x2/3, nearest back) goes through falnet_resize_planar; only the
host-side 95th percentile stays in numpy exactly as in the reference (opt-in: the exact device-side percentile of dumps.py); the two
network forwards are the HIP plan.  `evaluate(products=[...])` hands every frame, after the timed region, to each product's `frame(f)` as a `Frame`:
sparsification.SparsificationTable (curves of the confidence scores against the depth errors), ViewMetrics (the synthesised view against the right
image), dumps.FrameWriter (the frame's outputs on disk), dumps.SweepWriter (views along the baseline), freeview.FreeviewWriter (free-viewpoint views),
confidence.StatsWriter (statistics of the disparity distribution, the confidence-filtered point cloud), pseudo_lidar.PseudoLidarWriter (a
Velodyne-format scan), mesh.MeshWriter (a triangle mesh cut at the depth edges), cloud_metrics.CloudMetrics (Chamfer distance and F-score between
the back-projected prediction and ground truth), ground.GroundPlanes (the fitted road plane of the frame's scan) -- that is the order Test_KITTI.py
lists them in.
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


class Frame:
    """One evaluated frame as the products see it: a plain attribute holder.  `disp` is the disparity the run evaluates, after post-processing;
    `right` and `target` (the ground truth as (1, 1, H, W)) are None where the frame has none; mode: "kitti2015" / "eigen", as metrics.depth_errors
    takes it.  Nothing is cached: every stats() / conf() is one more disparity-only forward."""

    def __init__(self, index, model, left, disp, min_disp, max_disp, right=None, target=None, mode="eigen", use_median=False):
        self.index, self.model, self.left, self.right, self.disp = index, model, left, right, disp
        self.min_disp, self.max_disp, self.target, self.mode, self.use_median = min_disp, max_disp, target, mode, use_median

    def stats(self, which):
        """The statistics `which` of the logits of one more disparity-only forward of the plain view (confidence.from_model)."""
        from . import confidence
        return confidence.from_model(self.model, self.left, self.min_disp, self.max_disp, which)[0]

    def conf(self):
        return self.stats(("conf",))["conf"]


def run_products(products, f):
    """Frame `f` through every product, in list order.  A product is any object with frame(f); one with summary() also has `key`, the name of its
    JSON line, and one with result() has its entry under `key` in what evaluate() returns."""
    for p in products:
        p.frame(f)


class ViewMetrics:
    """The product behind Test_KITTI.py --view-metrics: every frame with a right image runs one more forward with ret_pan=True, and the synthesised
    view's RMSE, MAE and PSNR (metrics.view_errors) and SSIM (metrics.ssim) against it go into the next row of a metrics.MetricTable of its own.
    beside: what the JSON line carries next to `key`."""
    key = "view"

    def __init__(self, n_frames=1, device="cuda", beside=None):
        from . import metrics
        self.table, self.beside = metrics.MetricTable(n_frames, device), dict(beside or {})

    def frame(self, f):
        if f.right is None:
            return
        from . import metrics as M
        p_im, _ = f.model(f.left, f.min_disp, f.max_disp, ret_disp=True, ret_subocc=False, ret_pan=True)
        row = self.table.row(self.table.n)
        M.view_errors(p_im, f.right, out=row)
        M.ssim(p_im, f.right, out=row)

    def result(self):
        """{'rmse', 'mea', 'psnr', 'ssim': means over the frames, 'n'} -- one read of the table."""
        res = self.table.result()
        return {"rmse": res["rmse_mean"], "mea": res["mea_mean"], "psnr": res["psnr_mean"], "ssim": res["ssim_mean"], "n": int(len(res["view"]))}

    summary = result


def peak_disparity(pan_model, left, min_disp, max_pix):
    """The forward with the peak disparity (confidence.py: the expectation over the arg-max plane and its two neighbours) in the place of
    the expectation over all planes: one disparity-only forward and one statistics launch over its logits."""
    from . import confidence
    return confidence.from_model(pan_model, left, min_disp, max_pix, ("peak",))[0]["peak"]


def evaluate(pan_model, loader, data_name="Kitti2015", max_disp=300.0, min_disp=2.0, rel_baseline=1.0, post="ms_pp", use_median=False,
             print_freq=10, log=print, with_metrics=True, device_percentile=False, device_metrics=False, disparity="mean", products=()):
    """The evaluation loop of Test_KITTI.py:163-208,255-280 over a loader of full-size frames (batch size 1: KITTI mixes image
    sizes, :113): forward (+ flip or multi-scale post-processing, :196-205), then per image the KITTI depth errors and -- for
    KITTI 2015 -- the end-point error (:257-271).  `loader` yields lists of (left_u8, right_u8, gt) from
    datasets.StereoValDataset; gt is a disparity map (Kitti2015) or a depth map (Eigen split, listdataset_test.py:43-46 reads both
    as uint16 / 256); with datasets.StereoEvalDataset it may also be the depth map of a '.npy' file or a datasets.VeloScan (a raw Velodyne
    scan and its projection matrix: the depth map is then velodyne.project of it on the device) -- the original Eigen split.
    Returns {'epe', 'kitti': {name: value}, 'n', 'sec_per_image'} and, for every product with a result(), its result under its `key`.
    device_percentile: ms_pp.
    device_metrics: the depth errors (median scaling included) and the EPE come from the kernels behind fal_net_amd/metrics.py -- no map and no
    metric is copied to the host per frame; the results table is read after the last frame (and on the iterations that print, for the running a1).
    products: every frame goes through them as a Frame (run_products), after the timed region and after the metrics, in list order.
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
    mode = "kitti2015" if data_name == "Kitti2015" else "eigen"
    table = None
    if device_metrics and with_metrics:
        from . import metrics as M
        table = M.MetricTable(len(loader.dataset) if hasattr(loader, "dataset") else 1, dev)
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
                target = None
                if gt is not None and with_metrics:  # `-eval False`: forward and timing only (:255)
                    if isinstance(gt, DS.VeloScan):  # original Eigen split from a raw scan: the ground truth is projected here, at the left image's size
                        from . import velodyne
                        gt = velodyne.project(gt.points.to(dev), gt.P, left_u8.shape[0], left_u8.shape[1])
                    target = gt.to(dev).view(1, 1, *gt.shape)
                    if table is not None:
                        row = table.row(table.n)
                        if data_name == "Kitti2015":
                            M.epe(disp, target, sparse=True, out=row)
                        M.depth_errors(disp, target, mode, use_median=use_median, out=row)
                    else:
                        t_np, p_np = target.squeeze(1).cpu().numpy(), disp.float().squeeze(1).cpu().numpy()
                        if data_name == "Kitti2015":  # :265-271
                            epes.update(float(realEPE(disp, target, sparse=True)), 1)
                            gt_depth, pred_depth = utils.disps_to_depths_kitti2015(t_np, p_np)
                        else:  # Eigen split: :258-263
                            gt_depth, pred_depth = utils.disps_to_depths_kitti(t_np, p_np)
                        kitti.update(utils.compute_kitti_errors(gt_depth[0], pred_depth[0], use_median=use_median), 1)
                if products:
                    right = DS.to_model_input(right_u8, dev) if right_u8 is not None else None
                    run_products(products, Frame(n, pan_model, left, disp, mn, mx, right=right, target=target, mode=mode, use_median=use_median))
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
    for p in products:
        if hasattr(p, "result"):
            out[p.key] = p.result()
    return out

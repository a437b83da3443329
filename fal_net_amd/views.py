"""Views and disparities along the baseline from the logits of one forward (csrc/med_sweep.hip; inference only, no gradient).

The network's probability volume over N disparity planes describes the scene; the view at fraction t of the baseline is a plane sweep
that shifts plane n by t * d_n (W - 1) / W pixels.  t = 1 is the right view the training forward renders (`p_im0`) and its disparity is
the reference's commented-out `dispr` (models/FAL_netB.py:275-277, Test_KITTI.py:190-194); t = 0 gives back the left image and the
forward's `disp`; 0 < t < 1 are the views between the cameras, t > 1 and t < 0 the ones beyond them (|t| <= 2).

  sweep(dlog0, left, min_disp, max_disp, baselines)      the raw wrapper of falnet_med_sweep_fwd (launches of at most 8 views)
  render(model, left, min_disp, max_disp, baselines)     one no_grad disparity-only forward of the model, then the sweep over its logits
  right_disparity(model, left, min_disp, max_disp)       the t = 1 disparity alone

There is no host fallback: CUDA tensors only."""
import ctypes
import math

import torch

from . import _lib as L
from . import med_logits as M
from .med_logits import MAX_PLANES  # noqa: F401  (part of this module's interface)

MAX_VIEWS = 8      # views per launch (SW_MAXV of csrc/med_sweep.hip)
MAX_ABS_T = 2.0    # the library refuses |t| above this


def check_baselines(baselines):
    """The baseline fractions as a list of floats; ValueError on what the library would refuse (none, a non-finite one, |t| > 2)."""
    ts = [float(t) for t in baselines]
    if not ts:
        raise ValueError("views: no baseline fraction given")
    bad = [t for t in ts if not math.isfinite(t) or abs(t) > MAX_ABS_T]
    if bad:
        raise ValueError("views: baseline fraction(s) {} are not finite values in [-{}, {}]".format(bad, MAX_ABS_T, MAX_ABS_T))
    return ts


def sweep(dlog0, left, min_disp, max_disp, baselines, want_views=True, want_disps=True):
    """dlog0 (B, N, H, W) planar f32 logits, left (B, 3, H, W), min_disp / max_disp: B values in pixels, baselines: any number of fractions.
    -> (views (B, V, 3, H, W) or None, disps (B, V, 1, H, W) or None).  Every argument is checked before the first launch."""
    ts = check_baselines(baselines)
    if not (want_views or want_disps):
        raise ValueError("views.sweep: neither views nor disparities requested")
    (dlog0, left, mn, mx), (B, N, H, W) = M.check_logits("views.sweep", dlog0, min_disp, max_disp, left, with_left=True)
    V = len(ts)
    dev = dlog0.device
    views = torch.empty(B, V, 3, H, W, dtype=torch.float32, device=dev) if want_views else None
    disps = torch.empty(B, V, 1, H, W, dtype=torch.float32, device=dev) if want_disps else None
    lib, st = L.lib(), L.stream_ptr()

    def launch(part, bufs):
        t_host = (ctypes.c_float * len(part))(*part)
        L.check(lib.falnet_med_sweep_fwd(L.ptr(dlog0), L.ptr(left), L.ptr(mn), L.ptr(mx), ctypes.cast(t_host, ctypes.c_void_p), len(part),
                                         L.ptr(bufs[0]), L.ptr(bufs[1]), B, N, H, W, st), "med_sweep_fwd")
    M.launch_in_parts(ts, MAX_VIEWS, (views, disps), launch)
    return views, disps


def render(model, left, min_disp, max_disp, baselines, want_views=True, want_disps=True):
    """One no_grad disparity-only forward of `model` (FAL_netA / B / C, any compute dtype: the logits are planar f32 in all of them), then
    the sweep over the plan's own logits with the plan's prologue-processed min_disp / max_disp.  -> (views, disps, disp): as sweep(), plus
    the forward's disparity (B, 1, H, W)."""
    ts = check_baselines(baselines)
    if not (want_views or want_disps):
        raise ValueError("views.render: neither views nor disparities requested")
    with torch.no_grad():
        buf, disp = M.forward_logits(model, left, min_disp, max_disp)
        views, disps = sweep(buf["dlog0"], buf["left"], buf["min_disp"], buf["max_disp"], ts, want_views, want_disps)
    return views, disps, disp


def right_disparity(model, left, min_disp, max_disp):
    """The disparity in the right view's own frame (B, 1, H, W), in pixels of the full baseline: the reference's `dispr`."""
    return render(model, left, min_disp, max_disp, (1.0,), want_views=False)[1][:, 0]

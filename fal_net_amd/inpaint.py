"""Hole filling of a premultiplied image on the device: background-biased pull-push (csrc/inpaint.hip; inference only, no gradient).

`values` is a colour premultiplied by its own `weight` in [0, 1] -- what freeview.warp returns as `view` and `cover` -- and the result is the
un-premultiplied, fully weighted image: pixels of weight 1 come back bit for bit, the others are completed from a pyramid of normalised
convolutions, every hole size in one pass.  With beta > 0 and a `guide` (a disparity), what is filled in is taken from where the guide is SMALL,
the background: every kept pixel enters with the factor g = exp(-beta guide / guide_scale), in the pull as a weight of every sum and in the push
as the mean g of what a coarse cell holds.  The definition, restated: include/falnet_hip.h (falnet_inpaint_fwd); float64: tests/_inpaint_ref.py.

  levels(H, W)                          the number of pulls L of an H x W image
  workspace_bytes(C, H, W, images)      the size of the workspace a call needs
  fill(values, weight, guide, guide_scale, beta, floor, workspace)

There is no host fallback: CUDA tensors only."""
import math

import torch

from . import _lib as L

MAX_CHANNELS = 4
MAX_BETA = 8.0
MAX_PLANE = 1 << 30
FLOOR = 2.0 ** -10


def _check_shape(C, H, W, images):
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError("inpaint: C={} outside [1, {}]".format(C, MAX_CHANNELS))
    if min(H, W, images) < 1:
        raise ValueError("inpaint: empty shape images={} H={} W={}".format(images, H, W))
    if H * W > MAX_PLANE:
        raise ValueError("inpaint: H={} W={}: a plane of more than 2^30 pixels".format(H, W))


def _pyramid_cells(H, W):
    """The cells of levels 1..L together (the host's own count: fill checks a workspace before anything touches the device)."""
    n = 0
    while (H, W) != (1, 1):
        H, W = (H + 1) // 2, (W + 1) // 2
        n += H * W
    return n


def levels(H, W):
    """L: the number of pulls from H x W down to 1 x 1 (sizes halve rounding up)."""
    _check_shape(1, H, W, 1)
    return int(L.lib().falnet_inpaint_levels(int(H), int(W)))


def workspace_bytes(C, H, W, images=1):
    """Bytes of the workspace of one call: pyramid levels 1..L of C + 2 channels for every image."""
    _check_shape(C, H, W, images)
    return int(L.lib().falnet_inpaint_workspace_bytes(int(C), int(H), int(W), int(images)))


def check_params(beta, floor):
    """(beta, floor) as floats; ValueError on what the library would refuse."""
    beta, floor = float(beta), float(floor)
    if not (math.isfinite(beta) and 0.0 <= beta <= MAX_BETA):
        raise ValueError("inpaint: beta={} outside [0, {}]".format(beta, MAX_BETA))
    if not 0.0 < floor <= 1.0:
        raise ValueError("inpaint: floor={} outside (0, 1]".format(floor))
    return beta, floor


def _f32(x, what):
    if not torch.is_tensor(x):
        raise ValueError("inpaint.fill: {} must be a tensor".format(what))
    if not x.is_cuda:
        raise RuntimeError("fal_net_amd.inpaint runs on an MI355X only (no CPU fallback); {} is on {}".format(what, x.device))
    return x.detach().to(torch.float32).contiguous()


def fill(values, weight, guide=None, guide_scale=None, beta=0.0, floor=FLOOR, workspace=None):
    """values (..., C, H, W) premultiplied, 1 <= C <= 4; weight (..., 1, H, W) or (..., H, W) in [0, 1]; guide like weight, or None;
    guide_scale: a positive scalar or one value per image (numbers, or a tensor, whose values are taken as they are); beta in [0, 8] (0: no
    bias, guide is never read); floor in (0, 1]: a pixel of smaller weight counts as empty; workspace: a float32 CUDA tensor of at least
    workspace_bytes(C, H, W, images) bytes, or None (one is allocated).  Leading dimensions of any rank are folded into the images of ONE call.
    -> the filled image, shaped like values.  Every argument is checked before the first launch."""
    beta, floor = check_params(beta, floor)
    if not torch.is_tensor(values) or values.dim() < 3:
        raise ValueError("inpaint.fill: values must be a tensor (..., C, H, W)")
    lead, (C, H, W) = tuple(values.shape[:-3]), values.shape[-3:]
    images = 1
    for d in lead:
        images *= d
    _check_shape(C, H, W, images)

    def plane(t, what):
        if not torch.is_tensor(t) or tuple(t.shape) not in (lead + (1, H, W), lead + (H, W)):
            raise ValueError("inpaint.fill: {} must be {} or {}, got {}".format(what, lead + (1, H, W), lead + (H, W),
                                                                                 tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        return t
    plane(weight, "weight")
    if beta > 0.0:
        if guide is None or guide_scale is None:
            raise ValueError("inpaint.fill: beta={} > 0 needs guide and guide_scale".format(beta))
        plane(guide, "guide")
        if torch.is_tensor(guide_scale):
            if guide_scale.numel() not in (1, images):
                raise ValueError("inpaint.fill: guide_scale must hold one value, or one per image ({}), got {}".format(images, guide_scale.numel()))
        else:
            host = [float(s) for s in (guide_scale if isinstance(guide_scale, (list, tuple)) else [guide_scale])]
            if len(host) not in (1, images) or not all(math.isfinite(s) and s > 0.0 for s in host):
                raise ValueError("inpaint.fill: guide_scale must be positive and finite, one value or one per image ({}), got {}".format(images, host))
    need = 4 * images * (C + 2) * _pyramid_cells(H, W)
    if workspace is not None:
        if not torch.is_tensor(workspace) or workspace.dtype != torch.float32 or not workspace.is_contiguous():
            raise ValueError("inpaint.fill: workspace must be a contiguous float32 tensor")
        if workspace.numel() * 4 < need:
            raise ValueError("inpaint.fill: workspace of {} bytes, {} needed".format(workspace.numel() * 4, need))
    values, weight = _f32(values, "values"), _f32(weight, "weight")
    dev = values.device
    gd = gs = None
    if beta > 0.0:
        gd = _f32(guide, "guide")
        if torch.is_tensor(guide_scale):
            gs = _f32(guide_scale, "guide_scale").reshape(-1).expand(images).contiguous()
        else:
            gs = torch.tensor(host * (images if len(host) == 1 else 1), dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev)
    elif workspace.device != dev:
        raise RuntimeError("inpaint.fill: the workspace is on {}, values on {}".format(workspace.device, dev))
    out = torch.empty_like(values)
    L.check(L.lib().falnet_inpaint_fwd(L.ptr(values), L.ptr(weight), L.ptr(gd), L.ptr(gs), beta, floor, L.ptr(out), L.ptr(workspace),
                                       workspace.numel() * 4, images, C, H, W, L.stream_ptr()), "inpaint_fwd")
    return out

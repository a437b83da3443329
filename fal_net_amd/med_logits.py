"""What the readers of the MED head's logits share (views, freeview, confidence): the plane limit, the argument checks, the split of a
long list of views into launches, and the disparity-only forward that leaves the logits in the plan's buffers.  `who` is the calling
module's or function's name as it stands in the messages."""
import torch

MAX_PLANES = 128   # MED_MAXN of csrc/med_planes.h


def f32(x, what, who):
    """x as a contiguous f32 tensor; RuntimeError unless it is on the device.  who: the module's name."""
    if not x.is_cuda:
        raise RuntimeError("fal_net_amd.{} runs on an MI355X only (no CPU fallback); {} is on {}".format(who, what, x.device))
    return x.detach().to(torch.float32).contiguous()


def check_logits(who, dlog0, min_disp, max_disp, left=None, with_left=False):
    """The checks of dlog0 (B, N, H, W), left (B, 3, H, W) where the caller takes one, and min_disp / max_disp (B values each), in the
    order ValueError on shapes, then RuntimeError on a host tensor.  who: "module.function".
    -> (dlog0, left or None, min_disp, max_disp) as contiguous f32, (B, N, H, W)."""
    if with_left and (dlog0.dim() != 4 or left.dim() != 4):
        raise ValueError("{}: expected dlog0 (B, N, H, W) and left (B, 3, H, W), got {} and {}".format(who, tuple(dlog0.shape), tuple(left.shape)))
    if dlog0.dim() != 4:
        raise ValueError("{}: expected dlog0 (B, N, H, W), got {}".format(who, tuple(dlog0.shape)))
    B, N, H, W = dlog0.shape
    if not 2 <= N <= MAX_PLANES:
        raise ValueError("{}: N={} outside [2, {}]".format(who, N, MAX_PLANES))
    if with_left and (tuple(left.shape) != (B, 3, H, W) or min(B, H, W) < 1):
        raise ValueError("{}: left {} does not match the logits {}".format(who, tuple(left.shape), tuple(dlog0.shape)))
    if min(B, H, W) < 1:
        raise ValueError("{}: empty logits {}".format(who, tuple(dlog0.shape)))
    if min_disp.numel() != B or max_disp.numel() != B:
        raise ValueError("{}: min_disp / max_disp must hold one value per sample (B={})".format(who, B))
    mod = who.split(".")[0]
    dlog0 = f32(dlog0, "dlog0", mod)
    left = f32(left, "left", mod) if with_left else None
    return (dlog0, left, f32(min_disp, "min_disp", mod).reshape(-1), f32(max_disp, "max_disp", mod).reshape(-1)), (B, N, H, W)


def launch_in_parts(items, limit, outs, launch):
    """One launch per `limit` items.  outs: a tuple or a dict of result tensors (B, V, ...), V = len(items), entries may be None;
    launch(part, bufs) writes the items `part` densely into bufs, which has the form of outs with (B, len(part), ...) tensors: the
    results themselves when one launch takes every item, else fresh parts that are then copied into their slices."""
    named = outs if isinstance(outs, dict) else dict(enumerate(outs))
    V = len(items)
    for v0 in range(0, V, limit):
        part = items[v0:v0 + limit]
        n = len(part)
        whole = n == V
        bufs = {k: t if whole or t is None else t.new_empty((t.shape[0], n) + tuple(t.shape[2:])) for k, t in named.items()}
        launch(part, bufs if isinstance(outs, dict) else tuple(bufs.values()))
        if not whole:
            for k, t in named.items():
                if t is not None:
                    t[:, v0:v0 + n].copy_(bufs[k])


def forward_logits(model, left, min_disp, max_disp):
    """One disparity-only forward of `model` (FAL_netA / B / C, any compute dtype: the logits are planar f32 in all of them) -> (buf, disp):
    the buffers of the plan this forward has just run -- "dlog0", "left" and the prologue-processed "min_disp" / "max_disp", valid until
    the next forward -- and the forward's disparity (B, 1, H, W).  Call it under torch.no_grad()."""
    disp = model(left, min_disp, max_disp, ret_disp=True, ret_subocc=False, ret_pan=False)
    B, _, H, W = left.shape
    return model._plan(B, H, W, left.device).buf, disp

"""GPU parity at the BENCHMARK's own configurations (BASELINE configs[1] / configs[3]: B = 8, 256 x 512, N = 49; configs[4]: 384 x 1280,
N = 96, f16).

`bench.py` picks its kernels from the B-keyed entries of the committed autotune cache (`...|B8|...`: the persistent LDS-DMA /
weight-stationary variants on shapes no small test launches at that batch), so this module runs exactly those launches and holds
them to the CPU oracle (f32, the 1e-4 gate of north_star) and the 16-bit paths to the f32 HIP step (reported, bounded loosely:
the reference is f32-only).  Reference: Train_Stage1_K.py:233-262, Train_Stage2_K.py:233-331."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402
from oracle import falnet_oracle as O  # noqa: E402

from _grad_parity import grad_parity  # noqa: E402

DEV = "cuda"
TOL = 1e-4
B, H, W, N = 8, 256, 512, 49
_F32 = {}


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _build(dtype, train_mode=True, n=N):
    LF.set_compute_dtype(dtype)
    m = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(n)}, no_levels=n, compute_dtype=dtype).to(DEV)
    return m.train() if train_mode else m.eval()


def _stage1(dtype, shape=(B, H, W, N)):
    b, h, w, n = shape
    left, right, mn, mx = synthetic.synthetic_pair(b, h, w, seed=1234)  # bench.py's rank-0 batch
    m = _build(dtype, n=n)
    out = train.stage1_step(m, train.FlatAdam(m), left.to(DEV), right.to(DEV), mx.to(DEV), optimize=False)
    inv = 1.0 / float(out["scaler"].state[0]) if out.get("scaler") is not None else 1.0  # f16: the raw gradients carry the loss scale
    res = {"loss": float(out["loss"]), "rec": float(out["rec"]), "sm": float(out["sm"]), "ldisp": out["ldisp"].clone().cpu(),
           "rpan": out["rpan"].clone().cpu(), "flat_grad": m.flat_gradients().clone() * inv,
           "grads": {k: p.grad.detach().float().cpu() * inv for k, p in m.named_parameters() if p.grad is not None},
           "gnorm": {k: float(p.grad.norm()) * inv for k, p in m.named_parameters() if p.grad is not None}}
    del m
    LF.set_compute_dtype(torch.float32)
    return res


def _f32_stage1():
    if "s1" not in _F32:
        _F32["s1"] = _stage1(torch.float32)
    return _F32["s1"]


_O64 = {}


def _oracle64(shape, stage2=False, chunk=2):
    """The oracle's step on the inputs of _stage1 / _stage2 in FLOAT64 (weights, VGG, images): no f32 summation noise on the reference side.
    Run in chunks of `chunk` samples: every loss term is a batch mean, so the losses are averaged and the gradients summed with the chunk's
    share of the batch as weight.  Computed once per module and shape."""
    key = ("s2" if stage2 else "s1",) + tuple(shape)
    if key in _O64:
        return _O64[key]
    b, h, w, n = shape
    left, right, mn, mx = (t.double() for t in synthetic.synthetic_pair(b, h, w, seed=1234))
    sd = {k: v.double() for k, v in synthetic.seeded_falnetb_state_dict(n).items()}
    vsd = {k: v.double() for k, v in synthetic.seeded_vgg19_state_dict().items()}
    params = O.leaf_params(sd)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    names = ("loss", "rec", "sm", "mirror") if stage2 else ("loss", "rec", "sm")
    maps = ("ldisp", "rdisp", "O_L", "O_R") if stage2 else ("ldisp", "rpan")
    res = {k: 0.0 for k in names}
    parts = {k: [] for k in maps}
    for i in range(0, b, chunk):
        sl = slice(i, min(b, i + chunk))
        wgt = (sl.stop - sl.start) / b
        if stage2:
            out = O.stage2_losses(params, sd, vsd, left[sl], right[sl], mn[sl], mx[sl])
        else:
            out = O.stage1_losses(params, vsd, left[sl], right[sl], mn[sl], mx[sl])
        (out["loss"] * wgt).backward()
        for k in names:
            res[k] += float(out[k]) * wgt
        for k in maps:
            parts[k].append(out[k].detach())
        del out
    res.update({k: torch.cat(v, 0) for k, v in parts.items()})
    res["grads"] = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
    _O64[key] = res
    return res


def _f32_det(shape, tmp_path_factory, stage2=False):
    """The f32 HIP step of `shape` from a fresh process in deterministic mode (tests/_f32_det_step.py): no atomics-order noise on the f32 side."""
    key = ("det2" if stage2 else "det",) + tuple(shape)
    if key not in _F32:
        out = str(tmp_path_factory.mktemp("f32det") / "step.pt")
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_f32_det_step.py")] + [str(v) for v in shape] + [out] +
                           (["stage2"] if stage2 else []), capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _F32[key] = torch.load(out)
    return _F32[key]


# Per-TENSOR bounds of a 16-bit step against the deterministic f32 HIP step at the benchmark's own batch (a wrong border
# tile or a dropped K slice in ONE launch moves one layer's gradient, not the flat cosine): gradient norm within 3 % (bf16) / 0.5 % (f16),
# cosine >= 0.999 for every parameter tensor.
NORM_TOL = {torch.bfloat16: 3e-2, torch.float16: 5e-3}
COS_MIN = 0.999


def _compare_16bit(ref, got, dt, what, loss_tol=2e-2, disp_tol=None):
    lrel = abs(got["loss"] - ref["loss"]) / ref["loss"]
    drel = rel(got["ldisp"], ref["ldisp"])
    cos_flat = float(torch.nn.functional.cosine_similarity(got["flat_grad"].double().cpu(), ref["flat_grad"].double().cpu(), dim=0))
    rows = []
    for k, g in got["grads"].items():
        r = ref["grads"][k].double().reshape(-1)
        g = g.double().reshape(-1)
        rows.append((k, abs(float(g.norm()) - float(r.norm())) / float(r.norm()), float(torch.nn.functional.cosine_similarity(g, r, dim=0)), g.numel()))
    wn, wc = max(rows, key=lambda t: t[1]), min(rows, key=lambda t: t[2])
    print(f"{what} {dt} vs deterministic f32 HIP: loss rel {lrel:.2e}, disp max-rel {drel:.2e}, flat grad cosine {cos_flat:.6f}, "
          f"worst grad-norm rel {wn[0]} {wn[1]:.2e}, worst per-tensor cosine {wc[0]} {wc[2]:.6f}")
    bad = [t for t in rows if t[1] > NORM_TOL[dt] or t[2] < COS_MIN]
    for t in sorted(rows, key=lambda t: -t[1])[:6]:
        print(f"    norm dev {t[1]:.2e}  cosine {t[2]:.6f}  numel {t[3]:8d}  {t[0]}")
    assert torch.isfinite(got["flat_grad"]).all()
    assert lrel < loss_tol and cos_flat > 0.9995
    assert drel < (disp_tol or (1e-1 if dt == torch.bfloat16 else 2e-2))
    assert not bad, bad
    return rows


def _compare_16bit_vs_oracle(oref, got, dt, what):
    """The same per-tensor bounds (NORM_TOL / COS_MIN) against the float64 oracle's gradients of the same inputs."""
    bad, worst = [], ("", 0.0, 1.0)
    for k, g in got["grads"].items():
        r = oref["grads"][k].double().reshape(-1)
        g = g.double().reshape(-1)
        nd = abs(float(g.norm()) - float(r.norm())) / float(r.norm())
        cos = float(torch.nn.functional.cosine_similarity(g, r, dim=0))
        worst = (k, max(worst[1], nd), min(worst[2], cos))
        if nd > NORM_TOL[dt] or cos < COS_MIN:
            bad.append((k, nd, cos))
    print(f"{what} {dt} vs float64 oracle: worst grad-norm dev {worst[1]:.2e}, worst per-tensor cosine {worst[2]:.6f}")
    assert not bad, bad


def _check_vs_oracle(hip, shape, what):
    ref = _oracle64(shape, chunk=1 if shape[1] * shape[2] > H * W else 2)  # float64, gradients summed over chunks of the batch
    for k in ("loss", "rec", "sm"):
        assert abs(hip[k] - float(ref[k])) / abs(float(ref[k])) < TOL, (k, hip[k], float(ref[k]))
    assert rel(hip["ldisp"], ref["ldisp"]) < TOL
    assert rel(hip["rpan"], ref["rpan"]) < 2e-4
    worst = ("", 0.0)
    for k, gn in hip["gnorm"].items():
        g = ref["grads"].get(k)
        if g is None:
            continue
        e = abs(gn - float(g.norm())) / float(g.norm())
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < 2e-3, (k, gn, float(g.norm()))
    print(what, "f32 vs float64 oracle: worst gradient-norm deviation", worst)
    # element-wise: a norm is blind to swapped taps, flipped signs, permuted channels, misplaced tiles
    grad_parity({k: g for k, g in hip["grads"].items() if k in ref["grads"]}, ref["grads"], norm_tol=2e-3, what=f"{what} f32")


def test_stage1_b8_f32_vs_oracle():
    """One Stage-1 step at B=8, 256x512, N=49 in f32 against the float64 CPU oracle: loss scalars and disparity 1e-4, synthesised view
    2e-4 (the reference's own fp32 grid noise), every parameter's gradient norm 2e-3 and element-wise (grad_parity)."""
    _check_vs_oracle(_f32_stage1(), (B, H, W, N), "B=8 256x512 N=49")


def test_stage1_default_training_crop_f32_vs_oracle():
    """The reference's DEFAULT training crop, 192 x 640 (Train_Stage1_K.py:48-49 --crop_height 192 --crop_width 640; the benchmark's 256 x 512 is
    BASELINE's shape, not the script's): one f32 Stage-1 step at B=2 against the CPU oracle, same bounds as the configs[1] test."""
    shape = (2, 192, 640, N)
    _check_vs_oracle(_stage1(torch.float32, shape), shape, "B=2 192x640 N=49")


HIGHRES = (384, 1280, 96)  # BASELINE configs[4]


def test_highres_b1_f32_step_vs_oracle():
    """BASELINE configs[4]'s shape, forward AND backward: one Stage-1 step at 384x1280, N=96 (B=1: the oracle's step is ~1.6 TFLOP per pair)
    in f32 against the CPU oracle, same bounds as the configs[1] test.  The MED head runs on the 512-thread strided kernels here
    (tests/test_gpu_ops.py::test_med_head_cases_cover_every_head_kernel names them).  Reference: FAL_netB.py:200-297, Train_Stage1_K.py:233-262."""
    shape = (1,) + HIGHRES
    _check_vs_oracle(_stage1(torch.float32, shape), shape, "B=1 384x1280 N=96")


def test_highres_b8_f32_vs_oracle():
    """configs[4]'s shape at the benchmark's own batch, B=8, 384x1280, N=96, f32 (the `...|B8|...` entries of `bench.py --workload highres`)
    against the float64 oracle run one sample at a time: the bounds of the B=8 256x512 test, gradients element-wise (grad_parity)."""
    shape = (8,) + HIGHRES
    _check_vs_oracle(_stage1(torch.float32, shape), shape, "B=8 384x1280 N=96")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_highres_b8_16bit_vs_f32_hip(dt, tmp_path_factory):
    """configs[4] at the benchmark's own batch (the `...|B8|...` autotune entries of `bench.py --workload highres`, the wave-neighbour
    16-bit head backward): f16 (its dtype) and bf16 against the deterministic f32 HIP step of the same inputs (the f32 path is held to the
    oracle at B=1 above), per parameter tensor (NORM_TOL / COS_MIN)."""
    shape = (8,) + HIGHRES
    got = _stage1(dt, shape)
    _compare_16bit(_f32_det(shape, tmp_path_factory), got, dt, "highres B=8")
    _compare_16bit_vs_oracle(_oracle64(shape, chunk=1), got, dt, "highres B=8")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_stage1_b8_16bit_vs_f32_hip(dt, tmp_path_factory):
    """The benchmark's own dtype (bf16) and f16 at the benchmark's own batch -- the LDS-DMA / weight-stationary / row-streaming 16-bit kernels
    `bench.py` runs -- against the deterministic f32 HIP step of the same inputs, per parameter tensor: gradient norm within 3 % (bf16) /
    0.5 % (f16) and cosine >= 0.999 for EVERY tensor (NORM_TOL / COS_MIN)."""
    got = _stage1(dt)
    _compare_16bit(_f32_det((B, H, W, N), tmp_path_factory), got, dt, "B=8 256x512")
    _compare_16bit_vs_oracle(_oracle64((B, H, W, N)), got, dt, "B=8 256x512")


def _stage2(dtype):
    left, right, mn, mx = synthetic.synthetic_pair(B, H, W, seed=1234)
    m, fix = _build(dtype), _build(dtype, train_mode=False)
    for q in fix.parameters():
        q.requires_grad_(False)
    out = train.stage2_step(m, fix, train.FlatAdam(m, lr=5e-5), left.to(DEV), right.to(DEV), mx.to(DEV))
    inv = 1.0 / float(out["scaler"].state[0]) if out.get("scaler") is not None else 1.0  # f16: the raw gradients carry the loss scale
    res = {k: float(out[k]) for k in ("loss", "rec", "sm", "mirror")}
    res.update(ldisp=out["ldisp"].detach().clone().cpu(), rdisp=out["rdisp"].detach().clone().cpu(),
               O_L=out["O_L"].detach().clone().cpu(), O_R=out["O_R"].detach().clone().cpu(), flat_grad=m.flat_gradients().clone() * inv,
               grads={k: p.grad.detach().float().cpu() * inv for k, p in m.named_parameters() if p.grad is not None})
    del m, fix
    LF.set_compute_dtype(torch.float32)
    return res


def test_stage2_b8_f32_vs_oracle():
    """Stage-2 (BASELINE configs[3]) f32 at the benchmark's batch, B=8, 256x512, N=49 -- the `...|B8|...` cache entries of the 2B-batch plans --
    against the float64 oracle (run in chunks of two samples): loss scalars and both disparities 1e-4, occlusion masks 2e-4 (as at B=2), every
    gradient element-wise (grad_parity)."""
    got, ref = _stage2(torch.float32), _oracle64((B, H, W, N), stage2=True)
    for k in ("loss", "rec", "sm", "mirror"):
        assert abs(got[k] - ref[k]) / abs(ref[k]) < TOL, (k, got[k], ref[k])
    for k in ("O_L", "O_R"):
        assert rel(got[k], ref[k]) < 2e-4, (k, rel(got[k], ref[k]))
    for k in ("ldisp", "rdisp"):
        assert rel(got[k], ref[k]) < TOL, (k, rel(got[k], ref[k]))
    grad_parity(got["grads"], ref["grads"], norm_tol=2e-3, what="Stage-2 B=8 256x512 f32")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_stage2_b8_16bit_vs_f32_hip(dt, tmp_path_factory):
    """Stage-2 (BASELINE configs[3]) at B=8/GPU, held to Stage-1's standard: the 16-bit steps against the DETERMINISTIC f32 HIP
    Stage-2 step of the same inputs (itself pinned to the oracle at 256x512 B=2 by tests/test_gpu_step.py::test_stage2_step_256x512_vs_oracle and
    to the reference by golden G3), per parameter tensor -- gradient norm within 3 % (bf16) / 0.5 % (f16), cosine >= 0.999 -- so a dropped K slice
    in one Stage-2-only launch (the 2B-batch plans, falnet_mask_mix, the mirror loss's adjoint) cannot hide in a flat cosine; `rec`, `sm`, `mirror`
    and the total are all asserted.  Reference: Train_Stage2_K.py:267-331."""
    ref, got = _f32_det((B, H, W, N), tmp_path_factory, stage2=True), _stage2(dt)
    dev = {k: abs(got[k] - ref[k]) / abs(ref[k]) for k in ("loss", "rec", "sm", "mirror")}
    print(f"Stage-2 B=8 {dt} vs deterministic f32 HIP: {dev}, rdisp {rel(got['rdisp'], ref['rdisp']):.2e}")
    _compare_16bit(ref, got, dt, "Stage-2 B=8", loss_tol=3e-2, disp_tol=1.5e-1 if dt == torch.bfloat16 else 3e-2)
    _compare_16bit_vs_oracle(_oracle64((B, H, W, N), stage2=True), got, dt, "Stage-2 B=8")
    tol = 3e-2 if dt == torch.bfloat16 else 1e-2
    assert dev["rec"] < tol and dev["sm"] < tol and dev["mirror"] < tol, dev
    assert rel(got["rdisp"], ref["rdisp"]) < (1.5e-1 if dt == torch.bfloat16 else 3e-2)

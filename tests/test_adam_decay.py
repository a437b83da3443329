"""CPU: host side of weight decay / bias decay in the fused Adam (train.FlatAdam, the training scripts) -- no device is touched.
The kernels are held to a float64 torch.optim.Adam in tests/test_gpu_adam_decay.py."""
import importlib
import os

import pytest
import torch

from fal_net_amd import train
from fal_net_amd.models import FAL_netB

import _adam_decay_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_flat_adam_accepts_and_stores_both_decays():
    m = FAL_netB(no_levels=7)
    opt = train.FlatAdam(m, lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-2, bias_decay=3e-3)
    assert (opt.weight_decay, opt.bias_decay) == (1e-2, 3e-3)
    assert opt.param_groups[0]["lr"] == 2e-4 and opt.t == 0 and opt.m is None and opt.v is None
    assert m.flat_parameters() is None and all(not p.is_cuda for p in m.parameters())  # nothing was moved or allocated
    d = train.FlatAdam(m)
    assert (d.weight_decay, d.bias_decay) == (0.0, 0.0)
    with pytest.raises(ValueError):
        train.FlatAdam(m, weight_decay=-1e-4)


def test_training_script_offers_both_flags_and_no_longer_refuses_them():
    src = open(os.path.join(ROOT, "Train_Stage1_K.py")).read()
    assert "wd=0 only" not in src and "implements wd" not in src
    assert "weight_decay=args.weight_decay" in src and "bias_decay=args.bias_decay" in src
    mod = importlib.import_module("Train_Stage1_K")
    a = mod.parser.parse_args([])
    assert a.weight_decay == 0.0 and a.bias_decay == 0.0
    a = mod.parser.parse_args(["--weight-decay", "1e-4", "--bias-decay", "1e-5"])
    assert a.weight_decay == 1e-4 and a.bias_decay == 1e-5
    assert mod.parser.parse_args(["--wd", "2e-4"]).weight_decay == 2e-4


def test_state_dict_round_trip_of_a_never_stepped_optimiser():
    m = FAL_netB(no_levels=7)
    opt = train.FlatAdam(m, weight_decay=1e-2, bias_decay=3e-3)
    sd = opt.state_dict()
    assert set(sd) == {"t", "m", "v", "weight_decay", "bias_decay", "layout"}
    assert sd["t"] == 0 and sd["m"] is None and sd["v"] is None and sd["layout"] is None
    other = train.FlatAdam(FAL_netB(no_levels=7))
    other.load_state_dict(sd)
    assert (other.weight_decay, other.bias_decay, other.t, other.m, other.v) == (1e-2, 3e-3, 0, None, None)
    assert other.state_dict() == sd


def test_layout_names_every_trainable_parameter_and_guards_the_load():
    """The saved layout is name -> (offset, numel) in the flat buffer; a model of another no_levels has another one and is refused."""
    m = FAL_netB(no_levels=7)
    m.ensure_flat()
    opt = train.FlatAdam(m, weight_decay=1e-2)
    sd = opt.state_dict()
    names = [n for n, _ in m.named_parameters() if "amask_conv" not in n]
    assert list(sd["layout"]) == names and all("amask_conv" not in n for n in sd["layout"])
    for (n, p), (off, numel) in zip(m._trainable_named(), sd["layout"].values()):
        assert off % 4 == 0 and numel == p.numel()
    m9 = FAL_netB(no_levels=9)
    with pytest.raises(ValueError, match="layout"):
        train.FlatAdam(m9).load_state_dict(sd)
    with pytest.raises(ValueError):
        train.FlatAdam(FAL_netB(no_levels=7)).load_state_dict(dict(sd, m=torch.zeros(8), v=None))


def test_decay_segments_tile_the_flat_buffer_by_kind():
    """One segment per parameter slice, padding included, biases told from weights by name (the reference's bias_parameters() /
    weight_parameters()): what plan.py cuts the range list by and what the stand-alone decayed kernel looks its decay up in."""
    m = FAL_netB(no_levels=7)
    flat = m.ensure_flat()
    segs = m.decay_segments()
    named = m._trainable_named()
    assert len(segs) == len(named)
    pos = 0
    for (off, cnt, is_bias), (n, p) in zip(segs, named):
        assert off == pos and off % 4 == 0 and cnt % 4 == 0 and p.numel() <= cnt < p.numel() + 4
        assert is_bias == ("bias" in n) and is_bias != ("weight" in n)
        pos += cnt
    assert pos == flat.numel()


def test_bound_holds_for_f32_adam_and_sees_the_decay():
    """The tolerance of the GPU tests on the CPU: torch's own f32 Adam standing in for the device against the float64 reference (4 tensors,
    decays 1e-2 / 3e-3, |p| ~ 0.1, |g| ~ 1e-3 changing in size and sign every step, lr 1e-4, K = 5)."""
    g = torch.Generator().manual_seed(11)
    named = {"a.weight": torch.randn(10007, generator=g) * 0.1, "a.bias": torch.randn(33, generator=g) * 0.1,
             "b.weight": torch.randn(4096, generator=g) * 0.1, "b.bias": torch.randn(7, generator=g) * 0.1}
    lr, K, wd, bd = 1e-4, 5, 1e-2, 3e-3
    ref, ref0 = R.RefAdam64(named, lr=lr, weight_decay=wd, bias_decay=bd), R.RefAdam64(named, lr=lr)
    p32 = {k: torch.nn.Parameter(v.clone()) for k, v in named.items()}
    opt32 = torch.optim.Adam([{"params": [p for k, p in p32.items() if "bias" in k], "weight_decay": bd},
                              {"params": [p for k, p in p32.items() if "weight" in k], "weight_decay": wd}], lr=lr, betas=(0.5, 0.999), eps=1e-8)
    for s in range(K):
        grads = {k: torch.randn(v.shape, generator=g) * 1e-3 * (1 + s) * (-1) ** s for k, v in named.items()}
        ref.step(grads)
        ref0.step(grads)
        for k, p in p32.items():
            p.grad = grads[k].clone()
        opt32.step()
    for k in named:
        R.check(p32[k], ref.p[k].detach(), K, lr, k)
        R.check_decay_seen(p32[k], ref0.p[k].detach(), K, lr, k)


def test_f32_decayed_gradient_leaves_the_bound_at_scale_and_the_double_form_does_not():
    """Why the kernels form g + decay * p in double (csrc/adam.h: AdamGradL2) and the decays travel as doubles: 2 M elements, one step,
    gradients spread over several decades.  At the few elements per million where g and decay * p cancel, |gr| falls towards eps while an f32
    sum carries an error of 2^-24 |g|, and the first step lr * gr / (|gr| + eps) amplifies it by lr / eps: torch's own f32 Adam lands
    outside the float64 bound (about 10 x here); the kernels' arithmetic -- restated in torch f32 with gr formed in double and rounded
    once -- stays inside.  The small tensors of the test above never meet such an element."""
    g = torch.Generator().manual_seed(1)
    n, lr, b1, b2, eps, wd = 2_000_000, 1e-4, 0.5, 0.999, 1e-8, 1e-2
    p0 = torch.randn(n, generator=g) * 0.05
    grad = torch.randn(n, generator=g) * 1e-3 * torch.rand(n, generator=g) ** 4
    ref = R.RefAdam64({"a.weight": p0}, lr=lr, weight_decay=wd)
    ref.step({"a.weight": grad})
    want = ref.p["a.weight"].detach()
    p32 = torch.nn.Parameter(p0.clone())
    p32.grad = grad.clone()
    torch.optim.Adam([p32], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd).step()
    r32 = float(((p32.detach().double() - want).abs() / R.bound(want, 1, lr)).max())
    gr = (grad.double() + wd * p0.double()).float()  # AdamGradL2: one rounding
    m, v = (1 - b1) * gr, (1 - b2) * gr * gr
    step_size, rsqrt_bc2 = torch.tensor(lr / (1 - b1), dtype=torch.float32), torch.tensor((1 - b2) ** -0.5, dtype=torch.float32)
    dev = p0 - step_size * m / (v.sqrt() * rsqrt_bc2 + eps)
    print(f"adam-decay f32 torch Adam at {n} elements: {r32:.1f} x the bound")
    assert r32 > 1.0
    R.check(dev, want, 1, lr, "double-formed gr")

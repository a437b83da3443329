"""Reference and tolerance of the weight-decay / bias-decay tests (tests/test_adam_decay.py, tests/test_gpu_adam_decay.py).

Reference: torch.optim.Adam on the CPU in float64 with the two param groups of the reference's Train_Stage1_K.py:177-180 -- parameters whose
name contains `bias` with weight_decay = bias_decay, those whose name contains `weight` with weight_decay = weight_decay -- fed the same f32
inputs as the code under test.

Tolerance, per element after K steps:   |p - p_ref64| <= K * 2^-23 * |p_ref64| + K * 16 * lr * 2^-20
  first term: one f32 rounding of p per step, with a factor 2; second: a step is at most about lr * (1 - b1) / sqrt(1 - b2) ~ 16 lr for
  betas (0.5, 0.999), times a few f32 ulps for powf / sqrtf / the division.  Measured on the CPU with torch's own f32 Adam standing in for the
  device (tests/test_adam_decay.py::test_bound_holds_for_f32_adam_and_sees_the_decay): worst element 0.38 of the bound, and
  the decay moves every tensor by more than 1 000 x the bound."""
import torch

ULP_FACTOR = 1  # integer factor on the first term.  Measured on an MI355X over every comparison of test_gpu_adam_decay.py (1 250 tensors):
# worst element 0.452 of the bound, smallest decayed-vs-decay-0 distance 591 x the bound -- the factor stays 1.  It holds because the kernels
# form g + decay * p in double and round once: an f32 sum (torch's own f32 Adam, 2 M elements, K = 1: test_adam_decay.py, last test) lands 10 x outside, at
# the few elements per million where g and decay * p cancel while the second moment is still young.


class RefAdam64:
    """torch.optim.Adam in float64 over {name: f32 tensor}: two groups by name, like the reference builds them."""

    def __init__(self, named, lr=1e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.0, bias_decay=0.0):
        self.p = {k: torch.nn.Parameter(v.detach().cpu().double().clone()) for k, v in named.items()}
        bias = [p for k, p in self.p.items() if "bias" in k]
        weight = [p for k, p in self.p.items() if "weight" in k]
        assert len(bias) + len(weight) == len(self.p)
        groups = [{"params": bias, "weight_decay": bias_decay}, {"params": weight, "weight_decay": weight_decay}]
        self.opt = torch.optim.Adam([g for g in groups if g["params"]], lr=lr, betas=betas, eps=eps)
        self._bias, self._weight = bias, weight
        self.steps = 0

    def set_decays(self, weight_decay, bias_decay):
        for g in self.opt.param_groups:
            g["weight_decay"] = bias_decay if g["params"] and g["params"][0] is self._bias[0] else weight_decay

    def step(self, grads, scale=1.0):
        """grads: {name: f32 tensor}; `scale` multiplies them in float64 (grad_scale, 1 / loss scale)."""
        for k, p in self.p.items():
            p.grad = grads[k].detach().cpu().double().reshape(p.shape) * scale
        self.opt.step()
        self.steps += 1


def bound(p_ref64, K, lr):
    return K * ULP_FACTOR * 2.0 ** -23 * p_ref64.abs() + K * 16 * lr * 2.0 ** -20


def check(got, ref64, K, lr, what=""):
    """Worst |got - ref| / bound over the elements; asserts <= 1 after printing the figure."""
    r = float(((got.detach().cpu().double().reshape(ref64.shape) - ref64).abs() / bound(ref64, K, lr)).max()) if ref64.numel() else 0.0
    print(f"adam-decay {what}: worst |p - p_ref64| / bound = {r:.3f} (K = {K})")
    assert r <= 1.0, (what, r)
    return r


def check_decay_seen(got, ref64_nodecay, K, lr, what=""):
    """The decayed result must differ from the decay-0 run of the same inputs by more than 100 x the bound: a kernel that ignores the decay
    cannot pass."""
    r = float(((got.detach().cpu().double().reshape(ref64_nodecay.shape) - ref64_nodecay).abs() / bound(ref64_nodecay, K, lr)).max())
    print(f"adam-decay {what}: decayed vs decay-0 = {r:.0f} x bound")
    assert r > 100.0, (what, r)
    return r

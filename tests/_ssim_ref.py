"""The definition of SSIM that csrc/ssim.hip is held to, in torch on the CPU (Wang et al. 2004), and the case lists of the SSIM tests.

For a plane pair x, y (H x W) and a window w of radius R -- the outer product of a 1-D weight vector g[0..2R] of sum 1 -- at every VALID window
centre (no padding: (H - 2R) x (W - 2R) positions):
    mx = sum w x, my = sum w y, vx = sum w x^2 - mx^2, vy = sum w y^2 - my^2, cxy = sum w x y - mx my
    n1 = 2 mx my + C1, n2 = 2 cxy + C2, d1 = mx^2 + my^2 + C1, d2 = vx + vy + C2, S = n1 n2 / (d1 d2)
Every function takes a dtype: float64 is the definition, float32 the same formulas as a measure of what f32 rounding alone does to them."""
import torch

MEAN = (0.411, 0.432, 0.45)

METRIC_R, METRIC_SIGMA = 5, 1.5
METRIC_C1, METRIC_C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
LOSS_R = 1
LOSS_C1, LOSS_C2 = 0.01 ** 2, 0.03 ** 2

# (B, H, W) of the metric: one window | crosses a tile column | ragged in both directions, more than one tile row | several tiles each way
METRIC_SHAPES = [(1, 11, 11), (2, 13, 70), (1, 45, 77), (1, 75, 250)]
# (B, C, H, W) of the loss: one window per plane (every pixel a border pixel) | ... | more than one tile each way
LOSS_SHAPES = [(40, 3, 3, 3), (2, 3, 5, 9), (1, 1, 19, 35), (1, 3, 37, 70), (2, 3, 64, 128)]


def gauss_weights(radius=METRIC_R, sigma=METRIC_SIGMA):
    k = torch.arange(2 * radius + 1, dtype=torch.float64) - radius
    g = torch.exp(-k * k / (2.0 * sigma * sigma))
    return g / g.sum()


def box_weights(radius=LOSS_R):
    return torch.full((2 * radius + 1,), 1.0 / (2 * radius + 1), dtype=torch.float64)


def _window(t, g):
    """sum over the window of w * t at every valid position of (..., H, W): (..., H - 2R, W - 2R)."""
    n = len(g)
    H, W = t.shape[-2] - n + 1, t.shape[-1] - n + 1
    out = torch.zeros(t.shape[:-2] + (H, W), dtype=t.dtype)
    for i in range(n):
        for j in range(n):
            out = out + (g[i] * g[j]).to(t.dtype) * t[..., i:i + H, j:j + W]
    return out


def moments(x, y, g):
    mx, my = _window(x, g), _window(y, g)
    return mx, my, _window(x * x, g) - mx * mx, _window(y * y, g) - my * my, _window(x * y, g) - mx * my


def ssim_map(x, y, g, c1, c2):
    mx, my, vx, vy, cxy = moments(x, y, g)
    return (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def _mean_of(t, mean):
    return torch.tensor(mean[:t.shape[1]], dtype=t.dtype).view(1, -1, 1, 1)


# ---- the metric ------------------------------------------------------------------------------------------------------------------------------
def metric_operands(p_im, right, mean=MEAN):
    """get_psnr's operands, formed in f32 as torch forms them (an add, then a multiply, then round half to even), then exact in f64."""
    p_im, right = p_im.detach().float().cpu(), right.detach().float().cpu()
    m = _mean_of(p_im, mean)
    x = torch.round(torch.clamp((p_im + m) * 255, 0, 255))
    y = (right + m) * 255
    return x.double(), y.double()


def metric(p_im, right, mean=MEAN):
    """SSIM of a frame in f64: the mean of S over all B * 3 * (H - 10) * (W - 10) windows."""
    x, y = metric_operands(p_im, right, mean)
    return float(ssim_map(x, y, gauss_weights(), METRIC_C1, METRIC_C2).mean())


# ---- the loss ----------------------------------------------------------------------------------------------------------------------------------
def loss_map(synth, label, mean=MEAN, dtype=torch.float64):
    """(1 - S) / 2 at every window: the 3 x 3 box on x = synth + mean_c, y = label + mean_c."""
    x, y = synth.to(dtype) + _mean_of(synth, mean).to(dtype), label.to(dtype) + _mean_of(label, mean).to(dtype)
    return (1 - ssim_map(x, y, box_weights(), LOSS_C1, LOSS_C2)) / 2


def loss(synth, label, mean=MEAN, dtype=torch.float64):
    return loss_map(synth, label, mean, dtype).mean()


def loss_and_grad(synth, label, mean=MEAN, dtype=torch.float64, upstream=1.0):
    """(map, value, upstream * d value / d synth) by autograd, in `dtype` on the CPU."""
    s = synth.detach().cpu().to(dtype).requires_grad_(True)
    m = loss_map(s, label.detach().cpu().to(dtype), mean, dtype)
    v = m.mean()
    (v * upstream).backward()
    return m.detach(), v.detach(), s.grad


def analytic_grad(x, y, g, c1, c2, u):
    """The adjoint the kernel implements, for sum over the windows of u * S:
        dS/dmx = 2 my n2 / (d1 d2) - 2 mx S / d1, dS/dvx = -S / d2, dS/dcxy = 2 n1 / (d1 d2)
        A = u (dS/dmx - 2 mx dS/dvx - my dS/dcxy), Bm = 2 u dS/dvx, Cm = u dS/dcxy
        grad(q) = sum over the windows p that contain q of w(p - q) [A(p) + Bm(p) x(q) + Cm(p) y(q)]"""
    mx, my, vx, vy, cxy = moments(x, y, g)
    n1, n2, d1, d2 = 2 * mx * my + c1, 2 * cxy + c2, mx * mx + my * my + c1, vx + vy + c2
    S = n1 * n2 / (d1 * d2)
    s_mx, s_vx, s_cxy = 2 * my * n2 / (d1 * d2) - 2 * mx * S / d1, -S / d2, 2 * n1 / (d1 * d2)
    A, Bm, Cm = u * (s_mx - 2 * mx * s_vx - my * s_cxy), 2 * u * s_vx, u * s_cxy
    n = len(g)
    H, W = S.shape[-2:]

    def scatter(t):  # the transpose of _window
        out = torch.zeros_like(x)
        for i in range(n):
            for j in range(n):
                out[..., i:i + H, j:j + W] += (g[i] * g[j]).to(t.dtype) * t
        return out
    return scatter(A) + scatter(Bm) * x + scatter(Cm) * y


def pair(shape, seed, noise=0.1):
    """A normalised image pair as the model sees it: label in [-mean, 1 - mean], synth = label + noise, a little beyond the range."""
    gen = torch.Generator().manual_seed(seed)
    label = torch.rand(shape, generator=gen) - 0.43
    synth = label + noise * torch.randn(shape, generator=gen)
    return synth, label

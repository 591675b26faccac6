"""float64 restatement of the training loss (include/lograst.h: lograst_loss_forward), written from the formula

    mu1 = w*render  mu2 = w*gt  s11 = w*render^2 - mu1^2  s22 = w*gt^2 - mu2^2  s12 = w*(render*gt) - mu1*mu2
    ssim_map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),  C1 = 0.01^2, C2 = 0.03^2
    ssim = 1 - mean(ssim_map)     l1 = mean|render_l1 - gt|     loss = a * ssim + b * l1

as sums of 11 shifted slices per axis (no conv2d: the same code on CPU and on the device, no convolution library), the
gradient by autograd.  The window is the separable product of the library's own 11 fp32 taps (exact in float64)."""
import math

import numpy as np
import torch

WINDOW = 11


def taps64():
    """The 11 window weights: exp(-(x-5)^2 / (2 * 1.5^2)) in double, normalised, rounded to fp32 once -- as float64."""
    g = [math.exp(-float((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)) for k in range(WINDOW)]
    s = 0.0
    for v in g:
        s += v
    return torch.tensor([v / s for v in g], dtype=torch.float64).to(torch.float32).to(torch.float64)


def window2d(taps=None):
    t = taps64() if taps is None else taps
    return t[:, None] * t[None, :]


def blur(x, window=None):
    """Valid 11x11 correlation of x[..., H, W] with `window` ([11, 11] float64; default: the separable product of taps64,
    applied as two 1-D passes)."""
    H, W = x.shape[-2:]
    if window is None:
        t = taps64().to(device=x.device, dtype=x.dtype)
        h = sum(t[k] * x[..., :, k:W - WINDOW + 1 + k] for k in range(WINDOW))
        return sum(t[k] * h[..., k:H - WINDOW + 1 + k, :] for k in range(WINDOW))
    w = window.to(device=x.device, dtype=x.dtype)
    return sum(w[i, j] * x[..., i:H - WINDOW + 1 + i, j:W - WINDOW + 1 + j] for i in range(WINDOW) for j in range(WINDOW))


def ssim_map(render, gt, window=None):
    mu1, mu2 = blur(render, window), blur(gt, window)
    s11 = blur(render * render, window) - mu1 * mu1
    s22 = blur(gt * gt, window) - mu2 * mu2
    s12 = blur(render * gt, window) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def loss_ref(render, gt, render_l1=None, ssim_weight=0.2, l1_weight=0.8, window=None, upstream=1.0, dtype=torch.float64):
    """All inputs any float dtype / device; computed in `dtype` (float64: the reference value; float32: the same formula at
    the kernels' precision, whose distance to the float64 run is the yardstick for a second fp32 evaluation).  -> dict(loss,
    l1, ssim: python floats; grad_render, grad_render_l1 (None when render_l1 is None): tensors of `dtype`, the gradient of
    upstream * loss)."""
    r = render.detach().to(dtype).clone().requires_grad_(True)
    g = gt.detach().to(dtype)
    rl = None if render_l1 is None else render_l1.detach().to(dtype).clone().requires_grad_(True)
    ssim = 1.0 - ssim_map(r, g, window).mean()
    l1 = ((r if rl is None else rl) - g).abs().mean()
    loss = ssim_weight * ssim + l1_weight * l1
    (upstream * loss).backward()
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()), grad_render=r.grad,
                grad_render_l1=None if rl is None else rl.grad)


def load_case(path):
    """A tests/golden/loss_*.npz fixture -> dict: render, gt (a permuted [B,H,W,3] view where the fixture stores gt_nhwc, as
    LoG passes it), render_l1 or None as CPU tensors; the fixture's remaining entries as numpy."""
    z = dict(np.load(path))
    c = dict(z)
    c["render"] = torch.from_numpy(z["render"])
    c["gt"] = torch.from_numpy(z["gt_nhwc"]).permute(0, 3, 1, 2) if "gt_nhwc" in z else torch.from_numpy(z["gt"])
    c["render_l1"] = torch.from_numpy(z["render_l1"]) if "render_l1" in z else None
    return c


def rel_l2(a, b):
    return float(torch.linalg.norm(a.double() - b.double()) / torch.linalg.norm(b.double()))

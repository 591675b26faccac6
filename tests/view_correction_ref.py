"""float64 restatement of LoG's view correction as the device computes it (include/lograst.h: lograst_loss_*_gain,
lograst_corrector_step), written from the formulas

    l1 = mean | gain[b, c] * render[b, c, y, x] - gt |          l1_scale = l1_weight / (B C H W)
    d l1_weight*l1 / d render = gain * l1_scale * sign(gain * render - gt)          (sign(0) = 0)
    d l1_weight*l1 / d gain[b, c] = l1_scale * sum_{y, x} sign(gain * render - gt) * render

    Corrector.step on row i:  steps[i] += 1;  s = steps[i] - start_step;  s < 0: return (gradient kept)
        t = clip(s / 100, 0, 1);  lr = exp(log(lr_init) (1 - t) + log(lr_final) t)                      (double)
        bias_correction_k = 1 - beta_k ** s  as torch makes it of an int32 tensor: a FLOAT32 number, in every run
        step_size = (1 / bias_correction_1) * lr  in float32 (a Python scalar divided by a tensor)
        the Adam update with max_exp_avg_sq (tests/step_ref.py: adam), betas 0.9 / 0.999, eps 1e-15;  grad[i] = 0

The SSIM term is tests/loss_ref.py's.  Every function takes a dtype: float64 is the reference value, float32 the same formulas
at the kernels' precision.  Held to the reference's recorded results by tests/test_view_correction_cpu.py."""
import math

import numpy as np
import torch

import loss_ref
import step_ref

BETA1, BETA2, EPS, MAX_STEPS = 0.9, 0.999, 1e-15, 100


def l1_gain(render, gt, gain, l1_weight=0.8, upstream=1.0, dtype=torch.float64):
    """-> dict(l1: python float; grad_render [B,C,H,W], grad_gain [B,C]: the gradients of upstream * l1_weight * l1;
    S_gain [B,C] = upstream * l1_scale * sum |render|: the condition scale of grad_gain)."""
    r, g, k = render.detach().to(dtype), gt.detach().to(dtype), gain.detach().to(dtype)
    d = k[:, :, None, None] * r - g
    sgn = torch.sign(d)
    scale = upstream * l1_weight / d.numel()
    return dict(l1=float(d.abs().mean()), grad_render=scale * k[:, :, None, None] * sgn,
                grad_gain=scale * (sgn * r).sum(dim=(2, 3)), S_gain=abs(scale) * r.abs().sum(dim=(2, 3)))


def loss_gain(render, gt, gain, ssim_weight=0.2, l1_weight=0.8, upstream=1.0, dtype=torch.float64, window=None):
    """The whole loss with gain -> dict(loss, l1, ssim: python floats; grad_render, grad_gain, S_gain).  window: the
    [11, 11] weights of the SSIM (default: the separable product of the library's taps, as loss_ref has it)."""
    part = l1_gain(render, gt, gain, l1_weight, upstream, dtype)
    ssim = loss_ref.loss_ref(render, gt, None, ssim_weight, 0.0, window=window, upstream=upstream, dtype=dtype)
    return dict(loss=ssim_weight * ssim["ssim"] + l1_weight * part["l1"], l1=part["l1"], ssim=ssim["ssim"],
                grad_render=ssim["grad_render"] + part["grad_render"], grad_gain=part["grad_gain"], S_gain=part["S_gain"])


def learning_rate(s, lr_init, lr_final):
    t = min(max(s / MAX_STEPS, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def corrector_step(row, steps, start_step, lr_init, lr_final, dtype=torch.float64):
    """row: dict(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq) of [C] tensors, steps: the row's count before the call.
    -> (steps after, dict of the five rows after in `dtype`, dict of their condition scales S_<name>, or None for both after
    an early return: nothing but the count changes)."""
    steps = int(steps) + 1
    s = steps - int(start_step)
    if s < 0:
        return steps, None, None
    lr = learning_rate(s, float(lr_init), float(lr_final))
    st = torch.tensor([[s]], dtype=torch.int32)
    bc1, bc2 = 1 - BETA1 ** st, 1 - BETA2 ** st                       # float32, as in the reference
    assert bc1.dtype == torch.float32
    step_size = lr / bc1                                              # reciprocal() * lr, float32
    r = step_ref.adam(row["param"], row["grad"], row["exp_avg"], row["exp_avg_sq"], row["max_exp_avg_sq"], float(step_size),
                      BETA1, BETA2, float(torch.sqrt(bc2)), EPS, dtype=dtype)
    names = ("param", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
    after = {k: r[k] for k in names}
    after["grad"] = torch.zeros_like(after["param"])
    S = {k: r["S_" + k] for k in names}
    S["grad"] = torch.zeros_like(after["param"])
    return steps, after, S


# ---- fixtures --------------------------------------------------------------------------------------------------------

def load_loss_case(path):
    """A tests/golden/view_correction_loss_*.npz -> dict: render (the `[:, :3]` view of the four-channel tensor where the
    fixture stores render4), gt (a permuted [B,H,W,3] view where it stores gt_nhwc), gain as CPU tensors with the strides
    LoG passes; the fixture's remaining entries as numpy."""
    z = dict(np.load(path))
    c = dict(z)
    c["render"] = torch.from_numpy(z["render4"])[:, :3] if "render4" in z else torch.from_numpy(z["render"])
    c["gt"] = torch.from_numpy(z["gt_nhwc"]).permute(0, 3, 1, 2) if "gt_nhwc" in z else torch.from_numpy(z["gt"])
    c["gain"] = torch.from_numpy(z["gain"])
    return c


def gt_for(c, dtype):
    """The case's gt in the arithmetic of `dtype`: the stored one, except where the case is defined by gt == gain * render
    (equal_left: the product taken in `dtype`, as the generator takes it)."""
    g = c["gt"].to(dtype)
    if "equal_left" in c:
        n = int(c["equal_left"])
        g = g.clone()
        g[..., :n] = (c["gain"].to(dtype)[:, :, None, None] * c["render"].to(dtype))[..., :n]
    return g


STATE = ("param", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def step_rows(z, t, when, suffix):
    """The five rows of recorded step t ('before' / 'after', '32' / '64') as tensors."""
    return {k: torch.from_numpy(z[f"{k}_{when}{suffix}"][t]) for k in STATE}


def within(got, ref32, ref64, S, factor=8.0):
    """|got - ref64| <= factor * (|ref32 - ref64| + 2^-24 * S) per element, NaN exactly where ref64 has it -> (ok, the
    largest ratio error / bound)."""
    got, ref32, ref64, S = (torch.as_tensor(x).double().cpu() for x in (got, ref32, ref64, S))
    nan = torch.isnan(ref64)
    if not torch.equal(torch.isnan(got), nan):
        return False, math.inf
    err = torch.where(nan, torch.zeros_like(got), (got - ref64).abs())
    gap = torch.where(nan, torch.zeros_like(got), (ref32 - ref64).abs())
    bound = factor * (gap + 2.0 ** -24 * torch.where(torch.isfinite(S), S, torch.zeros_like(S)))
    ok = bool((err <= bound).all())
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    return ok, ratio

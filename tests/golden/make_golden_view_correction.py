"""Generates tests/golden/view_correction_*.npz by RUNNING the reference's own classes on the CPU (build container only:
needs the reference tree): LoG/model/corrector.py Corrector, LoG/render/loss.py SSIM(11, 3), torch.nn.L1Loss, combined as
LoG/render/renderer.py:243-266 combines them -- `render_correct = render * view_correction[:, None, None]` per view,
`0.2 * ssim(render, gt) + 0.8 * l1(render_correct[:, :3], gt)` -- once in fp32 and once in float64.

    LOG_REFERENCE=<LoG checkout> python tests/golden/make_golden_view_correction.py

Loss cases (view_correction_loss_*.npz): render (or `render4` [B,4,H,W] where the case passes the `[:, :3]` slice of a
four-channel tensor), gt (or `gt_nhwc` [B,H,W,3] where it is passed permuted, as LoG's batch['image'] is), gain [B,3], and
per quantity q in (l1, ssim, loss, grad_render, grad_gain): q32, q64 and gap32_q = the reference's own fp32-vs-float64
distance (absolute for the scalars, rel-L2 for the gradients).
Case half_equal_40x40 is DEFINED by `gt == gain * render` on the left `equal_left` columns: the stored gt holds the fp32
product there (one rounding), and each run takes the product in its own arithmetic, so that the L1 term is exactly zero on
that half in the float64 run as well (on the stored fp32 gt a float64 product would leave the rounding error of the fp32
one, a sign of +-1 per pixel and no yardstick for an fp32 evaluation).  The float64 run's gt so differs from the stored one
by at most half an fp32 ulp on that half.

Step cases (view_correction_steps_*.npz): a Corrector over V = 2 views from ones, stepped T times; every step hands out
row `index[t]`, takes the gradient of `0.8 * l1(render_correct, gt)` at 24x40 and calls Corrector.step().  Recorded per
step: index, steps_before / steps_after (the row's int32 count) and, for name in (param, grad, exp_avg, exp_avg_sq,
max_exp_avg_sq), the row before and after the call as `<name>_before32/64`, `<name>_after32/64` [T, 3]; start_step,
lr_init, lr_final; render, gt [V, 3, 24, 40] (fp32), the images behind the gradients.  The fp32 and the float64 runs are two closed loops of their own.  In both, `beta ** steps` of an int32
tensor is a float32 tensor (torch's type promotion), so the bias corrections are fp32 numbers in the float64 run as well.
With start_step = 3 the first two calls per view return early (count kept, gradient kept); the third has s = 0, where the
reference divides by a bias correction of zero and the row becomes NaN -- recorded as it is."""
import os
import sys

import numpy as np
import torch

REF = os.environ["LOG_REFERENCE"]          # a checkout of the reference (LoG)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from LoG.model.corrector import Corrector   # noqa: E402  reference code, imported not copied
from LoG.render.loss import SSIM   # noqa: E402

f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731


def smooth(rng, shape, cells):
    """A smooth random field in [0, 1]: bilinear interpolation of a coarse random grid."""
    B, C, H, W = shape
    coarse = torch.tensor(rng.random((B, C, cells, cells)), dtype=torch.float64)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).numpy()


def run_loss(c, dtype):
    ssim_loss = SSIM(window_size=11, channel=3).to(dtype)
    l1_loss = torch.nn.L1Loss()
    if "render4" in c:
        leaf = torch.tensor(c["render4"], dtype=dtype, requires_grad=True)
        r = leaf[:, :3]
    else:
        leaf = r = torch.tensor(c["render"], dtype=dtype, requires_grad=True)
    g = torch.tensor(c["gt_nhwc"], dtype=dtype).permute(0, 3, 1, 2) if "gt_nhwc" in c else torch.tensor(c["gt"], dtype=dtype)
    k = torch.tensor(c["gain"], dtype=dtype, requires_grad=True)
    if "equal_left" in c:            # the case's definition, in this run's arithmetic (see the module docstring)
        n = int(c["equal_left"])
        g = g.clone()
        g[..., :n] = (k.detach()[:, :, None, None] * r.detach())[..., :n]
        assert dtype != torch.float32 or np.array_equal(g.numpy(), c["gt"])
    render_correct = torch.stack([r[b] * k[b][:, None, None] for b in range(r.shape[0])])      # renderer.py:244-250
    ssim = ssim_loss(r, g)
    l1 = l1_loss(render_correct[:, :3], g)
    loss = 0.2 * ssim + 0.8 * l1
    loss.backward()
    return dict(l1=l1.item(), ssim=ssim.item(), loss=loss.item(), grad_render=leaf.grad[:, :3].numpy(), grad_gain=k.grad.numpy())


def loss_cases():
    rng = np.random.default_rng(20241018)
    # one output pixel
    yield "1x11x11", dict(render=f32(rng.random((1, 3, 11, 11))), gt=f32(rng.random((1, 3, 11, 11))),
                          gain=f32([[1.07, 0.95, 1.02]]))
    # odd sizes, tile edges, two images with two different gains
    r = smooth(rng, (2, 3, 37, 53), 6)
    yield "2x37x53", dict(render=f32(r + 0.1 * (rng.random(r.shape) - 0.5)), gt=f32(np.clip(r + 0.05 * rng.standard_normal(r.shape), 0, 1)),
                          gain=f32([[1.1, 0.93, 1.04], [0.88, 1.0, 1.21]]))
    # gt == fp32(gain * render) on the left half: exact zeros of the L1 term, as long as the product is rounded to fp32
    r = f32(smooth(rng, (1, 3, 40, 40), 5))
    gain = f32([[1.1, 0.93, 1.04]])
    g = f32(np.clip(r + 0.1 * rng.standard_normal(r.shape), 0, 1))
    g[..., :20] = (gain[:, :, None, None] * r)[..., :20]                 # one fp32 multiply
    assert g.dtype == np.float32
    yield "half_equal_40x40", dict(render=r, gt=g, gain=gain, equal_left=np.int32(20))
    # the strides LoG passes: gt built [B, H, W, 3] and permuted, render the [:, :3] slice of a four-channel tensor
    r = smooth(rng, (2, 3, 45, 70), 7)
    r4 = f32(np.concatenate([np.clip(r + 0.05 * rng.standard_normal(r.shape), 0, 1), rng.random((2, 1, 45, 70))], axis=1))
    gt_nhwc = f32(np.clip(r * np.array([0.9, 1.05, 1.1])[None, :, None, None] + 0.08 * rng.standard_normal(r.shape), 0, 1).transpose(0, 2, 3, 1))
    yield "nhwc_slice_45x70", dict(render4=r4, gt_nhwc=gt_nhwc, gain=f32([[0.92, 1.03, 1.12], [1.05, 0.97, 0.9]]))


def run_steps(T, start_step, dtype, seed):
    rng = np.random.default_rng(seed)
    V, H, W = 2, 24, 40
    render = smooth(rng, (V, 3, H, W), 4)
    true_gain = np.array([[1.15, 0.9, 1.05], [0.85, 1.1, 0.95]])
    gt = np.clip(render * true_gain[:, :, None, None] + 0.03 * rng.standard_normal(render.shape), 0, 1)
    index = [0 if rng.random() < 0.62 else 1 for _ in range(T)]
    images = dict(render=f32(render), gt=f32(gt))
    render, gt = torch.tensor(images["render"], dtype=dtype), torch.tensor(images["gt"], dtype=dtype)
    cor = Corrector(True, start_step=start_step)
    cor.init(V)
    cor.view_correction.data = cor.view_correction.data.to(dtype)
    cor.training_setup()
    l1_loss = torch.nn.L1Loss()
    opt = cor.optimizer
    state = lambda i: dict(param=cor.view_correction.data[i], grad=cor.view_correction.grad[i],   # noqa: E731
                           exp_avg=opt.exp_avg["view_correction"][i], exp_avg_sq=opt.exp_avg_sq["view_correction"][i],
                           max_exp_avg_sq=opt.max_exp_avg_sq["view_correction"][i])
    rec = {k + w: [] for k in ("param", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq") for w in ("_before", "_after")}
    rec.update(steps_before=[], steps_after=[])
    for i in index:
        row = cor[i]
        render_correct = render[i] * row[:, None, None]
        (0.8 * l1_loss(render_correct[None][:, :3], gt[i][None])).backward()
        rec["steps_before"].append(int(opt.steps["view_correction"][i]))
        for k, v in state(i).items():
            rec[k + "_before"].append(v.clone().numpy())
        cor.step()
        rec["steps_after"].append(int(opt.steps["view_correction"][i]))
        for k, v in state(i).items():
            rec[k + "_after"].append(v.clone().numpy())
    return np.array(index, np.int32), {k: np.array(v) for k, v in rec.items()}, (cor, images)


def main():
    for name, c in loss_cases():
        o32, o64 = run_loss(c, torch.float32), run_loss(c, torch.float64)
        out = dict(c)
        for k in o32:
            if k.startswith("grad"):
                out[k + "32"] = o32[k].astype(np.float32)
                out[k + "64"] = o64[k].astype(np.float64)
                out["gap32_" + k] = np.float64(np.linalg.norm(o32[k].astype(np.float64) - o64[k]) / np.linalg.norm(o64[k]))
            else:
                out[k + "32"] = np.float32(o32[k])
                out[k + "64"] = np.float64(o64[k])
                out["gap32_" + k] = np.float64(abs(float(o32[k]) - float(o64[k])))
        path = os.path.join(HERE, "view_correction_loss_%s.npz" % name)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), {k: float(v) for k, v in out.items() if k.startswith("gap32")})
    for name, T, start in (("start0", 250, 0), ("start3", 14, 3)):
        idx, r32, (cor, images) = run_steps(T, start, torch.float32, 7)
        idx64, r64, _ = run_steps(T, start, torch.float64, 7)
        assert np.array_equal(idx, idx64) and np.array_equal(r32["steps_after"], r64["steps_after"])
        out = dict(images, index=idx, start_step=np.int32(start), lr_init=np.float64(cor.lr_init), lr_final=np.float64(cor.lr_final),
                   steps_before=r32["steps_before"].astype(np.int32), steps_after=r32["steps_after"].astype(np.int32))
        for k in r32:
            if not k.startswith("steps"):
                out[k + "32"] = r32[k].astype(np.float32)
                out[k + "64"] = r64[k].astype(np.float64)
        path = os.path.join(HERE, "view_correction_steps_%s.npz" % name)
        np.savez_compressed(path, **out)
        with np.errstate(invalid="ignore"):
            drift = np.nanmax(np.abs(out["param_after32"].astype(np.float64) - out["param_after64"])) if T else 0.0
        print(path, os.path.getsize(path), "steps per view", [int((idx == v).sum()) for v in (0, 1)],
              "max |param32 - param64|", float(drift))


if __name__ == "__main__":
    main()

"""Generates tests/golden/loss_*.npz by RUNNING the reference's own loss on CPU (build container only: needs the
reference tree): LoG/render/loss.py SSIM(11, 3) + torch.nn.L1Loss + `0.2 * ssim + 0.8 * l1` (LoG/render/renderer.py:
253-266) + backward(), once in fp32 and once with module and inputs in float64.

    LOG_REFERENCE=<LoG checkout> python tests/golden/make_golden_loss.py

Every file holds: render, gt (fp32; `gt_nhwc` [B,H,W,3] instead of gt where the case passes a permuted view as LoG does),
render_l1 (only where it is a tensor of its own), window (the 121 fp32 weights of the reference's SSIM buffer), and per
quantity q in (l1, ssim, loss, grad_render[, grad_render_l1]): q32, q64 and gap32_q = the reference's own fp32-vs-float64
distance (absolute for the scalars, rel-L2 for the gradients)."""
import os
import sys

import numpy as np
import torch

REF = os.environ["LOG_REFERENCE"]          # a checkout of the reference (LoG)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from LoG.render.loss import SSIM   # noqa: E402  reference code, imported not copied


def run(render, gt, render_l1, dtype):
    ssim_loss = SSIM(window_size=11, channel=3).to(dtype)
    l1_loss = torch.nn.L1Loss()
    r = torch.tensor(render, dtype=dtype, requires_grad=True)
    g = torch.tensor(gt, dtype=dtype)
    rl = r if render_l1 is None else torch.tensor(render_l1, dtype=dtype, requires_grad=True)
    ssim = ssim_loss(r, g)
    l1 = l1_loss(rl, g)
    loss = 0.2 * ssim + 0.8 * l1
    loss.backward()
    out = dict(l1=l1.item(), ssim=ssim.item(), loss=loss.item(), grad_render=r.grad.numpy())
    if render_l1 is not None:
        out["grad_render_l1"] = rl.grad.numpy()
    return out, ssim_loss.window[0, 0].numpy()


def smooth(rng, shape, cells):
    """A smooth random field in [0, 1]: bilinear interpolation of a coarse random grid."""
    B, C, H, W = shape
    coarse = torch.tensor(rng.random((B, C, cells, cells)), dtype=torch.float64)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).numpy()


def cases():
    rng = np.random.default_rng(20240611)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    # one output pixel
    yield "1x11x11", dict(render=f32(rng.random((1, 3, 11, 11))), gt=f32(rng.random((1, 3, 11, 11))))
    # odd sizes, tile edges, two images
    r = smooth(rng, (2, 3, 37, 53), 6)
    yield "2x37x53", dict(render=f32(r + 0.1 * (rng.random(r.shape) - 0.5)), gt=f32(np.clip(r + 0.05 * rng.standard_normal(r.shape), 0, 1)))
    # gt built [B, H, W, 3] and permuted, as LoG's batch['image'] is
    r = smooth(rng, (1, 3, 64, 96), 8)
    gt_nhwc = f32(np.clip(r + 0.08 * rng.standard_normal(r.shape), 0, 1).transpose(0, 2, 3, 1))
    yield "nhwc_64x96", dict(render=f32(np.clip(r + 0.05 * rng.standard_normal(r.shape), 0, 1)), gt_nhwc=gt_nhwc)
    # render_l1 = render * per-channel gain (render_correct)
    r = f32(smooth(rng, (1, 3, 40, 40), 5))
    gain = np.array([1.1, 0.93, 1.04], np.float32)[None, :, None, None]
    yield "correct_40x40", dict(render=r, render_l1=f32(r * gain), gt=f32(np.clip(r + 0.1 * rng.standard_normal(r.shape), 0, 1)))
    # render == gt on the left half: sign(0) exactly, ssim_map == 1 there
    g = f32(smooth(rng, (1, 3, 48, 48), 6))
    r = g.copy()
    r[..., 24:] = f32(np.clip(g[..., 24:] + 0.1 * rng.standard_normal(g[..., 24:].shape), 0, 1))
    yield "half_equal_48x48", dict(render=r, gt=g)
    # smooth low contrast: both within 1e-3 of 0.5 (w*x^2 - mu^2 cancels to 1e-6 of its terms)
    yield "low_contrast_40x56", dict(render=f32(0.5 + 2e-3 * (smooth(rng, (1, 3, 40, 56), 4) - 0.5)),
                                     gt=f32(0.5 + 2e-3 * (smooth(rng, (1, 3, 40, 56), 4) - 0.5)))
    # values outside [0, 1] (LoG's colours are not clamped)
    yield "unclamped_33x45", dict(render=f32(-0.3 + 1.8 * rng.random((1, 3, 33, 45))), gt=f32(rng.random((1, 3, 33, 45))))


def main():
    for name, c in cases():
        gt = c["gt"] if "gt" in c else np.ascontiguousarray(c["gt_nhwc"].transpose(0, 3, 1, 2))
        o32, window = run(c["render"], gt, c.get("render_l1"), torch.float32)
        o64, window64 = run(c["render"], gt, c.get("render_l1"), torch.float64)
        assert window.dtype == np.float32 and np.array_equal(window.astype(np.float64), window64)
        out = dict(c, window=window)
        for k in o32:
            if k.startswith("grad"):
                out[k + "32"] = o32[k].astype(np.float32)
                out[k + "64"] = o64[k].astype(np.float64)
                out["gap32_" + k] = np.float64(np.linalg.norm(o32[k].astype(np.float64) - o64[k]) / np.linalg.norm(o64[k]))
            else:
                out[k + "32"] = np.float32(o32[k])
                out[k + "64"] = np.float64(o64[k])
                out["gap32_" + k] = np.float64(abs(float(o32[k]) - float(o64[k])))
        path = os.path.join(HERE, "loss_%s.npz" % name)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), {k: float(v) for k, v in out.items() if k.startswith("gap32")})


if __name__ == "__main__":
    main()

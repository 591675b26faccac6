"""Generates tests/golden/fgmask_*.npz by RUNNING the reference's own MaskForeground.forward (LoG/render/renderer.py:
343-373) on the CPU (build container only: needs the reference tree), once in fp32 and once with module and inputs in
float64: bound_from_mask with its padding, the crop, `gt * msk + (1 - msk) * background`, calculate_loss with and without
mask_ignore, backward() to a fixed `render` leaf.  `vis` is replaced by a subclass method that returns that leaf (no
rasterizer runs); use_randback is False, so the background is the module's buffer.  cv2 is stubbed, as in the CPU tests:
only the reference's visualisation helpers use it.

    LOG_REFERENCE=<LoG checkout> python tests/golden/make_golden_fgmask.py

Every file holds the inputs -- image [1, H, W, 3], mask [1, H, W], mask_ignore [1, H, W] (only where the case has one),
render [1, 3, H, W], background [3], all fp32 --, ltrb (what bound_from_mask returned), crop_shape (of output['render']),
crop_offset (its storage offset inside the render leaf), and per quantity q in (l1, ssim, loss, grad_render, gt): q32, q64
and gap32_q = the reference's own fp32-vs-float64 distance (absolute for the scalars, rel-L2 for grad_render and gt).
grad_render is the gradient of the leaf INSIDE the crop (the generator asserts that it is exactly zero outside), gt is
output['gt'].  gap32_grad_render < 1.25e-5 is asserted for every case, so that the tests' bound min(1e-4, 8 * gap32) is one
the reference's own fp32 run meets."""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ["LOG_REFERENCE"]          # a checkout of the reference (LoG)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the rasterizer packages the renderer imports by name
sys.path.insert(0, REF)
sys.modules.setdefault("cv2", types.ModuleType("cv2"))

import log_amd   # noqa: E402
log_amd.install_compute_radius()
from LoG.render.renderer import MaskForeground   # noqa: E402  reference code, imported not copied

f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)   # noqa: E731


def smooth(rng, shape, cells):
    """A smooth random field in [0, 1]: bilinear interpolation of a coarse random grid."""
    B, C, H, W = shape
    coarse = torch.tensor(rng.random((B, C, cells, cells)), dtype=torch.float64)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).numpy()


class FixedRender(MaskForeground):
    """MaskForeground with `vis` returning a fixed render leaf."""

    def vis(self, batch, model, background=None):
        self.seen_background = background
        return {"render": self.leaf}


def run(c, dtype):
    module = FixedRender(split="train", use_randback=False, background=[float(v) for v in c["background"]]).to(dtype)
    module.leaf = torch.tensor(c["render"], dtype=dtype, requires_grad=True)
    batch = {"image": torch.tensor(c["image"], dtype=dtype), "mask": torch.tensor(c["mask"], dtype=dtype)}
    if "mask_ignore" in c:
        batch["mask_ignore"] = torch.tensor(c["mask_ignore"], dtype=dtype)
    msk = batch["mask"][..., None]
    ltrb = [int(v) for v in module.bound_from_mask(msk, int(max(msk.shape) / 50))]
    output = module(batch, types.SimpleNamespace(training=True))
    assert module.seen_background is module.background
    output["loss"].backward()
    crop = output["render"]
    t, l = ltrb[1], ltrb[0]
    h, w = crop.shape[2:]
    grad = module.leaf.grad
    outside = grad.clone()
    outside[:, :, t:t + h, l:l + w] = 0
    assert float(outside.abs().max()) == 0.0
    if "mask_ignore" in c:
        assert output["mask_ignore"].shape == (1, h, w)
    return dict(l1=output["loss_dict"]["l1"], ssim=output["loss_dict"]["ssim"], loss=output["loss"].item(),
                grad_render=grad[:, :, t:t + h, l:l + w].numpy().copy(), gt=output["gt"].detach().numpy().copy(),
                ltrb=ltrb, crop_shape=list(crop.shape), crop_offset=int(crop.storage_offset()))


def scene(rng, H, W, cells=6):
    """image [1, H, W, 3], render [1, 3, H, W]: a smooth field with noise, as the loss fixtures' nhwc case."""
    r = smooth(rng, (1, 3, H, W), cells)
    image = f32(np.clip(r + 0.08 * rng.standard_normal(r.shape), 0, 1).transpose(0, 2, 3, 1))
    render = f32(np.clip(r + 0.05 * rng.standard_normal(r.shape), 0, 1))
    return image, render


def box(H, W, rows, cols):
    m = np.zeros((1, H, W), np.float32)
    m[:, rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = 1.0
    return m


def cases():
    rng = np.random.default_rng(20240917)
    bg = f32([0.2, 0.5, 0.8])
    # rows 10..44, columns 20..69 of 60 x 90: padding 1, crop [1, 3, 37, 52] at storage offset 829
    image, render = scene(rng, 60, 90)
    mask = box(60, 90, (10, 44), (20, 69))
    yield "box_60x90", dict(image=image, render=render, mask=mask, background=bg)
    # ... with an ignore mask: a binary blob and a soft band
    ignore = np.zeros((1, 60, 90), np.float32)
    ignore[:, 15:30, 30:50] = 1.0
    ignore[:, 30:40, :] = f32(rng.random((1, 10, 90)))
    yield "box_ignore_60x90", dict(image=image, render=render, mask=mask, mask_ignore=ignore, background=bg)
    # a box in the top right corner: the clamp to 0 at the top, the slice's clamp at the right
    image, render = scene(rng, 48, 64)
    yield "corner_48x64", dict(image=image, render=render, mask=box(48, 64, (0, 20), (40, 63)), background=f32([1, 1, 1]),
                               mask_ignore=f32(rng.random((1, 48, 64)) > 0.7))
    # one pixel: padding int(400 / 50) = 8 gives a crop of 17 x 17 (7 x 7 output pixels).  The composited ground truth is
    # the background everywhere else; over black the reference's fp32 `w * gt^2 - mu2^2` cancels nothing (over a bright
    # constant its own fp32-vs-float64 gap is 5e-5)
    image, render = scene(rng, 26, 400, 4)
    yield "pixel_26x400", dict(image=image, render=render, mask=box(26, 400, (12, 12), (100, 100)), background=f32([0, 0, 0]))
    # a non-binary mask: a bump with values in (0, 1) -- the composite mixes, the bounds cut at 0.5
    image, render = scene(rng, 60, 90)
    yy, xx = np.mgrid[0:60, 0:90]
    soft = f32(0.02 + 0.96 * np.exp(-(((yy - 30) / 18.0) ** 2 + ((xx - 45) / 24.0) ** 2)))[None]
    assert 0 < soft.min() and soft.max() < 1 and (soft > 0.5).any() and (soft <= 0.5).any()
    yield "soft_60x90", dict(image=image, render=render, mask=soft, background=f32([0, 0, 0]),
                             mask_ignore=f32(0.5 * rng.random((1, 60, 90))))
    # crops of exactly 42 columns (one tile of the loss) and 43 (a second tile of one column)
    for cols in (42, 43):
        image, render = scene(rng, 40, 80)
        yield "cols%d_40x80" % cols, dict(image=image, render=render, mask=box(40, 80, (5, 30), (20, 20 + cols - 3)),
                                          background=bg)


def main():
    for name, c in cases():
        o32, o64 = run(c, torch.float32), run(c, torch.float64)
        for k in ("ltrb", "crop_shape", "crop_offset"):
            assert o32[k] == o64[k]
        out = dict(c, ltrb=np.array(o32["ltrb"], np.int64), crop_shape=np.array(o32["crop_shape"], np.int64),
                   crop_offset=np.int64(o32["crop_offset"]))
        for k in ("l1", "ssim", "loss"):
            out[k + "32"], out[k + "64"] = np.float32(o32[k]), np.float64(o64[k])
            out["gap32_" + k] = np.float64(abs(float(o32[k]) - float(o64[k])))
        for k in ("grad_render", "gt"):
            out[k + "32"], out[k + "64"] = o32[k].astype(np.float32), o64[k].astype(np.float64)
            out["gap32_" + k] = np.float64(np.linalg.norm(o32[k].astype(np.float64) - o64[k]) / np.linalg.norm(o64[k]))
        assert out["gap32_grad_render"] < 1.25e-5, (name, out["gap32_grad_render"])
        path = os.path.join(HERE, "fgmask_%s.npz" % name)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), out["crop_shape"].tolist(), int(out["crop_offset"]),
              {k: float(v) for k, v in out.items() if k.startswith("gap32")})


if __name__ == "__main__":
    main()

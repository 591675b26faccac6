"""Restatement of the masked training loss as the device computes it (include/lograst.h: lograst_loss_forward_masked,
lograst_mask_bounds), on tests/loss_ref.py's ssim_map, in float64 or float32, the gradient by autograd:

    g = gt * f + (1 - f) * background[c]      with a foreground mask f [B, H, W]; else g = gt
    x = g * m + render * (1 - m)              with an ignore mask m [B, H, W]; else x = render
    ssim = 1 - mean(ssim_map(x, g))           l1 = mean|y - g|, y = render_l1, or gain[b, c] * render, or x
    loss = a * ssim + b * l1                  (means over all elements: nothing is renormalised by a mask)

and the bounds MaskForeground.bound_from_mask returns (LoG/render/renderer.py:319-326), from numpy.
tests/test_masked_loss_cpu.py holds it to the reference's own recorded results (tests/golden/fgmask_*.npz)."""
import numpy as np
import torch

import loss_ref


def composite(gt, foreground, background):
    """gt [B, C, H, W], foreground [B, H, W], background [C] -> gt * f + (1 - f) * bg, in gt's dtype."""
    f = foreground[:, None]
    return gt * f + (1 - f) * background.to(gt.dtype)[None, :, None, None]


def blend(render, gt, mask):
    m = mask[:, None]
    return gt * m + render * (1 - m)


def masked_loss(render, gt, mask=None, foreground=None, background=None, render_l1=None, gain=None, ssim_weight=0.2,
                l1_weight=0.8, window=None, upstream=1.0, dtype=torch.float64):
    """Inputs of any float dtype / device, computed in `dtype` -> dict(loss, l1, ssim: python floats; gt: the composited
    ground truth; grad_render, grad_render_l1, grad_gain: tensors of `dtype` or None, the gradient of upstream * loss)."""
    assert render_l1 is None or gain is None
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    cast = lambda t: None if t is None else t.detach().to(dtype)
    r, rl, k = leaf(render), leaf(render_l1), leaf(gain)
    g, m, f = cast(gt), cast(mask), cast(foreground)
    if f is not None:
        g = composite(g, f, cast(background))
    x = r if m is None else blend(r, g, m)
    ssim = 1.0 - loss_ref.ssim_map(x, g, window).mean()
    y = rl if rl is not None else (k[:, :, None, None] * r if k is not None else x)
    l1 = (y - g).abs().mean()
    loss = ssim_weight * ssim + l1_weight * l1
    (upstream * loss).backward()
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()), gt=g, grad_render=r.grad,
                grad_render_l1=None if rl is None else rl.grad, grad_gain=None if k is None else k.grad)


def bounds_record(mask, threshold=0.5):
    """numpy mask [B, H, W] -> int32 [B, 8]: (xmin, ymin, xmax, ymax, count, 0, 0, 0) of mask > threshold; an image without
    such a pixel: (W, H, -1, -1, 0, 0, 0, 0)."""
    mask = np.asarray(mask)
    B, H, W = mask.shape
    out = np.zeros((B, 8), np.int32)
    for b in range(B):
        ys, xs = np.nonzero(mask[b] > threshold)
        out[b, :5] = (xs.min(), ys.min(), xs.max(), ys.max(), len(xs)) if len(xs) else (W, H, -1, -1, 0)
    return out


def bounds(mask, padding, threshold=0.5):
    """-> (l, t, r, b) as bound_from_mask(mask[..., None], padding) for a mask [1, H, W]; IndexError for an empty one."""
    xmin, ymin, xmax, ymax, count = (int(v) for v in bounds_record(mask, threshold)[0, :5])
    if count == 0:
        raise IndexError("index 0 is out of bounds for dimension 0 with size 0")
    return max(xmin - padding, 0), max(ymin - padding, 0), xmax + padding, ymax + padding


def crop_of(shape_hw, ltrb):
    """The slices [t:b+1, l:r+1] clamp to: -> (t, l, height, width)."""
    H, W = shape_hw
    l, t, r, b = ltrb
    return t, l, min(b + 1, H) - t, min(r + 1, W) - l


def load_case(path):
    """A tests/golden/fgmask_*.npz fixture -> dict: image [1, H, W, 3], mask [1, H, W], mask_ignore or None, render
    [1, 3, H, W], background [3] as CPU tensors; the remaining entries as numpy."""
    z = dict(np.load(path))
    c = dict(z)
    for k in ("image", "mask", "render", "background"):
        c[k] = torch.from_numpy(z[k])
    c["mask_ignore"] = torch.from_numpy(z["mask_ignore"]) if "mask_ignore" in z else None
    return c


def cropped_inputs(c, ltrb=None):
    """The views MaskForeground.forward crops out of a fixture's tensors -> (render, gt, foreground, mask_ignore)."""
    l, t, r, b = ltrb if ltrb is not None else (int(v) for v in c["ltrb"])
    sl = (slice(t, b + 1), slice(l, r + 1))
    render = c["render"][:, :, sl[0], sl[1]]
    gt = c["image"].permute(0, 3, 1, 2)[:, :, sl[0], sl[1]]
    fg = c["mask"][:, sl[0], sl[1]]
    mi = None if c["mask_ignore"] is None else c["mask_ignore"][:, sl[0], sl[1]]
    return render, gt, fg, mi

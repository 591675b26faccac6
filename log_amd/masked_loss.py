"""The training loss with masks on the device: LoG's ``mask_ignore`` blend (LoG/render/renderer.py:253-266) and the
foreground training of ``MaskForeground`` (renderer.py:318-373) inside the fused loss kernels (log_amd/csrc/loss.hip, the
``MASKED`` instantiations; C ABI ``lograst_loss_*_masked``, ``lograst_mask_bounds*``).

* ``masked_l1_ssim_loss(render, gt, mask=None, foreground=None, background=None, render_l1=None, l1_gain=None,
  ssim_weight=0.2, l1_weight=0.8) -> (loss, l1, ssim, gt_used)``: ``g = gt * f + (1 - f) * background[c]`` with a
  foreground mask, ``x = g * m + render * (1 - m)`` with an ignore mask, ``ssim`` of ``(x, g)``, ``l1`` of ``x`` -- or of
  ``render_l1`` / ``l1_gain * render``, which stay unblended as the reference's ``render_correct`` does.  Every step is the
  fp32 operation the torch expression performs, so results carry the bits of the torch blend around ``log_amd.loss``.
  ``gt_used`` is the composited ground truth (detached), or ``gt`` itself without a foreground.
* ``mask_bounds(mask, threshold=0.5)`` -> int32 [B, 8] on the device (xmin, ymin, xmax, ymax, count, 0, 0, 0);
  ``mask_bounds_host(mask, padding)`` -> python ints ``(l, t, r, b)`` after ONE read-back, as ``bound_from_mask`` returns.
* ``set_enabled(True)``: the ``mask_ignore is not None`` branches of ``log_amd.loss``'s and ``log_amd.view_correction``'s
  ``calculate_loss`` go through the masked kernels (one forward, one backward); off (the default) they run as before.
* ``install()``: ``log_amd.loss`` first, the switch on, then the drop-ins ``MaskForeground.bound_from_mask`` and
  ``MaskForeground.forward`` (``split == 'train'``: two read-backs, the bounds and ``loss_dict``).

What the drop-ins do not cover goes to the reference's method, counted by reason in ``stats()``: a batch of more than one
image, tensors off the GPU or not float32, tensors that require a gradient, image / mask / background shapes that do not fit
each other, a crop under 11 pixels, view correction (``render_correct``: the reference itself fails on its shape) and loss
modules the kernels do not cover.  All of that is decided before the background is drawn; a ``vis`` that then returns a
``render_correct`` or a render of another shape, dtype or device after all raises ``LograstError``."""
import ctypes

import torch

from . import _lib
from . import loss as _loss
from ._dropin import DropIns, Fallback
from .rasterizer import _ptr, _stream_ptr

RECORD_INTS = 8      # int32 per image of the bounds record (launch.hpp: MB_RECORD_INTS)


def _fused_masked(render, gt, mask, foreground, background, render_l1, l1_gain, ssim_weight, l1_weight):
    """-> (loss, stats [l1, ssim], gt_used)."""
    if mask is None and foreground is None:
        raise ValueError("masked_l1_ssim_loss needs a mask or a foreground: without either use log_amd.loss.l1_ssim_loss")
    if l1_gain is not None and render_l1 is not None:
        raise ValueError("l1_gain and render_l1 are mutually exclusive: the L1 term reads one of them")
    if foreground is not None and background is None:
        raise ValueError("a foreground mask needs the background it composites the ground truth over")
    if render_l1 is render:
        render_l1 = None
    loss, stats, gt_out = _loss._L1SSIM.apply(render, gt, mask, foreground, background, render_l1, l1_gain, ssim_weight, l1_weight,
                                              _loss.FROM_MASKED_LOSS)
    return loss, stats, gt if gt_out is None else gt_out


def masked_l1_ssim_loss(render, gt, mask=None, foreground=None, background=None, render_l1=None, l1_gain=None, ssim_weight=0.2,
                        l1_weight=0.8):
    """-> (loss, l1, ssim, gt_used).  ``render``, ``gt``, ``render_l1`` [B, C, H, W]; ``mask`` (the ignore mask) and
    ``foreground`` [B, H, W]; ``background`` [C]; ``l1_gain`` [B, C]: float32 on the device, any strides; H, W >= 11; at least
    one of ``mask`` and ``foreground``.  ``loss`` carries the graph (gradients for ``render`` and ``render_l1`` or
    ``l1_gain``); ``l1`` and ``ssim`` are detached 0-dim views of one device buffer; the means run over all elements (the
    reference does not renormalise by a mask).  ``gt``, the masks and the background must not require a gradient."""
    loss, stats, gt_used = _fused_masked(render, gt, mask, foreground, background, render_l1, l1_gain, ssim_weight, l1_weight)
    return loss, stats[0], stats[1], gt_used


# ---- the bounding box of a foreground mask ---------------------------------------------------------------------------

def _bounds_mask(mask):
    if not torch.is_tensor(mask) or mask.device.type != "cuda":
        raise _lib.LograstError(
            f"log_amd.masked_loss needs tensors on the MI355X (mask is on '{getattr(mask, 'device', None)}'); the HIP kernels "
            "are the only implementation -- there is no CPU fallback")
    if mask.dtype != torch.float32 or mask.dim() != 3:
        raise ValueError(f"mask: expected a float32 tensor [B, H, W], got {mask.dtype} {tuple(mask.shape)}")
    return mask.detach()


def mask_bounds(mask, threshold=0.5):
    """-> int32 [B, 8] on the device: per image (xmin, ymin, xmax, ymax, count, 0, 0, 0) of the pixels with ``mask >
    threshold`` (strict; a NaN is no foreground); without such a pixel (W, H, -1, -1, 0).  Nothing is read back."""
    m = _bounds_mask(mask)
    L = _lib.lib()
    B, H, W = (int(s) for s in m.shape)
    record = torch.empty((B, RECORD_INTS), dtype=torch.int32, device=m.device)
    with torch.cuda.device(m.device):
        _lib.check(L.lograst_mask_bounds(B, H, W, _ptr(m), _loss._strides(m), float(threshold), _ptr(record),
                                         record.numel() * 4, _stream_ptr(m.device)))
    return record


def mask_bounds_host(mask, padding):
    """``MaskForeground.bound_from_mask`` for a mask [1, H, W]: -> python ints ``(l, t, r, b)`` = (max(xmin - padding, 0),
    max(ymin - padding, 0), xmax + padding, ymax + padding) after one read-back; the upper bounds stay unclamped (slicing
    clamps them, as in the reference).  IndexError when no pixel is above 0.5, as the reference's ``[0]`` on an empty
    ``where`` raises."""
    if int(mask.shape[0]) != 1:
        raise ValueError("only support batch size 1")
    record = mask_bounds(mask, 0.5)
    host = (ctypes.c_int32 * RECORD_INTS)()
    with torch.cuda.device(record.device):
        _lib.check(_lib.lib().lograst_mask_bounds_read(_ptr(record), 1, host, _stream_ptr(record.device)))
    xmin, ymin, xmax, ymax, count = host[0], host[1], host[2], host[3], host[4]
    if count == 0:
        raise IndexError("index 0 is out of bounds for dimension 0 with size 0")
    padding = int(padding)
    return max(xmin - padding, 0), max(ymin - padding, 0), xmax + padding, ymax + padding


# ---- the switch: calculate_loss's mask_ignore branch -----------------------------------------------------------------

def _mask_fits(mask_ignore, render):
    return (torch.is_tensor(mask_ignore) and mask_ignore.device == render.device and mask_ignore.dtype == torch.float32
            and tuple(mask_ignore.shape) == (render.shape[0],) + tuple(render.shape[2:]) and not mask_ignore.requires_grad)


def _calculate_loss_branch(gt_image, render, output, mask_ignore):
    """log_amd.loss's calculate_loss with a mask_ignore, behind its own predicate: one forward, one backward, no torch blend.
    -> True when it has filled ``output``; False leaves the call to the lines that were there."""
    if not _mask_fits(mask_ignore, render):
        return False
    render_l1 = output["render_correct"][:, :3] if "render_correct" in output.keys() else None
    if render_l1 is not None and not (_loss._fusable(render_l1) and render_l1.shape == render.shape
                                      and render_l1.device == render.device):
        return False
    _loss._publish(output, *_fused_masked(render, gt_image, mask_ignore, None, None, render_l1, None, 0.2, 0.8)[:2])
    return True


def set_enabled(on):
    """True: a ``mask_ignore`` in log_amd.loss's and log_amd.view_correction's ``calculate_loss`` goes through the masked
    kernels.  False (the default): both run their torch blend."""
    _loss._masked_branch = _calculate_loss_branch if on else None


def enabled():
    return _loss._masked_branch is not None


# ---- drop-ins for an unmodified LoG checkout -------------------------------------------------------------------------

def _targets():
    from LoG.render.renderer import MaskForeground
    return {"bound_from_mask": (MaskForeground, "bound_from_mask"), "forward": (MaskForeground, "forward")}


dropins = DropIns("masked_loss", _targets)
stats, reset_stats = dropins.stats, dropins.reset_stats

OFF_GPU = "tensors are off the GPU or not float32"
NEEDS_GRAD = "image, mask or background requires a gradient"
SHAPES = "image, mask and background shapes do not fit"


def _on_gpu(*tensors):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


@dropins.dropin
def bound_from_mask(self, msk, padding):
    """MaskForeground.bound_from_mask: one pass over the mask on the device and one read-back -> python ints."""
    if not torch.is_tensor(msk) or msk.dim() != 4 or int(msk.shape[0]) != 1:
        raise Fallback("a batch of more than one image")
    if not _on_gpu(msk):
        raise Fallback(OFF_GPU)
    bounds = mask_bounds_host(msk[..., 0], padding)
    dropins.count("readbacks", "bound_from_mask")
    return bounds


def _forward_inputs(self, batch, model):
    """The checks of MaskForeground.forward that need no device work -> (image, mask, mask_ignore or None, background)."""
    image, mask = batch["image"], batch["mask"]
    if not (torch.is_tensor(image) and torch.is_tensor(mask) and image.dim() == 4 and mask.dim() == 3
            and int(image.shape[0]) == 1 and int(mask.shape[0]) == 1):
        raise Fallback("a batch of more than one image")
    mask_ignore = batch["mask_ignore"] if "mask_ignore" in batch.keys() else None
    background = self.background
    tensors = [image, mask, background] + ([mask_ignore] if mask_ignore is not None else [])
    if not _on_gpu(*tensors) or any(t.device != image.device for t in tensors):
        raise Fallback(OFF_GPU)
    if any(t.requires_grad for t in tensors):
        raise Fallback(NEEDS_GRAD)
    if (tuple(image.shape[1:3]) != tuple(mask.shape[1:]) or int(image.shape[3]) != 3 or tuple(background.shape) != (3,)
            or (mask_ignore is not None and tuple(mask_ignore.shape) != tuple(mask.shape))):
        raise Fallback(SHAPES)
    if getattr(model, "view_correction", None) is not None and model.training:
        raise Fallback("render_correct in output")
    if not _loss._modules_covered(self):
        raise Fallback("loss modules the kernels do not cover")
    return image, mask, mask_ignore, background


@dropins.register
def forward(self, batch, model):
    """MaskForeground.forward (renderer.py:343-373): bounds by one kernel and one read-back, crops as views, the composite
    and the blend inside ONE loss call, one read-back for loss_dict."""
    dropins.count("calls", "forward")
    if self.split != "train":
        return self.vis(batch, model)
    try:
        image, mask, mask_ignore, background = _forward_inputs(self, batch, model)
        H, W = int(mask.shape[1]), int(mask.shape[2])
        padding = int(max(tuple(mask.shape) + (1,)) / 50)         # msk = batch['mask'][..., None] in the reference
        l, t, r, b = mask_bounds_host(mask, padding)
        dropins.count("readbacks", "forward")
        if min(b + 1, H) - t < _loss.WINDOW or min(r + 1, W) - l < _loss.WINDOW:
            raise Fallback("a crop under 11 pixels")
    except Fallback as why:
        return dropins.fall_back("forward", why, self, batch, model)
    rand_bkgd = torch.rand(3, device=image.device) if self.use_randback else background
    output = self.vis(batch, model, background=rand_bkgd)
    render = output["render"][:, :3]
    if ("render_correct" in output.keys() or not _loss._fusable(render) or render.device != image.device
            or tuple(render.shape) != (1, 3, H, W)):
        # Nothing checked above predicts this, the background is drawn and the view rendered: the reference's method would
        # draw and render again, another random stream than an unpatched run's.  An error, not a fall-back.
        raise _lib.LograstError(
            "log_amd.masked_loss: vis() returned " +
            ("'render_correct'" if "render_correct" in output.keys() else
             f"a render {getattr(render, 'dtype', None)} {tuple(getattr(render, 'shape', ()))} on "
             f"{getattr(render, 'device', None)}") +
            f" where a float32 render [1, >=3, {H}, {W}] on {image.device} without view correction was expected; "
            "uninstall log_amd.masked_loss for this configuration")
    render = render[:, :, t:b + 1, l:r + 1]
    gt = image.permute(0, 3, 1, 2)[:, :, t:b + 1, l:r + 1]
    fg = mask[:, t:b + 1, l:r + 1]
    if mask_ignore is not None:
        mask_ignore = mask_ignore[:, t:b + 1, l:r + 1]
    loss, values, gt_used = _fused_masked(render, gt, mask_ignore, fg, rand_bkgd, None, None, 0.2, 0.8)
    _loss._publish(output, loss, values)
    dropins.count("readbacks", "forward")
    if mask_ignore is not None:
        output["mask_ignore"] = mask_ignore
    output["gt"] = gt_used
    output["render"] = render
    return output


# ---- installation ----------------------------------------------------------------------------------------------------

_underneath = _loss.Underneath()
_was_enabled = None


def install():
    """Patch the reference in place (needs LoG importable): log_amd.loss first (where nothing of this package is installed
    as calculate_loss yet), the switch on, then the two MaskForeground methods -> MaskForeground."""
    global _was_enabled
    _underneath.install(_targets()["forward"][0])
    if _was_enabled is None:
        _was_enabled = enabled()
    set_enabled(True)
    return dropins.install()["forward"][0]


def uninstall():
    """Put back what install() replaced, the switch as it was, and log_amd.loss where install() installed it."""
    global _was_enabled
    dropins.uninstall()
    dropins._saved.clear()
    if _was_enabled is not None:
        set_enabled(_was_enabled)
        _was_enabled = None
    _underneath.uninstall()

"""The photometric training loss of LoG on the device: ``0.2 * (1 - SSIM) + 0.8 * L1`` as
LoG/render/renderer.py:253-266 (``calculate_loss``) and LoG/render/loss.py:6-44 (``SSIM``) compute it, in one forward
kernel + a fixed-order reduction and one backward kernel (log_amd/csrc/loss.hip, C ABI ``lograst_loss_*``) instead of
five grouped ``conv2d``, a dozen element-wise kernels and their autograd backward.

* ``l1_ssim_loss(render, gt, render_l1=None, ssim_weight=0.2, l1_weight=0.8, l1_gain=None) -> (loss, l1, ssim)``;
  ``l1_gain`` [B, C] puts the L1 term on ``l1_gain[b, c] * render`` inside the kernels (LoG's view correction without its
  ``render_correct`` image: C ABI ``lograst_loss_*_gain``, one image gradient and the gradient of the gain)
* ``ssim(img1, img2)`` = what ``SSIM(11, C).forward(img1, img2)`` returns (``1 - mean(ssim_map)``)
* ``install()`` assigns drop-ins onto the reference's classes (``SSIM.forward``, ``NaiveRendererAndLoss.calculate_loss``);
  ``log_amd.install_all(fused_loss=True)`` calls it.

Tensors are read through their strides (the channels-last ``batch['image'].permute(0, 3, 1, 2)`` LoG passes as ``gt`` is
not copied); results and gradients are bit-identical from run to run; nothing is read back to the host, so forward and
backward can be captured in a HIP graph."""
import ctypes
import math

import torch

from . import _lib
from .rasterizer import _ptr, _stream_ptr

WINDOW = 11          # taps of the SSIM window (sigma 1.5), the only size the kernel has
TILE = 32            # output pixels per workgroup tile side (loss.hip: LS_T)
GAIN_REDUCE_THREADS = 256    # threads that add one plane's partial sums of the gain gradient (loss.hip: LS_GAIN_RED_THREADS)


def window_taps():
    """The 11 fp32 window weights exactly as the library computes them: exp(-(x-5)^2 / (2 * 1.5^2)) in double,
    normalised in double, rounded to fp32 once.  -> float32 tensor [11] (CPU)."""
    g = [math.exp(-float((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)) for k in range(WINDOW)]
    s = 0.0
    for v in g:
        s += v
    return torch.tensor([v / s for v in g], dtype=torch.float64).to(torch.float32)


def _strides(t):
    """The element strides of an image [B, C, H, W] or a mask [B, H, W] as the library reads them; None for no tensor."""
    return None if t is None else (ctypes.c_int64 * t.dim())(*t.stride())


def _require(render, gt, render_l1):
    for name, t in (("render", render), ("gt", gt), ("render_l1", render_l1)):
        if t is None:
            continue
        if t.device.type != "cuda":
            raise _lib.LograstError(
                f"log_amd.loss needs tensors on the MI355X ({name} is on '{t.device}'); the HIP kernels are the only "
                "implementation -- there is no CPU fallback")
        if t.dtype != torch.float32 or t.dim() != 4:
            raise ValueError(f"{name}: expected a float32 tensor [B, C, H, W], got {t.dtype} {tuple(t.shape)}")
        if t.shape != render.shape or t.device != render.device:
            raise ValueError(f"{name}: shape {tuple(t.shape)} on {t.device} does not match render {tuple(render.shape)} on {render.device}")
    return _lib.lib()


def _require_mask(module, name, t, render):
    B, _, H, W = render.shape
    if not torch.is_tensor(t) or t.device != render.device:
        raise ValueError(f"{name}: expected a tensor on {render.device}")
    if t.dtype != torch.float32 or tuple(t.shape) != (B, H, W):
        raise ValueError(f"{name}: expected a float32 tensor [{B}, {H}, {W}], got {t.dtype} {tuple(t.shape)}")
    if t.requires_grad:
        raise _lib.LograstError(f"log_amd.{module}: {name} gets no gradient (detach it)")
    return t.detach()


def _require_gain(gain, B, C, device):
    if not torch.is_tensor(gain) or gain.device != device or gain.dtype != torch.float32 or tuple(gain.shape) != (B, C):
        raise ValueError(f"l1_gain: expected a float32 tensor [{B}, {C}] on {device}, got "
                         f"{getattr(gain, 'dtype', type(gain))} {tuple(getattr(gain, 'shape', ()))}")
    return gain.detach().contiguous()


def _call_forward(L, dims, r, g, rl, k, m, f, bg, gt_out, weights, out, maps):
    """The forward entry point the inputs ask for, on fresh scratch of its own sizing function: a mask or a foreground takes
    the masked one, else a gain the gain one, else the plain one."""
    if m is not None or f is not None:
        size, entry = L.lograst_loss_masked_scratch_bytes, L.lograst_loss_forward_masked
        own = (_ptr(rl), _strides(rl), _ptr(g), _strides(g), _ptr(k), _ptr(m), _strides(m), _ptr(f), _strides(f), _ptr(bg),
               _ptr(gt_out))
    elif k is not None:
        size, entry = L.lograst_loss_gain_scratch_bytes, L.lograst_loss_forward_gain
        own = (_ptr(g), _strides(g), _ptr(k))
    else:
        size, entry = L.lograst_loss_scratch_bytes, L.lograst_loss_forward
        own = (_ptr(rl), _strides(rl), _ptr(g), _strides(g))
    nbytes = size(*dims)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=r.device)
    with torch.cuda.device(r.device):
        _lib.check(entry(*dims, _ptr(r), _strides(r), *own, *weights, _ptr(out), _ptr(maps), _ptr(scratch), nbytes,
                         _stream_ptr(r.device)))


def _call_backward(L, dims, l1_weight, r, g, rl, k, m, gl, maps, g_render, g_l1, g_gain):
    """The backward entry point: an ignore mask takes the masked one, else a gain the gain one, else the plain one -- after a
    foreground alone too, where ``g`` is the composited ground truth.  Scratch only with a gain."""
    nbytes, scratch = 0, None
    if k is not None:
        nbytes = (L.lograst_loss_gain_scratch_bytes if m is None else L.lograst_loss_masked_scratch_bytes)(*dims)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=r.device)
    head = (*dims, _ptr(r), _strides(r))
    grads = (l1_weight, _ptr(gl), _ptr(maps), _ptr(g_render))
    with torch.cuda.device(r.device):
        stream = _stream_ptr(r.device)
        if m is not None:
            rc = L.lograst_loss_backward_masked(*head, _ptr(rl), _strides(rl), _ptr(g), _strides(g), _ptr(k), _ptr(m), _strides(m),
                                                *grads, _ptr(g_l1), _ptr(g_gain), _ptr(scratch), nbytes, stream)
        elif k is not None:
            rc = L.lograst_loss_backward_gain(*head, _ptr(g), _strides(g), _ptr(k), *grads, _ptr(g_gain), _ptr(scratch), nbytes,
                                              stream)
        else:
            rc = L.lograst_loss_backward(*head, _ptr(rl), _strides(rl), _ptr(g), _strides(g), *grads, _ptr(g_l1), stream)
        _lib.check(rc)


# How a gt that wants a gradient is refused differs between the two modules, and callers may rely on either: log_amd.loss asks
# autograd (ctx.needs_input_grad), log_amd.masked_loss the tensor (gt.requires_grad) -- torch does not promise that the two
# agree in every grad mode -- and each message names its module.  So the caller hands in its name and its rule: (module, the
# tensor is asked).
FROM_LOSS, FROM_MASKED_LOSS = ("loss", False), ("masked_loss", True)


class _L1SSIM(torch.autograd.Function):
    """The loss in all its forms -- an ignore mask, a foreground composite over a background, render_l1 or a gain for the L1
    term, each None where absent: gradients for render, render_l1 and the gain.  -> (loss, stats [l1, ssim], composited gt or
    None)."""

    @staticmethod
    def forward(ctx, render, gt, mask, foreground, background, render_l1, gain, ssim_weight, l1_weight, caller):
        L = _require(render, gt, render_l1)
        module, ask_tensor = caller
        if gt.requires_grad if ask_tensor else ctx.needs_input_grad[1]:
            raise _lib.LograstError(f"log_amd.{module}: gt gets no gradient (detach it)")
        device = render.device
        dims = B, C, H, W = tuple(int(s) for s in render.shape)
        m = None if mask is None else _require_mask(module, "mask", mask, render)
        f = None if foreground is None else _require_mask(module, "foreground", foreground, render)
        bg = None
        if f is not None:
            if (not torch.is_tensor(background) or background.device != device or background.dtype != torch.float32
                    or tuple(background.shape) != (C,)):
                raise ValueError(f"background: expected a float32 tensor [{C}] on {device} with a foreground mask")
            if background.requires_grad:
                raise _lib.LograstError(f"log_amd.{module}: background gets no gradient (detach it)")
            bg = background.detach().contiguous()
        k = None if gain is None else _require_gain(gain, B, C, device)
        r, g = render.detach(), gt.detach()
        rl = None
        if render_l1 is not None:
            rl = render_l1.detach()
            if rl.data_ptr() == r.data_ptr() and rl.stride() == r.stride():
                rl = None
        need_grad = any(ctx.needs_input_grad[i] for i in (0, 5, 6))
        out = torch.empty(3, dtype=torch.float32, device=device)
        nmaps = 3 * B * C * max(H - WINDOW + 1, 0) * max(W - WINDOW + 1, 0)
        maps = torch.empty(nmaps, dtype=torch.float32, device=device) if need_grad else None
        gt_out = torch.empty(dims, dtype=torch.float32, device=device) if f is not None else None
        _call_forward(L, dims, r, g, rl, k, m, f, bg, gt_out, (float(ssim_weight), float(l1_weight)), out, maps)
        ctx.geom = (dims, float(l1_weight))
        ctx.tensors = (r, gt_out if gt_out is not None else g, rl, k, m, maps)
        ctx.l1_is_input = render_l1 is not None
        loss, stats = out[0], out[1:3]
        if gt_out is None:
            ctx.mark_non_differentiable(stats)
        else:
            ctx.mark_non_differentiable(stats, gt_out)
        return loss, stats, gt_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_stats, _grad_gt):
        dims, l1_weight = ctx.geom
        r, g, rl, k, m, maps = ctx.tensors
        device = r.device
        gl = grad_loss.detach().to(device=device, dtype=torch.float32).reshape(1).contiguous()
        g_render = torch.empty(dims, dtype=torch.float32, device=device)
        g_l1 = torch.empty(dims, dtype=torch.float32, device=device) if rl is not None else None
        g_gain = torch.zeros(dims[:2], dtype=torch.float32, device=device) if k is not None else None
        _call_backward(_lib.lib(), dims, l1_weight, r, g, rl, k, m, gl, maps, g_render, g_l1, g_gain)
        if rl is None and ctx.l1_is_input:
            g_l1 = None          # render_l1 was render itself: its L1 term is already in g_render
        return (g_render if ctx.needs_input_grad[0] else None, None, None, None, None,
                g_l1 if ctx.l1_is_input and ctx.needs_input_grad[5] else None,
                g_gain if k is not None and ctx.needs_input_grad[6] else None, None, None, None)


def _fused_gain(render, gt, gain, ssim_weight, l1_weight):
    return _L1SSIM.apply(render, gt, None, None, None, None, gain, ssim_weight, l1_weight, FROM_LOSS)[:2]


def _fused(render, gt, render_l1, ssim_weight, l1_weight):
    if render_l1 is render:
        render_l1 = None
    return _L1SSIM.apply(render, gt, None, None, None, render_l1, None, ssim_weight, l1_weight, FROM_LOSS)[:2]


def l1_ssim_loss(render, gt, render_l1=None, ssim_weight=0.2, l1_weight=0.8, l1_gain=None):
    """-> (loss, l1, ssim): ``loss = ssim_weight * ssim + l1_weight * l1`` carries the graph (gradients for ``render`` and,
    when it is a tensor of its own, ``render_l1``); ``l1 = mean|render_l1 - gt|`` and ``ssim = 1 - mean(ssim_map(render,
    gt))`` are detached 0-dim views of the same device buffer.  All tensors [B, C, H, W] float32 on the device, any
    strides; H, W >= 11.
    ``l1_gain`` (float32 [B, C] on the device, instead of ``render_l1``): ``l1 = mean|l1_gain[b, c] * render - gt|``, the
    product taken inside the kernels; gradients for ``render`` (one image) and for ``l1_gain``."""
    if l1_gain is not None:
        if render_l1 is not None:
            raise ValueError("l1_gain and render_l1 are mutually exclusive: the L1 term reads one of them")
        loss, stats = _fused_gain(render, gt, l1_gain, ssim_weight, l1_weight)
        return loss, stats[0], stats[1]
    loss, stats = _fused(render, gt, render_l1, ssim_weight, l1_weight)
    return loss, stats[0], stats[1]


def ssim(img1, img2):
    """``SSIM(11, C).forward(img1, img2, reduce=True)``: 1 - mean(ssim_map)."""
    return _fused(img1, img2, None, 1.0, 0.0)[0]


# ---- drop-ins for an unmodified LoG checkout ------------------------------------------------------------------------

def _fusable(*tensors):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in tensors)


def _make_ssim_forward(original):
    def forward(self, img1, img2, reduce=True):
        if (reduce and self.window_size == WINDOW and getattr(self, "padding", 0) == 0 and _fusable(img1, img2)
                and img1.shape == img2.shape and not img2.requires_grad):
            return ssim(img1, img2)
        return original(self, img1, img2, reduce)
    forward._lograst_original = original
    return forward


def _modules_covered(self):
    """The renderer's loss modules are the ones the kernels compute: SSIM(11) without padding and a mean L1Loss."""
    ssim_mod = getattr(self, "ssim_loss", None)
    return (getattr(ssim_mod, "window_size", None) == WINDOW and getattr(ssim_mod, "padding", 0) == 0
            and isinstance(getattr(self, "l1_loss", None), torch.nn.L1Loss) and self.l1_loss.reduction == "mean")


def _publish(output, loss, stats):
    """How every calculate_loss of this package ends: ONE read-back for loss_dict; the loss keeps its graph."""
    l1_value, ssim_value = stats.tolist()
    output["loss_dict"] = {"l1": l1_value, "ssim": ssim_value}
    output["loss"] = loss


_masked_branch = None     # log_amd.masked_loss.set_enabled(True) puts its mask_ignore branch here; None: the torch blend below


def _make_calculate_loss(original):
    def calculate_loss(self, gt_image, render, output, mask_ignore=None):
        """renderer.py:253-266 with the two losses in one kernel and ONE read-back for loss_dict."""
        if not (_fusable(gt_image, render) and gt_image.shape == render.shape and not gt_image.requires_grad
                and _modules_covered(self)):
            return original(self, gt_image, render, output, mask_ignore)
        if mask_ignore is not None:
            if _masked_branch is not None and _masked_branch(gt_image, render, output, mask_ignore):
                return
            render = gt_image * mask_ignore[:, None] + render * (1 - mask_ignore[:, None])
        render_l1 = output["render_correct"][:, :3] if "render_correct" in output.keys() else render
        if not (_fusable(render_l1) and render_l1.shape == render.shape):
            return original(self, gt_image, render, output, None)     # (the blend is already applied)
        _publish(output, *_fused(render, gt_image, render_l1, 0.2, 0.8))
    calculate_loss._lograst_original = original
    return calculate_loss


def install(renderer=True):
    """Patch the reference in place (needs LoG importable): SSIM.forward, and -- when LoG.render.renderer can be
    imported (it needs cv2) -- NaiveRendererAndLoss.calculate_loss (MaskForeground inherits it).  Calls the kernels do not
    cover (reduce=False, another window, CPU tensors) go to the methods that were replaced."""
    from LoG.render.loss import SSIM
    if not hasattr(SSIM.forward, "_lograst_original"):
        SSIM.forward = _make_ssim_forward(SSIM.forward)
    if renderer:
        try:
            import LoG.render.renderer as rr
        except ImportError:
            rr = None
        if rr is not None and not hasattr(rr.NaiveRendererAndLoss.calculate_loss, "_lograst_original"):
            rr.NaiveRendererAndLoss.calculate_loss = _make_calculate_loss(rr.NaiveRendererAndLoss.calculate_loss)
    return SSIM


def uninstall():
    """Put back what install() replaced."""
    import sys
    mod = sys.modules.get("LoG.render.loss")
    if mod is not None and hasattr(mod.SSIM.forward, "_lograst_original"):
        mod.SSIM.forward = mod.SSIM.forward._lograst_original
    rr = sys.modules.get("LoG.render.renderer")
    if rr is not None and hasattr(rr.NaiveRendererAndLoss.calculate_loss, "_lograst_original"):
        rr.NaiveRendererAndLoss.calculate_loss = rr.NaiveRendererAndLoss.calculate_loss._lograst_original


class Underneath:
    """For a module whose drop-ins stand on this one's calculate_loss (masked_loss, view_correction): its install() gets
    install() here first, unless something of this package already stands as the renderer's calculate_loss, and its
    uninstall() takes this module away again only where it was this object that put it there."""

    def __init__(self):
        self.installed = False

    def install(self, renderer):
        standing = renderer.calculate_loss
        if not hasattr(standing, "_lograst_original") and not getattr(standing, "__module__", "").startswith("log_amd."):
            install()
            self.installed = True

    def uninstall(self):
        if self.installed:
            uninstall()
            self.installed = False

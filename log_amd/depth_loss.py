"""The depth term of LoG's depth-supervised training on the device: what LoG/render/renderer.py:268-292
(``append_depth_loss``) and LoG/render/loss.py:47-117 (``ScaleAndShiftInvariantLoss``, alpha 0.5, one gradient scale)
compute for 64 patches of 64 x 64 pixels, in one forward kernel + a fixed-order sum and one backward kernel
(log_amd/csrc/depth_loss.hip, C ABI ``lograst_depth_loss_*``) instead of 384 read-backs of slice bounds, three stacked
``[64, 64, 64]`` tensors, about sixty small kernels and their autograd backward.

* ``depth_patch_loss(pred_depth, gt_depth, accmap, rows, cols, alpha=0.5, eps=1e-5, threshold=0.5) -> loss``
* ``append_depth_loss(gt_depth, pred_depth, output, generator=None)`` = the reference's method as a plain function
* ``install()`` assigns a drop-in onto ``NaiveRendererAndLoss.append_depth_loss``;
  ``log_amd.install_all(fused_depth_loss=True)`` calls it.

All arithmetic inside the kernels is double (the reference's fp32 determinant cancels on patches of nearly constant
depth); inputs and outputs are fp32 and are read through their strides.  The patch positions stay on the device, nothing
is read back to the host, results and gradients are bit-identical from run to run, and forward and backward can be
captured in a HIP graph."""
import ctypes

import torch

from . import _lib
from .rasterizer import _ptr, _stream_ptr

PATCH = 64           # the patch side, the only one the kernels have (depth_loss.hip: DL_PATCH)
NUM_PATCHES = 64     # what the reference draws per view
MAX_PATCHES = 256


def _strides(t):
    return (ctypes.c_int64 * 2)(*t.stride())


def _require(pred, gt, acc, rows, cols):
    for name, t in (("pred_depth", pred), ("gt_depth", gt), ("accmap", acc), ("rows", rows), ("cols", cols)):
        if t.device.type != "cuda":
            raise _lib.LograstError(
                f"log_amd.depth_loss needs tensors on the MI355X ({name} is on '{t.device}'); the HIP kernels are the only "
                "implementation -- there is no CPU fallback")
        if t.device != pred.device:
            raise ValueError(f"{name} is on {t.device}, pred_depth on {pred.device}")
    for name, t in (("pred_depth", pred), ("gt_depth", gt), ("accmap", acc)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape != pred.shape:
            raise ValueError(f"{name}: expected a float32 tensor [H, W] like pred_depth {tuple(pred.shape)}, got {t.dtype} {tuple(t.shape)}")
    for name, t in (("rows", rows), ("cols", cols)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.shape != rows.shape:
            raise ValueError(f"{name}: expected an int64 tensor [n], got {t.dtype} {tuple(t.shape)}")
    H, W = (int(s) for s in pred.shape)
    n = int(rows.shape[0])
    if H < PATCH or W < PATCH:
        raise ValueError(f"image {H} x {W} is smaller than the {PATCH}-pixel patch")
    if not 1 <= n <= MAX_PATCHES:
        raise ValueError(f"1 .. {MAX_PATCHES} patches per call, got {n}")
    return _lib.lib()


class _DepthPatchLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, acc, rows, cols, alpha, eps, threshold):
        L = _require(pred, gt, acc, rows, cols)
        if ctx.needs_input_grad[1]:
            raise _lib.LograstError("log_amd.depth_loss: gt_depth gets no gradient (detach it)")
        # (accmap is LoG's rendered accumulation channel and does carry a graph: it is only thresholded, as in the
        # reference, so nothing flows back into it)
        device = pred.device
        H, W = (int(s) for s in pred.shape)
        n = int(rows.shape[0])
        p, g, a = pred.detach(), gt.detach(), acc.detach()
        rows, cols = rows.contiguous(), cols.contiguous()
        out = torch.empty(2, dtype=torch.float64, device=device)          # float loss at byte 0, double M at byte 8
        nbytes = L.lograst_depth_loss_record_bytes(n)
        records = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_depth_loss_forward(
                H, W, _ptr(p), _strides(p), _ptr(g), _strides(g), _ptr(a), _strides(a), n, _ptr(rows), _ptr(cols),
                float(alpha), float(eps), float(threshold), _ptr(out), _ptr(records), nbytes, _stream_ptr(device)))
        ctx.geom = (H, W, n)
        ctx.tensors = (p, g, a, records)
        return out.view(torch.float32)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        H, W, n = ctx.geom
        p, g, a, records = ctx.tensors
        device = p.device
        L = _lib.lib()
        gl = grad_loss.detach().to(device=device, dtype=torch.float32).reshape(1).contiguous()
        grad_pred = torch.empty((H, W), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_depth_loss_backward(
                H, W, _ptr(p), _strides(p), _ptr(g), _strides(g), _ptr(a), _strides(a), n, _ptr(records), _ptr(gl),
                _ptr(grad_pred), _stream_ptr(device)))
        return grad_pred, None, None, None, None, None, None, None


def depth_patch_loss(pred_depth, gt_depth, accmap, rows, cols, alpha=0.5, eps=1e-5, threshold=0.5):
    """-> loss, a 0-dim float32 tensor that carries the graph to ``pred_depth`` only.

    pred_depth, gt_depth, accmap: [H, W] float32 on the device, any strides, H, W >= 64; rows, cols: [n] int64 on the
    device, 1 <= n <= 256 -- the upper-left corners of the 64 x 64 patches (never read by the host).  With
    m = accmap > threshold and p = 1 / (pred_depth + eps), per patch (s, h) = argmin sum m (s p + h - gt)^2 and
    loss = (sum m (s p + h - gt)^2 + alpha * sum over neighbour pairs inside a patch of m m' |d' - d|) / sum m, the sums
    over all patches.  No valid pixel at all, or a patch that does not lie inside the image: nan."""
    return _DepthPatchLoss.apply(pred_depth, gt_depth, accmap, rows, cols, alpha, eps, threshold)


def append_depth_loss(gt_depth, pred_depth, output, generator=None):
    """renderer.py:268-292 as a plain function: 64 patch positions drawn on the device (rows, then columns, as the
    reference draws them, so the device generator advances as it does there), the fused loss, and the keys the reference
    sets: output['gt_depth'], output['pred_depth'] (normalised inverse depth for display, without the read-backs of
    boolean indexing), output['loss_dict']['depth'] (the tensor) and output['loss'] += loss."""
    accmap = output["accmap"][0]
    gt, pred = gt_depth[0], pred_depth[0]
    H, W = (int(s) for s in gt.shape)
    rows = torch.randint(0, H - PATCH, (NUM_PATCHES,), device=gt.device, generator=generator)
    cols = torch.randint(0, W - PATCH, (NUM_PATCHES,), device=gt.device, generator=generator)
    loss = depth_patch_loss(pred, gt, accmap, rows, cols)
    output["gt_depth"] = gt[None]
    mask = accmap > 0.5
    vis = 1. / (pred.detach() + 1e-5)
    lo = torch.where(mask, vis, torch.full_like(vis, float("inf"))).amin()
    hi = torch.where(mask, vis, torch.full_like(vis, float("-inf"))).amax()
    output["pred_depth"] = ((vis - lo) / (hi - lo))[None]
    output["loss_dict"]["depth"] = loss
    output["loss"] = output["loss"] + loss
    return output


# ---- drop-in for an unmodified LoG checkout -------------------------------------------------------------------------

def _fusable(self, gt_depth, pred_depth, output):
    mod = getattr(self, "depth_loss", None)
    if type(mod).__name__ != "ScaleAndShiftInvariantLoss" or type(mod).__module__ != "LoG.render.loss":
        return False
    if getattr(mod, "alpha", None) != 0.5 or getattr(getattr(mod, "regularization_loss", None), "scales", None) != 1:
        return False
    acc = output.get("accmap") if hasattr(output, "get") else None
    tensors = (gt_depth, pred_depth, acc)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 for t in tensors):
        return False
    H, W = gt_depth.shape[1:]
    return H > PATCH and W > PATCH and pred_depth.shape[1:] == (H, W) and acc.shape[1:] == (H, W) and not gt_depth.requires_grad


def _make_append_depth_loss(original):
    def wrapper(self, gt_depth, pred_depth, output):
        if not _fusable(self, gt_depth, pred_depth, output):
            return original(self, gt_depth, pred_depth, output)
        return append_depth_loss(gt_depth, pred_depth, output)
    wrapper.__name__ = "append_depth_loss"
    wrapper._lograst_original = original
    return wrapper


def install():
    """Patch the reference in place (needs LoG.render.renderer importable): NaiveRendererAndLoss.append_depth_loss
    (MaskForeground inherits it).  Calls the kernels do not cover (CPU or non-fp32 tensors, images of 64 pixels or less,
    another depth loss than ScaleAndShiftInvariantLoss(alpha=0.5, scales=1)) go to the method that was replaced."""
    import LoG.render.renderer as rr
    cls = rr.NaiveRendererAndLoss
    if not hasattr(cls.append_depth_loss, "_lograst_original"):
        cls.append_depth_loss = _make_append_depth_loss(cls.append_depth_loss)
    return cls


def uninstall():
    """Put back what install() replaced."""
    import sys
    rr = sys.modules.get("LoG.render.renderer")
    if rr is not None and hasattr(rr.NaiveRendererAndLoss.append_depth_loss, "_lograst_original"):
        rr.NaiveRendererAndLoss.append_depth_loss = rr.NaiveRendererAndLoss.append_depth_loss._lograst_original

"""Drop-ins for LoG's per-view colour correction (``use_view_correction: True``, both example configurations): the
``Corrector`` of LoG/model/corrector.py and the place its gain meets the loss, LoG/render/renderer.py:243-266.

* ``Corrector.step`` (corrector.py:35-62) becomes ONE launch of one wave (``lograst_corrector_step``, csrc/counter.hip): the
  step count of the row, the early return before ``start_step``, the learning-rate schedule, the AMSGrad update and the
  zeroing of the row's gradient, all on the device.  The reference indexes nine times with a Python list, tests a device
  tensor in an ``if``, calls ``.item()`` and runs about fifteen element-wise launches on three floats; here nothing comes
  back to the host.
* ``Corrector.__getitem__`` keeps ``self.index = index`` and returns the same differentiable row; it also notes the row as
  handed out.
* ``NaiveRendererAndLoss.calculate_loss`` is wrapped around whatever is installed there (``install()`` installs
  ``log_amd.loss`` first).  When ``'render_correct'`` is in ``output`` and exactly ``B`` rows were handed out since the
  previous loss call, the loss kernels take ``l1_gain = stack(rows)`` and the plain ``render``
  (``log_amd.loss.l1_ssim_loss(..., l1_gain=)``): ``render_correct`` is not read, its multiply gets no backward, and there
  is one image gradient instead of two and their sum.  ``view_correction.grad`` comes out dense ``[V, 3]`` with the
  gradient in the handed-out rows, as the reference leaves it.  A ``mask_ignore`` blend goes to the SSIM input only, as in
  the reference: the SSIM term then comes from the kernels without gain on the blend, the L1 term from the kernels with
  gain on the plain render -- or, with ``log_amd.masked_loss.set_enabled(True)``, both from ONE call of the masked kernels
  with gain and mask.

What this does not cover goes to the method that was there before ``install()``, counted by reason in ``stats()``:
``step`` for tensors off the GPU or not float32 (or not contiguous), ``use_amsgrad`` false, ``view_correction.grad is None``
and a ``self.index`` that is no integer in ``[0, V)``; ``calculate_loss`` for a missing ``render_correct``, a count of
handed-out rows other than ``B``, and shapes, devices or dtypes that do not fit.  The note of handed-out rows keeps the last
``MAX_NOTED`` rows and a count, so a ``vis`` that runs in training mode without a loss does not grow it.

Install with ``log_amd.view_correction.install()`` or ``log_amd.install_all(device_view_correction=True)``."""
import collections

import torch

from . import _lib
from . import loss as _loss
from . import masked_loss as _masked
from . import rasterizer as _r
from ._dropin import DropIns, Fallback

MAX_NOTED = 64          # rows kept between two loss calls: a batch of more views takes the wrapped method


def _targets():
    from LoG.model.corrector import Corrector
    from LoG.render.renderer import NaiveRendererAndLoss
    return {"step": (Corrector, "step"), "__getitem__": (Corrector, "__getitem__"),
            "calculate_loss": (NaiveRendererAndLoss, "calculate_loss")}


dropins = DropIns("view_correction", _targets)
stats, reset_stats = dropins.stats, dropins.reset_stats


class _HandedOut:
    """The rows ``Corrector.__getitem__`` returned since the previous loss call: how many, and the last MAX_NOTED of them."""

    def __init__(self):
        self.count, self.rows = 0, collections.deque(maxlen=MAX_NOTED)

    def note(self, row):
        self.count += 1
        self.rows.append(row)

    def take(self):
        count, rows = self.count, list(self.rows)
        self.count = 0
        self.rows.clear()
        return count, rows


handed_out = _HandedOut()


# ---- Corrector -------------------------------------------------------------------------------------------------------

def _state(t, device, dtype, shape):
    if not torch.is_tensor(t) or t.device != device:
        raise Fallback("tensors are not on the GPU")
    if t.dtype != dtype:
        raise Fallback("tensors are not float32" if dtype == torch.float32 else "the step counts are not int32")
    if tuple(t.shape) != shape or not t.is_contiguous():
        raise Fallback("buffers are not contiguous [V, C]")
    return t


@dropins.dropin
def step(self):
    """Corrector.step on the device: one launch, nothing read back (returns None where the reference returns 0 before
    ``start_step``: the host does not know)."""
    if not self.use_view_correction:
        return 0
    param = self.view_correction
    if param.device.type != "cuda":
        raise Fallback("tensors are not on the GPU")
    if param.dtype != torch.float32:
        raise Fallback("tensors are not float32")
    opt = self.optimizer
    if not (self.use_amsgrad and getattr(opt, "use_amsgrad", False)):
        raise Fallback("use_amsgrad is off")
    if param.grad is None:
        raise Fallback("view_correction.grad is None")
    if param.dim() != 2 or not 1 <= int(param.shape[1]) <= 64:
        raise Fallback("buffers are not contiguous [V, C]")
    V, C = int(param.shape[0]), int(param.shape[1])
    index = self.index
    if isinstance(index, bool) or not isinstance(index, int) or not 0 <= index < V:
        raise Fallback("index is not an integer in [0, V)")
    device = param.device
    data = _state(param.data, device, torch.float32, (V, C))
    grad = _state(param.grad, device, torch.float32, (V, C))
    moments = [_state(getattr(opt, k)["view_correction"], device, torch.float32, (V, C))
               for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")]
    steps = _state(opt.steps["view_correction"], device, torch.int32, (V,))
    lr_init, lr_final, start = float(self.lr_init), float(self.lr_final), int(self.start_step)
    if not (0.0 < lr_init < float("inf") and 0.0 < lr_final < float("inf")) or not -2 ** 31 <= start < 2 ** 31:
        raise Fallback("a learning rate that is not positive and finite")
    L = _lib.lib()
    with torch.cuda.device(device):
        _lib.check(L.lograst_corrector_step(V, C, index, start, lr_init, lr_final, _r._ptr(steps), _r._ptr(data),
                                            _r._ptr(grad), *(_r._ptr(m) for m in moments), _r._stream_ptr(device)))


@dropins.register
def __getitem__(self, index):
    """Corrector.__getitem__: the reference's method, its result noted as handed out."""
    dropins.count("calls", "__getitem__")
    row = dropins.original("__getitem__")(self, index)
    handed_out.note(row)
    return row


# ---- NaiveRendererAndLoss.calculate_loss -----------------------------------------------------------------------------

def _gain(self, gt_image, render, output, count, rows):
    """-> l1_gain [B, C] for the fused path, or raises Fallback."""
    if "render_correct" not in output.keys():
        raise Fallback("no render_correct in output")
    if not (_loss._fusable(gt_image, render) and gt_image.shape == render.shape and gt_image.device == render.device
            and not gt_image.requires_grad and _loss._modules_covered(self)):
        raise Fallback("tensors or loss modules the kernels do not cover")
    B, C = int(render.shape[0]), int(render.shape[1])
    if count != B or len(rows) != B:
        raise Fallback("rows handed out since the last loss are not one per image")
    if not all(torch.is_tensor(r) and r.device == render.device and r.dtype == torch.float32 and tuple(r.shape) == (C,)
               for r in rows):
        raise Fallback("handed-out rows do not fit the render")
    return torch.stack(rows)


@dropins.register
def calculate_loss(self, gt_image, render, output, mask_ignore=None):
    """renderer.py:253-266 with the gain inside the loss kernels and ONE read-back for loss_dict."""
    dropins.count("calls", "calculate_loss")
    count, rows = handed_out.take()
    try:
        gain = _gain(self, gt_image, render, output, count, rows)
    except Fallback as why:
        return dropins.fall_back("calculate_loss", why, self, gt_image, render, output, mask_ignore)
    if mask_ignore is None:
        loss, values = _loss._fused_gain(render, gt_image, gain, 0.2, 0.8)
    elif _masked.enabled() and _masked._mask_fits(mask_ignore, render):
        loss, values, _ = _masked._fused_masked(render, gt_image, mask_ignore, None, None, None, gain, 0.2, 0.8)
    else:
        blend = gt_image * mask_ignore[:, None] + render * (1 - mask_ignore[:, None])
        ssim = _loss._fused(blend, gt_image, None, 1.0, 0.0)[0]
        l1 = _loss._fused_gain(render, gt_image, gain, 0.0, 1.0)[0]
        loss = 0.2 * ssim + 0.8 * l1
        values = torch.stack([l1.detach(), ssim.detach()])
    _loss._publish(output, loss, values)
    dropins.count("readbacks", "calculate_loss")


# ---- installation ----------------------------------------------------------------------------------------------------

_underneath = _loss.Underneath()


def install():
    """Patch the reference classes in place (needs LoG importable): log_amd.loss first, then the three methods above, the
    loss wrapper around what is then installed as calculate_loss."""
    _underneath.install(_targets()["calculate_loss"][0])
    handed_out.take()
    return dropins.install()["step"][0]


def uninstall():
    """Put back what install() replaced (log_amd.loss too where install() installed it)."""
    dropins.uninstall()
    dropins._saved.clear()             # the next install() wraps what is installed then
    handed_out.take()
    _underneath.uninstall()

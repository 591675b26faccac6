"""The part of a LoG run that says how good the model is, on the device: what ``Trainer.make_validation``
(LoG/utils/trainer.py:298-364), ``LoG/utils/metric.py`` (``psnr``, ``ssim``) and ``BaseRender.tensor_to_bgr``
(LoG/render/renderer.py:19-23) compute per image, in the kernels of ``csrc/evaluate.hip`` (C ABI ``lograst_eval_*``,
``lograst_image_to_bgr8``) with ONE read-back of a 128-byte record -- instead of seven full-image reductions, an
``.item()`` and a float32 copy of the image to the host that numpy then converts on one CPU thread.

* ``image_to_bgr8(t) -> np.ndarray[H, W, C] uint8``: the bytes of ``tensor_to_bgr`` (for every input that is not a nan),
  converted on the device; H * W * C bytes cross to the host, through pinned memory.
* ``validation_metrics(pred, gt, fit_gain=False, ssim=False, max_val=1.0, corrected=False, bgr8=False) -> Metrics``: the
  view-correction fit over the left half, gain and clamp, L1, the squared error, the metric's SSIM (zero padding: not the
  training loss's) and, where asked, the corrected image and the 8-bit form of ``cat([corrected, gt], dim=1)``.
  ``Metrics.read()`` is the one synchronisation.
* ``install()`` / ``uninstall()`` / ``stats()`` / ``reset_stats()``: drop-ins for ``LoG.utils.metric.psnr``,
  ``LoG.utils.metric.ssim``, ``BaseRender.tensor_to_bgr`` and ``Trainer.make_validation``;
  ``log_amd.install_all(device_evaluate=True)`` calls ``install()``.

Images are fp32 ``[C, H, W]`` with 1 <= C <= 4 and are read through their strides (a permuted HWC image is read in
place).  Sums are double, added in a fixed order: the same input gives the same bits.  What the kernels do not cover --
tensors off the GPU, other dtypes, shapes that do not match, more than 4 channels, 2^31 elements or more, another SSIM
window than 11 taps of sigma 1.5, more than one image -- goes to the function that ``install()`` replaced, counted by
reason in ``stats()``.  LPIPS stays the torch network, the JPEG encoding stays cv2 on the CPU, and the ``batch['index']``
in the file name stays the reference's read-back."""
import ctypes
import math
import os
import sys
from collections import defaultdict

import torch

from . import _lib
from ._dropin import DropIns, Fallback
from .rasterizer import _ptr, _stream_ptr

MAX_CHANNELS = 4
SSIM_WINDOW, SSIM_SIGMA, SSIM_K1, SSIM_K2 = 11, 1.5, 0.01, 0.03


def _targets():
    """Where the drop-ins go; LoG.render.renderer needs cv2 and LoG.utils.trainer cv2 and tensorboardX: where one cannot
    be imported its targets are left out."""
    import LoG.utils.metric as metric
    targets = {"psnr": (metric, "psnr"), "ssim": (metric, "ssim")}
    try:
        from LoG.render.renderer import BaseRender
        targets["tensor_to_bgr"] = (BaseRender, "tensor_to_bgr")
    except ImportError:
        pass
    try:
        from LoG.utils.trainer import Trainer
        targets["make_validation"] = (Trainer, "make_validation")
    except ImportError:
        pass
    return targets


dropins = DropIns("evaluate", _targets)
install, uninstall, stats, reset_stats = dropins.install, dropins.uninstall, dropins.stats, dropins.reset_stats


# ---- the public functions ---------------------------------------------------------------------------------------------

def _strides(t):
    return (ctypes.c_int64 * 3)(*t.stride())


def _require(name, t, like=None):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        where = t.device if torch.is_tensor(t) else type(t).__name__
        raise _lib.LograstError(f"log_amd.evaluate needs tensors on the MI355X ({name} is on '{where}'); the HIP kernels are "
                                "the only implementation -- there is no CPU fallback")
    if t.dtype != torch.float32 or t.dim() != 3 or not 1 <= t.shape[0] <= MAX_CHANNELS or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"{name}: expected a float32 tensor [C, H, W] with 1 <= C <= {MAX_CHANNELS}, got {t.dtype} {tuple(t.shape)}")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{name}: 2^31 elements or more")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{name} is {tuple(t.shape)} on {t.device}, pred {tuple(like.shape)} on {like.device}")
    return t.detach()


def _to_host(dev):
    """A uint8 device tensor -> a numpy array of its own: one copy through a pinned buffer that the array keeps alive."""
    host = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(dev, non_blocking=True)
    torch.cuda.current_stream(dev.device).synchronize()
    return host.numpy()


def image_to_bgr8_device(t):
    """-> uint8 [H, W, C] on the device: channels reversed, each byte trunc(clip(x, 0, 1) * 255) in fp32."""
    t = _require("image", t)
    C, H, W = (int(s) for s in t.shape)
    out = torch.empty((H, W, C), dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().lograst_image_to_bgr8(C, H, W, _ptr(t), _strides(t), _ptr(out), _stream_ptr(t.device)))
    return out


def image_to_bgr8(t):
    """``BaseRender.tensor_to_bgr``: t float32 [C, H, W] on the device, any strides -> np.ndarray [H, W, C] uint8, a fresh
    array per call.  H * W * C bytes are copied to the host."""
    out = image_to_bgr8_device(t)
    with torch.cuda.device(out.device):
        return _to_host(out)


class Result:
    """What ``Metrics.read()`` returns: l1 = mean|p - gt|, mse, psnr = -10 log10(mse) (inf where mse == 0), ssim (the mean
    of the map, or None when it was not asked for), gain (the fitted fp32 gain per channel, 1.0 without the fit) and raw,
    the record's 16 doubles."""

    def __init__(self, raw, channels, with_ssim):
        self.raw = tuple(raw)
        n = self.raw[3]
        self.l1 = self.raw[0] / n
        self.mse = self.raw[1] / n
        self.psnr = math.inf if self.mse == 0 else (-10.0 * math.log10(self.mse) if self.mse > 0 else math.nan)
        self.ssim = self.raw[2] / n if with_ssim else None
        self.gain = list(self.raw[4:4 + channels])
        self.sum_gt_pred, self.sum_pred_pred = list(self.raw[8:8 + channels]), list(self.raw[12:12 + channels])


class Metrics:
    """One launch of ``validation_metrics``: ``record`` (float64 [16] on the device), ``corrected`` (float32 [C, H, W]) and
    ``bgr8`` (uint8 [2 H, W, C]) on the device where asked, else None.  Nothing has been synchronised until ``read()``."""

    def __init__(self, record, corrected, bgr8, channels, with_ssim):
        self.record, self.corrected, self.bgr8 = record, corrected, bgr8
        self._channels, self._with_ssim, self._result = channels, with_ssim, None

    def read(self):
        """-> Result; the first call copies the record to the host and synchronises the stream, later calls return it."""
        if self._result is None:
            out = (ctypes.c_double * 16)()
            with torch.cuda.device(self.record.device):
                _lib.check(_lib.lib().lograst_eval_read(_ptr(self.record), out, _stream_ptr(self.record.device)))
            self._result = Result(out, self._channels, self._with_ssim)
        return self._result

    def bgr8_host(self):
        """``bgr8`` as a numpy array of its own (2 H * W * C bytes to the host)."""
        with torch.cuda.device(self.bgr8.device):
            return _to_host(self.bgr8)


def validation_metrics(pred, gt, fit_gain=False, ssim=False, max_val=1.0, corrected=False, bgr8=False):
    """pred, gt: float32 [C, H, W] on the device, any strides, 1 <= C <= 4.  With ``fit_gain`` (trainer.py:313-317)
    gain[c] = sum(gt * pred) / sum(pred^2) over the columns [0, W // 2) and p = clamp(gain[c] * pred, 0, 1); without it
    p = pred, not clamped.  -> Metrics over p and gt; nothing is read back before its ``read()``."""
    pred = _require("pred", pred)
    gt = _require("gt", gt, like=pred)
    L = _lib.lib()
    device = pred.device
    C, H, W = (int(s) for s in pred.shape)
    record = torch.empty(16, dtype=torch.float64, device=device)
    nbytes = L.lograst_eval_scratch_bytes(C, H, W)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    out_corrected = torch.empty((C, H, W), dtype=torch.float32, device=device) if corrected else None
    out_bgr8 = torch.empty((2 * H, W, C), dtype=torch.uint8, device=device) if bgr8 else None
    flags = (_lib.EVAL_FIT_GAIN if fit_gain else 0) | (_lib.EVAL_SSIM if ssim else 0)
    with torch.cuda.device(device):
        _lib.check(L.lograst_eval_metrics(
            C, H, W, _ptr(pred), _strides(pred), _ptr(gt), _strides(gt), flags, float(max_val),
            _ptr(out_corrected) if corrected else None, _ptr(out_bgr8) if bgr8 else None, _ptr(record), _ptr(scratch), nbytes,
            _stream_ptr(device)))
    return Metrics(record, out_corrected, out_bgr8, C, bool(ssim))


# ---- drop-ins for an unmodified LoG checkout ---------------------------------------------------------------------------

def _image(t, what):
    """A tensor as the kernels read an image -- on the GPU, fp32, [C, H, W] with C <= 4, fewer than 2^31 elements -- or Fallback."""
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise Fallback("tensors are not on the GPU")
    if t.dtype != torch.float32:
        raise Fallback(f"{what} is {t.dtype}, not float32")
    if t.dim() != 3 or min(t.shape) < 1:
        raise Fallback(f"{what} is not one image of three dimensions")
    if t.shape[0] > MAX_CHANNELS:
        raise Fallback(f"more than {MAX_CHANNELS} channels")
    if t.numel() >= 2 ** 31:
        raise Fallback("2^31 elements or more")
    return t.detach()


def _pair(a, b):
    if torch.is_tensor(a) and torch.is_tensor(b) and (a.shape != b.shape or a.device != b.device):
        raise Fallback("the two images differ in shape or device")


def _channels_first(t):
    """[A, B, C] channels-last -> the [C, A, B] view; two dimensions -> one channel."""
    if torch.is_tensor(t) and t.dim() == 2:
        return t[None]
    if torch.is_tensor(t) and t.dim() == 3 and t.shape[0] > MAX_CHANNELS and t.shape[2] <= MAX_CHANNELS:
        return t.permute(2, 0, 1)
    return t


@dropins.dropin
def psnr(rgbs, target_rgbs):
    """metric.py:7-9: -10 log10(mean((rgbs - target_rgbs)^2)) as a Python float.  Images [C, H, W], [H, W, C] or [H, W]."""
    _pair(rgbs, target_rgbs)
    a, b = _image(_channels_first(rgbs), "rgbs"), _image(_channels_first(target_rgbs), "target_rgbs")
    m = validation_metrics(a, b)
    dropins.count("readbacks", "psnr")
    return m.read().psnr


@dropins.dropin
def ssim(rgbs, target_rgbs, max_val, filter_size=SSIM_WINDOW, filter_sigma=SSIM_SIGMA, k1=SSIM_K1, k2=SSIM_K2):
    """metric.py:33-103 for one channels-last image [..., W, H, C]: the mean of the SSIM map as a Python float."""
    if filter_size != SSIM_WINDOW or filter_sigma != SSIM_SIGMA or k1 != SSIM_K1 or k2 != SSIM_K2:
        raise Fallback("another window than 11 taps of sigma 1.5, or other k1 / k2")
    _pair(rgbs, target_rgbs)
    if not torch.is_tensor(rgbs) or rgbs.device.type != "cuda":
        raise Fallback("tensors are not on the GPU")
    if rgbs.dim() < 3:
        raise Fallback("rgbs is not one image of three dimensions")
    if rgbs.numel() != math.prod(rgbs.shape[-3:]):
        raise Fallback("more than one image")
    shape = tuple(rgbs.shape[-3:])
    a = _image(rgbs.reshape(shape).permute(2, 0, 1), "rgbs")
    b = _image(target_rgbs.reshape(shape).permute(2, 0, 1), "target_rgbs")
    m = validation_metrics(a, b, ssim=True, max_val=max_val)
    dropins.count("readbacks", "ssim")
    return m.read().ssim


@dropins.dropin
def tensor_to_bgr(tensor):
    """renderer.py:19-23 (a staticmethod there and here): [C, H, W] -> np.ndarray [H, W, C] uint8, channels reversed."""
    out = image_to_bgr8(_image(tensor, "tensor"))
    dropins.count("readbacks", "tensor_to_bgr")
    return out


@dropins.dropin
def make_validation(self, iteration, visualize=False):
    """trainer.py:298-364 with, per image, one ``validation_metrics`` launch (the fit exactly when the model has a view
    correction, ``corrected`` only for LPIPS, ``bgr8`` only when the image is written), ONE read-back, and the 8-bit copy
    when the image is written.  ``prepare_batch``, ``tqdm`` and ``cv2`` are the trainer module's own."""
    mod = sys.modules[type(self).__module__]
    prepare_batch, cv2 = mod.prepare_batch, mod.cv2
    tqdm = getattr(mod, "tqdm", lambda it, **kwargs: it)
    metric = defaultdict(list)
    model = self.model
    model.eval()
    logdir = os.path.join(self.exp, 'val', f'{iteration:06d}')
    for _data in tqdm(self.val, desc=f'val {iteration}'):
        batch = prepare_batch(_data, self.device)
        model.clear()
        output = self.render_val.vis(batch, self.model, background=torch.ones_like(self.render_val.background))
        pred = output['render'][0].detach()
        pred = self.render_val.process_pred(batch, pred)
        gt = self.render_val.process_gt(batch)[0]
        del output
        _pair(pred, gt)
        pred, gt = _image(pred, "pred"), _image(gt, "gt")
        write = (iteration + 1) % 1000 == 0 or visualize
        m = validation_metrics(pred, gt, fit_gain=getattr(model, 'view_correction', None) is not None,
                               corrected=self.lpips is not None, bgr8=write)
        if self.lpips is not None:      # queued behind the kernels, before the read-back waits for them
            ret_lpips = self.lpips(m.corrected[None], gt[None], retPerLayer=False, normalize=True)
        r = m.read()
        dropins.count("readbacks", "make_validation")
        metric['l1'].append(r.l1)
        metric['psnr'].append(r.psnr)
        if self.lpips is not None:
            metric['lpips'].append(ret_lpips.item())
        metric['imgname'].append(batch['imgname'][0])
        if write:
            os.makedirs(logdir, exist_ok=True)
            outname = os.path.join(logdir, f'{batch["index"][0]:06d}_{os.path.basename(metric["imgname"][-1])}.jpg')
            vis = m.bgr8_host()
            dropins.count("readbacks", "make_validation")
            cv2.imwrite(outname, vis)
    record = {
        'iteration': iteration,
        'num_points': model.num_points,
    }
    print(f'>>> Validation: {iteration}: {len(metric["imgname"])} images')
    for key, val in metric.items():
        if key == 'imgname':
            continue
        mean_val = sum(val) / len(val)
        record[key] = mean_val
        if self.global_iterations > 0:
            self.recorder.log(self.global_iterations, f'val/{key}', mean_val)
        print(f'    - {key}: {mean_val:.4f}')
    logname = os.path.join(self.exp, 'val', f'{iteration:06d}.yml')
    os.makedirs(os.path.dirname(logname), exist_ok=True)
    self.model.train()

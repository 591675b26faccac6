"""Generates tests/golden/evaluate_*.npz by RUNNING the reference's own evaluation code on the CPU (build container only:
needs the reference tree): LoG/utils/metric.py ``psnr`` and ``ssim``, ``BaseRender.tensor_to_bgr``, and -- for the part of
a validation that the reference has inline (the view-correction fit, the clamp, L1) -- ``Trainer.make_validation`` itself,
called unbound on a stand-in trainer with a one-image ``val`` list, ``global_iterations > 0`` and ``visualize=True``.  cv2
and tensorboardX are stubbed in sys.modules (absent here; only ``cv2.imwrite`` is reached, and it captures the array).

    LOG_REFERENCE=<LoG checkout> python tests/golden/make_golden_evaluate.py

Every file holds pred, gt (fp32; gt_hwc = 1: gt is stored [H, W, C]), fit (0 / 1: the model has a view correction),
max_val, and the reference's fp32 results: psnr, ssim (metric.py's functions on pred and gt as they are), bgr_pred, bgr_gt
(tensor_to_bgr) and mv_l1, mv_psnr, mv_vis (what make_validation logged and wrote)."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ["LOG_REFERENCE"]          # a checkout of the reference (LoG)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # this repository: diff_gaussian_rasterization_wodilate

WRITTEN = []
cv2 = types.ModuleType("cv2")
cv2.imwrite = lambda name, img: WRITTEN.append(np.array(img, copy=True))
tbx = types.ModuleType("tensorboardX")
tbx.SummaryWriter = object
sys.modules.setdefault("cv2", cv2)
sys.modules.setdefault("tensorboardX", tbx)

from LoG.render.renderer import BaseRender        # noqa: E402  reference code, imported not copied
from LoG.utils import metric                      # noqa: E402
from LoG.utils.trainer import Trainer             # noqa: E402


class _Model:
    def __init__(self, fit):
        self.view_correction = object() if fit else None
        self.num_points = 0

    def eval(self): pass
    def train(self): pass
    def clear(self): pass


class _Render:
    background = torch.ones(3)
    tensor_to_bgr = staticmethod(BaseRender.tensor_to_bgr)

    def vis(self, batch, model, background=None):
        return {"render": batch["pred"][None]}

    def process_pred(self, batch, pred):
        return pred

    def process_gt(self, batch):
        return batch["gt"][None]


class _Recorder:
    def __init__(self):
        self.logged = {}

    def log(self, step, key, value):
        self.logged[key] = float(value)


def run_make_validation(pred, gt, fit):
    """-> (l1, psnr, the written array) of Trainer.make_validation on one image."""
    del WRITTEN[:]
    me = types.SimpleNamespace(
        model=_Model(fit), render_val=_Render(), recorder=_Recorder(), lpips=None, device="cpu", global_iterations=1,
        exp=tempfile.mkdtemp(), val=[{"pred": torch.from_numpy(pred), "gt": torch.from_numpy(gt), "imgname": ["a.jpg"], "index": [0]}])
    Trainer.make_validation(me, 0, visualize=True)
    assert len(WRITTEN) == 1
    return me.recorder.logged["val/l1"], me.recorder.logged["val/psnr"], WRITTEN[0]


def smooth(rng, C, H, W, cells=4):
    coarse = torch.tensor(rng.random((1, C, cells, cells)), dtype=torch.float64)
    if H < 2 or W < 2:
        return rng.random((C, H, W))
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0].numpy()


def grid8(rng):
    """Every k / 255 with its two fp32 neighbours, -0.0, 1.0, negatives and values above 1 (no nan), as [3, 16, 17]."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    vals = [k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
            np.array([-0.0, 1.0, -1e-8, -0.5, -3.0, 1.0000001, 1.5, 7.0, 255.0, 1e-30, 0.999999], dtype=np.float32)]
    v = np.concatenate(vals).astype(np.float32)
    fill = rng.uniform(-0.1, 1.1, 3 * 16 * 17 - v.size).astype(np.float32)
    return np.concatenate([v, fill]).reshape(3, 16, 17)


def cases():
    rng = np.random.default_rng(20250611)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)

    def pair(C, H, W, noise=0.05, lo=0.05, hi=0.95):
        gt = lo + (hi - lo) * smooth(rng, C, H, W)
        pred = gt + noise * rng.standard_normal((C, H, W))
        return f32(np.clip(pred, 0., 1.)), f32(gt)

    def case(pred, gt, fit=0, max_val=1.0, gt_hwc=0):
        return dict(pred=pred, gt=gt, fit=np.int32(fit), max_val=np.float64(max_val), gt_hwc=np.int32(gt_hwc))

    yield "1x1", case(*pair(3, 1, 1))
    yield "2x3", case(*pair(1, 2, 3))
    yield "11x11", case(*pair(4, 11, 11))
    yield "33x65", case(*pair(3, 33, 65))                       # crosses tile edges on both axes
    yield "33x67_gain", case(*pair(3, 33, 67), fit=1)           # ... with an odd W // 2
    p, g = pair(3, 37, 53)
    yield "37x53_gain", case(f32(p * 0.8), g, fit=1)
    p, g = pair(3, 64, 96)
    yield "64x96_hwc", case(p, np.ascontiguousarray(g.transpose(1, 2, 0)), gt_hwc=1)
    p, g = pair(3, 16, 20)
    yield "identical", case(g, g.copy())
    yield "constant", case(np.full((3, 16, 20), 0.3, np.float32), np.full((3, 16, 20), 0.6, np.float32))
    base = 0.5 + 1e-3 * rng.standard_normal((3, 24, 40))
    yield "low_contrast", case(f32(base + 1e-4 * rng.standard_normal((3, 24, 40))), f32(base))
    yield "out_of_range", case(f32(rng.uniform(-0.5, 1.5, (3, 20, 36))), f32(rng.uniform(-0.5, 1.5, (3, 20, 36))), max_val=2.0)
    p, g = pair(3, 20, 36, lo=0.3, hi=0.9)
    p = f32(p * 0.5)
    p[:, :, 18:] *= np.float32(2.5)                             # the fit (about 2) pushes the right half above 1
    yield "gain_clamped", case(p, g, fit=1)
    yield "w1_gain", case(*pair(3, 5, 1), fit=1)                # an empty left half: 0 / 0
    g8 = grid8(rng)
    yield "grid8", case(g8, f32(np.ascontiguousarray(g8[:, ::-1, ::-1])))


def main():
    for name, c in cases():
        pred = c["pred"]
        gt = c["gt"].transpose(2, 0, 1) if int(c["gt_hwc"]) else c["gt"]
        tp, tg = torch.from_numpy(pred), torch.from_numpy(np.ascontiguousarray(gt))
        with np.errstate(all="ignore"):
            c["psnr"] = np.float64(metric.psnr(tp, tg))
            c["ssim"] = np.float64(metric.ssim(tp.permute(1, 2, 0).contiguous(), tg.permute(1, 2, 0).contiguous(), float(c["max_val"])))
            c["bgr_pred"] = BaseRender.tensor_to_bgr(tp)
            c["bgr_gt"] = BaseRender.tensor_to_bgr(tg)
            l1, ps, vis = run_make_validation(pred, np.ascontiguousarray(gt), int(c["fit"]))
        c["mv_l1"], c["mv_psnr"], c["mv_vis"] = np.float64(l1), np.float64(ps), vis
        path = os.path.join(HERE, "evaluate_%s.npz" % name)
        np.savez_compressed(path, **c)
        print("%-14s %s fit %d  psnr %.6f ssim %.6f  mv_l1 %.8f mv_psnr %.6f  %d bytes" % (
            name, pred.shape, int(c["fit"]), c["psnr"], c["ssim"], l1, ps, os.path.getsize(path)))


if __name__ == "__main__":
    main()

"""Generates tests/golden/depth_loss_*.npz by RUNNING the reference's own depth loss on CPU (build container only: needs
the reference tree): LoG/render/loss.py ScaleAndShiftInvariantLoss() on the patches sliced and stacked as
LoG/render/renderer.py:275-285 slices and stacks them, `1./(preds + 1e-5)`, backward() to the depth image -- once in fp32
and once in float64 on the same fp32 inputs.

    LOG_REFERENCE=<LoG checkout> python tests/golden/make_golden_depth_loss.py

Every file holds pred, gt, acc (fp32 [H, W]), rows, cols (int64 [n]), loss32, loss64, grad32, grad64 and the reference's
own fp32-vs-float64 distance gap32_loss (absolute) and gap32_grad (rel-L2); `empty` (no valid pixel: nan) holds the
inputs and the two losses only."""
import os
import sys

import numpy as np
import torch

REF = os.environ["LOG_REFERENCE"]          # a checkout of the reference (LoG)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from LoG.render.loss import ScaleAndShiftInvariantLoss   # noqa: E402  reference code, imported not copied

PATCH = 64


def run(c, dtype):
    depth_loss = ScaleAndShiftInvariantLoss()
    pred = torch.tensor(c["pred"], dtype=dtype, requires_grad=True)
    gt = torch.tensor(c["gt"], dtype=dtype)
    mask = torch.tensor(c["acc"]) > 0.5
    preds, gts, masks = [], [], []
    for r, k in zip(c["rows"].tolist(), c["cols"].tolist()):
        preds.append(pred[r:r + PATCH, k:k + PATCH])
        gts.append(gt[r:r + PATCH, k:k + PATCH])
        masks.append(mask[r:r + PATCH, k:k + PATCH])
    loss, _ = depth_loss(1. / (torch.stack(preds) + 1e-5), torch.stack(gts), mask=torch.stack(masks))
    if not bool(torch.isfinite(loss)):
        return loss.item(), None
    loss.backward()
    return loss.item(), pred.grad.numpy()


def smooth(rng, H, W, cells):
    """A smooth random field in [0, 1]: bilinear interpolation of a coarse random grid."""
    coarse = torch.tensor(rng.random((1, 1, cells, cells)), dtype=torch.float64)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0, 0].numpy()


def cases():
    rng = np.random.default_rng(20250117)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    H, W, n = 96, 128, 64
    ones = np.ones((H, W), np.float32)
    starts = lambda: dict(rows=rng.integers(0, H - PATCH, n).astype(np.int64), cols=rng.integers(0, W - PATCH, n).astype(np.int64))
    noisy = lambda: f32(2.0 + 2.0 * smooth(rng, H, W, 6) * 0.9 + 0.05 * rng.standard_normal((H, W)) + 0.1)
    gt = lambda: f32(0.1 + 0.5 * smooth(rng, H, W, 5))
    # a smooth depth in [2, 4] with noise, a smooth target, an accumulation map that crosses 0.5
    yield "smooth", dict(pred=noisy(), gt=gt(), acc=f32(0.15 + 0.8 * smooth(rng, H, W, 4)), **starts())
    yield "allmask", dict(pred=noisy(), gt=gt(), acc=ones, **starts())
    # the depth of the C1 plumbing test: uniform in [2, 4], both
    yield "uniform", dict(pred=f32(2.0 + 2.0 * rng.random((H, W))), gt=f32(2.0 + 2.0 * rng.random((H, W))), acc=ones, **starts())
    # nothing valid left of column 70: empty patches (start column <= 6), patches with narrow valid strips and patches valid
    # over most of their width (57 of 64 columns at start column 63) in one batch
    half = ones.copy()
    half[:, :70] = 0.0
    yield "half", dict(pred=noisy(), gt=gt(), acc=half, **starts())
    # nearly constant depth: the fp32 determinant cancels
    yield "nearly_const", dict(pred=f32(3.0 + 1e-3 * smooth(rng, H, W, 6)), gt=gt(), acc=ones, **starts())
    # 65 x 65: the only starts are 0 and 1
    yield "edges", dict(pred=f32(2.0 + 2.0 * smooth(rng, 65, 65, 5) + 0.05 * rng.standard_normal((65, 65))),
                        gt=f32(0.1 + 0.5 * smooth(rng, 65, 65, 4)), acc=f32(0.2 + 0.8 * smooth(rng, 65, 65, 3)),
                        rows=np.array([0, 1, 0], np.int64), cols=np.array([0, 1, 1], np.int64))
    # a patch with exactly one valid pixel (its determinant is exactly 0 in any arithmetic) next to an empty patch, a
    # patch that is valid in its right half and full patches
    one = ones.copy()
    one[:, :64] = 0.0
    one[10, 20] = 1.0
    yield "one_pixel", dict(pred=noisy(), gt=gt(), acc=one, rows=np.array([0, 20, 16, 0, 32], np.int64),
                            cols=np.array([0, 0, 32, 64, 64], np.int64))
    yield "empty", dict(pred=noisy(), gt=gt(), acc=np.zeros((H, W), np.float32), **starts())


def main():
    for name, c in cases():
        l32, g32 = run(c, torch.float32)
        l64, g64 = run(c, torch.float64)
        out = dict(c, loss32=np.float32(l32), loss64=np.float64(l64))
        if g64 is not None:
            out.update(grad32=g32.astype(np.float32), grad64=g64.astype(np.float64),
                       gap32_loss=np.float64(abs(float(l32) - float(l64))),
                       gap32_grad=np.float64(np.linalg.norm(g32.astype(np.float64) - g64) / np.linalg.norm(g64)))
        path = os.path.join(HERE, "depth_loss_%s.npz" % name)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), l32, l64, {k: float(v) for k, v in out.items() if k.startswith("gap32")})


if __name__ == "__main__":
    main()

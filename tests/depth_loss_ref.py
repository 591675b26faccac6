"""A torch restatement of the depth patch loss (log_amd/depth_loss.py, lograst_depth_loss_*), written from its formulas
(include/lograst.h) and differentiated by autograd, in any dtype and on any device.  tests/test_depth_loss_cpu.py holds it
to the reference's own float64 results (tests/golden/depth_loss_*.npz); the GPU tests measure the kernels against it at
shapes no fixture has.  Nothing here imports the reference.

Per pixel m = acc > thr, p = 1 / (pred + eps); per patch k (rows r..r+63, columns c..c+63) the sums a00 = sum m p^2,
a01 = sum m p, a11 = sum m, b0 = sum m p gt, b1 = sum m gt, det = a00 a11 - a01^2, (s, h) = the solution of the 2 x 2
normal equations where det != 0 and (0, 0), without gradient, elsewhere; d = m (s p + h - gt);
loss = (sum d^2 + alpha * sum over horizontal and vertical neighbour pairs m m' |d' - d|) / sum m, every sum over all
patches."""
import numpy as np
import torch

PATCH = 64


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def load_case(path):
    """-> dict: tensors for the inputs (pred, gt, acc fp32; rows, cols int64), numpy for everything else."""
    z = np.load(path)
    c = {k: z[k] for k in z.files}
    for k in ("pred", "gt", "acc", "rows", "cols"):
        c[k] = torch.from_numpy(c[k])
    return c


def patches(img, rows, cols):
    """[H, W] -> [n, 64, 64]: patch k = img[rows[k] : rows[k] + 64, cols[k] : cols[k] + 64], by index arithmetic."""
    ar = torch.arange(PATCH, device=img.device)
    ys = (rows.to(img.device)[:, None] + ar)[:, :, None]
    xs = (cols.to(img.device)[:, None] + ar)[:, None, :]
    return img[ys, xs]


def stack_loss(p, t, m, alpha=0.5):
    """The loss of stacked patches: p = 1 / (pred + eps), t = gt, m = mask as numbers, each [n, 64, 64] -> 0-dim tensor
    (with its graph), M."""
    a00, a01, a11 = (m * p * p).sum((1, 2)), (m * p).sum((1, 2)), m.sum((1, 2))
    b0, b1 = (m * p * t).sum((1, 2)), (m * t).sum((1, 2))
    det = a00 * a11 - a01 * a01
    ok = det != 0
    safe = torch.where(ok, det, torch.ones_like(det))
    zero = torch.zeros_like(det)
    s = torch.where(ok, (a11 * b0 - a01 * b1) / safe, zero)
    h = torch.where(ok, (a00 * b1 - a01 * b0) / safe, zero)
    d = m * (s[:, None, None] * p + h[:, None, None] - t)
    D = (d * d).sum()
    R = ((m[:, :, 1:] * m[:, :, :-1]) * (d[:, :, 1:] - d[:, :, :-1]).abs()).sum() \
        + ((m[:, 1:, :] * m[:, :-1, :]) * (d[:, 1:, :] - d[:, :-1, :]).abs()).sum()
    M = m.sum()
    return (D + alpha * R) / M, M


def depth_loss_ref(pred, gt, acc, rows, cols, alpha=0.5, eps=1e-5, thr=0.5, dtype=torch.float64, upstream=1.0):
    """-> {"loss": python float, "grad": d(upstream * loss)/d pred [H, W] in dtype, "M": python float}"""
    x = pred.detach().to(dtype).requires_grad_(True)
    p = 1.0 / (patches(x, rows, cols) + eps)
    t = patches(gt.detach().to(dtype), rows, cols)
    m = (patches(acc.detach(), rows, cols) > thr).to(dtype)
    loss, M = stack_loss(p, t, m, alpha)
    grad = torch.autograd.grad(upstream * loss, x)[0] if bool(M > 0) else torch.full_like(x, float("nan"))
    return {"loss": float(loss.detach()), "grad": grad.detach(), "M": float(M)}

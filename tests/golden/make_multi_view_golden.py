"""Generates tests/golden/multi_view_log.npz by RUNNING the reference's own code on the CPU (build container only): three
views of one model through the gathers of LoG.get_all (LoG/model/level_of_gaussian.py:262-281, fix_parent, training --
restated in the lines marked below because the method needs a whole LoG object, as make_golden_getall.py does) and
Activation.activate_root_return (imported), the compact gradients from torch autograd, then ONE step of the reference's
_single_tensor_adam (imported) with the scalars of SparseOptimizer.step at step STEP on the rows some view saw, from the fp32
sum of the views' gradients in view order -- the step the reference itself cannot take (LoG.step reads the last view only).

Values are drawn on coarse grids (model: multiples of 1/256) so that the file stays the size of the other fixtures; the
gradients and the stepped rows are whatever fp32 the reference computes.

    python tests/golden/make_multi_view_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("LOG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from LoG.model.activation import Activation                                    # noqa: E402  reference code, imported not copied
from LoG.model.sparse_optimizer import _single_tensor_adam, get_expon_lr_func  # noqa: E402

KEYS = ["scaling", "colors", "xyz", "opacity", "rotation", "shs"]     # GaussianPoint.keys order
P, K, DEGREE, STEP, VIEWS = 3000, 15, 3, 7, 3
LR = {"xyz": 0.00016, "xyz_final": 0.0000016, "colors": 0.0025, "shs": 0.000125, "scaling": 0.005, "opacity": 0.05,
      "rotation": 0.001, "max_steps": 300}


def grid(t, step):
    return torch.round(t / step) * step


def main():
    g = torch.Generator().manual_seed(20)
    model = {"scaling": grid(-1.0 - 4.6 * torch.rand(P, 3, generator=g), 1 / 256),        # exp: 0.0037 .. 0.37, two decades
             "colors": grid(torch.randn(P, 3, generator=g), 1 / 256),
             "xyz": grid(torch.rand(P, 3, generator=g) - 0.5, 1 / 1024),
             "opacity": grid(torch.randn(P, 1, generator=g) * 2, 1 / 256),
             "rotation": grid(torch.randn(P, 4, generator=g), 1 / 256),
             "shs": grid(torch.randn(P, K, 3, generator=g) * 0.3, 1 / 256)}
    model["rotation"][:5] *= 1e-3                                  # short quaternions
    # moments of an optimizer that has stepped some rows before: non-zero on 500 rows, part of which the views see
    warm = torch.randperm(P, generator=g)[:500]
    exp_avg = {k: torch.zeros_like(v) for k, v in model.items()}
    exp_avg_sq = {k: torch.zeros_like(v) for k, v in model.items()}
    for k, v in model.items():
        exp_avg[k][warm] = grid(torch.randn(v[warm].shape, generator=g) * 0.05, 1 / 4096)
        exp_avg_sq[k][warm] = grid(torch.rand(v[warm].shape, generator=g) * 0.01, 1 / 65536)
    out = {"degree": np.int32(DEGREE), "K": np.int32(K), "step": np.int32(STEP), "views": np.int32(VIEWS)}
    for k in KEYS:
        out["model_" + k] = model[k].numpy().copy()
        out["exp_avg_" + k] = exp_avg[k].numpy().copy()
        out["exp_avg_sq_" + k] = exp_avg_sq[k].numpy().copy()

    # three selections that overlap partly: each draws its leaves and nodes from a window of a common permutation
    perm = torch.randperm(P, generator=g)
    total = {k: torch.zeros_like(v) for k, v in model.items()}
    seen = torch.zeros(P, dtype=torch.int32)
    for v in range(VIEWS):
        window = perm[120 * v:120 * v + 420]
        pick = window[torch.randperm(420, generator=g)[:230]]
        index, index_node = pick[:200], pick[200:]
        camera = {"camera_center": torch.tensor([0.3 + 0.8 * v, -2.5 + 0.4 * v, 0.8 - 0.5 * v])}
        radii = torch.randint(-1, 9, (230,), generator=g, dtype=torch.int32)          # some <= 0
        # level_of_gaussian.py:267-281 (fix_parent, training)
        params = {k: nn.Parameter(val[index]) for k, val in model.items()}
        full = {k: torch.cat([params[k], val[index_node]]) for k, val in model.items()}
        act = Activation().activate_root_return(full, camera, DEGREE)
        ups = {k: grid(torch.randn(act[k].shape, generator=g), 1 / 64) for k in ("xyz", "scaling", "opacity", "rotation", "colors")}
        sum((act[k] * ups[k]).sum() for k in ups).backward()
        out.update({f"v{v}_index": index.numpy(), f"v{v}_index_node": index_node.numpy(), f"v{v}_radii": radii.numpy(),
                    f"v{v}_camera_center": camera["camera_center"].numpy()})
        for k in ups:
            out[f"v{v}_up_{k}"] = ups[k].numpy().astype(np.float16)               # exact: multiples of 1/64 below 8
            assert np.array_equal(out[f"v{v}_up_{k}"].astype(np.float32), ups[k].numpy())
        live = radii[:200] > 0                                                    # LoG.step: flag_vis[:index.shape[0]]
        rows = index[live]
        for k in KEYS:
            out[f"v{v}_grad_{k}"] = params[k].grad.numpy()
            total[k].index_add_(0, rows, params[k].grad[live])                    # fp32, view order
        seen.index_add_(0, rows, torch.ones_like(rows, dtype=torch.int32))

    # SparseOptimizer.step (sparse_optimizer.py:163-196) at global_steps = STEP on the rows some view saw
    rows = torch.nonzero(seen > 0).squeeze(1)
    xyz_lr = get_expon_lr_func(lr_init=LR["xyz"], lr_final=LR["xyz_final"], max_steps=LR["max_steps"])
    scaling_lr = get_expon_lr_func(lr_init=LR["scaling"], lr_final=LR["scaling"], max_steps=LR["max_steps"])
    out["rows"] = rows.numpy()
    out["seen"] = seen.numpy()
    for k in KEYS:
        lr = xyz_lr(STEP) if k == "xyz" else scaling_lr(STEP) if k == "scaling" else LR[k]
        p, m, s = model[k][rows].clone(), exp_avg[k][rows].clone(), exp_avg_sq[k][rows].clone()
        p, m, s, _ = _single_tensor_adam(p, total[k][rows], m, s, None, STEP, lr, eps=1e-15)
        out["lr_" + k] = np.float64(lr)
        out["sum_" + k] = total[k][rows].numpy()
        out["after_model_" + k], out["after_exp_avg_" + k], out["after_exp_avg_sq_" + k] = p.numpy(), m.numpy(), s.numpy()
    f = os.path.join(HERE, "multi_view_log.npz")
    np.savez_compressed(f, **out)
    print(os.path.getsize(f) // 1024, "KiB;", int(rows.numel()), "rows seen,", int((seen > 1).sum()), "by more than one view")


if __name__ == "__main__":
    main()

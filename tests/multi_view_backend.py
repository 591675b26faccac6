"""TEST DOUBLE: the oracle CPU backend (tests/oracle_backend.py) + the two calls of log_amd.multi_view, each composed from what
that backend already has -- ``activate_backward`` and ``index_add_`` for the accumulating backward, ``sparse_adam`` over
``arange(P)`` with ``seen > 0`` as the flag for the step -- so that the module's host logic runs through the reference's
unmodified classes on a machine without a GPU.  tests/test_gpu_multi_view.py holds the two kernels to the same compositions
(on the parent's kernels) bit for bit."""
import hashlib

import torch

from oracle_backend import OracleBackend

KEYS = ("xyz", "scaling", "opacity", "rotation", "colors", "shs")


class MultiViewBackend(OracleBackend):
    """+ what the backward's route reads of the HIP backend: the forward's ``radii`` in the saved state."""

    def __init__(self):
        self._memo = {}

    def forward(self, *args, **kw):
        *out, saved = super().forward(*args, **kw)
        return (*out, {"radii": out[1], "oracle": saved})

    def backward(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image, **kw):
        """The oracle's reverse walk sums with OpenMP atomics: two runs on the same inputs differ in the last bits.  The
        results are remembered by the bytes of the inputs, so that two models driven through identical views receive identical
        gradients and a test may compare what follows bit for bit."""
        key = hashlib.sha256()
        for t in (means3D, scales, rotations, grad_image, rs.viewmatrix, rs.projmatrix, saved["radii"]):
            key.update(t.detach().contiguous().numpy().tobytes())
        key = key.hexdigest()
        if key not in self._memo:
            self._memo[key] = super().backward(rs, flavour, use_filter, means3D, scales, rotations, saved["oracle"],
                                               grad_image, **kw)
        return tuple(None if t is None else t.clone() for t in self._memo[key])

    def activate_backward_accumulate(self, raw, n, degree, campos, g_xyz, g_scaling, g_opacity, g_rotation, g_colors, index,
                                     radii, targets, seen):
        g = self.activate_backward(raw, n, degree, campos, g_scaling, g_opacity, g_rotation, g_colors)
        g["xyz"] = g_xyz[:n]
        P = int(seen.numel())
        idx = index[:n].to(torch.int64)
        live = (radii[:n] > 0) & (idx >= 0) & (idx < P)
        rows = idx[live]
        for key, t in targets.items():
            t.index_add_(0, rows, g[key][live].to(torch.float32).reshape((-1,) + tuple(t.shape[1:])))
        seen.index_add_(0, rows, torch.ones_like(rows, dtype=torch.int32))

    def accumulated_adam(self, seen, entries, beta1, beta2, bias_correction2_sqrt, eps, moved_out=None):
        P = int(seen.numel())
        flag = seen > 0
        rows = torch.arange(P, dtype=torch.int64)
        self.sparse_adam(rows, flag, [(model, model.clone(), grad.contiguous(), m1, m2, mx, step)
                                      for model, grad, m1, m2, mx, step in (entries[k] for k in KEYS if k in entries)],
                         beta1, beta2, bias_correction2_sqrt, eps)
        for k in entries:
            entries[k][1][flag] = 0
        seen[flag] = 0
        if moved_out is not None:
            moved_out.copy_(flag.to(torch.uint8))

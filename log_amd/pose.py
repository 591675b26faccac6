"""A per-view pose table for refining camera poses against the rasterizer's camera gradients (for use outside LoG: LoG has
no pose parameters to replace, so there is no drop-in and no ``install_all`` switch; INTEGRATION.md has the recipe).

``PoseTable(num_views, device, lr_init, lr_final, start_step=0)`` keeps, in the layout ``log_amd.view_correction`` drives for
LoG's Corrector, a ``[num_views, 6]`` fp32 table of rows xi = (omega, upsilon), its gradient, the AMSGrad moments and one
step count per row.

* ``camera(index, viewmatrix, projmatrix) -> (viewmatrix', projmatrix', campos')``: the view's matrices under the
  camera-frame perturbation ``p_cam' = R(omega) p_cam + upsilon`` (Rodrigues' formula, its series near omega = 0).  With
  ``E = [[R^T - I, 0], [upsilon, 0]]`` and ``W = V E``: ``V' = V + W``, ``P' = P + W (V^-1 P)``, ``campos'`` = row 3 of
  ``V'^-1``, the inverses by the rigid closed form, in double inside one one-wave kernel (``lograst_pose_apply``).  A zero row
  returns ``V`` and ``P`` to the bit.  The results require grad; hand them to ``GaussianRasterizationSettings`` and the
  rasterizer's backward fills them (``log_amd.rasterizer``: camera gradients), from where the second one-wave kernel
  (``lograst_pose_backward``) ADDS dL/dxi into row ``index`` of ``table.grad``.  ``viewmatrix`` and ``projmatrix`` are constants
  of this function.  Nothing synchronises with the host.
* ``step(index)``: the AMSGrad step of that row with Corrector.step's schedule (``lograst_corrector_step`` at width 6: the
  row's count advances, nothing moves before ``start_step``, the row's gradient is cleared)."""
import torch

from . import _lib
from . import rasterizer as _r


def _matrix(t, device, what):
    t = t.detach().to(device=device, dtype=torch.float32).contiguous()
    if tuple(t.shape) != (4, 4):
        raise ValueError(f"{what} must be 4x4")
    return t


class _PoseCamera(torch.autograd.Function):
    """anchor: a scalar that requires grad (autograd runs a node's backward only behind such an input; the table itself is
    plain storage that the step kernel updates in place).  The gradient goes into ``pose.grad``; the anchor's is None."""

    @staticmethod
    def forward(ctx, anchor, pose, index, V, P):
        L = _lib.lib()
        device = pose.device
        f32 = dict(dtype=torch.float32, device=device)
        Vn, Pn, cp = torch.empty(4, 4, **f32), torch.empty(4, 4, **f32), torch.empty(3, **f32)
        with torch.cuda.device(device):
            _lib.check(L.lograst_pose_apply(pose.num_views, index, _r._ptr(pose.table), _r._ptr(V), _r._ptr(P), _r._ptr(Vn),
                                            _r._ptr(Pn), _r._ptr(cp), _r._stream_ptr(device)))
        ctx.pose, ctx.index = pose, index
        ctx.set_materialize_grads(False)
        # (the row as it was: a step between forward and backward must not move the point the derivative is taken at)
        ctx.save_for_backward(pose.table[index].clone(), V, P)
        return Vn, Pn, cp

    @staticmethod
    def backward(ctx, g_v, g_p, g_c):
        row, V, P = ctx.saved_tensors
        pose, device = ctx.pose, row.device
        L = _lib.lib()
        g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_v, g_p, g_c)]
        # the kernel reads row 0 of a one-row table (the saved row) and adds into row 0 of grad[index:]
        with torch.cuda.device(device):
            _lib.check(L.lograst_pose_backward(1, 0, _r._ptr(row), _r._ptr(V), _r._ptr(P), _r._ptr(g[0]), _r._ptr(g[1]),
                                               _r._ptr(g[2]), _r._ptr(pose.grad[ctx.index]), _r._stream_ptr(device)))
        return None, None, None, None, None


class PoseTable:
    def __init__(self, num_views, device, lr_init, lr_final, start_step=0):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.LograstError(f"log_amd.pose needs a table on the MI355X (got device '{device}'); the HIP kernels are "
                                    "the only implementation -- there is no CPU fallback")
        if int(num_views) < 1:
            raise ValueError("num_views must be >= 1")
        if not (0.0 < float(lr_init) < float("inf") and 0.0 < float(lr_final) < float("inf")):
            raise ValueError("lr_init and lr_final must be positive and finite")
        self.num_views, self.device = int(num_views), device
        self.lr_init, self.lr_final, self.start_step = float(lr_init), float(lr_final), int(start_step)
        z = lambda: torch.zeros(self.num_views, 6, dtype=torch.float32, device=device)
        self.table, self.grad = z(), z()
        self.exp_avg, self.exp_avg_sq, self.max_exp_avg_sq = z(), z(), z()
        self.steps = torch.zeros(self.num_views, dtype=torch.int32, device=device)

    def _index(self, index):
        if isinstance(index, bool) or not isinstance(index, int) or not 0 <= index < self.num_views:
            raise IndexError("index is not an integer in [0, num_views)")
        return index

    def camera(self, index, viewmatrix, projmatrix):
        """-> (viewmatrix', projmatrix', campos') on the table's device, fp32; differentiable in row ``index``."""
        index = self._index(index)
        V, P = _matrix(viewmatrix, self.device, "viewmatrix"), _matrix(projmatrix, self.device, "projmatrix")
        anchor = torch.zeros((), device=self.device, requires_grad=True)
        return _PoseCamera.apply(anchor, self, index, V, P)

    def step(self, index):
        """One AMSGrad step of row ``index`` (Corrector.step's schedule), then ``grad[index] = 0``; nothing is read back."""
        index = self._index(index)
        L = _lib.lib()
        with torch.cuda.device(self.device):
            _lib.check(L.lograst_corrector_step(self.num_views, 6, index, self.start_step, self.lr_init, self.lr_final,
                                                _r._ptr(self.steps), _r._ptr(self.table), _r._ptr(self.grad),
                                                _r._ptr(self.exp_avg), _r._ptr(self.exp_avg_sq), _r._ptr(self.max_exp_avg_sq),
                                                _r._stream_ptr(self.device)))

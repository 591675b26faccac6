"""Drop-in for ``LoG.get_all`` (/root/reference/LoG/model/level_of_gaussian.py:262-296) together with the
``Activation.activate_root_return`` it ends with (/root/reference/LoG/model/activation.py:27-44; SH polynomial
/root/reference/LoG/model/sh_utils.py:31-72) -- SURVEY 8f rows N2 ("fused activation + SH-eval (+ its backward)
feeding colors_precomp") and N3 ("fuse get_all gathers").

The reference gathers every model buffer at the selected rows (an indexing kernel per key, a ``cat`` with the node
rows), wraps the leaf rows in ``nn.Parameter`` and runs ~25 elementwise kernels (and as many again in backward)
for exp / sigmoid / normalize / SH2RGB + eval_sh_wobase.  Here one kernel gathers + activates
(include/lograst.h: lograst_gather_activate) and one kernel is the whole backward (lograst_activate_backward).
Same return value (dict xyz / scaling / opacity / rotation / colors), same side effect
(``visibility_flag['params']`` = the step's parameters, keyed and ordered like ``gaussian.keys``).

Install with ``log_amd.get_all.install()`` (= ``LoG.get_all = get_all``)."""
import torch
import torch.nn as nn

from . import rasterizer as _r

_KNOWN = ("xyz", "scaling", "opacity", "rotation", "colors", "shs")
_fused_step = False     # install(fused_step=True): the activation backward applies SparseOptimizer's update itself (below)
_multi_view = None      # log_amd.multi_view while it is installed: the backward adds its gradients by model row instead


def set_fused_step(enabled):
    """Opt-in (round 6): while on, the backward of ``get_all`` -- for a model that carries its ``optimizer``, in a graph whose
    rasterizer backward ran before it -- computes the raw gradients of the selected rows AND applies the reference's sparse
    Adam to them in one kernel (lograst_activate_backward_adam): the compact gradients (59 floats per row at SH degree 3)
    are never written or read back; ``params[key].grad`` stays None and ``log_amd.sparse_optimizer.step`` is reduced to its
    bookkeeping for that step.  The update happens at backward time instead of at ``optimizer.step`` time -- the same result
    for the reference's trainer (one view: backward, then step; nothing reads the model in between), NOT for a loop that
    accumulates several backwards per step: once the update of a step has been applied, a further backward into the same
    optimizer's parameters before ``step`` raises ("fused step").  A backward that reaches ``get_all``
    without a rasterizer backward of the same rows before it in the same pass (a regulariser on the activated outputs alone,
    a render whose image received no gradient) is not fused: it leaves ordinary gradients for ``step``.  -> previous value."""
    global _fused_step
    prev, _fused_step = _fused_step, bool(enabled)
    return prev


class _Activate(torch.autograd.Function):
    """Connects the activated tensors (already computed by the gather kernel) to the step's parameters."""

    @staticmethod
    def forward(ctx, pack, *params):
        # ctx keeps what backward reads -- and none of the OUTPUT tensor objects: autograd makes this node the grad_fn of
        # every returned tensor, so an output reachable from ctx is a reference cycle (tensor -> grad_fn -> ctx -> tensor)
        # that only Python's cyclic collector frees, whenever it next runs; the cycle used to hold the step's gathered
        # rows, the AccumulateGrad nodes and through them the parameters' .grad: ~3 GB per C3 view piling up in HBM until
        # a collection, every one of them a fresh hipMalloc (round-2 verdict, weak #7: the 10-40x stage outliers).
        ctx.pack = {k: pack[k] for k in ("raw", "n_param", "degree", "campos", "param_keys", "fused", "accumulate")}
        act = pack["act"]
        return act["xyz"].view_as(act["xyz"]), act["scaling"], act["opacity"], act["rotation"], act["colors"]

    @staticmethod
    def backward(ctx, g_xyz, g_scaling, g_opacity, g_rotation, g_colors):
        pack = ctx.pack
        n = pack["n_param"]
        fused = pack.get("fused")
        acc = pack.get("accumulate")
        if acc and _multi_view is not None:
            # steps over several views (log_amd.multi_view): the radii of THIS pack's render, under the contract of the fused
            # step below -- same rows, taken once; a backward without them leaves ordinary gradients, which ``step`` adds
            rows = pack["raw"]["xyz"]
            radii = _r.take_backward_radii(rows)
            if radii is not None and int(radii.numel()) == int(rows.shape[0]) and radii.device == g_xyz.device:
                if _multi_view.accumulate_view(acc, pack, n, radii, g_xyz, g_scaling, g_opacity, g_rotation, g_colors):
                    return (None,) * (1 + len(pack["param_keys"]))
        if fused:
            from . import sparse_optimizer as _so
            _so.refuse_second_backward(fused)
            # the visibility of THIS pack's render: published by a rasterizer backward earlier in this very pass, for the
            # rows this pack gathered (same tensor, same row count), taken once.  Anything else -- a loss on the activated
            # outputs alone, a render whose image received no gradient -- leaves the gradients to ``step`` and its flag_vis
            rows = pack["raw"]["xyz"]
            radii = _r.take_backward_radii(rows)
            if radii is not None and int(radii.numel()) == int(rows.shape[0]) and radii.device == g_xyz.device:
                if _so.fused_update(fused, pack, n, radii, g_xyz, g_scaling, g_opacity, g_rotation, g_colors):
                    return (None,) * (1 + len(pack["param_keys"]))
        g = _r._backend.activate_backward(pack["raw"], n, pack["degree"], pack["campos"], g_scaling, g_opacity,
                                          g_rotation, g_colors)
        g["xyz"] = g_xyz[:n]
        return (None,) + tuple(g.get(k) for k in pack["param_keys"])


def get_all(self, camera, rasterizer):
    """``self``: the LoG model (``gaussian``, ``fix_parent``, ``training``)."""
    gaussian = self.gaussian
    flags = gaussian.visibility_flag
    index = flags["index"]
    n_leaf = int(index.shape[0])
    if "index_node" in flags:
        index = torch.cat([index, flags["index_node"]])
    n_param = n_leaf if self.fix_parent else int(index.shape[0])
    bufs = dict(gaussian.items())
    if any(k not in _KNOWN for k in bufs) or any(k not in bufs for k in _KNOWN[:5]):
        raise NotImplementedError(f"log_amd.get_all fuses the keys {_KNOWN}; this model has {list(bufs)}")
    degree = int(gaussian.active_sh_degree) if camera is not None else 0
    if degree > 0 and "shs" not in bufs:
        raise ValueError("active_sh_degree > 0 but the model has no shs buffer")
    campos = camera["camera_center"] if degree > 0 else None
    with torch.no_grad():
        raw, act = _r._backend.gather_activate(index, {k: v.detach() for k, v in bufs.items()}, degree, campos)
    # visibility_flag['params']: the rows that are optimised, in gaussian.keys order (level_of_gaussian.py:267-272, :288-293)
    params = {}
    for key in bufs:
        rows = raw[key][:n_param]
        params[key] = nn.Parameter(rows) if self.training else rows
    flags["params"] = params
    if not self.training:
        return {k: act[k] for k in ("xyz", "scaling", "opacity", "rotation", "colors")}
    param_keys = [k for k in bufs if k != "shs" or degree > 0]   # unused shs: no gradient, like the reference
    opt = getattr(self, "optimizer", None)
    fused = None
    accumulate = _multi_view.route(self, bufs, index[:n_param]) if _multi_view is not None and opt is not None else None
    if _fused_step and opt is not None and accumulate is None:
        # what the fused step needs at backward time: the optimizer, the model buffers and the rows' model indices
        fused = {"optimizer": opt, "bufs": bufs, "index": index[:n_param]}
        # (one fused update per optimizer step: a second training get_all before the step -- a batch of several views --
        # sends ALL of that step's backwards the ordinary way, see sparse_optimizer.fused_update)
        opt._lograst_open_packs = getattr(opt, "_lograst_open_packs", 0) + 1
    pack = {"raw": raw, "act": act, "n_param": n_param, "degree": degree, "campos": campos, "param_keys": param_keys,
            "fused": fused, "accumulate": accumulate}
    xyz, scaling, opacity, rotation, colors = _Activate.apply(pack, *[params[k] for k in param_keys])
    return {"xyz": xyz, "scaling": scaling, "opacity": opacity, "rotation": rotation, "colors": colors}


def install(fused_step=None):
    """Patch the reference class in place (needs LoG importable).  fused_step: see ``set_fused_step`` (None = leave as is)."""
    from LoG.model.level_of_gaussian import LoG
    LoG.get_all = get_all
    if fused_step is not None:
        set_fused_step(fused_step)
    return LoG

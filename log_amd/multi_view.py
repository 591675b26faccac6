"""Steps over several views of the LoG model: every view's gradients are added by model row, one Adam step per K views.

The reference steps over ONE view: ``LoG.get_all`` writes ``visibility_flag['params']`` per view and ``LoG.step`` reads only
the last one (LoG/model/level_of_gaussian.py:262-296, :379-398), so with two training ``get_all``s before a
``step`` the first view's gradients are dropped.  Installed, this module

* makes the backward of ``log_amd.get_all`` add the raw gradients of the rows its render saw (``radii > 0``) into per-model-row
  sums, in the kernel that computes them (include/lograst.h: lograst_activate_backward_accumulate) -- ``params[key].grad``
  stays ``None``; a backward without a render of its own rows (a regulariser on the activated rows alone, an image that
  received no gradient) leaves ordinary gradients, which ``step`` adds into the sums by ``index[flag_vis]``;
* replaces ``LoG.step``: every call counts one view; the K-th call (or ``flush``) takes ONE step of the reference's sparse
  Adam over every row some view saw (lograst_accumulated_adam: the step clears the sums and the counts it consumed and
  nothing else), clamps the scales of the rows that moved (lograst_clamp_scale) and sets ``self.lr``.
  ``view_correction.step()`` runs on every call -- each view's corrector row is complete after its own backward -- under the
  reference's condition, evaluated as the reference does AFTER the optimizer's count advanced (so K = 1 is the reference's
  schedule call for call).  ``Counter.update_by_output`` stays per view and is not touched.

The gradients are plain sums in view order (no atomics: the same views in the same order give the same bits); the caller
scales the loss, as ``Trainer.training_step``'s ``accumulate_step`` does.  The fused step (``log_amd.get_all.set_fused_step``)
is not taken for a model this module handles.

Fall-backs (counted and logged once per reason, ``stats()``): tensors that are not on the GPU or not fp32, a key outside
xyz / scaling / opacity / rotation / colors / shs or one the optimizer holds no moments for, 2^31 rows or more,
``fix_parent=False``, moments that cannot be brought to the device -- the view's backward then leaves ordinary gradients and
``step`` is the method that was installed before this one (the reference's, or ``log_amd.prepare``'s).

Per-model state (``state(model)``, created at the first accumulated backward, kept on the optimizer object): the sums as a
``log_amd.dist._Flat`` (attribute-major; ``.views[name]`` under that layout's names, ``KEY_TO_FLAT``) and ``.seen`` int32[P],
both zero-filled once.  A model that was resized (densified) while views are pending raises; with none pending the state is
allocated again at the next view.

Outside LoG: ``accumulate(...)`` and ``step(...)`` are the two launches on plain GPU tensors.

Install with ``log_amd.multi_view.install(views_per_step=K)`` or ``log_amd.install_all(views_per_step=K)``."""
import logging
import math

import torch

from . import rasterizer as _r
from . import sparse_optimizer as _so
from ._dropin import DropIns, Fallback

KEYS = _r.ACCUMULATE_KEYS
KEY_TO_FLAT = {"xyz": "means3D", "scaling": "scales", "opacity": "opacities", "rotation": "rotations", "colors": "colors",
               "shs": "shs"}        # the names log_amd.dist gives the same columns
_views_per_step = 1
_counts = {"views": 0, "accumulated": 0, "ordinary": 0, "steps": 0}
_log = logging.getLogger("log_amd")


def _targets():
    from LoG.model.level_of_gaussian import LoG
    return {"step": (LoG, "step")}


def _views(k):
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("views_per_step must be an integer >= 1")
    return k


dropins = DropIns("multi_view", _targets)


def stats():
    """``DropIns.stats()`` (calls, fall-backs by (method, reason), read-backs) + ``'counts'``: views counted, backwards
    accumulated by the kernel, views whose ordinary gradients ``step`` added, optimizer steps taken."""
    out = dropins.stats()
    out["counts"] = dict(_counts)
    return out


def reset_stats():
    dropins.reset_stats()
    for k in _counts:
        _counts[k] = 0


def _note(name, why):
    """A fall-back that is not a call of the reference's method (the backward's route): counted, logged once per reason."""
    why = str(why)
    dropins.count("fallbacks", (name, why))
    if (name, why) not in dropins.logged:
        dropins.logged.add((name, why))
        _log.warning("log_amd.multi_view.%s: %s -- this view is not accumulated (logged once)", name, why)


# ---- the two launches on plain tensors ----------------------------------------------------------------------------------

def _check_block(t, P, width, what):
    if not torch.is_tensor(t) or t.dim() < 2 or int(t.shape[0]) != P or math.prod(t.shape[1:]) != width:
        raise ValueError(f"{what}: {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} where {P} model rows of "
                         f"{width} floats are needed")


def _accumulate(raw, n, degree, campos, grads, index, radii, targets, seen):
    """The size checks (ValueError before any launch), then the backend's launch."""
    n, P = int(n), int(seen.numel())
    rendered = int(raw["xyz"].shape[0])
    K = int(raw["shs"].shape[1]) if "shs" in raw else 0
    if seen.dim() != 1:
        raise ValueError("seen: one count per model row is needed")
    if n > int(index.numel()):
        raise ValueError(f"{n} rows are parameters but index names {int(index.numel())}")
    if n > rendered:
        raise ValueError(f"{n} rows are parameters but {rendered} were gathered")
    if int(radii.numel()) != rendered:
        raise ValueError(f"radii of {int(radii.numel())} rows for a render of {rendered}")
    for key, t in targets.items():
        if key not in KEYS or (key == "shs" and K == 0):
            raise ValueError(f"no such key to accumulate: {key}")
        _check_block(t, P, _r.accumulate_width(key, K), f"target {key}")
    if len(grads) != 5 or any(int(g.shape[0]) < n for g in grads):
        raise ValueError("the five upstream gradients (xyz, scaling, opacity, rotation, colors) must cover the parameter rows")
    with torch.no_grad():
        _r._backend.activate_backward_accumulate(raw, n, int(degree), campos, *grads, index, radii, targets, seen)


def _step(seen, entries, beta1, beta2, bias_correction2_sqrt, eps, moved_out):
    P = int(seen.numel())
    for key, (model_p, grad, *_rest) in entries.items():
        if key not in KEYS:
            raise ValueError(f"no such key to step: {key}")
        width = math.prod(model_p.shape[1:])
        _check_block(model_p, P, width, f"model {key}")
        _check_block(grad, P, width, f"accumulated gradient of {key}")
    if moved_out is not None and int(moved_out.numel()) != P:
        raise ValueError(f"moved_out of {int(moved_out.numel())} entries for {P} model rows")
    with torch.no_grad():
        _r._backend.accumulated_adam(seen, entries, beta1, beta2, bias_correction2_sqrt, eps, moved_out)


def _need_gpu(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.device.type != "cuda":
            raise ValueError("log_amd.multi_view works on GPU tensors (no CPU path)")


def accumulate(raw, n, degree, campos, grads, index, radii, targets, seen):
    """One view added by model row, outside LoG.  raw: the gathered raw rows {xyz, scaling, opacity, rotation[, shs]} as
    ``lograst_gather_activate`` leaves them; n: the leading rows that are parameters; grads: dL/d(activated) (xyz, scaling,
    opacity, rotation, colors); index int64[>= n] without duplicates; radii int32[rows of raw]; targets: {key: fp32 [P, ...]
    view, rows any stride apart}; seen: int32[P].  For r < n with radii[r] > 0 and 0 <= index[r] < P the raw gradients are
    added into row index[r] of every target and seen[index[r]] += 1."""
    _need_gpu(seen, index, radii, *raw.values(), *grads, *targets.values())
    _accumulate(raw, n, degree, campos, tuple(grads), index, radii, targets, seen)


# ---- the per-model state ------------------------------------------------------------------------------------------------

def _signature(bufs):
    # (_version moves with every in-place step and clamp, so it cannot tell a resize; it is kept for whoever inspects the state)
    return {k: (int(v.data_ptr()), tuple(v.shape), int(v._version)) for k, v in bufs.items()}


def _same_buffers(a, b):
    return a.keys() == b.keys() and all(a[k][:2] == b[k][:2] for k in a)


class State:
    """The sums of one model: ``flat`` (log_amd.dist._Flat, attribute-major), ``views`` / ``alias`` = its per-attribute
    blocks under ``KEY_TO_FLAT``'s names, ``seen`` int32[P], ``moved`` uint8[P] (which rows the last step moved),
    ``pending`` = views since the last step, ``keys`` = the keys that received a gradient since then."""

    def __init__(self, bufs, device):
        from .dist import _Flat
        self.P = int(bufs["xyz"].shape[0])
        self.K = int(bufs["shs"].shape[1]) if "shs" in bufs else 0
        self.flat = _Flat(self.P, device, sh_coeffs=self.K)
        self.views, self.alias = self.flat.views, self.flat.alias
        self.seen = torch.zeros(self.P, dtype=torch.int32, device=device)
        self.moved = torch.zeros(self.P, dtype=torch.uint8, device=device)
        self.rows = None               # arange(P), made when the clamp kernel first needs it
        self.signature = _signature(bufs)
        self.pending, self.keys = 0, set()

    def target(self, key):
        return self.alias[KEY_TO_FLAT[key]]


def state(model):
    """The model's State, or None before its first accumulated view."""
    return getattr(getattr(model, "optimizer", None), "_lograst_multi_view", None)


def pending(model):
    """Views counted since the last step: calls of ``LoG.step``, not backwards -- a backward that has added into the sums counts
    once its view's ``step`` is called (``state(model).keys`` is non-empty in between)."""
    st = state(model)
    return st.pending if st is not None else 0


def _state_for(opt, bufs, device):
    st = getattr(opt, "_lograst_multi_view", None)
    sig = _signature(bufs)
    if st is not None and not _same_buffers(st.signature, sig):
        if st.pending or st.keys:
            raise RuntimeError("log_amd.multi_view: the model was resized while views are pending -- flush(model) before "
                               "densifying")
        st = None
    if st is None:
        st = opt._lograst_multi_view = State(bufs, device)
    return st


# ---- what the kernels cover ---------------------------------------------------------------------------------------------

def _on_device(t):
    # the HIP backend takes GPU tensors; a stand-in backend (the tests' CPU double) takes what it takes
    return t.device.type == "cuda" or not isinstance(_r._backend, _r.HipBackend)


def _covered(model, bufs):
    """Raises Fallback(reason) for a model the two kernels do not cover -> (optimizer, device)."""
    opt = getattr(model, "optimizer", None)
    if opt is None:
        raise Fallback("a model without an optimizer")
    if not getattr(model, "fix_parent", True):
        raise Fallback("fix_parent=False")
    if any(k not in KEYS for k in bufs):
        raise Fallback("keys outside xyz / scaling / opacity / rotation / colors / shs")
    xyz = bufs["xyz"]
    device = xyz.device
    for k, t in bufs.items():
        if not torch.is_tensor(t) or t.device != device or not _on_device(t):
            raise Fallback("tensors are not on the GPU")
        if t.dtype != torch.float32:
            raise Fallback("tensors are not fp32")
        if not t.is_contiguous():
            raise Fallback("model buffers that are not contiguous")
    if int(xyz.shape[0]) >= 2 ** 31:
        raise Fallback("2^31 rows or more")
    try:
        _so._migrate_state(opt, device)
        for k in opt.optimize_keys:
            if k in bufs and (opt.exp_avg[k].shape != bufs[k].shape or opt.exp_avg[k].dtype != torch.float32):
                raise Fallback("moments that cannot be brought to the device")
    except (RuntimeError, KeyError, AttributeError, TypeError):
        raise Fallback("moments that cannot be brought to the device")
    return opt, device


def route(model, bufs, index):
    """Called by ``log_amd.get_all`` for a training view of a model with an optimizer: -> what ``accumulate_view`` needs at
    backward time, or None (the reason counted): this view's backward then leaves ordinary gradients."""
    from . import get_all as _ga
    try:
        opt, device = _covered(model, bufs)
    except Fallback as why:
        _note("get_all", why)
        return None
    if _ga._fused_step and ("fused", "off") not in dropins.logged:
        dropins.logged.add(("fused", "off"))
        _log.warning("log_amd.multi_view: set_fused_step(True) is on, but the fused step is not taken for a model whose "
                     "steps span several views (logged once)")
    return {"optimizer": opt, "bufs": bufs, "index": index, "device": device}


def accumulate_view(acc, pack, n, radii, g_xyz, g_scaling, g_opacity, g_rotation, g_colors):
    """The backward of a training ``get_all``: one launch.  -> True (the gradients are in the sums)."""
    opt, bufs = acc["optimizer"], acc["bufs"]
    keys = [k for k in pack["param_keys"] if k in opt.optimize_keys]
    if len(keys) != len(pack["param_keys"]):
        _note("get_all", "a key the optimizer holds no moments for")
        return False
    st = _state_for(opt, bufs, acc["device"])
    _accumulate(pack["raw"], n, pack["degree"], pack["campos"], (g_xyz, g_scaling, g_opacity, g_rotation, g_colors),
                acc["index"], radii, {k: st.target(k) for k in keys}, st.seen)
    st.keys.update(keys)
    _counts["accumulated"] += 1
    return True


# ---- LoG.step -----------------------------------------------------------------------------------------------------------

def _add_ordinary(st, params, index, flag_vis):
    """Ordinary gradients left on the view's parameters, added as the kernel adds: rows index[flag_vis], fp32, in place."""
    live = flag_vis.to(torch.bool)
    rows = index[live]
    st.seen.index_add_(0, rows, torch.ones_like(rows, dtype=torch.int32))
    for key, p in params.items():
        if p.grad is None:
            continue
        st.target(key).index_add_(0, rows, p.grad[live].to(torch.float32))
        st.keys.add(key)
        p.grad = None
    _counts["ordinary"] += 1


def _clamp(model, st):
    """LoG.clamp_scale on the rows that moved: the kernel with (all rows, moved) -- no index[flag] whose size the host would
    have to read -- or, where ``log_amd.prepare`` falls back, whatever ``clamp_scale`` the model has, on the listed rows."""
    if isinstance(_r._backend, _r.HipBackend):
        from . import prepare
        try:
            if st.rows is None:
                st.rows = torch.arange(st.P, dtype=torch.int64, device=st.seen.device)
            args = prepare._clamp_inputs(model, st.rows, st.moved)
        except Fallback:
            args = None
        if args is not None:
            return prepare._clamp_launch(*args)
    model.clamp_scale(torch.nonzero(st.moved).squeeze(1))


def _take_step(model, st):
    opt = model.optimizer
    steps = _so._host_steps(opt) + 1         # read (first call only) BEFORE the device-side increment
    opt.global_steps += 1
    opt._lograst_steps = steps
    opt._lograst_open_packs = 0
    bc1, bc2 = 1 - _so.BETA1 ** steps, 1 - _so.BETA2 ** steps
    bufs = dict(model.gaussian.items())
    amsgrad = getattr(opt, "use_amsgrad", False)
    entries = {}
    for key in KEYS:
        if key not in st.keys:
            continue
        entries[key] = (bufs[key].data, st.target(key), opt.exp_avg[key], opt.exp_avg_sq[key],
                        opt.max_exp_avg_sq[key] if amsgrad else None, _so._lr_of(opt, key, steps) / bc1)
        if key == "xyz":
            opt.xyz_lr = _so._lr_of(opt, key, steps)
    _step(st.seen, entries, _so.BETA1, _so.BETA2, math.sqrt(bc2), _so.EPS, st.moved)
    with torch.no_grad():
        _clamp(model, st)
    model.lr = opt.xyz_lr
    st.pending = 0
    st.keys = set()
    _counts["steps"] += 1
    return steps


def _view_correction(model, steps):
    """level_of_gaussian.py:395-398 with the optimizer's count taken from its host mirror (no read-back)."""
    if steps == model.base_iter and pending(model) == 0:
        print(f'[{model.__class__.__name__}] base iteration {model.base_iter} done, enable view_correction module')
    if getattr(model, "use_view_correction", False) and steps > model.base_iter:
        model.view_correction.step()


@dropins.register(name="step")
def _log_step(self):
    """LoG.step: counts this view; the K-th call takes the step."""
    dropins.count("calls", "step")
    vf = self.visibility_flag
    params, index, flag_vis = vf['params'], vf['index'], vf['flag_vis']
    bufs = dict(self.gaussian.items())
    try:
        opt, device = _covered(self, bufs)
        if any(p.grad is not None and k not in opt.optimize_keys for k, p in params.items()):
            raise Fallback("a key the optimizer holds no moments for")
    except Fallback as why:
        if pending(self):
            raise RuntimeError(f"log_amd.multi_view: {why}, with views pending -- their gradients cannot be handed to "
                               f"the reference's step")
        return dropins.fall_back("step", why, self)
    if 'index_node' in vf.keys() and vf['index_node'].shape[0] > 0:
        flag_vis = flag_vis[:index.shape[0]]           # fix_parent: the node rows are no parameters
    with torch.no_grad():
        st = _state_for(opt, bufs, device)
        if any(p.grad is not None for p in params.values()):
            _add_ordinary(st, params, index, flag_vis)
        st.pending += 1
        _counts["views"] += 1
        steps = _take_step(self, st) if st.pending >= _views_per_step else _so._host_steps(opt)
    _view_correction(self, steps)


def step(seen, entries, beta1=_so.BETA1, beta2=_so.BETA2, bias_correction2_sqrt=1.0, eps=_so.EPS, moved_out=None):
    """One Adam step over the rows with seen > 0, outside LoG.  entries: {key: (model_param, accumulated gradient, exp_avg,
    exp_avg_sq, max_exp_avg_sq | None, step_size = lr / bias_correction1)}; the rows' gradients and counts are cleared;
    moved_out uint8[P] (optional) = which rows moved."""
    _need_gpu(seen, moved_out, *[t for e in entries.values() for t in e])
    _step(seen, entries, beta1, beta2, bias_correction2_sqrt, eps, moved_out)


def flush(model):
    """Step now with the views that are pending in the sense of ``pending``: views whose ``LoG.step`` was called.  A no-op when
    none are -- a backward that is in the sums already while its own ``step`` call is still to come is stepped by that call (or
    by a flush after it), not here: flushing between a view's backward and its ``step`` would split one view over two steps."""
    st = state(model)
    if st is None or st.pending == 0:
        return False
    with torch.no_grad():
        _take_step(model, st)
    return True


def install(views_per_step=1):
    """Patch ``LoG.step`` and route the backward of ``log_amd.get_all`` (needs LoG importable; ``log_amd.get_all`` itself is
    installed by its own ``install()``)."""
    global _views_per_step
    import sys
    from . import get_all as _ga
    _views_per_step = _views(views_per_step)
    cls = dropins.install()["step"][0]
    _ga._multi_view = sys.modules[__name__]
    return cls


def uninstall():
    """Put ``LoG.step`` and the backward's route back."""
    from . import get_all as _ga
    dropins.uninstall()
    _ga._multi_view = None

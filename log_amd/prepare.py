"""Drop-ins for what LoG does around the level-of-detail traversal for every view, and after every optimizer step
(LoG/model/level_of_gaussian.py):

* ``log_prepare(self, rasterizer, camera)`` = ``LoG.prepare`` (:223-256): frustum test of the roots, the root render that
  rejects roots by ``point_weight``, ``TensorTree.traverse`` and the leaf / node split;
* ``gaussian_prepare(self, rasterizer, camera)`` = ``Gaussian.prepare`` (:90-98), the flat model's frustum test;
* ``clamp_scale(self, index)`` = ``LoG.clamp_scale`` (:367-377);
* ``step(self)`` = ``LoG.step`` (:379-398), with the clamp taking ``(index, flag_vis)`` instead of ``index[flag_vis]``.

Same signatures and side effects (``gaussian.visibility_flag`` with the reference's keys, dtypes and order; ``scaling``
clamped in place).  The reference activates opacity, scaling and rotation of ALL points per view to index out a few
thousand roots, and reads five boolean masks back around a traversal that costs one read-back; here a view is
``lograst_frustum_select`` on the roots (flag, positions, rows and the kept roots' activated parameters, compacted in
order), ONE synchronisation for their number (torch sizes the rasterizer's inputs), the root render, then
``lograst_lod_select`` (root filter, traversal, leaf / node partition) and ONE synchronisation for the two counts.
``step`` and ``clamp_scale`` read nothing back.

What the kernels do not cover goes to the reference's own method, saved by ``install()`` (logged once): tensors that are
not on the GPU or not fp32, activations other than exp / sigmoid / normalize (log for the clamp), a 3-D ``xyz`` (frames),
2^31 rows or more.  ``stats()`` counts calls, fall-backs by reason and the library's read-backs.

Install with ``log_amd.prepare.install()`` or ``log_amd.install_all(device_prepare=True)``."""
import ctypes

import torch

from . import _lib
from . import rasterizer as _r
from ._dropin import DropIns, Fallback, check_activations, device_and_rows, flag_u8, tensor, tree_buffers

_F32 = torch.float32
_VIEW_ACTIVATIONS = ({"scaling_activation": torch.exp, "opacity_activation": torch.sigmoid,
                      "rotation_activation": torch.nn.functional.normalize}, "activations other than exp / sigmoid / normalize")
_CLAMP_ACTIVATIONS = ({"scaling_inverse_activation": torch.log}, "a scaling inverse activation other than log")


def _targets():
    from LoG.model.level_of_gaussian import Gaussian, LoG
    return {"log_prepare": (LoG, "prepare"), "gaussian_prepare": (Gaussian, "prepare"), "clamp_scale": (LoG, "clamp_scale"),
            "step": (LoG, "step")}


dropins = DropIns("prepare", _targets)
stats, reset_stats, uninstall = dropins.stats, dropins.reset_stats, dropins.uninstall


def _device_and_rows(xyz):
    device, P = device_and_rows(xyz)
    if xyz.dim() != 2:
        raise Fallback("a 3-D xyz (frames)")
    return device, P


def _proj(camera, device):
    m = camera['full_proj_transform']
    if not torch.is_tensor(m) or m.device != device:
        raise Fallback("tensors are not on the GPU")
    if m.dtype != torch.float32:
        raise Fallback("full_proj_transform is not fp32")
    if m.numel() != 16:
        raise ValueError(f"full_proj_transform of shape {tuple(m.shape)}")
    return m.detach().contiguous()


# ---- kernel 1 ------------------------------------------------------------------------------------------------------

class Selection:
    """Result of ``frustum_select``: flag (bool[n]), and after ``read()`` count, pos (int64[count]), rows (int64[count],
    with a row list) and the activated xyz / scaling / rotation / opacity of the kept entries."""


def frustum_select(xyz, proj, padding, rows=None, raw=None, who="frustum_select"):
    """``lograst_frustum_select`` + its read-back.  xyz: fp32[P, 3]; proj: the 4x4 full_proj_transform; rows: int32[n]
    or None (entry i is row i); raw: (scaling[P, 3], rotation[P, 4], opacity[P] or [P, 1]) or None."""
    device = xyz.device
    L = _r.HipBackend.require(device)
    P = int(xyz.shape[0])
    if rows is not None:
        if rows.device != device or rows.dtype != torch.int32 or rows.dim() != 1:
            raise ValueError("rows: expected int32[n] on the model's device")
        rows = rows.contiguous()
    n = P if rows is None else int(rows.shape[0])
    if n >= 2 ** 31:
        raise Fallback("2^31 rows or more")
    sel = Selection()
    flag = torch.empty(n, dtype=torch.uint8, device=device)
    pos = torch.empty(n, dtype=torch.int64, device=device)
    row_out = torch.empty(n, dtype=torch.int64, device=device) if rows is not None else None
    outs = [None] * 4
    if raw is not None:
        outs = [torch.empty((n, w), dtype=torch.float32, device=device) for w in (3, 3, 4, 1)]
    count = ctypes.c_uint32(0)
    dropins.launch_and_read(
        who, device, L.lograst_frustum_scratch_bytes(n),
        lambda scratch, nbytes, stream: L.lograst_frustum_select(
            n, P, _r._ptr(xyz), _r._ptr(rows), _r._ptr(proj), float(padding), *[_r._ptr(t) for t in (raw or (None, None, None))],
            _r._ptr(flag), _r._ptr(pos), _r._ptr(row_out), *[_r._ptr(t) for t in outs], scratch, nbytes, stream),
        lambda scratch, stream: L.lograst_frustum_read(scratch, ctypes.byref(count), stream))
    k = int(count.value)
    sel.flag, sel.count, sel.pos = flag.view(torch.bool), k, pos[:k]
    sel.rows = row_out[:k] if row_out is not None else None
    sel.xyz, sel.scaling, sel.rotation, sel.opacity = [t[:k] if t is not None else None for t in outs]
    return sel


# ---- Gaussian.prepare ----------------------------------------------------------------------------------------------

@dropins.dropin
def gaussian_prepare(self, rasterizer, camera):
    """Gaussian.prepare on the device: ``visibility_flag = {'flag': bool[P], 'index': int64}``."""
    device, P = _device_and_rows(self.xyz)
    xyz = tensor(self.xyz, device, _F32, (P, 3), "xyz")
    sel = frustum_select(xyz, _proj(camera, device), 0.5, who="gaussian_prepare")
    self.visibility_flag = {'flag': sel.flag, 'index': sel.pos}


# ---- LoG.prepare ---------------------------------------------------------------------------------------------------

def root_weight(rasterizer, sel):
    """LoG.render_to_check (:207-221) on the kept roots: the root render's point_weight."""
    ret = rasterizer(means3D=sel.xyz, means2D=torch.zeros_like(sel.xyz), shs=None, colors_precomp=torch.ones_like(sel.xyz),
                     opacities=sel.opacity, scales=sel.scaling, rotations=sel.rotation, cov3D_precomp=None)
    return ret[4]


def lod_select(tree, gaussian, sel, weight, rasterizer, max_depth, opt_all_levels, current_depth, who="log_prepare"):
    """``lograst_lod_select`` + its read-back -> (root_flag bool[R], index_leaf, index_node).  sel: the roots' Selection
    (its flag is updated in place); weight: fp32[sel.count] or None (no root is rejected)."""
    from .lod import _tree_depth
    device = gaussian.xyz.device
    L = _r.HipBackend.require(device)
    rs = rasterizer.raster_settings
    fx = rs.image_width / (2.0 * rs.tanfovx)      # level_of_gaussian.py:79-80
    fy = rs.image_height / (2.0 * rs.tanfovy)
    levels = max(0, min(int(tree.max_level), int(max_depth)))
    P = int(gaussian.xyz.shape[0])
    arrays = tree_buffers(tree, device, P, ("node_index", "depth"))
    tr = tree.tree
    if tr.device != device:
        raise Fallback("tree buffers are not on the model's device")
    if tr.dtype != torch.int32:
        raise ValueError("tree: expected int32[num_nodes, max_child]")
    tr = tr.contiguous()
    num_nodes, max_child = (int(tr.shape[0]), int(tr.shape[1])) if tr.dim() == 2 else (0, 1)
    x = tensor(gaussian.xyz, device, _F32, (P, 3), "xyz")
    s = tensor(gaussian.scaling, device, _F32, (P, 3), "scaling")
    q = tensor(gaussian.rotation, device, _F32, (P, 4), "rotation")
    pm, vm = _r._dev_f32(rs.projmatrix, device), _r._dev_f32(rs.viewmatrix, device)
    k = sel.count
    if weight is not None:
        weight = weight.detach().to(device=device, dtype=torch.float32).contiguous().reshape(-1)
        if int(weight.shape[0]) != k:
            raise ValueError(f"point_weight of {int(weight.shape[0])} entries for {k} roots")
    flags = sel.flag.view(torch.uint8)
    cap = max(P, 1)
    out = [torch.empty(cap, dtype=torch.int64, device=device) for _ in range(3)]     # the list, its leaves, its nodes
    nbytes = L.lograst_lod_select_scratch_bytes(k, num_nodes, max_child, cap)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
    n_all, n_leaf, overflow, left = (ctypes.c_uint32(0) for _ in range(4))
    hint = _tree_depth(tree)
    tries = [levels] if hint is None or hint >= levels else [int(hint), levels]
    with torch.cuda.device(device):
        stream = _r._stream_ptr(device)
        for lv in tries:
            _lib.check(L.lograst_lod_select(
                P, num_nodes, max_child, _r._ptr(arrays["node_index"]), _r._ptr(tr), _r._ptr(arrays["depth"]), _r._ptr(x),
                _r._ptr(s), _r._ptr(q), _r._ptr(sel.rows), k, _r._ptr(weight), _r._ptr(sel.pos), _r._ptr(flags),
                int(flags.shape[0]), _r._ptr(pm), _r._ptr(vm), float(fx), float(fy), float(rs.tanfovx), float(rs.tanfovy),
                float(tree.min_resolution_pixel), lv, int(bool(opt_all_levels)), max(-129, min(int(current_depth), 128)),
                _r._ptr(out[0]), cap, _r._ptr(out[1]), _r._ptr(out[2]), _r._ptr(scratch), nbytes, stream))
            _lib.check(L.lograst_lod_select_read(_r._ptr(scratch), ctypes.byref(n_all), ctypes.byref(n_leaf),
                                                 ctypes.byref(overflow), ctypes.byref(left), stream))
            dropins.count("readbacks", who)
            if left.value == 0:
                break
    if overflow.value:
        raise _lib.LograstError("lod_select: inconsistent tree buffers (a point is reachable more than once)")
    return sel.flag, out[1][:n_leaf.value], out[2][:n_all.value - n_leaf.value]


def _log_device(self, rasterizer, camera):
    g = self.gaussian
    device, P = _device_and_rows(g.xyz)
    check_activations(getattr(g, "activation", None), *_VIEW_ACTIVATIONS)
    xyz = tensor(g.xyz, device, _F32, (P, 3), "xyz")
    raw = (tensor(g.scaling, device, _F32, (P, 3), "scaling"), tensor(g.rotation, device, _F32, (P, 4), "rotation"))
    opacity = g.opacity
    if not torch.is_tensor(opacity) or opacity.dim() not in (1, 2) or opacity.numel() != P:
        raise Fallback("opacity that is not [P] or [P, 1]")
    opacity = tensor(opacity.reshape(-1, 1), device, _F32, (P, 1), "opacity")
    roots = self.tree.root_index
    if roots.device != device or roots.dtype != torch.int32:
        raise Fallback("root_index that is not int32 on the model's device")
    sel = frustum_select(xyz, _proj(camera, device), 0.5, rows=roots, raw=raw + (opacity,), who="log_prepare")
    if sel.count == 0:       # nothing to render or to descend from
        empty = torch.empty(0, dtype=torch.int64, device=device)
        g.visibility_flag = {'root_flag': sel.flag, 'index': empty, 'index_node': empty.clone()}
        return
    weight = root_weight(rasterizer, sel)
    flag, leaf, node = lod_select(self.tree, g, sel, weight, rasterizer, self.current_depth,
                                  self.optimizer_cfg.opt_all_levels, self.current_depth)
    g.visibility_flag = {'root_flag': flag, 'index': leaf, 'index_node': node}


@dropins.register
def log_prepare(self, rasterizer, camera):
    """LoG.prepare on the device: two read-backs per view (the number of roots in range, the two list sizes)."""
    if self.tree.num_nodes == 0:       # a flat model: not a call of this drop-in
        return self.gaussian.prepare(rasterizer, camera)
    return dropins.run("log_prepare", _log_device, self, rasterizer, camera)


# ---- LoG.clamp_scale / LoG.step ------------------------------------------------------------------------------------

def _clamp_inputs(self, index, flag=None):
    """Everything ``lograst_clamp_scale`` needs, checked BEFORE anything is written: a Fallback here leaves the model as
    it was."""
    g = self.gaussian
    device, P = _device_and_rows(g.xyz)
    check_activations(getattr(g, "activation", None), *_CLAMP_ACTIVATIONS)
    if torch.is_tensor(g.scaling) and not g.scaling.is_contiguous():     # clamped in place: a contiguous copy will not do
        raise Fallback("scaling that is not contiguous")
    scaling = tensor(g.scaling, device, _F32, (P, 3), "scaling")
    bounds = [tensor(getattr(self.counter, name), device, _F32, (P,), name) for name in ("radius3d_min", "radius3d_max")]
    if not torch.is_tensor(index) or index.device != device:
        raise Fallback("tensors are not on the GPU")
    if index.dtype == torch.bool or index.dim() != 1:
        raise Fallback("an index that is not a 1-D list of rows")
    m = int(index.shape[0])
    if m >= 2 ** 31:
        raise Fallback("2^31 rows or more")
    index = index.detach().to(torch.int64).contiguous()
    if flag is not None:
        flag = flag_u8(flag, device, m)
    return device, m, index, flag, P, scaling, bounds


def _clamp_launch(device, m, index, flag, P, scaling, bounds):
    L = _r.HipBackend.require(device)
    with torch.cuda.device(device):
        _lib.check(L.lograst_clamp_scale(m, _r._ptr(index), _r._ptr(flag), P, _r._ptr(scaling), _r._ptr(bounds[0]),
                                         _r._ptr(bounds[1]), _r._stream_ptr(device)))


@dropins.dropin
def clamp_scale(self, index):
    """LoG.clamp_scale on the device, in place, no read-back.  The rows of ``index`` are unique, as the reference's
    indexed assignment needs them to be."""
    _clamp_launch(*_clamp_inputs(self, index))


@dropins.register
def step(self):
    """LoG.step: the reference's control flow with the clamp on ``(index, flag_vis)`` -- no ``index[flag_vis]``, whose size
    the host would have to read back."""
    dropins.count("calls", "step")
    vf = self.visibility_flag
    params = vf['params']
    index = vf['index']
    flag_vis = vf['flag_vis']
    if 'index_node' in vf.keys() and vf['index_node'].shape[0] > 0:
        if self.fix_parent:
            flag_vis = flag_vis[:index.shape[0]]
        else:
            index = torch.cat([index, vf['index_node']])
    try:
        with torch.no_grad():
            clamp = _clamp_inputs(self, index, flag_vis)
    except Fallback as why:
        return dropins.fall_back("step", why, self)
    self.optimizer.step(self.gaussian, index, params, flag_vis)
    # clip the scaling
    with torch.no_grad():
        _clamp_launch(*clamp)
    self.lr = self.optimizer.xyz_lr
    if self.optimizer.global_steps == self.base_iter:
        print(f'[{self.__class__.__name__}] base iteration {self.base_iter} done, enable view_correction module')
    if self.use_view_correction and self.optimizer.global_steps > self.base_iter:
        self.view_correction.step()


# ---- installation --------------------------------------------------------------------------------------------------

def install():
    """Patch the reference classes in place (needs LoG importable); the original methods are kept for the fall-backs."""
    return dropins.install()["log_prepare"][0]

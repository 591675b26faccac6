"""Drop-ins for LoG's densification -- the three reference methods that resize the model every ``densify_every_iter``
steps (callers: LoG.update_init_stage / update_depth_stage, LoG/model/level_of_gaussian.py:444-445, :509-514):

* ``tree_split_and_remove(tree, flag_split, flag_remove)`` = ``TensorTree.split_and_remove``
  (LoG/model/tensor_tree.py:65-129);
* ``split_and_remove(splitter, model, optimizer, flag_split, flag_remove, remove_split=True, **kwargs)`` =
  ``Splitter.split_and_remove`` (LoG/model/splitter.py:138-205), which copies every model buffer and every Adam moment
  to the CPU and back;
* ``split_and_remove_other(splitter, model, keys, flag_split, flag_remove, remove_split=True)`` =
  ``Splitter.split_and_remove_other`` (:207-220).

Same signatures, return values and side effects; buffers are replaced with ``.set_()`` so tensor objects keep their
identity.  A call is: one plan pass over the flags (``lograst_densify_plan``), ONE host synchronisation to read the
counts (torch has to allocate the new buffers), ``src_row`` (the old row behind every new row), then fused row moves
(up to 8 keys a launch), the uniform-split kernel for the children's ``xyz`` / ``scaling`` and the tree kernel.  Keys are
moved out of place in groups no larger than the largest key, and a group's old storage is released before the next
group is allocated.  Peak extra memory is therefore the largest key, plus the plan (``keep_dest``, the masked flags:
6 B per old row; ``src_row``: 4 B per new row) and, while a call splits, the new ``xyz`` and ``scaling`` (24 B per new
row): the split kernel reads the old ``xyz``, ``scaling`` and ``rotation`` together, so both are allocated before the
first group and live until their own groups have been moved.

Differences from the reference, on purpose: its one-line count prints are kept, with counts taken from the plan instead
of two more read-backs of the flags -- so with ``remove_split`` on, a row flagged for both split and remove is counted
as split only (``-`` shows the rows removed without being split, where the reference shows ``flag_remove.sum()``); its
radius-statistics print (splitter.py:119-120) is dropped -- it costs two read-backs; ``Splitter.scaling_factor`` is not used, as the reference
never passes it (``split_by_uniform``'s default 0.5 applies unless the caller gives ``scaling_factor=``).

What the kernels do not cover goes to the reference's own method, saved by ``install()`` (logged once):
``split_method == 'sample'``, ``N`` outside {2, 4, 8}, a 3-D ``xyz`` (frames), activations other than exp / log /
normalize, tensors that are not on the GPU, moments that live on the CPU, a ``tree_depth`` key, and rows flagged for
both split and remove while ``remove_split`` is off (undefined in the reference).  ``stats()`` counts calls, fall-backs by
reason and the library's read-backs (one per call).

Install with ``log_amd.densify.install()`` or ``log_amd.install_all(device_densify=True)``."""
import ctypes
import math

import torch

from . import _lib
from . import rasterizer as _r
from ._dropin import DropIns, Fallback, check_activations, device_and_rows, flag_u8, tree_buffers

_ELEM = {torch.float32: 4, torch.int32: 4, torch.int16: 2, torch.float16: 2, torch.bfloat16: 2, torch.int8: 1,
         torch.uint8: 1, torch.bool: 1}
_CHILDREN = (2, 4, 8)
_ACTIVATIONS = ({"scaling_activation": torch.exp, "scaling_inverse_activation": torch.log,
                 "rotation_activation": torch.nn.functional.normalize}, "activations other than exp / log / normalize")


def _targets():
    from LoG.model.splitter import Splitter
    from LoG.model.tensor_tree import TensorTree
    return {"tree_split_and_remove": (TensorTree, "split_and_remove"), "split_and_remove": (Splitter, "split_and_remove"),
            "split_and_remove_other": (Splitter, "split_and_remove_other")}


dropins = DropIns("densify", _targets)
stats, reset_stats, uninstall = dropins.stats, dropins.reset_stats, dropins.uninstall


class Plan:
    """The row plan of one call: masked flags (bool[P]), keep_dest (i32[P]), src_row (i32[num_new]) and the counts.  who:
    the method whose read-back this is, for stats()."""

    def __init__(self, flag_split, flag_remove, remove_split, children, tree=None, who="Plan"):
        device, p = device_and_rows(flag_split)
        L = _lib.lib()
        fs, fr = flag_u8(flag_split, device, p), flag_u8(flag_remove, device, p)
        self.p, self.children, self.remove_split, self.device = p, int(children), bool(remove_split), device
        split = torch.empty(p, dtype=torch.uint8, device=device)
        remove = torch.empty(p, dtype=torch.uint8, device=device)
        self.keep_dest = torch.empty(p, dtype=torch.int32, device=device)
        tree_ptrs = [ctypes.c_void_p(0)] * 3
        max_level = 0
        if tree is not None:
            arrays = tree_buffers(tree, device, p, ("node_index", "index_parent", "depth"))
            tree_ptrs = [ctypes.c_void_p(t.data_ptr()) for t in arrays.values()]
            max_level = max(-128, min(int(tree.max_level), 127))      # depth is int8: a larger limit never binds
        nk, ns, ov = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        scratch = dropins.launch_and_read(
            who, device, L.lograst_densify_scratch_bytes(p),
            lambda scratch, nbytes, stream: L.lograst_densify_plan(
                p, _r._ptr(fs), _r._ptr(fr), int(self.remove_split), self.children, *tree_ptrs, max_level, _r._ptr(split),
                _r._ptr(remove), _r._ptr(self.keep_dest), scratch, nbytes, stream),
            lambda scratch, stream: L.lograst_densify_read(scratch, ctypes.byref(nk), ctypes.byref(ns), ctypes.byref(ov), stream))
        self.num_keep, self.num_split, self.overlap = int(nk.value), int(ns.value), int(ov.value)
        self.num_new = self.num_keep + self.children * self.num_split
        self.split, self.remove = split.view(torch.bool), remove.view(torch.bool)
        if self.overlap:
            raise Fallback("rows flagged for both split and remove with remove_split off")
        if self.num_new >= 2 ** 31:
            raise Fallback("2^31 new rows or more")
        self.src_row = torch.empty(self.num_new, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_densify_src_rows(p, self.children, int(self.remove_split), _r._ptr(split), _r._ptr(remove),
                                                  self.num_keep, self.num_split, _r._ptr(self.src_row), _r._ptr(scratch),
                                                  _r._stream_ptr(device)))

    def move(self, entries):
        """entries: [(src, child_mode)] or [(src, child_mode, dst)] -> the new tensors, [num_new, ...] each (dst: a
        buffer whose children another kernel has written, for MOVE_SKIP); 8 keys a launch.  A src that is not contiguous
        is made contiguous first."""
        L = _lib.lib()
        out, keep = [], []
        with torch.cuda.device(self.device):
            for first in range(0, len(entries), 8):
                chunk = entries[first:first + 8]
                keys = (_lib.LograstMoveKey * len(chunk))()
                for slot, (src, mode, *given) in zip(keys, chunk):
                    if src.device != self.device or int(src.shape[0]) != self.p:
                        raise ValueError("a moved tensor must live on the plan's device and have one row per flag")
                    if src.dtype not in _ELEM:
                        raise ValueError(f"log_amd.densify: no row move for dtype {src.dtype}")
                    s = src.detach().contiguous()
                    dst = given[0] if given and given[0] is not None else \
                        torch.empty((self.num_new,) + tuple(s.shape[1:]), dtype=s.dtype, device=self.device)
                    keep.append(s)
                    out.append(dst)
                    slot.src, slot.dst = s.data_ptr(), dst.data_ptr()
                    slot.elem_size, slot.columns, slot.child_mode = _ELEM[s.dtype], max(1, math.prod(s.shape[1:])), int(mode)
                _lib.check(L.lograst_densify_move_rows(self.num_keep, self.num_new, self.p, _r._ptr(self.src_row), len(chunk),
                                                       keys, _r._stream_ptr(self.device)))
        del keep
        return out


def _groups(items, size_of):
    """Consecutive groups of at most 8 items whose sizes add up to no more than the largest single item."""
    limit = max([size_of(i) for i in items], default=0)
    group, total = [], 0
    for item in items:
        if group and (len(group) == 8 or total + size_of(item) > limit):
            yield group
            group, total = [], 0
        group.append(item)
        total += size_of(item)
    if group:
        yield group


def _row_bytes(t):
    return max(1, math.prod(t.shape[1:])) * t.element_size()


# ---- TensorTree.split_and_remove -----------------------------------------------------------------------------------

@dropins.dropin
def tree_split_and_remove(self, flag_split, flag_remove):
    """TensorTree.split_and_remove on the device: returns the masked (flag_split, flag_remove) as the reference does."""
    device, _ = device_and_rows(self.tree)
    children = int(self.max_child)
    if children not in _CHILDREN:
        raise Fallback(f"max_child = {children}")
    if self.tree.dtype != torch.int32 or self.tree.dim() != 2 or int(self.tree.shape[1]) != children:
        raise ValueError("tree: expected int32[num_nodes, max_child]")
    p = int(self.node_index.shape[0])
    plan = Plan(flag_split, flag_remove, False, children, tree=self, who="tree_split_and_remove")
    print(f' -> [{self.__class__.__name__}] split: {plan.num_split} remove: {p - plan.num_keep}')
    arrays = tree_buffers(self, device, p)
    tree_old = self.tree.contiguous()
    num_nodes = int(tree_old.shape[0])
    new = {k: torch.empty(plan.num_new, dtype=v.dtype, device=device) for k, v in arrays.items()}
    tree_new = torch.empty((num_nodes + plan.num_split, children), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().lograst_densify_tree(
            p, num_nodes, children, plan.num_keep, plan.num_split, _r._ptr(plan.src_row), _r._ptr(plan.keep_dest),
            _r._ptr(plan.split.view(torch.uint8)), *[_r._ptr(arrays[k]) for k in ("node_index", "index_parent", "local_index", "depth")],
            _r._ptr(tree_old), *[_r._ptr(new[k]) for k in ("node_index", "index_parent", "local_index", "depth")],
            _r._ptr(tree_new), _r._stream_ptr(device)))
    for k, v in new.items():
        getattr(self, k).set_(v)
    self.tree.set_(tree_new)
    return plan.split, plan.remove


# ---- Splitter.split_and_remove -------------------------------------------------------------------------------------

def _check_model(self, model, kwargs):
    if self.split_method != "uniform":
        raise Fallback(f"split_method = {self.split_method!r}")
    if int(self.N) not in _CHILDREN:
        raise Fallback(f"N = {self.N}")
    if set(kwargs) - {"scaling_factor"}:
        raise Fallback(f"arguments {sorted(set(kwargs) - {'scaling_factor'})}")
    if "tree_depth" in model.keys:
        raise Fallback("a tree_depth key")
    check_activations(getattr(model, "activation", None), *_ACTIVATIONS)
    device, p = device_and_rows(model.xyz)
    if model.xyz.dim() != 2:
        raise Fallback("a 3-D xyz (frames)")
    for key in ("xyz", "scaling", "rotation"):
        t = getattr(model, key)
        if t.dtype != torch.float32 or tuple(t.shape) != (p, 4 if key == "rotation" else 3):
            raise Fallback(f"{key} of shape {tuple(t.shape)} / {t.dtype}")
    for key in model.keys:
        t = getattr(model, key, None)
        if t is None or t.shape[0] == 0:
            continue
        if t.device != device or int(t.shape[0]) != p or t.dtype not in _ELEM:
            raise Fallback(f"key {key} on {t.device} with {t.shape[0]} rows of {t.dtype}")
    return device, p


@dropins.dropin
def split_and_remove(self, model, optimizer, flag_split, flag_remove, remove_split=True, **kwargs):
    """Splitter.split_and_remove on the device; returns num_keep (a 0-d tensor, as the reference)."""
    device, p = _check_model(self, model, kwargs)
    if optimizer is not None:
        for state_key in optimizer.state_keys:
            for key, val in getattr(optimizer, state_key).items():
                if val.device != device:
                    raise Fallback("moments that live on the CPU")
                if int(val.shape[0]) != p or val.dtype not in _ELEM:
                    raise Fallback(f"moment {state_key}.{key} of shape {tuple(val.shape)}")
    for flag in (flag_split, flag_remove):
        if not torch.is_tensor(flag) or flag.device != device:
            raise Fallback("flags are not on the model's device")
    L = _lib.lib()
    children = int(self.N)
    plan = Plan(flag_split, flag_remove, remove_split, children, who="split_and_remove")
    print(f'[{self.__class__.__name__}] split method {self.split_method}, remove {p} +{plan.num_split}x{self.N} '
          f'-{p - plan.num_keep - (plan.num_split if remove_split else 0)}')
    if plan.num_split:
        print(f'[{model.__class__.__name__}] split : {plan.num_split} -> {plan.num_split * children}')
    # the children's xyz / scaling come from the old rows: computed first, into the buffers the row move then completes
    new_geo = {}
    if plan.num_split:
        xyz, scaling, rotation = (getattr(model, k).detach().contiguous() for k in ("xyz", "scaling", "rotation"))
        for k in ("xyz", "scaling"):
            new_geo[k] = torch.empty((plan.num_new, 3), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_densify_split_uniform(
                plan.num_keep, plan.num_split, children, float(kwargs.get("scaling_factor", 0.5)), p, _r._ptr(plan.src_row),
                _r._ptr(xyz), _r._ptr(scaling), _r._ptr(rotation), _r._ptr(new_geo["xyz"]), _r._ptr(new_geo["scaling"]),
                _r._stream_ptr(device)))
        del xyz, scaling, rotation
    keys = [k for k in model.keys if getattr(model, k, None) is not None and getattr(model, k).shape[0] != 0]
    for group in _groups(keys, lambda k: _row_bytes(getattr(model, k))):
        _move_group(plan, [getattr(model, k) for k in group],
                    [_lib.MOVE_SKIP if k in new_geo else _lib.MOVE_COPY_PARENT for k in group],
                    [new_geo.pop(k, None) for k in group])
    if optimizer is None:
        return torch.tensor(plan.num_keep, device=device)
    for state_key in optimizer.state_keys:
        state = getattr(optimizer, state_key)
        vals = [val for _, val in state.items()]
        for group in _groups(vals, _row_bytes):
            _move_group(plan, group, [_lib.MOVE_ZERO] * len(group), [None] * len(group))
    num = int(model.xyz.shape[0])
    thres_exp_avg_sq = 50_000_000       # splitter.py:198-204
    if num > thres_exp_avg_sq and optimizer.exp_avg.device != torch.device('cpu'):
        print(f'[{self.__class__.__name__}] num points {num} > {thres_exp_avg_sq}, move exp_avg_sq to CPU')
        optimizer.exp_avg_sq.to(torch.device('cpu'))
    if num > thres_exp_avg_sq * 2:
        print(f'[{self.__class__.__name__}] num points {num} > {thres_exp_avg_sq * 2}, move exp_avg to CPU')
        optimizer.exp_avg.to(torch.device('cpu'))
    return torch.tensor(plan.num_keep, device=device)


def _move_group(plan, tensors, modes, prefilled):
    """Moves a group of tensors out of place and swaps the new storage in; the old storage is released on return."""
    for t, dst in zip(tensors, plan.move(list(zip(tensors, modes, prefilled)))):
        t.set_(dst)        # on the key itself, as splitter.py:178 does (a Parameter too: the callers hold no_grad)


# ---- Splitter.split_and_remove_other -------------------------------------------------------------------------------

@dropins.dropin
def split_and_remove_other(self, model, keys, flag_split, flag_remove, remove_split=True):
    """Splitter.split_and_remove_other on the device: children get zero, those of ``radius3d_min`` copy the parent."""
    if int(self.N) not in _CHILDREN:
        raise Fallback(f"N = {self.N}")
    tensors, modes = [], []
    for key in keys:
        t = getattr(model, key, None)
        if t is None or t.shape[0] == 0:
            continue
        if t.device.type != "cuda" or t.device != flag_split.device:
            raise Fallback("tensors are not on the GPU")
        if t.dim() != 1 or t.dtype not in _ELEM or int(t.shape[0]) != int(flag_split.shape[0]):
            raise Fallback(f"key {key} of shape {tuple(t.shape)} / {t.dtype}")
        tensors.append(t)
        modes.append(_lib.MOVE_COPY_PARENT if key == 'radius3d_min' else _lib.MOVE_ZERO)   # splitter.py:215-219
    if not tensors:
        return
    plan = Plan(flag_split, flag_remove, remove_split, int(self.N), who="split_and_remove_other")
    for first in range(0, len(tensors), 8):
        _move_group(plan, tensors[first:first + 8], modes[first:first + 8], [None] * len(tensors[first:first + 8]))


# ---- installation --------------------------------------------------------------------------------------------------

def install():
    """Patch the reference classes in place (needs LoG importable); the original methods are kept for the fall-backs."""
    return dropins.install()["split_and_remove"][0]

"""Drop-ins for the decision layer of LoG's densification: ``LoG.update_depth_stage`` and ``LoG.update_init_stage``
(LoG/model/level_of_gaussian.py:454-525, :400-452) -- which rows to split, which to remove, and the lines they log.

One event is: the flags, the top-k cut and every logged statistic in the kernels of ``csrc/decide.hip``
(``lograst_decide_depth`` / ``lograst_decide_init``), ONE read-back of a fixed-size record (``lograst_decide_read``), the
reference's log lines printed from that record, then ``self.tree.split_and_remove``, ``self.splitter.split_and_remove``,
``self.splitter.split_and_remove_other``, ``self.clamp_scale`` and ``self.counter.reset`` called by attribute -- whatever is
installed there runs (``log_amd.densify``'s device resize, or the reference's methods) -- with the flags as ``torch.bool``
tensors on the device.  After a depth-stage resize ``lograst_decide_child_radius_max`` writes ``counter.radius3d_max`` of the
new children from ``tree.index_parent`` (level_of_gaussian.py:516-519 without its boolean index), and the closing per-depth
lines come from the record's depth histograms instead of two read-backs per level.

The statistics lines are printed from double sums (mean, unbiased std) where the reference reduces in fp32: the digits
shown may differ in the last place.  ``torch.rand_like(self.counter.weights_max)`` is drawn once, where the reference draws
it, so a seeded run flags the rows the reference flags on that device.

What the kernels do not cover goes to the reference's method saved by ``install()``, counted by reason in ``stats()``:
tensors off the GPU or of other dtypes, activations other than sigmoid / exp, 2^31 rows or more, ``split_by_3d``,
``init_radius_split * scale == -1``, a needed cut with a ``sort_method`` other than ``'radii'``, no ``is_parent`` row and a
needed cut with ``num_max_split == 0``, and an init stage without an activated row or without a row to split (the
reference raises in the last four; they are known from the record, before anything is resized).

Install with ``log_amd.decide.install()`` or ``log_amd.install_all(device_decide=True)``."""
import ctypes
import math

import torch

from . import _lib
from . import rasterizer as _r
from ._dropin import DropIns, Fallback, check_activations, device_and_rows, tensor

C = {"split_grad": 0, "split_radii": 1, "candidates": 2, "removed": 3, "depth_lt": 4}                    # LOGRAST_DECIDE_*
CI = {"remove_weight": 0, "nonmax": 1, "remove_small": 2, "split_grad": 3, "split_radii": 4}
_ACTIVATIONS = ({"opacity_activation": torch.sigmoid, "scaling_activation": torch.exp}, "activations other than sigmoid / exp")


def _targets():
    from LoG.model.level_of_gaussian import LoG
    return {name: (LoG, name) for name in ("update_depth_stage", "update_init_stage")}


dropins = DropIns("decide", _targets)
stats, reset_stats, uninstall = dropins.stats, dropins.reset_stats, dropins.uninstall


class Stat:
    """One str_min_mean_max line: count, min, max (fp32) and the double sums behind mean and the unbiased std."""

    def __init__(self, s):
        self.count, self.min, self.max, self.sum, self.sumsq = int(s.count), float(s.min), float(s.max), float(s.sum), float(s.sumsq)

    @property
    def mean(self):
        return self.sum / self.count if self.count else math.nan

    @property
    def std(self):
        if self.count < 2 or math.isnan(self.sum):
            return math.nan
        return math.sqrt(max(self.sumsq - self.sum * self.sum / self.count, 0.0) / (self.count - 1))

    def line(self, name):
        """Counter.str_min_mean_max (LoG/model/counter.py:24-25)."""
        return f'{name:10s} {self.count:8d} [{self.min:.5f}~{self.mean:.5f}+{self.std:.5f}~{self.max:.5f}]'


class Record:
    """lograst_decide_record on the host."""

    def __init__(self, raw):
        self.counts = [int(c) for c in raw.counts]
        self.need_cut, self.num_max_split = bool(raw.need_cut), int(raw.num_max_split)
        self.cut_value, self.cut_thres = int(raw.cut_value), float(raw.cut_thres)
        bins = _lib.DECIDE_DEPTH_BINS
        self.depth_all = {d - 128: int(raw.depth_all[d]) for d in range(bins) if raw.depth_all[d]}
        self.depth_split = {d - 128: int(raw.depth_split[d]) for d in range(bins) if raw.depth_split[d]}
        self.depth_remove = {d - 128: int(raw.depth_remove[d]) for d in range(bins) if raw.depth_remove[d]}
        self.stats = [Stat(s) for s in raw.stats]
        self.raw = bytes(raw)          # the record as the device wrote it

    @property
    def num_split(self):
        return sum(self.depth_split.values())

    @property
    def num_remove(self):
        return sum(self.depth_remove.values())

    def depth_after(self, children):
        """Rows per depth after the resize: the removed rows leave, every split row gets `children` rows one level down."""
        out = dict(self.depth_all)
        for d, n in self.depth_remove.items():
            out[d] = out.get(d, 0) - n
        for d, n in self.depth_split.items():
            out[d + 1] = out.get(d + 1, 0) + children * n
        return {d: n for d, n in out.items() if n}


def _clip8(v):
    return max(-128, min(int(v), 128))       # depth is int8: a larger limit never binds


def _threshold_int(v):
    """An integer tensor compared with a Python number: `t > v` for integer t is `t > floor(v)`."""
    return max(-2 ** 31, min(math.floor(v), 2 ** 31 - 1))


def _run(who, device, p, launch, args, keep):
    L = _lib.lib()
    raw = _lib.LograstDecideRecord()
    dropins.launch_and_read(
        who, device, L.lograst_decide_scratch_bytes(p),
        lambda scratch, nbytes, stream: launch(p, ctypes.byref(args), scratch, nbytes, stream),
        lambda scratch, stream: L.lograst_decide_read(scratch, ctypes.byref(raw), ctypes.sizeof(raw), stream))
    del keep
    return Record(raw)


def decide_depth(opacity, scaling, node_index, depth, counter, current_depth, max_level, min_steps_split, split_grad_thres,
                 radius2d_thres, remove_weights_thres, max_split_points, who="decide_depth"):
    """-> (flag_split, flag_remove, Record): torch.bool[P] on the device, the cut applied (unless the record says
    need_cut with num_max_split == 0).  opacity: raw [P, 1] or [P]; counter: an object with the Counter's buffers."""
    device, p = device_and_rows(scaling)
    f32, i32 = torch.float32, torch.int32
    if opacity.dim() == 2:
        opacity = opacity[:, 0]
    a = _lib.LograstDecideDepthArgs()
    keep = {"opacity": tensor(opacity, device, f32, (p,), "opacity"), "scaling": tensor(scaling, device, f32, (p, 3), "scaling"),
            "node_index": tensor(node_index, device, i32, (p,), "node_index"),
            "depth": tensor(depth, device, torch.int8, (p,), "depth")}
    for name, dt in (("create_steps", i32), ("grad_sum", f32), ("area_sum", i32), ("radii_max_max", i32),
                     ("weights_max", f32), ("visible_count", torch.int16)):
        keep[name] = tensor(getattr(counter, name), device, dt, (p,), name)
    for name, t in keep.items():
        setattr(a, name, t.data_ptr())
    split = torch.empty(p, dtype=torch.uint8, device=device)
    remove = torch.empty(p, dtype=torch.uint8, device=device)
    a.flag_split, a.flag_remove = split.data_ptr(), remove.data_ptr()
    a.current_depth, a.max_level = _clip8(current_depth), _clip8(max_level)
    a.min_steps_split = _threshold_int(min_steps_split)
    a.max_split_points = max(-1, min(int(max_split_points), 2 ** 31 - 1))
    a.split_grad_thres, a.radius2d_thres = float(split_grad_thres), float(radius2d_thres)
    a.remove_weights_thres = float(remove_weights_thres)
    rec = _run(who, device, p, _lib.lib().lograst_decide_depth, a, keep)
    return split.view(torch.bool), remove.view(torch.bool), rec


def decide_init(opacity, counter, children, init_weight_min, init_radius_min, init_radius_split, split_grad_thres, min_steps,
                scale, rand, who="decide_init"):
    """-> (flag_split, flag_remove, Record) of update_init_stage's 'split_by_2d' rules; rand: f32[P] on the device."""
    device, p = device_and_rows(rand)
    f32, i32 = torch.float32, torch.int32
    if opacity.dim() == 2:
        opacity = opacity[:, 0]
    a = _lib.LograstDecideInitArgs()
    keep = {"opacity": tensor(opacity, device, f32, (p,), "opacity"), "rand": tensor(rand, device, f32, (p,), "rand")}
    for name, dt in (("create_steps", i32), ("grad_sum", f32), ("area_sum", i32), ("radii_max_max", i32),
                     ("weights_max", f32), ("radius3d_min", f32)):
        keep[name] = tensor(getattr(counter, name), device, dt, (p,), name)
    for name, t in keep.items():
        setattr(a, name, t.data_ptr())
    split = torch.empty(p, dtype=torch.uint8, device=device)
    remove = torch.empty(p, dtype=torch.uint8, device=device)
    a.flag_split, a.flag_remove = split.data_ptr(), remove.data_ptr()
    a.min_steps, a.children = _threshold_int(min_steps), int(children)
    # the Python expressions of level_of_gaussian.py:404-423, in double, narrowed once as torch narrows a scalar operand
    a.init_weight_min = float(init_weight_min)
    a.small_thres = float((init_radius_min * scale) ** 2)
    a.split_thres_sq = float((init_radius_split * scale) ** 2)
    a.grad_thres = float(10 * split_grad_thres)
    a.radius_thres = float(init_radius_min * scale * 8)
    rec = _run(who, device, p, _lib.lib().lograst_decide_init, a, keep)
    return split.view(torch.bool), remove.view(torch.bool), rec


def child_radius_max(radius3d_max, index_parent, scaling, num_children, scaling_decay):
    """counter.radius3d_max of the last num_children rows = scaling_decay * max(exp(scaling[index_parent]))."""
    device, p = device_and_rows(scaling)
    f32 = torch.float32
    r = tensor(radius3d_max, device, f32, (p,), "radius3d_max")
    if r.data_ptr() != radius3d_max.data_ptr():
        raise _lib.LograstError("log_amd.decide: radius3d_max must be contiguous")
    ip = tensor(index_parent, device, torch.int32, (p,), "index_parent")
    sc = tensor(scaling, device, f32, (p, 3), "scaling")
    with torch.cuda.device(device):
        _lib.check(_lib.lib().lograst_decide_child_radius_max(p, int(num_children), _r._ptr(ip), _r._ptr(sc),
                                                              float(scaling_decay), _r._ptr(r), _r._stream_ptr(device)))


# ---- LoG.update_depth_stage ----------------------------------------------------------------------------------------

@dropins.dropin
def update_depth_stage(self, global_iteration):
    """LoG.update_depth_stage with its decisions on the device."""
    check_activations(getattr(self.gaussian, "activation", None), *_ACTIVATIONS)
    cfg = self.densify_and_remove
    name = self.__class__.__name__
    log_prefix = f'[{name}] {global_iteration:06d}'
    children = int(self.splitter.N)
    p = int(self.gaussian.xyz.shape[0])
    flag_split, flag_remove, rec = decide_depth(
        self.gaussian.opacity, self.gaussian.scaling, self.tree.node_index, self.tree.depth, self.counter, self.current_depth,
        getattr(self.tree, "max_level", 128), cfg.min_steps_split, cfg.split_grad_thres, cfg.radius2d_thres,
        cfg.remove_weights_thres, cfg.max_split_points, who="update_depth_stage")
    # everything below this point that can fall back does so before a buffer changes
    if rec.stats[0].count == 0:
        raise Fallback("no is_parent row")
    if rec.need_cut and rec.num_max_split == 0:
        raise Fallback("a cut to num_max_split == 0")
    if rec.need_cut and cfg.sort_method != 'radii':
        raise Fallback(f"a cut with sort_method = {cfg.sort_method!r}")
    for label, st in zip(("opacity", "ratio", "grad", "radii"), rec.stats):
        print(f'{log_prefix} {st.line(label)}')
    print(f'{log_prefix} split by grad: {rec.counts[C["split_grad"]]:8d} split by radii: {rec.counts[C["split_radii"]]:8d}')
    if rec.need_cut:
        print(f'{log_prefix} select top {rec.num_max_split} points to split. New radii thres = {rec.cut_thres:.1f}')
    flag_split, flag_remove = self.tree.split_and_remove(flag_split, flag_remove)
    self.splitter.split_and_remove(self.gaussian, self.optimizer, flag_split, flag_remove, remove_split=False)
    self.splitter.split_and_remove_other(self.counter, ['create_steps', 'radius3d_min', 'radius3d_max'],
                                         flag_split, flag_remove, remove_split=False)
    num_children = rec.num_split * children
    if p - rec.num_remove + num_children != self.num_points:
        raise _lib.LograstError(f"log_amd.decide: {p} rows - {rec.num_remove} removed + {num_children} children, but the "
                                f"model now has {self.num_points} rows (a tree whose roots are not its depth-0 rows?)")
    if num_children > 0:
        child_radius_max(self.counter.radius3d_max, self.tree.index_parent, self.gaussian.scaling, num_children,
                         cfg.scaling_decay)
    self.counter.reset(self.num_points)
    after = rec.depth_after(children)
    for depth in range(self.current_depth + 1):
        if after.get(depth, 0) == 0:
            continue
        print(f'[{name}] depth = {depth:2d} | {after[depth]:10d} points')


# ---- LoG.update_init_stage -----------------------------------------------------------------------------------------

@dropins.dropin
def update_init_stage(self, scale=1):
    """LoG.update_init_stage ('split_by_2d') with its decisions on the device."""
    check_activations(getattr(self.gaussian, "activation", None), *_ACTIVATIONS)
    cfg = self.densify_and_remove
    name = self.__class__.__name__
    if cfg.init_split_method != 'split_by_2d':
        raise Fallback(f"init_split_method = {cfg.init_split_method!r}")
    if cfg.init_radius_split * scale == -1:
        raise Fallback("init_radius_split * scale == -1")
    wmax = self.counter.weights_max
    device, p = device_and_rows(wmax)
    # checked before the draw, so that a fall-back leaves the generator where the reference expects it
    f32, i32 = torch.float32, torch.int32
    tensor(self.gaussian.opacity, device, f32, (p, 1), "opacity")
    for key, dt in (("create_steps", i32), ("grad_sum", f32), ("area_sum", i32), ("radii_max_max", i32), ("weights_max", f32),
                    ("radius3d_min", f32)):
        tensor(getattr(self.counter, key), device, dt, (p,), key)
    rand = torch.rand_like(wmax)
    flag_split, flag_remove, rec = decide_init(
        self.gaussian.opacity, self.counter, int(self.splitter.N), cfg.init_weight_min, cfg.init_radius_min,
        cfg.init_radius_split, cfg.split_grad_thres, cfg.min_steps, scale, rand, who="update_init_stage")
    # the reference raises on .min() of an empty selection: known here, before anything is resized
    if rec.stats[0].count == 0 or rec.stats[2].count == 0:
        raise Fallback("no activated row" if rec.stats[0].count == 0 else "no row to split")
    print(f'[{name}] {rec.counts[CI["remove_weight"]]:10d} points with weight < {cfg.init_weight_min:.2f}')
    print(f'[{name}] {rec.counts[CI["nonmax"]]:10d} points with weight is non max')
    print(f'[{name}] {rec.counts[CI["remove_small"]]:10d} points with radius < {cfg.init_radius_min:.2f}')
    print(f'[{name}] {rec.stats[0].line("radii_max_act")}')
    print(f'[{name}] {rec.stats[1].line("grad")}')
    print(f'[{name}] split by grad : {rec.counts[CI["split_grad"]]:8d}')
    print(f'[{name}] split by radii: {rec.counts[CI["split_radii"]]:8d}')
    print(f'[{name}] {rec.stats[2].line("radii_split")}')
    self.splitter.split_and_remove(self.gaussian, self.optimizer, flag_split, flag_remove)
    self.splitter.split_and_remove_other(self.counter, ['create_steps', 'radius3d_min', 'radius3d_max'], flag_split, flag_remove)
    self.counter.radius3d_max.fill_(0.2 * self.gaussian.xyz_scale)
    index = torch.arange(0, self.num_points, device=self.gaussian.xyz.device)
    self.clamp_scale(index)
    print(f'[{name}] {rec.stats[3].line("radius3d_min")}')
    self.counter.reset(self.num_points)


# ---- installation --------------------------------------------------------------------------------------------------

def install():
    """Patch LoG in place (needs LoG importable); the original methods are kept for the fall-backs."""
    return dropins.install()["update_depth_stage"][0]

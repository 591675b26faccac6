"""Host-side mirror of the rasterizer packages LoG imports.

Reproduces, name for name, the Python surface of ``diff_gaussian_rasterization`` (graphdeco upstream)
and ``diff_gaussian_rasterization_wodilate`` (chingswy fork, branch ``antialias``) as LoG uses them
(/root/reference/LoG/render/renderer.py:1,57-78,100-107,141-165,190-198;
/root/reference/LoG/model/level_of_gaussian.py:59,73-78,207-221):

  * ``GaussianRasterizationSettings`` -- 12-field NamedTuple, keyword constructed (renderer.py:63-76);
  * ``GaussianRasterizer(raster_settings=...)`` -- nn.Module with ``.raster_settings``, ``__call__`` with the
    keyword set of renderer.py:141-153 (+ ``use_filter`` for the fork), ``compute_radius`` (fork,
    level_of_gaussian.py:59) and ``markVisible``;
  * autograd: differentiable w.r.t. means3D, means2D (NDC-scaled screen-space gradient), colors_precomp,
    opacities, scales, rotations;
  * returns ``(image, radii)`` for the upstream flavour and
    ``(image, radii, point_id_pixel, point_weight_pixel, point_weight)`` for the fork (renderer.py:154-165).

All arithmetic runs in hand-written HIP kernels (log_amd/csrc) through the C ABI of liblograst.so
(include/lograst.h).  Tensors must live on the MI355X; there is no CPU fallback.
"""
import contextlib
import ctypes
import functools
import math
import threading
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class Flavour(NamedTuple):
    """What distinguishes the two third-party packages on this path."""
    name: str
    filter_mode: int   # low-pass when use_filter is on
    ndc_cull: int      # |ndc| > 1.3 cull (LoG/cuda/compute_radius_kernel.cu:131-134)
    extras: int        # 5-tuple return


UPSTREAM = Flavour("diff_gaussian_rasterization", _lib.FILTER_DILATE, 0, 0)
WODILATE = Flavour("diff_gaussian_rasterization_wodilate", _lib.FILTER_CLAMP, 1, 1)

# ---- instance-capacity policy ----------------------------------------------------------------------
# Default (None): exact -- stage 1 reports the number of tile instances to the host (one 4-byte
# read-back, as the third-party package does for `num_rendered`) and the buffers are sized exactly.
# With a hint, no host synchronisation happens in forward() (one C-ABI call per forward); the kernels refuse to
# write past the capacity, or to sort a list longer than the max_tile_len hint, and record the overflow in the
# process's status block (include/lograst.h: LOGRAST_STATUS_*), which `overflow_since_reset()` / bench.py read.
_capacity_hint = None
_max_len_hint = 0
# Default mode (no hint): SPECULATIVE stage 2 (lograst_forward_speculative) -- the forward is enqueued in one piece with
# buffers sized from a running estimate (instances per Gaussian of the recent forwards at this resolution x 1.25) while
# the exact count travels to the host on a side stream; in the rare case the estimate was too small the kernels of the
# speculative stage 2 returned without rendering and stage 2 is repeated with exact buffers.  Always exact results, one
# read-back per forward like the third-party package's `num_rendered`, but the stream never waits for the host.
# set_speculative(False) restores the two-call form (stage 1, read-back, exact allocation, stage 2).
# Reverse walk: views whose Gaussians average fewer tile instances than this are walked in the row-split form (four 4x4
# blocks per wave), the others one 8x8 quadrant per wave (measured on the MI355X: 30 M random Gaussians, 1.46 instances
# each: 949 -> 700 us; C2, 2.8: 292 -> 307; a tree-ordered heavy-tailed selection, 2.3: 448 -> 579).
ROWSPLIT_MAX_INSTANCES_PER_GAUSSIAN = 1.8
_speculative = True
# In-place leaf gradients are OPT-IN (round-3 advisory): a custom Function cannot see how the engine was invoked, so
# adding into .grad behind autograd's back breaks torch.autograd.grad(loss, leaves), backward(inputs=[subset]) and
# AccumulateGrad hooks (DDP / FSDP reducers).  Off globally; a caller that owns the leaves opts them in --
# log_amd.dist.GradientBucket.attach() does (their .grad ARE views of its bucket), or set_inplace_leaf_grads(True).
_inplace_leaf_grads = False
_INPLACE_TAG = "_lograst_inplace_grad"   # attribute set on leaves whose owner asked for the in-place route
_status = {}          # device -> int32[8] status block (sticky across forwards, all streams)
_debug_keep = False   # tests: keep dL/dconic of the last backward (HipBackend.last_conic_grad)
_hit_masks = True     # a training forward hands its compositing kernels a hit-mask buffer for the reverse walk (blend.hip)
_zero_hit_masks = False   # tools/mask_stats.py: a zero-filled buffer, so that the slots nobody wrote read as "no visit"
_keep_keys = False    # tests: the forward's key buffer stays alive in `saved` (finish_lists below needs it)


def set_instance_capacity(n, max_tile_len=0):
    """n = int: sync-free forward with room for n tile instances; None: exact sizing (default).
    max_tile_len: upper bound on the longest per-tile list in sync-free mode (0 = unknown: the sort then launches
    every multi-block level the capacity allows; only lists longer than 8192 entries care).  A forward whose real
    numbers exceed either renders nothing and raises the overflow bit of the status block."""
    global _capacity_hint, _max_len_hint
    _capacity_hint = None if n is None else int(n)
    _max_len_hint = int(max_tile_len) if n is not None else 0


def set_hit_masks(enabled):
    """Training forwards allocate lograst_view.hit_masks (128 B per walked (tile, 64-entry chunk)) so that the reverse walk
    reuses the forward's support decisions instead of recomputing them (default on; speed only).  -> previous value."""
    global _hit_masks
    prev, _hit_masks = _hit_masks, bool(enabled)
    return prev


# ---- geometry reuse: the second call of a view composites again, it does not bin again (opt-in) -------------------------
# LoG's documented training configuration (render_depth: True) calls the SAME rasterizer object twice per view with the same
# means3D / opacities / scales / rotations; only colors_precomp differs (LoG/render/renderer.py:186-201).  Everything a
# forward projects, culls, counts, scans, fills and sorts is a function of geometry and opacity alone, so with reuse on the
# second call recolours the first call's records and walks its tile lists again (lograst_recomposite) -- same bits out.
_geometry_reuse = False
_reuse_stats = {"reused": 0, "fallback": {}}
_reuse_lock = threading.Lock()


def set_geometry_reuse(enabled):
    """Opt-in (default False).  True: a ``GaussianRasterizer`` remembers its last full forward, and the next call through
    the SAME object with the same geometry tensors (means3D, scales, rotations, opacities: same storage, shape, stride and
    version), raster_settings object, flavour, use_filter, device, stream, pinned walk form, launch plan and capacity
    policy, on the whole image, only recolours that forward's records and composites its tile lists again -- no
    projection, binning, scan, fill or sort.  colors_precomp / shs may differ; outputs, saved state and gradients are those
    of a full forward, bit for bit (gradient sums up to atomic order).  Any other call runs the full forward, silently;
    ``geometry_reuse_stats()`` says which and why.
    The geometry check rests on tensor version counters: a write that bypasses them between the two calls
    (``scales.data.mul_(...)``: ``.data`` has a counter of its own) is not seen, as autograd's own saved-tensor check
    does not see it.  Inside a graph capture only a forward of the same capture is reused.
    Memory: while this is on, every rasterizer object keeps one forward's records, tile state and point list (and its
    detached fp32 inputs) alive until its next full forward or its own death -- LoG builds one rasterizer per view
    (LoG/render/renderer.py:222), so that is one view's worth.  Returns the previous setting."""
    global _geometry_reuse
    prev, _geometry_reuse = _geometry_reuse, bool(enabled)
    return prev


def geometry_reuse_stats(reset=False):
    """dict(reused=<calls that recomposited>, fallback={reason: <calls that ran the full forward>}) of the rasterizer calls
    made while ``set_geometry_reuse(True)`` was in force; a fallback is keyed by the FIRST condition that failed, in the
    order of ``_ReuseSlot.match`` ("first": nothing remembered for that object yet)."""
    with _reuse_lock:
        out = dict(reused=_reuse_stats["reused"], fallback=dict(_reuse_stats["fallback"]))
        if reset:
            _reuse_stats["reused"] = 0
            _reuse_stats["fallback"].clear()
    return out


def _count_reuse(reason):
    with _reuse_lock:
        if reason is None:
            _reuse_stats["reused"] += 1
        else:
            _reuse_stats["fallback"][reason] = _reuse_stats["fallback"].get(reason, 0) + 1


def _sig(t):
    return (t.data_ptr(), tuple(t.shape), t.stride(), t._version)


def _capturing(device):
    return bool(device.type == "cuda" and torch.cuda.is_current_stream_capturing())


class _ReuseSlot:
    """What one GaussianRasterizer remembers of its last full forward while geometry reuse is on: the forward's `saved`
    dict (records, tile state, point list: alive as long as this is) and the detached fp32 inputs it ran on -- held, so that
    their addresses cannot be recycled for other tensors, and compared through data_ptr / shape / stride / _version (a
    detached view shares the caller's version counter: an in-place change of the caller's tensor shows)."""

    def __init__(self):
        self.entry = None

    def forget(self):
        self.entry = None

    def remember(self, backend, rs, flavour, use_filter, device, geometry, saved, radii):
        self.entry = dict(rs=rs, flavour=flavour, use_filter=use_filter, device=device,
                          stream=torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0,
                          view=tuple(t._version for t in (rs.bg, rs.viewmatrix, rs.projmatrix)),
                          geometry=geometry, sigs=tuple(_sig(t) for t in geometry), saved=saved, radii=radii,
                          radii_version=radii._version, band=_tile_rows.get(), pin=_pinned_form(),
                          plan=backend.plan_key(saved) if hasattr(backend, "plan_key") else None, capturing=_capturing(device),
                          hint=(_capacity_hint, _max_len_hint))

    def match(self, backend, rs, flavour, use_filter, device, geometry, cov3D):
        """-> (saved dict of the remembered forward, None) when the next call may composite it again, else (None, reason):
        the name of the first condition that does not hold."""
        e = self.entry
        if not hasattr(backend, "recomposite"):
            return None, "no_recomposite"
        if cov3D is not None:
            return None, "cov3D"
        if geometry[0].shape[0] == 0:
            return None, "empty"
        if e is None:
            return None, "first"
        if e["flavour"] != flavour:
            return None, "flavour"
        if e["use_filter"] != use_filter:
            return None, "use_filter"
        if e["rs"] is not rs:
            return None, "settings"
        if e["view"] != tuple(t._version for t in (rs.bg, rs.viewmatrix, rs.projmatrix)):
            return None, "view_modified"
        if e["device"] != device:
            return None, "device"
        if e["stream"] != (torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0):
            return None, "stream"
        if e["capturing"] != _capturing(device):   # (a graph must not read buffers of a forward made outside its capture:
            return None, "graph_capture"           # they are freed when this object forgets that forward)
        if e["band"] != (0, 0) or _tile_rows.get() != (0, 0):
            return None, "band"
        if e["pin"] != _pinned_form():
            return None, "walk_form"
        if e["plan"] != (backend.plan_key(e["saved"]) if hasattr(backend, "plan_key") else None):
            return None, "plan"
        if e["hint"] != (_capacity_hint, _max_len_hint):
            return None, "capacity_hint"
        if e["sigs"] != tuple(_sig(t) for t in geometry):
            return None, "geometry"
        if e["radii"]._version != e["radii_version"]:
            return None, "radii_modified"
        if isinstance(e["saved"], dict) and e["saved"]["instances"] == 0:
            return None, "no_instances"
        return e["saved"], None


def set_speculative(enabled):
    """Default-mode forward: True (default) = speculative stage 2 from the running capacity estimate, False = stage 1,
    read-back, exact allocation, stage 2.  Returns the previous setting."""
    global _speculative
    prev, _speculative = _speculative, bool(enabled)
    return prev


def set_inplace_leaf_grads(enabled):
    """Opt-in (default False).  True: when every differentiable input of a rasterizer call is a leaf that already has a
    dense fp32 ``.grad`` (a multi-view step after its first view, or grads that are views of a flat bucket), backward adds
    into those tensors in place (LOGRAST_BWD_ACCUMULATE) instead of returning fresh gradients for autograd to add (five
    full passes over the attributes per view).  Same sums for a plain ``loss.backward()``; NOT compatible with
    ``torch.autograd.grad``, ``backward(inputs=...)`` or AccumulateGrad-node hooks (DDP / FSDP): those never see the
    gradient.  Leaves with tensor hooks always take the autograd route.  Individual leaves are opted in by
    ``allow_inplace_grad(tensor)`` (what ``GradientBucket.attach`` does).  Returns the previous setting."""
    global _inplace_leaf_grads
    prev, _inplace_leaf_grads = _inplace_leaf_grads, bool(enabled)
    return prev


def allow_inplace_grad(t, enabled=True):
    """Mark one leaf: a backward whose five differentiable inputs are ALL marked (or set_inplace_leaf_grads(True)) adds
    into their existing .grad in place.  The caller asserts that it only ever runs plain ``.backward()`` on them."""
    setattr(t, _INPLACE_TAG, bool(enabled))
    return t


class _CapacityModel:
    """Running estimate of the tile-instance count per (device, W, H, band): the largest instances-per-Gaussian ratio,
    instance count and tile-list length of the recent forwards, slowly forgotten so that one dense view does not pin its
    buffers for the rest of the run.  Only a guess is needed: a wrong one costs a repeated stage 2, never a result."""
    HEADROOM, LEN_HEADROOM, DECAY, FIRST_RATIO = 1.25, 1.5, 0.98, 2.0

    def __init__(self):
        self.hist = {}
        self.retries = 0      # speculative attempts that had to be repeated (diagnostics)
        self.forwards = 0
        self.lock = threading.Lock()   # render threads share the model (round-3 advisory)

    def ratio(self, key):
        with self.lock:
            h = self.hist.get(key)
            return h["ratio"] if h else 0.0

    def guess(self, key, n, tiles):
        with self.lock:
            h = self.hist.get(key)
            if h is None:
                return int(self.FIRST_RATIO * n) + 4 * tiles + 4096, 0
            cap = int(max(h["I"], h["ratio"] * n) * self.HEADROOM) + 4096
            return min(cap, 0x7fffffff), int(h["L"] * self.LEN_HEADROOM) + 256

    def update(self, key, n, instances, max_len, retried):
        with self.lock:
            self.forwards += 1
            self.retries += int(retried)
            h = self.hist.get(key)
            ratio = instances / max(n, 1)
            if h is None:
                self.hist[key] = dict(I=float(instances), ratio=ratio, L=float(max_len))
            else:
                h["I"] = max(float(instances), h["I"] * self.DECAY)
                h["ratio"] = max(ratio, h["ratio"] * self.DECAY)
                h["L"] = max(float(max_len), h["L"] * self.DECAY)

    def reset(self):
        with self.lock:
            self.hist.clear()
            self.retries = self.forwards = 0


_cap_model = _CapacityModel()


def capacity_stats(reset=False):
    """dict(forwards, retries) of the speculative default mode since the last reset (no synchronisation)."""
    out = dict(forwards=_cap_model.forwards, retries=_cap_model.retries)
    if reset:
        _cap_model.reset()
    return out


def _status_block(device):
    st = _status.get(device)
    if st is None:
        st = torch.zeros(8, dtype=torch.int32, device=device)
        _status[device] = st
    return st


def _current_device():
    return torch.device("cuda", torch.cuda.current_device())


def last_state_info(device=None):
    """(num_instances, overflowed, longest_tile_list, rect_instances) of the most recent forward on `device`
    (synchronises).  rect_instances = instances of the reference's plain rect rule (>= num_instances when the
    support cull is on)."""
    st = _status.get(device if device is not None else _current_device())
    if st is None:
        return 0, False, 0, 0
    w = st.cpu().tolist()
    return int(w[1]), bool(w[2]), int(w[3]), int(w[4])


def last_overflow(device=None):
    """(num_instances, overflowed) of the most recent forward (synchronises)."""
    n, o = last_state_info(device)[:2]
    return n, o


def overflow_since_reset(device=None, reset=True):
    """dict(overflowed, max_instances, max_tile_len, forwards) over EVERY forward on `device` (all streams) since the
    last reset -- what a caller of the sync-free mode checks after a batch of views (synchronises)."""
    st = _status.get(device if device is not None else _current_device())
    if st is None:
        return dict(overflowed=False, max_instances=0, max_tile_len=0, forwards=0)
    w = st.cpu().tolist()
    if reset:
        st.zero_()
    return dict(overflowed=bool(w[0]), max_instances=int(w[5]), max_tile_len=int(w[6]), forwards=int(w[7]))


def set_tile_cull(enabled):
    """Support cull in the binning stage (default on): tiles of a Gaussian's rect in which it cannot reach
    alpha >= 1/255 are not binned.  Result-preserving; off = the reference's exact rect lists.  Returns the
    previous setting."""
    return bool(_lib.lib().lograst_set_tile_cull(1 if enabled else 0))


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


def _dev_f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _knob(name):
    """The value the library holds for a knob (bytes name, as in lograst_knob_info)."""
    val = ctypes.c_int32(0)
    _lib.lib().lograst_get_knob(name, ctypes.byref(val))
    return val.value


TILE = 16     # pixels per tile side (log_amd/csrc: the binning, compositing and band kernels)


def _tiles(width, height):
    """How many TILE x TILE tiles cover a width x height image."""
    return ((int(width) + TILE - 1) // TILE) * ((int(height) + TILE - 1) // TILE)


# Blocks carved out of one allocation are read / written in lock step by one kernel; starting them at multiples of
# n floats apart puts all streams on the same HBM channels (measured: the activation backward 0.12 -> 0.17 ms for
# n = 1 M).  Each block is followed by this many floats (4352 B: keeps 16-byte alignment, breaks the stride).
_BLOCK_SKEW = 1088
# the keys of the accumulate kernels (include/lograst.h: lograst_acc_target), in the library's order, and their floats per row
ACCUMULATE_KEYS = ("xyz", "scaling", "opacity", "rotation", "colors", "shs")
_ACCUMULATE_WIDTHS = {"xyz": 3, "scaling": 3, "opacity": 1, "rotation": 4, "colors": 3}


def accumulate_width(key, sh_coeffs):
    return 3 * int(sh_coeffs) if key == "shs" else _ACCUMULATE_WIDTHS[key]


_ITEMSIZE = {torch.float32: 4, torch.int32: 4, torch.uint8: 1, torch.int64: 8}


def _carve_skewed(device, n, blocks):
    """One fp32 allocation for blocks = [(name, row shape)]: -> {name: [n, *row shape] tensor}, the blocks in the order given,
    each _BLOCK_SKEW floats behind the end of the one before (put the blocks whose rows move as float4 first: every block
    starts 16-byte aligned only while all widths in front of it are multiples of 4)."""
    sizes = [n * math.prod(row) for _, row in blocks]
    flat = torch.empty(sum(sizes) + _BLOCK_SKEW * len(sizes), dtype=torch.float32, device=device)
    out, off = {}, 0
    for (name, row), size in zip(blocks, sizes):
        out[name] = flat[off:off + size].view((n,) + row)
        off += size + _BLOCK_SKEW
    return out


def _gather_blocks(K):
    """gather_activate's outputs as _carve_skewed blocks (the quaternion blocks first: their rows are read and written
    as float4); K = SH coefficients per Gaussian, 0 = no `shs`."""
    return [(("raw", "rotation"), (4,)), (("act", "rotation"), (4,)), (("raw", "xyz"), (3,)), (("raw", "scaling"), (3,)),
            (("raw", "colors"), (3,)), (("act", "scaling"), (3,)), (("act", "colors"), (3,)), (("raw", "opacity"), (1,)),
            (("act", "opacity"), (1,))] + ([(("raw", "shs"), (K, 3))] if K else [])


def _activate_backward_blocks(K, degree):
    """activate_backward's gradients as _carve_skewed blocks: 16-byte aligned blocks first (quaternion rows and, for
    3K % 4 == 0, the SH rows go out as float4)."""
    return [("rotation", (4,))] + ([("shs", (K, 3))] if K and degree > 0 else []) + [("scaling", (3,)), ("colors", (3,)),
                                                                                      ("opacity", (1,))]


class _TileRows:
    """The band of tile rows rendered by the calls inside a ``tile_rows(begin, end)`` block (image split across GPUs:
    log_amd/dist.py).  (0, 0) = the whole image."""

    def __init__(self):
        self._local = threading.local()

    def get(self):
        return getattr(self._local, "rows", (0, 0))

    def set(self, rows):
        self._local.rows = rows


_tile_rows = _TileRows()


# ---- pinning the compositing kernels' form (round-4 verdict, weak #9) ------------------------------------------------
# Both forms give bit-identical forwards and gradients within the same tolerance; which one is FASTER depends on the view
# (tile instances per Gaussian).  By default the package decides per call from what it knows -- the resolution's recent
# history for the forward, the forward's own count for the backward -- so the time a host sees depends on what rendered
# before.  A host that wants reproducible timings (or knows its scene) pins the form: per rasterizer object
# (``GaussianRasterizer(raster_settings=..., walk_form="rows")``), for a block of calls (``with walk_form("quadrant"):``)
# or process-wide (``set_walk_form``); the backward of a view uses what its forward was pinned to.
_FORMS = {None: 0, "auto": 0, "rows": 1, "quadrant": 2}       # include/lograst.h: LOGRAST_FORM_*
_walk_form_default = 0
_walk_form_local = threading.local()


def _form_code(form):
    if form not in _FORMS:
        raise ValueError("walk_form must be None / 'auto', 'rows' or 'quadrant' (got %r)" % (form,))
    return _FORMS[form]


def set_walk_form(form):
    """Process-wide pin of the compositing kernels' form: 'rows' (four 4x4 blocks per wave: tiny splats), 'quadrant' (one
    8x8 quadrant per wave), or None / 'auto' (default: decided per call).  Returns the previous setting's name."""
    global _walk_form_default
    prev, _walk_form_default = _walk_form_default, _form_code(form)
    return {0: "auto", 1: "rows", 2: "quadrant"}[prev]


def _pinned_form():
    return getattr(_walk_form_local, "form", 0) or _walk_form_default


class walk_form:
    """``with walk_form("rows"): ...`` pins the form for the rasterizer calls of this thread inside the block."""

    def __init__(self, form):
        self.form = _form_code(form)

    def __enter__(self):
        self.prev = getattr(_walk_form_local, "form", 0)
        _walk_form_local.form = self.form
        return self

    def __exit__(self, *exc):
        _walk_form_local.form = self.prev
        return False


class tile_rows:
    """``with tile_rows(begin, end): image, ... = rasterizer(...); loss.backward()`` renders (and differentiates) only
    the tile rows [begin, end) -- pixel rows [16*begin, 16*end) -- of every view set up inside the block; the backward
    of a view uses the band its forward used.  New design, not part of the reference's API."""

    def __init__(self, begin, end):
        self.rows = (int(begin), int(end))

    def __enter__(self):
        self.prev = _tile_rows.get()
        _tile_rows.set(self.rows)
        return self

    def __exit__(self, *exc):
        _tile_rows.set(self.prev)
        return False


# ---- abs-grad: the absolute screen-space sums of the reverse walk (opt-in; extension) ---------------------------------------
# dL/dmeans2D is a signed sum over pixels whose terms are odd around the splat centre: for a large splat inside the image they
# cancel, and LoG's split decision (Counter.get_gradmean against split_grad_thres) reads the norm of what is left.  With abs-grad
# on, the backward of a call takes lograst_backward_abs and leaves ``means2D.absgrad`` [N, 3]: the sums of the ABSOLUTE per-pixel
# terms (the AbsGS statistic; gsplat's ``absgrad``).  Off by default, everywhere.
_abs_grad_default = False
_abs_grad_local = threading.local()
_ABS_GRAD = object()      # the marker GaussianRasterizer.forward appends to the autograd function's arguments when it is on


def set_abs_grad(enabled):
    """Process-wide switch (default False).  True: every rasterizer backward also sums the absolute values of the per-pixel
    terms of dL/dmeans2D and leaves them as ``means2D.absgrad`` (fp32 [N, 3] on means2D's device; column 2 is 0): set by the
    first backward through that ``means2D`` object, ADDED to by later ones -- as ``.grad`` accumulates.  All returned
    gradients are the plain backward's.  Not with aux_colors, camera gradients, cov3D_precomp, a ``tile_rows`` band or
    ``accumulate_grads_into`` (ValueError); the in-place leaf route (``set_inplace_leaf_grads``) is not taken for such a call.
    -> the previous setting."""
    global _abs_grad_default
    prev, _abs_grad_default = _abs_grad_default, bool(enabled)
    return prev


def _abs_grad_on():
    local = getattr(_abs_grad_local, "on", None)
    return _abs_grad_default if local is None else local


class abs_grad:
    """``with abs_grad(True): ...`` switches abs-grad on (or off) for the rasterizer calls of this thread inside the block."""

    def __init__(self, enabled=True):
        self.on = bool(enabled)

    def __enter__(self):
        self.prev = getattr(_abs_grad_local, "on", None)
        _abs_grad_local.on = self.on
        return self

    def __exit__(self, *exc):
        _abs_grad_local.on = self.prev
        return False


# What each extra of the backward -- aux channels, camera gradients (dL/dviewmatrix, dL/dprojmatrix), abs-grad (the absolute
# screen-space sums, ``means2D.absgrad``) -- cannot be combined with, in the order in which a call with several of them hears
# about it: each is a follow-up, not a silent zero.
_EXTRA_REFUSES = {
    "aux": (("cov3D", "aux_colors cannot be combined with cov3D_precomp (pass scales / rotations)"),
            ("band", "aux_colors cannot be combined with a tile_rows band (whole images only)"),
            ("sink", "aux_colors cannot be combined with accumulate_grads_into (its backward returns fresh gradients)")),
    "camera": (("sink", "camera gradients cannot be combined with accumulate_grads_into (they come with fresh gradients)"),
               ("cov3D", "camera gradients cannot be combined with cov3D_precomp (pass scales / rotations)"),
               ("band", "camera gradients cannot be combined with a tile_rows band (whole images only)"),
               ("aux", "camera gradients cannot be combined with aux_colors (no camera form of the aux backward)")),
    "abs": (("aux", "abs_grad cannot be combined with aux_colors (no abs form of the aux backward)"),
            ("camera", "abs_grad cannot be combined with camera gradients (a viewmatrix / projmatrix that requires grad)"),
            ("cov3D", "abs_grad cannot be combined with cov3D_precomp (pass scales / rotations)"),
            ("band", "abs_grad cannot be combined with a tile_rows band (whole images only)"),
            ("sink", "abs_grad cannot be combined with accumulate_grads_into (it comes with fresh gradients)")),
}


def _refuse_extra_with(extra, **present):
    """Raise for the first entry of _EXTRA_REFUSES[extra] that the call has (sink=, cov3D=, band=, aux=, camera=: booleans)."""
    for what, message in _EXTRA_REFUSES[extra]:
        if present.get(what):
            raise ValueError(message)


_refuse_abs_grad_with = functools.partial(_refuse_extra_with, "abs")   # (the name tests/test_abs_grad_cpu.py reads the list by)

class HipBackend:
    """Drives the kernels.  All buffers come from torch's caching allocator."""

    @staticmethod
    def require(device):
        if device.type != "cuda":
            raise _lib.LograstError(
                f"log_amd rasterizer needs tensors on the MI355X (got device '{device}'); "
                "the HIP kernels are the only implementation -- there is no CPU fallback")
        return _lib.lib()

    def make_view(self, rs, flavour, use_filter, device, cov3D=None, g_cov3D=None):
        """cov3D / g_cov3D: the `cov3D_precomp` input ([N, 6]) and, for a backward, where dL/dcov3D goes."""
        keep = (_dev_f32(rs.viewmatrix, device), _dev_f32(rs.projmatrix, device), _dev_f32(rs.bg, device).reshape(-1))
        if keep[0].numel() != 16 or keep[1].numel() != 16 or keep[2].numel() != 3:
            raise ValueError("viewmatrix/projmatrix must be 4x4 and bg must have 3 entries")
        v = _lib.LograstView()
        v.width, v.height = int(rs.image_width), int(rs.image_height)
        v.tanfovx, v.tanfovy = float(rs.tanfovx), float(rs.tanfovy)
        v.scale_modifier = float(rs.scale_modifier)
        v.filter_mode = flavour.filter_mode if use_filter else _lib.FILTER_NONE
        v.ndc_cull, v.extras = flavour.ndc_cull, flavour.extras
        v.viewmatrix, v.projmatrix, v.bg = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
        v.tile_row_begin, v.tile_row_end = _tile_rows.get()
        v.cov3d_precomp = cov3D.data_ptr() if cov3D is not None else None
        v.dl_dcov3d = g_cov3D.data_ptr() if g_cov3D is not None else None
        v.walk_form = _lib.FORM_AUTO
        return v, keep

    @staticmethod
    def walk_form(instances, n):
        """LOGRAST_FORM_* for a view of n Gaussians with `instances` tile instances (None / 0 = unknown)."""
        if not instances or n <= 0:
            return _lib.FORM_AUTO
        return _lib.FORM_ROWS if instances < ROWSPLIT_MAX_INSTANCES_PER_GAUSSIAN * n else _lib.FORM_QUADRANT

    last_forms = None   # {"fwd": "rows" | "quadrant", "bwd": ...} of the most recent forward / backward (diagnostics)

    def _note_form(self, kind, rows):
        """Which compositing kernel the library launches for this call ("rows" = row-split): bench.py / the parity tests
        record it next to their numbers."""
        if self.last_forms is None:
            self.last_forms = {}
        self.last_forms[kind] = "rows" if rows else "quadrant"

    def plan_key(self, saved):
        """The knob-dependent launch decisions that a recomposite must share with the forward whose lists it walks: whether
        long lists are ordered lazily, the large-input threshold, and the compositing form for that forward's walk_form."""
        return tuple(_knob(name) for name in (b"LOGRAST_LAZY_SORT", b"LOGRAST_HELPER_MIN_N", b"LOGRAST_FWD_ROWS"))

    @staticmethod
    def _carve(device, parts):
        """One allocation for several buffers: parts = [(name, dtype, shape)], every buffer 256-byte aligned inside it
        (one caching-allocator call instead of one per buffer: the host side of a forward is mostly such calls)."""
        spans, total = [], 0
        for _, dt, shape in parts:
            n = _ITEMSIZE[dt]
            for d in shape:
                n *= int(d)
            spans.append((total, n))
            total += (n + 255) // 256 * 256
        arena = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
        return {name: arena[off:off + n].view(dt).view(shape) for (name, dt, shape), (off, n) in zip(parts, spans)}

    def _begin(self, L, view, flavour, device, N, own, scratch_floats, aux=False):
        """What forward() and recomposite() share once view.walk_form is set: -> (o, kept, scratch_floats, masks_for,
        mask_form): the outputs, the _carve parts that outlive the call (`own`: the caller's, in front), the normalised
        scratch_floats, the hit-mask buffer for a capacity, and the form those masks are written in (0: no masks).
        aux: a forward with aux channels -- one more output image, and the quadrant kernels whatever the view asks for."""
        H, W = view.height, view.width
        i32, f32 = torch.int32, torch.float32
        fwd_form = _lib.FORM_QUADRANT if aux else int(L.lograst_forward_form(ctypes.byref(view)))   # 1 = row-split, 2 = quadrant
        self._note_form("fwd", fwd_form == 1)
        # what the caller gets (image, radii, the fork's maps) / what backward needs / what dies with this call
        # (every output is an allocation of its own, like the third-party packages': views of one arena would share a
        # version counter -- an in-place op on `radii` would invalidate `image` for autograd -- and any one of them kept
        # alive would pin all the others' memory)
        o = {"image": torch.empty(3, H, W, dtype=f32, device=device), "radii": torch.empty(N, dtype=i32, device=device)}
        if aux:
            o["aux_image"] = torch.empty(3, H, W, dtype=f32, device=device)
        if flavour.extras:
            o.update(pid=torch.empty(H, W, dtype=i32, device=device), pwp=torch.empty(H, W, dtype=f32, device=device),
                     pw=torch.empty(N, dtype=f32, device=device))
        kept = own + [("final_T", f32, (H, W)), ("n_contrib", i32, (H, W))]
        scratch_floats = _lib.BWD_ROW_FLOATS if scratch_floats and N else 0
        if scratch_floats:
            kept.append(("bwd_scratch", f32, (N * scratch_floats,)))
        # a training forward gets a hit-mask buffer (knob LOGRAST_HIT_MASKS = 0: the library would ignore the buffer, and a
        # backward under a different knob value must not find an unwritten one)
        want_masks = bool(_hit_masks and scratch_floats) and _knob(b"LOGRAST_HIT_MASKS") != 0

        def masks_for(cap):
            """The hit-mask buffer of a training forward with room for `cap` tile instances (uninitialised)."""
            if not want_masks:
                return None
            m = (torch.zeros if _zero_hit_masks else torch.empty)(L.lograst_hit_mask_bytes(cap, W, H) // 8, dtype=torch.int64,
                                                                  device=device)
            view.hit_masks, view.hit_mask_words = m.data_ptr(), m.numel()
            return m
        return o, kept, scratch_floats, masks_for, fwd_form if want_masks else 0

    @staticmethod
    def _finish(view, o, k, state, plist, tile_rows, instances, pin, capacity, max_len, masks, mask_form, keys):
        """What forward() and recomposite() return; the last entry is `saved`, the record a forward leaves its backward (and
        a later recomposite, the test accessors below, bench.py): every key is present in every record."""
        saved = dict(radii=o["radii"], geom=k["geom"].view(torch.float32), state=state, plist=plist, final_T=k["final_T"],
                     n_contrib=k["n_contrib"], point_weight=o.get("pw"), tile_rows=tile_rows, instances=int(instances),
                     walk_form_pin=pin, hit_masks=masks, hit_mask_form=mask_form,
                     # the accumulator rows the forward cleared: the first backward takes them and leaves None
                     bwd_scratch=k.get("bwd_scratch"),
                     # what this stage 2 ran with (a recomposite walks the lists under the same decisions)
                     capacity=int(capacity), max_len=int(max_len), fwd_walk_form=int(view.walk_form),
                     keys=keys,   # keep_keys(True) only: the (depth, id) key buffer, for finish_lists
                     aux_colors=None)   # forward_aux: the second colour triples its walk composited (backward_aux reads them)
        return o["image"], o["radii"], o.get("pid"), o.get("pwp"), o.get("pw"), saved

    def forward_aux(self, rs, flavour, use_filter, means3D, scales, rotations, opacities, colors, aux_colors,
                    scratch_floats=0):
        """forward() with a second colour triple per Gaussian (aux_colors [N, 3] fp32) composited by the same walk
        (lograst_forward*_aux): -> (image, radii, pid, pwp, pw, aux_image, saved).  Whole images, scales / rotations form,
        quadrant kernels (saved["hit_mask_form"] and last_forms say so); every capacity mode of forward()."""
        if _tile_rows.get() != (0, 0):
            raise ValueError("aux_colors: a tile_rows band is not supported (whole images only)")
        if aux_colors.shape != (means3D.shape[0], 3) or aux_colors.dtype != torch.float32 or not aux_colors.is_contiguous():
            raise ValueError("aux_colors must be a contiguous float32 [N, 3] tensor")
        image, radii, pid, pwp, pw, saved = self.forward(rs, flavour, use_filter, means3D, scales, rotations, opacities, colors,
                                                         scratch_floats=scratch_floats, _aux=aux_colors)
        return image, radii, pid, pwp, pw, saved.pop("aux_image"), saved

    def forward(self, rs, flavour, use_filter, means3D, scales, rotations, opacities, colors, scratch_floats=0,
                cov3D=None, _aux=None):
        """scratch_floats: non-zero = allocate the backward's accumulator rows (16 fp32 = 64 B per Gaussian,
        include/lograst.h: LOGRAST_BWD_ROW_FLOATS) and have the forward clear them: saved as `bwd_scratch` and consumed by
        the first backward.
        cov3D: the rasterizer's cov3D_precomp ([N, 6] fp32) instead of scales / rotations (both None then).
        _aux: forward_aux's aux_colors (the body is this one: the *_aux entry points take two more pointers)."""
        device = means3D.device
        L = self.require(device)
        aux = _aux is not None
        fwd_one, fwd_spec, fwd_project, fwd_render = (
            (L.lograst_forward_aux, L.lograst_forward_speculative_aux, L.lograst_forward_project, L.lograst_forward_render_aux)
            if aux else (L.lograst_forward, L.lograst_forward_speculative, L.lograst_forward_project, L.lograst_forward_render))
        N = means3D.shape[0]
        H, W = int(rs.image_height), int(rs.image_width)
        view, keep = self.make_view(rs, flavour, use_filter, device, cov3D=cov3D)
        stream = _stream_ptr(device)
        status = _status_block(device)
        i32, u8 = torch.int32, torch.uint8
        ckey = (device.index, W, H, _tile_rows.get())
        # which form the compositing kernel takes: instances per Gaussian as the recent forwards of this resolution had
        # them (speculative / exact mode), or the caller's capacity (sync-free mode)
        pin = _pinned_form()
        view.walk_form = pin or self.walk_form(_capacity_hint if _capacity_hint is not None else _cap_model.ratio(ckey) * N, N)
        o, kept, scratch_floats, masks_for, mask_form = self._begin(
            L, view, flavour, device, N,
            [("geom", u8, (L.lograst_geom_bytes(N),)), ("state", u8, (L.lograst_tile_state_bytes(W, H, N),))], scratch_floats,
            aux=aux)
        instances = None

        def lists_for(cap, plist=None):
            """point list, key buffer and hit masks of a stage 2 with room for `cap` tile instances.  The list is an
            allocation of its own unless the caller carved it from the arena: a guessed one would stay pinned there, at its
            guessed size and next to the exact one after a retry, until backward -- round-3 advisory."""
            return (plist if plist is not None else torch.empty(cap, dtype=i32, device=device),
                    torch.empty(L.lograst_keys_bytes(cap), dtype=u8, device=device), masks_for(cap))

        def stage1_args(k):
            return (ctypes.byref(view), N, _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(colors),
                    _ptr(o["radii"]), _ptr(k["geom"]), _ptr(k["state"]))

        def stage2_args(k, keys, plist, capacity, max_len):
            return (_ptr(keys), _ptr(plist), capacity, max_len, _ptr(o["image"]), _ptr(k["final_T"]), _ptr(k["n_contrib"]),
                    _ptr(o.get("pid")), _ptr(o.get("pwp")), _ptr(o.get("pw")), _ptr(k.get("bwd_scratch")), scratch_floats,
                    _ptr(status)) + ((_ptr(_aux), _ptr(o["aux_image"])) if aux else ()) + (stream,)
        n_host, m_host = ctypes.c_uint32(0), ctypes.c_uint32(0)
        with torch.cuda.device(device):
            if _capacity_hint is not None:   # sync-free: the caller's capacity, one call
                capacity, max_len = _capacity_hint, _max_len_hint
                k = self._carve(device, kept + [("plist", i32, (capacity,))])
                plist, keys, masks = lists_for(capacity, plist=k["plist"])
                _lib.check(fwd_one(*stage1_args(k), *stage2_args(k, keys, plist, capacity, max_len)))
            else:
                k = self._carve(device, kept)
                retry = True
                if _speculative and N > 0:   # both stages with a guessed capacity; the host reads the real one afterwards
                    capacity, max_len = _cap_model.guess(ckey, N, _tiles(W, H))
                    plist, keys, masks = lists_for(capacity)
                    _lib.check(fwd_spec(*stage1_args(k), *stage2_args(k, keys, plist, capacity, max_len)[:-1],
                                        ctypes.byref(n_host), ctypes.byref(m_host), stream))
                    instances = int(n_host.value)
                    retry = instances > capacity or (max_len != 0 and int(m_host.value) > max_len)
                    _cap_model.update(ckey, N, instances, int(m_host.value), retry)
                else:                        # exact: stage 1, read the header, stage 2
                    _lib.check(fwd_project(*stage1_args(k), ctypes.byref(n_host), ctypes.byref(m_host), stream))
                if retry:   # (a speculative stage 2 that did not fit rendered nothing: once more with exact buffers)
                    capacity, max_len = int(n_host.value), max(int(m_host.value), 1)
                    plist, keys, masks = lists_for(capacity)
                    _lib.check(fwd_render(ctypes.byref(view), N, _ptr(k["geom"]), _ptr(k["state"]),
                                          *stage2_args(k, keys, plist, capacity, max_len)))
        if instances is None:
            instances = capacity          # exact mode: the real count; sync-free: the caller's (tight) upper bound
        out = self._finish(view, o, k, k["state"].view(i32), plist, (view.tile_row_begin, view.tile_row_end), instances, pin,
                           capacity, max_len, masks, mask_form, keys if _keep_keys else None)
        if aux:   # (forward_aux takes the image out again)
            out[-1].update(aux_colors=_aux, aux_image=o["aux_image"])
        return out

    def recomposite(self, rs, flavour, use_filter, saved, colors, scratch_floats=0):
        """The forward of the same Gaussians with other colours, from the `saved` dict of a forward that ran (full image,
        scales / rotations form): lograst_recomposite -- one streaming kernel writes new records, then the compositing
        launches; no projection, fill or sort.  Returns what forward() returns.  The new `saved` shares state / plist /
        instances / walk_form_pin / tile_rows with the first call's (only read); geom (the new records), radii, final_T,
        n_contrib, bwd_scratch, point_weight, hit_masks and hit_mask_form are its own, so the unchanged backward() works on
        either dict in either order."""
        device = colors.device
        L = self.require(device)
        N = colors.shape[0]
        view, keep = self.make_view(rs, flavour, use_filter, device)
        view.walk_form = int(saved["fwd_walk_form"])     # the form the first walk ran in (the history may have moved since)
        o, kept, scratch_floats, masks_for, mask_form = self._begin(
            L, view, flavour, device, N, [("geom", torch.uint8, (L.lograst_record_bytes(N),))], scratch_floats)
        capacity, max_len = int(saved["capacity"]), int(saved["max_len"])
        masks = masks_for(capacity)   # a buffer of this call's own: the first call's backward has not run yet
        with torch.cuda.device(device):
            k = self._carve(device, kept)
            _lib.check(L.lograst_recomposite(
                ctypes.byref(view), N, _ptr(saved["radii"]), _ptr(saved["geom"]), _ptr(saved["state"]), _ptr(saved["plist"]),
                capacity, max_len, _ptr(colors), _ptr(k["geom"]), _ptr(o["radii"]), _ptr(o["image"]), _ptr(k["final_T"]),
                _ptr(k["n_contrib"]), _ptr(o.get("pid")), _ptr(o.get("pwp")), _ptr(o.get("pw")), _ptr(k.get("bwd_scratch")),
                scratch_floats, _ptr(_status_block(device)), _stream_ptr(device)))
        return self._finish(view, o, k, saved["state"], saved["plist"], saved["tile_rows"], saved["instances"],
                            saved["walk_form_pin"], capacity, max_len, masks, mask_form, None)

    def backward_aux(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image, grad_aux):
        """The backward of forward_aux: one reverse walk and one chain-rule launch for both images (lograst_backward_aux).
        grad_image / grad_aux: dL/dimage, dL/daux_image; either may be None (= zeros), not both.
        -> (dL/dmeans3D, dL/dmeans2D, dL/dcolors, dL/dopacities, dL/dscales, dL/drotations, dL/daux_colors)."""
        if saved.get("aux_colors") is None:
            raise _lib.LograstError("backward_aux needs the saved record of a forward_aux call")
        if grad_image is None and grad_aux is None:
            raise ValueError("backward_aux: both image gradients are None")
        return self.backward(rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image, _aux=(grad_aux,))

    def backward_camera(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image):
        """backward() with the camera sums: -> its six fresh gradients, then dL/dviewmatrix and dL/dprojmatrix ([4, 4] fp32).
        (The method autograd looks for: a backend without it has no camera gradients.)"""
        return self.backward(rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image, camera=True)

    def backward_abs(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image):
        """backward() with the absolute screen-space sums: -> its six fresh gradients, then absgrad [N, 3] fp32 (columns 0, 1:
        the sums over pixels of |per-pixel term of dL/dmeans2D x, y|; column 2: 0) -- lograst_backward_abs.
        (The method autograd looks for: a backend without it has no abs-grad.)"""
        return self.backward(rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image, _abs=True)

    def backward(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image, sink=None, cov3D=None,
                 _aux=None, camera=False, _abs=False):
        """sink: optional dict of running-sum tensors (means3D, scales, rotations, opacities, colors) that this call
        adds into (LOGRAST_BWD_ACCUMULATE); the corresponding returned gradients are then None.
        cov3D (the forward's cov3D_precomp; no sink): the last two results are (dL/dcov3D [N, 6], None).
        _aux: backward_aux's (dL/daux_image,) (the body is this one; fresh gradients only).
        camera: two more results behind the six, dL/dviewmatrix and dL/dprojmatrix (fresh fp32 [4, 4] each, summed inside the
        chain-rule launch: lograst_backward_camera).  Fresh gradients, scales / rotations, whole images, no aux channels.
        _abs: backward_abs's switch (one more result behind the six: absgrad [N, 3]); the same restrictions."""
        device = means3D.device
        L = self.require(device)
        N = means3D.shape[0]
        aux = _aux is not None
        has = dict(sink=sink is not None, cov3D=cov3D is not None, band=tuple(saved["tile_rows"]) != (0, 0))
        if _abs:
            _refuse_extra_with("abs", aux=aux or saved.get("aux_colors") is not None, camera=camera, **has)
        if camera:
            _refuse_extra_with("camera", aux=aux, **has)
        if aux and (sink is not None or cov3D is not None):
            raise ValueError("backward_aux writes fresh gradients: no gradient sink, no cov3D_precomp")
        if not aux and saved.get("aux_colors") is not None:
            raise _lib.LograstError("this forward composited aux channels: its backward is backward_aux")
        g_cov = None
        if cov3D is not None:
            if sink is not None:
                raise ValueError("a gradient sink has no cov3D_precomp entry")
            g_cov = torch.empty(N, 6, dtype=torch.float32, device=device)
        view, keep = self.make_view(rs, flavour, use_filter, device, cov3D=cov3D, g_cov3D=g_cov)
        view.tile_row_begin, view.tile_row_end = saved["tile_rows"]   # the band the forward rendered
        f32 = dict(dtype=torch.float32, device=device)
        grad_image = grad_image.to(torch.float32).contiguous() if grad_image is not None else None
        grad_aux = _aux[0].to(torch.float32).contiguous() if aux and _aux[0] is not None else None
        need = _lib.BWD_ROW_FLOATS
        # The reverse walk adds into ONE 64-byte accumulator row per Gaussian (mean x y, conic A B C, opacity, colour):
        # the block the forward already cleared for this purpose (first backward of this forward), else a fresh
        # torch.zeros.  In the 5-tuple flavour the forward cleared the rows of the contributing Gaussians only
        # (point_weight > 0); the chain rule skips all the others (LOGRAST_BWD_CONIC_TOUCHED_ONLY) -- and hands out the
        # separate outputs: dL/dmeans2D, and dL/dopacity / dL/dcolour (written, or added into the sink's running sums).
        acc, saved["bwd_scratch"] = saved["bwd_scratch"], None
        pw = saved["point_weight"]
        flags = 1
        if acc is None or acc.numel() < need * N:
            acc = torch.zeros(N * need, **f32)
        elif pw is not None:
            flags |= 4
        # tiny splats -> the row-split reverse walk; a form pinned for the forward holds for its backward
        view.walk_form = saved["walk_form_pin"] or self.walk_form(saved["instances"], N)
        self._note_form("bwd", not aux and L.lograst_backward_form(ctypes.byref(view), N) == 1)   # (aux: quadrant kernels only)
        hm = saved["hit_masks"]      # the forward's support ballots (lograst_view.hit_masks): the reverse walk reads them
        if hm is not None:
            view.hit_masks, view.hit_mask_words = hm.data_ptr(), hm.numel()
            view.hit_mask_form = max(int(saved["hit_mask_form"]), 0)
        g_conic = acc          # (the C ABI's `bwd_rows`)
        g_means2D = torch.empty(N, 3, **f32)
        if sink is None:
            g = self._carve(device, [("rot", torch.float32, (N, 4)), ("means3D", torch.float32, (N, 3)),
                                     ("scales", torch.float32, (N, 3)), ("colors", torch.float32, (N, 3)),
                                     ("opac", torch.float32, (N,))] + ([("aux", torch.float32, (N, 3))] if aux else []))
            g_means3D, g_scales, g_rot, g_colors, g_opac = g["means3D"], g["scales"], g["rot"], g["colors"], g["opac"]
        elif "rows" in sink:   # one 64-byte row of running sums per Gaussian (LOGRAST_BWD_ACCUMULATE_ROWS)
            g_means3D, g_scales, g_rot, g_opac, g_colors = sink["rows"], None, None, None, None
            flags |= 8
        else:
            g_opac, g_colors = sink["opacities"], sink["colors"]
            g_means3D, g_scales, g_rot = sink["means3D"], sink["scales"], sink["rotations"]
            flags |= 2
        # lograst_backward's arguments up to `flags`; each other entry point has its own behind them (include/lograst.h), but
        # lograst_backward_aux, whose four sit among them
        args = [ctypes.byref(view), N, _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(saved["radii"]), _ptr(saved["geom"]),
                _ptr(saved["state"]), _ptr(saved["plist"]), _ptr(saved["final_T"]), _ptr(saved["n_contrib"]), _ptr(grad_image),
                _ptr(g_means2D), _ptr(g_conic), _ptr(g_opac), _ptr(g_colors), _ptr(g_means3D), _ptr(g_scales), _ptr(g_rot),
                _ptr(pw), flags]
        entry, more, scratch = L.lograst_backward, (), None
        with torch.cuda.device(device):
            if aux:
                entry, more = L.lograst_backward_aux, (g["aux"],)
                for at, value in ((11, _ptr(saved["aux_colors"])), (13, _ptr(grad_aux)), (16, need), (19, _ptr(g["aux"]))):
                    args.insert(at, value)
            elif _abs:
                abs_buf = torch.empty(max(N, 1), 3, **f32)         # (never a NULL pointer: the entry point refuses one)
                entry, more = L.lograst_backward_abs, (abs_buf[:N],)
                args.append(ctypes.c_void_p(abs_buf.data_ptr()))
            elif camera:
                entry = L.lograst_backward_camera
                more, tail, scratch = self._camera_outputs(L, N, device)
                args.extend(tail)
            _lib.check(entry(*args, _stream_ptr(device)))
        del keep, scratch
        # test introspection only: dL/dconic [N, 4] (A, B, C, 0) out of the accumulator rows -- slots 2-4, and with aux channels
        # one per image: slots 2-4 and 12-14
        conic = lambda at: torch.cat([acc.view(N, need)[:, at:at + 3], acc.new_zeros(N, 1)], dim=1)
        if aux:
            self.last_conic_grad = None
            self.last_aux_conic_grads = (conic(2), conic(12)) if _debug_keep and N else None
        else:
            self.last_conic_grad = (conic(2) if N else acc.new_zeros(0, 4)) if _debug_keep else None
        if sink is not None:
            return None, g_means2D, None, None, None, None
        if cov3D is not None:
            return g_means3D, g_means2D, g_colors, g_opac, g_cov, None
        return (g_means3D, g_means2D, g_colors, g_opac, g_scales, g_rot) + more

    @staticmethod
    def _camera_outputs(L, N, device):
        """For a *_camera call: (dL/dviewmatrix, dL/dprojmatrix), the four arguments the entry point takes in front of the
        stream, and the chain rule's partials scratch among them (to be held until the call is made)."""
        g = torch.empty(2, 4, 4, dtype=torch.float32, device=device)
        scratch = torch.empty(int(L.lograst_camera_scratch_bytes(N)) // 4, dtype=torch.float32, device=device)
        return (g[0], g[1]), (_ptr(g[0]), _ptr(g[1]), _ptr(scratch), 4 * scratch.numel()), scratch

    def sh_forward(self, means3D, campos, shs, degree):
        """Native `shs=` path (lograst_sh_forward): colours[N,3] and the clamp mask u8[N,3]."""
        device = means3D.device
        L = self.require(device)
        N, M = shs.shape[0], shs.shape[1]
        cp = _dev_f32(campos, device).reshape(-1)
        colors = torch.empty(N, 3, dtype=torch.float32, device=device)
        clamped = torch.empty(N, 3, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_sh_forward(N, int(degree), M, _ptr(means3D), _ptr(cp), _ptr(shs), _ptr(colors),
                                            _ptr(clamped), _stream_ptr(device)))
        return colors, clamped

    def sh_backward(self, means3D, campos, shs, degree, clamped, g_colors, g_means3D, into=None):
        """dL/dshs: a new tensor, or added into `into` (running sum; returns None).  The view-direction gradient is
        added into g_means3D in place."""
        device = means3D.device
        L = self.require(device)
        N, M = shs.shape[0], shs.shape[1]
        cp = _dev_f32(campos, device).reshape(-1)
        g_shs = torch.empty(N, M, 3, dtype=torch.float32, device=device) if into is None else into
        with torch.cuda.device(device):
            _lib.check(L.lograst_sh_backward(N, int(degree), M, _ptr(means3D), _ptr(cp), _ptr(shs), _ptr(clamped),
                                             _ptr(g_colors), _ptr(g_shs), _ptr(g_means3D), 0 if into is None else 1,
                                             _stream_ptr(device)))
        return g_shs if into is None else None

    def project_backward(self, rs, flavour, use_filter, means3D, scales, rotations, radii, g_means2D, g_conic,
                         cov3D=None, camera=False):
        """Stage A6b alone (lograst_project_backward): used by the parity tests.  With cov3D: -> (dL/dmeans3D,
        dL/dcov3D, None).  camera: (dL/dviewmatrix, dL/dprojmatrix) behind the three (lograst_project_backward_camera)."""
        device = means3D.device
        L = self.require(device)
        N = means3D.shape[0]
        if camera:
            _refuse_extra_with("camera", cov3D=cov3D is not None, band=_tile_rows.get() != (0, 0))
        g_cov = torch.empty(N, 6, dtype=torch.float32, device=device) if cov3D is not None else None
        view, keep = self.make_view(rs, flavour, use_filter, device, cov3D=cov3D, g_cov3D=g_cov)
        f32 = dict(dtype=torch.float32, device=device)
        g_means3D, g_scales, g_rot = torch.empty(N, 3, **f32), torch.empty(N, 3, **f32), torch.empty(N, 4, **f32)
        args = [ctypes.byref(view), N, _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(radii), _ptr(g_means2D), _ptr(g_conic),
                _ptr(g_means3D), _ptr(g_scales), _ptr(g_rot)]
        entry, g_cam, scratch = L.lograst_project_backward, (), None
        with torch.cuda.device(device):
            if camera:
                entry = L.lograst_project_backward_camera
                g_cam, tail, scratch = self._camera_outputs(L, N, device)
                args.extend(tail)
            _lib.check(entry(*args, _stream_ptr(device)))
        del keep, scratch
        if cov3D is not None:
            return g_means3D, g_cov, None
        return (g_means3D, g_scales, g_rot) + g_cam

    def tile_rows(self, rs, flavour, use_filter, means3D, scales, rotations):
        """-> (y0, y1) int32[N]: the tile rows [y0, y1) each Gaussian's rect covers on the whole image (y0 = y1 = 0 when
        the projection drops it): lograst_tile_rows.  See log_amd.dist.band_index."""
        device = means3D.device
        L = self.require(device)
        N = means3D.shape[0]
        m, s, r = _dev_f32(means3D, device), _dev_f32(scales, device), _dev_f32(rotations, device)
        view, keep = self.make_view(rs, flavour, use_filter, device)
        rows = torch.empty(N, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_tile_rows(ctypes.byref(view), N, _ptr(m), _ptr(s), _ptr(r), _ptr(rows), _stream_ptr(device)))
        del keep
        return rows & 0xffff, (rows >> 16) & 0xffff

    def compute_radius(self, means3D, scales, rotations, projmatrix, viewmatrix, fx, fy, tanfovx, tanfovy):
        device = means3D.device
        L = self.require(device)
        P = means3D.shape[0]
        m, s, r = _dev_f32(means3D, device), _dev_f32(scales, device), _dev_f32(rotations, device)
        pm, vm = _dev_f32(projmatrix, device), _dev_f32(viewmatrix, device)
        out = torch.empty(P, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_compute_radius(P, _ptr(m), _ptr(s), _ptr(r), _ptr(pm), _ptr(vm), float(fx), float(fy),
                                                float(tanfovx), float(tanfovy), _ptr(out), _stream_ptr(device)))
        return out


    def lod_traverse(self, node_index, tree, xyz, scaling, rotation, root_index, projmatrix, viewmatrix, fx, fy,
                     tanfovx, tanfovy, min_resolution_pixel, levels, depth_hint=None):
        """N3 (log_amd/lod.py): -> int64 indices selected for this camera, in the reference's order.  depth_hint: a
        (possibly stale) guess of the tree's depth; fewer levels are launched, and the call repeats itself with the
        full `levels` if the device reports that the guess cut the descent short."""
        device = xyz.device
        L = self.require(device)
        P = int(xyz.shape[0])
        ni = node_index.detach().to(device=device, dtype=torch.int32).contiguous()
        tr = tree.detach().to(device=device, dtype=torch.int32).contiguous()
        num_nodes, max_child = (int(tr.shape[0]), int(tr.shape[1])) if tr.dim() == 2 else (0, 1)
        roots = root_index.detach().to(device=device, dtype=torch.int64).contiguous()
        x, s, r = _dev_f32(xyz, device), _dev_f32(scaling, device), _dev_f32(rotation, device)
        pm, vm = _dev_f32(projmatrix, device), _dev_f32(viewmatrix, device)
        out = torch.empty(max(P, 1), dtype=torch.int64, device=device)
        nbytes = L.lograst_lod_scratch_bytes(int(roots.numel()), num_nodes, max_child)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        count, overflow, left = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        tries = [int(levels)] if depth_hint is None or depth_hint >= levels else [int(depth_hint), int(levels)]
        with torch.cuda.device(device):
            for lv in tries:
                _lib.check(L.lograst_lod_traverse(P, num_nodes, max_child, _ptr(ni), _ptr(tr), _ptr(x), _ptr(s), _ptr(r),
                                                  _ptr(roots), int(roots.numel()), _ptr(pm), _ptr(vm), float(fx),
                                                  float(fy), float(tanfovx), float(tanfovy), float(min_resolution_pixel),
                                                  lv, _ptr(out), int(out.numel()), _ptr(scratch), nbytes,
                                                  _stream_ptr(device)))
                _lib.check(L.lograst_lod_read(_ptr(scratch), ctypes.byref(count), ctypes.byref(overflow),
                                              ctypes.byref(left), _stream_ptr(device)))
                if left.value == 0:
                    break
        if overflow.value:
            raise _lib.LograstError("lod_traverse: inconsistent tree buffers (a point is reachable more than once)")
        return out[:count.value]


    def id_histogram(self, point_id_pixel, n):
        """N4a (log_amd/counter.py): sorted distinct ids >= 0 of the per-pixel id map and their pixel counts."""
        device = point_id_pixel.device
        L = self.require(device)
        pid = point_id_pixel.detach().to(torch.int32).contiguous()
        npix = int(pid.numel())
        cap = max(1, min(n, npix))
        ids = torch.empty(cap, dtype=torch.int32, device=device)
        counts = torch.empty(cap, dtype=torch.int64, device=device)
        nbytes = L.lograst_id_histogram_scratch_bytes(n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        k = ctypes.c_uint32(0)
        with torch.cuda.device(device):
            _lib.check(L.lograst_id_histogram(n, _ptr(pid), npix, _ptr(ids), _ptr(counts), _ptr(scratch), nbytes,
                                              _stream_ptr(device)))
            _lib.check(L.lograst_id_histogram_read(_ptr(scratch), ctypes.byref(k), _stream_ptr(device)))
        return ids[:k.value], counts[:k.value]

    def counter_update(self, buffers, visible_index, grad, radii, point_weight, point_id, point_count):
        """N4b (log_amd/counter.py): Counter.update_by_output for one view; -> flag_vis (bool[nv])."""
        device = radii.device
        L = self.require(device)
        want = {"weights_max": torch.float32, "weights_sum": torch.float32, "grad_sum": torch.float32,
                "radii_max": torch.int16, "visible_count": torch.int16, "radii_max_max": torch.int32,
                "area_sum": torch.int32, "create_steps": torch.int32}
        for name, dt in want.items():
            b = buffers[name]
            if b.dtype != dt or b.device != device or not b.is_contiguous():
                raise ValueError(f"counter buffer {name}: expected a contiguous {dt} tensor on {device}")
        num_points = int(buffers["weights_max"].shape[0])
        vi = visible_index.detach().to(device=device, dtype=torch.int64).contiguous()
        nv = int(vi.numel())
        g = _dev_f32(grad, device)
        if g.shape != (nv, 3):
            raise ValueError("viewspace gradient must be [nv, 3]")
        r = radii.detach().to(torch.int32).contiguous()
        w = _dev_f32(point_weight, device).reshape(-1)
        if int(r.numel()) != nv or int(w.numel()) != nv:
            raise ValueError("radii and point_weight must have one entry per visible_index row")
        pid = point_id.detach().to(device=device, dtype=torch.int32).contiguous()
        pc = point_count.detach().to(device=device, dtype=torch.int64).contiguous()
        flag = torch.empty(nv, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            _lib.check(L.lograst_counter_update(
                nv, _ptr(vi), _ptr(g), _ptr(r), _ptr(w), int(pid.numel()), _ptr(pid), _ptr(pc), num_points,
                *[_ptr(buffers[name]) for name in want], _ptr(flag), _stream_ptr(device)))
        return flag.view(torch.bool)

    @staticmethod
    def _adam_key(slot, device, entry, rows, grad):
        """Fills one LograstAdamKey from entry = (model_param, exp_avg, exp_avg_sq, max_exp_avg_sq | None, step_size) and the
        addresses of the rows being stepped and of their gradient (None: the launch computes it); -> floats per row."""
        model_p, m1, m2, mmax, step_size = entry
        width = int(model_p[0].numel()) if model_p.shape[0] else 1
        for t in (model_p, m1, m2) + ((mmax,) if mmax is not None else ()):
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous() or t.shape != model_p.shape:
                raise ValueError("parameters and Adam moments must be contiguous fp32 tensors on the parameter's "
                                 "device (log_amd.sparse_optimizer.step moves host-resident moments there)")
        slot.model_param, slot.param, slot.grad = model_p.data_ptr(), rows, grad
        slot.exp_avg, slot.exp_avg_sq = m1.data_ptr(), m2.data_ptr()
        slot.max_exp_avg_sq = mmax.data_ptr() if mmax is not None else None
        slot.width, slot.step_size = width, float(step_size)
        return width

    def sparse_adam(self, index, flag_vis, entries, beta1, beta2, bias_correction2_sqrt, eps):
        """N4c (log_amd/sparse_optimizer.py).  entries: (model_param, param, grad, exp_avg, exp_avg_sq,
        max_exp_avg_sq | None, step_size) per key."""
        device = index.device
        L = self.require(device)
        idx = index.detach().to(torch.int64).contiguous()
        m = int(idx.numel())
        fv = flag_vis.detach().to(device=device).contiguous()
        fv = fv.view(torch.uint8) if fv.dtype == torch.bool else fv.to(torch.uint8)
        if int(fv.numel()) != m:
            raise ValueError("flag_vis and index must have the same length")
        keep = []
        with torch.cuda.device(device):
            for first in range(0, len(entries), 8):
                chunk = entries[first:first + 8]
                keys = (_lib.LograstAdamKey * len(chunk))()
                for slot, (model_p, param, grad, *moments) in zip(keys, chunk):
                    num_points = int(model_p.shape[0])
                    p, g = _dev_f32(param, device), _dev_f32(grad, device)
                    width = self._adam_key(slot, device, (model_p, *moments), p.data_ptr(), g.data_ptr())
                    if int(p.numel()) != m * width or int(g.numel()) != m * width:
                        raise ValueError("param / grad rows do not match index")
                    keep += [p, g]
                _lib.check(L.lograst_sparse_adam(m, num_points, _ptr(idx), _ptr(fv), len(chunk), keys, float(beta1),
                                                 float(beta2), float(bias_correction2_sqrt), float(eps),
                                                 _stream_ptr(device)))
        del keep


    def gather_activate(self, index, bufs, degree, campos):
        """Rows N2/N3 (log_amd/get_all.py): gather rows `index` of the model buffers, -> (raw dict, activated dict)."""
        device = bufs["xyz"].device
        L = self.require(device)
        idx = index.detach().to(device=device, dtype=torch.int64).contiguous()
        n, P = int(idx.numel()), int(bufs["xyz"].shape[0])
        src = {k: _dev_f32(v, device) for k, v in bufs.items()}
        K = int(src["shs"].shape[1]) if "shs" in src else 0
        raw, act = {}, {}
        for (kind, key), block in _carve_skewed(device, n, _gather_blocks(K)).items():   # one allocation for all outputs
            (raw if kind == "raw" else act)[key] = block
        cp = _dev_f32(campos, device).reshape(-1) if campos is not None else None
        with torch.cuda.device(device):
            _lib.check(L.lograst_gather_activate(
                n, P, _ptr(idx), _ptr(src["xyz"]), _ptr(src["scaling"]), _ptr(src["opacity"]), _ptr(src["rotation"]),
                _ptr(src["colors"]), _ptr(src.get("shs")), K, int(degree), _ptr(cp), _ptr(raw["xyz"]),
                _ptr(raw["scaling"]), _ptr(raw["opacity"]), _ptr(raw["rotation"]), _ptr(raw["colors"]),
                _ptr(raw.get("shs")), _ptr(act["scaling"]), _ptr(act["opacity"]), _ptr(act["rotation"]),
                _ptr(act["colors"]), _stream_ptr(device)))
        act["xyz"] = raw["xyz"]
        return raw, act

    def activate_backward_adam(self, raw, n, degree, campos, g_xyz, g_scaling, g_opacity, g_rotation, g_colors, index, radii,
                               entries, beta1, beta2, bias_correction2_sqrt, eps):
        """Activation backward + sparse Adam in one launch (lograst_activate_backward_adam; log_amd.get_all's fused step).
        entries: {key: (model_param, exp_avg, exp_avg_sq, max_exp_avg_sq | None, step_size)} for the keys that are optimised
        (of xyz / scaling / opacity / rotation / colors / shs)."""
        device = raw["xyz"].device
        L = self.require(device)
        K = int(raw["shs"].shape[1]) if "shs" in raw else 0
        ups = [_dev_f32(t, device) for t in (g_xyz, g_scaling, g_opacity, g_rotation, g_colors)]
        cp = _dev_f32(campos, device).reshape(-1) if campos is not None else None
        idx = index.detach().to(torch.int64).contiguous()
        rad = radii.detach().to(torch.int32).contiguous()
        if int(idx.numel()) < n or int(rad.numel()) < n:
            raise ValueError("index / radii are shorter than the rows that are parameters")
        keys = (_lib.LograstAdamKey * 6)()
        num_points = int(next(iter(entries.values()))[0].shape[0])
        for slot, key in zip(keys, ("xyz", "scaling", "opacity", "rotation", "colors", "shs")):
            if key not in entries:
                continue
            p = raw[key]
            width = self._adam_key(slot, device, entries[key], p.data_ptr(), None)
            if not p.is_contiguous() or int(p.numel()) < n * width:
                raise ValueError("gathered parameter rows do not match")
        with torch.cuda.device(device):
            _lib.check(L.lograst_activate_backward_adam(
                int(n), _ptr(raw["xyz"]), _ptr(raw["scaling"]), _ptr(raw["opacity"]), _ptr(raw["rotation"]), K, int(degree),
                _ptr(cp), _ptr(ups[0]), _ptr(ups[1]), _ptr(ups[2]), _ptr(ups[3]), _ptr(ups[4]), num_points, _ptr(idx),
                _ptr(rad), keys, float(beta1), float(beta2), float(bias_correction2_sqrt), float(eps), _stream_ptr(device)))
        del ups

    def activate_backward(self, raw, n, degree, campos, g_scaling, g_opacity, g_rotation, g_colors):
        """-> dict of dL/d(raw rows [0, n)) for scaling / opacity / rotation / colors (/ shs when degree > 0)."""
        device = raw["xyz"].device
        L = self.require(device)
        K = int(raw["shs"].shape[1]) if "shs" in raw else 0
        g = _carve_skewed(device, int(n), _activate_backward_blocks(K, degree))
        ups = [_dev_f32(t, device) for t in (g_scaling, g_opacity, g_rotation, g_colors)]
        cp = _dev_f32(campos, device).reshape(-1) if campos is not None else None
        with torch.cuda.device(device):
            _lib.check(L.lograst_activate_backward(
                int(n), _ptr(raw["xyz"]), _ptr(raw["scaling"]), _ptr(raw["opacity"]), _ptr(raw["rotation"]), K,
                int(degree), _ptr(cp), _ptr(ups[0]), _ptr(ups[1]), _ptr(ups[2]), _ptr(ups[3]), _ptr(g["scaling"]),
                _ptr(g["opacity"]), _ptr(g["rotation"]), _ptr(g["colors"]), _ptr(g.get("shs")), _stream_ptr(device)))
        del ups
        return g

    @staticmethod
    def _row_block(t, device, num_points, width, what):
        """A key's per-model-row block as the accumulate kernels address it: fp32 on ``device``, ``num_points`` rows whose
        ``width`` floats are contiguous, any row stride >= width -> (address, row stride in floats)."""
        if t.device != device or t.dtype != torch.float32:
            raise ValueError(f"{what}: fp32 on the rows' device is needed")
        if t.dim() < 2 or int(t.shape[0]) != num_points or math.prod(t.shape[1:]) != width:
            raise ValueError(f"{what}: {tuple(t.shape)} where {num_points} rows of {width} floats are needed")
        if num_points > 1 and t[0].numel() and not t[0].is_contiguous():
            raise ValueError(f"{what}: the floats of a row must be contiguous")
        stride = int(t.stride(0)) if num_points > 1 else width
        if stride < width:
            raise ValueError(f"{what}: rows overlap")
        return t.data_ptr(), stride

    def activate_backward_accumulate(self, raw, n, degree, campos, g_xyz, g_scaling, g_opacity, g_rotation, g_colors, index,
                                     radii, targets, seen):
        """One view's activation backward added by model row (lograst_activate_backward_accumulate; log_amd.multi_view).
        targets: {key: [P, ...] fp32 view, rows any stride apart} for the keys that are accumulated (of xyz / scaling /
        opacity / rotation / colors / shs); seen: int32[P].  log_amd.multi_view.accumulate checks the sizes."""
        device = raw["xyz"].device
        L = self.require(device)
        K = int(raw["shs"].shape[1]) if "shs" in raw else 0
        P = int(seen.numel())
        ups = [_dev_f32(t, device) for t in (g_xyz, g_scaling, g_opacity, g_rotation, g_colors)]
        cp = _dev_f32(campos, device).reshape(-1) if campos is not None else None
        idx = index.detach().to(torch.int64).contiguous()
        rad = radii.detach().to(torch.int32).contiguous()
        if int(idx.numel()) < n or int(rad.numel()) < n:
            raise ValueError("index / radii are shorter than the rows that are parameters")
        if seen.device != device or seen.dtype != torch.int32 or not seen.is_contiguous():
            raise ValueError("seen must be a contiguous int32 tensor on the rows' device")
        slots = (_lib.LograstAccTarget * 6)()
        for slot, key in zip(slots, ACCUMULATE_KEYS):
            if key in targets:
                slot.base, slot.row_stride_floats = self._row_block(targets[key], device, P, accumulate_width(key, K),
                                                                    f"target {key}")
        with torch.cuda.device(device):
            _lib.check(L.lograst_activate_backward_accumulate(
                int(n), _ptr(raw["xyz"]), _ptr(raw["scaling"]), _ptr(raw["opacity"]), _ptr(raw["rotation"]), K, int(degree),
                _ptr(cp), _ptr(ups[0]), _ptr(ups[1]), _ptr(ups[2]), _ptr(ups[3]), _ptr(ups[4]), P, _ptr(idx), _ptr(rad),
                slots, _ptr(seen), _stream_ptr(device)))
        del ups

    def accumulated_adam(self, seen, entries, beta1, beta2, bias_correction2_sqrt, eps, moved_out=None):
        """One Adam step over the rows with seen > 0 (lograst_accumulated_adam; log_amd.multi_view).  entries: {key:
        (model_param, accumulated gradient [P, ...] view, exp_avg, exp_avg_sq, max_exp_avg_sq | None, step_size)};
        moved_out: uint8[P] or None."""
        device = seen.device
        L = self.require(device)
        P = int(seen.numel())
        if seen.dtype != torch.int32 or not seen.is_contiguous():
            raise ValueError("seen must be a contiguous int32 tensor")
        if moved_out is not None and (moved_out.device != device or moved_out.dtype != torch.uint8
                                      or not moved_out.is_contiguous() or int(moved_out.numel()) != P):
            raise ValueError("moved_out must be a contiguous uint8 tensor with one entry per model row")
        keys = (_lib.LograstAdamKey * 6)()
        strides = (ctypes.c_int32 * 6)()
        for i, key in enumerate(ACCUMULATE_KEYS):
            if key not in entries:
                continue
            model_p, grad, *rest = entries[key]
            if int(model_p.shape[0]) != P:
                raise ValueError(f"{key}: {int(model_p.shape[0])} model rows, {P} counts in seen")
            width = self._adam_key(keys[i], device, (model_p, *rest), None, None)
            keys[i].grad, strides[i] = self._row_block(grad, device, P, width, f"accumulated gradient of {key}")
        with torch.cuda.device(device):
            _lib.check(L.lograst_accumulated_adam(P, _ptr(seen), keys, strides, float(beta1), float(beta2),
                                                  float(bias_correction2_sqrt), float(eps), _ptr(moved_out),
                                                  _stream_ptr(device)))


_backend = HipBackend()
_backward_view = threading.local()     # .cur: what the rasterizer backward running on this thread published (see backward())


def _publish_backward_view(radii, means3D):
    """Called by the rasterizer's backward node: `radii` of its forward and the address of the means3D rows it rendered,
    for the nodes further down the SAME backward pass.  The record is emptied when the pass ends (a callback of the
    autograd engine, which may run on another thread: it empties the record itself, not this thread's slot) -- a later
    backward that never reaches a rasterizer node finds nothing."""
    rec = {"radii": radii, "means_ptr": int(means3D.data_ptr())}
    _backward_view.cur = None
    if radii is None:
        return
    try:
        torch.autograd.Variable._execution_engine.queue_callback(rec.clear)
    except RuntimeError:      # not inside an engine-driven backward: nothing can end the record's life, so none is left
        return
    _backward_view.cur = rec


def take_backward_radii(means3D=None):
    """The `radii` output of the rasterizer forward whose backward node ran before the caller's in this backward pass on
    this thread -- handed out ONCE (the record is consumed) -- or None: no rasterizer backward with a gradient ran in this
    pass, somebody took the radii already, or (means3D given) that render's means3D rows are not the tensor `means3D`."""
    rec, _backward_view.cur = getattr(_backward_view, "cur", None), None
    if not rec:
        return None
    radii, ptr = rec.get("radii"), rec.get("means_ptr")
    rec.clear()
    if radii is None or (means3D is not None and int(means3D.data_ptr()) != ptr):
        return None
    return radii


# ---- multi-view gradient accumulation (new design; not part of the reference's API) ---------------
_grad_sink = None


class accumulate_grads_into:
    """Context manager.  While active, every rasterizer backward ADDS its gradients w.r.t. means3D / scales /
    rotations / opacities / colors_precomp (or, with an "shs" entry, the SH coefficients) straight into the given fp32 tensors (e.g. the views of a
    log_amd.dist.GradientBucket) instead of returning them to autograd: the reverse walk's atomics and the
    chain-rule kernel write into the step's running sums, so a multi-view step needs no per-view accumulate pass.
    means2D (per-view, consumed by LoG's Counter) is still returned normally.  Row-major form: ``{"rows": [N, 16]}`` -- one
    64-byte row of running sums per Gaussian (columns 0-2 means3D, 3-5 scales, 6-9 rotations, 10 opacity, 11-13 colour;
    include/lograst.h: LOGRAST_BWD_ACCUMULATE_ROWS), what log_amd.dist.GradientBucket(row_major=True).sink() hands out.
    Otherwise the sink tensors must be
    contiguous fp32 [N,3],[N,3],[N,4],[N,1] or [N],[N,3] on the inputs' device; inputs routed through the sink get
    no autograd gradient."""

    def __init__(self, sink):
        if "rows" in sink:   # row-major running sums (log_amd.dist.GradientBucket(row_major=True).sink())
            t = sink["rows"]
            if (t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != _lib.GRAD_ROW_FLOATS
                    or t.data_ptr() % 64):
                raise ValueError("gradient sink 'rows' must be a contiguous, 64-byte aligned float32 [N, 16] tensor")
            if "shs" in sink:
                raise ValueError("the row-major gradient sink has no native-SH form (pass colors_precomp)")
            self.sink = {"rows": t}
            return
        need = ("means3D", "scales", "rotations", "opacities") + (() if "shs" in sink else ("colors",))
        missing = [k for k in need if k not in sink]
        if missing:
            raise KeyError(f"gradient sink lacks {missing}")
        for k in need + (("shs",) if "shs" in sink else ()):
            t = sink[k]
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"gradient sink '{k}' must be a contiguous float32 tensor")
        self.sink = dict(sink)

    def __enter__(self):
        global _grad_sink
        self.prev, _grad_sink = _grad_sink, self.sink
        return self

    def __exit__(self, *exc):
        global _grad_sink
        _grad_sink = self.prev
        return False


def _leaf_grad_sink(leaves, device):
    """The inputs' own ``.grad`` tensors as a gradient sink, or None unless EVERY differentiable input qualifies: a leaf
    that requires grad, without tensor hooks, whose .grad already exists as a dense contiguous fp32 tensor of its shape on
    this device (then adding in place is exactly what autograd's AccumulateGrad would do with a returned gradient)."""
    if torch.is_grad_enabled() or device.type != "cuda":   # create_graph=True: leave everything to autograd
        return None
    out = {}
    for name, t in zip(("means3D", "colors", "opacities", "scales", "rotations"), leaves):
        if t is None or not t.requires_grad or not t.is_leaf or t._backward_hooks:
            return None
        if getattr(t, "_post_accumulate_grad_hooks", None):
            return None
        g = t.grad
        if (g is None or g.dtype != torch.float32 or g.device != device or g.layout != torch.strided or
                not g.is_contiguous() or g.shape != t.shape or g.requires_grad):
            return None
        out[name] = g
    return out


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, colors, shs, opacities, scales, rotations, rs, flavour, use_filter, cov3D=None,
                reuse=None, aux_colors=None, *camera):
        """reuse: the calling rasterizer object's _ReuseSlot while geometry reuse is on (set_geometry_reuse), else None.
        aux_colors: a second colour triple per Gaussian [N, 3], composited into one more output image (the last one) by the
        same walk and differentiated by the same reverse walk (HipBackend.forward_aux / backward_aux).
        camera: absent, or (rs.viewmatrix, rs.projmatrix) when one of them requires grad (GaussianRasterizer.forward passes
        them then, so that autograd sees them as inputs): the backward returns dL/dviewmatrix / dL/dprojmatrix for those that do
        (HipBackend.backward_camera).  The values the kernels read are rs's, as always.
        Behind them, only while abs-grad is on: the marker _ABS_GRAD -- the backward then takes HipBackend.backward_abs and
        leaves / adds to ``means2D.absgrad``."""
        ctx.abs_grad = bool(camera) and camera[-1] is _ABS_GRAD
        if ctx.abs_grad:
            camera = camera[:-1]
            _refuse_extra_with("abs", sink=_grad_sink is not None, cov3D=cov3D is not None, band=_tile_rows.get() != (0, 0),
                               aux=aux_colors is not None, camera=bool(camera))
            if not hasattr(_backend, "backward_abs"):
                raise _lib.LograstError("this backend has no backward_abs: abs_grad is not available")
            ctx.abs_target = means2D      # (the caller's object: the backward hangs .absgrad on it)
        ctx.camera = len(camera) == 2
        if ctx.camera:
            _refuse_extra_with("camera", sink=_grad_sink is not None, cov3D=cov3D is not None, band=_tile_rows.get() != (0, 0),
                               aux=aux_colors is not None)
            if not hasattr(_backend, "backward_camera"):
                raise _lib.LograstError("this backend has no backward_camera: camera gradients (viewmatrix / projmatrix with "
                                        "requires_grad) are not available")
            if any(t.numel() != 16 for t in camera):
                raise ValueError("viewmatrix/projmatrix must be 4x4 and bg must have 3 entries")
            ctx.camera_like = tuple((t.shape, t.device) for t in camera)   # (a matrix kept on the host gets its gradient there)
            if reuse is not None:   # never a recomposited forward, never remembered as one
                reuse.forget()
                reuse = None
        elif camera:
            raise TypeError("viewmatrix and projmatrix go together")
        m = means3D.detach().to(torch.float32).contiguous()
        ax = None
        if aux_colors is not None:
            _refuse_extra_with("aux", cov3D=cov3D is not None, band=_tile_rows.get() != (0, 0), sink=_grad_sink is not None)
            if not (hasattr(_backend, "forward_aux") and hasattr(_backend, "backward_aux")):
                raise _lib.LograstError("this backend has no forward_aux / backward_aux: aux_colors is not available")
            ax = aux_colors.detach().to(torch.float32).contiguous()
            if ax.shape != (m.shape[0], 3):
                raise ValueError("aux_colors must be [N, 3]")
        cov = None
        if cov3D is not None:   # the packages' cov3D_precomp input (not LoG's path): scales / rotations are absent
            cov = cov3D.detach().to(torch.float32).contiguous()
            if cov.shape != (m.shape[0], 6):
                raise ValueError("cov3D_precomp must be [N, 6]")
            if _grad_sink is not None:
                raise ValueError("accumulate_grads_into has no entry for cov3D_precomp")
            s, r = m.new_empty(0, 3), m.new_empty(0, 4)    # placeholders for save_for_backward: never read
        else:
            s = scales.detach().to(torch.float32).contiguous()
            r = rotations.detach().to(torch.float32).contiguous()
        o = opacities.detach().to(torch.float32).contiguous().reshape(-1)
        n = m.shape[0]
        sh = clamped = None
        if shs is not None:   # the packages' native SH input (not LoG's path)
            sh = shs.detach().to(torch.float32).contiguous()
            if sh.dim() != 3 or sh.shape[0] != n or sh.shape[2] != 3 or sh.shape[1] < (int(rs.sh_degree) + 1) ** 2:
                raise ValueError("shs must be [N, >=(sh_degree+1)^2, 3]")
            c, clamped = _backend.sh_forward(m, rs.campos, sh, int(rs.sh_degree))
        else:
            c = colors.detach().to(torch.float32).contiguous()
        if not ((cov is not None or (s.shape == (n, 3) and r.shape == (n, 4))) and c.shape == (n, 3) and o.shape[0] == n
                and m.shape == (n, 3)):
            raise ValueError("rasterizer inputs must be means3D[N,3], scales[N,3], rotations[N,4], "
                             "colors_precomp[N,3], opacities[N,1]")
        wants_grad = any(ctx.needs_input_grad[:7])   # all False under torch.no_grad()
        wants_grad = wants_grad or (cov is not None and ctx.needs_input_grad[10]) or (ax is not None and ctx.needs_input_grad[12])
        wants_grad = wants_grad or (ctx.camera and any(ctx.needs_input_grad[13:15]))
        scratch_floats = _lib.BWD_ROW_FLOATS if wants_grad else 0
        first = None
        aux_image = None
        if reuse is not None and ax is None:   # the same Gaussians as this object's last forward: composite its lists again
            first, why = reuse.match(_backend, rs, flavour, use_filter, m.device, (m, s, r, o), cov)
            _count_reuse(why)
        if ax is not None:      # one walk for both images; never remembered as a reusable forward
            if reuse is not None:
                reuse.forget()
                _count_reuse("aux")
            image, radii, pid, pwp, pw, aux_image, saved = _backend.forward_aux(rs, flavour, use_filter, m, s, r, o, c, ax,
                                                                                scratch_floats=scratch_floats)
        elif first is not None:
            image, radii, pid, pwp, pw, saved = _backend.recomposite(rs, flavour, use_filter, first, c,
                                                                     scratch_floats=scratch_floats)
        else:
            image, radii, pid, pwp, pw, saved = _backend.forward(rs, flavour, use_filter, m, *((s, r) if cov is None else (None, None)),
                                                                 o, c, scratch_floats=scratch_floats, cov3D=cov)
            if reuse is not None:
                if cov is None and n > 0:
                    reuse.remember(_backend, rs, flavour, use_filter, m.device, (m, s, r, o), saved, radii)
                else:
                    reuse.forget()
        ctx.cov = cov
        ctx.rs, ctx.flavour, ctx.use_filter = rs, flavour, use_filter
        ctx.set_materialize_grads(False)   # no zero-filled gradients for radii / the fork maps (4 fill kernels per view)
        ctx.saved = saved   # the backend's own record: opaque here
        # the backward trusts the forward's point_weight (which Gaussians it may skip, which dL/dconic rows are cleared):
        # an in-place change of that output between forward and backward is refused, like autograd does for saved tensors
        ctx.radii, ctx.pw, ctx.pw_version = radii, pw, pw._version if pw is not None else None
        ctx.leaves = ((means3D, colors, opacities, scales, rotations)
                      if (sh is None and cov is None and ax is None and not ctx.camera and not ctx.abs_grad) else None)
        ctx.sh = (sh, clamped)
        ctx.aux = ax is not None
        # the reverse walk reads aux_colors again (the RGB colours sit in the records, a copy): an in-place change of the
        # caller's tensor between forward and backward is refused, as autograd refuses it for saved tensors
        ctx.aux_colors, ctx.aux_version = ax, ax._version if ax is not None else None
        ctx.shapes = (means2D.shape, opacities.shape)
        ctx.save_for_backward(m, s, r)
        tail = (aux_image,) if ax is not None else ()
        if flavour.extras:
            ctx.mark_non_differentiable(radii, pid, pwp, pw)
            return (image, radii, pid, pwp, pw) + tail
        ctx.mark_non_differentiable(radii)
        return (image, radii) + tail

    @staticmethod
    def backward(ctx, grad_image, *unused):
        m, s, r = ctx.saved_tensors
        grad_aux = unused[-1] if ctx.aux else None   # (the aux image is the last output)
        if grad_image is None and grad_aux is None:   # no gradient reached an image: nothing flows on, and no visibility is published
            _backward_view.cur = None
            return (None,) * ((15 if ctx.camera else 13) + (1 if ctx.abs_grad else 0))
        # which view's backward is running: nodes further down the same graph (log_amd.get_all's fused step) take the
        # visibility of THIS render from here (the rasterizer's node runs before the nodes that produced its inputs)
        _publish_backward_view(ctx.radii, m)
        m2_shape, o_shape = ctx.shapes
        sh, clamped = ctx.sh
        if ctx.pw is not None and ctx.pw._version != ctx.pw_version:
            raise RuntimeError("the rasterizer's point_weight output was modified in place between forward and backward; "
                               "the backward uses it to skip Gaussians that contributed to no pixel -- clone it first")
        if ctx.aux and ctx.aux_colors._version != ctx.aux_version:
            raise RuntimeError("the rasterizer's aux_colors input was modified in place between forward and backward; the "
                               "backward composites it again -- clone it first")
        # where the gradients go: back to autograd (sink None), or added into running sums -- one row per Gaussian, or one
        # tensor per input (with native SH: the colour gradient into a scratch, from there into the running dL/dshs)
        n = m.shape[0]
        sink = _grad_sink if ctx.cov is None else None
        for extra, on in (("camera", ctx.camera), ("aux", ctx.aux), ("abs", ctx.abs_grad)):
            if on:
                _refuse_extra_with(extra, sink=sink is not None)
        if sink is None and ctx.leaves is not None and (   # (leaves: None under cov3D_precomp or native SH)
                _inplace_leaf_grads or all(getattr(t, _INPLACE_TAG, False) for t in ctx.leaves if t is not None)):
            sink = _leaf_grad_sink(ctx.leaves, m.device)
        if sink is not None and "rows" in sink:
            if sh is not None:
                raise ValueError("the row-major gradient sink has no native-SH form (pass colors_precomp)")
            if sink["rows"].shape[0] != n or sink["rows"].device != m.device:
                raise ValueError("gradient sink does not match the rasterizer inputs")
        elif sink is not None and (sh is None or "shs" in sink):
            if not (sink["means3D"].shape == (n, 3) and sink["scales"].shape == (n, 3) and
                    sink["rotations"].shape == (n, 4) and sink["opacities"].numel() == n and
                    (sh is not None or sink["colors"].shape == (n, 3)) and sink["means3D"].device == m.device):
                raise ValueError("gradient sink does not match the rasterizer inputs")
            if sh is not None:
                # colours are an intermediate here: their gradient goes to a zeroed scratch, then through the SH
                # polynomial into the running dL/dshs (and the direction term into the running dL/dmeans3D)
                if sink["shs"].shape != sh.shape or not sink["shs"].is_contiguous():
                    raise ValueError("gradient sink 'shs' must be a contiguous tensor shaped like shs")
                sink = dict(sink, colors=torch.zeros(n, 3, dtype=torch.float32, device=m.device))
        else:
            sink = None   # (a sink without an "shs" entry under native SH: the gradients go back to autograd)
        # One call: the backend method of the extra this forward came with (camera: the chain-rule launch sums the camera
        # terms too; abs-grad: the plain gradients and the absolute sums; aux: both images through one reverse walk and one
        # chain rule, means2D gets the one summed gradient), else backward() -- the six gradients, then the extra's own.
        base = (ctx.rs, ctx.flavour, ctx.use_filter, m, *((s, r) if ctx.cov is None else (None, None)), ctx.saved, grad_image)
        if ctx.camera:
            out = _backend.backward_camera(*base)
        elif ctx.abs_grad:
            out = _backend.backward_abs(*base)
        elif ctx.aux:
            out = _backend.backward_aux(*base, grad_aux)
        else:
            out = _backend.backward(*base, sink=sink, cov3D=ctx.cov)
        (g_m3, g_m2, g_c, g_o, g_s, g_r), more = out[:6], out[6:]
        g_aux = more[0] if ctx.aux else None
        g_cam = ()
        if ctx.camera:   # a matrix that does not require grad gets None
            g_cam = tuple(g.reshape(shape).to(dev) if need else None
                          for g, need, (shape, dev) in zip(more, ctx.needs_input_grad[13:15], ctx.camera_like))
        elif ctx.abs_grad:   # the absolute sums go onto the caller's means2D
            target, g_abs = ctx.abs_target, more[0].reshape(m2_shape).to(ctx.abs_target.device)
            with torch.no_grad():
                old = getattr(target, "absgrad", None)
                if old is None:
                    target.absgrad = g_abs
                else:
                    old.add_(g_abs)
            g_cam = (None,)               # (the marker's slot)
        g_sh = g_cov = None
        if ctx.cov is not None:   # (the backend's last two results are then (dL/dcov3D, None))
            g_cov, g_s = g_s, None
        if sh is not None and sink is None:
            g_sh = _backend.sh_backward(m, ctx.rs.campos, sh, int(ctx.rs.sh_degree), clamped, g_c.contiguous(), g_m3)
            g_c = None
        elif sh is not None:
            _backend.sh_backward(m, ctx.rs.campos, sh, int(ctx.rs.sh_degree), clamped, sink["colors"], sink["means3D"],
                                 into=sink["shs"])
        return (g_m3, g_m2.reshape(m2_shape), g_c, g_sh, g_o.reshape(o_shape) if g_o is not None else None, g_s, g_r,
                None, None, None, g_cov, None, g_aux) + g_cam


class GaussianRasterizer(nn.Module):
    FLAVOUR = WODILATE

    def __init__(self, raster_settings, walk_form=None, abs_grad=None):
        """walk_form (extension; the third-party packages take raster_settings only): pin the compositing kernels' form
        for this object's calls -- 'rows' / 'quadrant' / None (decided per call); see ``log_amd.rasterizer.walk_form``.
        abs_grad (extension): True / False switches abs-grad on / off for this object's calls, None (default) leaves it to
        ``set_abs_grad`` / ``with abs_grad(...)``; see ``log_amd.rasterizer.set_abs_grad``."""
        super().__init__()
        self.raster_settings = raster_settings
        self.walk_form = walk_form
        self.abs_grad = None if abs_grad is None else bool(abs_grad)
        _form_code(walk_form)

    def markVisible(self, positions):
        """Frustum test of the third-party package (not called by LoG): view z > 0.2."""
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix.to(positions.device, torch.float32)
            z = positions.to(torch.float32) @ vm[:3, 2] + vm[3, 2]
            return z > 0.2

    def compute_radius(self, xyz, scaling, rotation):
        """Fork-only method (level_of_gaussian.py:59): projected radius per point, 0 = not visible."""
        rs = self.raster_settings
        fx = rs.image_width / (2.0 * rs.tanfovx)
        fy = rs.image_height / (2.0 * rs.tanfovy)
        with torch.no_grad():
            return _backend.compute_radius(xyz, scaling * rs.scale_modifier, rotation, rs.projmatrix, rs.viewmatrix,
                                           fx, fy, rs.tanfovx, rs.tanfovy)

    def tile_rows(self, xyz, scaling, rotation, use_filter=True):
        """New (image split across GPUs): (y0, y1) int32[N], the tile rows [y0, y1) of each Gaussian's rect on
        the whole image under this rasterizer's settings, (0, 0) when the forward would drop it.  The Gaussians a forward
        inside ``tile_rows(b, e)`` keeps are exactly those with y0 < e and y1 > b (log_amd.dist.band_index)."""
        with torch.no_grad():
            return _backend.tile_rows(self.raster_settings, self.FLAVOUR, use_filter, xyz, scaling, rotation)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, aux_colors=None, **kwargs):
        """aux_colors (extension; the third-party packages have no such argument): a second colour triple per Gaussian,
        [N, 3].  The call then returns its usual tuple plus ``aux_image`` [3, H, W] as the last element: the image a second
        call with ``colors_precomp=aux_colors`` would return, bit for bit, from the same compositing walk; one autograd node
        whose backward takes either or both image gradients.  Not with cov3D_precomp, a ``tile_rows`` band or
        ``accumulate_grads_into``.

        Camera gradients (extension): when ``raster_settings.viewmatrix`` or ``.projmatrix`` requires grad, the backward
        fills its ``.grad`` (or hands the gradient on, if it is no leaf): a fresh fp32 [4, 4], zeros when nothing is visible.
        Column 3 of dL/dviewmatrix and column 2 of dL/dprojmatrix are exactly zero.  Not with cov3D_precomp, a ``tile_rows``
        band, ``accumulate_grads_into`` or ``aux_colors``.  ``raster_settings.campos`` gets no gradient (it matters only
        under native ``shs=``)."""
        flavour = self.FLAVOUR
        use_filter = True
        if "use_filter" in kwargs:
            if not flavour.extras:
                raise TypeError("forward() got an unexpected keyword argument 'use_filter'")
            use_filter = bool(kwargs.pop("use_filter"))
        if kwargs:
            raise TypeError(f"forward() got unexpected keyword arguments {sorted(kwargs)}")
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        if shs is not None and not 0 <= int(self.raster_settings.sh_degree) <= 3:
            raise ValueError("sh_degree must be 0..3")
        # (a rasterizer without a form of its own leaves an enclosing ``with walk_form(...)`` block in force)
        slot = None
        if _geometry_reuse:   # (opt-in: set_geometry_reuse) this object remembers its last full forward
            slot = self.__dict__.get("_reuse_slot")
            if slot is None:
                slot = self.__dict__["_reuse_slot"] = _ReuseSlot()
        elif "_reuse_slot" in self.__dict__:
            del self.__dict__["_reuse_slot"]    # switched off: nothing stays pinned
        with walk_form(self.walk_form) if self.walk_form not in (None, "auto") else contextlib.nullcontext():
            rs = self.raster_settings
            camera = tuple(t for t in (rs.viewmatrix, rs.projmatrix) if torch.is_tensor(t) and t.requires_grad)
            if camera and torch.is_grad_enabled():
                camera = (rs.viewmatrix, rs.projmatrix)
            else:
                camera = ()
            if (_abs_grad_on() if self.abs_grad is None else self.abs_grad) and torch.is_grad_enabled():
                camera = camera + (_ABS_GRAD,)   # (off: the call below is the parent's, argument for argument)
            ret = _RasterizeGaussians.apply(means3D, means2D, colors_precomp, shs, opacities, scales, rotations,
                                            rs, flavour, use_filter, cov3D_precomp, slot, aux_colors, *camera)
        if flavour.extras:
            # how many Gaussians the ids of point_id_pixel index: lets log_amd.counter's stand-in for the
            # torch.unique call at LoG/render/renderer.py:156 recognise the map and take the histogram kernel
            ret[2]._lograst_num_gaussians = int(means3D.shape[0])
        return ret


class UpstreamGaussianRasterizer(GaussianRasterizer):
    FLAVOUR = UPSTREAM


def keep_keys(enabled):
    """Test/debug switch: forwards keep their (depth, id) key buffer in `saved` (16 bytes per tile instance, otherwise
    released when the forward returns) so that finish_lists can order the lists' tails.  Returns the previous setting."""
    global _keep_keys
    prev, _keep_keys = _keep_keys, bool(enabled)
    return prev


def ordered_lengths_of(saved, width, height):
    """Test/debug accessor: per tile, how many leading positions of its list are in final order (lists of more than
    4096 keys are ordered over their first window only unless a pixel needed more: include/lograst.h,
    lograst_ordered_lengths)."""
    tiles = _tiles(width, height)
    st = saved["state"]
    out = torch.empty(tiles, dtype=torch.int32, device=st.device)
    with torch.cuda.device(st.device):
        _lib.check(_lib.lib().lograst_ordered_lengths(_ptr(st), int(width), int(height), _ptr(out), _stream_ptr(st.device)))
    return out


def parked_waves_of(saved, width, height):
    """Test/debug accessor (synchronises): (open[tiles] int32, header word LR_HDR_OPEN) of a forward's tile state -- per
    tile one bit for each of its four compositing waves that ran out of ordered entries with a pixel still open and parked
    for the second sort / compositing pair, and the view's "somebody parked" flag (layout: log_amd/csrc/common.hpp,
    sorted[] / open[]).  Only lists of more than 4096 keys of a view whose sort left lists at their first window have such a
    word (elsewhere the array still holds the fill's cursors): every other tile reads as 0."""
    tiles = _tiles(width, height)
    st = saved["state"]
    offs = tile_offsets_of(saved, width, height)
    first = (offs.data_ptr() - st.data_ptr()) // 4
    sorted_off = first + ((tiles + 1 + 15) & ~15)                       # lr_sorted_off = lr_offsets_off + lr_tpad
    hdr = st[:16].cpu()
    lazy, hdr_open = int(hdr[9]), int(hdr[10])                          # LR_HDR_LAZY, LR_HDR_OPEN
    lens = (offs[1:].to(torch.int64) & 0xffffffff) - (offs[:-1].to(torch.int64) & 0xffffffff)
    words = st[sorted_off + tiles:sorted_off + 2 * tiles]
    streamed = (lens > 4096) if lazy else torch.zeros_like(lens, dtype=torch.bool)
    return torch.where(streamed, words, torch.zeros_like(words)), hdr_open


def finish_lists(saved, width, height):
    """Test/debug: orders every tile list of a forward made under keep_keys(True) to its end, in place
    (lograst_finish_lists): saved["plist"] is then what LOGRAST_LAZY_SORT=0 would have produced."""
    st = saved["state"]
    if saved["keys"] is None:
        raise RuntimeError("finish_lists: this forward did not keep its key buffer -- run it under keep_keys(True) "
                           "(the forward treats `keys` as dead scratch otherwise)")
    with torch.cuda.device(st.device):
        _lib.check(_lib.lib().lograst_finish_lists(_ptr(st), int(width), int(height), _ptr(saved["keys"]), _ptr(saved["plist"]),
                                                  int(saved["capacity"]), _stream_ptr(st.device)))


def tile_offsets_of(saved, width, height):
    """Test/debug accessor: the per-tile exclusive offsets (tiles+1 entries) inside a tile_state tensor
    (layout: log_amd/csrc/common.hpp)."""
    tiles = _tiles(width, height)
    st = saved["state"]
    L = _lib.lib()
    first = (L.lograst_tile_offsets(ctypes.c_void_p(st.data_ptr()), int(width), int(height)) - st.data_ptr()) // 4
    return st[first:first + tiles + 1]

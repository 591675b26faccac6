"""Poisoned allocations: what a kernel finds in a buffer nobody wrote must not reach a result.

Every device buffer the library works in comes from ``torch.empty`` in the Python layer (log_amd/*.py; there is no hipMalloc in
log_amd/csrc), most of them through ``log_amd.rasterizer.HipBackend._carve``.  In a test process the caching allocator hands
back the block the previous, nearly identical call released, so a kernel that forgets a clear usually finds the value it needed.
``poisoned(fill)`` takes that luck away: while it is active every ``torch.empty`` that returns a tensor on one of `devices` is
filled before it is handed out, on the current stream, by dtype:

    fill      floating dtypes   integer / bool dtypes   uint8 (untyped bytes)
    zero      +0.0              0                       32-bit words of 0
    nan       quiet NaN         1                       words of 1
    huge      +1e30             1                       words of 1
    -huge     -1e30             1                       words of 1

Integers stay 0 or 1 on purpose: a latent read of a stale index must land inside its buffer and show as a differing result,
never as a fault.  ``ints=0`` (a scenario with fewer than two rows, pixels or entries: 1 is no valid index there) fills integers
and bytes with 0 under every fill.  The named parts of a ``_carve`` arena are filled by their OWN dtype (final_T, bwd_scratch and
the gradient arrays are floats inside a uint8 allocation: they would otherwise never see a NaN).  Every hooked allocation is
recorded in the context's census (dtype, bytes, _carve part name).  Everything is restored on exit, exceptions included; an inner
context takes over from an outer one and hands back to it.  Not for use around graph capture or multi-process code.

    with poisoned("nan") as census:
        out = call()
    assert census.parts() >= {"geom", "state"}
"""
import contextlib
import functools
import math

import torch

FILLS = ("zero", "nan", "huge", "-huge")
_FLOAT_VALUE = {"zero": 0.0, "nan": float("nan"), "huge": 1e30, "-huge": -1e30}
ARENA = "(arena)"          # the census name of a _carve allocation as a whole (its named parts follow it)


def float_value(fill):
    return _FLOAT_VALUE[fill]


def int_value(fill, ints=None):
    if fill not in _FLOAT_VALUE:
        raise ValueError("fill must be one of %r (got %r)" % (FILLS, fill))
    return (0 if fill == "zero" else 1) if ints is None else int(ints)


def fill_(t, fill, ints=None):
    """Fill tensor t (any shape; as torch.empty returns it: dense) in place by the table above; -> t."""
    if t.numel() == 0:
        int_value(fill, ints)
        return t
    if t.is_floating_point() or t.is_complex():
        x = float_value(fill)
        if t.is_floating_point() and abs(x) > torch.finfo(t.dtype).max:       # (1e30 in half precision: the infinity of its sign)
            x = math.copysign(math.inf, x)
        return t.fill_(x)
    v = int_value(fill, ints)
    if t.dtype != torch.uint8:
        return t.fill_(bool(v) if t.dtype == torch.bool else v)
    # untyped bytes: little-endian 32-bit words of v from the tensor's first byte; a tail of 1..3 bytes = the first bytes of one more
    t.fill_(0)
    if v:
        t.view(-1)[0::4] = v          # (dense, as torch.empty and _carve hand buffers out)
    return t


class Census:
    """The hooked allocations of one poisoned() block, in order: dicts(dtype, bytes, part).  part: None = a plain torch.empty;
    ARENA = a _carve allocation as a whole; a name = one part of the arena before it (its bytes are inside the arena's)."""

    def __init__(self, fill, ints):
        self.fill, self.ints, self.entries = fill, ints, []

    def record(self, t, part=None):
        self.entries.append(dict(dtype=str(t.dtype).replace("torch.", ""), bytes=int(t.numel() * t.element_size()), part=part))

    def __len__(self):
        return len(self.entries)

    def allocations(self):
        """The entries that are allocations of their own (plain ones and whole arenas)."""
        return [e for e in self.entries if e["part"] is None or e["part"] == ARENA]

    def bytes(self):
        return sum(e["bytes"] for e in self.allocations())

    def parts(self):
        """The names of the _carve parts that were handed out."""
        return {e["part"] for e in self.entries if e["part"] not in (None, ARENA)}

    def part_dtypes(self):
        return {e["part"]: e["dtype"] for e in self.entries if e["part"] not in (None, ARENA)}

    def summary(self):
        """'<allocations> buffers, <bytes> B (parts: a, b, ...)' for the record."""
        return "%d buffers, %d B%s" % (len(self.allocations()), self.bytes(),
                                        (" (parts: %s)" % ", ".join(sorted(self.parts()))) if self.parts() else "")


_active = []      # the stack of (census, devices) of the poisoned() blocks in force; the last one gets the allocations


def _hooked(device_type):
    return bool(_active) and device_type in _active[-1][1]


def _wrap_empty(orig):
    @functools.wraps(orig)
    def empty(*args, **kwargs):
        t = orig(*args, **kwargs)
        if isinstance(t, torch.Tensor) and _hooked(t.device.type):
            census = _active[-1][0]
            fill_(t, census.fill, census.ints)
            census.record(t, ARENA if _in_carve[0] else None)
        return t
    empty._poison_orig = orig
    return empty


_in_carve = [0]


def _wrap_carve(orig):
    @functools.wraps(orig)
    def _carve(device, parts):
        _in_carve[0] += 1
        try:
            out = orig(device, parts)       # (its torch.empty is hooked: the arena, padding included, is filled as bytes first)
        finally:
            _in_carve[0] -= 1
        if _hooked(torch.device(device).type):
            census = _active[-1][0]
            for name, _, _ in parts:
                fill_(out[name], census.fill, census.ints)
                census.record(out[name], name)
        return out
    _carve._poison_orig = orig
    return _carve


@contextlib.contextmanager
def poisoned(fill, ints=None, devices=("cuda",)):
    """-> the block's Census.  fill: one of FILLS; ints: None = the table, 0 = integers and bytes are 0 under every fill;
    devices: the device types whose tensors are filled (the CPU tests of the harness itself pass ("cpu",))."""
    int_value(fill, ints)
    from log_amd import rasterizer as R
    census = Census(fill, ints)
    prev_empty = torch.empty
    prev_carve = R.HipBackend.__dict__["_carve"]                 # the staticmethod object (or an outer block's)
    plain_carve = prev_carve.__func__ if isinstance(prev_carve, staticmethod) else prev_carve
    torch.empty = _wrap_empty(getattr(prev_empty, "_poison_orig", prev_empty))
    R.HipBackend._carve = staticmethod(_wrap_carve(getattr(plain_carve, "_poison_orig", plain_carve)))
    _active.append((census, tuple(devices)))
    try:
        yield census
    finally:
        _active.pop()
        torch.empty = prev_empty
        R.HipBackend._carve = prev_carve


def run_fills(call, fills=FILLS, ints=None, devices=("cuda",), sync=None, parts=()):
    """call() once unpoisoned and once under each fill -> ({None: result, fill: result, ...}, {fill: Census}).  sync: called
    inside every block after call() (torch.cuda.synchronize for device work).  Every poisoned call must have made hooked
    allocations (else the harness does not reach it and the comparison says nothing), the carved `parts` among them."""
    results, census = {None: call()}, {}
    if sync is not None:
        sync()
    for f in fills:
        with poisoned(f, ints=ints, devices=devices) as c:
            results[f] = call()
            if sync is not None:
                sync()
        assert len(c) > 0, "no hooked allocation under fill %r: the harness does not reach this call" % (f,)
        assert set(parts) <= c.parts(), (f, sorted(set(parts) - c.parts()))
        census[f] = c
    return results, census


# ---- what a call into the library's Python layer handed back -----------------------------------------------------------------

def snapshot(x, depth=3):
    """The tensors inside x as host arrays, structure kept: tensors, numbers, dicts / sequences of them, and the attributes of
    plain objects (a plan, a record) down to `depth`; anything else -> None."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().copy()
    if isinstance(x, (bool, int, float)) or x is None:
        return x
    if depth == 0:
        return None
    if isinstance(x, dict):
        return {str(k): snapshot(v, depth - 1) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [snapshot(v, depth - 1) for v in x]
    d = getattr(x, "__dict__", None)
    if isinstance(d, dict) and not isinstance(x, (type, torch.nn.Module)) and not callable(x):
        return {k: snapshot(v, depth - 1) for k, v in sorted(d.items()) if not k.startswith("__")}
    return None


@contextlib.contextmanager
def spied(*targets):
    """Record every call into `targets` -- modules (their public functions and the public methods of the classes they define)
    or classes -- while the block is active: -> the log, a list of [qualified name, snapshot of the return value, snapshot of the
    positional and keyword arguments AFTER the call (what a call wrote in place)].  Only the outermost spied call of a nest is
    logged.  Everything is restored on exit."""
    import inspect
    import types
    log, depth, undo = [], [0], []

    def wrap(owner, name, fn, qual):
        @functools.wraps(fn)
        def spy(*a, **k):
            depth[0] += 1
            try:
                out = fn(*a, **k)
            finally:
                depth[0] -= 1
            if depth[0] == 0:
                log.append([qual, snapshot(out), snapshot([list(a), k])])
            return out
        undo.append((owner, name, owner.__dict__[name]))
        setattr(owner, name, spy)

    def wrap_class(cls):
        for name, attr in list(cls.__dict__.items()):
            if not name.startswith("_") and isinstance(attr, types.FunctionType):
                wrap(cls, name, attr, "%s.%s" % (cls.__name__, name))

    for t in targets:
        if inspect.isclass(t):
            wrap_class(t)
            continue
        for name, attr in list(vars(t).items()):
            if name.startswith("_") and not name.startswith(("_pack", "_unpack")):
                continue
            if isinstance(attr, types.FunctionType) and attr.__module__ == t.__name__:
                wrap(t, name, attr, "%s.%s" % (t.__name__, name))
            elif inspect.isclass(attr) and attr.__module__ == t.__name__:
                wrap_class(attr)
    try:
        yield log
    finally:
        for owner, name, orig in reversed(undo):
            setattr(owner, name, orig)


def differing(results):
    """The fills whose result is not bit-identical to the unpoisoned one.  Results: tensors / numpy arrays / numbers, or
    dicts / sequences of them."""
    return [f for f in results if f is not None and not same_bits(results[None], results[f])]


def same_bits(a, b):
    import numpy as np
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    if isinstance(b, torch.Tensor):
        b = b.detach().cpu().numpy()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()

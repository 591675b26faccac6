"""Stage benchmark of densification on the device (log_amd.densify.split_and_remove: plan + fused row moves + the uniform
split kernel) at the sizes a user runs, three ways on the same state and flags:

1. ``dropin``: log_amd.densify.split_and_remove on a GaussianPoint-shaped model with both Adam moments;
2. ``torch_device``: the same result from torch ops ON THE DEVICE, written here: per key a boolean index, a repeat and a
   cat (moments: an index and a cat with zeros), the children's xyz / scaling from the uniform split in torch;
3. ``host_round_trip``: the shape of the reference's method (LoG/model/splitter.py:148-197), written here: every key and
   every moment to the CPU, boolean index + cat there, back to the device; the uniform split itself runs on the device,
   as the reference's does, and its result is copied (timed once per configuration).

    python tools/bench_densify.py [--sizes 10000000,30000000] [--degrees 1,3] [--reps 3] [--children 4]
        -> one JSON line per configuration

Times are wall times around the call with a synchronize on both sides (ways 1 and 2 alternate, after one warm-up round
each); the state is drawn again before every call, outside the timed region.  ``row_move``: HIP events around the
lograst_densify_move_rows launches alone, all keys and moments of the configuration on a prepared plan; its bytes are the
payload read plus written (a zeroed row is only written), and ``share_of_copy`` is that rate over the rate of
lograst_stream_copy (its best form, 1 GiB) in the same run."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from log_amd import _lib, densify  # noqa: E402
from log_amd import rasterizer as R  # noqa: E402

dev = torch.device("cuda:0")
KEYS = ("scaling", "colors", "xyz", "opacity", "rotation", "shs")


def widths(degree):
    w = {"scaling": (3,), "colors": (3,), "xyz": (3,), "opacity": (1,), "rotation": (4,), "shs": ((degree + 1) ** 2 - 1, 3)}
    if degree == 0:
        del w["shs"]
    return w


def make_state(n, degree, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    w = widths(degree)
    model = types.SimpleNamespace(keys=[k for k in KEYS if k in w], activation=types.SimpleNamespace(
        scaling_activation=torch.exp, scaling_inverse_activation=torch.log,
        rotation_activation=torch.nn.functional.normalize))
    for k in model.keys:
        setattr(model, k, torch.randn((n,) + w[k], device=dev, generator=g))
    model.scaling.mul_(0.5).sub_(4.0)
    opt = types.SimpleNamespace(state_keys=["exp_avg", "exp_avg_sq"])
    for sk in opt.state_keys:
        d = {k: torch.randn((n,) + w[k], device=dev, generator=g) for k in model.keys}
        setattr(opt, sk, types.SimpleNamespace(keys=list(d), items=lambda d=d: d.items(), device=dev, tensors=d))
    return model, opt


def make_flags(n, seed, split=0.05, remove=0.02):
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(n, device=dev, generator=g)
    return u < split, (u >= split) & (u < split + remove)


def dropin(model, opt, fs, fr, children):
    splitter = types.SimpleNamespace(N=children, split_method="uniform", scaling_factor=0.7)
    return densify.split_and_remove(splitter, model, opt, fs, fr, remove_split=True)


def split_uniform_torch(xyz, raw, rot, children):
    """splitter.py:5-31, :95-130 with torch ops on whatever device the inputs live on."""
    q = rot / rot.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    scale, centre = torch.exp(raw), xyz
    m = 1
    while m < children:
        axis = scale.max(dim=-1).indices
        rows = torch.arange(scale.shape[0], device=scale.device)
        step = Rm[rows, :, axis] * (0.5 * scale[rows, axis])[:, None]
        centre = torch.stack([centre - step, centre + step], dim=1).reshape(-1, 3)
        scale = scale.clone()
        scale[rows, axis] *= 0.5
        scale = scale[:, None].repeat(1, 2, 1).reshape(-1, 3)
        Rm = Rm[:, None].repeat(1, 2, 1, 1).reshape(-1, 3, 3)
        m *= 2
    return centre, torch.log(scale)


def by_torch(model, opt, fs, fr, children, where):
    """Ways 2 (where = the device) and 3 (where = the CPU: every tensor goes there and comes back)."""
    gone = (fs | fr).to(where)
    keep, split = ~gone, fs.to(where)
    num_keep = int(keep.sum())
    cx, cs = split_uniform_torch(model.xyz[fs], model.scaling[fs], model.rotation[fs], children)
    kids = {"xyz": cx.to(where), "scaling": cs.to(where)}
    for k in model.keys:
        old = getattr(model, k).to(where)
        kid = kids[k] if k in kids else old[split][:, None].repeat(1, children, *[1] * (old.dim() - 1)).reshape(-1, *old.shape[1:])
        getattr(model, k).set_(torch.cat([old[keep], kid]).to(dev))
        del old, kid
    index = torch.where(keep)[0]
    for sk in opt.state_keys:
        for k, val in getattr(opt, sk).items():
            old = val.to(where)
            zeros = torch.zeros((getattr(model, k).shape[0] - num_keep,) + tuple(old.shape[1:]), dtype=old.dtype, device=where)
            val.set_(torch.cat([old[index], zeros]).to(dev))
            del old, zeros
    return num_keep


def wall_ms(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stream_copy_rate(mib=1024, reps=4):
    """Best GB/s (read + write) of lograst_stream_copy over its forms and a few grid sizes, as bench.py measures it."""
    L = _lib.lib()
    nbytes = mib << 20
    a = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    stream = R._stream_ptr(dev)
    pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
    best = float("inf")
    for form in range(5):
        for blocks in ((0,) if form in (1, 4) else (2048, 4096, 8192)):
            arg = (form << 20) | blocks
            _lib.check(L.lograst_stream_copy(pb, pa, nbytes, arg, stream))
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(L.lograst_stream_copy(pb, pa, nbytes, arg, stream))
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1))
    return 2 * nbytes / (best * 1e-3) / 1e9


def row_move(n, degree, fs, fr, children, reps):
    """-> kernel ms of all row-move launches of one split_and_remove, the payload bytes, and the streaming copy's rate."""
    model, opt = make_state(n, degree, 5)
    plan = densify.Plan(fs, fr, True, children)
    items = [(getattr(model, k), _lib.MOVE_SKIP if k in ("xyz", "scaling") else _lib.MOVE_COPY_PARENT) for k in model.keys]
    for sk in opt.state_keys:
        items += [(v, _lib.MOVE_ZERO) for _, v in getattr(opt, sk).items()]
    payload = 0
    for t, mode in items:
        rb = t[0].numel() * t.element_size()
        payload += 2 * plan.num_keep * rb + (2 if mode == _lib.MOVE_COPY_PARENT else (1 if mode == _lib.MOVE_ZERO else 0)) \
            * (plan.num_new - plan.num_keep) * rb
    L = _lib.lib()
    groups = list(densify._groups(items, lambda it: densify._row_bytes(it[0])))
    ms = []
    for _ in range(reps + 1):
        total = 0.0
        for group in groups:
            dsts = [torch.empty((plan.num_new,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t, _ in group]
            keys = (_lib.LograstMoveKey * len(group))()
            for slot, (t, mode), d in zip(keys, group, dsts):
                slot.src, slot.dst, slot.elem_size, slot.columns, slot.child_mode = t.data_ptr(), d.data_ptr(), 4, t[0].numel(), mode
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(L.lograst_densify_move_rows(plan.num_keep, plan.num_new, n, R._ptr(plan.src_row), len(group), keys,
                                                   R._stream_ptr(dev)))
            e1.record()
            e1.synchronize()
            total += e0.elapsed_time(e1)
            del dsts
        ms.append(total)
    ms = ms[1:]
    del model, opt, items
    move_rate = payload / (statistics.median(ms) * 1e-3) / 1e9
    copy_rate = stream_copy_rate()
    return {"kernel_ms": statistics.median(ms), "launches": len(groups), "payload_GB": payload / 1e9, "GBps": move_rate,
            "stream_copy_GBps": copy_rate, "share_of_copy": move_rate / copy_rate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000000,30000000")
    ap.add_argument("--degrees", default="1,3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--children", type=int, default=4)
    ap.add_argument("--no-host", action="store_true", help="leave out the host round trip")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_densify needs the MI355X"
    import contextlib
    import io
    for n in (int(v) for v in a.sizes.split(",")):
        for degree in (int(v) for v in a.degrees.split(",")):
            fs, fr = make_flags(n, 1)
            times = {"dropin": [], "torch_device": []}
            counts = {}
            for it in range(a.reps + 1):
                for name, fn in (("dropin", lambda m, o: dropin(m, o, fs, fr, a.children)),
                                 ("torch_device", lambda m, o: by_torch(m, o, fs, fr, a.children, dev))):
                    model, opt = make_state(n, degree, 2)
                    with contextlib.redirect_stdout(io.StringIO()):
                        ms = wall_ms(fn, model, opt)
                    counts[name] = (int(model.xyz.shape[0]), float(model.xyz.double().sum()), float(opt.exp_avg.tensors["shs" if degree else "xyz"].double().sum()))
                    if it:
                        times[name].append(ms)
                    del model, opt
            host = None
            if not a.no_host:
                model, opt = make_state(n, degree, 2)
                host = wall_ms(by_torch, model, opt, fs, fr, a.children, torch.device("cpu"))
                counts["host_round_trip"] = (int(model.xyz.shape[0]), float(model.xyz.double().sum()), float(opt.exp_avg.tensors["shs" if degree else "xyz"].double().sum()))
                del model, opt
            rows = {k: v[0] for k, v in counts.items()}
            assert len(set(rows.values())) == 1, rows
            s = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            out = {"workload": f"Splitter.split_and_remove, {n} points, SH degree {degree}, children {a.children}, 5 % split, "
                               f"2 % removed, both Adam moments", "rows_after": rows["dropin"],
                   "bytes_per_point": 3 * 4 * sum(torch.Size(w).numel() for w in widths(degree).values()),
                   "reps": a.reps, "dropin": s(times["dropin"]), "torch_device": s(times["torch_device"]),
                   "host_round_trip_ms": host, "checksums": counts,
                   "row_move": row_move(n, degree, fs, fr, a.children, a.reps)}
            out["dropin_no_slower_than_torch_device"] = out["dropin"]["median_ms"] <= out["torch_device"]["median_ms"]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""The initialisation pass (Trainer.init -> LoG.init per training view, over ALL points) at the reference's own start-up
size: 3 M points, 64 orbit cameras at 1920x1080.  Three variants on a stand-in model, alternating in one process:

  (a) the op sequence LoG.init runs today on the device -- torch activations, the installed compute_radius, the four
      boolean-mask reads and writes (written from the reference's op list, LoG/model/level_of_gaussian.py:55-63, :328-332);
  (b) the drop-in of log_amd/init_pass.py with views_per_launch = 1: one launch per view;
  (c) the drop-in with all views in one launch.

One warm-up round, then ROUNDS rounds over all views; wall time between synchronisations around a whole pass, median and
min - max, also per view.  Host synchronisations per view are counted with torch's synchronisation check in "warn" mode
(one separate, untimed view per variant).  HIP-event time of the kernel alone for one view and for all views, next to
lograst_stream_copy moving the same 52 bytes per point (48 read + 4 written) in the same process.  (b) and (c) must agree
bit for bit; (a) differs from them in the last bits (torch.exp against the kernel's exp, 1 / r * 3 against 3 / r): the
largest relative difference is reported.

    python tools/bench_init_pass.py [--points N] [--views V] [--rounds R] [--out FILE.md]
-> a markdown report (also written to --out, default profiles/init_pass_stage.md) + one JSON line
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
import types
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from log_amd import _lib, init_pass, rasterizer as R, scenes       # noqa: E402

W, H = 1920, 1080
BYTES_PER_POINT = 52        # xyz 12 + scaling 12 + rotation 16 + radius3d_min 4 read, radius3d_min 4 written


def make_model(P, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    f = dict(device=dev, generator=gen)
    act = types.SimpleNamespace(scaling_activation=torch.exp, scaling_inverse_activation=torch.log,
                                rotation_activation=torch.nn.functional.normalize)
    lo, hi = math.log(0.002), math.log(0.05)
    g = types.SimpleNamespace(xyz=torch.rand(P, 3, **f) - 0.5, scaling=torch.rand(P, 3, **f) * (hi - lo) + lo,
                              rotation=torch.randn(P, 4, **f), activation=act)
    return types.SimpleNamespace(gaussian=g, counter=types.SimpleNamespace(radius3d_min=torch.ones(P, device=dev)),
                                 num_views=0)


def reset(model):
    model.counter.radius3d_min.fill_(1.0)       # LoG's own start value
    model.num_views = 0


def rasterizers(n, dev):
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    out = []
    for c in scenes.orbit_cameras(n, W=W, H=H):
        rs = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(c["FoVx"] * 0.5), tanfovy=math.tan(c["FoVy"] * 0.5),
            bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=T(c["world_view_transform"]),
            projmatrix=T(c["full_proj_transform"]), sh_degree=0, campos=T(c["camera_center"]), prefiltered=False, debug=False)
        out.append(GaussianRasterizer(raster_settings=rs))
    return out


# ---- (a): the reference's ops, on the device ---------------------------------------------------------------------------
def torch_init(model, renderer, batch, iteration):
    g = model.gaussian
    scaling = torch.exp(g.scaling)
    rotation = torch.nn.functional.normalize(g.rotation)
    camera, rasterizer, background = renderer.prepare_camera(batch, 0, renderer.background)
    radius2d = rasterizer.compute_radius(g.xyz, scaling, rotation)
    valid = radius2d > 0
    radius3d = scaling[:, 0]
    radius3d[valid] = radius3d[valid] * (3. / radius2d[valid])
    rmin = model.counter.radius3d_min
    rmin[valid] = torch.minimum(rmin[valid], radius3d[valid])
    model.num_views += 1


# ---- timing ----------------------------------------------------------------------------------------------------------
def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def synchronisations(fn):
    """Host synchronisations torch reports for one call of fn."""
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def summary(xs, views):
    med = statistics.median(xs)
    return {"median_ms": med, "min_ms": min(xs), "max_ms": max(xs), "per_view_ms": med / views, "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=3_000_000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_pass_stage.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_init_pass needs the MI355X: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    P, V = a.points, a.views
    rasts = rasterizers(V, dev)
    renderer = types.SimpleNamespace(background=None, prepare_camera=lambda batch, bn, bg: ({}, batch["rasterizer"], bg))
    batches = [{"rasterizer": r} for r in rasts]
    models = {k: make_model(P, dev) for k in ("torch", "per_view", "one_launch")}

    def run_pass(model, init, k):
        reset(model)
        init_pass.set_views_per_launch(k)
        for i, b in enumerate(batches):
            init(model, renderer, b, i)
        init_pass.flush(model)

    variants = {"torch": (torch_init, 1), "per_view": (init_pass.log_init, 1), "one_launch": (init_pass.log_init, V)}
    times = {k: [] for k in variants}
    init_pass.reset_stats()
    try:
        for rnd in range(a.rounds + 1):
            for name, (init, k) in variants.items():
                t = wall(lambda: run_pass(models[name], init, k))
                if rnd:
                    times[name].append(t)
        rmin = {k: m.counter.radius3d_min for k, m in models.items()}
        assert torch.equal(rmin["per_view"], rmin["one_launch"]), "batching changed a bit"
        rel = ((rmin["torch"].double() / rmin["per_view"].double()) - 1).abs().max().item()
        lowered = (rmin["per_view"] < 1.0).float().mean().item()
        stats = init_pass.stats()
        syncs = {}
        for name, (init, k) in variants.items():
            init_pass.set_views_per_launch(k)
            reset(models[name])
            syncs[name] = synchronisations(lambda: init(models[name], renderer, batches[0], 0))
            init_pass.flush(models[name])
    finally:
        init_pass.set_views_per_launch(1)

    # ---- the kernel alone (HIP events), next to a streaming copy of the same bytes ----
    L = _lib.lib()
    g = models["per_view"].gaussian
    one, every = init_pass.CameraTable(dev, 1), init_pass.CameraTable(dev, V)
    one.add(rasts[0].raster_settings)
    for r in rasts:
        every.add(r.raster_settings)
    t1, tv = one.finish(), every.finish()
    buf = models["per_view"].counter.radius3d_min
    k_one = events(lambda: init_pass._launch(dev, P, g.xyz, g.scaling, g.rotation, t1, buf))
    k_all = events(lambda: init_pass._launch(dev, P, g.xyz, g.scaling, g.rotation, tv, buf), reps=3)
    half = (BYTES_PER_POINT // 2 * P + 15) // 16 * 16
    src, dst = (torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(2))
    stream = R._stream_ptr(dev)
    t_copy = events(lambda: _lib.check(L.lograst_stream_copy(R._ptr(dst), R._ptr(src), half, 0, stream)))
    traffic = BYTES_PER_POINT * P

    out = {"shape": {"points": P, "views": V, "width": W, "height": H, "rounds": a.rounds},
           "wall": {k: summary(v, V) for k, v in times.items()},
           "kernel": {"one_view_ms": k_one, "all_views_ms": k_all, "all_views_per_view_ms": k_all / V,
                      "bytes_per_launch": traffic, "one_view_GBps": traffic / k_one / 1e6,
                      "stream_copy_ms": t_copy, "stream_copy_GBps": 2 * half / t_copy / 1e6,
                      "one_view_fraction_of_stream_copy": t_copy / k_one},
           "host_synchronisations_per_view": syncs,
           "readbacks": {str(k): v for k, v in stats["readbacks"].items()},
           "fallbacks": {str(k): v for k, v in stats["fallbacks"].items()},
           "rows_lowered": lowered, "torch_vs_kernel_max_relative": rel}

    w = out["wall"]
    names = {"torch": "(a) torch ops + compute_radius + boolean masks", "per_view": "(b) drop-in, views_per_launch = 1",
             "one_launch": f"(c) drop-in, {V} views in one launch"}
    md = ["# Initialisation pass on the device (`log_amd/init_pass.py`, `init.hip`)", "",
          f"`tools/bench_init_pass.py`: {P} points in a unit cube (raw scales log-uniform 0.002 - 0.05, random quaternions, "
          f"`radius3d_min` = 1), {V} orbit cameras at {W}x{H}, MI355X.  The three variants alternate in one process: one warm-up "
          f"round, {a.rounds} measured rounds; wall time between synchronisations around a whole pass of {V} views.", "",
          f"| variant | pass median (min - max) ms | per view ms | host synchronisations per view |", "|---|---|---|---|"]
    for k in ("torch", "per_view", "one_launch"):
        md.append(f"| {names[k]} | {w[k]['median_ms']:.3f} ({w[k]['min_ms']:.3f} - {w[k]['max_ms']:.3f}) | "
                  f"{w[k]['per_view_ms']:.4f} | {syncs[k]} |")
    kk = out["kernel"]
    md += ["", f"Read-backs of the library on behalf of the drop-ins (`init_pass.stats()['readbacks']`): {out['readbacks'] or 'none'}; "
               f"fall-backs: {out['fallbacks'] or 'none'}.", "",
           f"The kernel alone (HIP events): one view {kk['one_view_ms']:.4f} ms = {kk['one_view_GBps']:.0f} GB/s over "
           f"{BYTES_PER_POINT} B per point; {V} views in one launch {kk['all_views_ms']:.3f} ms = {kk['all_views_per_view_ms']:.4f} ms "
           f"per view.  `lograst_stream_copy` moving the same {traffic / 1e6:.0f} MB in the same process: {kk['stream_copy_ms']:.4f} ms "
           f"({kk['stream_copy_GBps']:.0f} GB/s): the one-view launch runs at {kk['one_view_fraction_of_stream_copy']:.2f} of the copy's "
           f"rate.  (At this size both the model and the copy's buffers fit the 256 MiB Infinity Cache, so neither rate is an HBM "
           f"rate.)", "",
           f"Results: (b) and (c) agree bit for bit; (a) differs from them by at most {rel:.1e} relative (torch.exp against the "
           f"kernel's exp, `1 / r * 3` against `3 / r`); {lowered:.3f} of the rows end below their start value.  No time here "
           f"is an acceptance threshold: the file records what was measured.", ""]
    text = "\n".join(md)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

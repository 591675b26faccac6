#!/usr/bin/env python3
"""What LoG's depth pass costs with and without geometry reuse (log_amd.rasterizer.set_geometry_reuse).

    python tools/bench_depth_pass.py [--scenes c2,trained,headline] [--repeats 20] [--warmup 3] [--out FILE.json]

For every scene one process times, with HIP events on the launch stream and after warm-up, the pair of rasterizer calls a
training view of `render_depth: True` makes (LoG/render/renderer.py:141-201): RGB forward, then the forward with colours
[view depth, world z, 1] through the SAME rasterizer object, then one backward over both.  Repeats with reuse off and on
alternate (off, on, off, on, ...), so that clocks, allocator state and the capacity model drift under both alike; medians
and min-max are reported for the first forward, the second forward and the whole pair.  "reuse off" is the code path of a
build without the feature, through the same library, in the same run: the reference every "on" figure is read against.
The package runs in its default mode (speculative stage 2: one 8-byte read-back per full forward on a side stream).

Scenes: c2 = BASELINE.json configs[1] (1 M random Gaussians, 1920x1080), headline = the 30 M point of bench.py, trained =
log_amd.scenes.trained_like_scene at 1 M.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SCENES = {"c2": ("random", 1_000_000), "trained": ("trained", 1_000_000), "headline": ("random", 30_000_000)}


def setup(kind, n, W, H, dev):
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    from log_amd import scenes
    sc = scenes.trained_like_scene(n, seed=0) if kind == "trained" else scenes.random_scene(n, seed=0)
    cam = scenes.orbit_cameras(8, W=W, H=H, focal=2139.0 * W / 1920.0)[1]
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    leaves = {k: T(sc[k]).requires_grad_(True) for k in ("xyz", "scaling", "rotation", "opacity", "colors")}
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam["FoVx"] * 0.5), tanfovy=math.tan(cam["FoVy"] * 0.5),
        bg=T([1.0, 1.0, 1.0]), scale_modifier=1.0, viewmatrix=T(cam["world_view_transform"]),
        projmatrix=T(cam["full_proj_transform"]), sh_degree=0, campos=T(cam["camera_center"]), prefiltered=False, debug=False)
    view = T(cam["world_view_transform"])
    rng = np.random.default_rng(1)
    w = [torch.tensor(rng.random((3, H, W), dtype=np.float32), device=dev) for _ in range(2)]
    return (lambda: GaussianRasterizer(raster_settings=rs)), leaves, view, w


def one_pair(make_rast, leaves, view, w, ev):
    """renderer.py:135-201 for one view; ev: four events around first forward | second forward | backward.  A rasterizer
    object per view, as LoG builds them (renderer.py:222)."""
    rast = make_rast()
    xyz = leaves["xyz"]
    m2 = torch.zeros_like(xyz, requires_grad=True)
    kw = dict(means3D=xyz, means2D=m2, shs=None, opacities=leaves["opacity"], scales=leaves["scaling"],
              rotations=leaves["rotation"], cov3D_precomp=None)
    xyz1 = torch.cat([xyz.detach(), torch.ones_like(xyz[:, :1])], dim=1)
    depth = (xyz1 @ view)[:, 2]
    colors_depth = torch.stack([depth, xyz[:, 2], torch.ones_like(depth)], dim=-1)
    ev[0].record()
    out1 = rast(colors_precomp=leaves["colors"], **kw)
    ev[1].record()
    out2 = rast(colors_precomp=colors_depth, **kw)
    ev[2].record()
    ((out1[0] * w[0]).sum() + (out2[0] * w[1]).sum()).backward()
    ev[3].record()
    for t in leaves.values():
        t.grad = None
    return out2[0]


def stats(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), n=len(xs))


def bench_scene(name, args, dev):
    from log_amd import rasterizer as R
    kind, n = SCENES[name]
    make_rast, leaves, view, w = setup(kind, n, args.width, args.height, dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    times = {mode: dict(first_forward=[], second_forward=[], backward=[], pair=[]) for mode in ("off", "on")}
    images = {}
    try:
        for rep in range(-args.warmup, args.repeats):
            for mode in ("off", "on"):
                R.set_geometry_reuse(mode == "on")
                R.geometry_reuse_stats(reset=True)
                img = one_pair(make_rast, leaves, view, w, ev)
                torch.cuda.synchronize()
                assert R.geometry_reuse_stats()["reused"] == (1 if mode == "on" else 0), R.geometry_reuse_stats()
                if rep < 0:
                    images[mode] = img.detach().clone()
                    continue
                t = times[mode]
                t["first_forward"].append(ev[0].elapsed_time(ev[1]))
                t["second_forward"].append(ev[1].elapsed_time(ev[2]))
                t["backward"].append(ev[2].elapsed_time(ev[3]))
                t["pair"].append(ev[0].elapsed_time(ev[3]))
    finally:
        R.set_geometry_reuse(False)
    same = bool(torch.equal(images["on"], images["off"]))
    res = dict(scene=name, gaussians=n, width=args.width, height=args.height, instances=R.last_state_info(dev)[0],
               depth_image_bitwise_equal=same,
               ms={mode: {k: stats(v) for k, v in t.items()} for mode, t in times.items()})
    off2, on2 = res["ms"]["off"]["second_forward"], res["ms"]["on"]["second_forward"]
    spread = off2["max"] - off2["min"]
    res["second_forward_saved_ms"] = round(off2["median"] - on2["median"], 4)
    res["second_forward_off_spread_ms"] = round(spread, 4)
    res["second_forward_beats_spread"] = bool(off2["median"] - on2["median"] > spread)
    f_off, f_on = res["ms"]["off"]["first_forward"], res["ms"]["on"]["first_forward"]
    res["first_forward_same_within_spread"] = bool(abs(f_on["median"] - f_off["median"]) <= f_off["max"] - f_off["min"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="c2,trained,headline")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 1 or args.warmup < 1:
        ap.error("--repeats and --warmup must be at least 1")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(dev), repeats=args.repeats, warmup=args.warmup, scenes=[])
    for name in args.scenes.split(","):
        if name not in SCENES:
            ap.error("unknown scene %r (of %s)" % (name, ", ".join(SCENES)))
        out["scenes"].append(bench_scene(name, args, dev))
        torch.cuda.empty_cache()
        print(json.dumps(out["scenes"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

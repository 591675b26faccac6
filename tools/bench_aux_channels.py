#!/usr/bin/env python3
"""What a depth-supervised view costs as two rasterizer calls, as two calls with geometry reuse, and as ONE call with aux
channels (GaussianRasterizer.forward(aux_colors=): colour and [view z, world z, 1] composited by the same walk).

    python tools/bench_aux_channels.py [--scenes c2,trained,headline] [--repeats 20] [--warmup 3] [--out FILE.json]

The protocol of tools/bench_depth_pass.py: one process per run, HIP events on the launch stream, after warm-up; the three
modes alternate (off, on, aux, off, on, aux, ...) so that clocks, allocator state and the capacity model drift under all
alike; every pair has one backward over both images.  Medians and min-max are reported for the forward part (both calls,
or the one aux call), the backward and the whole pair.

The reference is the reuse-on pair of the same run (the best path without aux channels).  A saving is claimed for a scene
only where the aux pair's median beats the reuse-on median by more than the min-max spread of the reuse-on repeats.

Scenes: c2 = BASELINE.json configs[1] (1 M random Gaussians, 1920x1080), headline = the 30 M point of bench.py, trained =
log_amd.scenes.trained_like_scene at 1 M.  Prints one JSON object per scene (and writes all to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from bench_depth_pass import SCENES, setup, stats  # noqa: E402

MODES = ("off", "on", "aux")


def one_view(mode, make_rast, leaves, view, w, ev):
    """LoG/render/renderer.py:135-201 for one view; ev: three events around forward(s) | backward.  -> (image, depth image)."""
    rast = make_rast()
    xyz = leaves["xyz"]
    m2 = torch.zeros_like(xyz, requires_grad=True)
    kw = dict(means3D=xyz, means2D=m2, shs=None, opacities=leaves["opacity"], scales=leaves["scaling"],
              rotations=leaves["rotation"], cov3D_precomp=None)
    xyz1 = torch.cat([xyz.detach(), torch.ones_like(xyz[:, :1])], dim=1)
    depth = (xyz1 @ view)[:, 2]
    colors_depth = torch.stack([depth, xyz[:, 2], torch.ones_like(depth)], dim=-1)
    ev[0].record()
    if mode == "aux":
        out = rast(colors_precomp=leaves["colors"], aux_colors=colors_depth, **kw)
        image, depth_image = out[0], out[-1]
    else:
        image = rast(colors_precomp=leaves["colors"], **kw)[0]
        depth_image = rast(colors_precomp=colors_depth, **kw)[0]
    ev[1].record()
    ((image * w[0]).sum() + (depth_image * w[1]).sum()).backward()
    ev[2].record()
    for t in leaves.values():
        t.grad = None
    return image, depth_image


def bench_scene(name, args, dev):
    from log_amd import rasterizer as R
    kind, n = SCENES[name]
    make_rast, leaves, view, w = setup(kind, n, args.width, args.height, dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    times = {mode: dict(forward=[], backward=[], pair=[]) for mode in MODES}
    images, forms = {}, {}
    try:
        for rep in range(-args.warmup, args.repeats):
            for mode in MODES:
                R.set_geometry_reuse(mode == "on")
                R.geometry_reuse_stats(reset=True)
                img = one_view(mode, make_rast, leaves, view, w, ev)
                torch.cuda.synchronize()
                assert R.geometry_reuse_stats()["reused"] == (1 if mode == "on" else 0), R.geometry_reuse_stats()
                forms[mode] = dict(R._backend.last_forms)
                if rep < 0:
                    images[mode] = [t.detach().clone() for t in img]
                    continue
                t = times[mode]
                t["forward"].append(ev[0].elapsed_time(ev[1]))
                t["backward"].append(ev[1].elapsed_time(ev[2]))
                t["pair"].append(ev[0].elapsed_time(ev[2]))
    finally:
        R.set_geometry_reuse(False)
    same = all(bool(torch.equal(a, b)) for m in ("on", "aux") for a, b in zip(images[m], images["off"]))
    res = dict(scene=name, gaussians=n, width=args.width, height=args.height, instances=R.last_state_info(dev)[0],
               images_bitwise_equal=same, forms=forms,
               ms={mode: {k: stats(v) for k, v in t.items()} for mode, t in times.items()})
    on, aux = res["ms"]["on"]["pair"], res["ms"]["aux"]["pair"]
    res["reuse_on_spread_ms"] = round(on["max"] - on["min"], 4)
    res["aux_saved_ms"] = round(on["median"] - aux["median"], 4)
    res["aux_beats_reuse_on_by_more_than_its_spread"] = bool(on["median"] - aux["median"] > on["max"] - on["min"])
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

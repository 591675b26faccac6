#!/usr/bin/env python3
"""What the camera sums (dL/dviewmatrix, dL/dprojmatrix) cost in the backward's chain-rule stage.

    python tools/bench_camera_grad.py [--scenes c2,trained,headline] [--repeats 20] [--warmup 3] [--out FILE.json]

One process, HIP events on the launch stream, after warm-up; within every arm the plain call and the camera call alternate
(plain, camera, plain, camera, ...) so that clocks and allocator state drift under both alike.  Milliseconds, median and
min-max.  The yardstick is the plain call of the SAME run: its kernels have the parent's instructions
(profiles/camera_gradients.md), so "the plain path is unchanged" is read off the plain figures against the parent's own run
of this scene, and the camera cost off the difference inside one run.  Arms:

  backward   HipBackend.backward / backward_camera on one forward's record: reverse walk + chain rule, the instantiations the
             autograd route launches (accumulator rows in, live flags from point_weight).  The accumulator rows are cleared
             before every call, outside the timed span.
  chain      HipBackend.project_backward(camera=False / True) on that backward's dL/dmeans2D / dL/dconic: the chain-rule launch
             alone (+ the finishing kernel), the isolated form.
  dead       the same with radii = 0 everywhere: no live row, so both calls are the flag pass and the zero stores, and
             camera - plain is the partials' stores plus the finishing kernel over ceil(N / 1024) rows of partials.

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


def bench_scene(name, args, dev):
    from log_amd import _lib, rasterizer as R
    kind, n = SCENES[name]
    make_rast, leaves, _, w = setup(kind, n, args.width, args.height, dev)
    rs = make_rast().raster_settings
    m, s, r, o, c = (leaves[k].detach() for k in ("xyz", "scaling", "rotation", "opacity", "colors"))
    B, fl = R._backend, R.WODILATE
    R._debug_keep = True
    _, radii, _, _, _, saved = B.forward(rs, fl, True, m, s, r, o.reshape(-1), c, scratch_floats=_lib.BWD_ROW_FLOATS)
    g_image = w[0].contiguous()
    rows = saved["bwd_scratch"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out

    def backward(camera):
        rows.zero_()
        saved["bwd_scratch"] = rows          # (the call takes the block; handed back for the next one)
        fn = B.backward_camera if camera else B.backward
        return timed(lambda: fn(rs, fl, True, m, s, r, saved, g_image))

    _, g = backward(False)           # (once with the test hook that keeps dL/dconic: the isolated form's input)
    R._debug_keep = False
    g_m2 = g[1].clone()
    g_conic = B.last_conic_grad.clone().contiguous()
    B.last_conic_grad = None
    live = int((saved["point_weight"] > 0).sum())
    dead_radii = torch.zeros_like(radii)
    arms = {
        "backward": backward,
        "chain": lambda camera: timed(lambda: B.project_backward(rs, fl, True, m, s, r, radii, g_m2, g_conic, camera=camera)),
        "dead": lambda camera: timed(lambda: B.project_backward(rs, fl, True, m, s, r, dead_radii, g_m2, g_conic, camera=camera)),
    }
    res = dict(scene=name, gaussians=n, live_rows=live, width=args.width, height=args.height, ms={})
    for arm, call in arms.items():
        times = {False: [], True: []}
        keep = {}
        for rep in range(-args.warmup, args.repeats):
            for camera in (False, True):
                t, out = call(camera)
                keep[camera] = out
                if rep >= 0:
                    times[camera].append(t)
        plain, cam = stats(times[False]), stats(times[True])
        res["ms"][arm] = dict(plain=plain, camera=cam, camera_minus_plain=round(cam["median"] - plain["median"], 4),
                              plain_spread=round(plain["max"] - plain["min"], 4))
        if arm == "chain":   # the per-Gaussian outputs of the isolated form are the plain call's bits
            res["chain_outputs_bitwise_equal"] = all(bool(torch.equal(a, b)) for a, b in zip(keep[False], keep[True][:3]))
        if arm == "dead":
            res["dead_camera_gradients_are_zero"] = not bool(keep[True][3].any() or keep[True][4].any())
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

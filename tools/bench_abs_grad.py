#!/usr/bin/env python3
"""What the absolute screen-space sums (lograst_backward_abs: ``means2D.absgrad``) cost in the backward.

    python tools/bench_abs_grad.py [--scenes c2,trained,headline] [--repeats 20] [--warmup 3] [--form rows|quadrant] [--out FILE.json]

One process, HIP events on the launch stream, after warm-up; the plain backward and the abs backward alternate (plain, abs,
plain, abs, ...) on one forward's record, so that clocks and allocator state drift under both alike.  Milliseconds, median
and min-max.  The yardstick is the plain backward of the SAME run: its kernels have the parent's instructions
(profiles/abs_grad.md), and the cost of the abs sums is read off the difference inside one run, against the plain
backward's own min-max spread.

  backward   HipBackend.backward / backward_abs: reverse walk + chain rule, the instantiations the autograd route launches
             (accumulator rows in, live flags from point_weight).  The accumulator rows are cleared before every call,
             outside the timed span.
  kernels    the same calls once more under the library's own per-kernel events (lograst_profile_*): the reverse walk and
             the chain rule apart, mean over --repeats calls.

--form pins the walk form of forward and backward (default: the package's choice -- quadrant for c2 and trained, row-split
for the headline).  Scenes: c2 = BASELINE.json configs[1] (1 M random Gaussians, 1920x1080), headline = the 30 M point of
bench.py, trained = log_amd.scenes.trained_like_scene at 1 M.  Prints one JSON object per scene (and writes all to --out)."""
import argparse
import contextlib
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
    with (R.walk_form(args.form) if args.form else contextlib.nullcontext()):
        _, radii, _, _, _, saved = B.forward(rs, fl, True, m, s, r, o.reshape(-1), c, scratch_floats=_lib.BWD_ROW_FLOATS)
    g_image = w[0].contiguous()
    rows = saved["bwd_scratch"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def backward(abs_sums, timed=True):
        rows.zero_()
        saved["bwd_scratch"] = rows          # (the call takes the block; handed back for the next one)
        fn = B.backward_abs if abs_sums else B.backward
        ev[0].record()
        out = fn(rs, fl, True, m, s, r, saved, g_image)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out

    times = {False: [], True: []}
    keep = {}
    for rep in range(-args.warmup, args.repeats):
        for abs_sums in (False, True):
            t, out = backward(abs_sums)
            keep[abs_sums] = out
            if rep >= 0:
                times[abs_sums].append(t)
    form = B.last_forms.get("bwd")
    plain, ab = stats(times[False]), stats(times[True])
    spread = round(plain["max"] - plain["min"], 4)
    diff = round(ab["median"] - plain["median"], 4)
    res = dict(scene=name, gaussians=n, live_rows=int((saved["point_weight"] > 0).sum()), width=args.width, height=args.height,
               bwd_form=form, hit_mask_form=int(saved["hit_mask_form"]),
               ms=dict(backward=dict(plain=plain, abs=ab, abs_minus_plain=diff, plain_spread=spread,
                                     exceeds_plain_spread=bool(abs(diff) > spread))))
    # the ordinary gradients of both calls agree (same sums, another order of the atomics); the abs sums dominate the signed ones
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))
    res["max_rel_l2_of_the_six_gradients"] = max(rel(a, b) for a, b in zip(keep[True][:6], keep[False]))
    g2, a2 = keep[True][1], keep[True][6]
    res["absgrad_norm_over_signed_norm"] = float(a2.double().norm() / g2.double().norm().clamp_min(1e-300))
    res["signed_within_abs"] = bool((g2[:, :2].abs() <= a2[:, :2] * (1.0 + 2.0 * args.width * args.height * 2.0 ** -24)).all())
    # per kernel
    kern = {}
    for abs_sums in (False, True):
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        _lib.profile_reset()
        for _ in range(args.repeats):
            backward(abs_sums)
        prof = _lib.profile_read()
        _lib.profile_enable(False)
        kern["abs" if abs_sums else "plain"] = {k: round(ms / cnt, 4) for k, (ms, cnt) in prof.items()}
    res["ms"]["kernels"] = kern
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="c2,trained,headline")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--form", default=None, choices=["rows", "quadrant"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 1 or args.warmup < 1:
        ap.error("--repeats and --warmup must be at least 1")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(dev), repeats=args.repeats, warmup=args.warmup, form=args.form,
               library=os.path.basename(_lib_path()), scenes=[])
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


def _lib_path():
    from log_amd import _lib
    return _lib.LIB_PATH


if __name__ == "__main__":
    main()

"""Steps over several views at the C3 shape (BASELINE.json configs[2]: the 10 M-point 4-ary tree of tools/bench_log_step.py, SH
degree 3, 1080p orbit views, the level-of-detail selection the bench's C3 leg makes and the radii of its render): what the two
kernels of log_amd/csrc/accumulate.hip cost next to the parent's kernels doing the same work.

  per view   lograst_activate_backward_accumulate  vs  lograst_activate_backward alone (compact gradients, nothing added)
                                                   vs  that kernel + index_add_ of the live rows per key (the live row list
                                                       is made outside the timed region)
  per step   lograst_accumulated_adam over the rows K views saw, K in {1, 4, 16}
                                                   vs  K calls of lograst_sparse_adam, one per view (the parent's steps: K
                                                       Adam steps, not one -- the work the parent does for K views)

HIP events around each side, one warm-up round, then ROUNDS rounds with the sides alternating in one process; medians with
min - max.  Next to every time: the bytes derived from the shapes (header of accumulate.hip).

    python tools/bench_multi_view.py [rounds] [roots] [levels] [out.md]     (default out: profiles/multi_view_stage.md)
"""
import json
import math
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_log_step as B          # noqa: E402
from log_amd import lod, multi_view as mv, rasterizer as R       # noqa: E402
from log_amd.dist import _Flat      # noqa: E402

KS = (1, 4, 16)
B1, B2, EPS = 0.9, 0.999, 1e-15
LRS = {"xyz": 1.6e-4, "scaling": 5e-3, "opacity": 0.05, "rotation": 1e-3, "colors": 2.5e-3, "shs": 1.25e-4}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def fmt(s):
    return f"{s['median_ms']:.3f} ({s['min_ms']:.3f} - {s['max_ms']:.3f})"


def make_view(wl, bufs, cam):
    """The C3 leg's selection and render of one camera -> what a backward of that view holds."""
    rast, camera = wl.rasterizer_for(cam)
    g = torch.Generator(device=wl.dev).manual_seed(int(1000 * cam["camera_center"][0]) % 9973)
    gaussian = types.SimpleNamespace(**bufs)
    with torch.no_grad():
        index_all = lod.traverse(wl.tree, gaussian, wl.roots, rast)
        index, index_node = B.split_leaf_node(wl, index_all)
        rows = torch.cat([index, index_node])
        raw, act = R._backend.gather_activate(rows, bufs, wl.D, camera["camera_center"])
        radii = rast(means3D=act["xyz"], means2D=torch.zeros_like(act["xyz"]), shs=None, colors_precomp=act["colors"],
                     opacities=act["opacity"], scales=act["scaling"], rotations=act["rotation"], cov3D_precomp=None)[1]
    n = int(index.shape[0])
    ups = tuple(torch.randn(rows.shape[0], w, device=wl.dev, generator=g) for w in (3, 3, 1, 4, 3))
    live = radii[:n] > 0
    return {"n": n, "rows": int(rows.shape[0]), "index": index, "radii": radii.to(torch.int32), "raw": raw, "ups": ups,
            "campos": camera["camera_center"], "live": live, "live_rows": torch.nonzero(live).squeeze(1),
            "n_live": int(live.sum())}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    roots = int(sys.argv[2]) if len(sys.argv) > 2 else 40000
    levels = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "multi_view_stage.md")
    wl = B.Workload(roots=roots, levels=levels, sh_degree=3, views=max(KS))
    dev, P, K, D = wl.dev, wl.P, wl.K, wl.D
    bufs = {k: v.clone() for k, v in wl.bufs.items()}
    views = [make_view(wl, bufs, cam) for cam in wl.cams]
    keys = ("xyz", "scaling", "opacity", "rotation", "colors", "shs")
    flat = _Flat(P, dev, sh_coeffs=K)
    acc = {k: flat.alias[mv.KEY_TO_FLAT[k]] for k in keys}
    seen = torch.zeros(P, dtype=torch.int32, device=dev)
    moved = torch.zeros(P, dtype=torch.uint8, device=dev)
    m1 = {k: torch.zeros_like(v) for k, v in bufs.items()}
    m2 = {k: torch.zeros_like(v) for k, v in bufs.items()}
    bc1, bc2 = 1 - B1 ** 10, 1 - B2 ** 10

    def parent_backward(v):
        g = R._backend.activate_backward(v["raw"], v["n"], D, v["campos"], v["ups"][1], v["ups"][2], v["ups"][3], v["ups"][4])
        g["xyz"] = v["ups"][0][:v["n"]]
        return g

    def parent_add(v):
        g = parent_backward(v)
        rows = v["index"].index_select(0, v["live_rows"])
        for k in keys:
            acc[k].index_add_(0, rows, g[k].index_select(0, v["live_rows"]))
        seen.index_add_(0, rows, torch.ones_like(rows, dtype=torch.int32))

    def ours(v):
        R._backend.activate_backward_accumulate(v["raw"], v["n"], D, v["campos"], *v["ups"], v["index"], v["radii"], acc, seen)

    def our_step():
        R._backend.accumulated_adam(seen, {k: (bufs[k], acc[k], m1[k], m2[k], None, LRS[k] / bc1) for k in keys}, B1, B2,
                                    math.sqrt(bc2), EPS, moved)

    def parent_steps(batch, grads):
        for v, g in zip(batch, grads):
            R._backend.sparse_adam(v["index"], v["live"], [(bufs[k], v["raw"][k][:v["n"]], g[k], m1[k], m2[k], None, LRS[k] / bc1)
                                                           for k in keys], B1, B2, math.sqrt(bc2), EPS)

    per_view = {"accumulate": [], "parent_backward": [], "parent_backward_index_add": []}
    per_step = {k: {"accumulated_adam": [], "parent_sparse_adam_x_K": [], "rows_seen": 0, "row_visits": 0} for k in KS}
    for rnd in range(rounds + 1):
        for v in views[:4]:
            t = {"parent_backward": timed(lambda: parent_backward(v)), "accumulate": timed(lambda: ours(v)),
                 "parent_backward_index_add": timed(lambda: parent_add(v))}
            if rnd:
                for k, x in t.items():
                    per_view[k].append(x)
        flat.flat.zero_()
        seen.zero_()
        for k in KS:
            batch = views[:k]
            for v in batch:
                ours(v)
            per_step[k]["rows_seen"] = int((seen > 0).sum())
            per_step[k]["row_visits"] = int(seen.sum())
            t_ours = timed(our_step)
            grads = [parent_backward(v) for v in batch]
            t_parent = timed(lambda: parent_steps(batch, grads))
            del grads
            if rnd:
                per_step[k]["accumulated_adam"].append(t_ours)
                per_step[k]["parent_sparse_adam_x_K"].append(t_parent)
    assert int(seen.abs().sum()) == 0 and float(flat.flat.abs().sum()) == 0.0

    W = 14 + 3 * K
    n_live = statistics.mean(v["n_live"] for v in views[:4])
    n_rows = statistics.mean(v["n"] for v in views[:4])
    bytes_acc = n_live * (112 + 8 * W + 8) + (n_rows - n_live) * 12
    bytes_parent = n_rows * (100 + 4 * (W - 3))
    out = {"shape": {"points": P, "sh_coeffs": K, "degree": D, "views": len(views), "rounds": rounds,
                     "parameter_rows_per_view": n_rows, "live_rows_per_view": n_live},
           "per_view": {k: summary(v) for k, v in per_view.items()},
           "per_step": {str(k): {"accumulated_adam": summary(d["accumulated_adam"]),
                                 "parent_sparse_adam_x_K": summary(d["parent_sparse_adam_x_K"]), "rows_seen": d["rows_seen"],
                                 "row_visits": d["row_visits"]} for k, d in per_step.items()}}
    gbs = lambda b, ms: b / ms / 1e6
    lines = ["# Steps over several views: what the two kernels cost (tools/bench_multi_view.py)", "",
             f"One MI355X, the C3 shape: {P} points, SH degree {D} ({K} coefficients, {W} floats per row), "
             f"{len(views)} orbit views at 1080p, each with the level-of-detail selection of the bench's C3 leg and the radii of "
             f"its render: {n_rows:.0f} parameter rows per view, {n_live:.0f} of them live (radii > 0), mean of the four views "
             f"timed.  HIP events around each side, one warm-up round, {rounds} rounds, the sides alternating in one process; "
             "median (min - max) in ms.", "",
             "## Per view: the backward of `get_all`", "",
             "| side | ms | derived bytes | GB/s from them |", "|---|---|---|---|"]
    pv = out["per_view"]
    lines += [f"| `lograst_activate_backward_accumulate` (sums by model row) | {fmt(pv['accumulate'])} | {bytes_acc / 1e6:.1f} MB | "
              f"{gbs(bytes_acc, pv['accumulate']['median_ms']):.0f} |",
              f"| parent: `lograst_activate_backward` alone (compact gradients, nothing added) | {fmt(pv['parent_backward'])} | "
              f"{bytes_parent / 1e6:.1f} MB | {gbs(bytes_parent, pv['parent_backward']['median_ms']):.0f} |",
              f"| parent: that kernel + `index_add_` of the live rows per key | {fmt(pv['parent_backward_index_add'])} | | |", "",
             f"Derived bytes per live row, accumulate: 100 upstream and raw + 12 index and radii + 2 x 4 x {W} sums read and "
             f"written + 8 for the count = {112 + 8 * W + 8}; a row with radii <= 0 costs its 12 bytes of index and radii.  "
             f"Parent alone: 100 read + 4 x {W - 3} written per parameter row (dL/dxyz passes through unwritten).  The "
             "`index_add_` side's live row list is made outside the timed region; its gathers and adds are torch's kernels.", "",
             "## Per step: Adam over the rows K views saw", "",
             "| K | rows seen | row visits | `lograst_accumulated_adam` ms | derived bytes | GB/s | parent: K x `lograst_sparse_adam` ms |",
             "|---|---|---|---|---|---|---|"]
    for k in KS:
        d = out["per_step"][str(k)]
        b = P * 5 + d["rows_seen"] * 32 * W
        lines.append(f"| {k} | {d['rows_seen']} | {d['row_visits']} | {fmt(d['accumulated_adam'])} | {b / 1e6:.1f} MB | "
                     f"{gbs(b, d['accumulated_adam']['median_ms']):.0f} | {fmt(d['parent_sparse_adam_x_K'])} |")
    lines += ["", f"Derived bytes, accumulated step: 5 per model row (the count read, the moved flag written) + 32 x {W} per seen "
              "row (gradient, parameter and two moments read; all four written, the gradient as zero).  The parent's side is K "
              "single-view steps -- K Adam updates of a row K views saw, not one: it is the work the parent does for K views, not "
              "the same result.  A separate zero pass over the sums (P x " + str(W) + " floats = "
              f"{P * W * 4 / 1e9:.2f} GB written) is what the one-pass step avoids; it was not run.", "",
              "## Not measured", "",
              "- `bench.py` does not touch this code (it is unchanged).",
              "- A LoG training run end to end with `views_per_step` > 1, and the clamp of the moved rows (`lograst_clamp_scale` "
              "over all rows with the moved flag), which follows each step.",
              "- The row-major target layout (16-float rows); the attribute-major blocks of `log_amd.dist._Flat` were timed.",
              "- Counters (`rocprofv3 --pmc`): the GB/s above are the derived bytes over the event times.", "",
              "```json", json.dumps(out), "```", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

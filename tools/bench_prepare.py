"""View preparation at the C3 shape (BASELINE.json configs[2]: the 10 M-point 4-ary tree of tools/bench_log_step.py, 1080p,
8 orbit views): the drop-ins of log_amd/prepare.py against the same results from torch ops on the device, written from the
reference's op list (LoG.prepare / LoG.clamp_scale, LoG/model/level_of_gaussian.py:223-256, :367-377) around the SAME
rasterizer and the SAME log_amd.lod.traverse.  The two sides alternate in one process: one warm-up round, then ROUNDS
rounds over all views; wall time between synchronisations, median and min - max per view.  Also: HIP-event time of the new
entry points alone with the bytes they move (from the shapes), next to lograst_stream_copy in the same process.

    python tools/bench_prepare.py [rounds] [roots] [levels]  -> a markdown table + one JSON line
(also written to the file named by the environment variable BENCH_PREPARE_OUT, when set)
"""
import ctypes
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_log_step as B          # noqa: E402
from log_amd import _lib, lod, prepare, rasterizer as R       # noqa: E402


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def model_of(wl):
    act = types.SimpleNamespace(scaling_activation=torch.exp, scaling_inverse_activation=torch.log,
                                opacity_activation=torch.sigmoid, rotation_activation=torch.nn.functional.normalize)
    g = types.SimpleNamespace(activation=act, visibility_flag=None, **{k: v.clone() for k, v in wl.bufs.items()})
    tree = types.SimpleNamespace(node_index=wl.tree.node_index, tree=wl.tree.tree, depth=wl.tree.depth,
                                 root_index=wl.roots.to(torch.int32), max_level=30, min_resolution_pixel=B.MIN_PX,
                                 num_nodes=wl.num_nodes)
    gen = torch.Generator(device=wl.dev).manual_seed(1)
    mid = g.scaling.mean(dim=1)
    rmin = torch.exp(mid + 0.3 * torch.randn(wl.P, device=wl.dev, generator=gen))
    rmax = rmin * torch.exp(torch.rand(wl.P, device=wl.dev, generator=gen) * 1.2 - 0.2)
    counter = types.SimpleNamespace(radius3d_min=rmin, radius3d_max=rmax)
    return types.SimpleNamespace(gaussian=g, tree=tree, counter=counter, current_depth=wl.tree_levels,
                                 optimizer_cfg=_Cfg(opt_all_levels=True))


# ---- the reference's ops, on the device ------------------------------------------------------------------------------
def torch_visible(xyz, proj, padding):
    xyz1 = torch.cat([xyz, torch.ones_like(xyz[:, :1])], dim=1)
    h = xyz1 @ proj
    pw = 1.0 / (h[..., 3:4] + 1e-7)
    p = h[:, :3] * pw
    depth = p[:, 2]
    return (depth > 0.) & (depth < 1.) & (p[:, 0] > -1 - padding) & (p[:, 0] < 1. + padding) & \
        (p[:, 1] > -1 - padding) & (p[:, 1] < 1. + padding)


def torch_prepare(m, rast, camera):
    g, tree = m.gaussian, m.tree
    root_index = tree.root_index.long()
    xyz = g.xyz[root_index]
    flag = torch_visible(xyz, camera["full_proj_transform"], 0.5)
    in_range = root_index[flag]                                                     # read-back 1
    opacity = torch.sigmoid(g.opacity)
    scaling = torch.exp(g.scaling)
    rotation = torch.nn.functional.normalize(g.rotation)
    sel = types.SimpleNamespace(xyz=xyz[in_range], scaling=scaling[in_range], rotation=rotation[in_range],
                                opacity=opacity[in_range])
    weight = prepare.root_weight(rast, sel)
    flag[flag.clone()] = weight > 1e-8                                              # read-back 2
    roots = root_index[flag]                                                        # read-back 3
    index_all = lod.traverse(tree, g, roots, rast, max_depth=m.current_depth)       # the traversal's own read-back
    leaf = (tree.node_index[index_all] == -1) & (tree.depth[index_all] > 0)
    g.visibility_flag = {"root_flag": flag, "index": index_all[leaf], "index_node": index_all[~leaf]}    # read-backs 4, 5


def torch_clamp(m, index, flag_vis):
    g = m.gaussian
    index = index[flag_vis]                                                         # LoG.step's read-back
    scaling = g.scaling[index]
    smax = m.counter.radius3d_max[index][:, None].expand(-1, 3)
    smin = m.counter.radius3d_min[index][:, None].expand(-1, 3)
    g.scaling[index] = torch.clamp(scaling, torch.log(smin), torch.log(smax))


def device_clamp(m, index, flag_vis):
    prepare._clamp_launch(*prepare._clamp_inputs(m, index, flag_vis))


# ---- timing ----------------------------------------------------------------------------------------------------------
def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    roots = int(sys.argv[2]) if len(sys.argv) > 2 else 40000
    levels = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    wl = B.Workload(roots=roots, levels=levels, sh_degree=0, views=8)
    dev = wl.dev
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    views = [(wl.rasterizer_for(c)[0], {"full_proj_transform": T(c["full_proj_transform"])}) for c in wl.cams]
    models = {"device": model_of(wl), "torch": model_of(wl)}
    sides = {"device": (prepare.log_prepare, device_clamp), "torch": (torch_prepare, torch_clamp)}
    gen = torch.Generator(device=dev).manual_seed(2)
    times = {s: {"prepare": [], "clamp_scale": []} for s in sides}
    shapes = []
    for rnd in range(rounds + 1):
        for vi, (rast, camera) in enumerate(views):
            vis = None
            for side, (prep, clamp) in sides.items():
                m = models[side]
                t_prep = wall(lambda: prep(m, rast, camera))
                vf = m.gaussian.visibility_flag
                if vis is None:
                    vis = torch.rand(vf["index"].shape[0], device=dev, generator=gen) < 0.8
                index = vf["index"]
                t_clamp = wall(lambda: clamp(m, index, vis))
                if rnd:
                    times[side]["prepare"].append(t_prep)
                    times[side]["clamp_scale"].append(t_clamp)
            a, b = models["device"].gaussian, models["torch"].gaussian
            for k in ("root_flag", "index", "index_node"):
                assert torch.equal(a.visibility_flag[k], b.visibility_flag[k]), (vi, k)
            assert torch.allclose(a.scaling, b.scaling, rtol=0, atol=2e-6, equal_nan=True), vi
            if rnd == 0:
                shapes.append({"view": vi, "roots_in_range": int(prepare.frustum_select(
                    a.xyz, camera["full_proj_transform"], 0.5, rows=models["device"].tree.root_index).count),
                    "roots_kept": int(a.visibility_flag["root_flag"].sum()), "index": int(a.visibility_flag["index"].shape[0]),
                    "index_node": int(a.visibility_flag["index_node"].shape[0]), "clamped_rows": int(vis.sum())})
    out = {"shape": {"points": wl.P, "roots": wl.R0, "levels": wl.tree_levels, "width": B.W, "height": B.H, "views": len(views),
                     "rounds": rounds}, "views": shapes,
           "wall": {s: {k: summary(v) for k, v in t.items()} for s, t in times.items()}}

    # ---- the new entry points alone (HIP events), bytes from the shapes ----
    L = _lib.lib()
    m = models["device"]
    g, tree = m.gaussian, m.tree
    rast, camera = views[0]
    stream = R._stream_ptr(dev)
    proj = camera["full_proj_transform"].contiguous()
    Rn = int(tree.root_index.shape[0])
    sel = prepare.frustum_select(g.xyz, proj, 0.5, rows=tree.root_index, raw=(g.scaling, g.rotation, g.opacity))
    K = sel.count
    flag = torch.empty(Rn, dtype=torch.uint8, device=dev)
    pos, row = (torch.empty(Rn, dtype=torch.int64, device=dev) for _ in range(2))
    o = [torch.empty((Rn, w), device=dev) for w in (3, 3, 4, 1)]
    nb = L.lograst_frustum_scratch_bytes(Rn)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = R._ptr
    t_roots = events(lambda: _lib.check(L.lograst_frustum_select(
        Rn, wl.P, p(g.xyz), p(tree.root_index), p(proj), 0.5, p(g.scaling), p(g.rotation), p(g.opacity), p(flag), p(pos), p(row),
        *[p(t) for t in o], p(scratch), nb, stream)))
    bytes_roots = Rn * (4 + 12 + 1 + 1) + K * (8 + 8 + 12 + 28 + 44)
    flagP = torch.empty(wl.P, dtype=torch.uint8, device=dev)
    posP = torch.empty(wl.P, dtype=torch.int64, device=dev)
    nbP = L.lograst_frustum_scratch_bytes(wl.P)
    scratchP = torch.empty(nbP, dtype=torch.uint8, device=dev)
    t_flat = events(lambda: _lib.check(L.lograst_frustum_select(
        wl.P, wl.P, p(g.xyz), None, p(proj), 0.5, None, None, None, p(flagP), p(posP), None, None, None, None, None,
        p(scratchP), nbP, stream)))
    cnt = ctypes.c_uint32(0)
    _lib.check(L.lograst_frustum_read(p(scratchP), ctypes.byref(cnt), stream))
    bytes_flat = wl.P * (12 + 1 + 1) + int(cnt.value) * 8
    weight = prepare.root_weight(rast, sel)
    prepare.lod_select(tree, g, sel, weight, rast, m.current_depth, True, m.current_depth)      # caches the depth hint
    sel = prepare.frustum_select(g.xyz, proj, 0.5, rows=tree.root_index, raw=(g.scaling, g.rotation, g.opacity))
    roots_kept = tree.root_index.long()[sel.flag.clone().index_put_((sel.pos,), weight > 1e-8)]
    t_select = wall(lambda: [prepare.lod_select(tree, g, sel, weight, rast, m.current_depth, True, m.current_depth) for _ in range(10)]) / 10
    t_traverse = wall(lambda: [lod.traverse(tree, g, roots_kept, rast, max_depth=m.current_depth) for _ in range(10)]) / 10
    index = g.visibility_flag["index"]
    vis = (torch.rand(index.shape[0], device=dev, generator=gen) < 0.8)
    args = prepare._clamp_inputs(m, index, vis)
    t_clamp = events(lambda: prepare._clamp_launch(*args))
    msel = int(vis.sum())
    bytes_clamp = int(index.shape[0]) * 9 + msel * (24 + 8)
    nbytes = 1 << 30
    src, dst = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
    t_copy = events(lambda: _lib.check(L.lograst_stream_copy(p(dst), p(src), nbytes, 0, stream)))
    gbs = lambda b, ms: b / ms / 1e6
    out["kernels"] = {
        "frustum_select_roots": {"ms": t_roots, "bytes": bytes_roots, "GBps": gbs(bytes_roots, t_roots), "entries": Rn, "kept": K},
        "frustum_select_all_points": {"ms": t_flat, "bytes": bytes_flat, "GBps": gbs(bytes_flat, t_flat), "entries": wl.P,
                                      "kept": int(cnt.value)},
        "lod_select_with_readback": {"ms": t_select, "selected": int(index.shape[0] + g.visibility_flag["index_node"].shape[0])},
        "lod_traverse_with_readback": {"ms": t_traverse},
        "clamp_scale": {"ms": t_clamp, "bytes": bytes_clamp, "GBps": gbs(bytes_clamp, t_clamp), "rows": int(index.shape[0]),
                        "selected": msel},
        "stream_copy_1GiB": {"ms": t_copy, "bytes": 2 * nbytes, "GBps": gbs(2 * nbytes, t_copy)}}
    out["stats"] = {k: {str(a): b for a, b in v.items()} for k, v in prepare.stats().items()}

    print(f"| stage (per view, {wl.P} points, {len(views)} views x {rounds} rounds) | drop-in median (min - max) ms | torch-on-device median (min - max) ms |")
    print("|---|---|---|")
    for k in ("prepare", "clamp_scale"):
        d, t = out["wall"]["device"][k], out["wall"]["torch"][k]
        print(f"| {k} | {d['median_ms']:.3f} ({d['min_ms']:.3f} - {d['max_ms']:.3f}) | {t['median_ms']:.3f} ({t['min_ms']:.3f} - {t['max_ms']:.3f}) |")
    for k, v in out["kernels"].items():
        print(k, {a: (round(b, 4) if isinstance(b, float) else b) for a, b in v.items()})
    path = os.environ.get("BENCH_PREPARE_OUT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Generates tests/golden/prepare_*.npz by RUNNING the reference's own per-view preparation on the CPU (build container
only: needs the reference checkout; the fixtures are committed and travel to the GPU box).

What is pinned: LoG.prepare, Gaussian.prepare, LoG.clamp_scale and LoG.step -- unmodified -- on the reference's LoG model
set up as tests/test_log_plumbing_cpu.py::_log_model does (a two-level tree grown through its own densification plumbing),
with the oracle backend below the rasterizer boundary.  One fixture holds one model and, per view and per mode
(opt_all_levels on; off with current_depth below the tree's depth, so the depth limit leaves a frontier): the camera, the
in-range flag of the roots, the root render's point_weight, root_flag, index and index_node; the flat model's flag over
all points; and per step: index, flag_vis, the clamped rows (radius3d_min / radius3d_max drawn so that both bounds bind,
some rows with min > max).  The optimizer of LoG.step is a stand-in that does nothing, so the step's only change to
`scaling` is the clamp.

Asserted here, redrawing the seed otherwise: no root (no point, for the flat model) is undecided (prepare_ref.frustum); no
in-range root has point_weight in [0.5e-8, 2e-8]; at least 5 % of the roots are out of range and at least 5 % of the
in-range roots are rejected by weight in the ordinary views; leaf and node lists are non-empty; one view sees no root and
one sees all of them; the restatement reproduces every flag and list; rows outside a step's selection stay bit for bit.

    python tests/golden/make_golden_prepare.py
"""
import math
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("LOG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (REF, ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import prepare_ref as PR                                     # noqa: E402
from make_golden_densify import _Cfg, cpu_shims              # noqa: E402
from make_golden_lod import reference_env, save_lzma         # noqa: E402

MODES = (("all", True, 2), ("depth1", False, 1))             # (name, opt_all_levels, current_depth)


class _Redraw(Exception):
    pass


def log_model(seed, n, split_prob=0.3):
    """_log_model of tests/test_log_plumbing_cpu.py with fewer splits (the fixture's size) and random raw rotations and
    opacities (the reference initialises both to constants)."""
    from LoG.model.level_of_gaussian import LoG
    from log_amd import scenes
    sc = scenes.random_scene(n, seed=seed, smax=0.08)
    cfg_opt = _Cfg(optimize_keys=["xyz", "colors", "scaling", "opacity", "rotation", "shs"], opt_all_levels=True,
                   lr_dict={"xyz": 0.00016, "xyz_final": 0.0000016, "colors": 0.0025, "shs": 0.000125, "scaling": 0.005,
                            "opacity": 0.05, "rotation": 0.001, "max_steps": 300})
    torch.manual_seed(seed)
    model = LoG(gaussian=_Cfg(init_ply=dict(filename={"xyz": sc["xyz"], "colors": sc["colors"]}, scale3d=1.0,
                                            init_opacity=0.3), sh_degree=1, xyz_scale=1.0),
                tree=_Cfg(max_child=4, max_level=30), optimizer=cfg_opt, densify_and_remove=_Cfg())
    model.base_iter = 1
    model.set_stage("tree")
    model.training_setup()
    model.upgrade_tree()
    gen = torch.Generator().manual_seed(seed + 1)
    for level in range(2):
        leaf = (model.tree.node_index == -1) & (model.tree.depth == level)
        flag_split = leaf & (torch.rand(leaf.shape[0], generator=gen) < split_prob)
        flag_remove = torch.zeros_like(flag_split)
        flag_split, flag_remove = model.tree.split_and_remove(flag_split, flag_remove)
        model.splitter.split_and_remove(model.gaussian, model.optimizer, flag_split, flag_remove, remove_split=False)
        model.splitter.split_and_remove_other(model.counter, ["create_steps", "radius3d_min", "radius3d_max"],
                                              flag_split, flag_remove, remove_split=False)
        model.counter.reset(model.num_points)
    p = model.num_points
    model.gaussian.rotation.set_(torch.randn(p, 4, generator=gen))
    model.gaussian.opacity.set_(torch.randn(p, 1, generator=gen) + 1.0)
    model.train()
    return model


def cameras():
    """(name, camera dict, ordinary) -- orbit cameras near the unit cube at 160x120, one at 1920x1080, one that looks at the
    whole cloud from a distance (sees all roots) and one that looks away from it (sees none)."""
    from log_amd import scenes
    small = scenes.orbit_cameras(8, radius=1.1, W=160, H=120, focal=1.1 * 160)
    out = [(f"s{i}", small[i], True) for i in (0, 3, 6)]
    out.append(("hd", scenes.orbit_cameras(8, radius=1.2, W=1920, H=1080, focal=1.1 * 1920)[2], True))
    out.append(("allroots", scenes.orbit_cameras(1, radius=1.1, center=(5.0, 0.0, 0.0), W=160, H=120, focal=176.0)[0], False))
    out.append(("none", scenes.orbit_cameras(1, radius=1.1, center=(5.0, 0.0, 0.0), W=160, H=120, focal=176.0,
                                             start_deg=180.0)[0], False))
    return out


def rasterizer_for(cam):
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=math.tan(cam["FoVx"] * 0.5),
        tanfovy=math.tan(cam["FoVy"] * 0.5), bg=torch.ones(3), scale_modifier=1.0,
        viewmatrix=torch.tensor(cam["world_view_transform"]), projmatrix=torch.tensor(cam["full_proj_transform"]),
        sh_degree=0, campos=torch.tensor(cam["camera_center"]), prefiltered=False, debug=False)
    return GaussianRasterizer(raster_settings=rs)


def run_view(model, name, cam, ordinary, out):
    from LoG.model.level_of_gaussian import Gaussian
    g, tree = model.gaussian, model.tree
    camera = {"full_proj_transform": torch.tensor(cam["full_proj_transform"])}
    rast = rasterizer_for(cam)
    roots = tree.root_index.long()
    in_range = g._visible_flag_by_camera(g.xyz[roots].detach(), camera, padding=0.5)[0].numpy()
    want, und = PR.frustum(g.xyz.numpy(), cam["full_proj_transform"], 0.5, rows=roots.numpy())
    if und.any():
        raise _Redraw(f"view {name}: {int(und.sum())} undecided roots")
    assert np.array_equal(want, in_range), name
    frac = in_range.mean()
    if ordinary and not 0.05 <= frac <= 0.95:
        raise _Redraw(f"view {name}: {frac:.2f} of the roots in range")
    if name == "allroots":
        assert in_range.all()
    if name == "none":
        assert not in_range.any()
    out[f"{name}_proj"] = np.asarray(cam["full_proj_transform"], np.float32)
    out[f"{name}_view"] = np.asarray(cam["world_view_transform"], np.float32)
    out[f"{name}_wh"] = np.array([cam["image_width"], cam["image_height"]], np.int32)
    out[f"{name}_tanfov"] = np.array([rast.raster_settings.tanfovx, rast.raster_settings.tanfovy], np.float64)
    out[f"{name}_in_range"] = np.packbits(in_range)
    # the flat model's test over all points (Gaussian.prepare, padding 0.5)
    Gaussian.prepare(g, rast, camera)
    flat, und = PR.frustum(g.xyz.numpy(), cam["full_proj_transform"], 0.5)
    if und.any():
        raise _Redraw(f"view {name}: {int(und.sum())} undecided points")
    assert np.array_equal(g.visibility_flag["flag"].numpy(), flat)
    assert np.array_equal(g.visibility_flag["index"].numpy(), np.nonzero(flat)[0])
    assert g.visibility_flag["index"].dtype == torch.int64
    out[f"{name}_flat"] = np.packbits(flat)
    seen = {}
    render = model.render_to_check

    def spy(*a, **k):
        seen["w"] = render(*a, **k)
        return seen["w"]
    model.render_to_check = spy
    try:
        for mode, all_levels, current_depth in MODES:
            model.optimizer_cfg["opt_all_levels"] = all_levels
            model.current_depth = current_depth
            seen.clear()
            model.prepare(rast, camera)
            vf = g.visibility_flag
            w = seen["w"].numpy().astype(np.float32)
            if ((w >= 0.5e-8) & (w <= 2e-8)).any():
                raise _Redraw(f"view {name}: a point_weight next to 1e-8")
            root_flag = vf["root_flag"].numpy()
            assert vf["root_flag"].dtype == torch.bool and vf["index"].dtype == torch.int64
            assert np.array_equal(PR.root_filter(in_range, w), root_flag)
            rejected = 1.0 - root_flag.sum() / max(1, in_range.sum())
            if ordinary and rejected < 0.05:
                raise _Redraw(f"view {name}: {rejected:.3f} of the in-range roots rejected by weight")
            leaf, node = vf["index"].numpy(), vf["index_node"].numpy()
            if ordinary and (leaf.size == 0 or node.size == 0):
                raise _Redraw(f"view {name} / {mode}: an empty list")
            index_all = tree.traverse(g, roots[vf["root_flag"]], rast, max_depth=current_depth).numpy()
            wl, wn = PR.partition(index_all, tree.node_index.numpy(), tree.depth.numpy(), all_levels, current_depth)
            assert np.array_equal(wl, leaf) and np.array_equal(wn, node)
            if mode == "depth1" and ordinary:
                assert (tree.node_index.numpy()[leaf] >= 0).any(), "the depth limit left no frontier"
            if mode == "all":
                out[f"{name}_weight"] = w
            else:
                assert np.array_equal(out[f"{name}_weight"], w)
            out[f"{name}_{mode}_root_flag"] = np.packbits(root_flag)
            out[f"{name}_{mode}_index"] = leaf.astype(np.int32)
            out[f"{name}_{mode}_index_node"] = node.astype(np.int32)
            print(f"  view {name:8s} {mode:6s} in range {frac:.2f} rejected {rejected:.2f} leaf {leaf.size} node {node.size}")
    finally:
        del model.render_to_check
    return leaf


class _NoOptimizer(torch.nn.Module):
    """What LoG.step touches of its SparseOptimizer (an nn.Module child of the model), doing nothing."""
    xyz_lr, global_steps = 0.0, 0

    def step(self, *args, **kwargs):
        pass


def run_steps(model, seed, index_view, out):
    """LoG.step (with an optimizer that does nothing) on a view's list with a random flag_vis, then LoG.clamp_scale on all
    rows as update_init_stage calls it."""
    from LoG.model.level_of_gaussian import LoG
    g = model.gaussian
    p = model.num_points
    rng = np.random.default_rng([seed, 0xC1])
    mid = g.scaling.numpy().astype(np.float64).mean(axis=1)
    rmin = np.exp(mid + 0.3 * rng.standard_normal(p)).astype(np.float32)
    rmax = (rmin * np.exp(rng.uniform(-0.2, 1.0, p))).astype(np.float32)
    assert 0.02 < (rmin > rmax).mean() < 0.5
    model.counter.radius3d_min.set_(torch.from_numpy(rmin.copy()))
    model.counter.radius3d_max.set_(torch.from_numpy(rmax.copy()))
    out["radius3d_min"], out["radius3d_max"] = rmin, rmax
    before = g.scaling.numpy().copy()
    stub = _NoOptimizer()
    real = model.optimizer
    cases = {"step": (torch.from_numpy(index_view.astype(np.int64)), True), "init": (torch.arange(p), False)}
    worst = 0.0
    for name, (index, with_flag) in cases.items():
        g.scaling.set_(torch.from_numpy(before.copy()))
        flag = None
        if with_flag:
            flag = rng.random(index.shape[0]) < 0.7
            g.visibility_flag = {"params": {}, "index": index, "flag_vis": torch.from_numpy(flag),
                                 "index_node": torch.zeros(0, dtype=torch.int64)}
            model.optimizer = stub
            try:
                LoG.step(model)
            finally:
                model.optimizer = real
            out[f"{name}_flag_vis"] = np.packbits(flag)
        else:
            LoG.clamp_scale(model, index)
        after = g.scaling.numpy().copy()
        rows, want = PR.clamp_scale(before, index.numpy(), flag, rmin, rmax)
        untouched = np.ones(p, bool)
        untouched[rows] = False
        assert np.array_equal(after[untouched], before[untouched]), "rows outside the selection changed"
        err = PR.ulp_error(after[rows], want)
        worst = max(worst, float(err.max()))
        low = (after[rows] > before[rows]).mean()
        high = (after[rows] < before[rows]).mean()
        assert low > 0.02 and high > 0.02, "a bound that does not bind"
        out[f"{name}_index"] = index.numpy().astype(np.int32)
        out[f"{name}_after"] = after[index.numpy()]
        print(f"  {name}: {rows.size} rows, raised {low:.2f} lowered {high:.2f}, reference vs float64 {err.max():.2f} ulp")
    g.scaling.set_(torch.from_numpy(before.copy()))
    assert worst <= 2.0, worst
    out["meta_clamp_ulp"] = np.float64(worst)


def case(name, seed, n):
    model = log_model(seed, n)
    g, tree = model.gaussian, model.tree
    assert int(tree.depth.max()) == 2 and tree.num_nodes > 0
    out = {"meta_seed": np.int64(seed), "meta_views": np.array([c[0] for c in cameras()]),
           "meta_modes": np.array([m[0] for m in MODES]), "meta_all_levels": np.array([m[1] for m in MODES]),
           "meta_current_depth": np.array([m[2] for m in MODES], np.int32), "max_level": np.int32(tree.max_level),
           "min_resolution_pixel": np.float64(tree.min_resolution_pixel)}
    for k in ("xyz", "scaling", "rotation", "opacity"):
        out[k] = getattr(g, k).detach().numpy().copy()
    for k in ("node_index", "tree", "depth", "root_index"):
        out[k] = getattr(tree, k).numpy().copy()
    assert tree.root_index.dtype == torch.int32
    leaf = None
    for vname, cam, ordinary in cameras():
        got = run_view(model, vname, cam, ordinary, out)
        if vname == "s0":
            leaf = got
    model.optimizer_cfg["opt_all_levels"] = True
    run_steps(model, seed, leaf, out)
    path = os.path.join(HERE, f"prepare_{name}.npz")
    save_lzma(path, out)
    print(f"{name}: seed {seed}, {model.num_points} points, {tree.root_index.shape[0]} roots, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


def main():
    reference_env()
    cpu_shims()
    for name, seed, n in (("tree", 61, 2500),):
        for attempt in range(20):
            try:
                case(name, seed + 1000 * attempt, n)
                break
            except _Redraw as why:
                print(name, "seed", seed + 1000 * attempt, "redrawn:", why)
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")


if __name__ == "__main__":
    main()

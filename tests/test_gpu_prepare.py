"""The device view preparation (log_amd/prepare.py -> log_amd/csrc/prepare.hip, lod.hip) against the fixtures recorded from
the reference's own LoG.prepare / Gaussian.prepare / LoG.clamp_scale / LoG.step (tests/golden/prepare_*.npz) and the numpy
restatement tests/prepare_ref.py (held to those fixtures by tests/test_prepare_cpu.py).  No test here reads the reference
tree: the drop-ins run on stand-in objects that carry the attributes the reference's LoG / GaussianPoint / TensorTree /
Counter carry.

Flags and index lists must match exactly (the fixtures and the generated inputs hold no row that fp32 could decide either
way: prepare_ref.frustum's `undecided`).  Clamped elements: within 2 fp32 ulp of the float64 restatement (logf is
documented at <= 1 ulp, the rounding of the float64 bound to fp32 is another half), every other row bit for bit."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prepare_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_FX = {}
_ACT = types.SimpleNamespace(scaling_activation=torch.exp, scaling_inverse_activation=torch.log,
                             opacity_activation=torch.sigmoid, rotation_activation=torch.nn.functional.normalize)


def fixture(name="tree"):
    if name not in _FX:
        _FX[name] = {k: v for k, v in PR.load(name).items()}
    return _FX[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def stand_in(fx, all_levels=True, current_depth=2):
    """A LoG model's attributes, as far as the drop-ins read them."""
    from log_amd import prepare
    g = types.SimpleNamespace(xyz=dev(fx["xyz"]), scaling=dev(fx["scaling"]), rotation=dev(fx["rotation"]),
                              opacity=dev(fx["opacity"]), activation=_ACT, visibility_flag=None)
    g.prepare = lambda rasterizer, camera: prepare.gaussian_prepare(g, rasterizer, camera)
    tree = types.SimpleNamespace(node_index=dev(fx["node_index"]), tree=dev(fx["tree"]), depth=dev(fx["depth"]),
                                 root_index=dev(fx["root_index"]), max_level=int(fx["max_level"]),
                                 min_resolution_pixel=float(fx["min_resolution_pixel"]), num_nodes=int(fx["tree"].shape[0]))
    counter = types.SimpleNamespace(radius3d_min=dev(fx["radius3d_min"]), radius3d_max=dev(fx["radius3d_max"]))
    opt = types.SimpleNamespace(step=lambda *a, **k: None, xyz_lr=1e-4, global_steps=0)
    return types.SimpleNamespace(gaussian=g, tree=tree, counter=counter, optimizer=opt, current_depth=current_depth,
                                 optimizer_cfg=_Cfg(opt_all_levels=all_levels), fix_parent=True, base_iter=1,
                                 use_view_correction=False)


def camera_of(fx, v):
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    W, H = (int(x) for x in fx[f"{v}_wh"])
    tfx, tfy = (float(x) for x in fx[f"{v}_tanfov"])
    view = fx[f"{v}_view"]
    campos = np.linalg.inv(view.astype(np.float64))[3, :3].astype(np.float32)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tfx, tanfovy=tfy, bg=torch.ones(3, device=DEV), scale_modifier=1.0,
        viewmatrix=dev(view), projmatrix=dev(fx[f"{v}_proj"]), sh_degree=0, campos=dev(campos), prefiltered=False, debug=False)
    return GaussianRasterizer(raster_settings=rs), {"full_proj_transform": dev(fx[f"{v}_proj"])}


def cpu(t):
    return t.detach().cpu().numpy()


# ---- kernel 1 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 1024 * 1025 + 1])
def test_frustum_select_sizes(n):
    """Every size at which the compaction takes another path: partial waves and chunks, more than one chunk, and more
    than 1024 chunks (the second round of the chunk scan).  Generated rows are all decided, so none is skipped."""
    from log_amd import prepare
    fx = fixture()
    for pad, v in ((0.5, "s0"), (0.05, "s3"))[:1 if n > 10 ** 6 else 2]:      # the largest size once: its float64 twin takes seconds
        proj = fx[f"{v}_proj"]
        xyz, want = PR.planted_points(np.random.default_rng([n, int(pad * 100)]), n, proj, pad)
        sel = prepare.frustum_select(dev(xyz).reshape(n, 3), dev(proj), pad)
        assert sel.flag.dtype == torch.bool and sel.pos.dtype == torch.int64
        assert np.array_equal(cpu(sel.flag), want), (n, pad)
        assert sel.count == int(want.sum()) and np.array_equal(cpu(sel.pos), np.nonzero(want)[0]), (n, pad)
        if n > 100:
            assert 0 < sel.count < n


def _fp32_flags(xyz, hw_is_z, pad):
    """The kernel's op sequence in numpy fp32, for projections whose dot products are exact (identity; hw = z)."""
    x = xyz.astype(np.float32)
    with np.errstate(all="ignore"):
        hw = x[:, 2] if hw_is_z else np.ones(len(x), np.float32)
        pw = np.float32(1.0) / (hw + np.float32(1e-7))
        px, py, d = x[:, 0] * pw, x[:, 1] * pw, (x[:, 2] * np.float32(0.5) if hw_is_z else x[:, 2]) * pw
        lo, hi = np.float32(-1.0 - pad), np.float32(1.0 + pad)
        return (d > 0) & (d < 1) & (px > lo) & (px < hi) & (py > lo) & (py < hi), px, d


def test_frustum_select_planted_rows():
    """hw = -1e-7 (division by zero), NaN / inf coordinates, depth exactly 0 and exactly 1, |x| exactly 1 + padding: strict
    comparisons, False for everything that is not finite.  The projections make every dot product exact, so the kernel's
    fp32 result is known bit for bit."""
    from log_amd import prepare
    pad = 0.5
    ident = np.eye(4, dtype=np.float32)
    f = np.float32
    step = lambda c, k: f(c) + f(k) * np.spacing(f(c))
    rows = [[0, 0, 0.5], [0, 0, 0.0], [0, 0, -0.0], [np.nan, 0, 0.5], [0, np.nan, 0.5], [0, 0, np.nan], [np.inf, 0, 0.5],
            [0, -np.inf, 0.5], [0, 0, np.inf]]
    rows += [[0, 0, step(1.0, k)] for k in range(-3, 4)]
    rows += [[s * step(1.5, k), 0, 0.5] for k in range(-3, 4) for s in (1, -1)]
    rows += [[0, s * step(1.5, k), 0.5] for k in range(-3, 4) for s in (1, -1)]
    xyz = np.array(rows, np.float32)
    want, px, d = _fp32_flags(xyz, False, pad)
    assert (d == 1.0).any() and (d == 0.0).any() and (np.abs(px) == 1.5).any()       # the exact boundaries are among the rows
    assert want[0] and not want[1:9].any()
    sel = prepare.frustum_select(dev(xyz), dev(ident), pad)
    assert np.array_equal(cpu(sel.flag), want) and np.array_equal(cpu(sel.pos), np.nonzero(want)[0])
    persp = np.eye(4, dtype=np.float32)
    persp[3, 3], persp[2, 3], persp[2, 2] = 0.0, 1.0, 0.5                            # hw = z, hz = z / 2
    xyz = np.array([[0.1, 0.1, 0.5], [0, 0, -1e-7], [0.1, 0.1, -1e-7], [0, 0, 0], [0.8, 0, 0.5], [0.1, 0.1, -0.5]], np.float32)
    want, _, _ = _fp32_flags(xyz, True, pad)
    assert list(want) == [True, False, False, False, False, True]     # the last: behind the camera, kept as the reference keeps it
    sel = prepare.frustum_select(dev(xyz), dev(persp), pad)
    assert np.array_equal(cpu(sel.flag), want) and sel.count == 2


def test_frustum_select_activations_and_row_list():
    """The kept entries' activated parameters are bit for bit what log_amd.get_all's gather kernel writes for the same
    rows; with a row list (int32, as TensorTree keeps root_index) and without one; rows outside the model are not kept."""
    from log_amd import prepare, rasterizer as R
    fx = fixture()
    m = stand_in(fx)
    g = m.gaussian
    P = g.xyz.shape[0]
    proj = dev(fx["s0_proj"])
    raw = (g.scaling, g.rotation, g.opacity)
    rng = np.random.default_rng(5)
    rows_np = rng.permutation(P)[:3000].astype(np.int32)
    rows_np[[7, 1500]] = [-1, P]                               # invalid rows: flag 0, never read
    for rows in (None, dev(rows_np)):
        sel = prepare.frustum_select(g.xyz, proj, 0.5, rows=rows, raw=raw)
        want, und = PR.frustum(fx["xyz"], fx["s0_proj"], 0.5, rows=None if rows is None else np.clip(rows_np, 0, P - 1))
        assert not und.any()
        if rows is not None:
            want[[7, 1500]] = False
        assert np.array_equal(cpu(sel.flag), want) and sel.count > 100
        pos = np.nonzero(want)[0]
        assert np.array_equal(cpu(sel.pos), pos)
        index = torch.from_numpy(pos if rows is None else rows_np[pos].astype(np.int64)).to(DEV)
        if rows is not None:
            assert sel.rows.dtype == torch.int64 and torch.equal(sel.rows, index)
        bufs = {"xyz": g.xyz, "scaling": g.scaling, "opacity": g.opacity, "rotation": g.rotation,
                "colors": torch.zeros_like(g.xyz)}
        _, act = R._backend.gather_activate(index, bufs, 0, None)
        for k in ("xyz", "scaling", "rotation", "opacity"):
            got, ref = getattr(sel, k), act[k]
            assert got.shape == ref.shape and got.dtype == torch.float32, (k, got.shape, ref.shape)
            assert torch.equal(got.view(torch.int32), ref.contiguous().view(torch.int32)), k


def test_gaussian_prepare_flat_model():
    from log_amd import prepare
    fx = fixture()
    m = stand_in(fx)
    m.tree.num_nodes = 0                                        # LoG.prepare hands a model without a tree to Gaussian.prepare
    P = fx["xyz"].shape[0]
    for v in PR.views(fx):
        rast, camera = camera_of(fx, v)
        prepare.log_prepare(m, rast, camera)
        vf = m.gaussian.visibility_flag
        want = PR.bits(fx, f"{v}_flat", P)
        assert set(vf) == {"flag", "index"} and vf["flag"].dtype == torch.bool and vf["index"].dtype == torch.int64
        assert np.array_equal(cpu(vf["flag"]), want) and np.array_equal(cpu(vf["index"]), np.nonzero(want)[0]), v


# ---- kernel 2 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", ["s0", "s3", "s6", "hd", "allroots", "none"])
def test_log_prepare_reproduces_fixture_views(v):
    """Every fixture view end to end through the drop-in (frustum test, root render on the device, root filter, traversal,
    partition): root_flag, index and index_node exactly as the reference left them, in both modes; and the same lists as
    log_amd.lod.traverse plus torch masks on the device."""
    from log_amd import lod, prepare
    fx = fixture()
    R = fx["root_index"].shape[0]
    rast, camera = camera_of(fx, v)
    for mode, all_levels, current_depth in PR.modes(fx):
        m = stand_in(fx, all_levels, current_depth)
        prepare.log_prepare(m, rast, camera)
        vf = m.gaussian.visibility_flag
        assert set(vf) == {"root_flag", "index", "index_node"}
        assert vf["root_flag"].dtype == torch.bool and vf["index"].dtype == torch.int64 and vf["index_node"].dtype == torch.int64
        assert np.array_equal(cpu(vf["root_flag"]), PR.bits(fx, f"{v}_{mode}_root_flag", R)), (v, mode)
        assert np.array_equal(cpu(vf["index"]), fx[f"{v}_{mode}_index"]), (v, mode)
        assert np.array_equal(cpu(vf["index_node"]), fx[f"{v}_{mode}_index_node"]), (v, mode)
        roots = m.tree.root_index.long()[vf["root_flag"]]
        index_all = lod.traverse(m.tree, m.gaussian, roots, rast, max_depth=current_depth)
        if all_levels:
            leaf = (m.tree.node_index[index_all] == -1) & (m.tree.depth[index_all] > 0)
        else:
            leaf = m.tree.depth[index_all] == current_depth
        assert torch.equal(vf["index"], index_all[leaf]) and torch.equal(vf["index_node"], index_all[~leaf])


def _roots_selection(m, fx, v="allroots"):
    from log_amd import prepare
    g = m.gaussian
    return prepare.frustum_select(g.xyz, dev(fx[f"{v}_proj"]), 0.5, rows=m.tree.root_index,
                                  raw=(g.scaling, g.rotation, g.opacity))


def test_lod_select_partition_edges():
    """All-leaf, all-node and empty partitions, every root rejected, counts that cross chunk boundaries, and a stale depth
    hint -- lograst_lod_select against the restatement's partition of log_amd.lod.traverse's list."""
    from log_amd import lod, prepare
    fx = fixture()
    rast, _ = camera_of(fx, "allroots")
    m = stand_in(fx)
    sel = _roots_selection(m, fx)
    assert sel.count == fx["root_index"].shape[0]
    full = cpu(lod.traverse(m.tree, m.gaussian, sel.rows, rast, max_depth=2))
    assert full.shape[0] > 2 * 1024                            # the lists cross chunk boundaries
    ni, depth = fx["node_index"], fx["depth"]
    # (max_depth, opt_all_levels, current_depth)
    for max_depth, all_levels, cur in ((2, True, 2), (2, False, 2), (2, False, 1), (2, False, 99), (2, False, -1),
                                       (0, False, 0), (1, True, 1), (1, False, 1)):
        index_all = full if max_depth == 2 else cpu(lod.traverse(m.tree, m.gaussian, sel.rows, rast, max_depth=max_depth))
        flag, leaf, node = prepare.lod_select(m.tree, m.gaussian, sel, None, rast, max_depth, all_levels, cur)
        wl, wn = PR.partition(index_all, ni, depth, all_levels, cur)
        assert np.array_equal(cpu(leaf), wl) and np.array_equal(cpu(node), wn), (max_depth, all_levels, cur)
        assert bool(flag.all())
        if cur in (99, -1):
            assert wl.size == 0 and wn.size == index_all.size          # all node
        if max_depth == 0:
            assert wn.size == 0 and wl.size == sel.count               # all leaf: the roots, at depth 0
    # every root rejected by weight: the flag is cleared, both lists are empty
    zero = torch.zeros(sel.count, device=DEV)
    flag, leaf, node = prepare.lod_select(m.tree, m.gaussian, sel, zero, rast, 2, True, 2)
    assert not bool(flag.any()) and leaf.numel() == 0 and node.numel() == 0
    # a weight pattern: NaN and 1e-8 itself are rejected (the reference keeps `point_weight > 1e-8`)
    sel = _roots_selection(m, fx)
    w = np.full(sel.count, 1.0, np.float32)
    w[::3], w[1::7], w[5::11] = 0.0, np.nan, 1e-8
    flag, leaf, node = prepare.lod_select(m.tree, m.gaussian, sel, dev(w), rast, 2, True, 2)
    want_flag = PR.root_filter(np.ones(sel.count, bool), w)
    assert np.array_equal(cpu(flag), want_flag) and not want_flag[5] and not want_flag[1]
    index_all = cpu(lod.traverse(m.tree, m.gaussian, m.tree.root_index.long()[flag], rast, max_depth=2))
    wl, wn = PR.partition(index_all, ni, depth, True, 2)
    assert np.array_equal(cpu(leaf), wl) and np.array_equal(cpu(node), wn)
    # no root at all
    none = _roots_selection(m, fx, "none")
    assert none.count == 0
    flag, leaf, node = prepare.lod_select(m.tree, m.gaussian, none, None, rast, 2, True, 2)
    assert leaf.numel() == 0 and node.numel() == 0 and not bool(flag.any())
    # a stale depth hint (the tree grew since it was cached): detected on the device, the selection repeated in full
    m = stand_in(fx)
    m.tree.min_resolution_pixel = 0.5                          # every node is expanded: level 1 leaves a frontier behind
    sel = _roots_selection(m, fx)
    deep = cpu(lod.traverse(m.tree, m.gaussian, sel.rows, rast, max_depth=2))
    assert (ni[deep] == -1).all() and (depth[deep] == 2).any()
    key = (m.tree.depth.data_ptr(), int(m.tree.depth.numel()))
    assert m.tree._lograst_depth == (key, 2)
    m.tree._lograst_depth = (key, 1)
    prepare.reset_stats()
    flag, leaf, node = prepare.lod_select(m.tree, m.gaussian, sel, None, rast, 2, True, 2)
    wl, wn = PR.partition(deep, ni, depth, True, 2)
    assert np.array_equal(cpu(leaf), wl) and np.array_equal(cpu(node), wn)
    assert prepare.stats()["readbacks"] == {"log_prepare": 2}          # the short try and the full one


# ---- kernel 3 ------------------------------------------------------------------------------------------------------

def _clamp_case(m_rows, with_flag, seed):
    rng = np.random.default_rng([seed, m_rows])
    P = m_rows + 64
    scaling = rng.normal(-3.0, 1.0, (P, 3)).astype(np.float32)
    rmin = np.exp(rng.normal(-3.2, 0.5, P)).astype(np.float32)
    rmax = (rmin * np.exp(rng.uniform(-0.3, 1.0, P))).astype(np.float32)          # some rows with min > max
    index = rng.permutation(P)[:m_rows].astype(np.int64)
    if m_rows >= 255:
        k = index[:40]
        scaling[k[0:4]] = np.nan
        rmin[k[4:8]], rmax[k[8:12]] = np.nan, np.nan
        rmin[k[12:16]], rmax[k[16:20]] = 0.0, 0.0                                  # log -> -inf
        rmin[k[20:24]] = -1.0                                                      # log -> NaN
        scaling[k[24:28], 1] = np.inf
        rmax[k[28:32]] = np.inf
    flag = (rng.random(m_rows) < 0.6) if with_flag else None
    return scaling, rmin, rmax, index, flag


@pytest.mark.parametrize("with_flag", [False, True])
@pytest.mark.parametrize("m_rows", [0, 1, 255, 256, 257, 100003])
def test_clamp_scale_sizes(m_rows, with_flag):
    """lograst_clamp_scale through the drop-ins (LoG.clamp_scale: no flag; LoG.step: flag_vis): selected rows within 2 fp32
    ulp of the float64 restatement with torch.clamp's NaN and lo > hi rules, every other row bit for bit."""
    from log_amd import prepare
    scaling, rmin, rmax, index, flag = _clamp_case(m_rows, with_flag, 3)
    g = types.SimpleNamespace(xyz=torch.zeros(scaling.shape[0], 3, device=DEV), scaling=dev(scaling), activation=_ACT)
    model = types.SimpleNamespace(gaussian=g, counter=types.SimpleNamespace(radius3d_min=dev(rmin), radius3d_max=dev(rmax)),
                                  optimizer=types.SimpleNamespace(step=lambda *a, **k: None, xyz_lr=1e-4, global_steps=0),
                                  fix_parent=True, base_iter=1, use_view_correction=False)
    if with_flag:
        model.visibility_flag = {"params": {}, "index": dev(index), "flag_vis": dev(flag),
                                 "index_node": torch.zeros(0, dtype=torch.int64, device=DEV)}
        prepare.step(model)
        assert model.lr == 1e-4
    else:
        prepare.clamp_scale(model, dev(index))
    got = cpu(g.scaling)
    rows, want = PR.clamp_scale(scaling, index, flag, rmin, rmax)
    untouched = np.ones(scaling.shape[0], bool)
    untouched[rows] = False
    assert np.array_equal(got[untouched].view(np.uint32), scaling[untouched].view(np.uint32))
    err = PR.ulp_error(got[rows], want)
    print("clamp_scale", m_rows, with_flag, "worst error", float(err.max(initial=0.0)), "ulp")
    assert np.array_equal(np.isnan(got[rows]), np.isnan(want))
    assert (err <= 2.0).all()
    if m_rows >= 255:
        swapped = (rmin[rows] > rmax[rows]) & np.isfinite(want).all(axis=1)
        assert swapped.any() and (PR.ulp_error(got[rows][swapped], np.log(rmax[rows][swapped].astype(np.float64))[:, None]) <= 2).all()


def test_clamp_scale_reproduces_fixture_steps():
    from log_amd import prepare
    fx = fixture()
    for case in ("step", "init"):
        m = stand_in(fx)
        index = fx[f"{case}_index"].astype(np.int64)
        if f"{case}_flag_vis" in fx:
            flag = PR.bits(fx, f"{case}_flag_vis", index.shape[0])
            m.visibility_flag = {"params": {}, "index": dev(index), "flag_vis": dev(flag),
                                 "index_node": torch.zeros(0, dtype=torch.int64, device=DEV)}
            prepare.step(m)
        else:
            flag = None
            prepare.clamp_scale(m, dev(index))
        got = cpu(m.gaussian.scaling)
        rows, want = PR.clamp_scale(fx["scaling"], index, flag, fx["radius3d_min"], fx["radius3d_max"])
        untouched = np.ones(got.shape[0], bool)
        untouched[rows] = False
        assert np.array_equal(got[untouched], fx["scaling"][untouched])
        assert (PR.ulp_error(got[rows], want) <= 2.0).all()
        sel = np.ones(index.shape[0], bool) if flag is None else flag
        assert (PR.ulp_error(got[rows], fx[f"{case}_after"][sel].astype(np.float64)) <= 2.0).all()      # and next to the reference's


# ---- synchronisations ----------------------------------------------------------------------------------------------

def test_readbacks_and_no_other_synchronisation():
    """Two library read-backs per prepare, none per step or clamp; and nothing else in the drop-ins synchronises: they run
    under torch's sync debug mode (the library's own two reads are stream synchronisations torch does not see)."""
    from log_amd import prepare
    fx = fixture()
    rast, camera = camera_of(fx, "s0")
    m = stand_in(fx)
    prepare.log_prepare(m, rast, camera)                       # warm-up: caches the tree's depth (one read, once per tree)
    index = m.gaussian.visibility_flag["index"]
    flag_vis = torch.rand(index.shape[0], device=DEV) < 0.5
    prepare.reset_stats()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            prepare.log_prepare(m, rast, camera)
            m.visibility_flag = dict(m.gaussian.visibility_flag, params={}, flag_vis=flag_vis)
            prepare.step(m)
            prepare.clamp_scale(m, index)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    st = prepare.stats()
    assert st["calls"] == {"log_prepare": 3, "step": 3, "clamp_scale": 3} and st["fallbacks"] == {}
    assert st["readbacks"] == {"log_prepare": 6}
    assert np.array_equal(cpu(m.gaussian.visibility_flag["index"]), fx["s0_all_index"])
    assert math.isfinite(float(m.gaussian.scaling.sum()))

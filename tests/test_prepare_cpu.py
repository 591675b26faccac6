"""CPU checks of the device view preparation (log_amd/prepare.py, log_amd/csrc/prepare.hip): the numpy restatement
(tests/prepare_ref.py) against the fixtures recorded from the reference (tests/golden/prepare_*.npz), the new entry points
of the C ABI, their argument validation, and the drop-ins' fall-back to the reference's own methods."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import prepare_ref as PR
from test_log_plumbing_cpu import REF, _log_model, _run_steps, cpu_cuda_shims, log_env   # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lograst_frustum_scratch_bytes", "lograst_frustum_select", "lograst_frustum_read",
               "lograst_lod_select_scratch_bytes", "lograst_lod_select", "lograst_lod_select_read", "lograst_clamp_scale")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")


def test_fixture_set_is_complete():
    names = PR.fixture_names()
    assert "tree" in names
    for n in names:
        assert os.path.getsize(os.path.join(PR.GOLDEN, f"prepare_{n}.npz")) < 1_000_000
    fx = PR.load("tree")
    assert {"allroots", "none", "hd"} <= set(PR.views(fx)) and [m[1] for m in PR.modes(fx)] == [True, False]
    assert 2000 <= fx["root_index"].shape[0] <= 4000 and int(fx["depth"].max()) == 2
    assert fx["root_index"].dtype == np.int32 and fx["depth"].dtype == np.int8


@pytest.mark.parametrize("name", PR.fixture_names())
def test_restatement_reproduces_fixture_views(name, oracle_mod):
    """Flags and every index list exactly: the frustum test of the roots and of all points, the root filter from the
    recorded point_weight, the traversal (the oracle's) from the filtered roots and the leaf / node partition."""
    fx = PR.load(name)
    roots = fx["root_index"]
    R, P = roots.shape[0], fx["xyz"].shape[0]
    for v in PR.views(fx):
        flag, und = PR.frustum(fx["xyz"], fx[f"{v}_proj"], 0.5, rows=roots)
        assert not und.any() and np.array_equal(flag, PR.bits(fx, f"{v}_in_range", R)), v
        flat, und = PR.frustum(fx["xyz"], fx[f"{v}_proj"], 0.5)
        assert not und.any() and np.array_equal(flat, PR.bits(fx, f"{v}_flat", P)), v
        w = fx[f"{v}_weight"]
        assert w.shape == (int(flag.sum()),) and not ((w >= 0.5e-8) & (w <= 2e-8)).any()
        root_flag = PR.root_filter(flag, w)
        W, H = (int(x) for x in fx[f"{v}_wh"])
        tfx, tfy = (float(x) for x in fx[f"{v}_tanfov"])
        for mode, all_levels, current_depth in PR.modes(fx):
            assert np.array_equal(root_flag, PR.bits(fx, f"{v}_{mode}_root_flag", R)), (v, mode)
            index_all = oracle_mod.lod_traverse(fx["node_index"], fx["tree"], fx["xyz"], fx["scaling"], fx["rotation"],
                                                roots[root_flag].astype(np.int64), fx[f"{v}_proj"], fx[f"{v}_view"],
                                                W / (2 * tfx), H / (2 * tfy), tfx, tfy, float(fx["min_resolution_pixel"]),
                                                int(fx["max_level"]), current_depth)
            leaf, node = PR.partition(index_all, fx["node_index"], fx["depth"], all_levels, current_depth)
            assert np.array_equal(leaf, fx[f"{v}_{mode}_index"]) and np.array_equal(node, fx[f"{v}_{mode}_index_node"]), (v, mode)
    none, full = PR.bits(fx, "none_in_range", R), PR.bits(fx, "allroots_in_range", R)
    assert not none.any() and full.all()
    ordinary = [PR.bits(fx, f"{v}_in_range", R) for v in PR.views(fx) if v not in ("none", "allroots")]
    assert all(0.05 <= 1 - f.mean() for f in ordinary)


@pytest.mark.parametrize("name", PR.fixture_names())
def test_restatement_reproduces_fixture_steps(name):
    """Clamped elements within 2 fp32 ulp of the float64 result (torch's log and logf are documented at <= 1 ulp each);
    the fixture's generator asserted that every other row stayed bit for bit."""
    fx = PR.load(name)
    before, rmin, rmax = fx["scaling"], fx["radius3d_min"], fx["radius3d_max"]
    assert (rmin > rmax).any()
    worst = 0.0
    for case in ("step", "init"):
        index = fx[f"{case}_index"].astype(np.int64)
        flag = PR.bits(fx, f"{case}_flag_vis", index.shape[0]) if f"{case}_flag_vis" in fx else None
        rows, want = PR.clamp_scale(before, index, flag, rmin, rmax)
        after = fx[f"{case}_after"]
        sel = np.ones(index.shape[0], bool) if flag is None else flag
        err = PR.ulp_error(after[sel], want)
        worst = max(worst, float(err.max()))
        assert np.array_equal(after[~sel], before[index[~sel]])          # selected by index but not by flag: bit for bit
        assert (after[sel] > before[rows]).any() and (after[sel] < before[rows]).any()
        swapped = rmin[rows] > rmax[rows]
        assert swapped.any() and np.allclose(after[sel][swapped], np.log(rmax[rows][swapped].astype(np.float64))[:, None],
                                             rtol=0, atol=1e-5)      # lo > hi gives hi
    print(name, "worst clamp error of the reference against float64:", worst, "ulp")
    assert worst <= 2.0


def test_clamp_rules_are_torch_clamp_s():
    """NaN in the value, the lower or the upper bound (in that order) is the result; lo > hi gives hi."""
    nan = float("nan")
    x = np.array([0.5, nan, 0.5, 0.5, nan, 3.0, -3.0, 0.0, nan], np.float32)
    lo = np.array([0.0, 0.0, nan, 0.0, nan, 1.0, 1.0, 2.0, 2.0], np.float32)
    hi = np.array([1.0, 1.0, 1.0, nan, nan, 2.0, 2.0, 1.0, nan], np.float32)
    want = torch.clamp(torch.from_numpy(x), torch.from_numpy(lo), torch.from_numpy(hi)).numpy()
    got = PR.clamp(x, lo, hi).astype(np.float32)
    assert np.array_equal(got, want, equal_nan=True)
    assert got[7] == 1.0 and np.isnan(got[[1, 2, 3, 4, 8]]).all()


def test_frustum_restatement_edges():
    """Planted rows of the frustum test: hw = -1e-7 (a division by zero), NaN / inf coordinates, depth exactly 0 and 1,
    |x| = 1 + padding -- strict comparisons, False (and decided) for anything that is not finite."""
    proj = np.eye(4, dtype=np.float32)
    proj[3, 3], proj[2, 3], proj[2, 2] = 0.0, 1.0, 0.5    # h = (x, y, z / 2), hw = z: p = (x, y, z / 2) / (z + 1e-7)
    rows = np.array([[0.1, 0.1, 0.5], [np.nan, 0, 0.5], [0, np.inf, 0.5], [0, 0, -1e-7], [0.8, 0, 0.5]], np.float32)
    flag, und = PR.frustum(rows, proj, 0.5)
    assert list(flag) == [True, False, False, False, False] and not und.any()
    ident = np.eye(4, dtype=np.float32)               # hw = 1: p = xyz / (1 + 1e-7)
    s = 1.0 + PR.ADD
    edge = np.array([[0, 0, 0.0], [0, 0, s], [1.5 * s, 0, 0.5], [-1.5 * s, 0, 0.5], [0, 0, 0.5]], np.float64).astype(np.float32)
    flag, und = PR.frustum(edge, ident, 0.5)
    assert not flag[0] and flag[4]                    # depth exactly 0 fails the strict comparison
    assert und[1] and und[2] and und[3] and not und[4]      # on a boundary: fp32 may fall either way
    assert PR.bounds(0.05) == (float(np.float32(-1.05)), float(np.float32(1.05)))


def test_symbols_are_declared_exported_and_bound():
    from log_amd import _lib
    header = open(os.path.join(ROOT, "include", "lograst.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in _lib._SIGNATURES and name in _lib.EXPORTS, name
    assert _lib.lib().lograst_version() == 4


def test_argument_validation_needs_no_gpu():
    from log_amd import _lib
    L = _lib.lib()
    err = lambda: L.lograst_last_error().decode()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.lograst_frustum_scratch_bytes(0) >= 16
    assert L.lograst_frustum_scratch_bytes(2 ** 31 - 1) >= 16 + 4 * 2 ** 21
    fs = lambda n, P, rows, scratch, nbytes, act=(None,) * 3, outs=(None,) * 4, pad=0.5, xyz=p: L.lograst_frustum_select(
        n, P, xyz, rows, p, pad, *act, p, p, None, *outs, scratch, nbytes, None)
    assert fs(-1, 8, None, p, 4096) == -1 and "negative" in err()
    assert fs(9, 8, None, p, 4096) == -1 and "without a row list" in err()
    assert fs(8, 8, None, p, 8) == -1 and "scratch too small" in err()
    assert fs(8, 8, None, None, 4096) == -1 and "scratch too small" in err()
    assert fs(8, 8, None, p, 4096, xyz=None) == -1 and "NULL" in err()
    assert fs(8, 8, None, p, 4096, act=(p, p, None)) == -1 and "go together" in err()
    assert fs(8, 8, None, p, 4096, act=(p, p, p), outs=(p, p, None, p)) == -1 and "go together" in err()
    assert fs(8, 8, None, p, 4096, pad=float("nan")) == -1 and "NaN" in err()
    assert L.lograst_frustum_read(None, None, None) == -1 and "NULL" in err()
    need = L.lograst_lod_select_scratch_bytes(8, 2, 4, 64)
    assert need > L.lograst_lod_scratch_bytes(8, 2, 4) and need % 8 == 0
    sel = lambda **kw: L.lograst_lod_select(
        kw.get("P", 16), kw.get("nodes", 2), kw.get("mc", 4), p, p, kw.get("depth", p), p, p, p, p, kw.get("roots", 8),
        kw.get("weight", p), kw.get("pos", p), p, 8, p, p, 1.0, 1.0, 1.0, 1.0, 3.0, 2, 1, 2, p, 64, p, p, kw.get("scratch", p),
        kw.get("nbytes", 1 << 16), None)
    assert sel(P=-1) == -1 and "negative" in err()
    assert sel(mc=0) == -1 and "max_child" in err()
    assert sel(nodes=2 ** 30, nbytes=2 ** 40) == -1 and "tree too large" in err()
    assert sel(nbytes=need - 1) == -1 and "scratch too small" in err()
    assert sel(depth=None) == -1 and "NULL" in err()
    assert sel(pos=None) == -1 and "root_weight needs" in err()
    assert L.lograst_lod_select_read(p, None, None, None, None, None) == -1 and "NULL" in err()
    clamp = lambda m, P, index=p, scaling=p: L.lograst_clamp_scale(m, index, None, P, scaling, p, p, None)
    assert clamp(-1, 8) == -1 and "negative" in err()
    assert clamp(8, 8, index=None) == -1 and "NULL" in err()
    assert clamp(8, 8, scaling=None) == -1 and "NULL" in err()
    assert clamp(0, 8, index=None) == 0          # nothing to do is not an error, and touches no device


def _methods():
    from LoG.model.level_of_gaussian import Gaussian, LoG
    return (LoG.prepare, Gaussian.prepare, LoG.clamp_scale, LoG.step)


def _set_methods(saved):
    from LoG.model.level_of_gaussian import Gaussian, LoG
    LoG.prepare, Gaussian.prepare, LoG.clamp_scale, LoG.step = saved


@needs_reference
def test_dropins_fall_back_to_the_reference_on_cpu_tensors(cpu_cuda_shims, caplog):
    """Tensors that are not on the GPU go to the reference's own methods: training steps through the installed drop-ins on
    the CPU select the same points and leave the same model as the reference's; every fall-back is counted by reason."""
    from LoG.model.level_of_gaussian import Gaussian, LoG
    from log_amd import prepare
    saved = _methods()
    ref = _log_model(0, 400)
    ref.counter.radius3d_max.fill_(0.05)                      # a bound that binds, so the clamp changes rows
    sel_ref = _run_steps(ref, 2, 96, 72)
    try:
        assert prepare.install() is LoG
        assert _methods() == (prepare.log_prepare, prepare.gaussian_prepare, prepare.clamp_scale, prepare.step)
        prepare.dropins.logged.clear()
        prepare.reset_stats()
        new = _log_model(0, 400)
        new.counter.radius3d_max.fill_(0.05)
        with caplog.at_level("WARNING", logger="log_amd"):
            sel_new = _run_steps(new, 2, 96, 72)
            pre = new.gaussian.scaling.detach().clone() + 0.5       # the steps' round-off aside: one state for both clamps
            new.gaussian.scaling.copy_(pre)
            new.clamp_scale(torch.arange(new.num_points))
            flat = Gaussian()
            flat.xyz = new.gaussian.xyz
            flat.prepare(None, {"full_proj_transform": torch.eye(4)})
        prepare.uninstall()
        assert _methods() == saved
    finally:
        _set_methods(saved)
    assert all(a.numel() > 100 and torch.equal(a, b) for a, b in zip(sel_ref, sel_new))
    ref.gaussian.scaling.copy_(pre)
    ref.counter.radius3d_min.copy_(new.counter.radius3d_min)
    ref.clamp_scale(torch.arange(ref.num_points))
    assert torch.equal(ref.gaussian.scaling, new.gaussian.scaling) and not torch.equal(pre, new.gaussian.scaling)
    st = prepare.stats()
    why = "tensors are not on the GPU"
    # the reference's step calls self.clamp_scale: two of the three clamp calls come from the two steps that fell back
    assert st["calls"] == {"log_prepare": 2, "step": 2, "clamp_scale": 3, "gaussian_prepare": 1}
    assert st["fallbacks"] == {("log_prepare", why): 2, ("step", why): 2, ("clamp_scale", why): 3, ("gaussian_prepare", why): 1}
    assert st["readbacks"] == {}
    logged = [r.getMessage() for r in caplog.records if "log_amd.prepare" in r.getMessage()]
    assert len(logged) == 4 and all("not on the GPU" in m for m in logged), logged       # once per method, not per call


def test_fallback_reasons():
    """What the kernels do not cover is named before anything is launched."""
    import types
    from log_amd import _dropin, prepare
    with pytest.raises(_dropin.Fallback, match="not on the GPU"):
        prepare._device_and_rows(torch.zeros(4, 3))
    act = types.SimpleNamespace(scaling_activation=torch.sigmoid, opacity_activation=torch.sigmoid,
                                rotation_activation=torch.nn.functional.normalize)
    with pytest.raises(_dropin.Fallback, match="activations other than exp / sigmoid / normalize"):
        _dropin.check_activations(act, *prepare._VIEW_ACTIVATIONS)
    with pytest.raises(_dropin.Fallback, match="activations"):
        _dropin.check_activations(None, *prepare._VIEW_ACTIVATIONS)
    act.scaling_activation = torch.exp
    _dropin.check_activations(act, *prepare._VIEW_ACTIVATIONS)


@needs_reference
def test_install_all_without_the_flag_patches_nothing_new(cpu_cuda_shims):
    from LoG.model.counter import Counter
    from LoG.model.level_of_gaussian import LoG
    from LoG.model.sparse_optimizer import SparseOptimizer
    from LoG.model.tensor_tree import TensorTree
    import LoG.render.renderer as ref_renderer
    import log_amd
    methods = _methods()
    saved = (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
             ref_renderer.torch)
    try:
        patched = log_amd.install_all()
        assert [c.__name__ for c in patched] == ["LoG", "TensorTree", "Counter", "SparseOptimizer"]
        assert _methods() == methods
        patched = log_amd.install_all(device_prepare=True)
        assert len(patched) == 5 and patched[-1] is LoG and LoG.prepare is log_amd.prepare.log_prepare
        assert LoG.step is log_amd.prepare.step and LoG.clamp_scale is log_amd.prepare.clamp_scale
        log_amd.prepare.uninstall()
        assert _methods() == methods
    finally:
        (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
         ref_renderer.torch) = saved
        _set_methods(methods)
        if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
            del SparseOptimizer._lograst_load_state_dict


def test_docs_name_the_switch():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "device_prepare" in open(os.path.join(ROOT, doc)).read(), doc

"""Steps over several views (log_amd/multi_view.py), CPU side: the restatement (tests/multi_view_ref.py) against the fixture
made by the reference's own code (tests/golden/make_multi_view_golden.py), the library's wide offsets on the host, and the
module's host logic through the reference's UNMODIFIED classes on the CPU test double (tests/multi_view_backend.py)."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

import multi_view_ref as mref
from test_log_plumbing_cpu import REF, _batch, _log_model, cpu_cuda_shims, log_env   # noqa: F401  (fixtures)


def test_restatement_reproduces_the_fixture():
    """accumulate + step restated in float64 and fp32 hold the reference's recorded sums, model rows and moments within
    8 * (|ref32 - ref64| + 2^-24 S); the rows and their counts are the fixture's exactly; rows no view saw are not in it."""
    bufs, m1, m2, views, g = mref.load()
    refs = mref.reference(bufs, m1, m2, views, g)
    (s64, _, seen64, _, rows), (_, _, seen32, _, _) = refs
    assert torch.equal(seen64, torch.from_numpy(g["seen"])) and torch.equal(seen32, seen64)
    assert torch.equal(rows, torch.from_numpy(g["rows"]))
    assert 300 < rows.numel() < bufs["xyz"].shape[0] // 4 and int((seen64 > 1).sum()) > 50 and int(seen64.max()) == 3
    assert set(s64) == set(bufs)
    sums = {k: torch.from_numpy(g["sum_" + k]) for k in bufs}
    stepped = {k: tuple(torch.from_numpy(g[f"after_{name}_{k}"]) for name in ("model", "exp_avg", "exp_avg_sq")) for k in bufs}
    worst = mref.check_against_fixture(sums, stepped, g, refs)
    print(f"fixture vs float64 restatement: largest error / bound {worst:.3f}")
    # a view's dead rows (radii <= 0) and its node rows are in no sum: the first view's alone
    v0 = views[0]
    dead = v0["index"][v0["radii"][:v0["index"].shape[0]] <= 0]
    only0 = dead[(seen64[dead] == 0)]
    assert only0.numel() > 10 and all(float(s64[k][only0].abs().sum()) == 0.0 for k in s64)


def test_wide_offsets_on_the_host():
    """num_points times the widest row does not fit 32 bits: the library's own offset expression (the kernels' lr_acc_offset,
    through lograst_accumulate_target_floats), on the host."""
    from log_amd import _lib
    L = _lib.lib()
    f = L.lograst_accumulate_target_floats
    assert f(0, 59, 45) == 0 and f(1, 3, 3) == 3 and f(5000, 16, 3) == 4999 * 16 + 3
    for P, stride, width in ((2 ** 31 - 1, 45, 45), (2 ** 31 - 1, 59, 45), (30_000_000, 16, 4), (2 ** 31 - 1, 2 ** 31 - 1, 1),
                             (47_721_859, 45, 45)):           # the last: the first P whose 45-float rows pass 2^31 floats
        want = (P - 1) * stride + width
        assert f(P, stride, width) == want, (P, stride, width)
        assert want > 2 ** 31 or P == 30_000_000
    assert _lib.LograstAccTarget.row_stride_floats.offset == ctypes.sizeof(ctypes.c_void_p)
    assert L.lograst_version() == 4


# ---- the module through the reference's classes --------------------------------------------------------------------------
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")

@pytest.fixture()
def mv_env(cpu_cuda_shims):     # noqa: F811
    """The CPU double with the two new calls, every drop-in the trainer needs installed on the reference's classes, and all
    of it taken back afterwards."""
    import oracle_backend
    from multi_view_backend import MultiViewBackend
    from LoG.model.tensor_tree import TensorTree
    from LoG.model.counter import Counter
    from LoG.model.sparse_optimizer import SparseOptimizer
    from LoG.model.level_of_gaussian import LoG
    import LoG.render.renderer as ref_renderer
    import log_amd
    from log_amd import get_all, multi_view
    saved = (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
             LoG.step, ref_renderer.torch)
    old = oracle_backend.install(MultiViewBackend())
    log_amd.install_all()
    multi_view.reset_stats()
    multi_view.dropins.logged.clear()
    yield multi_view
    multi_view.uninstall()
    multi_view.dropins._saved.clear()
    (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all, LoG.step,
     ref_renderer.torch) = saved
    if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
        del SparseOptimizer._lograst_load_state_dict
    get_all._multi_view = None
    oracle_backend.install(old)


W, H = 96, 72
NARROW = 3.0 * W


def _views(model, n, step=True, first=0, focal=1.1 * W):
    """trainer.py:144-160 per view: render -> loss.backward -> update_by_output -> step; -> per view (index, flag_vis)."""
    from LoG.render.renderer import NaiveRendererAndLoss
    from log_amd import scenes
    renderer = NaiveRendererAndLoss(split="train", use_origin_render=False, background=[1., 1., 1.])
    cams = scenes.orbit_cameras(8, W=W, H=H, focal=focal, radius=2.2)
    out = []
    for it in range(first, first + n):
        torch.manual_seed(100 + it)
        batch = _batch([cams[it]])
        batch["image"] = torch.rand(1, H, W, 3)
        output = renderer(batch, model)
        output["loss"].backward()
        model.update_by_output(output)
        vf = output["visibility_flag"][0]
        out.append((vf["index"].clone(), vf["flag_vis"][:vf["index"].shape[0]].clone(), vf["params"]))
        if step:
            model.step()
    return out


def _tensors(model):
    out = {"model_" + k: v for k, v in model.gaussian.items()}
    out.update({"exp_avg_" + k: model.optimizer.exp_avg[k] for k in model.optimizer.optimize_keys})
    out.update({"exp_avg_sq_" + k: model.optimizer.exp_avg_sq[k] for k in model.optimizer.optimize_keys})
    return {k: v.detach().clone() for k, v in out.items()}


@needs_reference
def test_one_view_per_step_is_the_installed_single_view_path(mv_env):
    """K = 1 over three steps: model, moments, global_steps and xyz_lr are those of the installed single-view drop-ins, bit
    for bit (both go through the same backend arithmetic; the accumulated path adds each gradient to a zero)."""
    single = _log_model(0, 400)
    _views(single, 3)
    mv_env.install(views_per_step=1)
    multi = _log_model(0, 400)
    per_view = _views(multi, 3)
    assert all(p.grad is None for _, _, params in per_view for p in params.values())
    a, b = _tensors(single), _tensors(multi)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(multi.optimizer.global_steps) == float(single.optimizer.global_steps) == 3.0
    assert multi.optimizer.xyz_lr == single.optimizer.xyz_lr and multi.lr == single.lr
    st = mv_env.stats()
    assert st["counts"] == {"views": 3, "accumulated": 3, "ordinary": 0, "steps": 3} and not st["fallbacks"]
    assert mv_env.pending(multi) == 0
    state = mv_env.state(multi)
    assert int(state.seen.abs().sum()) == 0 and float(state.flat.flat.abs().sum()) == 0.0
    assert set(state.views) == {"means3D", "scales", "rotations", "opacities", "colors", "shs"}


@needs_reference
def test_two_views_per_step_move_the_rows_only_the_first_view_saw(mv_env):
    """K = 2: after two views and two calls of step, the rows that only the FIRST view saw have moved and carry moments, rows
    that neither saw keep their bits, and one optimizer step was counted.  On the code without this module the first view's
    gradients are dropped: those rows stay.  (That the step is Adam on the SUM is the kernels' test, tests/test_gpu_multi_view.py,
    and the restatement's against the fixture.)"""
    mv_env.install(views_per_step=2)
    model = _log_model(0, 400)
    before = _tensors(model)
    (i0, f0, _), (i1, f1, _) = _views(model, 2, focal=NARROW)       # narrow cameras 45 degrees apart: each sees its own part
    after = _tensors(model)
    assert float(model.optimizer.global_steps) == 1.0 and mv_env.pending(model) == 0
    P = model.num_points
    seen0, seen1 = torch.zeros(P, dtype=torch.bool), torch.zeros(P, dtype=torch.bool)
    seen0[i0[f0]] = True
    seen1[i1[f1]] = True
    only_first, neither = seen0 & ~seen1, ~seen0 & ~seen1
    print('rows: only the first view', int(only_first.sum()), 'neither', int(neither.sum()), 'both', int((seen0 & seen1).sum()))
    assert int(only_first.sum()) > 20 and int(neither.sum()) > 20 and int((seen0 & seen1).sum()) > 20
    moved = (after["model_xyz"] != before["model_xyz"]).any(1)
    # (a seen row whose gradient is exactly zero -- covered or off the image -- stays: more than half of them moved; none
    # would without the module)
    assert int((moved & only_first).sum()) > 0.5 * int(only_first.sum())
    for k in before:
        assert torch.equal(after[k][neither], before[k][neither]), k
    assert bool((after["exp_avg_xyz"][only_first] != 0).any(1).float().mean() > 0.5)
    assert mv_env.stats()["counts"] == {"views": 2, "accumulated": 2, "ordinary": 0, "steps": 1}


@needs_reference
def test_flush_steps_with_the_views_that_are_pending(mv_env):
    """K = 3, one view, flush: the step K = 1 takes with that view alone; a second flush is a no-op."""
    mv_env.install(views_per_step=1)
    one = _log_model(0, 400)
    _views(one, 1)
    mv_env.install(views_per_step=3)
    model = _log_model(0, 400)
    _views(model, 1)
    assert mv_env.pending(model) == 1 and float(model.optimizer.global_steps) == 0.0
    assert mv_env.flush(model) is True and mv_env.pending(model) == 0
    a, b = _tensors(one), _tensors(model)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(model.optimizer.global_steps) == 1.0 and model.lr == one.lr
    assert mv_env.flush(model) is False and float(model.optimizer.global_steps) == 1.0
    assert mv_env.flush(_log_model(1, 100)) is False          # a model that never accumulated


@needs_reference
def test_ordinary_gradients_are_added_by_step(mv_env):
    """A backward that reaches get_all without a render of its own rows leaves ordinary gradients; step adds them by
    index[flag_vis] -- the same sums, so the same step, as K = 1 takes from an accumulated backward of the same gradients."""
    from log_amd import rasterizer as R
    mv_env.install(views_per_step=1)
    a = _log_model(0, 400)
    _views(a, 1)
    b = _log_model(0, 400)
    took = R.take_backward_radii
    try:
        R.take_backward_radii = lambda rows=None: None      # the render's radii are not there to be taken
        _views(b, 1)
    finally:
        R.take_backward_radii = took
    ta, tb = _tensors(a), _tensors(b)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert mv_env.stats()["counts"] == {"views": 2, "accumulated": 1, "ordinary": 1, "steps": 2}


@needs_reference
def test_size_checks_raise_before_any_launch(mv_env):
    from log_amd import multi_view as mv
    P, n, rows, K = 50, 6, 8, 3
    raw = {"xyz": torch.zeros(rows, 3), "scaling": torch.zeros(rows, 3), "opacity": torch.zeros(rows, 1),
           "rotation": torch.ones(rows, 4), "colors": torch.zeros(rows, 3), "shs": torch.zeros(rows, K, 3)}
    grads = tuple(torch.ones(rows, w) for w in (3, 3, 1, 4, 3))
    targets = {"xyz": torch.zeros(P, 3), "shs": torch.zeros(P, K, 3)}
    seen = torch.zeros(P, dtype=torch.int32)
    index, radii, campos = torch.arange(rows), torch.ones(rows, dtype=torch.int32), torch.zeros(3)
    mv._accumulate(raw, n, 1, campos, grads, index, radii, targets, seen)           # the sizes as they should be
    assert int(seen.sum()) == n and float(targets["xyz"].sum()) == 3.0 * n
    bad = [dict(index=index[:n - 1]), dict(radii=radii[:rows - 1]), dict(radii=torch.ones(rows + 1, dtype=torch.int32)),
           dict(targets={"xyz": torch.zeros(P - 1, 3)}), dict(targets={"shs": torch.zeros(P, K + 1, 3)}),
           dict(seen=torch.zeros(P + 1, dtype=torch.int32)), dict(n=rows + 1), dict(targets={"nope": torch.zeros(P, 3)})]
    for change in bad:
        kw = dict(raw=raw, n=n, degree=1, campos=campos, grads=grads, index=index, radii=radii, targets=targets, seen=seen)
        kw.update(change)
        before = (seen.clone(), targets["xyz"].clone())
        with pytest.raises(ValueError):
            mv._accumulate(**kw)
        assert torch.equal(seen, before[0]) and torch.equal(targets["xyz"], before[1]), change
    entry = (torch.zeros(P, 3), targets["xyz"], torch.zeros(P, 3), torch.zeros(P, 3), None, 1e-3)
    for change in (dict(seen=torch.zeros(P - 1, dtype=torch.int32)), dict(moved_out=torch.zeros(P + 1, dtype=torch.uint8)),
                   dict(entries={"xyz": (torch.zeros(P, 4),) + entry[1:]})):
        kw = dict(seen=seen, entries={"xyz": entry}, beta1=0.9, beta2=0.999, bias_correction2_sqrt=1.0, eps=1e-15, moved_out=None)
        kw.update(change)
        with pytest.raises(ValueError):
            mv._step(**kw)
    # the public pair takes GPU tensors only
    with pytest.raises(ValueError, match="GPU"):
        mv.accumulate(raw, n, 1, campos, grads, index, radii, targets, seen)
    with pytest.raises(ValueError, match="GPU"):
        mv.step(seen, {"xyz": entry})
    for k in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            mv.install(views_per_step=k)


@needs_reference
def test_a_resize_with_views_pending_raises(mv_env):
    mv_env.install(views_per_step=2)
    model = _log_model(0, 400)
    _views(model, 1)
    assert mv_env.pending(model) == 1
    old = mv_env.state(model)
    g = model.gaussian
    grow = lambda t: torch.cat([t, t[:1]])
    for k in list(g.keys):                                          # what a densification leaves: new buffers, one row more
        setattr(g, k, grow(getattr(g, k)))
        for d in (model.optimizer.exp_avg, model.optimizer.exp_avg_sq):
            setattr(d, k, grow(d[k]))
    with pytest.raises(RuntimeError, match="resized"):
        model.step()
    assert mv_env.state(model) is old and old.pending == 1           # nothing was stepped, nothing thrown away
    # with none pending the state is made again, lazily
    model2 = _log_model(0, 400)
    _views(model2, 2)
    st = mv_env.state(model2)
    g2 = model2.gaussian
    for k in list(g2.keys):
        setattr(g2, k, getattr(g2, k).clone())                       # same size, new storage: also a new state
    mv_env._state_for(model2.optimizer, dict(g2.items()), g2.xyz.device)
    assert mv_env.state(model2) is not st and mv_env.state(model2).P == st.P


@needs_reference
def test_fall_backs_are_counted_and_logged_once(mv_env, caplog):
    from log_amd import get_all
    mv_env.install(views_per_step=2)
    model = _log_model(0, 400)
    model.fix_parent = False
    with caplog.at_level(logging.WARNING, logger="log_amd"):
        _views(model, 2)
    st = mv_env.stats()
    assert st["fallbacks"][("step", "fix_parent=False")] == 2 and st["fallbacks"][("get_all", "fix_parent=False")] == 2
    assert st["counts"]["steps"] == 0 and float(model.optimizer.global_steps) == 2.0      # the installed step ran, per view
    assert sum("fix_parent=False" in r.getMessage() for r in caplog.records) == 2         # once per method
    # tensors that are not fp32, and (with the HIP backend in place) tensors that are not on the GPU
    model = _log_model(0, 400)
    bufs = {k: v.double() for k, v in model.gaussian.items()}
    with pytest.raises(mv_env.Fallback, match="fp32"):
        mv_env._covered(model, bufs)
    import oracle_backend
    old = oracle_backend.install(None)
    try:
        with pytest.raises(mv_env.Fallback, match="not on the GPU"):
            mv_env._covered(model, dict(model.gaussian.items()))
    finally:
        oracle_backend.install(old)
    bufs = dict(model.gaussian.items())
    bufs["extra"] = bufs["xyz"]
    with pytest.raises(mv_env.Fallback, match="keys outside"):
        mv_env._covered(model, bufs)
    model.optimizer.exp_avg.xyz = torch.zeros(3, 3)
    with pytest.raises(mv_env.Fallback, match="moments"):
        mv_env._covered(model, dict(model.gaussian.items()))
    # the fused step is not taken for a model this module handles: said once
    prev = get_all.set_fused_step(True)
    try:
        with caplog.at_level(logging.WARNING, logger="log_amd"):
            model = _log_model(0, 400)
            _views(model, 2)
        assert not getattr(model.optimizer, "_lograst_fused_pending", False)
        assert sum("fused step is not taken" in r.getMessage() for r in caplog.records) == 1
        assert mv_env.stats()["counts"]["steps"] == 1
    finally:
        get_all.set_fused_step(prev)


@needs_reference
def test_uninstall_restores_both_methods(mv_env):
    from LoG.model.level_of_gaussian import LoG
    from log_amd import get_all
    before = LoG.step
    assert get_all._multi_view is None
    assert mv_env.install(views_per_step=2) is LoG
    assert LoG.step is not before and get_all._multi_view is mv_env
    mv_env.uninstall()
    assert LoG.step is before and get_all._multi_view is None
    import log_amd
    assert "views_per_step" in log_amd.install_all.__code__.co_varnames
    log_amd.install_all(views_per_step=2)
    assert LoG.step is not before and get_all._multi_view is mv_env and mv_env._views_per_step == 2
    mv_env.uninstall()
    log_amd.install_all()
    assert LoG.step is before and get_all._multi_view is None

"""CPU checks of the device initialisation pass (log_amd/init_pass.py, log_amd/csrc/init.hip): the numpy restatement
(tests/init_ref.py) against the fixture recorded from the reference (tests/golden/init_log.npz), the new entry point of the
C ABI and its argument validation, and the drop-ins' fall-back to the saved methods."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import init_ref as IR
from test_log_plumbing_cpu import log_env   # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("LOG_REFERENCE", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")
_ACT = types.SimpleNamespace(scaling_activation=torch.exp, scaling_inverse_activation=torch.log,
                             rotation_activation=torch.nn.functional.normalize)


@pytest.fixture(scope="module")
def fx():
    return {k: v for k, v in IR.load("log").items()}


def _cams(fx):
    return [IR.camera_args(fx, v) for v in IR.views(fx)]


def test_fixture_is_what_the_generator_promises(fx):
    assert os.path.getsize(os.path.join(IR.GOLDEN, "init_log.npz")) < 1_000_000
    P = fx["xyz"].shape[0]
    views = IR.views(fx)
    assert 2500 <= P <= 3500 and len(views) == 9 and int(fx["num_views"]) == 9
    assert views[-2:] == ["away", "all"] and [int(x) for x in fx["hd_wh"]] == [1920, 1080]
    flags = {v: IR.bits(fx, f"{v}_valid", P) for v in views}
    assert not flags["away"].any() and flags["all"].all()
    assert all(0.05 <= flags[v].mean() <= 0.95 for v in views[:-2])
    ever = np.any([flags[v] for v in views[:-1]], axis=0)
    assert 0 < (~ever).sum() == int(fx["meta_never_valid_before_all"])
    start, final = fx["radius3d_min_start"], fx["all_radius3d_min"]
    assert IR.same_bits(fx["away_radius3d_min"][~ever], start[~ever])        # valid in no view so far: bit for bit
    assert np.mean(final.view(np.uint32) == start.view(np.uint32)) >= 0.05     # the start value binds for some rows ...
    assert np.mean(final < start) >= 0.05                                      # ... and the views for others
    s = fx["scaling"]
    assert s.max() - s.min() > np.log(50.0)                                    # raw scales over two decades


def test_torch_mode_reproduces_the_reference_bit_for_bit(fx, oracle_mod):
    """Flags and values after every view, and at_init_final's scaling = max(scaling, log(radius3d_min))."""
    got = IR.log_init("torch", fx["xyz"], fx["scaling"], fx["rotation"], _cams(fx), fx["radius3d_min_start"])
    P = fx["xyz"].shape[0]
    for v, (valid, rmin) in zip(IR.views(fx), got):
        assert np.array_equal(valid, IR.bits(fx, f"{v}_valid", P)), v
        assert IR.same_bits(rmin, fx[f"{v}_radius3d_min"]), v
    want = torch.maximum(torch.from_numpy(fx["scaling"]), torch.log(torch.from_numpy(got[-1][1]))[:, None].repeat(1, 3))
    assert IR.same_bits(want.numpy(), fx["scaling_final"])
    assert (fx["scaling_final"] > fx["scaling"]).any()


def test_fixed_mode_has_the_fixture_s_flags(fx, oracle_mod):
    """The kernel's activations (lr_exp_any, lr_normalize4) decide every row of every view as torch's do; the values
    differ in the last bits (printed, not gated: each side is compared exactly with its own restatement)."""
    got = IR.log_init("fixed", fx["xyz"], fx["scaling"], fx["rotation"], _cams(fx), fx["radius3d_min_start"])
    P = fx["xyz"].shape[0]
    worst = 0.0
    for v, (valid, rmin) in zip(IR.views(fx), got):
        assert np.array_equal(valid, IR.bits(fx, f"{v}_valid", P)), v
        worst = max(worst, float(np.abs(rmin.astype(np.float64) / fx[f"{v}_radius3d_min"] - 1).max()))
    print("radius3d_min, fixed against torch activations: worst relative difference", worst)


def test_exp_any_restatement():
    """The restated lr_exp_any (libm fmaf): NaN loses against the lower clamp as fmaxf has it, +-200 are clamped to finite
    values, and over the scales a model has it is exp to a few ulp (a sanity bound: the GPU tests compare the kernel's
    activated scale with this function bit for bit)."""
    raw = np.array([np.nan, 200.0, -200.0, 0.0, -1.0, 1.0, 80.0, -80.0, 0.5, np.log(0.05)], np.float32)
    got = IR.exp_any(raw)
    assert got[0] == got[2] and got[0] > 0 and got[1] < np.inf
    assert np.abs(got[3:] / np.exp(raw[3:].astype(np.float64)) - 1).max() < 2e-6
    rng = np.random.default_rng(5)
    x = rng.uniform(-7, 1, 4000).astype(np.float32)
    assert np.abs(IR.exp_any(x) / np.exp(x.astype(np.float64)) - 1).max() < 2e-6
    assert IR.same_bits(IR.exp_any(x[:64].reshape(8, 8)), IR.exp_any(x[:64]).reshape(8, 8))


def test_minimum_is_torch_minimum():
    nan = float("nan")
    a = np.array([1.0, nan, 1.0, nan, 2.0, -0.0], np.float32)
    b = np.array([2.0, 1.0, nan, nan, 1.0, 0.0], np.float32)
    want = torch.minimum(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    got = IR.minimum(a, b)
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[[1, 2, 3]]).all() and got[4] == 1.0


def test_symbol_is_declared_exported_and_bound():
    import re
    from log_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lograst.h")).read(), flags=re.S)
    name = "lograst_init_radius3d"
    assert re.search(r"\b%s\s*\(" % name, header)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and name in _lib._SIGNATURES and name in _lib.EXPORTS
    assert _lib.lib().lograst_version() == 4


def test_argument_validation_needs_no_gpu():
    from log_amd import _lib
    L = _lib.lib()
    err = lambda: L.lograst_last_error().decode()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda P, V, xyz=p, rmin=p, valid=None, r3d=None: L.lograst_init_radius3d(P, xyz, p, p, V, p, rmin, valid, r3d, None)
    assert call(-1, 1) == -1 and "negative" in err()
    assert call(8, -1) == -1 and "negative" in err()
    assert call(8, 2, valid=p) == -1 and "num_views must be 1" in err()
    assert call(8, 0, r3d=p) == -1 and "num_views must be 1" in err()
    assert call(8, 1, xyz=None) == -1 and "NULL" in err()
    assert call(0, 1, xyz=None) == 0 and call(8, 0, xyz=None) == 0        # nothing to do: no error, no device work


# ---- the drop-ins on stand-in objects --------------------------------------------------------------------------------

def _stand_in(P=6):
    g = types.SimpleNamespace(xyz=torch.zeros(P, 3), scaling=torch.zeros(P, 3), rotation=torch.ones(P, 4), activation=_ACT)
    model = types.SimpleNamespace(gaussian=g, counter=types.SimpleNamespace(radius3d_min=torch.ones(P)), num_views=0)
    return model


def test_dropins_fall_back_on_cpu_tensors_and_count_the_reason(caplog):
    from log_amd import init_pass
    model = _stand_in()
    calls = []

    def ref_init(self, renderer, batch, iteration):
        calls.append(("init", iteration))
        self.num_views += 1

    def ref_radius(self, batch, renderer):
        calls.append(("radius3d", batch))
        return "flag", "radius"

    init_pass.reset_stats()
    init_pass.dropins.logged.clear()
    with init_pass.dropins.substituted(log_init=ref_init, init_radius3d=ref_radius), \
            caplog.at_level("WARNING", logger="log_amd"):
        for i in range(3):
            init_pass.log_init(model, None, {"b": i}, i)
        assert init_pass.init_radius3d(model.gaussian, "batch", None) == ("flag", "radius")
    assert calls == [("init", 0), ("init", 1), ("init", 2), ("radius3d", "batch")] and model.num_views == 3
    why = "tensors are not on the GPU"
    st = init_pass.stats()
    assert st["calls"] == {"log_init": 3, "init_radius3d": 1}
    assert st["fallbacks"] == {("log_init", why): 3, ("init_radius3d", why): 1} and st["readbacks"] == {}
    logged = [r.getMessage() for r in caplog.records if "log_amd.init_pass" in r.getMessage()]
    assert len(logged) == 2 and all("not on the GPU" in m for m in logged), logged
    assert getattr(model, init_pass._PENDING, None) is None


def test_fallback_reasons():
    """What the kernel does not cover is named before anything is launched."""
    from log_amd import _dropin, init_pass
    g = _stand_in().gaussian
    with pytest.raises(_dropin.Fallback, match="not on the GPU"):
        init_pass._model_inputs(g)
    act = types.SimpleNamespace(scaling_activation=torch.sigmoid, rotation_activation=torch.nn.functional.normalize)
    with pytest.raises(_dropin.Fallback, match="activations other than exp / normalize"):
        _dropin.check_activations(act, *init_pass._ACTIVATIONS)
    _dropin.check_activations(_ACT, *init_pass._ACTIVATIONS)
    with pytest.raises(_dropin.Fallback, match="without compute_radius"):
        renderer = types.SimpleNamespace(background=None, prepare_camera=lambda b, n, bg: (None, object(), bg))
        init_pass._rasterizer_settings(renderer, None)
    with pytest.raises(ValueError, match="at least 1"):
        init_pass.install(views_per_launch=0)
    from log_amd import _lib
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        init_pass.update_radius3d_min(g.xyz, g.scaling, g.rotation, [], torch.ones(6))


def _methods():
    from LoG.model.level_of_gaussian import Gaussian, LoG
    return (Gaussian.init_radius3d, LoG.init, LoG.at_init_final)


def _set_methods(saved):
    from LoG.model.level_of_gaussian import Gaussian, LoG
    Gaussian.init_radius3d, LoG.init, LoG.at_init_final = saved


@needs_reference
def test_install_and_uninstall_put_every_method_back(log_env):
    from LoG.model.level_of_gaussian import LoG
    from log_amd import init_pass
    saved = _methods()
    try:
        assert init_pass.install(views_per_launch=4) is LoG and init_pass._views_per_launch == 4
        assert _methods() == (init_pass.init_radius3d, init_pass.log_init, init_pass.at_init_final)
        assert init_pass.dropins.original("log_init") is saved[1]
        init_pass.uninstall()
        assert _methods() == saved and init_pass._views_per_launch == 1
    finally:
        _set_methods(saved)


@needs_reference
def test_install_all_installs_the_module_on_request(log_env):
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
        assert len(patched) == 4 and _methods() == methods
        patched = log_amd.install_all(device_init=True)
        assert len(patched) == 5 and patched[-1] is LoG and LoG.init is log_amd.init_pass.log_init
        assert log_amd.init_pass._views_per_launch == 1
        log_amd.init_pass.uninstall()
        assert _methods() == methods
    finally:
        (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
         ref_renderer.torch) = saved
        _set_methods(methods)
        if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
            del SparseOptimizer._lograst_load_state_dict


def test_docs_name_the_switch():
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "device_init" in open(os.path.join(ROOT, doc)).read(), doc

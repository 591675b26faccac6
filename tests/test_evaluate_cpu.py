"""CPU checks of the evaluation path (log_amd/evaluate.py, lograst_eval_*, lograst_image_to_bgr8): the restatement the GPU
tests measure against (tests/evaluate_ref.py) is itself held to the reference's own results (tests/golden/evaluate_*.npz,
written by tests/golden/make_golden_evaluate.py from LoG's metric.py, tensor_to_bgr and Trainer.make_validation); the sizing
helper, argument validation and the no-CPU-fallback rule work without a GPU; the drop-ins hand CPU tensors to what they
replaced, count it, and leave a staticmethod a staticmethod."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from evaluate_ref import evaluate_ref, golden_cases, to_bgr8, within  # noqa: E402

CASES = golden_cases()
REF = os.environ.get("LOG_REFERENCE", "/root/reference")
NAMES = ["1x1", "2x3", "11x11", "33x65", "33x67_gain", "37x53_gain", "64x96_hwc", "identical", "constant", "low_contrast",
         "out_of_range", "gain_clamped", "w1_gain", "grid8"]


def chw(c):
    gt = c["gt"].transpose(2, 0, 1) if int(c["gt_hwc"]) else c["gt"]
    return c["pred"], np.ascontiguousarray(gt)


def test_all_cases_present():
    assert sorted(CASES) == sorted(NAMES)
    for name, c in CASES.items():
        assert os.path.getsize(os.path.join(HERE, "golden", "evaluate_%s.npz" % name)) < 400 * 1000
        pred, gt = chw(c)
        assert pred.dtype == np.float32 and gt.dtype == np.float32 and pred.shape == gt.shape and 1 <= pred.shape[0] <= 4
        assert not np.isnan(pred).any() and not np.isnan(gt).any()
        assert c["mv_vis"].shape == (2 * pred.shape[1], pred.shape[2], pred.shape[0]) and c["mv_vis"].dtype == np.uint8


def test_fixtures_hold_the_cases_they_are_named_for():
    shape = lambda n: chw(CASES[n])[0].shape
    assert shape("1x1") == (3, 1, 1) and shape("2x3") == (1, 2, 3) and shape("11x11") == (4, 11, 11)
    assert shape("33x65") == (3, 33, 65) and shape("37x53_gain") == (3, 37, 53) and shape("64x96_hwc") == (3, 64, 96)
    assert shape("33x67_gain")[2] // 2 % 2 == 1 and CASES["64x96_hwc"]["gt"].shape == (64, 96, 3)
    assert {n for n in NAMES if int(CASES[n]["fit"])} == {"33x67_gain", "37x53_gain", "gain_clamped", "w1_gain"}
    assert math.isinf(float(CASES["identical"]["psnr"])) and float(CASES["identical"]["ssim"]) == pytest.approx(1.0, abs=1e-6)
    for k in ("pred", "gt"):
        assert len(np.unique(CASES["constant"][k])) == 1
    p, g = chw(CASES["low_contrast"])
    assert np.abs(p - g).max() < 1e-3 and p.std() < 2e-3
    p, g = chw(CASES["out_of_range"])
    assert p.min() < 0 and p.max() > 1 and float(CASES["out_of_range"]["mv_l1"]) > 0.5            # nothing was clamped
    c = CASES["gain_clamped"]
    r = evaluate_ref(*chw(c), fit_gain=True)
    assert (c["pred"] * r["gain"][:, None, None] > 1).mean() > 0.2 and r["corrected"].max() == 1.0
    assert np.isnan(float(CASES["w1_gain"]["mv_l1"])) and np.isnan(float(CASES["w1_gain"]["mv_psnr"]))
    g8 = CASES["grid8"]["pred"].reshape(-1)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    for v in (k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))):
        assert np.isin(v, g8).all()
    assert np.signbit(g8[g8 == 0]).any() and (g8 == 1).any() and (g8 < 0).any() and (g8 > 1).any()
    assert set(np.unique(CASES["grid8"]["bgr_pred"])) == set(range(256))


@pytest.mark.parametrize("name", NAMES)
def test_fp32_mirror_reproduces_the_8bit_goldens_bit_for_bit(name):
    c = CASES[name]
    pred, gt = chw(c)
    assert np.array_equal(to_bgr8(pred), c["bgr_pred"]) and np.array_equal(to_bgr8(gt), c["bgr_gt"])
    if name == "w1_gain":
        return              # the corrected half is a nan image: its bytes are unspecified
    r32 = evaluate_ref(pred, gt, fit_gain=bool(c["fit"]), dtype=np.float32)
    assert np.array_equal(to_bgr8(np.concatenate([r32["corrected"], gt], axis=1)), c["mv_vis"])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_references_scalars(name):
    """The reference's own fp32 results against the float64 restatement, within what the fp32 mirror says fp32 can give:
    |golden - ref64| <= 8 (|ref32 - ref64| + 2^-24 S).  L1 and the SSIM are means (S = the mean magnitude of the terms).  The
    PSNR is -10 log10 of a mean: its error is (10 / ln 10) times the relative error of the mean, plus the rounding of the
    logarithm and of the product, relative to the value: S = 10 / ln 10 + |psnr|."""
    c = CASES[name]
    pred, gt = chw(c)
    fit = bool(c["fit"])
    r64, r32 = evaluate_ref(pred, gt, fit_gain=fit), evaluate_ref(pred, gt, fit_gain=fit, dtype=np.float32)
    checks = [("mv_l1", float(c["mv_l1"]), r64["l1"], r32["l1"], r64["l1"]),
              ("mv_psnr", float(c["mv_psnr"]), r64["psnr"], r32["psnr"], 10 / math.log(10) + abs(r64["psnr"]))]
    p64 = evaluate_ref(pred, gt, ssim=True, max_val=float(c["max_val"]))
    p32 = evaluate_ref(pred, gt, ssim=True, max_val=float(c["max_val"]), dtype=np.float32)
    checks += [("psnr", float(c["psnr"]), p64["psnr"], p32["psnr"], 10 / math.log(10) + abs(p64["psnr"])),
               ("ssim", float(c["ssim"]), p64["ssim"], p32["ssim"], p64["ssim_S"])]
    for what, golden, v64, v32, S in checks:
        ok, err, bound = within(golden, v64, v32, S if np.isfinite(S) else 0.0)
        print(f"{name} {what}: golden {golden!r} ref64 {v64!r} ref32 {v32!r} err {err:.3g} bound {bound:.3g}")
        assert ok, (what, golden, v64, v32, err, bound)


def test_scratch_sizing_by_hand():
    from log_amd import _lib
    L = _lib.lib()
    # 3 doubles per 32 x 32 tile and channel, 2 doubles per 4096 left-half elements and channel, rounded up to 256 bytes
    assert L.lograst_eval_scratch_bytes(3, 1080, 1920) == (8 * (3 * 34 * 60 * 3 + 2 * 3 * 254) + 255) // 256 * 256
    assert L.lograst_eval_scratch_bytes(1, 1, 1) == 256
    assert L.lograst_eval_scratch_bytes(0, 8, 8) == 0 and L.lograst_eval_scratch_bytes(5, 8, 8) == 0
    assert L.lograst_eval_scratch_bytes(3, 0, 8) == 0 and L.lograst_eval_scratch_bytes(3, 8, -1) == 0


def test_argument_validation_without_gpu():
    from log_amd import _lib
    L = _lib.lib()
    s = (ctypes.c_int64 * 3)(64 * 48, 64, 1)
    one = ctypes.c_void_p(16)             # a non-NULL, aligned address nobody dereferences: every call below is refused first
    need = L.lograst_eval_scratch_bytes(3, 48, 64)
    met = lambda C, H, W, p=one, ps=s, g=one, gs=s, flags=3, rec=one, scr=one, n=need: L.lograst_eval_metrics(
        C, H, W, p, ps, g, gs, flags, 1.0, None, None, rec, scr, n, None)
    bgr = lambda C, H, W, p=one, ps=s, out=one: L.lograst_image_to_bgr8(C, H, W, p, ps, out, None)
    err = lambda: L.lograst_last_error()
    for C in (0, 5, -1):
        assert met(C, 48, 64) < 0 and b"1..4" in err()
        assert bgr(C, 48, 64) < 0 and b"1..4" in err()
    for H, W in ((0, 64), (48, 0), (-3, 64)):
        assert met(3, H, W) < 0 and b"at least 1" in err()
        assert bgr(3, H, W) < 0 and b"at least 1" in err()
    assert met(3, 48, 64, p=None) < 0 and b"NULL" in err()
    assert met(3, 48, 64, ps=None) < 0 and b"NULL" in err()
    assert met(3, 48, 64, g=None) < 0 and b"NULL" in err()
    assert met(3, 48, 64, gs=None) < 0 and b"NULL" in err()
    assert met(3, 48, 64, rec=None) < 0 and b"NULL" in err()
    assert bgr(3, 48, 64, p=None) < 0 and b"NULL" in err()
    assert bgr(3, 48, 64, ps=None) < 0 and b"NULL" in err()
    assert bgr(3, 48, 64, out=None) < 0 and b"NULL" in err()
    assert bgr(3, 48, 64, out=ctypes.c_void_p(18)) < 0 and b"4-byte aligned" in err()
    assert met(3, 48, 64, rec=ctypes.c_void_p(20)) < 0 and b"8-byte aligned" in err()
    assert met(3, 48, 64, flags=4) < 0 and b"flag" in err()
    assert met(3, 48, 64, n=need - 1) < 0 and b"scratch too small" in err()
    assert met(3, 48, 64, scr=None) < 0 and b"scratch too small" in err()
    assert met(3, 32768, 32768) < 0 and b"2^31" in err()
    far = (ctypes.c_int64 * 3)(1, 2 ** 26, 1)                     # a plane whose last row starts beyond 32-bit offsets
    assert met(3, 48, 64, ps=far) < 0 and b"strides" in err()
    assert met(3, 48, 64, gs=far) < 0 and b"strides" in err()
    assert bgr(3, 48, 64, ps=far) < 0 and b"strides" in err()
    assert L.lograst_eval_read(None, (ctypes.c_double * 16)(), None) < 0 and b"NULL" in err()
    assert L.lograst_eval_read(one, None, None) < 0 and b"NULL" in err()
    assert L.lograst_version() == 4 and _lib.NUM_KERNEL_SLOTS == 23


def test_no_cpu_fallback():
    from log_amd import _lib, evaluate
    img = lambda: torch.rand(3, 8, 9)
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        evaluate.image_to_bgr8(img())
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        evaluate.validation_metrics(img(), img(), fit_gain=True, ssim=True)


def test_dropins_hand_cpu_tensors_to_what_they_replaced_and_count_it():
    from log_amd import evaluate
    calls = []
    stand_in = lambda name, value: lambda *a, **k: (calls.append((name, a, k)), value)[1]
    a, b = torch.rand(3, 8, 9), torch.rand(3, 8, 9)
    me = types.SimpleNamespace()
    evaluate.reset_stats()
    with evaluate.dropins.substituted(psnr=stand_in("psnr", 1.5), ssim=stand_in("ssim", 0.25), tensor_to_bgr=stand_in("bgr", "vis"),
                                      make_validation=stand_in("mv", None)):
        assert evaluate.psnr(a, b) == 1.5
        assert evaluate.ssim(a.permute(1, 2, 0), b.permute(1, 2, 0), 1.0) == 0.25
        assert evaluate.ssim(a, b, 1.0, filter_size=7) == 0.25
        assert evaluate.tensor_to_bgr(a) == "vis"
    assert [c[0] for c in calls] == ["psnr", "ssim", "ssim", "bgr"]
    assert calls[0][1][0] is a and calls[0][1][1] is b and calls[2][2] == {"filter_size": 7}      # the caller's own arguments
    st = evaluate.stats()
    assert st["calls"] == {"psnr": 1, "ssim": 2, "tensor_to_bgr": 1}
    assert st["fallbacks"] == {("psnr", "tensors are not on the GPU"): 1, ("ssim", "tensors are not on the GPU"): 1,
                               ("ssim", "another window than 11 taps of sigma 1.5, or other k1 / k2"): 1,
                               ("tensor_to_bgr", "tensors are not on the GPU"): 1}
    assert st["readbacks"] == {}
    # make_validation: the stand-in trainer renders CPU images, so the whole method goes to the original
    module = types.ModuleType("stand_in_trainer")
    module.prepare_batch, module.cv2 = (lambda data, device: data), types.SimpleNamespace(imwrite=None)
    sys.modules[module.__name__] = module
    try:
        class Model:
            view_correction, num_points = None, 0
            eval = train = clear = lambda self: None

        class Render:
            background = torch.ones(3)
            vis = lambda self, batch, model, background=None: {"render": a[None]}
            process_pred = lambda self, batch, pred: pred
            process_gt = lambda self, batch: b[None]

        Trainer = type("Trainer", (), {"__module__": module.__name__})
        me = Trainer()
        me.model, me.render_val, me.lpips, me.device, me.exp, me.val = Model(), Render(), None, "cpu", "unused", [{}]
        evaluate.reset_stats()
        with evaluate.dropins.substituted(make_validation=stand_in("mv", "original ran")):
            assert evaluate.make_validation(me, 7, visualize=True) == "original ran"
        assert calls[-1] == ("mv", (me, 7), {"visualize": True})
        assert evaluate.stats()["fallbacks"] == {("make_validation", "tensors are not on the GPU"): 1}
    finally:
        del sys.modules[module.__name__]
        evaluate.reset_stats()


def test_a_staticmethod_target_stays_one(monkeypatch):
    """DropIns.install / uninstall put functions with a plain setattr; BaseRender.tensor_to_bgr is a staticmethod and is
    called on instances (self.render.tensor_to_bgr(vis)): it must not become an instance method, installed or restored."""
    from log_amd import evaluate

    class BaseRender:
        @staticmethod
        def tensor_to_bgr(tensor):
            return ("original", tensor)

    class Trainer:
        def make_validation(self, iteration, visualize=False):
            return "original"

    metric = types.SimpleNamespace(psnr=lambda a, b: "psnr", ssim=lambda a, b, m: "ssim")
    originals = (metric.psnr, metric.ssim, BaseRender.tensor_to_bgr, Trainer.make_validation)
    fresh = evaluate.DropIns("evaluate", lambda: {"psnr": (metric, "psnr"), "ssim": (metric, "ssim"),
                                                  "tensor_to_bgr": (BaseRender, "tensor_to_bgr"),
                                                  "make_validation": (Trainer, "make_validation")})
    fresh._ours.update(evaluate.dropins._ours)
    fresh.install()
    assert isinstance(BaseRender.__dict__["tensor_to_bgr"], staticmethod) and BaseRender.tensor_to_bgr is evaluate.tensor_to_bgr
    assert not isinstance(Trainer.__dict__["make_validation"], staticmethod) and Trainer.make_validation is evaluate.make_validation
    assert metric.psnr is evaluate.psnr and metric.ssim is evaluate.ssim
    with fresh.substituted():
        pass
    t = torch.rand(3, 4, 5)
    saved = fresh.original("tensor_to_bgr")
    assert saved(t) == ("original", t)
    fresh.uninstall()
    assert isinstance(BaseRender.__dict__["tensor_to_bgr"], staticmethod)
    assert BaseRender().tensor_to_bgr(t) == ("original", t) and BaseRender.tensor_to_bgr(t) == ("original", t)
    assert (metric.psnr, metric.ssim, BaseRender.tensor_to_bgr, Trainer.make_validation) == originals
    assert Trainer().make_validation(1) == "original"
    # a target module that cannot be imported is left out, the others are installed
    partial = evaluate.DropIns("evaluate", lambda: {"psnr": (metric, "psnr"), "ssim": (metric, "ssim")})
    partial._ours.update(evaluate.dropins._ours)
    assert set(partial.install()) == {"psnr", "ssim"} and metric.psnr is evaluate.psnr
    partial.uninstall()
    assert (metric.psnr, metric.ssim) == originals[:2]


@pytest.fixture()
def reference_modules():
    """The reference importable with cv2 and tensorboardX stubbed (absent here); what the test installs is put back."""
    added = REF not in sys.path
    if added:
        sys.path.insert(0, REF)
    stubs = {}
    if "cv2" not in sys.modules:
        stubs["cv2"] = types.ModuleType("cv2")
    if "tensorboardX" not in sys.modules:
        stubs["tensorboardX"] = types.ModuleType("tensorboardX")
        stubs["tensorboardX"].SummaryWriter = object
    sys.modules.update(stubs)
    yield
    from log_amd import evaluate
    evaluate.uninstall()
    for k in stubs:
        sys.modules.pop(k, None)
    if added:
        sys.path.remove(REF)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")
def test_install_on_the_reference_and_back(reference_modules):
    from log_amd import evaluate
    import LoG.utils.metric as metric
    from LoG.render.renderer import BaseRender
    from LoG.utils.trainer import Trainer
    originals = (metric.psnr, metric.ssim, BaseRender.tensor_to_bgr, Trainer.make_validation)
    targets = evaluate.install()
    assert set(targets) == {"psnr", "ssim", "tensor_to_bgr", "make_validation"}
    assert (metric.psnr, metric.ssim, Trainer.make_validation) == (evaluate.psnr, evaluate.ssim, evaluate.make_validation)
    assert isinstance(BaseRender.__dict__["tensor_to_bgr"], staticmethod) and BaseRender.tensor_to_bgr is evaluate.tensor_to_bgr
    evaluate.install()                                            # a second call keeps the saved originals
    # CPU tensors reach the reference's own code, through an instance as the trainer calls it
    c = CASES["33x65"]
    pred, gt = torch.from_numpy(c["pred"]), torch.from_numpy(c["gt"])
    evaluate.reset_stats()
    assert np.array_equal(BaseRender().tensor_to_bgr(pred), c["bgr_pred"])
    assert metric.psnr(pred, gt) == float(c["psnr"])
    assert metric.ssim(pred.permute(1, 2, 0), gt.permute(1, 2, 0), 1.0) == float(c["ssim"])
    assert sum(evaluate.stats()["fallbacks"].values()) == 3
    evaluate.uninstall()
    assert (metric.psnr, metric.ssim, BaseRender.tensor_to_bgr, Trainer.make_validation) == originals
    assert isinstance(BaseRender.__dict__["tensor_to_bgr"], staticmethod)
    assert np.array_equal(BaseRender().tensor_to_bgr(pred), c["bgr_pred"])
    evaluate.reset_stats()


def test_install_all_has_the_switch_and_it_is_off():
    import inspect
    import log_amd
    assert inspect.signature(log_amd.install_all).parameters["device_evaluate"].default is False

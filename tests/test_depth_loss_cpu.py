"""CPU checks of the fused depth patch loss (log_amd/depth_loss.py, lograst_depth_loss_*): the restatement the GPU tests
measure against (tests/depth_loss_ref.py) is itself held to the reference's float64 results
(tests/golden/depth_loss_*.npz, written by tests/golden/make_golden_depth_loss.py from LoG's own
ScaleAndShiftInvariantLoss), and in fp32 to the reference's fp32 results; the sizing helper, argument validation and the
no-CPU-fallback rule work without a GPU; install_all(fused_depth_loss=...) patches what it says and falls through on CPU."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from depth_loss_ref import depth_loss_ref, load_case, rel_l2  # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "depth_loss_*.npz")))
IDS = [os.path.basename(p)[11:-4] for p in GOLDEN]
REF = os.environ.get("LOG_REFERENCE", "/root/reference")


def test_all_cases_present():
    assert set(IDS) == {"smooth", "allmask", "uniform", "half", "nearly_const", "edges", "one_pixel", "empty"}
    for p in GOLDEN:
        assert os.path.getsize(p) < 400 * 1000, p
        c = load_case(p)
        H, W = c["pred"].shape
        assert H <= 96 and W <= 128 and c["gt"].shape == (H, W) and c["acc"].shape == (H, W)
        assert c["pred"].dtype == torch.float32 and c["rows"].dtype == torch.int64
        assert int(c["rows"].min()) >= 0 and int(c["rows"].max()) <= H - 64
        assert int(c["cols"].min()) >= 0 and int(c["cols"].max()) <= W - 64


def test_fixtures_hold_the_cases_they_are_named_for():
    by = {n: load_case(p) for n, p in zip(IDS, GOLDEN)}
    counts = lambda c: [int((c["acc"][r:r + 64, k:k + 64] > 0.5).sum()) for r, k in zip(c["rows"].tolist(), c["cols"].tolist())]
    half = counts(by["half"])
    # empty patches, narrow valid strips and nearly full ones (a start column is at most 63, so at most columns 70..126)
    assert 0 in half and any(0 < v <= 64 * 8 for v in half) and max(half) == 64 * 57
    one = counts(by["one_pixel"])
    assert one[0] == 1 and 0 in one and 4096 in one
    assert by["edges"]["pred"].shape == (65, 65) and sorted(zip(by["edges"]["rows"].tolist(), by["edges"]["cols"].tolist())) == [(0, 0), (0, 1), (1, 1)]
    assert float(by["nearly_const"]["gap32_grad"]) > 0.5         # the reference's own fp32 run is lost there
    assert set(counts(by["empty"])) == {0} and set(counts(by["allmask"])) == {4096}


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_restatement_against_reference_float64(path):
    """The same formulas on the same numbers in float64: only the summation order differs (torch.sum over [n, 64, 64] in
    both; autograd in both), so 1e-12 relative leaves four digits over float64 round-off for the conditioning of the
    2 x 2 solve on the nearly constant fixture."""
    c = load_case(path)
    r = depth_loss_ref(c["pred"], c["gt"], c["acc"], c["rows"], c["cols"])
    if "grad64" not in c:
        assert np.isnan(r["loss"]) and np.isnan(float(c["loss64"])) and np.isnan(float(c["loss32"])) and r["M"] == 0.0
        return
    e_loss = abs(r["loss"] - float(c["loss64"])) / abs(float(c["loss64"]))
    e_grad = rel_l2(r["grad"], torch.from_numpy(c["grad64"]))
    print(f"loss rel {e_loss:.3e}   grad rel-L2 {e_grad:.3e}")
    assert e_loss <= 1e-12 and e_grad <= 1e-12


def _fp32_is_a_yardstick(path):
    z = np.load(path)
    return "gap32_grad" in z.files and float(z["gap32_grad"]) < 1e-3


FP32_CASES = [p for p in GOLDEN if _fp32_is_a_yardstick(p)]


@pytest.mark.parametrize("path", FP32_CASES, ids=[os.path.basename(p)[11:-4] for p in FP32_CASES])
def test_restatement_in_fp32_is_the_references_arithmetic(path):
    """Where the reference's fp32 run is meaningful (gap32_grad < 1e-3), the restatement in fp32 lands as close to float64
    as the reference's fp32 run does, within a factor 4: it is the reference's arithmetic, not only its limit."""
    c = load_case(path)
    assert {"smooth", "uniform", "half", "edges", "one_pixel"} <= {os.path.basename(p)[11:-4] for p in FP32_CASES}
    r = depth_loss_ref(c["pred"], c["gt"], c["acc"], c["rows"], c["cols"], dtype=torch.float32)
    e_loss = abs(r["loss"] - float(c["loss64"]))
    e_grad = rel_l2(r["grad"], torch.from_numpy(c["grad64"]))
    print(f"loss {e_loss:.3e} <= 4 * {float(c['gap32_loss']):.3e}   grad {e_grad:.3e} <= 4 * {float(c['gap32_grad']):.3e}")
    assert e_loss <= 4 * float(c["gap32_loss"]) and e_grad <= 4 * float(c["gap32_grad"])


def test_empty_fixture_is_nan():
    c = load_case(GOLDEN[IDS.index("empty")])
    for dtype in (torch.float32, torch.float64):
        assert np.isnan(depth_loss_ref(c["pred"], c["gt"], c["acc"], c["rows"], c["cols"], dtype=dtype)["loss"])


def test_record_sizing_by_hand():
    from log_amd import _lib
    L = _lib.lib()
    # a header and one record per patch, 16 doubles = 128 bytes each
    assert L.lograst_depth_loss_record_bytes(64) == 65 * 128 == 8320
    assert L.lograst_depth_loss_record_bytes(1) == 256
    assert L.lograst_depth_loss_record_bytes(256) == 257 * 128 == 32896
    assert L.lograst_depth_loss_record_bytes(0) == 0 and L.lograst_depth_loss_record_bytes(-3) == 0


def test_argument_validation_without_gpu():
    from log_amd import _lib
    L = _lib.lib()
    s = (ctypes.c_int64 * 2)(128, 1)
    one = ctypes.c_void_p(8)              # a non-NULL, aligned address nobody dereferences: every call below is refused first
    fwd = lambda H, W, p, n, rows, out, rec, nbytes: L.lograst_depth_loss_forward(
        H, W, p, s, p, s, p, s, n, rows, rows, 0.5, 1e-5, 0.5, out, rec, nbytes, None)
    bwd = lambda H, W, p, n, rec, gl, gp: L.lograst_depth_loss_backward(H, W, p, s, p, s, p, s, n, rec, gl, gp, None)
    for H, W in ((63, 128), (128, 63)):
        assert fwd(H, W, None, 64, None, None, None, 0) < 0 and b"64-pixel patch" in L.lograst_last_error()
        assert bwd(H, W, None, 64, None, None, None) < 0 and b"64-pixel patch" in L.lograst_last_error()
    assert fwd(-1, 128, None, 64, None, None, None, 0) < 0 and b"negative" in L.lograst_last_error()
    for n in (0, -1, 257):
        assert fwd(96, 128, None, n, None, None, None, 0) < 0 and b"1..256" in L.lograst_last_error()
        assert bwd(96, 128, None, n, None, None, None) < 0 and b"1..256" in L.lograst_last_error()
    assert fwd(96, 128, None, 64, None, None, None, 0) < 0 and b"NULL" in L.lograst_last_error()
    assert fwd(96, 128, one, 64, None, None, None, 0) < 0 and b"NULL" in L.lograst_last_error()
    assert bwd(96, 128, None, 64, None, None, None) < 0 and b"NULL" in L.lograst_last_error()
    assert bwd(96, 128, one, 64, one, None, None) < 0 and b"NULL" in L.lograst_last_error()
    need = L.lograst_depth_loss_record_bytes(64)
    assert fwd(96, 128, one, 64, one, one, one, need - 1) < 0 and b"records too small" in L.lograst_last_error()
    assert fwd(96, 128, one, 64, one, one, None, need) < 0 and b"records too small" in L.lograst_last_error()
    assert L.lograst_version() == 4


def test_kernel_slot_list_is_unchanged():
    from log_amd import _lib
    L = _lib.lib()
    names = [L.lograst_kernel_name(i) for i in range(_lib.NUM_KERNEL_SLOTS)]
    assert _lib.NUM_KERNEL_SLOTS == 23 and names[-1] == b"recolor" and names[-3:-1] == [b"loss_fwd", b"loss_bwd"]
    assert not any(b"depth" in n for n in names)


def test_no_cpu_fallback():
    from log_amd import _lib, depth_loss
    img = lambda: torch.rand(80, 80)
    rows = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        depth_loss.depth_patch_loss(img().requires_grad_(True), img(), img(), rows, rows)
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        depth_loss.append_depth_loss(img()[None], img()[None], {"accmap": img()[None], "loss": 0, "loss_dict": {}})


@pytest.fixture()
def log_path():
    """The reference importable (cv2 stubbed: only its visualisation helpers use it); everything this file's test assigns
    onto the reference's classes is put back afterwards, so the tests that follow see the classes as they were."""
    import types
    added = REF not in sys.path
    if added:
        sys.path.insert(0, REF)
    stubs = {}
    if "cv2" not in sys.modules:
        stubs["cv2"] = types.ModuleType("cv2")
    sys.modules.update(stubs)
    old_radius = sys.modules.get("LoG.cuda.compute_radius")
    import log_amd
    log_amd.install_compute_radius()                      # level_of_gaussian.py imports it at import time
    from LoG.model.tensor_tree import TensorTree
    from LoG.model.counter import Counter
    from LoG.model.sparse_optimizer import SparseOptimizer
    from LoG.model.level_of_gaussian import LoG
    import LoG.render.renderer as ref_renderer
    saved = (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict,
             LoG.get_all, ref_renderer.torch)
    yield
    from log_amd import depth_loss, loss
    depth_loss.uninstall()
    loss.uninstall()
    (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
     ref_renderer.torch) = saved
    if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
        del SparseOptimizer._lograst_load_state_dict
    if old_radius is not None:
        sys.modules["LoG.cuda.compute_radius"] = old_radius
    else:
        sys.modules.pop("LoG.cuda.compute_radius", None)
    for k in stubs:
        sys.modules.pop(k, None)
    if added:
        sys.path.remove(REF)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")
def test_install_all_patches_the_depth_loss_only_when_asked(log_path):
    import log_amd
    from log_amd import depth_loss, loss
    from LoG.render.renderer import MaskForeground, NaiveRendererAndLoss
    original = NaiveRendererAndLoss.append_depth_loss
    log_amd.install_all()
    assert NaiveRendererAndLoss.append_depth_loss is original
    log_amd.install_all(fused_loss=True)
    assert NaiveRendererAndLoss.append_depth_loss is original
    loss.uninstall()
    log_amd.install_all(fused_depth_loss=True)
    patched = NaiveRendererAndLoss.append_depth_loss
    assert patched is not original and patched._lograst_original is original
    assert MaskForeground.append_depth_loss is patched
    assert not hasattr(NaiveRendererAndLoss.calculate_loss, "_lograst_original")      # the photometric loss is its own switch
    log_amd.install_all(fused_depth_loss=True)                # a second call does not wrap the wrapper
    assert NaiveRendererAndLoss.append_depth_loss is patched
    # CPU tensors fall through to the reference's own code: the original's results under the same seed
    g = torch.Generator().manual_seed(3)
    gt, acc = 2.0 + 2.0 * torch.rand(1, 80, 90, generator=g), torch.rand(1, 80, 90, generator=g)
    pred = 2.0 + 2.0 * torch.rand(1, 80, 90, generator=g)
    r = NaiveRendererAndLoss(split="train", use_origin_render=False, background=[1., 1., 1.], render_depth=True)
    outs = []
    for fn in (lambda *a: r.append_depth_loss(*a), lambda *a: original(r, *a)):
        p = pred.clone().requires_grad_(True)
        out = {"accmap": acc, "loss": torch.zeros(()), "loss_dict": {}}
        torch.manual_seed(11)
        fn(gt, p, out)
        out["loss"].backward()
        outs.append((out, p.grad))
    (a, ga), (b, gb) = outs
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["loss_dict"]["depth"], b["loss_dict"]["depth"])
    assert torch.equal(a["pred_depth"], b["pred_depth"]) and torch.equal(a["gt_depth"], b["gt_depth"]) and torch.equal(ga, gb)
    depth_loss.uninstall()
    assert NaiveRendererAndLoss.append_depth_loss is original

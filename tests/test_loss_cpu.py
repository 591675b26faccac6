"""CPU checks of the fused L1 + SSIM loss (log_amd/loss.py, lograst_loss_*): the float64 restatement the GPU tests
measure against (tests/loss_ref.py) is itself held to the reference's float64 results (tests/golden/loss_*.npz, written
by tests/golden/make_golden_loss.py from LoG's own SSIM + L1Loss); the sizing helper, argument validation and the
no-CPU-fallback rule work without a GPU; install_all(fused_loss=...) patches what it says and falls through on CPU."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_ref  # noqa: E402
from loss_ref import load_case, rel_l2  # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "loss_*.npz")))
REF = os.environ.get("LOG_REFERENCE", "/root/reference")
C1, C2 = 0.01 ** 2, 0.03 ** 2
EPS64 = 2.0 ** -53


def test_all_cases_present():
    names = {os.path.basename(p)[5:-4] for p in GOLDEN}
    assert names == {"1x11x11", "2x37x53", "nhwc_64x96", "correct_40x40", "half_equal_48x48", "low_contrast_40x56",
                     "unclamped_33x45"}
    for p in GOLDEN:
        assert os.path.getsize(p) <= os.path.getsize(os.path.join(HERE, "golden", "train_random_0.npz"))


def test_taps_are_the_librarys():
    from log_amd import loss
    assert torch.equal(loss.window_taps().double(), loss_ref.taps64())
    assert abs(float(loss_ref.taps64().sum()) - 1.0) < 11 * 2.0 ** -25     # 11 roundings to fp32 of a unit sum


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[5:-4] for p in GOLDEN])
def test_restatement_against_reference_float64(path):
    """Two comparisons with the reference's float64 run.

    (a) The restatement evaluated with the REFERENCE's 121 window weights (stored in the fixture) is the same function of
    the same numbers in another summation order: only float64 round-off separates the two.  Bound: each window sum is 121
    products, so at most 121 * 2^-53 relative error per moment (linear accumulation, worst case), of magnitude M^2 with
    M = max(1, max|x|); a moment error e moves ssim_map = (N1/D1) * (N2/D2), |N1/D1| <= 1, |N2/D2| <= 1, by at most
    e * (8/C1 + 12/C2): N1 and D1 each hold 2 products of two means (error <= 4e each), D1 >= C1, so the first factor
    moves by <= 8e/C1; N2 and D2 each hold two variances (a second moment and a product of means, <= 3e each, so <= 6e),
    D2 >= C2, so the second factor moves by <= 12e/C2.  The means (ssim, l1, loss) move by no more than their terms.
    The gradient is a sum of first derivatives of those quotients, whose relative sensitivity to e is one more factor
    1/C1 at worst; it is compared in rel-L2 against 121 * 2^-53 * (8/C1 + 12/C2) / C1 * M^2.

    (b) The restatement with ITS OWN window (exact product of the library's fp32 taps, normalised in double) differs from
    the reference's (fp32-rounded outer product of taps normalised in fp32) by d_ij, a few fp32 ulps per weight; with
    eps = sum|d_ij| every moment moves by at most eps * M^2, so by the same propagation the scalars move by at most
    eps * M^2 * (8/C1 + 12/C2).  For the gradient the worst-case propagation (another 1/C1) is vacuous at fp32-sized d, so
    its yardstick is the reference's own fp32 error: the reference's fp32 run rounds each of its 5 * 121 window products
    to fp32 (half an ulp each) and lands gap32 away from float64; moving every weight by u ulps is 2u times that
    perturbation per product, so the bound is 2 * u * gap32 with u = max|d_ij| in ulps of the weight."""
    c = load_case(path)
    M = max(1.0, float(c["render"].abs().max()), float(c["gt"].abs().max()))
    amp = 8.0 / C1 + 12.0 / C2
    w_ref = torch.from_numpy(c["window"].astype(np.float64))
    w_own = loss_ref.window2d()
    d = (w_ref - w_own).abs()
    eps_w = float(d.sum())
    ulp = torch.from_numpy(np.spacing(c["window"]).astype(np.float64))
    u = float((d / ulp).max())
    assert 0.0 < u < 8.0, u          # "a few fp32 ulps per weight"

    a = loss_ref.loss_ref(c["render"], c["gt"], c["render_l1"], window=w_ref)
    b = loss_ref.loss_ref(c["render"], c["gt"], c["render_l1"])
    bound_a = 121 * EPS64 * amp * M * M
    bound_a_grad = bound_a / C1
    bound_b = eps_w * amp * M * M
    bound_b_grad = 2.0 * u * float(c["gap32_grad_render"])
    for k in ("l1", "ssim", "loss"):
        ea, eb = abs(a[k] - float(c[k + "64"])), abs(b[k] - float(c[k + "64"]))
        print(f"{k}: (a) {ea:.3e} <= {bound_a:.3e}   (b) {eb:.3e} <= {bound_b:.3e}")
        assert ea <= bound_a and eb <= bound_b, (k, ea, eb)
    g64 = torch.from_numpy(c["grad_render64"])
    ga, gb = rel_l2(a["grad_render"], g64), rel_l2(b["grad_render"], g64)
    print(f"grad_render: (a) {ga:.3e} <= {bound_a_grad:.3e}   (b) {gb:.3e} <= {bound_b_grad:.3e}   (u = {u:.2f} ulps, eps = {eps_w:.3e})")
    assert ga <= bound_a_grad and gb <= bound_b_grad
    if c["render_l1"] is not None:
        # the L1 gradient is 0.8 * sign / count in both: exact up to the rounding of one quotient
        for r in (a, b):
            assert rel_l2(r["grad_render_l1"], torch.from_numpy(c["grad_render_l164"])) <= 4 * EPS64
    else:
        assert a["grad_render_l1"] is None


def test_scratch_sizing_by_hand():
    from log_amd import _lib
    L = _lib.lib()
    # 1920x1080, B=1, C=3: outputs 1910 x 1070 -> 60 x 34 tiles of 32 x 32, 3 planes, 2 floats each = 48960 B
    # = 191.25 * 256 -> rounded up to 192 * 256
    assert L.lograst_loss_scratch_bytes(1, 3, 1080, 1920) == 192 * 256 == 49152
    # 37x53, B=2, C=3: outputs 27 x 43 -> 1 x 2 tiles, 6 planes: 12 workgroups * 8 B = 96 B -> 256
    assert L.lograst_loss_scratch_bytes(2, 3, 37, 53) == 256
    # one output pixel
    assert L.lograst_loss_scratch_bytes(1, 3, 11, 11) == 256
    assert L.lograst_loss_scratch_bytes(4, 3, 2160, 3840) == (8 * 120 * 68 * 12 + 255) // 256 * 256


def test_argument_validation_without_gpu():
    from log_amd import _lib
    L = _lib.lib()
    s = (ctypes.c_int64 * 4)(3 * 10 * 64, 10 * 64, 64, 1)
    rc = L.lograst_loss_forward(1, 3, 10, 64, None, s, None, None, None, s, 0.2, 0.8, None, None, None, 0, None)
    assert rc < 0 and b"11-pixel window" in L.lograst_last_error()
    rc = L.lograst_loss_forward(1, 3, 64, 10, None, s, None, None, None, s, 0.2, 0.8, None, None, None, 0, None)
    assert rc < 0 and b"11-pixel window" in L.lograst_last_error()
    rc = L.lograst_loss_backward(1, 3, 10, 64, None, s, None, None, None, s, 0.8, None, None, None, None, None)
    assert rc < 0 and b"11-pixel window" in L.lograst_last_error()
    rc = L.lograst_loss_forward(1, 3, 64, 64, None, s, None, None, None, s, 0.2, 0.8, None, None, None, 0, None)
    assert rc < 0 and b"NULL" in L.lograst_last_error()
    rc = L.lograst_loss_forward(-1, 3, 64, 64, None, s, None, None, None, s, 0.2, 0.8, None, None, None, 0, None)
    assert rc < 0 and b"negative" in L.lograst_last_error()
    names = [L.lograst_kernel_name(i) for i in range(_lib.NUM_KERNELS)]
    assert names[-2:] == [b"loss_fwd", b"loss_bwd"] and names[:3] == [b"compute_radius", b"project", b"scan_tiles"]


def test_no_cpu_fallback():
    from log_amd import _lib, loss
    r = torch.rand(1, 3, 16, 16, requires_grad=True)
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        loss.l1_ssim_loss(r, torch.rand(1, 3, 16, 16))
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        loss.ssim(r, torch.rand(1, 3, 16, 16))


@pytest.fixture()
def log_path():
    """The reference importable (cv2 stubbed: only its visualisation helpers use it); everything install_all() assigns
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
    from log_amd import loss
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
def test_install_all_patches_the_loss_only_when_asked(log_path):
    import log_amd
    from log_amd import loss
    from LoG.render.loss import SSIM
    from LoG.render.renderer import NaiveRendererAndLoss
    ssim_forward, calc = SSIM.forward, NaiveRendererAndLoss.calculate_loss
    log_amd.install_all()
    assert SSIM.forward is ssim_forward and NaiveRendererAndLoss.calculate_loss is calc
    log_amd.install_all(fused_loss=True)
    assert SSIM.forward is not ssim_forward and SSIM.forward._lograst_original is ssim_forward
    assert NaiveRendererAndLoss.calculate_loss._lograst_original is calc
    patched = SSIM.forward
    log_amd.install_all(fused_loss=True)                      # a second call does not wrap the wrapper
    assert SSIM.forward is patched
    # CPU tensors fall through to the reference's own code: exactly the unpatched results
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(2, 3, 24, 31, generator=g), torch.rand(2, 3, 24, 31, generator=g)
    m = SSIM(11, 3)
    assert torch.equal(m(a, b), ssim_forward(m, a, b))
    assert torch.equal(m(a, b, reduce=False), ssim_forward(m, a, b, False))
    r = NaiveRendererAndLoss(split="train", use_origin_render=False, background=[1., 1., 1.])
    out_p, out_o = {}, {}
    r.calculate_loss(b, a.clone().requires_grad_(True), out_p)
    calc(r, b, a.clone().requires_grad_(True), out_o)
    assert torch.equal(out_p["loss"], out_o["loss"]) and out_p["loss_dict"] == out_o["loss_dict"]
    loss.uninstall()
    assert SSIM.forward is ssim_forward and NaiveRendererAndLoss.calculate_loss is calc

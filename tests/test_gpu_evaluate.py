"""The evaluation path on the device (log_amd/evaluate.py over lograst_eval_metrics, lograst_eval_read and
lograst_image_to_bgr8; csrc/evaluate.hip) against the reference's recorded bytes (tests/golden/evaluate_*.npz) and the
float64 restatement (tests/evaluate_ref.py).

Bounds.  8-bit images: bit for bit -- the kernel's conversion is the IEEE operations of numpy's line.  Scalars (l1, the
mean squared error, the mean SSIM, the fitted gain): tools/fuzz_step_ops.py's rule |got - ref64| <= 8 (|ref32 - ref64| +
2^-24 S) with ref32 the restatement run in fp32 as the reference runs and S the mean magnitude of the summed terms; the
corrected image: max |got - ref64| <= 8 (max |ref32 - ref64| + 2^-24) (values in [0, 1]).  Where the float64 result is inf
or nan, so is the kernel's.  Nothing here reads the reference tree."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from evaluate_ref import EPS24, F, evaluate_ref, golden_cases, to_bgr8, within  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = golden_cases()
NAMES = sorted(CASES)
DEV = "cuda"


def _dev(c):
    """-> (pred, gt) on the device; an HWC ground truth stays HWC in memory and is handed over as its [C, H, W] view."""
    pred = torch.from_numpy(c["pred"]).to(DEV)
    gt = torch.from_numpy(c["gt"]).to(DEV)
    return pred, (gt.permute(2, 0, 1) if int(c["gt_hwc"]) else gt)


def _host(c):
    return c["pred"], np.ascontiguousarray(c["gt"].transpose(2, 0, 1) if int(c["gt_hwc"]) else c["gt"])


def _check_scalars(tag, r, r64, r32, fit, ssim):
    rows = [("l1", r.l1, r64["l1"], r32["l1"], r64["l1"]), ("mse", r.mse, r64["mse"], r32["mse"], r64["mse"])]
    if ssim:
        rows.append(("ssim", r.ssim, r64["ssim"], r32["ssim"], r64["ssim_S"]))
    if fit:
        rows += [(f"gain[{i}]", r.gain[i], float(r64["gain"][i]), float(r32["gain"][i]), float(r64["gain_S"][i]))
                 for i in range(len(r.gain))]
    else:
        assert r.gain == [1.0] * len(r.gain)
    for what, got, v64, v32, S in rows:
        ok, err, bound = within(got, v64, v32, S if np.isfinite(S) else 0.0)
        print(f"{tag} {what}: got {got!r} ref64 {v64!r} ref32 {v32!r} err {err:.3g} bound {bound:.3g}")
        assert ok, (tag, what, got, v64, v32, err, bound)
    if np.isfinite(r64["mse"]):
        assert r.psnr == (np.inf if r.mse == 0 else pytest.approx(-10 * np.log10(r.mse), rel=1e-12))
        assert (r.mse == 0) == (r64["mse"] == 0)
    else:
        assert np.isnan(r.psnr)


def _check_corrected(tag, got, r64, r32):
    c64, c32 = r64["corrected"], r32["corrected"].astype(np.float64)
    nan = np.isnan(c64)
    assert np.array_equal(np.isnan(got), nan), tag
    if nan.all():
        return
    err = np.abs(got.astype(np.float64) - c64)[~nan].max()
    bound = F * (np.abs(c32 - c64)[~nan].max() + EPS24)
    print(f"{tag} corrected: max err {err:.3g} bound {bound:.3g}")
    assert err <= bound, (tag, err, bound)


@pytest.mark.parametrize("name", NAMES)
def test_golden_cases(name):
    from log_amd import evaluate
    c = CASES[name]
    fit, max_val = bool(c["fit"]), float(c["max_val"])
    pred, gt = _dev(c)
    assert np.array_equal(evaluate.image_to_bgr8(pred), c["bgr_pred"])
    assert np.array_equal(evaluate.image_to_bgr8(gt), c["bgr_gt"])
    m = evaluate.validation_metrics(pred, gt, fit_gain=fit, ssim=True, max_val=max_val, corrected=True, bgr8=True)
    r = m.read()
    H = pred.shape[1]
    vis, corrected = m.bgr8_host(), m.corrected.cpu().numpy()
    assert vis.shape == c["mv_vis"].shape and vis.dtype == np.uint8
    assert np.array_equal(vis[H:], c["bgr_gt"]) and np.array_equal(vis[H:], c["mv_vis"][H:])
    mine = to_bgr8(corrected)
    keep = ~np.isnan(corrected.transpose(1, 2, 0)[:, :, ::-1])         # a nan's byte is unspecified
    assert np.array_equal(vis[:H][keep], mine[keep])
    if not fit:
        assert np.array_equal(corrected, c["pred"]) and np.array_equal(vis, c["mv_vis"])
    else:
        print(f"{name}: {int((vis[:H] != c['mv_vis'][:H])[keep].sum())} of {int(keep.sum())} corrected bytes differ from the reference's")
    hp, hg = _host(c)
    r64 = evaluate_ref(hp, hg, fit_gain=fit, ssim=True, max_val=max_val)
    r32 = evaluate_ref(hp, hg, fit_gain=fit, ssim=True, max_val=max_val, dtype=np.float32)
    _check_scalars(name, r, r64, r32, fit, True)
    _check_corrected(name, corrected, r64, r32)
    assert r.raw[3] == pred.numel()
    # the same launch without the SSIM and without the optional outputs: the other sums do not move
    r2 = evaluate.validation_metrics(pred, gt, fit_gain=fit).read()
    assert r2.ssim is None and r2.raw[2] == 0.0
    same = lambda a, b: np.array_equal(np.array(a), np.array(b), equal_nan=True)
    assert same(r2.raw[:2], r.raw[:2]) and same(r2.raw[3:], r.raw[3:])


def _random_pair(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(C, H, W, generator=g)
    pred = (0.7 * gt + 0.1 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
    return pred, gt


def _bits(m):
    return m.record.cpu().numpy().tobytes()


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channel_counts(C):
    from log_amd import evaluate
    pred, gt = _random_pair(C, 45, 70, 100 + C)
    m = evaluate.validation_metrics(pred.to(DEV), gt.to(DEV), fit_gain=True, ssim=True, corrected=True, bgr8=True)
    r64 = evaluate_ref(pred.numpy(), gt.numpy(), fit_gain=True, ssim=True)
    r32 = evaluate_ref(pred.numpy(), gt.numpy(), fit_gain=True, ssim=True, dtype=np.float32)
    _check_scalars(f"C={C}", m.read(), r64, r32, True, True)
    corrected = m.corrected.cpu().numpy()
    _check_corrected(f"C={C}", corrected, r64, r32)
    assert np.array_equal(m.bgr8_host(), to_bgr8(np.concatenate([corrected, gt.numpy()], axis=1)))
    assert np.array_equal(evaluate.image_to_bgr8(pred.to(DEV)), to_bgr8(pred.numpy()))
    assert m.read().raw[4 + C:8] == (0.0,) * (4 - C)


def test_strided_inputs_give_the_bits_of_their_contiguous_copies():
    from log_amd import evaluate
    pred, gt = _random_pair(3, 50, 84, 7)
    pred, gt = pred.to(DEV), gt.to(DEV)
    base = evaluate.validation_metrics(pred, gt, fit_gain=True, ssim=True, corrected=True, bgr8=True)
    hwc = gt.permute(1, 2, 0).contiguous().permute(2, 0, 1)                   # an HWC image, read in place
    wide = torch.rand(3, 50, 100, device=DEV)
    wide[:, :, 9:93] = pred                                                   # a column slice: rows 100 apart, odd start
    views = {"hwc gt": (pred, hwc), "sliced pred": (wide[:, :, 9:93], gt), "both": (wide[:, :, 9:93], hwc),
             "transposed": (pred.transpose(1, 2).contiguous().transpose(1, 2), gt)}
    for tag, (p, g) in views.items():
        assert not (p.is_contiguous() and g.is_contiguous())
        m = evaluate.validation_metrics(p, g, fit_gain=True, ssim=True, corrected=True, bgr8=True)
        assert _bits(m) == _bits(base), tag
        assert torch.equal(m.corrected, base.corrected) and torch.equal(m.bgr8, base.bgr8), tag
        assert np.array_equal(evaluate.image_to_bgr8(p), evaluate.image_to_bgr8(pred)), tag
        assert np.array_equal(evaluate.image_to_bgr8(g), evaluate.image_to_bgr8(gt)), tag
    # the 16-byte path of the export (contiguous, W a multiple of 4) against the scalar path on the same numbers
    assert np.array_equal(evaluate.image_to_bgr8(pred), to_bgr8(pred.cpu().numpy()))
    odd = pred[:, :, 1:]                                                      # W = 83, rows off 16-byte alignment
    assert np.array_equal(evaluate.image_to_bgr8(odd), to_bgr8(odd.cpu().numpy()))
    assert np.array_equal(evaluate.image_to_bgr8(pred), evaluate.image_to_bgr8(pred).copy())


@pytest.fixture(scope="module")
def full_hd():
    pred, gt = _random_pair(3, 1080, 1920, 1080)
    return pred, gt, evaluate_ref(pred.numpy(), gt.numpy(), fit_gain=True), evaluate_ref(pred.numpy(), gt.numpy(), fit_gain=True,
                                                                                       dtype=np.float32)


def test_full_hd_and_two_runs_give_the_same_bits(full_hd):
    """1080 x 1920: 34 x 60 tiles per channel, 254 workgroups of the fit per channel, more partial sums than the reducing
    workgroup has threads, the export's 16-byte path.  The SSIM of this size is measured where it is cheap to state: the
    top-left 96 x 128 corner as an image of its own against the restatement, and run-to-run bits for the whole image."""
    from log_amd import evaluate
    pred, gt, r64, r32 = full_hd
    dp, dg = pred.to(DEV), gt.to(DEV)
    a = evaluate.validation_metrics(dp, dg, fit_gain=True, ssim=True, corrected=True, bgr8=True)
    b = evaluate.validation_metrics(dp, dg, fit_gain=True, ssim=True, corrected=True, bgr8=True)
    assert _bits(a) == _bits(b) and torch.equal(a.corrected, b.corrected) and torch.equal(a.bgr8, b.bgr8)
    r = a.read()
    _check_scalars("1080p", r, r64, r32, True, False)
    corrected = a.corrected.cpu().numpy()
    _check_corrected("1080p", corrected, r64, r32)
    assert np.array_equal(a.bgr8_host(), to_bgr8(np.concatenate([corrected, gt.numpy()], axis=1)))
    assert np.array_equal(evaluate.image_to_bgr8(dp), to_bgr8(pred.numpy()))
    assert 0.0 < r.ssim < 1.0
    cp, cg = pred[:, :96, :128], gt[:, :96, :128]
    m = evaluate.validation_metrics(dp[:, :96, :128], dg[:, :96, :128], ssim=True)
    _check_scalars("1080p corner", m.read(), evaluate_ref(cp.numpy(), cg.numpy(), ssim=True),
                   evaluate_ref(cp.numpy(), cg.numpy(), ssim=True, dtype=np.float32), False, True)


def test_bad_arguments_raise():
    from log_amd import evaluate
    img = torch.rand(3, 8, 9, device=DEV)
    with pytest.raises(ValueError):
        evaluate.validation_metrics(img, img[:, :, :8])
    with pytest.raises(ValueError):
        evaluate.validation_metrics(img.double(), img.double())
    with pytest.raises(ValueError):
        evaluate.image_to_bgr8(torch.rand(5, 8, 9, device=DEV))


def test_metric_dropins_on_the_device():
    """psnr, ssim and tensor_to_bgr as LoG calls them (ssim channels-last), and what they hand back to the original."""
    from log_amd import evaluate
    c = CASES["33x65"]
    pred, gt = _dev(c)
    hp, hg = _host(c)
    r64 = evaluate_ref(hp, hg, ssim=True)
    calls = []
    original = lambda name: lambda *a, **k: calls.append(name) or name
    evaluate.reset_stats()
    with evaluate.dropins.substituted(psnr=original("psnr"), ssim=original("ssim"), tensor_to_bgr=original("bgr")):
        assert evaluate.psnr(pred, gt) == pytest.approx(r64["psnr"], abs=1e-4)
        assert evaluate.psnr(pred.permute(1, 2, 0), gt.permute(1, 2, 0)) == pytest.approx(r64["psnr"], abs=1e-4)
        last = pred.permute(1, 2, 0).contiguous(), gt.permute(1, 2, 0).contiguous()
        s = evaluate.ssim(last[0][None], last[1][None], 1.0)
        assert s == evaluate.validation_metrics(pred, gt, ssim=True).read().ssim
        assert np.array_equal(evaluate.tensor_to_bgr(pred), c["bgr_pred"])
        assert calls == []
        assert evaluate.psnr(pred.double(), gt.double()) == "psnr"
        assert evaluate.psnr(pred, gt[:, :, :-1]) == "psnr"
        assert evaluate.ssim(torch.stack(last[:1] * 2), torch.stack(last[1:] * 2), 1.0) == "ssim"
        assert evaluate.ssim(last[0], last[1], 1.0, filter_sigma=2.0) == "ssim"
        assert evaluate.tensor_to_bgr(torch.rand(5, 8, 9, device=DEV)) == "bgr"
        assert evaluate.tensor_to_bgr(pred.half()) == "bgr"
    st = evaluate.stats()
    assert st["readbacks"] == {"psnr": 2, "ssim": 1, "tensor_to_bgr": 1}
    assert sorted(k[0] for k in st["fallbacks"]) == ["psnr", "psnr", "ssim", "ssim", "tensor_to_bgr", "tensor_to_bgr"]
    evaluate.reset_stats()


@pytest.mark.parametrize("fit", [False, True], ids=["plain", "view_correction"])
def test_make_validation_without_the_reference(fit, tmp_path, capsys):
    """The drop-in of Trainer.make_validation on stand-in trainer, model and renderer objects: what it logs is
    validation_metrics(...).read(), what it writes is bgr8, and it reads back once per image plus once per written image."""
    from log_amd import evaluate
    written, logged, toggles = [], {}, []
    module = types.ModuleType("stand_in_trainer_gpu")
    module.prepare_batch = lambda data, device: {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in data.items()}
    module.cv2 = types.SimpleNamespace(imwrite=lambda name, img: written.append((name, img)))
    sys.modules[module.__name__] = module

    class Model:
        view_correction = object() if fit else None
        num_points = 123
        eval = lambda self: toggles.append("eval")
        train = lambda self: toggles.append("train")
        clear = lambda self: toggles.append("clear")

    class Render:
        background = torch.zeros(3, device=DEV)
        vis = lambda self, batch, model, background=None: {"render": batch["pred"][None].clone(), "bg": background}
        process_pred = lambda self, batch, pred: pred
        process_gt = lambda self, batch: batch["gt"][None]

    images = [_random_pair(3, 37, 53, 11), _random_pair(3, 37, 53, 12)]
    Trainer = type("Trainer", (), {"__module__": module.__name__})
    me = Trainer()
    me.model, me.render_val, me.device, me.exp, me.global_iterations = Model(), Render(), DEV, str(tmp_path), 5
    me.recorder = types.SimpleNamespace(log=lambda step, key, value: logged.__setitem__(key, (step, value)))
    me.val = [{"pred": p, "gt": g, "imgname": [f"dir/img{i}.png"], "index": [i]} for i, (p, g) in enumerate(images)]
    # LPIPS stays a torch module: a stand-in that shows which image it was given
    me.lpips = (lambda a, b, retPerLayer, normalize: (a - b).abs().amax()) if fit else None
    try:
        evaluate.reset_stats()
        with evaluate.dropins.substituted(make_validation=lambda *a, **k: pytest.fail("fell back")):
            evaluate.make_validation(me, 41, visualize=True)
            want = [evaluate.validation_metrics(p.to(DEV), g.to(DEV), fit_gain=fit, corrected=True, bgr8=True) for p, g in images]
            reads = [m.read() for m in want]
            assert logged["val/l1"] == (5, sum(r.l1 for r in reads) / 2) and logged["val/psnr"] == (5, sum(r.psnr for r in reads) / 2)
            if fit:
                assert logged["val/lpips"] == (5, sum(float((m.corrected - g.to(DEV)).abs().amax()) for m, (p, g) in zip(want, images)) / 2)
                assert max(float(m.corrected.max()) for m in want) <= 1.0
            else:
                assert "val/lpips" not in logged
            assert [os.path.relpath(n, str(tmp_path)) for n, _ in written] == [os.path.join("val", "000041", f"{i:06d}_img{i}.png.jpg") for i in range(2)]
            for (_, img), m in zip(written, want):
                assert isinstance(img, np.ndarray) and img.shape == (74, 53, 3) and np.array_equal(img, m.bgr8_host())
            assert written[0][1].ctypes.data != written[1][1].ctypes.data       # an array of its own per call
            assert evaluate.stats()["readbacks"] == {"make_validation": 4} and evaluate.stats()["fallbacks"] == {}
            assert toggles == ["eval", "clear", "clear", "train"]
            out = capsys.readouterr().out
            assert ">>> Validation: 41: 2 images" in out and f"    - l1: {logged['val/l1'][1]:.4f}" in out
            # nothing is written outside a thousandth iteration, and then nothing but the record is read back
            evaluate.reset_stats()
            del written[:]
            evaluate.make_validation(me, 41)
            assert written == [] and evaluate.stats()["readbacks"] == {"make_validation": 2}
            evaluate.make_validation(me, 999)
            assert len(written) == 2
            # an image the kernels do not cover sends the whole call to the original
        me.val = [{"pred": torch.rand(5, 8, 8), "gt": torch.rand(5, 8, 8), "imgname": ["a"], "index": [0]}]
        with evaluate.dropins.substituted(make_validation=lambda *a, **k: "original"):
            assert evaluate.make_validation(me, 3) == "original"
    finally:
        del sys.modules[module.__name__]
        evaluate.reset_stats()

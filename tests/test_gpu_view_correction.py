"""The view correction on the device: the loss kernels with a per-image channel gain (log_amd.loss.l1_ssim_loss(l1_gain=) ->
lograst_loss_forward_gain / _backward_gain), the one-row AMSGrad step (lograst_corrector_step) and the drop-ins of
log_amd.view_correction, against

* today's path (gain = ones: the same bits),
* the reference's own results (tests/golden/view_correction_*.npz, written by tests/golden/make_golden_view_correction.py),
* the float64 restatement tests/view_correction_ref.py (held to those results by tests/test_view_correction_cpu.py) at sizes
  no fixture has.

Tolerances, as in tests/test_gpu_loss.py: the three scalars within 8 * gap32 of float64 (gap32 = the reference's own
fp32-vs-float64 distance, the largest over the fixtures; an input that is no fixture may add its own |fp32 - float64| of the
restatement); grad_render rel-L2 <= min(1e-4, 8 * gap32) against float64.  grad_gain and the step's state are a handful of
numbers with no stable gap32 of their own, so they carry a floor: per element within 8 * (|ref32 - ref64| + 2^-24 * S) of
float64, S the condition scale the restatement returns (l1_scale * sum |render|; tests/step_ref.py: adam)."""
import glob
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import view_correction_ref as vref  # noqa: E402
from loss_ref import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS = sorted(glob.glob(os.path.join(HERE, "golden", "view_correction_loss_*.npz")))
LOSS_IDS = [os.path.basename(p)[len("view_correction_loss_"):-4] for p in LOSS]
STEPS = sorted(glob.glob(os.path.join(HERE, "golden", "view_correction_steps_*.npz")))
STEP_IDS = [os.path.basename(p)[len("view_correction_steps_"):-4] for p in STEPS]
DEV = "cuda:0"
GRAD_TOL, FACTOR = 1e-4, 8.0


def _gaps():
    zs = [np.load(p) for p in LOSS]
    return {k: max(float(z["gap32_" + k]) for z in zs) for k in ("l1", "ssim", "loss")}


def _run(render, gt, gain=None, a=0.2, b=0.8, render_l1=None):
    """-> ((loss, l1, ssim) as 0-dim tensors, grad_render, grad_gain or None)."""
    from log_amd.loss import l1_ssim_loss
    r = render.detach().requires_grad_(True)
    k = None if gain is None else gain.detach().clone().requires_grad_(True)
    loss, l1, ssim = l1_ssim_loss(r, gt, render_l1, a, b, l1_gain=k)
    assert loss.requires_grad and not l1.requires_grad and not ssim.requires_grad and loss.dim() == 0
    loss.backward()
    return (loss.detach(), l1, ssim), r.grad, None if k is None else k.grad


def _pair(B, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.rand(B, 3, max(H // 8, 2), max(W // 8, 2), device=DEV, generator=g, dtype=torch.float64)
    field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    noisy = lambda s: (field + s * torch.randn(field.shape, device=DEV, generator=g, dtype=torch.float64)).clamp(0, 1).float().contiguous()  # noqa: E731
    return noisy(0.05), noisy(0.08)


def _check(tag, got, ref64, ref32, scalar_gaps):
    """got = _run's result; ref64 / ref32: the restatement's or the fixture's dicts (loss, l1, ssim, grad_render, grad_gain,
    gap32_grad_render, S_gain)."""
    scalars, g, gk = got
    for k, t in zip(("loss", "l1", "ssim"), scalars):
        err, bound = abs(float(t) - float(ref64[k])), FACTOR * scalar_gaps[k]
        print(f"{tag} {k}: |{float(t):.9f} - {float(ref64[k]):.9f}| = {err:.3e} <= {bound:.3e}")
        assert err <= bound, (tag, k, err, bound)
    assert torch.isfinite(g).all()
    err, bound = rel_l2(g.cpu(), ref64["grad_render"].cpu()), min(GRAD_TOL, FACTOR * ref64["gap32_grad_render"])
    print(f"{tag} grad_render rel-L2 {err:.3e} <= {bound:.3e}")
    assert err <= bound, (tag, err, bound)
    ok, ratio = vref.within(gk, ref32["grad_gain"], ref64["grad_gain"], ref64["S_gain"], FACTOR)
    print(f"{tag} grad_gain {gk.flatten().tolist()}: error / bound {ratio:.3f}")
    assert ok, (tag, gk, ref64["grad_gain"], ratio)


@pytest.mark.parametrize("shape", [(1, 11, 11), (2, 37, 53), (1, 75, 131)])
def test_gain_of_ones_is_todays_path_bit_for_bit(shape):
    B, H, W = shape
    render, gt = _pair(B, H, W, 100 + H)
    gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)             # the strides LoG passes
    plain = _run(render, gt)
    ones = _run(render, gt, torch.ones(B, 3, device=DEV))
    assert all(torch.equal(x, y) for x, y in zip(plain[0], ones[0])) and torch.equal(plain[1], ones[1])
    # any gain: the SSIM term does not see it
    gain = torch.tensor([[1.1, 0.93, 1.04], [0.88, 1.0, 1.21]], device=DEV)[:B].contiguous()
    other = _run(render, gt, gain)
    assert torch.equal(other[0][2], plain[0][2]) and not torch.equal(other[0][1], plain[0][1])
    # ... and it is the loss with render_l1 = gain * render, the image this path does not build
    twin = _run(render, gt, render_l1=(render * gain[:, :, None, None]))
    assert all(torch.equal(x, y) for x, y in zip(twin[0], other[0]))


@pytest.mark.parametrize("path", LOSS, ids=LOSS_IDS)
def test_golden_cases(path):
    c = vref.load_loss_case(path)
    render, gt, gain = c["render"].to(DEV), c["gt"].to(DEV), c["gain"].to(DEV)
    if "render4" in c:
        render = torch.from_numpy(c["render4"]).to(DEV)[:, :3]
        assert not render.is_contiguous() and gt.stride()[1] == 1
    S = vref.l1_gain(c["render"], vref.gt_for(c, torch.float64), c["gain"])["S_gain"]
    t = lambda k: torch.from_numpy(np.asarray(c[k]))  # noqa: E731
    ref64 = dict(loss=c["loss64"], l1=c["l164"], ssim=c["ssim64"], grad_render=t("grad_render64"), grad_gain=t("grad_gain64"),
                 gap32_grad_render=float(c["gap32_grad_render"]), S_gain=S)
    _check(LOSS_IDS[LOSS.index(path)], _run(render, gt, gain), ref64, dict(grad_gain=t("grad_gain32")), _gaps())
    if "equal_left" in c:
        # gt == fp32(gain * render) on the left half: the L1 term is exactly 0 there (sign(0) = 0) only while the product is
        # rounded to fp32 before gt is subtracted; contracted into an fma it leaves the product's rounding error and a sign
        n = int(c["equal_left"])
        _, only_l1, gk = _run(render, gt, gain, 0.0, 1.0)
        assert float(only_l1[..., :n].abs().max()) == 0.0 and float(only_l1[..., n:].abs().min()) > 0.0
        right = vref.l1_gain(render[..., n:], gt[..., n:], gain, l1_weight=0.5)      # half the pixels: l1_scale of the whole
        ok, ratio = vref.within(gk, right["grad_gain"].float(), right["grad_gain"], right["S_gain"], FACTOR)
        assert ok, (gk, right["grad_gain"], ratio)


def test_more_tiles_per_plane_than_reduction_threads_and_the_same_bits_twice():
    """530 x 530: 17 x 17 = 289 image tiles per plane, more than the 256 threads that add a plane's partial sums of the gain
    gradient, so that some threads take a second partial."""
    from log_amd import loss
    H = W = 530
    tiles = ((H + loss.TILE - 1) // loss.TILE) * ((W + loss.TILE - 1) // loss.TILE)
    assert tiles > loss.GAIN_REDUCE_THREADS
    render, gt = _pair(1, H, W, 7)
    gain = torch.tensor([[1.06, 0.97, 1.02]], device=DEV)
    ref64, ref32 = vref.loss_gain(render, gt, gain), vref.loss_gain(render, gt, gain, dtype=torch.float32)
    ref64["gap32_grad_render"] = rel_l2(ref32["grad_render"].cpu(), ref64["grad_render"].cpu())
    gaps = {k: max(v, abs(ref32[k] - ref64[k])) for k, v in _gaps().items()}
    first = _run(render, gt, gain)
    _check("530x530", first, ref64, ref32, gaps)
    second = _run(render, gt, gain)
    assert all(torch.equal(x, y) for x, y in zip(first[0], second[0]))
    assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])


def test_two_images_give_the_same_bits_twice():
    c = vref.load_loss_case(LOSS[LOSS_IDS.index("2x37x53")])
    render, gt, gain = c["render"].to(DEV), c["gt"].to(DEV), c["gain"].to(DEV)
    a, b = _run(render, gt, gain), _run(render, gt, gain)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # each image's gain gradient is its own plane's sum: the batch of one gives the same numbers scaled by the mean's count
    one = _run(render[:1], gt[:1], gain[:1])
    ok, ratio = vref.within(a[2][:1], 0.5 * one[2], 0.5 * one[2].double(), 0.5 * one[2].abs(), FACTOR)
    assert ok, ratio


def test_graph_capture_replays_the_eager_result():
    from log_amd.loss import l1_ssim_loss
    render, gt = _pair(1, 135, 240, 4)
    gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    gain = torch.tensor([[1.1, 0.93, 1.04]], device=DEV)
    eager = _run(render, gt, gain)
    r, k = render.clone().requires_grad_(True), gain.clone().requires_grad_(True)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):                       # warm-up on the capture stream
        l1_ssim_loss(r, gt, l1_gain=k)[0].backward()
    torch.cuda.synchronize()
    r.grad = k.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        loss, l1, ssim = l1_ssim_loss(r, gt, l1_gain=k)
        loss.backward()
    torch.cuda.synchronize()
    for _ in range(2):
        r.grad.zero_()
        k.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip((loss.detach(), l1, ssim), eager[0]))
        assert torch.equal(r.grad, eager[1]) and torch.equal(k.grad, eager[2])


# ---- the row step ----------------------------------------------------------------------------------------------------

def _launch_step(index, start, lr_init, lr_final, steps, rows):
    from log_amd import _lib
    from log_amd.rasterizer import _ptr, _stream_ptr
    V, C = rows["param"].shape
    _lib.check(_lib.lib().lograst_corrector_step(V, C, index, start, lr_init, lr_final, _ptr(steps),
                                                  *(_ptr(rows[k]) for k in vref.STATE), _stream_ptr(torch.device(DEV))))


@pytest.mark.parametrize("path", STEPS, ids=STEP_IDS)
def test_every_recorded_step_teacher_forced(path):
    """Recorded step t is row t of [T, 3] buffers holding the fixture's fp32 state BEFORE that step: T launches, no closed
    loop on the device, one read-back at the end."""
    z = np.load(path)
    T = len(z["index"])
    start, lr_init, lr_final = int(z["start_step"]), float(z["lr_init"]), float(z["lr_final"])
    rows = {k: torch.from_numpy(z[k + "_before32"]).to(DEV).contiguous() for k in vref.STATE}
    steps = torch.from_numpy(z["steps_before"]).to(DEV)
    for t in range(T):
        _launch_step(t, start, lr_init, lr_final, steps, rows)
    assert np.array_equal(steps.cpu().numpy(), z["steps_after"])                   # exact
    got = {k: v.cpu() for k, v in rows.items()}
    s_after = z["steps_after"] - start
    early = s_after < 0
    assert np.array_equal(got["grad"].numpy()[early], z["grad_before32"][early])   # kept, to the bit
    assert not got["grad"].numpy()[~early].any()                                   # zeroed
    covered = set(int(s) for s in s_after)
    assert ({1, 99, 100, 101} <= covered) if start == 0 else (early.sum() >= 2 and 0 in covered)
    worst = 0.0
    for t in range(T):
        before = vref.step_rows(z, t, "before", "32")
        _, after, S = vref.corrector_step(before, z["steps_before"][t], start, lr_init, lr_final)
        for k in vref.STATE:
            if after is None:                                                      # an early return: nothing else is touched
                assert np.array_equal(got[k][t].numpy(), z[k + "_before32"][t]), (t, k)
                continue
            ok, ratio = vref.within(got[k][t], z[k + "_after32"][t], z[k + "_after64"][t], S[k], FACTOR)
            worst = max(worst, ratio)
            assert ok, (t, k, got[k][t], z[k + "_after32"][t], z[k + "_after64"][t])
    print(f"{T} steps, largest error / bound {worst:.3f}")


# ---- the drop-ins, on stand-ins for the reference's objects ----------------------------------------------------------

class _Corrector:
    """What log_amd.view_correction reads of a Corrector (corrector.py:7-33)."""

    def __init__(self, V, device=DEV, dtype=torch.float32, start_step=0, amsgrad=True):
        self.lr_init, self.lr_final, self.start_step = 0.1, 0.001, start_step
        self.use_view_correction, self.use_amsgrad, self.index = True, amsgrad, None
        self.view_correction = torch.nn.Parameter(torch.ones(V, 3, device=device, dtype=dtype))
        z = lambda: {"view_correction": torch.zeros(V, 3, device=device, dtype=dtype)}  # noqa: E731
        self.optimizer = types.SimpleNamespace(exp_avg=z(), exp_avg_sq=z(), max_exp_avg_sq=z(), use_amsgrad=amsgrad,
                                               steps={"view_correction": torch.zeros(V, dtype=torch.int32, device=device)})

    def state(self):
        o = self.optimizer
        grad = self.view_correction.grad
        return dict(param=self.view_correction.data, grad=None if grad is None else grad, exp_avg=o.exp_avg["view_correction"],
                    exp_avg_sq=o.exp_avg_sq["view_correction"], max_exp_avg_sq=o.max_exp_avg_sq["view_correction"],
                    steps=o.steps["view_correction"])

    def snapshot(self):
        return {k: None if v is None else v.detach().cpu().clone() for k, v in self.state().items()}


def _reference_getitem(self, index):
    self.index = index
    return self.view_correction[index]


def _reference_step(self):
    """The reference's Corrector.step in the words of the restatement (float32, on the host): the count first, then the
    update of row self.index -- a missing gradient raises after the count, as the reference's indexing of None does."""
    st = self.state()
    i = self.index
    st["steps"][[i]] += 1
    if st["grad"] is None:
        raise TypeError("'NoneType' object is not subscriptable")
    row = {k: st[k][i].detach().cpu() for k in vref.STATE}
    _, after, _ = vref.corrector_step(row, int(st["steps"][i]) - 1, self.start_step, self.lr_init, self.lr_final, dtype=row["param"].dtype)
    if after is not None:
        for k in vref.STATE:
            st[k][i] = after[k].to(st[k].device)


class _Renderer:
    """What calculate_loss reads of NaiveRendererAndLoss."""

    def __init__(self):
        self.ssim_loss = types.SimpleNamespace(window_size=11, padding=0)
        self.l1_loss = torch.nn.L1Loss()


def _reference_calculate_loss(self, gt_image, render, output, mask_ignore=None):
    """renderer.py:253-266 on today's fused loss (what log_amd.loss installs there)."""
    from log_amd.loss import l1_ssim_loss
    if mask_ignore is not None:
        render = gt_image * mask_ignore[:, None] + render * (1 - mask_ignore[:, None])
    render_l1 = output["render_correct"][:, :3] if "render_correct" in output else None
    loss, l1, ssim = l1_ssim_loss(render, gt_image, render_l1)
    output["loss_dict"] = {"l1": float(l1), "ssim": float(ssim)}
    output["loss"] = loss


def _vis(cor, render, indices, getitem):
    """renderer.py:243-250: one row handed out per view, render_correct built and stacked."""
    return torch.stack([render[b] * getitem(cor, i)[:, None, None] for b, i in enumerate(indices)])


@pytest.fixture()
def standins():
    from log_amd import view_correction as vc
    vc.reset_stats()
    vc.handed_out.take()
    with vc.dropins.substituted(step=_reference_step, __getitem__=_reference_getitem, calculate_loss=_reference_calculate_loss):
        yield vc
    vc.handed_out.take()
    vc.reset_stats()


@pytest.mark.parametrize("B,masked", [(1, False), (2, False), (2, True)])
def test_hand_over_from_the_corrector_to_the_loss(standins, B, masked):
    vc = standins
    V, H, W = 4, 37, 53
    render0, gt = _pair(B, H, W, 20 + B)
    gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    mask = (torch.rand(B, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) < 0.3).float() if masked else None
    indices = [2, 0][:B]
    cor = _Corrector(V)
    with torch.no_grad():
        cor.view_correction[:] = torch.tensor([[1.1, 0.93, 1.04], [1.0, 1.0, 1.0], [0.88, 1.02, 1.21], [1.0, 1.0, 1.0]], device=DEV)
    render = render0.clone().requires_grad_(True)
    output = {"render_correct": _vis(cor, render, indices, vc.__getitem__)}
    assert cor.index == indices[-1] and vc.handed_out.count == B
    vc.calculate_loss(_Renderer(), gt, render, output, mask)
    assert vc.stats()["fallbacks"] == {} and vc.stats()["readbacks"] == {"calculate_loss": 1} and vc.handed_out.count == 0
    output["loss"].backward()
    # torch autograd of the plain formula, float64 and float32, on the device
    refs = {}
    for dtype in (torch.float64, torch.float32):
        r = render0.to(dtype).requires_grad_(True)
        k = cor.view_correction.detach().to(dtype).requires_grad_(True)
        g = gt.to(dtype)
        correct = torch.stack([r[b] * k[i][:, None, None] for b, i in enumerate(indices)])
        blend = r if mask is None else g * mask.to(dtype)[:, None] + r * (1 - mask.to(dtype)[:, None])
        ssim = 1.0 - vref.loss_ref.ssim_map(blend, g).mean()
        l1 = (correct - g).abs().mean()
        loss = 0.2 * ssim + 0.8 * l1
        loss.backward()
        refs[dtype] = dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()), grad_render=r.grad, grad_gain=k.grad)
    ref64, ref32 = refs[torch.float64], refs[torch.float32]
    ref64["gap32_grad_render"] = rel_l2(ref32["grad_render"].cpu(), ref64["grad_render"].cpu())
    ref64["S_gain"] = torch.zeros(V, 3, dtype=torch.float64, device=DEV)
    ref64["S_gain"][indices] = 0.8 / (B * 3 * H * W) * render0.double().abs().sum(dim=(2, 3))
    gaps = {k: max(v, abs(ref32[k] - ref64[k])) for k, v in _gaps().items()}
    d = output["loss_dict"]
    assert set(d) == {"l1", "ssim"} and all(isinstance(v, float) for v in d.values())
    got = ((output["loss"].detach(), torch.tensor(d["l1"]), torch.tensor(d["ssim"])), render.grad, cor.view_correction.grad)
    assert tuple(cor.view_correction.grad.shape) == (V, 3)                      # dense, the rows not handed out hold zeros
    assert not cor.view_correction.grad[[i for i in range(V) if i not in indices]].any()
    _check(f"hand-over B={B} masked={masked}", got, ref64, ref32, gaps)
    # ... and the step of the last row handed out, through the drop-in: one launch, no fall-back
    before = cor.snapshot()
    vc.step(cor)
    after = cor.snapshot()
    i = indices[-1]
    assert vc.stats()["fallbacks"] == {} and vc.stats()["calls"]["step"] == 1
    _, want, S = vref.corrector_step({k: before[k][i] for k in vref.STATE}, 0, 0, 0.1, 0.001)
    _, want32, _ = vref.corrector_step({k: before[k][i] for k in vref.STATE}, 0, 0, 0.1, 0.001, dtype=torch.float32)
    for k in vref.STATE:
        ok, ratio = vref.within(after[k][i], want32[k], want[k], S[k], FACTOR)
        assert ok, (k, after[k][i], want[k], ratio)
        others = [j for j in range(V) if j != i]
        assert torch.equal(after[k][others], before[k][others]), k
    assert after["steps"].tolist() == [1 if j == i else 0 for j in range(V)]


def test_loss_calls_the_wrapped_method_when_the_rows_do_not_fit(standins):
    vc = standins
    B, V = 2, 3
    render0, gt = _pair(B, 24, 40, 31)
    cor = _Corrector(V)

    def both(output_of, expect):
        """The drop-in and the wrapped method on the same inputs -> the same loss and gradients, the reason counted."""
        results = []
        for fn in (vc.calculate_loss, _reference_calculate_loss):
            cor.view_correction.grad = None
            render = render0.clone().requires_grad_(True)
            output = output_of(render)
            fn(_Renderer(), gt, render, output)
            output["loss"].backward()
            results.append((output["loss"].detach(), render.grad, output["loss_dict"]))
            vc.handed_out.take()
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]) and results[0][2] == results[1][2]
        assert vc.stats()["fallbacks"] == expect

    both(lambda render: {}, {("calculate_loss", "no render_correct in output"): 1})
    # three rows handed out for two images (a vis that ran without a loss before this one)
    both(lambda render: (vc.__getitem__(cor, 1), {"render_correct": _vis(cor, render, [0, 2], vc.__getitem__)})[1],
         {("calculate_loss", "no render_correct in output"): 1,
          ("calculate_loss", "rows handed out since the last loss are not one per image"): 1})
    # the note is empty again after every loss call, whatever path it took
    assert vc.handed_out.count == 0
    # rows handed out without end and no loss: the note stays bounded
    for _ in range(3 * vc.MAX_NOTED):
        vc.__getitem__(cor, 0)
    assert len(vc.handed_out.rows) == vc.MAX_NOTED and vc.handed_out.count == 3 * vc.MAX_NOTED


def test_every_fall_back_of_the_step_is_counted_and_leaves_what_the_reference_leaves(standins):
    vc = standins

    def case(reason, make, raises=None):
        ours, theirs = make(), make()
        for cor, fn in ((ours, vc.step), (theirs, _reference_step)):
            if raises:
                with pytest.raises(raises):
                    fn(cor)
            else:
                fn(cor)
        a, b = ours.snapshot(), theirs.snapshot()
        for k in a:
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (reason, k)
        assert vc.stats()["fallbacks"].get(("step", reason)) == 1, (reason, vc.stats())

    def made(index=1, grad=True, **kw):
        def make():
            cor = _Corrector(3, **kw)
            cor.index = index
            if grad:
                cor.view_correction.grad = torch.full_like(cor.view_correction.data, 0.25)
            return cor
        return make

    case("tensors are not on the GPU", made(device="cpu"))
    case("tensors are not float32", made(dtype=torch.float64))
    case("use_amsgrad is off", made(amsgrad=False))
    case("view_correction.grad is None", made(grad=False), raises=TypeError)
    case("index is not an integer in [0, V)", made(index=-1))
    assert len(vc.stats()["fallbacks"]) == 5 and vc.stats()["calls"]["step"] == 5
    # ... and none of them on the path the kernel covers
    cor = made()()
    vc.step(cor)
    assert len(vc.stats()["fallbacks"]) == 5 and cor.snapshot()["steps"].tolist() == [0, 1, 0]
    assert not cor.view_correction.grad[1].any() and cor.view_correction.grad[0].eq(0.25).all()

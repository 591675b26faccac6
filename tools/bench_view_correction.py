"""Stage benchmark of one training view's loss forward + backward + Corrector.step with `use_view_correction: True`, two ways
on the same inputs in one process, alternating after a warm-up:

  torch_device  what an unmodified LoG process runs around today's fused loss (log_amd.install_all(fused_loss=True)): the
                row handed out, `render_correct = render * row[:, None, None]`, the loss with render_l1 = render_correct,
                one read-back for loss_dict, backward (two image gradients, the multiply's backward, their sum), then the
                reference's Corrector.step as torch ops on the device, written here from its description: nine list-indexed
                reads / writes, `if steps < 0` on a device tensor, `.item()`, the schedule in numpy, AMSGrad element-wise
  device        log_amd.view_correction: the same hand-out and the same (unread) render_correct multiply that LoG's `vis`
                still does, the loss with l1_gain = the row, one read-back, backward (one image gradient + the gain's), then
                lograst_corrector_step

    python tools/bench_view_correction.py [--reps 30] [--warmup 5] [--size 1920x1080]        -> one JSON line

Per way: wall time between two device synchronisations, HIP-event time of the same span (medians, min, max over --reps) and
the calls torch's sync debug mode flags in one extra, untimed repetition (blocking copies in either direction and `.item()` /
`.tolist()`: each waits for the stream).  `saved` = median(torch_device) - median(device); it counts as a gain only where it
exceeds the min-max spread of the torch_device repetitions (the criterion of profiles/depth_pass_reuse.md)."""
import argparse
import json
import os
import statistics
import sys
import time
import types
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from log_amd import view_correction as vc  # noqa: E402
from log_amd.loss import l1_ssim_loss  # noqa: E402

dev = torch.device("cuda:0")


class Corrector:
    """The state of LoG's Corrector (corrector.py:7-33) for V views."""

    def __init__(self, V):
        self.lr_init, self.lr_final, self.start_step = 0.1, 0.001, 0
        self.use_view_correction, self.use_amsgrad, self.index = True, True, None
        self.view_correction = torch.nn.Parameter(torch.ones(V, 3, device=dev))
        z = lambda: {"view_correction": torch.zeros(V, 3, device=dev)}  # noqa: E731
        self.optimizer = types.SimpleNamespace(exp_avg=z(), exp_avg_sq=z(), max_exp_avg_sq=z(), use_amsgrad=True,
                                               steps={"view_correction": torch.zeros(V, dtype=torch.int32, device=dev)})

    def hand_out(self, index):
        self.index = index
        return self.view_correction[index]


def torch_step(cor):
    """Corrector.step as the reference runs it on the device: list indices, a device tensor in an `if`, `.item()`."""
    opt, sel = cor.optimizer, [cor.index]
    opt.steps["view_correction"][sel] += 1
    s = opt.steps["view_correction"][sel] - cor.start_step
    if s < 0:
        return
    m, v, vmax = (getattr(opt, k)["view_correction"][sel] for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
    t = np.clip(s.item() / 100, 0, 1)
    lr = np.exp(np.log(cor.lr_init) * (1 - t) + np.log(cor.lr_final) * t)
    p, g = cor.view_correction.data[sel], cor.view_correction.grad[sel]
    m.mul_(0.9).add_(g, alpha=1 - 0.9)
    v.mul_(0.999).addcmul_(g, g, value=1 - 0.999)
    sc = s[:, None]
    step_size = lr / (1 - 0.9 ** sc)
    torch.max(vmax, v, out=vmax)
    denom = (vmax.sqrt() / torch.sqrt(1 - 0.999 ** sc)).add_(1e-15)
    p.add_(-step_size * (m / denom))
    cor.view_correction.data[sel] = p
    cor.view_correction.grad[sel] = 0
    opt.exp_avg["view_correction"][sel] = m
    opt.exp_avg_sq["view_correction"][sel] = v
    opt.max_exp_avg_sq["view_correction"][sel] = vmax


def way_torch_device(cor, index, render, gt):
    row = cor.hand_out(index)
    render_correct = torch.stack([render[0] * row[:, None, None]])
    loss, l1, ssim = l1_ssim_loss(render, gt, render_correct[:, :3])
    loss_dict = torch.stack([l1, ssim]).tolist()
    loss.backward()
    torch_step(cor)
    return loss_dict


def way_device(cor, index, render, gt):
    row = cor.hand_out(index)
    render_correct = torch.stack([render[0] * row[:, None, None]])          # LoG's vis still builds it; nothing reads it
    loss, l1, ssim = l1_ssim_loss(render, gt, l1_gain=torch.stack([row]))
    loss_dict = torch.stack([l1, ssim]).tolist()
    loss.backward()
    vc.step(cor)
    del render_correct
    return loss_dict


def flagged_syncs(fn, *args):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="1920x1080")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_view_correction needs the MI355X"
    W, H = (int(v) for v in a.size.split("x"))
    g = torch.Generator(device=dev).manual_seed(H)
    base = torch.rand(1, 3, H, W, device=dev, generator=g)
    gt = (base * torch.tensor([1.1, 0.93, 1.04], device=dev)[None, :, None, None]
          + 0.05 * torch.randn(1, 3, H, W, device=dev, generator=g)).clamp(0, 1)
    gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # [B,H,W,3] permuted: LoG's batch['image']
    ways = {"torch_device": (way_torch_device, Corrector(8)), "device": (way_device, Corrector(8))}
    wall = {k: [] for k in ways}
    event = {k: [] for k in ways}
    vc.reset_stats()
    for it in range(a.warmup + a.reps):
        for name, (fn, cor) in ways.items():                               # the ways alternate
            render = base.clone().requires_grad_(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn(cor, 3, render, gt)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it >= a.warmup:
                wall[name].append((t1 - t0) * 1e6)
                event[name].append(e0.elapsed_time(e1) * 1e3)
    assert vc.stats()["fallbacks"] == {}, vc.stats()
    out = {"workload": f"loss forward + backward + Corrector.step, one view {W}x{H}, B=1 C=3 fp32", "reps": a.reps, "warmup": a.warmup}
    for name, (fn, cor) in ways.items():
        render = base.clone().requires_grad_(True)
        out[name] = {"wall_us": {"median": statistics.median(wall[name]), "min": min(wall[name]), "max": max(wall[name])},
                     "event_us": {"median": statistics.median(event[name]), "min": min(event[name]), "max": max(event[name])},
                     "flagged_synchronisations": flagged_syncs(fn, cor, 3, render, gt),
                     "row_after": cor.view_correction.data[3].tolist(), "steps_after": int(cor.optimizer.steps["view_correction"][3])}
    for k in ("wall_us", "event_us"):
        saved = out["torch_device"][k]["median"] - out["device"][k]["median"]
        spread = out["torch_device"][k]["max"] - out["torch_device"][k]["min"]
        out["saved_" + k] = saved
        out["torch_device_spread_" + k] = spread
        out["gain_" + k] = bool(saved > spread)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

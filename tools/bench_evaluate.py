"""Stage benchmark of the evaluation path (log_amd.evaluate: lograst_eval_metrics / lograst_eval_read /
lograst_image_to_bgr8) against the sequence of torch and numpy calls an unmodified LoG process makes per validation image
(LoG/utils/trainer.py:313-332, LoG/utils/metric.py, LoG/render/renderer.py:19-23), written here from the formulas: the
view-correction fit over the left half, gain and clamp, the L1 mean, the PSNR with its .item(), the metric's SSIM as
grouped conv2d with zero padding, and tensor_to_bgr of cat([pred, gt], dim=1) (float32 copy to the host, numpy on one
thread).

    python tools/bench_evaluate.py [--reps 20] [--warmup 3] [--size 1920x1080] [--markdown FILE]     -> one JSON line

The two sides ALTERNATE in one process (device, torch, device, torch, ...): --warmup rounds, then --reps rounds.  Per side
and configuration: the median and (min - max) of
  * metrics_event_us: HIP events around the metrics alone (device side: one validation_metrics launch; torch side: the fit,
    clamp, L1 and PSNR up to, not including, the .item());
  * wall_us: perf_counter from before the first call until the host holds the scalars AND the 8-bit image (device side:
    launch, read(), bgr8_host(); torch side: the sequence above).
The export on its own (image_to_bgr8 against tensor_to_bgr of one image: the demo's per-frame cost) is timed the same way.
--markdown writes the table of profiles/evaluate_stage.md."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from log_amd import evaluate  # noqa: E402

dev = torch.device("cuda:0")


def images(H, W, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    coarse = torch.rand(1, 3, 12, 12, device=dev, generator=g)
    gt = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0].contiguous()
    pred = (0.8 * gt + 0.05 * torch.randn(3, H, W, device=dev, generator=g)).clamp(0, 1).contiguous()
    return pred, gt


def tensor_to_bgr(tensor):
    vis = tensor.detach().cpu().numpy().transpose(1, 2, 0)
    vis = (np.clip(vis[:, :, ::-1], 0., 1.) * 255).astype(np.uint8)
    return np.ascontiguousarray(vis)


def torch_ssim(rgbs, target, max_val):
    """metric.py:56-103 for one [C, A, B] image."""
    C = rgbs.shape[0]
    f = ((torch.arange(11, device=dev) - 5) / 1.5) ** 2
    filt = torch.exp(-0.5 * f)
    filt /= torch.sum(filt)
    f1 = lambda z: F.conv2d(z, filt.view(1, 1, -1, 1).repeat(C, 1, 1, 1), padding=[5, 0], groups=C)
    f2 = lambda z: F.conv2d(z, filt.view(1, 1, 1, -1).repeat(C, 1, 1, 1), padding=[0, 5], groups=C)
    blur = lambda z: f1(f2(z))
    a, b = rgbs[None], target[None]
    mu0, mu1 = blur(a), blur(b)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = torch.clamp(blur(a ** 2) - mu00, min=0.0)
    s11 = torch.clamp(blur(b ** 2) - mu11, min=0.0)
    s01 = blur(a * b) - mu01
    s01 = torch.sign(s01) * torch.min(torch.sqrt(s00 * s11), torch.abs(s01))
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    ssim_map = ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return torch.mean(ssim_map.reshape([-1, ssim_map[0].numel()]), dim=-1).item()


def torch_side(pred, gt, fit, ssim, events):
    events[0].record()
    if fit:
        gt_left = gt[:, :, :gt.shape[2] // 2]
        pred_left = pred[:, :, :pred.shape[2] // 2]
        view_correct = (gt_left * pred_left).sum(dim=-1).sum(dim=-1) / (pred_left ** 2).sum(dim=-1).sum(dim=-1)
        pred = torch.clamp(pred * view_correct[:, None, None], 0., 1.)
    l1 = torch.mean(torch.abs(pred - gt))
    mse = torch.mean((pred - gt) ** 2)
    log = torch.log10(mse)
    events[1].record()
    out = {"l1": float(l1), "psnr": -10 * log.item()}
    if ssim:
        out["ssim"] = torch_ssim(pred, gt, 1.0)
    out["vis"] = tensor_to_bgr(torch.cat([pred, gt], dim=1))
    return out


def device_side(pred, gt, fit, ssim, events):
    events[0].record()
    m = evaluate.validation_metrics(pred, gt, fit_gain=fit, ssim=ssim, bgr8=True)
    events[1].record()
    r = m.read()
    return {"l1": r.l1, "psnr": r.psnr, "ssim": r.ssim, "vis": m.bgr8_host()}


def torch_export(pred, gt, fit, ssim, events):
    events[0].record()
    events[1].record()
    return {"vis": tensor_to_bgr(pred)}


def device_export(pred, gt, fit, ssim, events):
    events[0].record()
    out = evaluate.image_to_bgr8_device(pred)
    events[1].record()
    with torch.cuda.device(dev):
        return {"vis": evaluate._to_host(out)}


def once(fn, pred, gt, fit, ssim):
    events = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(pred, gt, fit, ssim, events)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6
    return wall, events[0].elapsed_time(events[1]) * 1e3, out


def summary(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_evaluate needs the MI355X"
    W, H = (int(v) for v in a.size.split("x"))
    pred, gt = images(H, W, 5)
    configs = [("metrics + image", False, False, device_side, torch_side), ("fit + metrics + image", True, False, device_side, torch_side),
               ("metrics + ssim + image", False, True, device_side, torch_side),
               ("fit + metrics + ssim + image", True, True, device_side, torch_side),
               ("export of one image", False, False, device_export, torch_export)]
    result = {"workload": f"evaluation of one {W}x{H} image, 3 channels", "reps": a.reps, "warmup": a.warmup, "configs": {}}
    for name, fit, ssim, ours, theirs in configs:
        t = {"device": {"wall": [], "event": []}, "torch": {"wall": [], "event": []}}
        for it in range(a.warmup + a.reps):
            for side, fn in (("device", ours), ("torch", theirs)):
                wall, ev, out = once(fn, pred, gt, fit, ssim)
                if it >= a.warmup:
                    t[side]["wall"].append(wall)
                    t[side]["event"].append(ev)
        d, r = once(ours, pred, gt, fit, ssim)[2], once(theirs, pred, gt, fit, ssim)[2]
        entry = {side: {"wall_us": summary(t[side]["wall"]), "metrics_event_us": summary(t[side]["event"])} for side in t}
        entry["bytes_differing"] = int((d["vis"] != r["vis"]).sum())
        entry["bytes"] = int(d["vis"].size)
        for k in ("l1", "psnr", "ssim"):
            if d.get(k) is not None and k in r:
                entry[k] = {"device": d[k], "torch_fp32": r[k]}
        result["configs"][name] = entry
    print(json.dumps(result))
    if a.markdown:
        lines = ["| configuration | device wall us (min - max) | torch + numpy wall us (min - max) | device metrics kernels us | torch metrics kernels us |",
                 "|---|---|---|---|---|"]
        cell = lambda s: f"{s['median_us']} ({s['min_us']} - {s['max_us']})"
        for name, e in result["configs"].items():
            lines.append(f"| {name} | {cell(e['device']['wall_us'])} | {cell(e['torch']['wall_us'])} | "
                         f"{cell(e['device']['metrics_event_us'])} | {cell(e['torch']['metrics_event_us'])} |")
        with open(a.markdown, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

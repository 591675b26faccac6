"""A numpy restatement of what LoG computes per validation image -- the view-correction fit, gain and clamp, L1, PSNR
(LoG/utils/trainer.py:313-320, LoG/utils/metric.py:7-9), the metric's SSIM (metric.py:33-103: 11 taps, sigma 1.5, ZERO
padding, clamped variances, limited covariance) and the 8-bit export (LoG/render/renderer.py:19-23) -- written from the
formulas, in float64 or, with ``dtype=np.float32``, operation for operation in fp32 as the reference runs them.  The tests
measure log_amd.evaluate against the float64 form; the fp32 form is the yardstick of what fp32 can give
(tools/fuzz_step_ops.py's rule: |got - ref64| <= 8 (|ref32 - ref64| + 2^-24 S), S the mean magnitude of the summed terms)."""
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS24 = 2.0 ** -24
F = 8.0


def golden_cases():
    """-> {name: dict of arrays} of tests/golden/evaluate_*.npz."""
    out = {}
    for p in sorted(glob.glob(os.path.join(HERE, "golden", "evaluate_*.npz"))):
        with np.load(p) as z:
            out[os.path.basename(p)[9:-4]] = {k: z[k] for k in z.files}
    return out


def to_bgr8(img):
    """renderer.py:20-22 on an fp32 [C, H, W] array -> uint8 [H, W, C]."""
    vis = np.asarray(img, dtype=np.float32).transpose(1, 2, 0)
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray((np.clip(vis[:, :, ::-1], np.float32(0.), np.float32(1.)) * np.float32(255)).astype(np.uint8))


def gain_fit(pred, gt, dtype=np.float64):
    """trainer.py:314-316 -> (gain [C], sum gt * pred [C], sum pred^2 [C], S [C] = sum |gt * pred| / sum pred^2)."""
    p, g = pred.astype(dtype), gt.astype(dtype)
    half = p.shape[2] // 2
    pl, gl = p[:, :, :half], g[:, :, :half]
    sgp = (gl * pl).sum(axis=-1, dtype=dtype).sum(axis=-1, dtype=dtype)
    spp = (pl ** 2).sum(axis=-1, dtype=dtype).sum(axis=-1, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        gain = sgp / spp
        S = np.abs(gl * pl).sum(axis=(-1, -2), dtype=np.float64) / spp.astype(np.float64)
    return gain.astype(dtype), sgp, spp, S


def window(dtype=np.float64):
    """metric.py:63-67."""
    f = ((np.arange(11).astype(dtype) - dtype(5)) / dtype(1.5)) ** 2
    filt = np.exp(dtype(-0.5) * f).astype(dtype)
    return (filt / filt.sum(dtype=dtype)).astype(dtype)


def _blur(z, w, axis):
    """11 taps along ``axis`` with zero padding of 5 on both sides, taps added in ascending order."""
    pad = [(0, 0)] * z.ndim
    pad[axis] = (5, 5)
    zp = np.pad(z, pad)
    n = z.shape[axis]
    out = np.zeros_like(z)
    for k in range(11):
        out = out + w[k] * np.take(zp, np.arange(k, k + n), axis=axis)
    return out


def ssim_map(p, g, max_val=1.0, dtype=np.float64):
    """metric.py:69-101 for [C, A, B] arrays -> the map [C, A, B]."""
    p, g = p.astype(dtype), g.astype(dtype)
    w = window(dtype)
    blur = lambda z: _blur(_blur(z, w, 2), w, 1)
    mu0, mu1 = blur(p), blur(g)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = np.maximum(blur(p ** 2) - mu00, dtype(0))
    s11 = np.maximum(blur(g ** 2) - mu11, dtype(0))
    s01 = blur(p * g) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = dtype((0.01 * max_val) ** 2), dtype((0.03 * max_val) ** 2)
    numer = (dtype(2) * mu01 + c1) * (dtype(2) * s01 + c2)
    denom = (mu00 + mu11 + c1) * (s00 + s11 + c2)
    return (numer / denom).astype(dtype)


def evaluate_ref(pred, gt, fit_gain=False, ssim=False, max_val=1.0, dtype=np.float64):
    """pred, gt: fp32 [C, H, W] -> dict: gain, sgp, spp, gain_S (with the fit), corrected (p, in ``dtype``), l1, mse, psnr,
    ssim and ssim_S (with ssim).  The sums of l1, mse and ssim have S = the value itself (non-negative terms) resp.
    mean |ssim_map|."""
    out = {}
    p, g = pred.astype(dtype), gt.astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        if fit_gain:
            gain, out["sgp"], out["spp"], out["gain_S"] = gain_fit(pred, gt, dtype)
            out["gain"] = gain
            p = np.clip(p * gain[:, None, None], dtype(0), dtype(1))       # np.clip keeps a nan, as torch.clamp does
        out["corrected"] = p
        d = p - g
        out["l1"] = float(np.abs(d).mean(dtype=dtype))
        out["mse"] = float((d ** 2).mean(dtype=dtype))
        out["psnr"] = float(-10 * np.log10(dtype(out["mse"])))
        if ssim:
            m = ssim_map(p, g, max_val, dtype)
            out["ssim"] = float(m.mean(dtype=dtype))
            out["ssim_S"] = float(np.abs(m).mean(dtype=np.float64))
    return out


def within(got, r64, r32, S):
    """The rule for one scalar; values that are not finite match by class.  -> (ok, error, bound)."""
    if not np.isfinite(r64):
        same = (np.isnan(got) and np.isnan(r64)) or (np.isinf(got) and np.isinf(r64) and np.sign(got) == np.sign(r64))
        return bool(same), 0.0, 0.0
    if not np.isfinite(got):
        return False, float("inf"), 0.0
    bound = F * (abs(r32 - r64) + EPS24 * S + 2.0 ** -126)
    err = abs(got - r64)
    return bool(err <= bound), float(err), float(bound)

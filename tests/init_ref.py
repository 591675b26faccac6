"""numpy restatement of the initialisation pass (LoG.init with Gaussian.init_radius3d, LoG/model/level_of_gaussian.py:55-63,
:328-332) for the tests of log_amd/init_pass.py and log_amd/csrc/init.hip, in two modes that differ in how a view's radius,
the first scale column and the factor 3 / r come about:

* ``"torch"``: what the reference runs -- ``torch.exp``, ``F.normalize``, ``oracle.compute_radius`` on the activated
  rows, and ``3. / r`` as torch evaluates a Python scalar over a tensor: ``r.reciprocal() * 3`` (``Tensor.__rdiv__``), two
  roundings.  It reproduces the fixtures recorded from the reference bit for bit.
* ``"fixed"``: what the kernel runs -- ``oracle.lod_radius`` on the RAW rows (lr_exp_any, lr_normalize4 and lr_cov3d, the
  fixed op sequences of the level-of-detail kernel), the first scale column from a restatement of lr_exp_any whose fused
  steps are libm's ``fmaf`` (a double-precision a * b + c rounds twice and is not the same thing), and ``3.f / r`` as one
  correctly rounded division.

The rest is shared: ``valid = r > 0``, ``r3d = fp32(s0 * t)``, ``minimum`` with a NaN on either side propagating, every
other row untouched."""
import ctypes
import ctypes.util
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3
_EXP_COEFFS = [float.fromhex(h) for h in ("0x1.5c08e4p-10", "0x1.3d0c52p-7", "0x1.c6b6e4p-5", "0x1.ebf918p-3",
                                         "0x1.62e428p-1", "0x1.000002p+0")]


def _fmaf(a, b, c):
    """Element-wise fmaf(a, b, c) on fp32 arrays: ONE rounding, libm's."""
    a, b = np.asarray(a, _F), np.asarray(b, _F)
    out = np.empty(a.shape, _F)
    flat = out.reshape(-1)
    for i, (x, y) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist())):
        flat[i] = _libm.fmaf(x, y, c)
    return out


def exp_any(x):
    """lr_exp_any (log_amd/csrc/common.hpp) / ora_exp_any on an fp32 array, op for op."""
    x = np.asarray(x, _F)
    with np.errstate(all="ignore"):
        t = x * _F(1.44269504088896341)
        t = np.fmin(np.fmax(t, _F(-125.0)), _F(125.0))        # fmaxf / fminf: a NaN loses against the bound
        n = np.rint(t).astype(_F)
        f = (t - n).astype(_F)
        p = np.full(x.shape, _EXP_COEFFS[0], _F)
        for c in _EXP_COEFFS[1:]:
            p = _fmaf(p, f, c)
        bits = p.view(np.uint32) + (n.astype(np.int32).astype(np.uint32) << np.uint32(23))
    return bits.view(_F)


def minimum(a, b):
    """torch.minimum: b where it is smaller or NaN, else a (a NaN a fails the comparison and stays)."""
    with np.errstate(invalid="ignore"):
        return np.where((b < a) | np.isnan(b), b, a).astype(_F)


def camera_args(fx, v):
    """-> (proj, view, fx, fy, tanfovx, tanfovy) of view ``v`` of a fixture, as lograst_compute_radius takes them."""
    W, H = (int(x) for x in fx[f"{v}_wh"])
    tfx, tfy = (float(x) for x in fx[f"{v}_tanfov"])
    return fx[f"{v}_proj"], fx[f"{v}_view"], W / (2.0 * tfx), H / (2.0 * tfy), tfx, tfy


def first_scale(mode, scaling):
    """The activated first scale column, fp32[P] (it does not depend on the camera)."""
    col = np.ascontiguousarray(np.asarray(scaling, _F)[:, 0])
    if mode == "torch":
        import torch
        return torch.exp(torch.from_numpy(col)).numpy()
    assert mode == "fixed", mode
    return exp_any(col)


def radius2d(mode, xyz, scaling, rotation, cam):
    """One view's projected radius, fp32[P]; 0 = not visible."""
    from oracle import oracle
    proj, view, fx, fy, tfx, tfy = cam
    if mode == "torch":
        import torch
        s = torch.exp(torch.from_numpy(np.ascontiguousarray(scaling, _F))).numpy()
        q = torch.nn.functional.normalize(torch.from_numpy(np.ascontiguousarray(rotation, _F))).numpy()
        return oracle.compute_radius(xyz, s, q, proj, view, fx, fy, tfx, tfy)
    assert mode == "fixed", mode
    return oracle.lod_radius(np.arange(xyz.shape[0]), xyz, scaling, rotation, proj, view, fx, fy, tfx, tfy)


def init_radius3d(mode, xyz, scaling, rotation, cam, s0=None):
    """Gaussian.init_radius3d -> (valid bool[P], radius3d fp32[P]: s0 where not valid).  s0: first_scale(mode, scaling)."""
    s0 = first_scale(mode, scaling) if s0 is None else s0
    r = radius2d(mode, xyz, scaling, rotation, cam)
    with np.errstate(all="ignore"):
        valid = r > 0
        rv = r[valid]
        t = ((_F(1.0) / rv).astype(_F) * _F(3.0)).astype(_F) if mode == "torch" else (_F(3.0) / rv).astype(_F)
        radius3d = s0.copy()
        radius3d[valid] = (s0[valid] * t).astype(_F)
    return valid, radius3d


def log_init(mode, xyz, scaling, rotation, cams, radius3d_min):
    """LoG.init once per camera -> [(valid, radius3d_min after the view)]; ``radius3d_min`` itself is not written."""
    rmin = np.array(radius3d_min, _F)
    s0 = first_scale(mode, scaling)
    out = []
    for cam in cams:
        valid, r3d = init_radius3d(mode, xyz, scaling, rotation, cam, s0)
        rmin = rmin.copy()
        rmin[valid] = minimum(rmin[valid], r3d[valid])
        out.append((valid, rmin))
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, _F).view(np.uint32),
                                                 np.ascontiguousarray(b, _F).view(np.uint32))


def load(name="log"):
    return np.load(os.path.join(GOLDEN, f"init_{name}.npz"))


def views(fx):
    return [str(v) for v in fx["meta_views"]]


def bits(fx, key, n):
    return np.unpackbits(fx[key])[:n].astype(bool)

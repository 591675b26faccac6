"""numpy restatement of the view preparation (log_amd/prepare.py, log_amd/csrc/prepare.hip), i.e. of the reference's
Gaussian._visible_flag_by_camera, the root filter and leaf / node split of LoG.prepare, and LoG.clamp_scale
(LoG/model/level_of_gaussian.py:39-53, :241-251, :367-377).  float64 for the arithmetic; the filter and the partition as
index operations; clamp with torch.clamp's rules for NaN and for lo > hi."""
import os

import numpy as np

EPS = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ADD = float(np.float32(1e-7))          # the fp32 constant of `xyz1RTK[..., 3:4] + 1e-7`


def bounds(padding):
    """(-1 - padding, 1 + padding) as torch compares them with an fp32 tensor: the Python doubles narrowed to fp32."""
    return float(np.float32(-1.0 - padding)), float(np.float32(1.0 + padding))


def frustum(xyz, proj, padding, rows=None):
    """-> (flag bool[n], undecided bool[n]).  undecided: one of the six float64 margins is within 64 * 2^-24 * S * |pw|,
    S = the sum of |terms| of the two dot products behind the coordinate: an fp32 evaluation in another summation order
    may decide such an entry either way.  Entries with a NaN or an infinity are decided: False."""
    x = np.asarray(xyz, np.float64)
    if rows is not None:
        x = x[np.asarray(rows, np.int64)]
    m = np.asarray(proj, np.float64).reshape(4, 4)
    lo, hi = bounds(padding)
    with np.errstate(all="ignore"):
        terms = x[:, :, None] * m[None, :3, :]                 # [n, 3, 4]
        h = terms.sum(axis=1) + m[3]
        s = np.abs(terms).sum(axis=1) + np.abs(m[3])
        pw = 1.0 / (h[:, 3] + ADD)
        p = h[:, :3] * pw[:, None]
        margins = np.stack([p[:, 2] - 0.0, 1.0 - p[:, 2], p[:, 0] - lo, hi - p[:, 0], p[:, 1] - lo, hi - p[:, 1]], axis=1)
        flag = (margins > 0).all(axis=1)
        sc = np.stack([s[:, 2], s[:, 2], s[:, 0], s[:, 0], s[:, 1], s[:, 1]], axis=1) + s[:, 3:4]
        tol = 64.0 * EPS * sc * np.abs(pw)[:, None]
        finite = np.isfinite(x).all(axis=1) & np.isfinite(p).all(axis=1)
        undecided = finite & (np.abs(margins) <= tol).any(axis=1)
    return flag & finite, undecided


def root_filter(in_range, weight):
    """level_of_gaussian.py:241: valid_root_flag[valid_root_flag.clone()] = point_weight > 1e-8 (fp32 comparison)."""
    in_range = np.asarray(in_range, bool)
    pos = np.nonzero(in_range)[0]
    keep = np.asarray(weight, np.float32) > np.float32(1e-8)
    assert keep.shape == pos.shape
    flag = in_range.copy()
    flag[pos[~keep]] = False
    return flag


def partition(index_all, node_index, depth, opt_all_levels, current_depth):
    """level_of_gaussian.py:244-251 -> (index_leaf, index_node), both in the order of index_all."""
    index_all = np.asarray(index_all, np.int64)
    if opt_all_levels:
        leaf = (node_index[index_all] == -1) & (depth[index_all] > 0)
    else:
        leaf = depth[index_all].astype(np.int64) == int(current_depth)
    return index_all[leaf], index_all[~leaf]


def clamp(x, lo, hi):
    """torch.clamp(x, lo, hi) with tensor bounds, elementwise in float64: a NaN in x, lo or hi (in that order) is the
    result; otherwise min(max(x, lo), hi), so lo > hi gives hi."""
    x, lo, hi = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64))
    with np.errstate(all="ignore"):
        out = np.minimum(np.maximum(x, lo), hi)
    out = np.where(np.isnan(hi), hi, out)
    out = np.where(np.isnan(lo), lo, out)
    return np.where(np.isnan(x), x, out)


def clamp_scale(scaling, index, flag, rmin, rmax):
    """LoG.clamp_scale on the rows index[flag] -> (rows int64[k], float64[k, 3] the clamped rows); other rows stay."""
    index = np.asarray(index, np.int64)
    rows = index if flag is None else index[np.asarray(flag, bool)]
    with np.errstate(all="ignore"):
        lo = np.log(np.asarray(rmin, np.float64)[rows])[:, None]
        hi = np.log(np.asarray(rmax, np.float64)[rows])[:, None]
    return rows, clamp(np.asarray(scaling)[rows], lo, hi)


def ulp_error(got, want64):
    """|got - want| in units of the fp32 spacing at want; 0 where both are the same NaN / infinity."""
    got64 = np.asarray(got, np.float64)
    want64 = np.asarray(want64, np.float64)
    same = (np.isnan(got64) & np.isnan(want64)) | (got64 == want64)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
        err = np.abs(got64 - want64) / ulp
    return np.where(same, 0.0, np.where(np.isfinite(err), err, np.inf))


def load(name):
    return np.load(os.path.join(GOLDEN, f"prepare_{name}.npz"))


def planted_points(rng, n, proj, padding):
    """xyz fp32[n, 3] around the frustum of `proj` with every undecided row nudged away (redrawn) -- for tests of the
    kernel at sizes the fixtures do not have.  -> (xyz, flag)."""
    xyz = ((rng.random((n, 3)) - 0.5) * 3.0).astype(np.float32)
    for _ in range(50):
        flag, und = frustum(xyz, proj, padding)
        bad = np.nonzero(und)[0]
        if bad.size == 0:
            return xyz, flag
        xyz[bad] = ((rng.random((bad.size, 3)) - 0.5) * 3.0).astype(np.float32)
    raise AssertionError("could not nudge the undecided rows away")


def fixture_names():
    return sorted(f[len("prepare_"):-4] for f in os.listdir(GOLDEN) if f.startswith("prepare_") and f.endswith(".npz"))


def bits(fx, key, n):
    return np.unpackbits(fx[key])[:n].astype(bool)


def modes(fx):
    """[(name, opt_all_levels, current_depth)]"""
    return [(str(m), bool(a), int(d)) for m, a, d in zip(fx["meta_modes"], fx["meta_all_levels"], fx["meta_current_depth"])]


def views(fx):
    return [str(v) for v in fx["meta_views"]]

"""N1: simple_knn._C.distCUDA2 drop-in vs an exact CPU oracle (scipy cKDTree, float64), and lograst_knn_mean_dist2 itself,
with guarded buffers, against brute force in float64 at the workgroup (256) and box (1024) boundaries and on degenerate
clouds, to a bound derived from the kernel's arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _oracle(pts):
    from scipy.spatial import cKDTree
    p64 = pts.astype(np.float64)
    d, _ = cKDTree(p64).query(p64, k=4)          # column 0 is the point itself (distance 0)
    return (d[:, 1:] ** 2).mean(axis=1)


def _clouds():
    rng = np.random.default_rng(0)
    uni = rng.random((200_000, 3), dtype=np.float32) * np.array([4, 2, 1], np.float32)
    # COLMAP-like: dense surface patches + sparse far outliers that stretch the bounding box
    centers = rng.normal(size=(40, 3)) * 5
    clustered = np.concatenate([
        (centers[rng.integers(0, 40, 250_000)] + rng.normal(size=(250_000, 3)) * 0.05 *
         np.array([1, 1, 0.02])),
        rng.normal(size=(500, 3)) * 200]).astype(np.float32)
    dup = np.repeat(rng.random((5_000, 3), dtype=np.float32), 3, axis=0)   # exact duplicates -> zero distances
    small = rng.random((5, 3), dtype=np.float32)
    return {"uniform": uni, "clustered": clustered, "duplicates": dup, "five_points": small}


@pytest.mark.parametrize("name", ["uniform", "clustered", "duplicates", "five_points"])
def test_dist_cuda2_matches_exact_knn(name):
    from simple_knn._C import distCUDA2
    pts = _clouds()[name]
    out = distCUDA2(torch.tensor(pts, device="cuda:0")).cpu().numpy()
    ref = _oracle(pts)
    assert out.shape == ref.shape and np.isfinite(out).all()
    # fp32 distances vs float64: relative to the coordinate scale
    scale = float(np.abs(pts).max()) ** 2
    np.testing.assert_allclose(out, ref, rtol=2e-4, atol=2e-6 * scale)


def test_dist_cuda2_call_site_contract():
    """The two reference call sites do clamp_min(distCUDA2(xyz.cuda()), 1e-7) then sqrt (file.py:88-91)."""
    from simple_knn._C import distCUDA2
    xyz = torch.rand(10_000, 3)
    dist2 = torch.clamp_min(distCUDA2(xyz.cuda()), 1e-7)
    scales = torch.sqrt(dist2).cpu()
    assert scales.shape == (10_000,) and scales.min() > 0
    with pytest.raises(Exception, match="MI355X"):
        distCUDA2(xyz)


# ---- the C entry point at its edges ----------------------------------------------------------------------------------------
# Bound.  The inputs are exact fp32 values and the reference sees the same values.  Per neighbour the kernel rounds each
# coordinate difference once (relative u = 2^-24 each, so 2 u on its square), the product once (3 u), and adds three
# non-negative terms (two more roundings, never a cancellation: 5 u).  Choosing the three smallest of values that are each
# within 5 u of the true ones gives order statistics within 5 u.  The mean is two more sums and a division: 8 u in all.
# rtol = 16 u leaves a factor of two, atol = 0, and a reference of exactly 0 (duplicates) must come out as exactly 0.
U24 = 2.0 ** -24
RTOL = 16 * U24
KNN_GUARD = 256       # bytes, in front of and behind the scratch block; floats, around `out`
KNN_WORST = {}


def _brute(pts):
    p = pts.astype(np.float64)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)[:, :3].mean(axis=1)


def _knn(pts):
    """lograst_knn_mean_dist2 with buffers this test owns: -> out[P]; guards around `out` and the scratch block checked."""
    from log_amd import _lib
    L = _lib.lib()
    P = int(pts.shape[0])
    d_pts = torch.tensor(np.ascontiguousarray(pts, np.float32), device="cuda:0")
    nbytes = int(L.lograst_knn_scratch_bytes(P))
    assert nbytes > 0
    scratch = torch.full((KNN_GUARD + nbytes + KNN_GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out = torch.full((KNN_GUARD + P + KNN_GUARD,), -7.25, device="cuda:0")
    assert scratch.data_ptr() % 256 == 0
    _lib.check(L.lograst_knn_mean_dist2(P, ctypes.c_void_p(d_pts.data_ptr()), ctypes.c_void_p(out.data_ptr() + 4 * KNN_GUARD),
                                        ctypes.c_void_p(scratch.data_ptr() + KNN_GUARD), nbytes,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    s, o = scratch.cpu(), out.cpu()
    assert bool((s[:KNN_GUARD] == 0xA5).all()) and bool((s[KNN_GUARD + nbytes:] == 0xA5).all()), "scratch guard written"
    assert bool((o[:KNN_GUARD] == -7.25).all()) and bool((o[KNN_GUARD + P:] == -7.25).all()), "guard around out written"
    assert torch.equal(d_pts.cpu(), torch.from_numpy(np.ascontiguousarray(pts, np.float32)))
    return o[KNN_GUARD: KNN_GUARD + P].numpy().copy()


def _check(name, pts, rows=None):
    out, ref = _knn(pts), _brute(pts)
    sel = slice(None) if rows is None else rows
    out, ref = out[sel], ref[sel]
    assert np.isfinite(out).all(), name
    zero = ref == 0
    assert (out[zero] == 0).all(), name
    err = np.abs(out[~zero] - ref[~zero]) / ref[~zero]
    if err.size:
        KNN_WORST[name] = float(err.max() / U24)
        assert err.max() <= RTOL, (name, float(err.max() / U24), "u")
    return out, ref


def _box(rng, P):
    """Uniform in a box with negative and positive coordinates, a -0.0 among them."""
    pts = ((rng.random((P, 3), dtype=np.float32) - np.float32(0.4)) * np.array([4, 2, 1], np.float32)).astype(np.float32)
    pts[P // 2, 1] = np.float32(-0.0)
    return pts


def test_point_counts_at_the_workgroup_and_box_boundaries():
    rng = np.random.default_rng(11)
    for P in (4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 2049):
        pts = _box(rng, P)
        assert (pts < 0).any() and (pts > 0).any() and np.signbit(pts[P // 2, 1])
        _check("uniform P=%d" % P, pts)
    print({k: "%.2f u" % v for k, v in KNN_WORST.items()})


def test_degenerate_clouds():
    rng = np.random.default_rng(12)
    planar = _box(rng, 1500)
    planar[:, 2] = np.float32(0.37)                               # zero extent on one axis: ext = max(hi - lo, 1e-30)
    _check("planar", planar)
    t = rng.random(1200, dtype=np.float32)
    collinear = np.stack([t * 3 - 1, np.full_like(t, -0.5), np.full_like(t, 2.0)], axis=1).astype(np.float32)
    _check("collinear", collinear)
    same = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (1100, 1))
    out, _ = _check("identical", same)
    assert (out == 0).all()
    # a run of duplicates longer than the +-3 Morton seed window: the copies get 0, everybody else stays exact
    dup = _box(rng, 300)
    copies = rng.choice(300, 12, replace=False)
    dup[copies] = dup[copies[0]]
    out, ref = _check("12 copies among 300", dup)
    assert (out[copies] == 0).all() and (ref[copies] == 0).all() and int((ref == 0).sum()) == 12
    # integer lattice: every interior point has six neighbours at distance 1 -- exact ties, exact results
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    lattice = lattice[rng.permutation(512)]
    out, ref = _check("lattice 8x8x8", lattice)
    assert (out == ref.astype(np.float32)).all() and (ref == 1.0).all()
    print({k: "%.2f u" % v for k, v in KNN_WORST.items()})


def test_far_outlier_and_shifted_cloud():
    rng = np.random.default_rng(13)
    cube = rng.random((1500, 3), dtype=np.float32)
    outlier = np.concatenate([cube, np.array([[1e6, -1e6, 1e6]], np.float32)])
    outlier = outlier[rng.permutation(1501)]
    # every point of the cube quantises to one Morton code (pruning has no power); the outlier does not loosen the bound
    # for the others: rtol is relative to each point's own result
    out, ref = _check("unit cube + far outlier", outlier)
    far = int(np.argmax(outlier[:, 0]))
    assert ref[far] > 1e11 and ref[np.arange(1501) != far].max() < 1.0
    # coordinates near 1e4 (spacing of fp32 there: 1e-3): the box is still one unit wide, 10-bit quantisation separates
    shifted = (rng.random((1500, 3), dtype=np.float32) + np.float32(1e4)).astype(np.float32)
    assert np.unique(shifted, axis=0).shape[0] > 1400
    _check("shifted by 1e4", shifted)
    print({k: "%.2f u" % v for k, v in KNN_WORST.items()})


@pytest.mark.parametrize("P", [1, 2, 3])
def test_fewer_than_three_other_points(P):
    """include/lograst.h: the result is unspecified for P < 4.  The call succeeds, writes exactly P floats, none a NaN."""
    pts = _box(np.random.default_rng(14), 8)[:P]
    out = _knn(pts)
    assert out.shape == (P,) and not np.isnan(out).any()

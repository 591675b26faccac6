"""Code paths of the step kernels that exist only above a size: the `carry` loops of cnt_scan_kernel / lod_scan_kernel
(more than 1024 chunks of 1024), the grid strides of cnt_chunk_count / cnt_emit / lod_classify<false> / lod_scatter<false>
(more than 2048 chunks), adam_kernel<false> (m * width >= 2^31 - 1: 64-bit element indices) and lr_knn_bbox_kernel's grid
stride (more than 524,288 points) -- the sizes the project is built for (30 M Gaussians per view, LoG trees with millions
of roots).  Every comparison of an integer result is exact; KNN keeps the tolerance of tests/test_gpu_knn.py."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 1024                      # CNT_CHUNK / LOD_CHUNK
SCAN_ROUND = 1024 * CHUNK         # ids / slots one round of the one-workgroup scan covers
GRID_ROUND = 2048 * CHUNK         # ids / slots the 2048-workgroup grids cover before they stride
HIST_GRID_PIXELS = 4096 * 256     # pixels cnt_hist_kernel's grid covers before it strides


# ---- id histogram ---------------------------------------------------------------------------------------------------
def _runs(ids, lengths, npix):
    return torch.repeat_interleave(ids, lengths)[:npix].contiguous()


def _id_map(pattern, n, npix, gen):
    """An id map [npix] int32 in which the chunk prefixes matter; id n - 1 is always present."""
    ri = lambda lo, hi, k: torch.randint(lo, hi, (k,), generator=gen, device=DEV, dtype=torch.int32)
    nruns = (npix + 4) // 5
    five = torch.full((nruns,), 5, device=DEV)
    if pattern == "last_chunk":                  # everything in front of it is empty: its offset is the carry alone
        pid = _runs(ri((n - 1) // CHUNK * CHUNK, n, nruns), five, npix)
    elif pattern == "high_chunks":               # only chunks the first scan round never sees
        assert n > SCAN_ROUND
        pid = _runs(ri(SCAN_ROUND, n, nruns), five, npix)
    elif pattern == "every_chunk":               # no chunk count is zero: every prefix differs from its neighbour's
        nchunks = (n + CHUNK - 1) // CHUNK
        assert nruns >= 2 * nchunks
        ids = ri(0, n, nruns)
        one = torch.arange(nchunks, device=DEV, dtype=torch.int32) * CHUNK + ri(0, CHUNK, nchunks)
        ids[torch.randperm(nruns, generator=gen, device=DEV)[:nchunks]] = one.clamp(max=n - 1)
        pid = _runs(ids, five, npix)
    elif pattern == "long_runs":                 # runs over several waves, one across the seam of the histogram's grid
        k = npix // 65 + 1
        pid = _runs(ri(0, n, k), torch.randint(65, 700, (k,), generator=gen, device=DEV), npix)
        assert pid.numel() == npix and npix > HIST_GRID_PIXELS + 300
        pid[HIST_GRID_PIXELS - 300:HIST_GRID_PIXELS + 300] = n - 2
    else:
        raise KeyError(pattern)
    if pattern != "long_runs":
        pid[torch.rand(npix, generator=gen, device=DEV) < 0.2] = -1
    pid[-3:] = n - 1
    return pid


HIST_SIZES = [SCAN_ROUND, SCAN_ROUND + 1, GRID_ROUND + 1, 5_000_003]
HIST_CASES = [(n, p) for n in HIST_SIZES for p in ("last_chunk", "high_chunks", "every_chunk", "long_runs")
              if not (p == "high_chunks" and n <= SCAN_ROUND)]


@pytest.mark.parametrize("shape", [(1080, 1920), (2160, 3840)], ids=["1080p", "4K"])
@pytest.mark.parametrize("n,pattern", HIST_CASES)
def test_id_histogram_above_the_scan_and_grid_thresholds(n, pattern, shape):
    """1024 chunks (one scan round, no carry), 1025 (the carry of a second round with ONE chunk in it), 2049 (the first
    chunk of the grid stride) and about 5 M ids, against torch.unique, exactly."""
    from log_amd import counter
    gen = torch.Generator(device=DEV).manual_seed(n % 1000 + shape[0])
    npix = shape[0] * shape[1]
    pid = _id_map(pattern, n, npix, gen).view(shape)
    ids, counts = counter.unique_ids(pid, n)
    want_ids, want_counts = torch.unique(pid, sorted=True, return_counts=True)
    if want_ids[0] == -1:
        want_ids, want_counts = want_ids[1:], want_counts[1:]
    assert int(want_ids[-1]) == n - 1                                   # the last id of the last chunk is there
    if pattern in ("last_chunk", "high_chunks") and n > SCAN_ROUND:
        assert int(want_ids[0]) >= SCAN_ROUND                           # nothing below the second scan round
    if pattern == "every_chunk":
        assert int(torch.unique(want_ids // CHUNK).numel()) == (n + CHUNK - 1) // CHUNK
    assert ids.dtype == torch.int32 and counts.dtype == torch.int64
    assert torch.equal(ids, want_ids.to(torch.int32)) and torch.equal(counts, want_counts)
    assert int(counts.sum()) == int((pid >= 0).sum())


# ---- LoD ------------------------------------------------------------------------------------------------------------
# (roots, levels, max_child, min_px, root level > chunks, level 1 > chunks)
LOD_CASES = [(1_500_000, 1, 2, 60.0, 1024, 0),        # root scan goes round its carry loop once more
             (2_600_000, 2, 2, 60.0, 2048, 2048)]     # level 1: carry loop AND grid stride of classify / scatter <false>


@pytest.mark.parametrize("n_roots,levels,max_child,min_px,root_chunks,level1_chunks", LOD_CASES)
def test_traverse_above_the_scan_and_grid_thresholds(n_roots, levels, max_child, min_px, root_chunks, level1_chunks,
                                                     oracle_mod):
    """Trees whose root level and whose first level below the roots exceed 1024 / 2048 chunks of 1024 slots, against the
    oracle, exactly, order included.  min_px = 60 at this camera makes the projected-radius test go both ways (with 3 it
    keeps nothing but leaves); the shares are asserted."""
    from log_amd import lod, scenes
    from lod_util import synth_tree
    from test_gpu_lod import _objects
    s = synth_tree(n_roots, levels, max_child, seed=n_roots)
    W, H = 1920, 1080
    cam = scenes.orbit_cameras(8, W=W, H=H)[3]
    tfx, tfy = math.tan(cam["FoVx"] * 0.5), math.tan(cam["FoVy"] * 0.5)
    tree, model, rast = _objects(s["node_index"], s["tree"], s["xyz"], s["scaling"], s["rotation"], W, H, tfx, tfy,
                                 cam["world_view_transform"], cam["full_proj_transform"])
    tree.min_resolution_pixel = min_px
    roots = s["root_index"]
    want = None
    for max_depth in (1000, 1):
        got = lod.traverse(tree, model, torch.from_numpy(roots).cuda(), rast, max_depth=max_depth).cpu().numpy()
        w = oracle_mod.lod_traverse(s["node_index"], s["tree"], s["xyz"], s["scaling"], s["rotation"], roots,
                                    cam["full_proj_transform"], cam["world_view_transform"], W / (2 * tfx),
                                    H / (2 * tfy), tfx, tfy, min_px, 30, max_depth)
        np.testing.assert_array_equal(got, w)
        want = w if want is None else want
    # the sizes really crossed the thresholds, and every level under test both kept and descended a good share
    depth, inner = s["depth"][want], s["node_index"] != -1
    assert n_roots > root_chunks * CHUNK
    kept0 = int((depth == 0).sum())
    kept0_inner = int((inner[want] & (depth == 0)).sum())
    descended0 = n_roots - kept0
    assert kept0 > 0.2 * n_roots and descended0 > 0.2 * n_roots and kept0_inner > 0.02 * n_roots, (kept0, descended0, kept0_inner)
    slots1 = descended0 * max_child
    assert slots1 > level1_chunks * CHUNK, slots1
    if levels > 1:
        kept1 = int((depth == 1).sum())
        kept1_inner = int((inner[want] & (depth == 1)).sum())
        kept2 = int((depth == 2).sum())                                  # every node descended at level 1 hands on its children
        assert kept1 > 0.2 * slots1 and kept2 > 0.2 * slots1 and kept1_inner > 0.02 * slots1, (kept1, kept2, kept1_inner)
    assert len(np.unique(want)) == len(want)


# ---- sparse Adam, 64-bit element indices ----------------------------------------------------------------------------
def test_sparse_adam_with_64_bit_element_indices():
    """One call with m * width >= 2^31 (width 45: K = 15 coefficients x 3): adam_kernel<false>.  Zero moments, so the
    first step moves every visible element by -lr * sign(g) and leaves every other row bit-identical (the identity of
    test_sparse_adam_many_rows_and_untouched_rows); checked in row chunks on the device, the rows whose flat element index
    is >= 2^31 and the last row explicitly.  Five arrays of 8.7 GB."""
    from log_amd import rasterizer as R
    width, m, extra = 45, 48_500_000, 1000
    P = m + extra
    assert m * width >= 2 ** 31 + 10_000_000
    need = 5 * P * width * 4 + 12 * m + (6 << 30)                        # the arrays, index + flag, 6 GiB of working room
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        print("sparse Adam 64-bit case: %.1f GB free, %.1f GB needed" % (free / 1e9, need / 1e9))
        pytest.skip("less than %.1f GB of device memory free" % (need / 1e9))
    gen = torch.Generator(device=DEV).manual_seed(5)
    step_rows = 2_000_000
    model = torch.empty(P, width, device=DEV)
    grad = torch.empty(m, width, device=DEV)
    for a in range(0, P, step_rows):
        model[a:a + step_rows].normal_(generator=gen)
    for a in range(0, m, step_rows):                                     # |g| in [0.5, 1.5): no element near eps
        g = grad[a:a + step_rows]
        g.uniform_(0.5, 1.5, generator=gen)
        g.mul_(torch.randint(0, 2, g.shape, generator=gen, device=DEV, dtype=torch.int8) * 2 - 1)
    # index: a permutation of [0, P) without its last `extra` values (i -> (i * a) mod P, a coprime to P)
    mult = 1_000_003
    assert math.gcd(mult, P) == 1
    index = (torch.arange(m, device=DEV, dtype=torch.int64) * mult) % P
    flag_vis = torch.rand(m, device=DEV, generator=gen) < 0.7
    first_hi = 2 ** 31 // width                                          # first row holding a flat index >= 2^31
    flag_vis[-1] = True
    flag_vis[first_hi] = True
    flag_vis[first_hi + 1] = False
    param = torch.empty(m, width, device=DEV)
    for a in range(0, m, step_rows):
        param[a:a + step_rows] = model[index[a:a + step_rows]]
    outside = torch.ones(P, dtype=torch.bool, device=DEV)
    outside[index] = False
    outside = torch.where(outside)[0]
    assert outside.numel() == extra
    outside_before = model[outside].clone()
    m1, m2 = torch.zeros(P, width, device=DEV), torch.zeros(P, width, device=DEV)
    lr, bc1, bc2 = 1e-3, 1 - 0.9, 1 - 0.999
    R._backend.sparse_adam(index, flag_vis, [(model, param, grad, m1, m2, None, lr / bc1)], 0.9, 0.999, math.sqrt(bc2), 1e-15)
    torch.cuda.synchronize()

    def check(a, b):
        idx, vis = index[a:b], flag_vis[a:b]
        now, was, g = model[idx], param[a:b], grad[a:b]
        assert torch.equal(now[~vis], was[~vis]), (a, b)
        assert bool((m1[idx][~vis] == 0).all()) and bool((m2[idx][~vis] == 0).all()), (a, b)
        torch.testing.assert_close(now[vis] - was[vis], -lr * torch.sign(g[vis]), rtol=1e-3, atol=1e-6)
        torch.testing.assert_close(m1[idx][vis], g[vis] * 0.1, rtol=1e-6, atol=0)       # m = g * (1 - beta1)
        assert bool((m2[idx][vis] > 0).all()), (a, b)

    for a in range(0, m, step_rows):
        check(a, min(a + step_rows, m))
    check(first_hi - 2, m)                                               # every element with a flat index >= 2^31 ...
    check(m - 1, m)                                                      # ... and the last row
    assert bool(flag_vis[first_hi:].any()) and not bool(flag_vis[first_hi:].all())
    assert torch.equal(model[outside], outside_before)
    assert not bool(m1[outside].any())


# ---- KNN ------------------------------------------------------------------------------------------------------------
def _knn_oracle(pts):
    from scipy.spatial import cKDTree
    p64 = pts.astype(np.float64)                                        # from the fp32 coordinates the kernel sees
    d, _ = cKDTree(p64).query(p64, k=4, workers=16)                     # column 0 is the point itself (distance 0)
    return (d[:, 1:] ** 2).mean(axis=1)


def _knn_clouds(name):
    rng = np.random.default_rng(7)
    if name == "uniform_1.5M":
        return rng.random((1_500_000, 3), dtype=np.float32) * np.array([4, 2, 1], np.float32)
    if name == "clustered_1.5M":                 # dense surface patches + sparse far outliers that stretch the bounding box
        centers = rng.normal(size=(200, 3)) * 5
        return np.concatenate([
            centers[rng.integers(0, 200, 1_499_000)] + rng.normal(size=(1_499_000, 3)) * 0.05 * np.array([1, 1, 0.02]),
            rng.normal(size=(1000, 3)) * 200]).astype(np.float32)
    if name.startswith("P="):
        return rng.random((int(name[2:]), 3), dtype=np.float32)
    if name == "plane":                          # zero extent on one axis: the Morton code's ext = 1e-30 branch
        p = rng.random((100_000, 3), dtype=np.float32)
        p[:, 2] = 0.75
        return p
    if name == "line":                           # zero extent on two axes
        p = np.zeros((20_000, 3), np.float32)
        p[:, 1] = rng.random(20_000, dtype=np.float32) * 50
        p[:, 0], p[:, 2] = -2.5, 3.0
        return p
    if name == "far_from_origin":                # spread 1 around (1e4, 1e4, 1e4)
        return (rng.random((100_000, 3)) - 0.5 + 1e4).astype(np.float32)
    if name == "negative":
        return (-1.0 - 4.0 * rng.random((100_000, 3))).astype(np.float32)
    raise KeyError(name)


KNN_CLOUDS = ["uniform_1.5M", "clustered_1.5M", "P=4", "P=5", "P=1023", "P=1024", "P=1025", "plane", "line",
              "far_from_origin", "negative"]


@pytest.mark.parametrize("name", KNN_CLOUDS)
def test_dist_cuda2_sizes_and_degenerate_clouds(name):
    from simple_knn._C import distCUDA2
    pts = _knn_clouds(name)
    out = distCUDA2(torch.tensor(pts, device=DEV)).cpu().numpy()
    ref = _knn_oracle(pts)
    assert out.shape == ref.shape and np.isfinite(out).all()
    scale = float(np.abs(pts).max()) ** 2
    err = np.abs(out - ref)
    print("%s: max abs err %.3e, max rel err %.3e" % (name, err.max(), (err / np.maximum(ref, 1e-30)).max()))
    np.testing.assert_allclose(out, ref, rtol=2e-4, atol=2e-6 * scale)  # tests/test_gpu_knn.py's tolerance
    # That atol says little where the cloud is small against its coordinates (200 far from the origin, 5e-3 on the line, about
    # 1 for the clusters with their outliers, against values of 1e-5).  So, on every cloud, relative to the value itself: the
    # oracle starts from the same fp32 coordinates; a difference of two of them is rounded once (2^-24 of itself, however
    # large the coordinates), its square carries that twice plus its own rounding, the sum of three non-negative squares two
    # more, the mean of three such sums two more and the division one: 8 roundings, 4.8e-7.  Equal points give exactly 0.
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=0)


def test_dist_cuda2_fewer_than_four_points():
    """Fewer than 3 other points (distCUDA2's docstring): a missing neighbour counts as the 3.4e38 the best-3 list starts
    from, like simple-knn's FLT_MAX; the mean is taken in fp32.  So P = 3 gives (d1 + d2 + 3.4e38) / 3, finite, and
    P <= 2 gives +inf; never NaN."""
    from simple_knn._C import distCUDA2
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [-3.0, 0.0, 4.0]], np.float32)
    big = np.float32(3.4e38)
    for P in (1, 2, 3):
        out = distCUDA2(torch.tensor(pts[:P], device=DEV)).cpu().numpy()
        assert out.shape == (P,) and not np.isnan(out).any()
        if P < 3:
            assert np.isposinf(out).all()
        else:
            d = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
            want = np.array([(np.float32(np.sort(d[i])[1] + np.sort(d[i])[2]) + big) / np.float32(3.0) for i in range(3)],
                            np.float32)
            assert np.isfinite(want).all()
            np.testing.assert_array_equal(out, want)

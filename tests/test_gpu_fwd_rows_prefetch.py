"""The row-split forward (lr_blend_fwd_rows_kernel, both EXTRAS flavours) on the smallest shapes at which its chunk loop can go
wrong: the two-chunk prefetch (the gather of chunk ch + 1 and the ids of chunk ch + 2 are requested while chunk ch is
composited), the per-chunk commit of point_weight, the hit-mask buffer and its flush, and the park / resume of a lazily
ordered list.  The kernel keeps its wave index, and with it the quadrant origin, the LDS bases and the mask bookkeeping, in
scalar registers (tests/test_kernel_resources_cpu.py: no scratch); nothing it computes may change by that.

Shapes:
  64x64 (16 tiles) and 48x40 (partial tiles on both edges), random scenes;
  one list of exactly L entries in one tile (the other tiles but one are lists of 0 entries), starting at list offset 37:
    L = 0, 1, 63, 64, 65, 129    chunk boundaries: a last partial chunk, and the id load of the "chunk after next" past the end;
    L = 64 * LR_MBUF_CHUNKS + 1  the wave's LDS mask buffer fills once: it is flushed in the walk and again after it;
    L = 8193                     the first ordered window ends (at about 7680) with pixels open: the waves park their state
                                 in the outputs and resume in the second pass.
  In a list the deepest eighth of the entries lies over pixels that nothing nearer touches, so the entries of the last chunks
  -- behind a flush, behind the window's end -- contribute: some pixel's last contributor is the list's last entry (8193:
  an entry behind the first window's end).
Every shape with opacity 0.999 and with random opacities, in both flavours, pinned to the row-split form with walk_form.

Every case: the forward runs on NaN-poisoned allocations (tests/poison.py; the hit-mask buffer alone is zero-filled, which
is what decoding it needs) and its lists, image, final_T, n_contrib and per-pixel maps are the oracle's bit for bit.  Its hit
masks name exactly the Gaussians with point_weight > 0, hold no bit behind a block's deepest contributor and one at it, and
the reverse walk on them sums what a walk that finds its visits itself sums (up to the order of the float atomics)."""
import numpy as np
import pytest

import list_cases as LC
import poison as P
from util import rel_l2, small_case

pytestmark = pytest.mark.gpu

BG = (0.3, 0.6, 0.9)
EXACT = ("radii_mismatch", "rec_bits_mismatch", "offsets_mismatch", "list_mismatch", "n_contrib_mismatch",
         "image_bits_mismatch", "final_T_bits_mismatch")
WALK = ("means2D", "conic", "opacities", "colors")
ORDER_TOL = 1e-5              # two reverse walks over the same visits: the order of the float atomics (test_gpu_list_boundaries.py)
def _mbuf_chunks():
    """LR_MBUF_CHUNKS as log_amd/csrc/blend.hip defines it: the flush case follows the constant."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "log_amd", "csrc", "blend.hip")).read()
    return int(re.search(r"^#define\s+LR_MBUF_CHUNKS\s+(\d+)u?\b", src, re.M).group(1))


MBUF_ENTRIES = 64 * _mbuf_chunks()   # entries a wave walks between two bursts of mask stores
T4, BEG = LC.MAIN_TILE, 37
LENGTHS = [0, 1, 63, 64, 65, 129, MBUF_ENTRIES + 1, 8193]
SHAPES = ["64x64", "48x40"] + ["list-%d" % L for L in LENGTHS]
OPACITIES = ["0.999", "rand"]
FLAVOURS = ["wodilate", "upstream"]


def _splats(u, v, z32, rng):
    """Isotropic Gaussians LC.SIGMA_PX wide whose centres project to pixel (u, v) of LC.camera() at view depth z32."""
    n = len(z32)
    z = z32.astype(np.float64)
    xyz = np.stack([(u + 0.5 - LC.W / 2.0) * z / LC.FOCAL, (v + 0.5 - LC.H / 2.0) * z / LC.FOCAL, z], 1).astype(np.float32)
    xyz[:, 2] = z32
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(xyz=xyz, scaling=np.repeat((LC.SIGMA_PX * z / LC.FOCAL).reshape(n, 1), 3, axis=1).astype(np.float32),
                rotation=q.astype(np.float32), opacity=np.zeros((n, 1), np.float32), colors=rng.random((n, 3), dtype=np.float32))


def _one_list(L, rng):
    """BEG entries in tile 0 and L in tile T4 (pixels 16..31 on both axes), distinct depths.  The list's nearer entries lie
    over the tile's pixels 2..10, its deepest max(1, L // 8) over pixels 8..14: pixel (11, 11) meets only those, and the
    tile's corner pixels meet nothing, so every wave walks the list to its end."""
    z0, z = LC.depths(BEG, "spread", rng), LC.depths(L, "spread", rng)
    u0, v0 = rng.uniform(4.5, 11.5, BEG), rng.uniform(4.5, 11.5, BEG)
    deep = np.zeros(L, bool)
    deep[np.argsort(z, kind="stable")[L - max(1, L // 8):]] = True
    x0, y0 = 16 * (T4 % LC.GX), 16 * (T4 // LC.GX)
    u = x0 + np.where(deep, rng.uniform(10.5, 11.5, L), rng.uniform(4.5, 7.5, L))
    v = y0 + np.where(deep, rng.uniform(10.5, 11.5, L), rng.uniform(4.5, 7.5, L))
    parts = [_splats(u0, v0, z0, rng), _splats(u, v, z, rng)]
    return LC.camera(), {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def scene(shape, opacity):
    """-> (cam, sc).  Random opacities: U(0.1, 1) -- every splat passes the 1/255 floor at its own centre, so a list keeps the
    length it was built with."""
    rng = np.random.default_rng([11, SHAPES.index(shape), OPACITIES.index(opacity)])
    if shape.startswith("list-"):
        cam, sc = _one_list(int(shape[5:]), rng)
    else:
        W, H = (int(x) for x in shape.split("x"))
        cam, sc = small_case(n=400, W=W, H=H, seed=3)
        sc = dict(sc)
    n = len(sc["xyz"])
    sc["opacity"] = (np.full((n, 1), 0.999) if opacity == "0.999" else rng.uniform(0.1, 1.0, (n, 1))).astype(np.float32)
    return cam, sc


def _flavour(name):
    from log_amd import rasterizer as R
    return {"wodilate": R.WODILATE, "upstream": R.UPSTREAM}[name]


_refs = {}


def _reference(oracle_mod, shape, opacity, flavour_name):
    """The scene and the oracle's forward of it: computed once per case, shared, left unchanged."""
    import gpu_util as G
    key = (shape, opacity, flavour_name)
    if key not in _refs:
        cam, sc = scene(shape, opacity)
        _refs[key] = (cam, sc, G.oracle_forward(oracle_mod, cam, sc, BG, flavour=_flavour(flavour_name))[1])
    return _refs[key]


def _assert_masks(hf, n):
    """The decoded hit masks against the forward's own outputs (tests/test_gpu_exact_masks.py has the same rules)."""
    import gpu_util as G
    H, W = hf["n_contrib"].shape
    exact = G.visits(hf)
    with_bit = np.zeros(n, bool)
    with_bit[hf["point_list"][exact.any(axis=1)]] = True
    if "point_weight" in hf:
        assert (with_bit == (hf["point_weight"] > 0)).all(), int((with_bit != (hf["point_weight"] > 0)).sum())
    nc = np.zeros((((H + 15) // 16) * 16, ((W + 15) // 16) * 16), np.int64)
    nc[:H, :W] = hf["n_contrib"]
    gy, gx = nc.shape[0] // 16, nc.shape[1] // 16
    rmax = nc.reshape(gy, 2, 2, 4, gx, 2, 2, 4).max(axis=(3, 7)).transpose(0, 3, 1, 4, 2, 5).reshape(gy * gx, 16)
    offs = hf["tile_offsets"].astype(np.int64)
    lens = np.diff(offs)
    tile = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(hf["I"]) - offs[tile]
    assert not (exact & (pos[:, None] >= rmax[tile])).any()     # no bit behind a block's deepest contributor ...
    deepest = np.zeros_like(rmax)
    rows, cols = np.nonzero(exact)
    np.maximum.at(deepest, (tile[rows], cols), pos[rows] + 1)
    assert (deepest == rmax).all()                              # ... and one at it
    return exact


@pytest.mark.parametrize("flavour_name", FLAVOURS)
@pytest.mark.parametrize("opacity", OPACITIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_row_split_forward(oracle_mod, shape, opacity, flavour_name):
    import gpu_util as G
    from log_amd import rasterizer as R
    cam, sc, of = _reference(oracle_mod, shape, opacity, flavour_name)
    fl = _flavour(flavour_name)
    prev_zero, R._zero_hit_masks = R._zero_hit_masks, True
    try:
        with R.walk_form("rows"), P.poisoned("nan") as census:
            hf = G.hip_forward(cam, sc, BG, flavour=fl, scratch_floats=16)
    finally:
        R._zero_hit_masks = prev_zero
    assert hf["fwd_form"] == "rows" and {"geom", "state", "final_T", "n_contrib"} <= census.parts(), census.parts()
    assert ("point_weight" in hf) == (flavour_name == "wodilate")            # EXTRAS = true / false
    st = G.compare_forward(hf, of)
    for k in EXACT + (("pid_mismatch",) if "pid_mismatch" in st else ()):
        assert st[k] == 0, (k, st)
    if "pwp_max_abs" in st:
        assert st["pwp_max_abs"] == 0.0 and st["pw_max_abs"] == 0.0, st
    assert np.isfinite(hf["image"]).all() and np.isfinite(hf["final_T"]).all()
    lens = np.diff(hf["tile_offsets"].astype(np.int64))
    if shape.startswith("list-"):
        # the scene is what its name says
        L = int(shape[5:])
        assert lens[T4] == L and lens[0] == BEG and (lens == 0).sum() >= LC.GX * LC.GY - 2, lens
        tile = (slice(16, 32), slice(16, 32))
        assert hf["final_T"][tile].max() == 1.0                 # a pixel nothing touches: its wave never stops early
        # the list's last entry contributes (a list of two windows: entries behind the first window's end do)
        assert hf["n_contrib"][tile].max() == L if L <= LC.LONG_WIN else hf["n_contrib"][tile].max() > LC.LONG_WIN
        first, opened = int(hf["first_window"][T4]), int(hf["open_words"][T4])
        print("%s %s %s: first window %d, open %#x, LR_HDR_OPEN %d" % (shape, opacity, flavour_name, first, opened, hf["hdr_open"]))
        assert not np.delete(hf["open_words"], T4).any() and hf["lazy_lists"] == 0
        if L > LC.LONG_WIN:                                     # parked at the window's end, resumed, and went on accumulating
            assert LC.LONG_WIN - LC.BUCKET_MAX < first <= LC.LONG_WIN and opened == 0xf and hf["hdr_open"] == 1
            assert ((hf["n_contrib"][tile] > 0) & (hf["n_contrib"][tile] <= first)).any()
        else:
            assert first == L and opened == 0 and hf["hdr_open"] == 0
    else:
        W, H = (int(x) for x in shape.split("x"))
        assert hf["image"].shape == (3, H, W) and len(lens) == ((W + 15) // 16) * ((H + 15) // 16) and lens.max() > 64, lens
    exact = _assert_masks(hf, len(sc["xyz"]))
    assert exact.any()
    if shape.startswith("list-") and int(shape[5:]) > MBUF_ENTRIES:
        # the wave's mask buffer filled and was written out inside the walk: visits on both sides of that burst came through
        b = int(hf["tile_offsets"][T4])
        assert exact[b:b + MBUF_ENTRIES].any() and exact[b + MBUF_ENTRIES:b + int(shape[5:])].any()
    # the reverse walk on these masks against a walk that runs the support tests itself: the same visits but for exact zeros
    dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
    g = G.hip_backward(hf, dL, bwd_form="rows")
    with R.walk_form("rows"):
        hf1 = G.hip_forward(cam, sc, BG, flavour=fl, scratch_floats=16, hit_masks=False)
    g1 = G.hip_backward(hf1, dL, bwd_form="rows")
    assert g["bwd_masks"] and not g1["bwd_masks"]
    for k in WALK:
        assert np.isfinite(g[k]).all() and g1[k].any(), k
        assert rel_l2(g[k], g1[k]) < ORDER_TOL, (k, rel_l2(g[k], g1[k]))

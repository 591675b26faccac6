"""The row-split compositing kernel's hit masks record CONTRIBUTIONS (LOGRAST_HIT_MASKS=1, default): bit j of a 4x4
block's mask of a 64-entry chunk is set iff some pixel of the block accumulated entry j.  With the knob at 2 the masks are
the ballots of the support tests, a superset: an entry whose alpha >= 1/255 region touches the block's hull without
reaching a pixel centre, that meets only saturated pixels, or that lies behind every pixel's last contributor gets a
support bit and adds exactly +-0 to every sum of the reverse walk.

Checked on scenes of a 72x40 image (not a multiple of the tile: lanes outside the image), both flavours (the fork's kernel
has the row maxima at hand, upstream's takes the row's share of two ballots):
  the forward's outputs do not depend on the knob, bit for bit; the contribution masks are a bitwise subset of the support
  masks (a strict one where rows finish early or splats graze blocks); the Gaussians with a bit are exactly those with
  point_weight > 0; the masked walk's gradients are the oracle's, and the support-mask walk's up to the order of the float
  atomics (bit for bit where every Gaussian has a single contributing visit); a zeroed buffer means no visit at all."""
import numpy as np
import pytest

from util import rel_l2

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4   # relative L2 against the oracle (BASELINE.json)
W, H = 72, 40
BG = (0.3, 0.6, 0.9)
MBUF_ENTRIES = 64 * 64   # 64 * LR_MBUF_CHUNKS (blend.hip): entries a wave walks between two bursts of mask stores


def _cam():
    from log_amd import scenes
    return scenes.orbit_cameras(3, W=W, H=H, focal=60.0, radius=2.5)[1]


def _place(cam, u, v, z, sigma_px, opacity, rng, aniso=None):
    """Gaussians whose centres project to pixel (u, v) at view depth z, about sigma_px pixels wide (aniso: per-axis
    factors, with random orientations)."""
    n = len(u)
    f = float(cam["K"][0, 0])
    z = np.asarray(z, np.float64)
    pc = np.stack([(np.asarray(u, np.float64) + 0.5 - W / 2.0) * z / f, (np.asarray(v, np.float64) + 0.5 - H / 2.0) * z / f, z], 1)
    R, T = cam["R"].astype(np.float64), cam["T"].astype(np.float64).reshape(1, 3)
    xyz = (pc - T) @ R                                          # rows of R^T (p - T)
    s = (np.asarray(sigma_px, np.float64) * z / f).reshape(n, 1) * (np.ones((n, 3)) if aniso is None else aniso)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(xyz=xyz.astype(np.float32), scaling=s.astype(np.float32), rotation=q.astype(np.float32),
                opacity=np.broadcast_to(np.asarray(opacity, np.float32).reshape(-1, 1), (n, 1)).copy(),
                colors=rng.random((n, 3), dtype=np.float32))


def _cat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _scene(name):
    cam = _cam()
    rng = np.random.default_rng(7)
    if name == "stack":
        # 300 nearly opaque splats one behind the other over the first 4x4 block of a quadrant: that block's row is
        # saturated after three entries, the far block of the quadrant (alpha ~ 0.01) is still open after all five chunks;
        # a few faint splats elsewhere, and tiles without any entry
        n = 300
        st = _place(cam, np.full(n, 17.5), np.full(n, 17.5), 2.0 + 1e-3 * np.arange(n), 2.5, 0.999, rng)
        m = 40
        rest = _place(cam, rng.uniform(40, 52, m), rng.uniform(2, 14, m), 2.0 + 1e-3 * rng.permutation(m), 1.0, 0.4, rng)
        return cam, _cat(st, rest)
    if name == "grazing":
        # splats of about 2 px radius centred between pixel centres on the borders of the 4x4 blocks (a little jitter, mild
        # anisotropy), all over the image including its ragged right and bottom edges: regions that touch a block's hull
        # between its pixel centres
        n = 1500
        u = 3.5 + 4.0 * rng.integers(0, W // 4, n) + rng.uniform(-0.5, 0.5, n)
        v = 3.5 + 4.0 * rng.integers(0, H // 4, n) + rng.uniform(-0.5, 0.5, n)
        on_x = rng.random(n) < 0.5                              # on a vertical border / on a horizontal border
        u = np.where(on_x, u, u - 2.0)
        v = np.where(on_x, v - 2.0, v)
        return cam, _place(cam, u, v, 2.0 + 1e-4 * rng.permutation(n), 0.67, 0.3, rng, aniso=rng.uniform(0.6, 1.4, (n, 3)))
    if name == "flush":
        # one tile holding more than 64 * LR_MBUF_CHUNKS faint entries and no pixel ever stops: the wave's LDS mask buffer
        # is written out in the middle of the walk and filled again
        n = 4700
        return cam, _place(cam, rng.uniform(33, 46, n), rng.uniform(17, 30, n), 2.0 + 1e-4 * rng.permutation(n), 0.7, 0.02, rng)
    if name == "park":
        # one tile above 7680 keys with pixels left open: its waves park at the end of the first ordered window and resume
        # in the second pass (tests/test_gpu_scale.py: test_every_long_list_needs_its_tail, at the smallest size that parks)
        n = 9000
        return cam, _place(cam, rng.uniform(33, 46, n), rng.uniform(17, 30, n), 2.0 + 1e-4 * rng.permutation(n), 0.7, 0.02, rng)
    if name == "flat":
        # the same tile and count as `park`, at three distinct depths with thousands of ties each: the depth buckets of the
        # long-list sort overflow and the list goes to the network, which orders it to its END in the first pass
        # (tests/test_gpu_parity.py: the flat_depth_* recipe)
        n = 9000
        return cam, _place(cam, rng.uniform(33, 46, n), rng.uniform(17, 30, n), 2.0 + 1e-3 * rng.integers(0, 3, n), 0.7, 0.02, rng)
    if name == "apart":
        # one faint small splat in the middle of every 4x4 block: each reaches pixels of its own block only, so every
        # Gaussian has ONE contributing visit and no sum depends on the order of the atomics
        bx, by = np.meshgrid(np.arange(W // 4), np.arange(H // 4))
        u, v = 4.0 * bx.reshape(-1) + 1.5, 4.0 * by.reshape(-1) + 1.5
        return cam, _place(cam, u, v, 2.0 + 1e-3 * rng.permutation(len(u)), 0.6, 0.1, rng)
    raise KeyError(name)


def _flavour(name):
    from log_amd import rasterizer as R
    return {"wodilate": R.WODILATE, "upstream": R.UPSTREAM}[name]


_CACHE = {}


def _run(oracle_mod, name, flavour_name):
    """Forward with LOGRAST_HIT_MASKS at 1 and at 2 (keys 1 and 0 below) (zero-filled mask buffers), the oracle, and the gradients of three reverse
    walks: on the contribution masks, on the support masks, on a zeroed buffer.  Computed once per (scene, flavour)."""
    key = (name, flavour_name)
    if key in _CACHE:
        return _CACHE[key]
    import gpu_util as G
    from log_amd import rasterizer as R, tune
    cam, sc = _scene(name)
    fl = _flavour(flavour_name)
    v, of = G.oracle_forward(oracle_mod, cam, sc, BG, flavour=fl)
    dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
    og = oracle_mod.backward(v, of, dL)
    hf, g = {}, {}
    prev_zero, R._zero_hit_masks = R._zero_hit_masks, True
    try:
        for knob in (1, 0):
            tune.set_knob("LOGRAST_HIT_MASKS", 1 if knob else 2)
            hf[knob] = G.hip_forward(cam, sc, BG, flavour=fl, scratch_floats=16, fwd_form="rows")
            g[knob] = G.hip_backward(hf[knob], dL, bwd_form="rows")
            assert g[knob]["bwd_masks"]
    finally:
        R._zero_hit_masks = prev_zero
        tune.reset_knobs()
    vis = {k: G.visits(hf[k]) for k in (1, 0)}
    hf[1]["_torch"][-1]["hit_masks"].zero_()
    g["zeroed"] = G.hip_backward(hf[1], dL, bwd_form="rows")
    out = dict(cam=cam, sc=sc, of=of, og=og, hf=hf, g=g, vis=vis)
    _CACHE[key] = out
    return out


SCENES = ["stack", "grazing", "flush", "park", "apart"]
FLAVOURS = ["wodilate", "upstream"]


@pytest.mark.parametrize("flavour_name", FLAVOURS)
@pytest.mark.parametrize("name", SCENES)
def test_forward_outputs_do_not_depend_on_the_knob(oracle_mod, name, flavour_name):
    import gpu_util as G
    r = _run(oracle_mod, name, flavour_name)
    a, b = r["hf"][1], r["hf"][0]
    keys = ["image", "final_T"] + (["point_weight"] if "point_weight" in a else [])
    for k in keys:
        assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), k
    assert (a["n_contrib"] == b["n_contrib"]).all() and (a["point_list"] == b["point_list"]).all()
    assert (a["tile_offsets"] == b["tile_offsets"]).all()
    st = G.compare_forward(a, r["of"])                          # and they are the oracle's
    for k in ("offsets_mismatch", "list_mismatch", "n_contrib_mismatch", "image_bits_mismatch", "final_T_bits_mismatch"):
        assert st[k] == 0, (k, st)
    # the scene is what its name says
    lens = np.diff(a["tile_offsets"].astype(np.int64))
    if name == "stack":
        assert (lens == 0).any() and lens.max() > 256          # empty tiles; rows finish chunks apart (below)
    if name == "flush":
        assert MBUF_ENTRIES < lens.max() <= 7680 and a["n_contrib"].max() > MBUF_ENTRIES
    if name == "park":
        assert lens.max() > 7680 and a["n_contrib"].max() > 7680 and a["lazy_lists"] == 0   # walked into the tail


@pytest.mark.parametrize("flavour_name", FLAVOURS)
@pytest.mark.parametrize("name", SCENES)
def test_contribution_masks_are_a_subset_of_the_support_masks(oracle_mod, name, flavour_name):
    r = _run(oracle_mod, name, flavour_name)
    exact, support = r["vis"][1], r["vis"][0]
    print("%s %s: support visits %d, contributing visits %d" % (name, flavour_name, support.sum(), exact.sum()))
    assert exact.any() and not (exact & ~support).any()
    if name in ("stack", "grazing"):
        assert exact.sum() < support.sum()
    hf = r["hf"][1]
    if name == "stack":
        # the stack's quadrant (tile 6 = (1, 1), wave 0): its first block stops after a few entries and leaves zero masks in
        # every later chunk, where the support ballots still name every entry; its far block goes on to the end
        offs = hf["tile_offsets"].astype(np.int64)
        t = (17 // 16) * ((W + 15) // 16) + 17 // 16
        e, s = exact[offs[t]:offs[t + 1]], support[offs[t]:offs[t + 1]]
        assert len(e) >= 300
        assert e[:64, 0].any() and not e[64:, 0].any() and s[64:, 0].sum() >= 200
        assert e[256:, 3].any()
    # a Gaussian has a bit somewhere iff it contributed to some pixel (point_weight = its largest alpha T over the image;
    # upstream's package has no such output: there, every Gaussian the oracle's colour gradient reaches has a bit)
    with_bit = np.zeros(len(r["sc"]["xyz"]), bool)
    with_bit[hf["point_list"][exact.any(axis=1)]] = True
    assert with_bit[(r["og"]["colors"] != 0).any(axis=1)].all()
    if "point_weight" in hf:
        assert (with_bit == (hf["point_weight"] > 0)).all(), int((with_bit != (hf["point_weight"] > 0)).sum())
    # no bit behind a block's deepest contributor, and the deepest contributor of every block has one
    nc = np.zeros((((H + 15) // 16) * 16, ((W + 15) // 16) * 16), np.int64)
    nc[:H, :W] = hf["n_contrib"]
    gy, gx = nc.shape[0] // 16, nc.shape[1] // 16
    rmax = nc.reshape(gy, 2, 2, 4, gx, 2, 2, 4).max(axis=(3, 7)).transpose(0, 3, 1, 4, 2, 5).reshape(gy * gx, 16)
    offs = hf["tile_offsets"].astype(np.int64)
    lens = np.diff(offs)
    tile = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(hf["I"]) - offs[tile]
    assert not (exact & (pos[:, None] >= rmax[tile])).any()
    deepest = np.zeros_like(rmax)
    rows, cols = np.nonzero(exact)
    np.maximum.at(deepest, (tile[rows], cols), pos[rows] + 1)
    assert (deepest == rmax).all()


@pytest.mark.parametrize("flavour_name", FLAVOURS)
@pytest.mark.parametrize("name", SCENES)
def test_masked_walk_gradients(oracle_mod, name, flavour_name):
    r = _run(oracle_mod, name, flavour_name)
    g, g0, og = r["g"][1], r["g"][0], r["og"]
    for k in ("means2D", "conic", "opacities", "colors"):
        e, e0 = rel_l2(g[k], og[k]), rel_l2(g[k], g0[k])
        print("%s %s %s: against the oracle %.2e, against the support-mask walk %.2e" % (name, flavour_name, k, e, e0))
        assert e < GRAD_TOL, (k, e)
        assert e0 < 1e-5, (k, e0)
    for k in ("means3D", "scales", "rotations"):
        assert rel_l2(g[k], g0[k]) < 1e-4, (k, rel_l2(g[k], g0[k]))
    gz = r["g"]["zeroed"]                                       # the masks ARE the visits: none left, nothing summed
    assert gz["bwd_masks"] and not gz["colors"].any() and not gz["conic"].any() and not gz["opacities"].any()
    assert not gz["means2D"].any()


@pytest.mark.parametrize("flavour_name", FLAVOURS)
def test_single_visit_rows_are_bit_identical(oracle_mod, flavour_name):
    """Non-overlapping splats: one contributing visit per Gaussian, so each accumulator row receives one commit and the two
    walks -- with and without the visits that add +-0 -- must agree in every bit."""
    r = _run(oracle_mod, "apart", flavour_name)
    exact = r["vis"][1]
    per_gaussian = np.bincount(r["hf"][1]["point_list"][np.nonzero(exact)[0]], minlength=len(r["sc"]["xyz"]))
    assert per_gaussian.max() == 1 and per_gaussian.sum() > 100, (per_gaussian.max(), per_gaussian.sum())
    g, g0 = r["g"][1], r["g"][0]
    for k in ("means2D", "conic", "opacities", "colors"):
        assert g[k].any() and (g[k].view(np.uint32) == g0[k].view(np.uint32)).all(), k


@pytest.mark.parametrize("form", ["rows", "quadrant"])
@pytest.mark.parametrize("name", ["flush", "flat", "park"])
def test_a_list_ordered_to_its_end_parks_nobody(oracle_mod, name, form):
    """A streamed list (more than 4096 keys) whose length is no multiple of 64 and whose pixels never stop.  `flush`
    (4700 keys: the first window holds the whole list) and `flat` (9000 keys at three depths: the network fallback) are
    ordered to their end by the first pass, so the first compositing pass must walk them to their last entry: no wave parks
    for the entries behind the last whole 64-entry chunk (open[] and header word LR_HDR_OPEN stay zero, so the second sort /
    compositing pair has nothing to do).  `park` is the control: 9000 keys at distinct depths are ordered over the first
    window only, and there the waves must still park and resume.  Both compositing forms; forward bit for bit the
    oracle's, and the reverse walk on the forward's hit masks within GRAD_TOL, as for every other scene."""
    import gpu_util as G
    cam, sc = _scene(name)
    v, of = G.oracle_forward(oracle_mod, cam, sc, BG)
    hf = G.hip_forward(cam, sc, BG, scratch_floats=16, fwd_form=form)
    lens = np.diff(hf["tile_offsets"].astype(np.int64))
    t = int(lens.argmax())
    L = int(lens[t])
    assert L % 64 != 0, L
    assert (4096 < L <= 7680) if name == "flush" else L > 7680, L
    assert (lens > 4096).sum() == 1                                     # the one list this test is about
    assert hf["final_T"].min() > 1e-4                                   # no pixel ever stopped ...
    assert hf["n_contrib"].max() > (L & ~63)                            # ... and some pixel's walk went into the last, partial chunk
    st = G.compare_forward(hf, of)
    for k in ("radii_mismatch", "rec_bits_mismatch", "offsets_mismatch", "list_mismatch", "n_contrib_mismatch",
              "image_bits_mismatch", "final_T_bits_mismatch", "pid_mismatch"):
        assert st[k] == 0, (k, st)
    assert hf["lazy_lists"] == 0 and hf["ordered_len"][t] == L          # the walked list is in final order to its end
    print("%s %s: L = %d, open[tile] = %#x, LR_HDR_OPEN = %d" % (name, form, L, hf["open_words"][t], hf["hdr_open"]))
    if name == "park":
        assert hf["hdr_open"] == 1 and hf["open_words"][t] != 0 and not np.delete(hf["open_words"], t).any()
    else:
        assert hf["hdr_open"] == 0 and not hf["open_words"].any(), (hf["hdr_open"], hf["open_words"][t])
    dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
    og = oracle_mod.backward(v, of, dL)
    g = G.hip_backward(hf, dL, bwd_form=form)
    assert g["bwd_masks"]
    for k in ("means2D", "conic", "opacities", "colors"):
        assert rel_l2(g[k], og[k]) < GRAD_TOL, (k, rel_l2(g[k], og[k]))

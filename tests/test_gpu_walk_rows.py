"""The reverse walk's nine sums (eleven with the absolute ones) held ROW BY ROW, SLOT BY SLOT against the float64 twin
(tests/gpu_util.py: walk_row_stats / assert_walk_rows) on scenes built for the places where the walk can go wrong without an
aggregate noticing: the lane-to-slot routes of the packed reductions, the pair loop's second entry, splats across tile /
quadrant / block borders, lanes outside the image, transmittance amplified by 1 / (1 - alpha) at the clamp, the aux form's
fifteen sums.  Both forms (lr_blend_bwd_rows_kernel, lr_blend_bwd_kernel), with the forward's hit masks and without.

Camera as in tests/list_cases.py: R = I, T = 0, so a splat's pixel centre, depth and width are what the scene says.  Images of
at most 64x48; the references of a scene are computed once."""
import numpy as np
import pytest
import torch

from log_amd import scenes

pytestmark = pytest.mark.gpu

FOCAL = 60.0
FORMS = [("rows", True), ("rows", False), ("quadrant", True), ("quadrant", False)]
FORM_IDS = ["rows-masks", "rows-nomasks", "quadrant-masks", "quadrant-nomasks"]
BG = (0.3, 0.6, 0.9)
_REF = {}


def _camera(W, H):
    K = np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1.0]])
    return scenes.make_camera(np.eye(3), np.zeros(3), K, W=W, H=H)


def _splats(W, H, u, v, z, sigma_px, opacity, seed):
    """Isotropic Gaussians centred on pixel coordinates (u, v) at depth z, sigma_px wide."""
    rng = np.random.default_rng(seed)
    u, v, z = (np.asarray(a, np.float64).reshape(-1) for a in (u, v, z))
    n = len(u)
    xyz = np.stack([(u + 0.5 - W / 2.0) * z / FOCAL, (v + 0.5 - H / 2.0) * z / FOCAL, z], 1).astype(np.float32)
    s = np.repeat((np.broadcast_to(np.asarray(sigma_px, np.float64), (n,)) * z / FOCAL).reshape(n, 1), 3, axis=1)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(xyz=xyz, scaling=s.astype(np.float32), rotation=q.astype(np.float32),
                opacity=np.broadcast_to(np.asarray(opacity, np.float32), (n,)).reshape(n, 1).copy(),
                colors=(0.1 + 0.8 * rng.random((n, 3))).astype(np.float32))


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


# ---- scenes: () -> (W, H, sc) -------------------------------------------------------------------------------------------

def every_lane():
    """256 one-pixel splats, one under each pixel of tile (1, 1) of a 48x32 image, (0.25, -0.15) px off the pixel's centre:
    narrower than the low-pass (so 0.3 px^2 wide after it) and faint enough that the neighbouring pixels fall under the alpha
    floor -- each row's nine sums come from ONE lane of one wave, through that lane's route alone."""
    W, H = 48, 32
    ys, xs = np.mgrid[16:32, 16:32]
    z = 2.0 + 1e-3 * np.random.default_rng(5).permutation(256)
    return W, H, _splats(W, H, xs.reshape(-1) + 0.25, ys.reshape(-1) - 0.15, z, 0.35, 0.006, 5)


PAIR_STACKS = [(28, 28, 64), (16, 16, 1), (20, 16, 2), (24, 20, 3)]      # (block x, block y, splats)


def pair_parity():
    """Stacks of 64, 1, 2 and 3 faint splats over four different 4x4 blocks of one tile, nearest first: the 64 fill the list's
    first 64-entry chunk (a row with 32 full pairs), the second chunk has rows with one visit (entry b is the all-zero slot),
    two, and three (a pair and a single)."""
    W, H = 48, 32
    parts = []
    for k, (bx, by, n) in enumerate(PAIR_STACKS):
        rng = np.random.default_rng(k)
        parts.append(_splats(W, H, bx + 1.3 + rng.uniform(-0.2, 0.2, n), by + 1.8 + rng.uniform(-0.2, 0.2, n),
                             2.0 + 0.01 * k + 1e-4 * np.arange(n), 0.6, 0.03 if n == 64 else 0.4, 10 + k))
    return W, H, _cat(parts)


def straddling():
    """Wide splats on the corners where four tiles, four quadrants and four blocks meet (64x48: 4x3 tiles)."""
    W, H = 64, 48
    pts = [(16, 16), (32, 16), (48, 32), (32, 32), (24, 24), (40, 8), (20, 20), (36, 28), (16, 32), (48, 16), (8, 40), (56, 24)]
    rng = np.random.default_rng(6)
    u = np.array([p[0] for p in pts]) - 0.5 + rng.uniform(-0.3, 0.3, len(pts))
    v = np.array([p[1] for p in pts]) - 0.5 + rng.uniform(-0.3, 0.3, len(pts))
    return W, H, _splats(W, H, u, v, 2.0 + 0.05 * rng.permutation(len(pts)), rng.uniform(1.5, 3.5, len(pts)), 0.5, 6)


def _ragged(W, H):
    rng = np.random.default_rng(W)
    n = 60
    return W, H, _splats(W, H, rng.uniform(-1.0, W, n), rng.uniform(-1.0, H, n), 2.0 + 0.01 * rng.permutation(n),
                         rng.uniform(0.6, 2.5, n), rng.uniform(0.1, 0.9, n), W)


def ragged_33x17():
    return _ragged(33, 17)


def ragged_15x17():
    return _ragged(15, 17)


def opaque_stacks():
    """70 near-opaque splats (alpha at the 0.99 clamp under their centres: 1 / (1 - alpha) = 100), half of them in front of one
    wide transparent splat and half behind it."""
    W, H = 48, 32
    rng = np.random.default_rng(8)
    n = 70
    z = np.where(np.arange(n) % 2 == 0, 1.5, 2.5) + 1e-3 * rng.permutation(n)
    dense = _splats(W, H, rng.uniform(4.0, W - 4.0, n), rng.uniform(4.0, H - 4.0, n), z, rng.uniform(1.0, 2.0, n), 0.999, 8)
    veil = _splats(W, H, [W / 2.0 - 0.2], [H / 2.0 + 0.3], [2.0], 12.0, 0.15, 9)
    return W, H, _cat([dense, veil])


SCENES = [every_lane, pair_parity, straddling, ragged_33x17, ragged_15x17, opaque_stacks]


def _reference(oracle_mod, G, make, bg):
    key = (make.__name__, bg)
    if key not in _REF:
        W, H, sc = make()
        cam = _camera(W, H)
        v, of = G.oracle_forward(oracle_mod, cam, sc, bg)
        dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
        _REF[key] = (cam, sc, v, of, dL, oracle_mod.backward(v, of, dL, abs_sums=True),
                     oracle_mod.backward_f64(v, of, dL, cond=False, abs_sums=True))
    return _REF[key]


def _device(G, cam, sc, bg, dL, form, masks):
    hf = G.hip_forward(cam, sc, bg, scratch_floats=16, fwd_form=form, hit_masks=masks)
    g = G.hip_backward(hf, dL, bwd_form=form)
    assert g["bwd_form"] == form and g["bwd_masks"] == masks
    return hf, g


def _exact_forward(G, hf, of):
    st = G.compare_forward(hf, of)
    for k in ("radii_mismatch", "rec_bits_mismatch", "list_mismatch", "n_contrib_mismatch", "final_T_bits_mismatch"):
        assert st[k] == 0, (k, st)


@pytest.mark.parametrize("form, masks", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("make", SCENES, ids=lambda f: f.__name__)
def test_rows_of_a_scene(oracle_mod, make, form, masks):
    import gpu_util as G
    for bg in ((BG, (0.0, 0.0, 0.0)) if make.__name__.startswith("ragged") else (BG,)):
        cam, sc, v, of, dL, og, g64 = _reference(oracle_mod, G, make, bg)
        hf, g = _device(G, cam, sc, bg, dL, form, masks)
        _exact_forward(G, hf, of)
        st = G.walk_row_stats(g, og, g64)
        assert st["slots"] == 9 and st["live"] > 0
        G.assert_walk_rows(st, name="walk_%s_%s_%s%s" % (make.__name__, form, "masks" if masks else "nomasks", "" if any(bg) else "_bg0"))


# ---- the aux form: fifteen sums ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("make", [straddling, ragged_33x17, opaque_stacks], ids=lambda f: f.__name__)
def test_aux_rows(oracle_mod, make, masks):
    """lograst_backward_aux against TWO twins: the scene as it is under dL/dimage, and the scene with the aux triples as its
    colours under dL/daux.  dL/dmean and dL/dopacity are committed as the sums over both images (the twins', and their units',
    added); dL/dconic and the colour gradient are committed per image and held per image."""
    import gpu_util as G
    from log_amd import rasterizer as R
    cam, sc, v, of, dL, og, g64 = _reference(oracle_mod, G, make, BG)
    aux = np.random.default_rng(11).random((len(sc["xyz"]), 3)).astype(np.float32)
    key = ("aux", make.__name__)
    if key not in _REF:
        _, of2 = G.oracle_forward(oracle_mod, cam, dict(sc, colors=aux), BG)
        dA = np.random.default_rng(12).standard_normal(of["image"].shape).astype(np.float32)
        _REF[key] = (of2, dA, oracle_mod.backward(v, of2, dA), oracle_mod.backward_f64(v, of2, dA, cond=False))
    of2, dA, og2, g64b = _REF[key]
    dev = torch.device("cuda:0")
    rs = G.settings(cam, BG, dev)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    m, s, r, o, c = t(sc["xyz"]), t(sc["scaling"]), t(sc["rotation"]), t(sc["opacity"]).reshape(-1), t(sc["colors"])
    prev = R.set_hit_masks(masks)
    try:
        image, radii, pid, pwp, pw, aux_image, saved = R._backend.forward_aux(rs, R.WODILATE, True, m, s, r, o, c, t(aux), scratch_floats=16)
        g3, g2, gc, go, gs, gr, ga = R._backend.backward_aux(rs, R.WODILATE, True, m, s, r, saved, t(dL), t(dA))
    finally:
        R.set_hit_masks(prev)
    torch.cuda.synchronize()
    assert (image.cpu().numpy().view(np.uint32) == of["image"].view(np.uint32)).all()
    assert (aux_image.cpu().numpy().view(np.uint32) == of2["image"].view(np.uint32)).all()
    conic1, conic2 = (x.clone() for x in R._backend.last_aux_conic_grads)
    for x in (conic1, conic2):
        x[pw == 0] = 0                                                          # rows nobody cleared and nobody reads
    n9 = lambda a: a[:, :9]
    both = lambda a, b: {k: np.asarray(a[k], np.float64) + np.asarray(b[k], np.float64) for k in ("means2D", "opacities")}
    shared = np.array([1, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)                   # slots summed over both images
    for name, own, other, own_o, other_o, conic, colour in (("image", g64, g64b, og, og2, conic1, gc), ("aux", g64b, g64, og2, og, conic2, ga)):
        hg = dict(means2D=g2.cpu().numpy(), opacities=go.cpu().numpy().reshape(-1, 1), conic=conic.cpu().numpy(), colors=colour.cpu().numpy())
        ref = dict(both(own, other), conic=own["conic"], colors=own["colors"], walk_unit=n9(own["walk_unit"]) + shared * n9(other["walk_unit"]))
        oo = dict(both(own_o, other_o), conic=own_o["conic"], colors=own_o["colors"])
        st = G.walk_row_stats(hg, oo, ref)
        assert st["live"] > 0
        G.assert_walk_rows(st, name="walk_aux_%s_%s_%s" % (name, make.__name__, "masks" if masks else "nomasks"))

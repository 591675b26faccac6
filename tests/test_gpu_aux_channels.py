"""Aux channels (``GaussianRasterizer.forward(..., aux_colors=)``): a second colour triple per Gaussian composited into a
second image by the SAME walk, and differentiated by the same reverse walk and the same chain-rule launch.

The comparator is always the two-call path on the same inputs: two separate rasterizer calls with geometry reuse off,
first with ``colors``, then with ``aux_colors`` as ``colors_precomp``.

* Forward: bit for bit -- derivable, not measured: the aux sums are accumulated with the same ``w``, in the same list
  order, with the same fma as the RGB sums, and every other output is the untouched walk's.
* Backward: two device evaluations of the same sums that differ only in the order of float additions: within
  ORDER_TOL = 1e-5 relative L2 (the bound of tests/test_gpu_parity.py:126,197); against the CPU oracle's two backwards
  added: within GRAD_TOL = 1e-4 (BASELINE.json).  Both are the bounds of tests/test_gpu_recomposite.py:8-19.

aux_colors are drawn with both signs and magnitudes around 1e3; the background is a non-zero random triple drawn per scene.

dL/dconic is kept per image through the reverse walk and takes the chain rule once per image inside the one launch (the
chain rule is ill-conditioned in fp32 for needle-shaped Gaussians, and two of the `_ragged` scene's 2000 are: differences
of 1e-7 in dL/dconic come out as 1e-5 and more in dL/dscales and dL/drotations, see the cross-form case below), so every
gradient of every case is held to ORDER_TOL against the pair.

One case compares across forms: walk_form="rows" is requested, the aux call runs the quadrant kernels, the pair the
row-split ones.  Those two are not the same sums in another atomic order (other reduction trees, other visit sets), and the
two-call path's own two forms lie 1.1e-5 (scales) and 2.5e-5 (rotations) apart on this scene, measured on pairs without any
aux call.  So that case holds the forward bits against the row-split pair, as everywhere, the gradients to ORDER_TOL against
the pair in the form that ran (quadrant), and to GRAD_TOL -- the bound the package states for form against form: "gradients
within the same tolerance", log_amd/rasterizer.py -- against the row-split pair."""
import contextlib

import numpy as np
import pytest
import torch

import list_cases
from test_gpu_recomposite import _culled_scene, _lazy_scene, _ragged
from util import rel_l2, small_case

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4     # relative L2 against the oracle, stated by BASELINE.json
ORDER_TOL = 1e-5    # two device evaluations of the same sums, order of the additions only


def _bg(cam, sc):
    """A non-zero random background, drawn per scene (seeded by its size and the image's): the aux call, its comparator and
    the oracle of one case get the same triple, different cases different ones."""
    rng = np.random.default_rng([len(sc["xyz"]), cam["image_width"], cam["image_height"]])
    return tuple(float(x) for x in rng.uniform(0.05, 0.95, 3).astype(np.float32))
LEAVES = ("xyz", "scaling", "rotation", "opacity", "colors", "aux")
DEV = "cuda:0"


def _package(name):
    import diff_gaussian_rasterization as up
    import diff_gaussian_rasterization_wodilate as wo
    return wo if name == "wodilate" else up


def _aux_colors(n, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * 1.0e3).astype(np.float32)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Run:
    """mode "aux": one call with aux_colors; "pair": the two-call comparator; "plain": the first call alone.
    which: the images that receive a gradient ("image", "aux")."""

    def __init__(self, cam, sc, mode, package="wodilate", which=("image", "aux"), backward=True, aux=None, form=None,
                 rast_form=None, zero_aux_grad=False):
        import gpu_util as G
        from log_amd import rasterizer as R
        mod = _package(package)
        dev = torch.device(DEV)
        n = len(sc["xyz"])
        sc = dict(sc, aux=_aux_colors(n) if aux is None else aux)
        T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
        self.leaves = {k: T(sc[k]) for k in LEAVES}
        L = self.leaves
        self.m2 = torch.zeros(n, 3, device=dev, requires_grad=True)
        self.bg = _bg(cam, sc)
        rs = G.settings(cam, self.bg, dev)
        rast = mod.GaussianRasterizer(raster_settings=rs, **({"walk_form": rast_form} if rast_form else {}))
        kw = dict(means3D=L["xyz"], means2D=self.m2, shs=None, colors_precomp=L["colors"], opacities=L["opacity"],
                  scales=L["scaling"], rotations=L["rotation"], cov3D_precomp=None)
        rng = np.random.default_rng(7)
        H, W = cam["image_height"], cam["image_width"]
        self.w1 = rng.standard_normal((3, H, W)).astype(np.float32)
        self.w2 = rng.standard_normal((3, H, W)).astype(np.float32) * np.float32(0.0 if zero_aux_grad else 1.0e-3)
        prev = R.set_geometry_reuse(False)
        R.capacity_stats(reset=True)
        try:
            with (R.walk_form(form) if form else contextlib.nullcontext()):
                if mode == "aux":
                    out = rast(aux_colors=L["aux"], **kw)
                    self.out, self.aux_image = out[:-1], out[-1]
                    self.fwd_form = R._backend.last_forms["fwd"]
                else:
                    self.out = rast(**kw)
                    self.aux_image = rast(**dict(kw, colors_precomp=L["aux"]))[0] if mode == "pair" else None
            self.forwards = R.capacity_stats()["forwards"]
            self.saved = self.out[0].grad_fn.saved
            self.final_T, self.n_contrib = self.saved["final_T"].clone(), self.saved["n_contrib"].clone()
            if backward:
                loss = 0
                if "image" in which:
                    loss = loss + (self.out[0] * torch.from_numpy(self.w1).to(dev)).sum()
                if "aux" in which and self.aux_image is not None:
                    loss = loss + (self.aux_image * torch.from_numpy(self.w2).to(dev)).sum()
                loss.backward()
                self.bwd_form = R._backend.last_forms.get("bwd")
        finally:
            R.set_geometry_reuse(prev)
        torch.cuda.synchronize()

    def grads(self):
        g = {k: (t.grad.detach().cpu().numpy() if t.grad is not None else None) for k, t in self.leaves.items()}
        g["means2D"] = self.m2.grad.detach().cpu().numpy() if self.m2.grad is not None else None
        return g


def _same_forward(a, p, extras):
    """The aux call's outputs against the pair's, bit for bit."""
    names = ("image", "radii", "point_id_pixel", "point_weight_pixel", "point_weight") if extras else ("image", "radii")
    assert len(a.out) == len(p.out) == len(names)
    for name, x, y in zip(names, a.out, p.out):
        assert np.array_equal(_bits(x), _bits(y)), name
    assert np.array_equal(_bits(a.aux_image), _bits(p.aux_image)), "aux_image"
    assert np.array_equal(_bits(a.final_T), _bits(p.final_T)), "final_T"
    assert np.array_equal(_bits(a.n_contrib), _bits(p.n_contrib)), "n_contrib"


def _same_grads(a, p, tol=ORDER_TOL, skip=()):
    """Every figure is printed before the first assertion."""
    ga, gp = a.grads(), p.grads()
    figures = {}
    for k in ga:
        if k in skip:
            continue
        if ga[k] is None or gp[k] is None:     # (an input of a call that received no gradient: None there, zeros here)
            assert all(g is None or not np.any(g) for g in (ga[k], gp[k])), k
            continue
        if np.any(gp[k]) or np.any(ga[k]):
            figures[k] = rel_l2(ga[k], gp[k])
            print("grad %-9s aux call vs two calls: rel L2 %.3g" % (k, figures[k]))
    assert all(f < tol for f in figures.values()), {k: f for k, f in figures.items() if not f < tol}


def _check(cam, sc, package="wodilate", which=("image", "aux"), **kw):
    a, p = Run(cam, sc, "aux", package, which, **kw), Run(cam, sc, "pair", package, which, **kw)
    assert a.forwards == 1 and p.forwards == 2, (a.forwards, p.forwards)      # one launch sequence against two
    assert a.fwd_form == "quadrant" and a.bwd_form == "quadrant"
    _same_forward(a, p, package == "wodilate")
    _same_grads(a, p)
    return a, p


# ---- forward bits and pair gradients over shapes, list lengths and regimes ------------------------------------------------

@pytest.mark.parametrize("package", ["wodilate", "upstream"])
@pytest.mark.parametrize("shape", [(16, 16), (37, 21), (64, 48)])
def test_image_shapes_both_packages(shape, package):
    """One tile; partial tiles on both edges; several full tiles."""
    W, H = shape
    cam, sc = small_case(n=400, W=W, H=H, focal=1.1 * W, seed=2, smax=0.1)
    a, _ = _check(cam, sc, package)
    assert len(a.out) == (5 if package == "wodilate" else 2)


@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 129])
def test_tile_lists_on_the_chunk_edges(L):
    """A list of exactly L entries: the 64-entry chunk edge and the odd tail of the two-entries-per-iteration loop."""
    cam, sc, lens = list_cases.one_tile(L, "spread")
    a, _ = _check(cam, sc)
    assert lens[list_cases.MAIN_TILE] == L
    assert int(a.n_contrib[16:32, 16:32].max()) == L          # the main tile's open pixel walked its whole list


def test_opaque_stack_saturates_pixels_mid_chunk():
    """Three opaque splats in front of a list of 200: every pixel stops inside the first chunk, and no aux sum may take
    anything from the 197 entries behind."""
    cam, sc, _ = list_cases.one_tile(200, "spread", front="closed")
    a, _ = _check(cam, sc)
    deepest = int(a.n_contrib[16:32, 16:32].max())
    assert 0 < deepest <= list_cases.N_FRONT, deepest
    assert float(a.final_T[16:32, 16:32].max()) < 1e-2


@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("kind", ["open", "mixed"])
def test_long_lists_park_and_resume(kind, lazy):
    """Lists above LR_LONG_LIST: with the lazy sort the waves park at the end of the first window, with the three aux sums
    in the aux image's planes, and resume in the tails."""
    from log_amd import tune
    cam, sc = _lazy_scene(kind)
    tune.set_knob("LOGRAST_LAZY_SORT", lazy)
    try:
        a, _ = _check(cam, sc)
    finally:
        tune.reset_knobs()
    assert int(a.n_contrib.max()) > 7680


def test_empty_input_and_nothing_hit():
    cam, sc = _ragged()
    empty = {k: v[:0] for k, v in sc.items()}
    for scene in (empty, _culled_scene(cam, sc)):
        a, p = Run(cam, scene, "aux", backward=False), Run(cam, scene, "pair", backward=False)
        _same_forward(a, p, True)
        H, W = cam["image_height"], cam["image_width"]
        want = np.broadcast_to(np.asarray(a.bg, np.float32)[:, None, None], (3, H, W))
        assert np.array_equal(_bits(a.aux_image), want.view(np.uint32))         # fma(1, bg, 0)
    a = Run(cam, _culled_scene(cam, sc), "aux")                                 # and its backward: all zeros
    assert all(not np.any(g) for g in a.grads().values() if g is not None)


@pytest.mark.parametrize("masks", [True, False])
def test_hit_masks_on_and_off(masks):
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    prev = R.set_hit_masks(masks)
    try:
        a, _ = _check(cam, sc)
    finally:
        R.set_hit_masks(prev)
    assert (a.saved["hit_masks"] is not None) == masks
    assert a.saved["hit_mask_form"] == (2 if masks else 0)


def test_touched_only_regime_at_small_size():
    """LOGRAST_HELPER_MIN_N below n: the compositing kernel clears the accumulator rows it meets (all sixteen slots: the
    aux sums' too) and nobody clears the others."""
    from log_amd import tune
    cam, sc = _ragged()
    tune.set_knob("LOGRAST_HELPER_MIN_N", 1000)
    try:
        _check(cam, sc)
    finally:
        tune.reset_knobs()


@pytest.mark.parametrize("how", ["context", "object"])
def test_rows_form_requested_runs_the_quadrant_kernels(how):
    """walk_form="rows" together with aux: the same bits, and the caller can see that the quadrant form ran."""
    cam, sc = _ragged()
    kw = dict(form="rows") if how == "context" else dict(rast_form="rows")
    a, p = Run(cam, sc, "aux", **kw), Run(cam, sc, "pair", **kw)
    assert p.bwd_form == "rows" and a.fwd_form == "quadrant" and a.bwd_form == "quadrant"
    assert a.saved["hit_mask_form"] == 2
    _same_forward(a, p, True)
    q = Run(cam, sc, "pair", form="quadrant")     # the pair in the form the aux call ran: the same sums in another order
    assert q.bwd_form == "quadrant"
    _same_forward(a, q, True)
    _same_grads(a, q)
    _same_grads(a, p, tol=GRAD_TOL)               # form against form (module docstring)


# ---- backward ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged_oracle(oracle_mod):
    """The oracle's forward and backward of both calls of the ragged scene, computed once."""
    import gpu_util as G
    cam, sc = _ragged()
    aux = _aux_colors(len(sc["xyz"]))
    ref = Run(cam, sc, "pair", backward=False)
    v, of1 = G.oracle_forward(oracle_mod, cam, sc, _bg(cam, sc))
    _, of2 = G.oracle_forward(oracle_mod, cam, dict(sc, colors=aux), _bg(cam, sc))
    og1, og2 = oracle_mod.backward(v, of1, ref.w1), oracle_mod.backward(v, of2, ref.w2)
    return cam, sc, of1, of2, og1, og2


@pytest.mark.parametrize("which", [("image",), ("aux",), ("image", "aux")])
def test_gradients_against_the_pair_and_the_oracle(ragged_oracle, which):
    cam, sc, of1, of2, og1, og2 = ragged_oracle
    a, _ = _check(cam, sc, which=which)
    assert np.array_equal(_bits(a.out[0]), of1["image"].view(np.uint32))
    assert np.array_equal(_bits(a.aux_image), of2["image"].view(np.uint32))
    z = lambda g: {k: np.zeros_like(np.asarray(v)) for k, v in g.items()}
    g1, g2 = (og1 if "image" in which else z(og1)), (og2 if "aux" in which else z(og2))
    add = lambda k: np.asarray(g1[k]) + np.asarray(g2[k])
    want = dict(xyz=add("means3D"), scaling=add("scales"), rotation=add("rotations"), opacity=add("opacities").reshape(-1, 1),
                colors=np.asarray(g1["colors"]), aux=np.asarray(g2["colors"]), means2D=add("means2D")[:, :2])
    got = a.grads()
    got = dict(got, means2D=got["means2D"][:, :2], opacity=got["opacity"].reshape(-1, 1))
    figures = {}
    for k, ref in want.items():
        if not np.any(ref):
            assert got[k] is None or not np.any(got[k]), k
            continue
        figures[k] = rel_l2(got[k], ref)
        print("grad %-9s aux call vs oracle: rel L2 %.3g" % (k, figures[k]))
    assert all(f < GRAD_TOL for f in figures.values()), {k: f for k, f in figures.items() if not f < GRAD_TOL}


def test_zero_aux_gradient_leaves_the_plain_gradients():
    cam, sc = _ragged()
    a, b = Run(cam, sc, "aux", zero_aux_grad=True), Run(cam, sc, "plain", which=("image",))
    _same_grads(a, b, skip=("aux",))
    assert not np.any(a.grads()["aux"])


def test_native_sh_colours_with_aux():
    """shs= works with aux_colors: its colours are computed in front of the walk."""
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    cam, sc = small_case(n=300, W=37, H=21, focal=40.0, seed=4, smax=0.1)
    dev = torch.device(DEV)
    T = lambda a, g=True: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=g)
    rng = np.random.default_rng(5)
    res = []
    for mode in ("aux", "pair"):
        m3, sca, rot, op = (T(sc[k]) for k in ("xyz", "scaling", "rotation", "opacity"))
        shs, aux = T(rng.standard_normal((300, 1, 3)) if mode == "aux" else res[0][2]), T(_aux_colors(300))
        rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, _bg(cam, sc), dev))
        kw = dict(means3D=m3, means2D=torch.zeros_like(m3, requires_grad=True), opacities=op, scales=sca, rotations=rot)
        if mode == "aux":
            out = rast(shs=shs, aux_colors=aux, **kw)
            img, aimg = out[0], out[-1]
        else:
            img, aimg = rast(shs=shs, **kw)[0], rast(colors_precomp=aux, **kw)[0]
        (img.sum() + 1e-3 * aimg.sum()).backward()
        res.append((img.detach().cpu().numpy(), aimg.detach().cpu().numpy(), shs.detach().cpu().numpy(),
                    shs.grad.cpu().numpy(), aux.grad.cpu().numpy(), m3.grad.cpu().numpy()))
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1]))
    for i in (3, 4, 5):
        assert rel_l2(res[0][i], res[1][i]) < ORDER_TOL, (i, rel_l2(res[0][i], res[1][i]))


# ---- capacity modes, graph capture, rejected combinations ----------------------------------------------------------------

@pytest.mark.parametrize("mode", ["speculative", "exact", "fixed"])
def test_capacity_modes(mode):
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    ref = Run(cam, sc, "pair")
    n_inst, _, max_len, _ = R.last_state_info(torch.device(DEV))
    prev = R.set_speculative(mode == "speculative")
    if mode == "fixed":
        R.set_instance_capacity(n_inst + 64, max_tile_len=max_len + 64)
    try:
        a = Run(cam, sc, "aux")
    finally:
        R.set_instance_capacity(None)
        R.set_speculative(prev)
    _same_forward(a, ref, True)
    _same_grads(a, ref)


def test_captured_forward_and_backward_replay_identically():
    """Sync-free mode with a fixed capacity: the aux forward and its backward captured into a HIP graph replay, twice, to
    the bits of the eager forward and gradients within the order bound."""
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    dev = torch.device(DEV)
    eager = Run(cam, sc, "aux")
    ge = eager.grads()
    n_inst, _, max_len, _ = R.last_state_info(dev)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
    sc = dict(sc, aux=_aux_colors(len(sc["xyz"])))
    leaves = {k: T(sc[k]) for k in LEAVES}
    m2 = torch.zeros(len(sc["xyz"]), 3, device=dev, requires_grad=True)
    rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, _bg(cam, sc), dev))
    w1, w2 = torch.from_numpy(eager.w1).to(dev), torch.from_numpy(eager.w2).to(dev)
    order = [leaves[k] for k in LEAVES] + [m2]

    def step():
        out = rast(means3D=leaves["xyz"], means2D=m2, shs=None, colors_precomp=leaves["colors"], opacities=leaves["opacity"],
                   scales=leaves["scaling"], rotations=leaves["rotation"], cov3D_precomp=None, aux_colors=leaves["aux"])
        loss = (out[0] * w1).sum() + (out[-1] * w2).sum()
        return out, torch.autograd.grad(loss, order)

    R.set_instance_capacity(n_inst + 64, max_tile_len=max_len + 64)
    try:
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            step()                                   # warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            out, grads = step()
        for _ in range(2):
            for t in tuple(out) + tuple(grads):
                t.detach().zero_()
            g.replay()
            torch.cuda.synchronize()
            for x, y in zip(out[:-1], eager.out):
                assert np.array_equal(_bits(x), _bits(y))
            assert np.array_equal(_bits(out[-1]), _bits(eager.aux_image))
            for k, t in zip(LEAVES + ("means2D",), grads):
                assert rel_l2(t.detach().cpu().numpy(), ge[k]) < ORDER_TOL, k
        assert not R.overflow_since_reset(dev)["overflowed"]
    finally:
        R.set_instance_capacity(None)


def test_rejected_combinations_raise():
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    from log_amd.dist import GradientBucket
    cam, sc = small_case(n=64, W=32, H=32, focal=40.0, seed=1)
    dev = torch.device(DEV)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    m3, sca, rot, op, col = (T(sc[k]) for k in ("xyz", "scaling", "rotation", "opacity", "colors"))
    aux = T(_aux_colors(64))
    rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, _bg(cam, sc), dev))
    kw = dict(means3D=m3, means2D=torch.zeros_like(m3), shs=None, colors_precomp=col, opacities=op, aux_colors=aux)
    with pytest.raises(ValueError, match="cov3D_precomp"):
        rast(cov3D_precomp=torch.zeros(64, 6, device=dev), **kw)
    with R.tile_rows(0, 1):
        with pytest.raises(ValueError, match="tile_rows"):
            rast(scales=sca, rotations=rot, **kw)
    bucket = GradientBucket(64, dev, 1, row_major=True)
    with R.accumulate_grads_into(bucket.sink()):
        with pytest.raises(ValueError, match="accumulate_grads_into"):
            rast(scales=sca, rotations=rot, **kw)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        rast(scales=sca, rotations=rot, **dict(kw, aux_colors=aux[:10]))


def test_in_place_change_of_aux_colors_before_backward_is_refused():
    """The reverse walk composites aux_colors again: a caller that overwrites them in between gets an error, not gradients
    of other colours."""
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    cam, sc = small_case(n=64, W=32, H=32, focal=40.0, seed=1)
    dev = torch.device(DEV)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    m3, sca, rot, op = (T(sc[k]) for k in ("xyz", "scaling", "rotation", "opacity"))
    col, aux = T(sc["colors"]).requires_grad_(True), T(_aux_colors(64))
    rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, _bg(cam, sc), dev))
    out = rast(means3D=m3, means2D=torch.zeros_like(m3), shs=None, colors_precomp=col, opacities=op, scales=sca, rotations=rot,
               cov3D_precomp=None, aux_colors=aux)
    aux.mul_(2.0)
    with pytest.raises(RuntimeError, match="aux_colors input was modified in place"):
        (out[0].sum() + out[-1].sum()).backward()


def test_aux_forward_is_not_remembered_by_geometry_reuse():
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    dev = torch.device(DEV)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    m3, sca, rot, op, col = (T(sc[k]) for k in ("xyz", "scaling", "rotation", "opacity", "colors"))
    aux = T(_aux_colors(len(sc["xyz"])))
    rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, _bg(cam, sc), dev))
    kw = dict(means3D=m3, means2D=torch.zeros_like(m3), shs=None, opacities=op, scales=sca, rotations=rot)
    prev = R.set_geometry_reuse(True)
    R.geometry_reuse_stats(reset=True)
    try:
        with torch.no_grad():
            one = rast(colors_precomp=col, aux_colors=aux, **kw)
            two = rast(colors_precomp=aux, **kw)                # a full forward: nothing was remembered
        assert R.geometry_reuse_stats() == dict(reused=0, fallback={"aux": 1, "first": 1})
    finally:
        R.set_geometry_reuse(prev)
    assert np.array_equal(_bits(one[-1]), _bits(two[0]))


# ---- the LoG drop-in's proxy, driven by a stand-in render -----------------------------------------------------------------

class _StandInRenderer:
    """The two rasterizer calls of LoG/render/renderer.py:153,190 and the depth outputs of :191-201, nothing else."""
    render_depth = True
    use_origin_render = False

    def render(self, rasterizer, camera, means3D, means2D, colors, opacity, scales, rotations):
        out = {}
        image, radii, pid, pwp, pw = rasterizer(means3D=means3D, means2D=means2D, shs=None, colors_precomp=colors,
                                                opacities=opacity, scales=scales, rotations=rotations, cov3D_precomp=None)
        out["render"], out["radii"], out["point_weight"] = image, radii, pw
        if self.render_depth:
            xyz1 = torch.cat([means3D.detach(), torch.ones_like(means3D[:, :1])], dim=1)
            point_depth = (xyz1 @ camera["world_view_transform"])[:, 2]
            colors_depth = torch.stack([point_depth, means3D[:, 2], torch.ones_like(point_depth)], dim=-1)
            ret = rasterizer(means3D=means3D, means2D=means2D, shs=None, colors_precomp=colors_depth, opacities=opacity,
                             scales=scales, rotations=rotations, cov3D_precomp=None)
            out["depth"], out["height"], out["accmap"] = ret[0][0:1], ret[0][1:2], ret[0][2:3]
        return out


def test_depth_pass_proxy_with_a_stand_in_render():
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import depth_pass, rasterizer as R
    cam, sc = _ragged()
    dev = torch.device(DEV)
    camera = {"world_view_transform": torch.tensor(np.asarray(cam["world_view_transform"], np.float32), device=dev)}
    rs = G.settings(cam, _bg(cam, sc), dev)
    H, W = cam["image_height"], cam["image_width"]
    rng = np.random.default_rng(9)
    wr, wd = (torch.from_numpy(rng.standard_normal((3, H, W)).astype(np.float32)).to(dev) for _ in range(2))
    results = {}
    for name in ("plain", "wrapped"):
        T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
        leaves = {k: T(sc[k]) for k in ("xyz", "scaling", "rotation", "opacity", "colors")}
        m2 = torch.zeros(len(sc["xyz"]), 3, device=dev, requires_grad=True)
        renderer = _StandInRenderer()
        render = _StandInRenderer.render if name == "plain" else depth_pass.wrap_render(_StandInRenderer.render)
        depth_pass.reset_stats()
        depth_pass.set_verify(True)
        R.capacity_stats(reset=True)
        try:
            out = render(renderer, wo.GaussianRasterizer(raster_settings=rs), camera, leaves["xyz"], m2, leaves["colors"],
                         leaves["opacity"], leaves["scaling"], leaves["rotation"])
        finally:
            depth_pass.set_verify(False)
        forwards = R.capacity_stats()["forwards"]
        loss = (out["render"] * wr).sum() + 1e-2 * (torch.cat([out["depth"], out["height"], out["accmap"]]) * wd).sum()
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: t.grad.cpu().numpy() for k, t in leaves.items()}
        grads["means2D"] = m2.grad.cpu().numpy()
        results[name] = (out, forwards, grads, depth_pass.stats())
    (po, pf, pg, _), (wo_, wf, wg, st) = results["plain"], results["wrapped"]
    assert pf == 2 and wf == 1, (pf, wf)                      # exactly one forward launch sequence
    assert st["fused"] == 1 and st["fallback"] == {}, st
    for k in ("render", "depth", "height", "accmap", "radii", "point_weight"):
        assert np.array_equal(_bits(wo_[k]), _bits(po[k])), k
    figures = {k: rel_l2(wg[k], pg[k]) for k in pg}
    for k, f in figures.items():
        print("grad %-9s proxy vs two calls: rel L2 %.3g" % (k, f))
    assert all(f < ORDER_TOL for f in figures.values()), {k: f for k, f in figures.items() if not f < ORDER_TOL}

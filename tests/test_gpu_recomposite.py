"""Geometry reuse (log_amd.rasterizer.set_geometry_reuse): the second call of a view through the same rasterizer object --
LoG's depth pass, LoG/render/renderer.py:186-201 -- recolours the first call's records and composites its tile lists again
(lograst_recomposite) instead of projecting, binning, filling and sorting again.

Every case runs three passes on the same seeded inputs: (a) two calls with reuse off, (b) two calls with reuse on through
a fresh rasterizer object, the same kind of leaves and a fresh means2D, (c) the CPU oracle's forward with the second
call's colours ([view-space z, world z, 1], as renderer.py:167-189 builds them).  Forward outputs are compared bit for
bit; gradients of two device evaluations of the same sums that differ only in atomic order within 1e-5 relative L2 (the
bound of tests/test_gpu_parity.py:126,197), against the oracle within GRAD_TOL = 1e-4 (BASELINE.json)."""
import numpy as np
import pytest
import torch

from util import rel_l2, small_case

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4     # relative L2 against the oracle, stated by BASELINE.json
ORDER_TOL = 1e-5    # two device evaluations of the same sums, atomic order only
BG = (0.3, 0.6, 0.9)
LEAVES = ("xyz", "scaling", "rotation", "opacity", "colors")


def _package(name):
    import diff_gaussian_rasterization as up
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    return (wo, R.WODILATE) if name == "wodilate" else (up, R.UPSTREAM)


def _ragged():
    return small_case(n=2000, W=150, H=97, focal=170.0, seed=3, smax=0.08)


def _dense_tile():
    cam, sc = small_case(n=12000, W=64, H=64, focal=70.0, seed=6, smax=0.01)
    sc["xyz"] *= 0.05
    return cam, sc


def _lazy_scene(kind):
    """The scenes of tests/test_gpu_parity.py::test_lazily_ordered_lists_both_ways."""
    rng = np.random.default_rng(31)
    n = 11000
    cam, sc = small_case(n=n, W=64, H=48, focal=70.0, seed=30, opacity=(0.999 if kind == "closed" else 0.05),
                         smax=(0.6 if kind == "closed" else 0.004))
    if kind == "closed":
        sc["scaling"] = (0.3 + 0.3 * rng.random((n, 3))).astype(np.float32)
    else:
        sc["xyz"] = (sc["xyz"] * 0.06).astype(np.float32)
    if kind == "mixed":
        k = 60
        sc["xyz"][:k] = (0.02 * rng.standard_normal((k, 3)) + np.array([0.03, 0.0, 0.0])).astype(np.float32)
        sc["scaling"][:k] = 0.05
        sc["opacity"][:k] = 0.999
    return cam, sc


def _point_depth(cam, sc):
    """View-space z of every Gaussian (renderer.py:167-169), computed once on the host so that every pass and the oracle
    get the same bits."""
    xyz1 = np.concatenate([sc["xyz"], np.ones((len(sc["xyz"]), 1), np.float32)], axis=1).astype(np.float32)
    return np.ascontiguousarray((xyz1 @ np.asarray(cam["world_view_transform"], np.float32))[:, 2], np.float32)


def _depth_scene(cam, sc):
    """The scene of the second call: colours [view depth, world z, 1]."""
    col = np.stack([_point_depth(cam, sc), sc["xyz"][:, 2], np.ones(len(sc["xyz"]), np.float32)], axis=-1)
    return dict(sc, colors=np.ascontiguousarray(col, np.float32))


class Pair:
    """Two calls through the public package, the way LoG makes them, and one backward over both."""

    def __init__(self, cam, sc, reuse, package="wodilate", between=None, other_object=False, second_kw=None,
                 second_ctx=None, cov3D=False, grad=(True, True), backward=True, sink_rows=False, dev="cuda:0", order=None):
        """order: None = one backward over the sum of both calls' losses; (1, 2) / (2, 1) = one backward per call, in that
        order (the leaves' .grad hold the same sums either way)."""
        import contextlib
        import gpu_util as G
        from log_amd import rasterizer as R
        mod, flavour = _package(package)
        self.flavour = flavour
        dev = torch.device(dev)
        n = len(sc["xyz"])
        T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
        self.leaves = {k: T(sc[k]) for k in LEAVES}
        L = self.leaves
        self.m2 = torch.zeros(n, 3, device=dev, requires_grad=True)
        rs = G.settings(cam, BG, dev)
        rast = mod.GaussianRasterizer(raster_settings=rs)
        kw = dict(means3D=L["xyz"], means2D=self.m2, shs=None, colors_precomp=L["colors"], opacities=L["opacity"],
                  scales=L["scaling"], rotations=L["rotation"], cov3D_precomp=None)
        if cov3D:
            from oracle import torch_oracle
            Rm = torch_oracle._rot(torch.tensor(sc["rotation"], dtype=torch.float64))
            M = Rm * torch.tensor(sc["scaling"], dtype=torch.float64)[:, None, :]
            S = (M @ M.transpose(1, 2)).numpy()
            self.cov = T(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1))
            kw.update(scales=None, rotations=None, cov3D_precomp=self.cov)
        rng = np.random.default_rng(7)
        H, W = cam["image_height"], cam["image_width"]
        self.w1 = rng.standard_normal((3, H, W)).astype(np.float32)
        self.w2 = rng.standard_normal((3, H, W)).astype(np.float32)
        bucket = None
        if sink_rows:
            from log_amd.dist import GradientBucket
            bucket = GradientBucket(n, dev, 1, row_major=True)
            bucket.zero()
        prev = R.set_geometry_reuse(reuse)
        R.geometry_reuse_stats(reset=True)
        try:
            with (R.accumulate_grads_into(bucket.sink()) if bucket is not None else contextlib.nullcontext()):
                with (contextlib.nullcontext() if grad[0] else torch.no_grad()):
                    self.out1 = rast(**kw)
                if between is not None:
                    between(self)
                pd = torch.tensor(_point_depth(cam, sc), device=dev)
                self.cd = torch.stack([pd, L["xyz"][:, 2], torch.ones_like(pd)], dim=-1)      # renderer.py:187-189
                if self.cd.requires_grad:
                    self.cd.retain_grad()
                kw2 = dict(kw, colors_precomp=self.cd, **(second_kw or {}))
                rast2 = mod.GaussianRasterizer(raster_settings=rs) if other_object else rast
                with (second_ctx() if second_ctx is not None else contextlib.nullcontext()):
                    with (contextlib.nullcontext() if grad[1] else torch.no_grad()):
                        self.out2 = rast2(**kw2)
                self.stats = R.geometry_reuse_stats()
                if backward:
                    losses = {}
                    if grad[0]:
                        losses[1] = (self.out1[0] * torch.from_numpy(self.w1).to(dev)).sum()
                    if grad[1]:
                        losses[2] = (self.out2[0] * torch.from_numpy(self.w2).to(dev)).sum()
                    if order is None:
                        sum(losses.values()).backward()
                    else:
                        for i in order:
                            losses[i].backward()
        finally:
            R.set_geometry_reuse(prev)
        torch.cuda.synchronize()
        self.rows = bucket.views["rows"].detach().cpu().numpy() if bucket is not None else None

    def grads(self):
        g = {k: (t.grad.detach().cpu().numpy() if t.grad is not None else None) for k, t in self.leaves.items()}
        g["means2D"] = self.m2.grad.detach().cpu().numpy() if self.m2.grad is not None else None
        g["depth_colors"] = self.cd.grad.detach().cpu().numpy() if self.cd.grad is not None else None
        return g


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_outputs(x, y, extras):
    """Outputs of one rasterizer call against another's: float maps bit for bit, integer maps equal."""
    names = ("image", "radii", "point_id_pixel", "point_weight_pixel", "point_weight") if extras else ("image", "radii")
    assert len(x) == len(y) == len(names)
    for name, p, q in zip(names, x, y):
        assert np.array_equal(_bits(p), _bits(q)), name


def _reused(stats):
    return stats["reused"], sum(stats["fallback"].values())


def _check_pair(oracle_mod, cam, sc, a, b, oracle_grads=True):
    """The assertions every reuse case shares."""
    import gpu_util as G
    extras = bool(a.flavour.extras)
    assert a.stats == dict(reused=0, fallback={}), a.stats                       # reuse off: nothing counted, nothing reused
    assert b.stats["reused"] == 1 and b.stats["fallback"] == {"first": 1}, b.stats
    _same_outputs(b.out1, a.out1, extras)                                        # the first call is untouched
    _same_outputs(b.out2, a.out2, extras)
    assert b.out2[1].data_ptr() != b.out1[1].data_ptr()                          # radii: a tensor of the second call's own
    b.out2[1].add_(1)
    assert np.array_equal(_bits(b.out1[1]), _bits(a.out1[1]))
    b.out2[1].sub_(1)
    s1, s2 = b.out1[0].grad_fn.saved, b.out2[0].grad_fn.saved                    # a forward's record and a recomposite's
    assert set(s1) == set(s2) and s2["state"] is s1["state"] and s2["plist"] is s1["plist"]
    assert s1["bwd_scratch"] is None and s2["bwd_scratch"] is None               # each backward took its own accumulator rows
    sc2 = _depth_scene(cam, sc)
    v, of2 = G.oracle_forward(oracle_mod, cam, sc2, BG, flavour=a.flavour)
    assert np.array_equal(_bits(b.out2[0]), of2["image"].view(np.uint32))
    ga, gb = a.grads(), b.grads()
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        if ga[k] is not None:
            assert rel_l2(gb[k], ga[k]) < ORDER_TOL, (k, rel_l2(gb[k], ga[k]))
    if oracle_grads:
        _, of1 = G.oracle_forward(oracle_mod, cam, sc, BG, flavour=a.flavour)
        og1, og2 = oracle_mod.backward(v, of1, a.w1), oracle_mod.backward(v, of2, a.w2)
        want = dict(colors=og1["colors"], depth_colors=og2["colors"],
                    opacity=np.asarray(og1["opacities"]).reshape(-1, 1) + np.asarray(og2["opacities"]).reshape(-1, 1),
                    means2D=np.asarray(og1["means2D"])[:, :2] + np.asarray(og2["means2D"])[:, :2])
        got = dict(gb, means2D=gb["means2D"][:, :2], opacity=gb["opacity"].reshape(-1, 1))
        for k, ref in want.items():
            assert rel_l2(got[k], ref) < GRAD_TOL, (k, rel_l2(got[k], ref))
    return of2


@pytest.mark.parametrize("package", ["wodilate", "upstream"])
def test_second_call_recomposites_ragged(oracle_mod, package):
    """Case 1: odd image size, mixed opacities, several tiles and blocks; both packages (the upstream one returns
    2-tuples and has no fork outputs)."""
    cam, sc = _ragged()
    a, b = Pair(cam, sc, False, package), Pair(cam, sc, True, package)
    assert len(b.out2) == (5 if package == "wodilate" else 2)
    _check_pair(oracle_mod, cam, sc, a, b)


@pytest.mark.parametrize("kind", ["closed", "open", "mixed"])
@pytest.mark.parametrize("form", ["quadrant", "rows"])
def test_lazily_ordered_lists_are_walked_again_without_a_sort(oracle_mod, kind, form):
    """Case 2: lists of more than 4096 keys.  `open` / `mixed`: waves park at the end of the first window and resume in
    the tails -- which the second call cannot order again (the keys are gone): it must find them ordered by the first
    forward and park and resume at the same places.  `closed`: the tails stay unordered and must never be read."""
    from log_amd import rasterizer as R
    cam, sc = _lazy_scene(kind)
    with R.walk_form(form):
        a, b = Pair(cam, sc, False), Pair(cam, sc, True)
    of2 = _check_pair(oracle_mod, cam, sc, a, b)
    deepest = int(of2["n_contrib"].astype(np.int64).max())
    if kind == "closed":
        assert deepest <= 7680, deepest
    else:
        assert deepest > 7680, deepest             # parked waves really resumed, with no sort in between


def test_dense_tile_lists(oracle_mod):
    """Case 3: lists in the LDS sort classes and long lists that are never streamed lazily."""
    cam, sc = _dense_tile()
    a, b = Pair(cam, sc, False), Pair(cam, sc, True)
    _check_pair(oracle_mod, cam, sc, a, b)


@pytest.mark.parametrize("order", [(1, 2), (2, 1)])
@pytest.mark.parametrize("package", ["wodilate", "upstream"])
def test_backward_on_either_record_in_either_order(oracle_mod, package, order):
    """The forward's record and the recomposite's hold the same keys (_check_pair), and the unchanged backward runs on
    either one first: 64 Gaussians on 2 x 2 tiles, one backward per call."""
    cam, sc = small_case(n=64, W=32, H=32, focal=40.0, seed=1)
    a, b = Pair(cam, sc, False, package, order=order), Pair(cam, sc, True, package, order=order)
    _check_pair(oracle_mod, cam, sc, a, b)


def test_touched_only_regime_at_small_size(oracle_mod):
    """Case 4: with LOGRAST_HELPER_MIN_N below n the 5-tuple package is in the touched-only regime: the compositing kernel
    clears the accumulator rows it meets and nobody clears the others -- the recolour kernel's zero-fill must not be what
    the gradients rest on."""
    from log_amd import tune
    cam, sc = _ragged()
    tune.set_knob("LOGRAST_HELPER_MIN_N", 1000)
    try:
        a, b = Pair(cam, sc, False), Pair(cam, sc, True)
    finally:
        tune.reset_knobs()
    _check_pair(oracle_mod, cam, sc, a, b)


@pytest.mark.parametrize("masks", [True, False])
def test_hit_masks_on_and_off(oracle_mod, masks):
    """Case 5: the second call's backward reads masks that its own forward wrote into a buffer of its own (on), or runs
    the support tests again (off)."""
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    prev = R.set_hit_masks(masks)
    try:
        a, b = Pair(cam, sc, False), Pair(cam, sc, True)
    finally:
        R.set_hit_masks(prev)
    _check_pair(oracle_mod, cam, sc, a, b)


def _bump_scales(p):
    """An in-place write that autograd sees.  (A write through ``.data`` -- ``scales.data.mul_(1.0)`` -- does NOT move the
    tensor's version counter: no check built on ``_version`` can see it, here or in autograd's own saved-tensor checks.
    log_amd.rasterizer.set_geometry_reuse says so.)"""
    with torch.no_grad():
        p.leaves["scaling"].mul_(1.0)


def _band():
    from log_amd import rasterizer as R
    return R.tile_rows(1, 3)


def _culled_scene(cam, sc):
    sc = dict(sc)
    sc["xyz"] = np.tile(np.asarray(cam["camera_center"], np.float32), (len(sc["xyz"]), 1))   # depth 0: behind the near plane
    return sc


FALLBACKS = {
    "version_bump": (dict(between=_bump_scales), "geometry"),
    "other_object": (dict(other_object=True), "first"),
    "use_filter": (dict(second_kw=dict(use_filter=False)), "use_filter"),
    "cov3D": (dict(cov3D=True), "cov3D"),
    "empty": (dict(), "empty"),
    "all_culled": (dict(), "no_instances"),
    "band": (dict(second_ctx=_band), "band"),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_run_the_full_forward(name):
    """Case 6: whenever one condition of the match does not hold the second call is a full forward: said so by
    geometry_reuse_stats(), and its outputs are the bits of the same call with reuse off."""
    kw, reason = FALLBACKS[name]
    cam, sc = _ragged()
    if name == "empty":
        sc = {k: v[:0] for k, v in sc.items()}
    if name == "all_culled":
        sc = _culled_scene(cam, sc)
    # (version_bump: autograd itself refuses the first call's backward after an in-place write it has seen)
    backward = name not in ("empty", "all_culled", "version_bump")
    a, b = Pair(cam, sc, False, backward=backward, **kw), Pair(cam, sc, True, backward=backward, **kw)
    assert a.stats == dict(reused=0, fallback={})
    assert b.stats["reused"] == 0, b.stats
    first = "empty" if name == "empty" else ("cov3D" if name == "cov3D" else "first")
    want = {first: 1}
    want[reason] = want.get(reason, 0) + 1
    assert b.stats["fallback"] == want, b.stats
    if name == "all_culled":
        assert int(b.out1[1].max()) == 0
    _same_outputs(b.out1, a.out1, True)
    _same_outputs(b.out2, a.out2, True)
    if backward:
        ga, gb = a.grads(), b.grads()
        for k in ga:
            if ga[k] is not None:
                assert rel_l2(gb[k], ga[k]) < ORDER_TOL, k


@pytest.mark.parametrize("grad", [(False, True), (True, False)])
def test_one_call_without_gradients(oracle_mod, grad):
    """Case 7: the first call under torch.no_grad() and the second with gradients, and the reverse.  The implementation
    REUSES in both: a forward under no_grad keeps its records and lists alive through the rasterizer object all the same,
    and a recomposite under no_grad just prepares no accumulator rows and no hit masks."""
    import gpu_util as G
    cam, sc = _ragged()
    a, b = Pair(cam, sc, False, grad=grad), Pair(cam, sc, True, grad=grad)
    assert b.stats["reused"] == 1 and b.stats["fallback"] == {"first": 1}, b.stats
    _same_outputs(b.out1, a.out1, True)
    _same_outputs(b.out2, a.out2, True)
    ga, gb = a.grads(), b.grads()
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        if ga[k] is not None:
            assert rel_l2(gb[k], ga[k]) < ORDER_TOL, k
    sc_used = sc if grad[0] else _depth_scene(cam, sc)          # the one call that was differentiated, against the oracle
    v, of = G.oracle_forward(oracle_mod, cam, sc_used, BG)
    og = oracle_mod.backward(v, of, a.w1 if grad[0] else a.w2)
    assert rel_l2(gb["colors" if grad[0] else "depth_colors"], og["colors"]) < GRAD_TOL
    assert rel_l2(gb["opacity"].reshape(-1), np.asarray(og["opacities"]).reshape(-1)) < GRAD_TOL
    assert rel_l2(gb["means2D"][:, :2], np.asarray(og["means2D"])[:, :2]) < GRAD_TOL


def test_captured_pair_replays_identically():
    """Case 8: sync-free mode with a capacity just above what the view needs; the pair of forwards captured into a
    torch.cuda.graph replays, twice, to the bits of the eager pair."""
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    dev = torch.device("cuda:0")
    eager = Pair(cam, sc, True, backward=False)
    n_inst, _, max_len, _ = R.last_state_info(dev)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    m3, sca, rot, op, col = (T(sc[k]) for k in LEAVES)
    cd = T(_depth_scene(cam, sc)["colors"])
    m2 = torch.zeros_like(m3)
    rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, BG, dev))
    kw = dict(means3D=m3, means2D=m2, shs=None, opacities=op, scales=sca, rotations=rot, cov3D_precomp=None)

    def pair():
        with torch.no_grad():
            return rast(colors_precomp=col, **kw), rast(colors_precomp=cd, **kw)

    prev = R.set_geometry_reuse(True)
    R.set_instance_capacity(n_inst + 64, max_tile_len=max_len + 64)
    try:
        R.overflow_since_reset(dev)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            pair()                                   # warm-up on the capture stream
        torch.cuda.synchronize()
        R.geometry_reuse_stats(reset=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            o1, o2 = pair()
        # (the first captured call does not reuse the warm-up's forward: a graph must own what it reads)
        assert R.geometry_reuse_stats() == dict(reused=1, fallback={"graph_capture": 1})
        for _ in range(2):
            for t in o1 + o2:
                t.zero_()
            g.replay()
            torch.cuda.synchronize()
            _same_outputs(o1, eager.out1, True)
            _same_outputs(o2, eager.out2, True)
        chk = R.overflow_since_reset(dev)
        assert not chk["overflowed"] and chk["forwards"] >= 6, chk     # a recomposite records itself as a forward
    finally:
        R.set_instance_capacity(None)
        R.set_geometry_reuse(prev)


def test_row_major_bucket_over_the_pair():
    """Case 9: accumulate_grads_into with a row-major bucket: both calls of the pair add into the same rows."""
    cam, sc = _ragged()
    a, b = Pair(cam, sc, False, sink_rows=True), Pair(cam, sc, True, sink_rows=True)
    assert b.stats["reused"] == 1
    assert float(np.abs(a.rows).sum()) > 0
    assert rel_l2(b.rows, a.rows) < ORDER_TOL, rel_l2(b.rows, a.rows)
    assert rel_l2(b.grads()["means2D"], a.grads()["means2D"]) < ORDER_TOL

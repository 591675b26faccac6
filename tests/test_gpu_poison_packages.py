"""Calls through the drop-in packages (autograd, the capacity modes, the gradient sinks, the extensions) rerun with every buffer
the Python layer hands the library filled first (tests/poison.py): once unpoisoned, once under each of the four fills.

Forward outputs are bit-identical across the five runs and are the oracle's bits; the gradients (sums of float atomics) are
finite, exactly 0.0 on the rows the oracle leaves at zero, and within the suite's "same sums, other order" bounds of the
unpoisoned run: ORDER_TOL for the reverse walk's outputs, CHAIN_TOL behind the chain rule.  The exemptions are those of
tests/test_gpu_poison_rasterizer.py (EXEMPT); none applies to what is compared here."""
import contextlib

import numpy as np
import pytest
import torch

import poison as P
from test_gpu_poison_rasterizer import CHAIN_TOL, ORDER_TOL
from util import cam_tan, rel_l2, small_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BG = (0.2, 0.5, 0.1)
N, W, H = 2000, 150, 97
WALK = ("means2D", "opacities", "colors", "aux_colors", "absgrad")
CHAIN = ("means3D", "scales", "rotations", "cov3D", "shs", "viewmatrix", "projmatrix")
PER_ROW = ("means2D", "opacities", "colors", "aux_colors", "absgrad", "means3D", "scales", "rotations", "cov3D", "shs")


def _scene(view=1):
    """The `ragged` scene of tests/test_gpu_parity.py (image no multiple of the tile, mixed opacities), seen from `view`."""
    return small_case(n=N, W=W, H=H, focal=170.0, seed=3, smax=0.08, view=view)


_refs = {}


def _reference(oracle_mod, package, view=1, colors=None, cov=None, key=None):
    """-> (oracle forward, dL/dimage, dead rows: the Gaussians every oracle gradient leaves at zero).  Once per key."""
    from log_amd import rasterizer as R
    key = (package, view, key)
    if key not in _refs:
        cam, sc = _scene(view)
        fl = R.WODILATE if package == "wodilate" else R.UPSTREAM
        tfx, tfy = cam_tan(cam)
        v = oracle_mod.make_view(W, H, tfx, tfy, cam["world_view_transform"], cam["full_proj_transform"], BG,
                                 filter_mode=fl.filter_mode, ndc_cull=fl.ndc_cull)
        col = sc["colors"] if colors is None else colors
        if cov is None:
            of = oracle_mod.forward(v, sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], col, extras=bool(fl.extras))
        else:
            of = oracle_mod.forward(v, sc["xyz"], None, None, sc["opacity"], col, cov3d=cov, extras=bool(fl.extras))
        dL = np.random.default_rng(4).random(of["image"].shape, dtype=np.float32)
        og = oracle_mod.backward(v, of, dL)
        dead = np.ones(N, bool)
        for k in ("means3D", "means2D", "opacities", "colors", "conic"):
            dead &= ~og[k].reshape(N, -1).any(axis=1)
        assert 0 < dead.sum() < N
        _refs[key] = (of, dL, dead)
    return _refs[key]


def _leaves(sc, dev, cov=None, shs=None):
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
    lv = dict(means3D=T(sc["xyz"]), opacities=T(sc["opacity"]))
    if cov is None:
        lv.update(scales=T(sc["scaling"]), rotations=T(sc["rotation"]))
    else:
        lv["cov3D"] = T(cov)
    if shs is None:
        lv["colors"] = T(sc["colors"])
    else:
        lv["shs"] = T(shs)
    return lv


def _call(rast, lv, dev, **extra):
    m2 = torch.zeros(N, 3, device=dev, requires_grad=True)
    out = rast(means3D=lv["means3D"], means2D=m2, shs=lv.get("shs"), colors_precomp=lv.get("colors"), opacities=lv["opacities"],
               scales=lv.get("scales"), rotations=lv.get("rotations"), cov3D_precomp=lv.get("cov3D"), **extra)
    return out, m2


def _package(name):
    import diff_gaussian_rasterization as up
    import diff_gaussian_rasterization_wodilate as wo
    return wo if name == "wodilate" else up


def _fwd(out, extras):
    """The deterministic outputs of a package call, by name."""
    names = ("image", "radii", "point_id_pixel", "point_weight_pixel", "point_weight") if extras else ("image", "radii")
    return {k: t.detach().cpu().numpy() for k, t in zip(names, out)}


def _grads(lv, m2):
    g = {k: t.grad.cpu().numpy() for k, t in lv.items() if t.grad is not None}
    g["means2D"] = m2.grad.cpu().numpy()
    return g


TRAINING_PARTS = ("geom", "state", "final_T", "n_contrib", "bwd_scratch")     # a training forward's carved parts ...
GRAD_PARTS = ("rot", "means3D", "scales", "colors", "opac")                    # ... and a fresh-gradient backward's


def _five_runs(call, ints=None, parts=TRAINING_PARTS + GRAD_PARTS):
    """call() -> (exact: dict of deterministic arrays, grads: dict) unpoisoned and under each fill -> {fill: (exact, grads)};
    every poisoned call made hooked allocations, the carved `parts` among them."""
    return P.run_fills(call, ints=ints, sync=torch.cuda.synchronize, parts=parts)


def _assert_runs(what, runs, dead=None, live_keys=()):
    ex0, g0 = runs[None]
    for fill, (ex, g) in runs.items():
        assert ex.keys() == ex0.keys() and g.keys() == g0.keys(), (what, fill)
        for k in ex0:
            assert P.same_bits(ex[k], ex0[k]), (what, fill, k)
            if np.asarray(ex[k]).dtype.kind == "f":
                assert np.isfinite(ex[k]).all(), (what, fill, k)
        for k in g0:
            assert np.isfinite(g[k]).all(), (what, fill, k, int((~np.isfinite(g[k])).sum()))
            if dead is not None and k in PER_ROW:
                assert not g[k].reshape(N, -1)[dead].any(), (what, fill, k)           # exactly 0.0 where the oracle's row is
            assert k in WALK or k in CHAIN, k
            e = rel_l2(g[k], g0[k])
            if fill is not None:
                print("ORDER %s %s %s: %.2e" % (what, fill, k, e))
            assert e < (ORDER_TOL if k in WALK else CHAIN_TOL), (what, fill, k, e)
    for k in live_keys:
        assert float(np.abs(g0[k]).sum()) > 0, (what, k)


def _assert_oracle_forward(what, runs, of):
    for fill, (ex, _) in runs.items():
        assert np.array_equal(ex["image"].view(np.uint32), of["image"].view(np.uint32)), (what, fill)
        assert np.array_equal(ex["radii"], of["radii"]), (what, fill)
        if "point_id_pixel" in ex:
            assert np.array_equal(ex["point_id_pixel"], of["point_id_pixel"]), (what, fill)
            assert np.array_equal(ex["point_weight"].view(np.uint32), of["point_weight"].view(np.uint32)), (what, fill)
            assert np.array_equal(ex["point_weight_pixel"].view(np.uint32), of["point_weight_pixel"].view(np.uint32)), (what, fill)


def _record(what, census):
    print("CENSUS %s: %s; fills %s" % (what, census["nan"].summary(), ", ".join(P.FILLS)))


@contextlib.contextmanager
def _mode(mode):
    """exact: stage 1, read-back, stage 2; speculative: the default; fixed: the caller's capacity, no read-back."""
    from log_amd import rasterizer as R
    prev = R.set_speculative(mode != "exact")
    if mode == "fixed":
        R.set_instance_capacity(16384)                 # the scene has 12 K tile instances in either flavour
        R.overflow_since_reset(torch.device(DEV))      # (the status block is sticky: whatever an earlier test left is read off)
    try:
        yield
    finally:
        R.set_instance_capacity(None)
        R.set_speculative(prev)
        R.capacity_stats(reset=True)


@pytest.mark.parametrize("mode", ["exact", "speculative", "fixed"])
@pytest.mark.parametrize("package", ["wodilate", "upstream"])
def test_plain_call_in_every_capacity_mode(oracle_mod, package, mode):
    import gpu_util as G
    from log_amd import rasterizer as R
    dev = torch.device(DEV)
    cam, sc = _scene()
    of, dL, dead = _reference(oracle_mod, package)
    w = torch.tensor(dL, device=dev)
    extras = package == "wodilate"

    def call():
        lv = _leaves(sc, dev)
        rast = _package(package).GaussianRasterizer(raster_settings=G.settings(cam, BG, dev))
        out, m2 = _call(rast, lv, dev)
        out[0].backward(gradient=w)
        return _fwd(out, extras), _grads(lv, m2)

    with _mode(mode):
        runs, census = _five_runs(call)
        if mode == "fixed":
            assert not R.overflow_since_reset(dev)["overflowed"]
    for c in census.values():
        assert {"geom", "state", "final_T", "n_contrib", "bwd_scratch", "means3D", "rot"} <= c.parts(), sorted(c.parts())
        assert ("plist" in c.parts()) == (mode == "fixed")
    _record("package-%s-%s" % (package, mode), census)
    _assert_oracle_forward((package, mode), runs, of)
    _assert_runs((package, mode), runs, dead, live_keys=("means3D", "scales", "rotations", "opacities", "colors", "means2D"))


def test_speculative_guess_that_is_too_small(oracle_mod):
    """The failed attempt wrote into state, final_T, the outputs; stage 2 is repeated into those buffers (forced as
    tests/test_gpu_dropin_modes.py forces it: the resolution's history says one instance)."""
    import gpu_util as G
    from log_amd import rasterizer as R
    from test_gpu_parity import _case
    cam, sc = _case("dense_tile")
    key = (0, cam["image_width"], cam["image_height"], (0, 0))
    _, of = G.oracle_forward(oracle_mod, cam, sc, BG)
    dL = np.random.default_rng(4).random(of["image"].shape, dtype=np.float32)
    too_small = [dict(I=1.0, ratio=1e-6, L=float(1 << 20)), dict(I=float(4 * of["I"]), ratio=0.0, L=1.0)]

    def call(guess):
        R.capacity_stats(reset=True)
        R._cap_model.hist[key] = dict(guess)
        hf = G.hip_forward(cam, sc, BG, scratch_floats=16)
        assert R.capacity_stats() == dict(forwards=1, retries=1)
        hg = G.hip_backward(hf, dL)
        return hf, hg

    prev = R.set_speculative(True)
    try:
        for guess in too_small:
            runs = {}
            for fill in (None,) + P.FILLS:
                with (P.poisoned(fill) if fill else contextlib.nullcontext()) as c:
                    runs[fill] = call(guess)
                assert fill is None or {"geom", "state", "final_T", "n_contrib", "bwd_scratch"} <= c.parts()
            assert not R.overflow_since_reset(torch.device(DEV))["overflowed"]
            hf0, hg0 = runs[None]
            for fill, (hf, hg) in runs.items():
                st = G.compare_forward(hf, of)
                for k in ("radii_mismatch", "rec_bits_mismatch", "offsets_mismatch", "list_mismatch", "n_contrib_mismatch",
                          "image_bits_mismatch", "final_T_bits_mismatch", "pid_mismatch"):
                    assert st[k] == 0, (fill, k, st)
                assert st["pwp_max_abs"] == 0.0 and st["pw_max_abs"] == 0.0, (fill, st)
                for k in hg0:
                    assert np.isfinite(hg[k]).all(), (fill, k)
                    e = rel_l2(hg[k], hg0[k])
                    assert e < (ORDER_TOL if k in ("means2D", "conic", "opacities", "colors") else CHAIN_TOL), (fill, k, e)
    finally:
        R.set_speculative(prev)
        R.capacity_stats(reset=True)


def test_aux_pair(oracle_mod):
    """colour and a second triple composited by one walk, both images differentiated by one reverse walk."""
    import gpu_util as G
    dev = torch.device(DEV)
    cam, sc = _scene()
    aux = np.random.default_rng(8).random((N, 3), dtype=np.float32)
    of, dL, dead = _reference(oracle_mod, "wodilate")
    of_aux, _, _ = _reference(oracle_mod, "wodilate", colors=aux, key="aux")
    w = torch.tensor(dL, device=dev)
    w2 = torch.tensor(np.random.default_rng(9).random((3, H, W), dtype=np.float32), device=dev)

    def call():
        lv = _leaves(sc, dev)
        lv["aux_colors"] = torch.tensor(aux, device=dev, requires_grad=True)
        rast = _package("wodilate").GaussianRasterizer(raster_settings=G.settings(cam, BG, dev))
        m2 = torch.zeros(N, 3, device=dev, requires_grad=True)
        out = rast(means3D=lv["means3D"], means2D=m2, shs=None, colors_precomp=lv["colors"], opacities=lv["opacities"],
                   scales=lv["scales"], rotations=lv["rotations"], cov3D_precomp=None, aux_colors=lv["aux_colors"])
        ((out[0] * w).sum() + (out[-1] * w2).sum()).backward()
        return dict(_fwd(out[:5], True), aux_image=out[-1].detach().cpu().numpy()), _grads(lv, m2)

    runs, census = _five_runs(call)
    _record("aux-pair", census)
    _assert_oracle_forward("aux", runs, of)
    for fill, (ex, _) in runs.items():
        assert np.array_equal(ex["aux_image"].view(np.uint32), of_aux["image"].view(np.uint32)), fill
    for c in census.values():
        assert "aux" in c.parts()
    _assert_runs("aux", runs, dead, live_keys=("aux_colors", "colors", "means3D"))


def test_second_pass_with_geometry_reuse(oracle_mod):
    """The same rasterizer object called twice with the same geometry: the second call recolours the first call's records and
    walks its lists again (lograst_recomposite) into buffers of its own."""
    import gpu_util as G
    from log_amd import rasterizer as R
    dev = torch.device(DEV)
    cam, sc = _scene()
    depth = np.random.default_rng(10).random((N, 3), dtype=np.float32)
    of, dL, dead = _reference(oracle_mod, "wodilate")
    of2, _, _ = _reference(oracle_mod, "wodilate", colors=depth, key="second")
    w = torch.tensor(dL, device=dev)

    def call():
        R.geometry_reuse_stats(reset=True)
        lv = _leaves(sc, dev)
        lv["second"] = torch.tensor(depth, device=dev, requires_grad=True)
        rast = _package("wodilate").GaussianRasterizer(raster_settings=G.settings(cam, BG, dev))
        m2, m2b = (torch.zeros(N, 3, device=dev, requires_grad=True) for _ in range(2))
        kw = dict(means3D=lv["means3D"], shs=None, opacities=lv["opacities"], scales=lv["scales"], rotations=lv["rotations"],
                  cov3D_precomp=None)
        a = rast(means2D=m2, colors_precomp=lv["colors"], **kw)
        b = rast(means2D=m2b, colors_precomp=lv["second"], **kw)
        assert R.geometry_reuse_stats()["reused"] == 1
        ((a[0] * w).sum() + (b[0] * w).sum()).backward()
        ex = _fwd(a, True)
        ex.update({"second_" + k: v for k, v in _fwd(b, True).items()})
        g = _grads(lv, m2)
        g["colors"] = np.concatenate([g["colors"], g.pop("second")])            # (both colour gradients: reverse-walk outputs)
        g["means2D"] = np.concatenate([g["means2D"], m2b.grad.cpu().numpy()])
        return ex, g

    prev = R.set_geometry_reuse(True)
    try:
        runs, census = _five_runs(call)
    finally:
        R.set_geometry_reuse(prev)
        R.geometry_reuse_stats(reset=True)
    _record("second-pass", census)
    _assert_oracle_forward("first pass", runs, of)
    _assert_oracle_forward("second pass", {f: ({k[7:]: v for k, v in ex.items() if k.startswith("second_")}, g)
                                           for f, (ex, g) in runs.items()}, of2)
    ex0, g0 = runs[None]
    dead2 = np.concatenate([dead, dead])
    for fill, (ex, g) in runs.items():
        for k in ("colors", "means2D"):
            assert not g[k][dead2].any(), (fill, k)
    _assert_runs("second pass", {f: (ex, {k: v for k, v in g.items() if k not in ("colors", "means2D")})
                                 for f, (ex, g) in runs.items()}, dead, live_keys=("means3D",))
    for fill, (_, g) in runs.items():
        for k in ("colors", "means2D"):
            assert np.isfinite(g[k]).all() and rel_l2(g[k], g0[k]) < ORDER_TOL, (fill, k, rel_l2(g[k], g0[k]))


def test_camera_gradients(oracle_mod):
    import gpu_util as G
    dev = torch.device(DEV)
    cam, sc = _scene()
    of, dL, dead = _reference(oracle_mod, "wodilate")
    w = torch.tensor(dL, device=dev)

    def call():
        lv = _leaves(sc, dev)
        rs = G.settings(cam, BG, dev)
        rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True), projmatrix=rs.projmatrix.clone().requires_grad_(True))
        out, m2 = _call(_package("wodilate").GaussianRasterizer(raster_settings=rs), lv, dev)
        out[0].backward(gradient=w)
        g = _grads(lv, m2)
        g.update(viewmatrix=rs.viewmatrix.grad.cpu().numpy(), projmatrix=rs.projmatrix.grad.cpu().numpy())
        return _fwd(out, True), g

    runs, census = _five_runs(call)
    _record("camera-gradients", census)
    _assert_oracle_forward("camera", runs, of)
    for fill, (_, g) in runs.items():
        assert g["viewmatrix"].shape == (4, 4) and not g["viewmatrix"][:, 3].any() and not g["projmatrix"][:, 2].any(), fill
    _assert_runs("camera", runs, dead, live_keys=("viewmatrix", "projmatrix", "means3D"))


@pytest.mark.parametrize("min_n", [None, 1000], ids=["default", "min_n-1000"])
@pytest.mark.parametrize("form", ["rows", "quadrant"])
def test_abs_grad(oracle_mod, form, min_n):
    """min_n = 1000: LOGRAST_HELPER_MIN_N below the 2000 Gaussians -- the touched-only regime (the forward clears the accumulator
    rows it meets, nobody clears the others) with the absolute sums in slots 9 and 10 of those rows."""
    import gpu_util as G
    from log_amd import rasterizer as R, tune
    dev = torch.device(DEV)
    cam, sc = _scene()
    of, dL, dead = _reference(oracle_mod, "wodilate")
    w = torch.tensor(dL, device=dev)

    def call():
        lv = _leaves(sc, dev)
        rast = _package("wodilate").GaussianRasterizer(raster_settings=G.settings(cam, BG, dev), walk_form=form, abs_grad=True)
        out, m2 = _call(rast, lv, dev)
        out[0].backward(gradient=w)
        assert R._backend.last_forms == {"fwd": form, "bwd": form}
        g = _grads(lv, m2)
        g["absgrad"] = m2.absgrad.cpu().numpy()
        return _fwd(out, True), g

    tune.reset_knobs()
    if min_n is not None:
        tune.set_knob("LOGRAST_HELPER_MIN_N", min_n)
    try:
        runs, census = _five_runs(call)
    finally:
        tune.reset_knobs()
    _record("abs-grad-%s%s" % (form, "" if min_n is None else "-min_n-%d" % min_n), census)
    _assert_oracle_forward("abs-grad", runs, of)
    for fill, (_, g) in runs.items():
        assert not g["absgrad"][:, 2].any() and (g["absgrad"] >= 0).all(), fill
    _assert_runs("abs-grad-%s-%s" % (form, min_n), runs, dead, live_keys=("absgrad", "means2D"))


@pytest.mark.parametrize("degree", [1, 3])
def test_native_shs(oracle_mod, degree):
    """`shs=` at degree 1 and 3 (16 stored coefficients): the image is the oracle's for the colours the SH kernel gives."""
    import gpu_util as G
    from log_amd import rasterizer as R
    dev = torch.device(DEV)
    cam, sc = _scene()
    shs = (0.3 * np.random.default_rng(11).standard_normal((N, 16, 3))).astype(np.float32)
    shs[:, 0] += 0.8
    rs = G.settings(cam, BG, dev)._replace(sh_degree=degree)
    colours, _ = R._backend.sh_forward(torch.tensor(sc["xyz"], device=dev), rs.campos, torch.tensor(shs, device=dev), degree)
    of, dL, dead = _reference(oracle_mod, "wodilate", colors=colours.cpu().numpy(), key=("shs", degree))
    w = torch.tensor(dL, device=dev)

    def call():
        lv = _leaves(sc, dev, shs=shs)
        out, m2 = _call(_package("wodilate").GaussianRasterizer(raster_settings=rs), lv, dev)
        out[0].backward(gradient=w)
        return _fwd(out, True), _grads(lv, m2)

    runs, census = _five_runs(call)
    _record("shs-degree-%d" % degree, census)
    _assert_oracle_forward(("shs", degree), runs, of)
    for fill, (_, g) in runs.items():
        assert not g["shs"][:, (degree + 1) ** 2:].any(), fill                   # coefficients above the active degree
    _assert_runs(("shs", degree), runs, dead, live_keys=("shs", "means3D"))


@pytest.mark.parametrize("package", ["wodilate", "upstream"])
def test_cov3d_precomp(oracle_mod, package):
    import gpu_util as G
    from oracle import torch_oracle
    dev = torch.device(DEV)
    cam, sc = _scene()
    Rm = torch_oracle._rot(torch.tensor(sc["rotation"], dtype=torch.float64))
    M = Rm * torch.tensor(sc["scaling"], dtype=torch.float64)[:, None, :]
    S = (M @ M.transpose(1, 2)).numpy()
    cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32)
    of, dL, dead = _reference(oracle_mod, package, cov=cov, key="cov3D")
    w = torch.tensor(dL, device=dev)
    extras = package == "wodilate"

    def call():
        lv = _leaves(sc, dev, cov=cov)
        out, m2 = _call(_package(package).GaussianRasterizer(raster_settings=G.settings(cam, BG, dev)), lv, dev)
        out[0].backward(gradient=w)
        return _fwd(out, extras), _grads(lv, m2)

    runs, census = _five_runs(call)
    _record("cov3D-" + package, census)
    _assert_oracle_forward(("cov3D", package), runs, of)
    _assert_runs(("cov3D", package), runs, dead, live_keys=("cov3D", "means3D"))


# ---- the caller's running sums ---------------------------------------------------------------------------------------------

def _prefill(numel, dev, seed=5):
    """Known values for a sink that is already under way: small dyadic numbers (k / 1024, k = -7 .. 7), so that what a backward
    adds to them is recovered by an exact subtraction."""
    k = np.random.default_rng(seed).integers(-7, 8, size=numel).astype(np.float32) / np.float32(1024)
    return torch.tensor(k, device=dev)


@pytest.mark.parametrize("row_major", [False, True], ids=["planar", "rows"])
def test_two_views_into_one_sink(oracle_mod, row_major):
    """accumulate_grads_into: the sums of two views are ADDED to exactly the values the caller's sink held (the sink is the
    caller's: prefilled outside the poisoned block); rows dead in both views keep those values bit for bit."""
    import gpu_util as G
    from log_amd import rasterizer as R
    from log_amd.dist import GradientBucket, ROW_COLUMNS
    dev = torch.device(DEV)
    views = (0, 1)
    refs = [_reference(oracle_mod, "wodilate", view=v) for v in views]
    dead = refs[0][2] & refs[1][2]
    assert dead.sum() > 0
    w = torch.tensor(refs[1][1], device=dev)
    sc = _scene()[1]

    def readout(bucket):
        src = bucket.alias if row_major else bucket.views
        return {k: src[k].reshape(N, b - a).clone() for k, (a, b) in ROW_COLUMNS.items()}

    def call(poison_ctx):
        bucket = GradientBucket(N, dev, row_major=row_major)
        bucket.flat.copy_(_prefill(bucket.flat.numel(), dev))
        if row_major:
            bucket.views["rows"][:, 14:] = 7.0
        before = readout(bucket)
        lv = _leaves(sc, dev)
        m2s = []
        with poison_ctx as c, R.accumulate_grads_into(bucket.sink()):
            for v in views:
                rast = _package("wodilate").GaussianRasterizer(raster_settings=G.settings(_scene(v)[0], BG, dev))
                out, m2 = _call(rast, lv, dev)
                (out[0] * w).sum().backward()
                m2s.append(m2.grad.cpu().numpy())
            torch.cuda.synchronize()
        assert all(t.grad is None for t in lv.values())
        if row_major:
            assert bool((bucket.views["rows"][:, 14:] == 7.0).all())
        after = readout(bucket)
        added = {k: (after[k].double() - before[k].double()).cpu().numpy() for k in after}
        for k in after:                                                   # nothing is added to a row dead in both views
            assert torch.equal(after[k][torch.tensor(dead, device=dev)], before[k][torch.tensor(dead, device=dev)]), k
        added["means2D"] = np.concatenate(m2s)
        return added, c

    base, _ = call(contextlib.nullcontext())
    assert set(base) - {"means2D"} == set(ROW_COLUMNS)
    for fill in P.FILLS:
        got, census = call(P.poisoned(fill))
        assert {"geom", "state", "bwd_scratch"} <= census.parts(), (fill, sorted(census.parts()))
        for k in base:
            assert np.isfinite(got[k]).all(), (fill, k)
            tol = ORDER_TOL if k in WALK else CHAIN_TOL
            assert float(np.abs(base[k]).sum()) > 0 and rel_l2(got[k], base[k]) < tol, (fill, k, rel_l2(got[k], base[k]))
        if fill == "nan":
            print("CENSUS sink-%s: %s; fills %s" % ("rows" if row_major else "planar", census.summary(), ", ".join(P.FILLS)))


def test_in_place_leaf_gradients(oracle_mod):
    """set_inplace_leaf_grads: the second view's backward adds into the .grad tensors the first view's left."""
    import gpu_util as G
    from log_amd import rasterizer as R
    dev = torch.device(DEV)
    views = (0, 1)
    refs = [_reference(oracle_mod, "wodilate", view=v) for v in views]
    dead = refs[0][2] & refs[1][2]
    w = torch.tensor(refs[1][1], device=dev)
    sc = _scene()[1]

    def call():
        lv = _leaves(sc, dev)
        ptrs = None
        for i, v in enumerate(views):
            rast = _package("wodilate").GaussianRasterizer(raster_settings=G.settings(_scene(v)[0], BG, dev))
            out, m2 = _call(rast, lv, dev)
            (out[0] * w).sum().backward()
            if i == 0:
                ptrs = {k: t.grad.data_ptr() for k, t in lv.items()}
        assert all(t.grad.data_ptr() == ptrs[k] for k, t in lv.items())      # added in place
        return {}, _grads(lv, m2)

    prev = R.set_inplace_leaf_grads(True)
    try:
        runs, census = _five_runs(call)
    finally:
        R.set_inplace_leaf_grads(prev)
    _record("in-place-leaf-grads", census)
    for fill, (_, g) in runs.items():
        for k in ("means3D", "scales", "rotations", "opacities", "colors"):
            assert not g[k].reshape(N, -1)[dead].any(), (fill, k)
    _assert_runs("in-place", runs, None, live_keys=("means3D", "scales", "rotations", "opacities", "colors"))

"""Every mode the two backward launchers can select (log_amd/csrc/blend.hip: lr_launch_blend_bwd; project_bwd.hip:
lr_launch_project_bwd), each on the smallest scene that still reaches every branch and each against the plain fresh-gradient
backward of the same forward.

The scene: 2000 trained-like Gaussians on 64 x 64 -- 16 tiles, two chain-rule workgroups of 1024 rows, the second partial
(976) -- with at least one tile list of more than 64 entries (asserted), so that the walks cross a chunk boundary.  One
training forward (hit masks on) per record: the 5-tuple flavour (point_weight) pinned to the row-split form, the upstream
flavour (no point_weight) pinned to the quadrant form, the 5-tuple flavour on a tile_rows band, and both flavours with aux
channels and with cov3D_precomp.

  reverse walk   {quadrant, row-split} x {masks used, masks not usable}: each record in its forward's form (its masks are
                 used) and in the other one (they are not); the same four with abs-grad; aux: masks, no masks, with and
                 without point_weight
  chain rule     fresh gradients with and without point_weight; the attribute-major and the row-major sink, on small and on
                 large inputs (LOGRAST_HELPER_MIN_N = 0: the staged slice) and through the list form (LOGRAST_PBWD_LIST = 2);
                 the row-major sink on a band (the four-wave form); cov3D_precomp with and without point_weight and through
                 project_backward(cov3D=); camera sums through backward_camera and through project_backward(camera=True)

The bar is the project's own: rel-L2 <= 1e-4 per tensor over ALL rows.  The plain backward of each record
is first held to the C oracle and the float64 twin (gpu_util.assert_gradients_anchored).  A chain-rule mode does not reorder
the walk, so its dL/dmeans2D must be the plain backward's bit for bit: it is handed a copy of the accumulator rows the plain
backward's reverse walk left, with dL/dimage = 0 -- its own walk runs and adds nothing -- because two walks of the same
gradient commit their float atomics in different orders.  Sinks start from zeros."""
import numpy as np
import pytest
import torch

from util import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-4          # relative L2 per tensor, every row
N, W, H = 2000, 64, 64
BG = (0.1, 0.2, 0.3)
BAND = (1, 3)       # tile rows [1, 3) of 4
SIX = ("means3D", "means2D", "colors", "opacities", "scales", "rotations")
FORM_CODE = {"rows": 1, "quadrant": 2}

_cache = {}


def setup():
    """The scene, its tensors and dL/dimage: built once, never changed."""
    if "setup" not in _cache:
        from log_amd import scenes
        import gpu_util as G
        dev = torch.device("cuda:0")
        cam = scenes.orbit_cameras(3, W=W, H=H, focal=150.0)[1]
        sc = scenes.trained_like_scene(N, seed=3)
        t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
        dL = np.random.default_rng(4).standard_normal((3, H, W)).astype(np.float32)
        _cache["setup"] = dict(dev=dev, cam=cam, sc=sc, rs=G.settings(cam, BG, dev), m=t(sc["xyz"]), s=t(sc["scaling"]),
                               r=t(sc["rotation"]), o=t(sc["opacity"]).reshape(-1), c=t(sc["colors"]), dL_np=dL, dL=t(dL),
                               zero=torch.zeros(3, H, W, device=dev))
    return _cache["setup"]


def flavour_of(name):
    from log_amd import rasterizer as R
    return {"wodilate": R.WODILATE, "upstream": R.UPSTREAM}[name]


def cov3d_of(sc):
    from oracle import torch_oracle
    Rm = torch_oracle._rot(torch.tensor(sc["rotation"], dtype=torch.float64))
    M = Rm * torch.tensor(sc["scaling"], dtype=torch.float64)[:, None, :]
    S = (M @ M.transpose(1, 2)).numpy()
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32)


def record(flavour, form, band=(0, 0), aux=False, cov=False):
    """One training forward (shared, left unchanged) -> dict(saved, flavour, args of the backend's backward)."""
    key = (flavour, form, band, aux, cov)
    if key not in _cache:
        from log_amd import rasterizer as R
        u = setup()
        fl = flavour_of(flavour)
        cv = torch.tensor(cov3d_of(u["sc"]), device=u["dev"]) if cov else None
        s, r = (None, None) if cov else (u["s"], u["r"])
        with R.walk_form(form), R.tile_rows(*band):
            if aux:
                out = R._backend.forward_aux(u["rs"], fl, True, u["m"], s, r, u["o"], u["c"], u["c"].clone(), scratch_floats=16)
            else:
                out = R._backend.forward(u["rs"], fl, True, u["m"], s, r, u["o"], u["c"], scratch_floats=16, cov3D=cv)
        torch.cuda.synchronize()
        saved = out[-1]
        assert saved["hit_masks"] is not None and saved["hit_mask_form"] == FORM_CODE["quadrant" if aux else form]
        assert tuple(saved["tile_rows"]) == tuple(band)
        lens = np.diff(R.tile_offsets_of(saved, W, H).cpu().numpy().astype(np.int64))
        assert len(lens) == 16 and lens.max() > 64, lens            # a walk that crosses a chunk boundary
        assert (N + 1023) // 1024 == 2 and N % 1024 != 0            # two chain-rule workgroups, the second partial
        _cache[key] = dict(saved=saved, flavour=fl, name=flavour, cov=cv, head=(u["rs"], fl, True, u["m"], s, r))
    return _cache[key]


def as_dict(six):
    return {k: (g.detach().cpu().numpy() if g is not None else None) for k, g in zip(SIX, six)}


def plain(rec):
    """The plain fresh-gradient backward of a record, once -> (gradients, the accumulator rows its reverse walk left,
    dL/dconic [N, 4]).  Its rows start as zeros of the test's own, so that they can be copied afterwards."""
    if "plain" not in rec:
        from log_amd import rasterizer as R
        import gpu_util as G   # noqa: F401  (keeps dL/dconic of the last backward: R._debug_keep)
        u = setup()
        rows = torch.zeros(N * 16, device=u["dev"])
        six = R._backend.backward(*rec["head"], dict(rec["saved"], bwd_scratch=rows), u["dL"], cov3D=rec["cov"])
        torch.cuda.synchronize()
        g = as_dict(six)
        if rec["cov"] is not None:
            g["cov3D"], g["scales"] = g["scales"], None
        rec["plain"] = (g, rows, R._backend.last_conic_grad.clone())
    return rec["plain"]


def oracle_of(oracle_mod, rec):
    """(view, forward, fp32 backward, float64 twin) of the record's flavour and band, once."""
    if "oracle" not in rec:
        import gpu_util as G
        u = setup()
        v, of = G.oracle_forward(oracle_mod, u["cam"], u["sc"], BG, flavour=rec["flavour"], tile_rows=rec["saved"]["tile_rows"])
        rec["oracle"] = (v, of, oracle_mod.backward(v, of, u["dL_np"], abs_sums=True), oracle_mod.backward_f64(v, of, u["dL_np"]))
    return rec["oracle"]


def check(name, got, want, keys=SIX, exact=()):
    """rel-L2 <= TOL per tensor over all rows (printed before it is asserted); `exact`: bit for bit."""
    fig = {}
    for k in keys:
        a, b = np.asarray(got[k], np.float32).reshape(np.shape(want[k])), np.asarray(want[k], np.float32)
        assert np.isfinite(a).all(), (name, k)
        fig[k] = 0.0 if np.array_equal(a.view(np.uint32), b.view(np.uint32)) else max(rel_l2(a, b), 1e-300)
    print("BWDMODE %-44s %s" % (name, "  ".join("%s %.2e" % (k, e) for k, e in fig.items())))
    for k in keys:
        assert float(np.abs(want[k]).sum()) > 0, (name, k)
        assert fig[k] <= TOL, (name, k, fig[k])
        assert k not in exact or fig[k] == 0.0, (name, k, fig[k])
    return fig


RECORDS = {"pw-rows": ("wodilate", "rows"), "nopw-quadrant": ("upstream", "quadrant")}


@pytest.mark.parametrize("which", list(RECORDS))
def test_plain_backward_against_the_oracle(oracle_mod, which):
    """Fresh gradients with point_weight (5-tuple flavour) and without (upstream flavour): the reference of every other
    test here, held to the C oracle and the float64 twin; dL/dconic included."""
    import gpu_util as G
    rec = record(*RECORDS[which])
    g, rows, conic = plain(rec)
    assert float(rows.view(N, 16)[:, :9].abs().sum()) > 0
    v, of, og, g64 = oracle_of(oracle_mod, rec)
    hg = dict(g, conic=conic.cpu().numpy(), opacities=g["opacities"].reshape(-1, 1))
    check("plain %s vs oracle" % which, hg, og, keys=SIX + ("conic",))
    G.assert_gradients_anchored(G.gradient_anchor_stats(hg, og, g64), tol=TOL, max_excluded=0.10,
                                name="backward_modes_" + which, all_rows_tol=TOL)


@pytest.mark.parametrize("abs_sums", [False, True], ids=["plain", "abs"])
@pytest.mark.parametrize("form", ["rows", "quadrant"])
@pytest.mark.parametrize("which", list(RECORDS))
def test_reverse_walk_forms_and_masks(oracle_mod, which, form, abs_sums):
    """The record's masks serve a walk of its forward's form only: each record in both forms = {quadrant, row-split} x {masks
    used, masks not usable}, plain and with the absolute sums (against the oracle's: the same fp32 addends)."""
    from log_amd import rasterizer as R
    u, rec = setup(), record(*RECORDS[which])
    want, _, _ = plain(rec)
    saved = dict(rec["saved"], bwd_scratch=None, walk_form_pin=FORM_CODE[form])
    call = R._backend.backward_abs if abs_sums else R._backend.backward
    out = call(*rec["head"], saved, u["dL"])
    torch.cuda.synchronize()
    assert R._backend.last_forms["bwd"] == form
    masks = "masks used" if saved["hit_mask_form"] == FORM_CODE[form] else "masks not usable"
    assert (masks == "masks used") == (form == RECORDS[which][1])
    check("walk %s %s %s%s" % (which, form, masks, " abs" if abs_sums else ""), as_dict(out[:6]), want)
    if abs_sums:
        assert len(out) == 7 and out[6].shape == (N, 3) and bool((out[6][:, 2] == 0).all())
        check("walk %s %s %s absgrad" % (which, form, masks), dict(a=out[6][:, :2].cpu().numpy()),
              dict(a=oracle_of(oracle_mod, rec)[2]["absgrad"]), keys=("a",))


@pytest.mark.parametrize("masks", [True, False], ids=["masks", "no-masks"])
@pytest.mark.parametrize("which", list(RECORDS))
def test_aux_walk(which, masks):
    """The aux forward composited the colours a second time (aux_colors = colors), so dL/dimage through either image gives
    the plain backward's geometry gradients, and the colour gradient comes out on that image's side.  Both flavours: the aux
    chain rule with and without point_weight."""
    from log_amd import rasterizer as R
    u = setup()
    rec = record(RECORDS[which][0], "quadrant", aux=True)
    want, _, _ = plain(record(*RECORDS[which]))
    zeros = np.zeros((N, 3), np.float32)
    for side, grads in (("image", (u["dL"], None)), ("aux image", (None, u["dL"]))):
        saved = dict(rec["saved"], bwd_scratch=None)
        if not masks:
            saved["hit_masks"] = None
        out = R._backend.backward_aux(*rec["head"], saved, *grads)
        torch.cuda.synchronize()
        assert R._backend.last_forms["bwd"] == "quadrant" and len(out) == 7
        g = as_dict(out[:6])
        g_aux = out[6].cpu().numpy()
        if side == "aux image":
            g["colors"], g_aux = g_aux, g["colors"]
        check("aux %s %s through the %s" % (which, "masks" if masks else "no masks", side), g, want)
        assert np.array_equal(g_aux, zeros)


def chain_rule(rec, **kw):
    """backward() of the record on a copy of the plain backward's accumulator rows, with dL/dimage = 0."""
    from log_amd import rasterizer as R
    u = setup()
    _, rows, _ = plain(rec)
    out = R._backend.backward(*rec["head"], dict(rec["saved"], bwd_scratch=rows.clone()), u["zero"], **kw)
    torch.cuda.synchronize()
    return out


def sink_of(kind, dev):
    z = lambda *shape: torch.zeros(*shape, device=dev)
    return dict(rows=z(N, 16)) if kind == "rows" else dict(means3D=z(N, 3), scales=z(N, 3), rotations=z(N, 4), opacities=z(N),
                                                           colors=z(N, 3))


def sums_of(kind, sink):
    if kind == "rows":
        a = sink["rows"].cpu().numpy()
        assert not a[:, 14:].any()
        return dict(means3D=a[:, 0:3], scales=a[:, 3:6], rotations=a[:, 6:10], opacities=a[:, 10], colors=a[:, 11:14])
    return {k: v.cpu().numpy() for k, v in sink.items()}


SINK_KNOBS = {"small": {}, "staged": {"LOGRAST_HELPER_MIN_N": 0, "LOGRAST_PBWD_LIST": 0},
              "list": {"LOGRAST_HELPER_MIN_N": 0, "LOGRAST_PBWD_LIST": 2}}


@pytest.mark.parametrize("route", list(SINK_KNOBS))
@pytest.mark.parametrize("kind", ["attributes", "rows"])
@pytest.mark.parametrize("which", list(RECORDS) + ["pw-band"])
def test_chain_rule_sinks(which, kind, route):
    """Running sums from zeros = the fresh gradients: attribute-major and row-major, on a small input, on a large one (the
    staged slice of dL/dmeans2D) and through the list form (with point_weight; without, the knob leaves the one-kernel form);
    on a band the row-major sink takes the four-wave form."""
    from log_amd import tune
    rec = record("wodilate", "quadrant", band=BAND) if which == "pw-band" else record(*RECORDS[which])
    want, _, _ = plain(rec)
    sink = sink_of(kind, setup()["dev"])
    try:
        for k, val in SINK_KNOBS[route].items():
            tune.set_knob(k, val)
        out = chain_rule(rec, sink=sink)
    finally:
        tune.reset_knobs()
    assert [g is None for g in out] == [True, False, True, True, True, True]
    got = dict(sums_of(kind, sink), means2D=out[1].cpu().numpy())
    check("sink %s %s %s" % (which, kind, route), got, want, exact=("means2D",))


@pytest.mark.parametrize("which", list(RECORDS) + ["pw-band"])
def test_chain_rule_fresh_again(which):
    """The chain rule alone on the copied rows: what the modes above are compared through, bit for bit the plain backward."""
    rec = record("wodilate", "quadrant", band=BAND) if which == "pw-band" else record(*RECORDS[which])
    check("fresh %s" % which, as_dict(chain_rule(rec)), plain(rec)[0], exact=SIX)


@pytest.mark.parametrize("flavour", ["wodilate", "upstream"])
def test_chain_rule_cov3d(oracle_mod, flavour):
    """cov3D_precomp: its own record (the covariances of the same scales and rotations), against the C oracle's cov3D path,
    with and without point_weight; then the same dL/dmeans2D and dL/dconic through project_backward(cov3D=)."""
    from log_amd import rasterizer as R
    from util import cam_tan
    u = setup()
    rec = record(flavour, "quadrant", cov=True)
    g = plain(rec)[0]
    fl = rec["flavour"]
    tfx, tfy = cam_tan(u["cam"])
    v = oracle_mod.make_view(W, H, tfx, tfy, u["cam"]["world_view_transform"], u["cam"]["full_proj_transform"], BG,
                             filter_mode=fl.filter_mode, ndc_cull=fl.ndc_cull)
    of = oracle_mod.forward(v, u["sc"]["xyz"], None, None, u["sc"]["opacity"], u["sc"]["colors"], cov3d=cov3d_of(u["sc"]),
                            extras=bool(fl.extras))
    og = oracle_mod.backward(v, of, u["dL_np"])
    keys = ("cov3D", "means3D", "means2D", "colors", "opacities")
    check("cov3D %s vs oracle" % flavour, g, og, keys=keys)
    again = as_dict(chain_rule(rec, cov3D=rec["cov"]))
    again["cov3D"] = again["scales"]
    check("cov3D %s chain rule again" % flavour, again, g, keys=keys, exact=keys)
    p = R._backend.project_backward(*rec["head"], rec["saved"]["radii"], torch.tensor(g["means2D"], device=u["dev"]), plain(rec)[2],
                                    cov3D=rec["cov"])
    torch.cuda.synchronize()
    assert len(p) == 3 and p[2] is None
    check("cov3D %s project_backward" % flavour, dict(means3D=p[0].cpu().numpy(), cov3D=p[1].cpu().numpy()), g,
          keys=("means3D", "cov3D"))


@pytest.mark.parametrize("which", list(RECORDS))
def test_chain_rule_camera(which):
    """The camera sums ride on the chain rule: backward_camera's six gradients are the plain ones, and the same dL/dmeans2D
    and dL/dconic through project_backward(camera=True) give the same three gradients and the same two matrices."""
    from log_amd import rasterizer as R
    u, rec = setup(), record(*RECORDS[which])
    want, rows, conic = plain(rec)
    out = R._backend.backward_camera(*rec["head"], dict(rec["saved"], bwd_scratch=rows.clone()), u["zero"])
    torch.cuda.synchronize()
    assert len(out) == 8
    check("camera %s backward_camera" % which, as_dict(out[:6]), want, exact=("means2D",))
    cam = dict(V=out[6].cpu().numpy(), P=out[7].cpu().numpy())
    assert not cam["V"][:, 3].any() and not cam["P"][:, 2].any()
    m2 = torch.tensor(want["means2D"], device=u["dev"])
    three = ("means3D", "scales", "rotations")
    for camera in (False, True):
        p = R._backend.project_backward(*rec["head"], rec["saved"]["radii"], m2, conic, camera=camera)
        torch.cuda.synchronize()
        assert len(p) == (5 if camera else 3)
        check("camera %s project_backward(camera=%s)" % (which, camera), dict(zip(three, (t.cpu().numpy() for t in p[:3]))), want,
              keys=three)
    check("camera %s matrices, both routes" % which, dict(V=p[3].cpu().numpy(), P=p[4].cpu().numpy()), cam, keys=("V", "P"))

"""The binning stage ON its class, chunk and batch boundaries (log_amd/csrc/project.hip: the projection's counting and
ranking, lr_count_huge_kernel, the scan, the two fill kernels; api.hip: lr_pick_batch), instead of wherever a random scene
lands:

  rect class    nt = w h: 4/5 (LR_RANKED_TILES), 16/17 (LOGRAST_DEFER_TILES, LR_MID_ROW), 64/65 (one whole-wave pass), the whole
                grid; every tile order of the ranked class (row, column, 2x2)
  lr_mid_rects  1, 4, 5, 64 mid rects in one wave (four per pass); 16 / 17 (LOGRAST_MID_COOP: cooperative / per lane)
  rank rows     1023 / 1024 / 1025 rankable rects in a batch of 4096 (lr_mid_cap), rows of the next batch behind them
  deferred      8 / 9 per 256-Gaussian chunk (LR_HUGE_DIRECT), flagged chunks at a batch's end and start, hugemask words 0 / 1
  array ends    N = 1, 63, 64, 65, 4095, 4096, 4097, 4160 with a special rect in the last Gaussian
  plan          batch 4096 / 6144 / 10240 / 18432, one and two planes per workgroup, staged fill K = 2 / 3 / off
  band form     0 ... 129 survivors in one wave's ring, 300 over two slot chunks, all waves sharing the slot cursor

The scenes (tests/rect_cases.py) are fillers behind the camera with live rects at stated indices; which path every live
Gaussian takes is declared there and asserted on the CPU (tests/test_rect_cases_cpu.py).  Here every case runs with the
support cull on and off: everything the forward returns bit for bit the oracle's, and the device's own record of the path --
fill records, rank rows, header words, hugemask (gpu_util.binning_record) -- is what the case declares."""
import numpy as np
import pytest

import rect_cases as RC
from util import cam_tan, rel_l2

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4   # relative L2 against the oracle (BASELINE.json)
BG = (0.3, 0.6, 0.9)
EXACT = ("radii_mismatch", "rec_bits_mismatch", "offsets_mismatch", "list_mismatch", "n_contrib_mismatch",
         "image_bits_mismatch", "final_T_bits_mismatch")
FULL_CASES = [c for c in RC.CASES if not c.band]


def _same_bits(a, b, what):
    for k in ("image", "final_T", "point_weight_pixel", "point_weight"):
        if k in a:
            assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), (what, k)
    for k in ("radii", "tile_offsets", "point_list", "n_contrib", "point_id_pixel"):
        if k in a:
            assert (a[k] == b[k]).all(), (what, k)


def _assert_exact(G, hf, of, what):
    st = G.compare_forward(hf, of)
    for k in EXACT + (("pid_mismatch",) if "pid_mismatch" in st else ()):
        assert st[k] == 0, (what, k, st)
    if "pwp_max_abs" in st:
        assert st["pwp_max_abs"] == 0.0 and st["pw_max_abs"] == 0.0, (what, st)


def _list_pairs(hf):
    lens = np.diff(hf["tile_offsets"].astype(np.int64))
    tile = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    return set(zip(tile.tolist(), hf["point_list"].astype(np.int64).tolist()))


def _assert_ranks(G, rec, hf, cull, owner=None):
    """The ranks of a (batch, tile) run -- the rects of up to four tiles and the ranked 5..16-tile rects together -- are a
    permutation of 0 .. count - 1; 0xffff exactly where the device's lists do not hold the instance (cull off: nowhere)."""
    b, t, r, g = G.ranked_instances(rec, owner)
    pairs = _list_pairs(hf)
    kept = r != 0xffff
    in_list = np.array([(int(tt), int(gg)) in pairs for tt, gg in zip(t, g)], bool)
    assert (kept == in_list).all(), np.nonzero(kept != in_list)[0][:8]
    if not cull:
        assert kept.all()
    key = b[kept] * rec["tiles"] + t[kept]
    order = np.lexsort((r[kept], key))
    key, rk = key[order], r[kept][order]
    start = np.r_[0, np.nonzero(np.diff(key))[0] + 1]
    first = np.repeat(start, np.diff(np.r_[start, len(key)]))
    assert (rk == np.arange(len(key)) - first).all()


def _assert_path(G, case, decl, hf, cull, what):
    """The device's record against the declaration (full views)."""
    rec = G.binning_record(hf)
    B, cap = decl["batch"], RC.mid_cap(decl["batch"])
    assert rec["batch"] == B and rec["sparse"] == 0, (what, rec["batch"], B)
    live = np.array([d["i"] for d in decl["live"]])
    filler = np.ones(case.N, bool)
    filler[live] = False
    assert not rec["has_rect"][filler].any(), what                       # fr.y == ~0 for every filler
    assert rec["has_rect"][live].all(), what
    got = np.stack([rec["x0"][live], rec["y0"][live], rec["w"][live], rec["h"][live]], 1).tolist()
    assert got == [list(d["rect"]) for d in decl["live"]], what          # the rect bits
    for d in decl["live"]:
        i, cls = d["i"], d["cls"]
        assert bool(rec["big"][i]) == (cls != "small"), (what, d)        # bit 30
        if cls != "mid":
            assert bool(rec["ranked_mid"][i]) == (cls == "mid-ranked"), (what, d)      # bit 31
    rowed = np.nonzero(rec["ranked_mid"])[0]
    per_batch = np.bincount(rowed // B, minlength=rec["batches"])
    assert {b: int(n) for b, n in enumerate(per_batch) if n} == decl["rows"], (what, per_batch)
    for b in decl["rows"]:
        idx = rec["fill"][rowed[rowed // B == b], 3]
        assert len(np.unique(idx)) == len(idx) and idx.max() < cap, (what, b)          # distinct rows, inside the batch's
    for i in rowed:                                                       # a row's first nt entries are ranks or 0xffff
        row = rec["rows"][(i // B) * cap + int(rec["fill"][i, 3])][:int(rec["w"][i] * rec["h"][i])]
        assert ((row < B) | (row == 0xffff)).all(), (what, i, row)
    _assert_ranks(G, rec, hf, cull)
    assert rec["flagged"] == decl["flagged"], (what, rec["flagged"], decl["flagged"])
    assert rec["huge"] == (1 if decl["flagged"] else 0), what
    return rec


class _knobs:
    """The case's knobs plus a leg's, back to the defaults on exit."""

    def __init__(self, *dicts):
        self.kv = {k: v for d in dicts for k, v in d.items()}

    def __enter__(self):
        from log_amd import tune
        tune.reset_knobs()
        for k, v in self.kv.items():
            tune.set_knob(k, v)

    def __exit__(self, *exc):
        from log_amd import tune
        tune.reset_knobs()


def _decl_for(case, knobs):
    return case.declaration(defer_tiles=knobs.get("LOGRAST_DEFER_TILES", RC.COOP_TILES), mid_rank=knobs.get("LOGRAST_MID_RANK", 1))


def _run_both_culls(oracle_mod, case, sc, cam, flavour=None, cov3d=None, what=""):
    """Cull off: the oracle's lists entry for entry, I = n_rect.  Cull on: the same image bits, I <= n_rect.  Both: the
    declared path.  -> (hf with the cull on, its oracle forward, the view)."""
    import gpu_util as G
    from log_amd import rasterizer as R
    flavour = R.WODILATE if flavour is None else flavour
    decl = case.declaration()
    if cov3d is None:
        v, of = G.oracle_forward(oracle_mod, cam, sc, BG, flavour=flavour)
    else:
        v = oracle_mod.make_view(case.W, case.H, *cam_tan(cam), cam["world_view_transform"],
                                 cam["full_proj_transform"], BG, filter_mode=flavour.filter_mode, ndc_cull=flavour.ndc_cull)
        of = oracle_mod.forward(v, sc["xyz"], None, None, sc["opacity"], sc["colors"], cov3d=cov3d, extras=bool(flavour.extras))
        of["_view"] = v
    assert of["I"] == decl["n_rect"]
    run = lambda: G.hip_forward(cam, sc, BG, flavour=flavour, scratch_floats=16, cov3d=cov3d)
    prev = R.set_tile_cull(False)
    try:
        with _knobs(case.knobs):
            off = run()
            n_rect = R.last_state_info()[3]
            again = run()
        assert off["I"] == of["I"] == n_rect == decl["n_rect"], (what, off["I"], of["I"], n_rect)
        assert (off["point_list"] == of["point_list"]).all() and (off["tile_offsets"] == of["tile_offsets"]).all(), what
        assert (off["point_list"] == again["point_list"]).all(), what          # run to run
        _assert_exact(G, off, of, what + " cull off")
        _assert_path(G, case, decl, off, False, what + " cull off")
        R.set_tile_cull(True)
        with _knobs(case.knobs):
            on = run()
            n_rect = R.last_state_info()[3]
            again = run()
        assert on["I"] <= n_rect == decl["n_rect"], (what, on["I"], n_rect)
        assert (on["point_list"] == again["point_list"]).all(), what
        _assert_exact(G, on, of, what + " cull on")
        assert (on["image"].view(np.uint32) == off["image"].view(np.uint32)).all(), what
        _assert_path(G, case, decl, on, True, what + " cull on")
    finally:
        R.set_tile_cull(prev)
    return on, of, v


@pytest.mark.parametrize("case", FULL_CASES, ids=lambda c: c.id)
def test_rects_on_a_boundary(oracle_mod, case):
    import gpu_util as G
    from test_gpu_list_boundaries import _assert_gradients
    cam, sc = case.scene()
    hf, of, v = _run_both_culls(oracle_mod, case, sc, cam, what=case.id)
    if case.backward:
        # the chain rule and the reverse walk both take N and these lists
        dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
        og, g64 = oracle_mod.backward(v, of, dL), oracle_mod.backward_f64(v, of, dL, cond=False)
        g = G.hip_backward(hf, dL, bwd_form=hf["fwd_form"])
        fig = {k: rel_l2(g[k], og[k].reshape(g[k].shape)) for k in g if k in og}
        print("RECTCASE %s %s" % (case.id, {k: "%.3e" % e for k, e in fig.items()}))
        for k, e in fig.items():
            assert e < GRAD_TOL, (k, e)
        _assert_gradients(case.id, g, og, g64)


@pytest.mark.parametrize("case", [c for c in FULL_CASES if c.legs], ids=lambda c: c.id)
def test_knob_legs_give_the_same_bits(case):
    """Every knob leg of the case: the bits of the default run, and the path the leg's knobs declare."""
    import gpu_util as G
    cam, sc = case.scene()
    with _knobs(case.knobs):
        ref = G.hip_forward(cam, sc, BG, scratch_floats=16)
    _assert_path(G, case, case.declaration(), ref, True, case.id)
    for leg in case.legs:
        what = "%s %s" % (case.id, leg)
        with _knobs(case.knobs, leg):
            hf = G.hip_forward(cam, sc, BG, scratch_floats=16)
        _same_bits(hf, ref, what)
        assert (hf["rec"].view(np.uint32) == ref["rec"].view(np.uint32))[ref["radii"] > 0].all(), what
        _assert_path(G, case, _decl_for(case, leg), hf, True, what)


@pytest.mark.parametrize("case", [c for c in FULL_CASES if c.cov3d], ids=lambda c: c.id)
def test_cov3d_precomp(oracle_mod, case):
    """lr_project_batched_kernel<true> is an instantiation of its own: the same rects from the [N, 6] covariances."""
    cam, sc = case.scene()
    _run_both_culls(oracle_mod, case, sc, cam, cov3d=RC.cov3d_of(sc), what=case.id + " cov3d")


@pytest.mark.parametrize("case", [c for c in FULL_CASES if c.flavours], ids=lambda c: c.id)
def test_upstream_flavour(oracle_mod, case):
    """The other package's flavour (dilating low-pass, no ndc cull, no per-pixel maps) on the class cases."""
    from log_amd import rasterizer as R
    cam, sc = case.scene(RC.FILTER_DILATE)
    _run_both_culls(oracle_mod, case, sc, cam, flavour=R.UPSTREAM, what=case.id + " upstream")


def _assert_band_path(G, case, decl, hf, cull, what):
    rec = G.binning_record(hf)
    B, span = decl["batch"], decl["span"]
    assert (rec["batch"], rec["sparse"], rec["span"]) == (B, 1, span), (what, rec["batch"], rec["sparse"], rec["span"])
    groups = (case.N + span - 1) // span
    want = np.zeros(groups, np.int64)
    for (wg, wave), n in decl["share"].items():
        want[wg] += n
    assert rec["survcount"][:groups].tolist() == want.tolist(), what
    by_i = {d["i"]: d for d in decl["live"]}
    for wg in range(groups):
        slots = np.arange(wg * span, wg * span + want[wg])
        assert rec["has_rect"][slots].all(), what
        owners = rec["survivor"][slots].astype(np.int64)
        mine = sorted(d["i"] for d in decl["live"] if d["survivor"] and d["i"] // span == wg)
        assert sorted(owners.tolist()) == mine, what
        if decl["slots"].get(wg) is not None:
            assert owners.tolist() == decl["slots"][wg], what             # one wave: ring order
        for s, i in zip(slots, owners):
            d = by_i[int(i)]
            assert (rec["x0"][s], rec["y0"][s], rec["w"][s], rec["h"][s]) == d["rect"], (what, d)
            assert bool(rec["big"][s]) == (d["cls"] != "small") and not rec["ranked_mid"][s], (what, d)
    owner = np.where(rec["has_rect"], rec["survivor"].astype(np.int64), 0)
    _assert_ranks(G, rec, hf, cull, owner=owner)
    assert rec["flagged"] == decl["flagged"], (what, rec["flagged"], decl["flagged"])
    assert rec["huge"] == (1 if decl["flagged"] else 0), what


@pytest.mark.parametrize("case", RC.BAND_CASES, ids=lambda c: c.id)
def test_band_ring(oracle_mod, case):
    """lr_project_band_kernel: the declared survivors per workgroup in the declared slots, their classes, the slot chunks of
    the deferred ones; cull on and off against oracle.forward(tile_rows=...); LOGRAST_BAND_SPARSE = 0 gives the same bits."""
    import gpu_util as G
    from log_amd import rasterizer as R
    cam, sc = case.scene()
    decl = case.band_declaration()
    v, of = G.oracle_forward(oracle_mod, cam, sc, BG, tile_rows=case.band)
    assert of["I"] == decl["n_rect"]
    res = {}
    prev = R.set_tile_cull(False)
    try:
        for cull in (False, True):
            R.set_tile_cull(cull)
            what = "%s cull %d" % (case.id, cull)
            with _knobs(case.knobs), R.tile_rows(*case.band):
                hf = G.hip_forward(cam, sc, BG, scratch_floats=16)
                n_rect = R.last_state_info()[3]
                again = G.hip_forward(cam, sc, BG, scratch_floats=16)
            assert n_rect == decl["n_rect"] and (hf["I"] == of["I"] if not cull else hf["I"] <= n_rect), (what, hf["I"], n_rect)
            assert (hf["point_list"] == again["point_list"]).all(), what
            if not cull:
                assert (hf["point_list"] == of["point_list"]).all(), what
            _assert_exact(G, hf, of, what)
            _assert_band_path(G, case, decl, hf, cull, what)
            res[cull] = hf
        assert (res[True]["image"].view(np.uint32) == res[False]["image"].view(np.uint32)).all()
        for leg in case.legs:
            with _knobs(case.knobs, leg), R.tile_rows(*case.band):
                hf = G.hip_forward(cam, sc, BG, scratch_floats=16)
            _same_bits(hf, res[True], "%s %s" % (case.id, leg))
            assert G.binning_record(hf)["sparse"] == 0
    finally:
        R.set_tile_cull(prev)

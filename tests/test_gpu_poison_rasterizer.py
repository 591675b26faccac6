"""The rasterizer's small scenarios (the parity, list, band and edge cases of the existing GPU tests, through tests/gpu_util.py)
rerun with every buffer the Python layer hands the library filled first: tests/poison.py.  No result may depend on what an
uninitialised buffer held.

Each scenario runs once unpoisoned and once under each of the four fills; the oracle is computed once per (scene, flavour).
  * Deterministic outputs -- radii, tile offsets, the finished point lists, n_contrib, the fork's id map, image, final_T, the
    fork's weight maps, the records of the visible Gaussians -- are bit-identical across the five runs and equal the oracle's
    by the base tests' own rule (gpu_util.compare_forward: no mismatch).
  * The gradients are sums of float atomics: every element finite under every fill; rows the oracle leaves at zero exactly 0.0;
    against the unpoisoned run the reverse walk's outputs within ORDER_TOL, the chain rule's within CHAIN_TOL (both the suite's
    own constants for "same sums, other order": a stale 1e30 or NaN is far outside either).
  * Only what include/lograst.h declares unspecified is left out: EXEMPT below.
Every poisoned call must have made hooked allocations, and the carved parts a forward / backward works in must be among them."""
import contextlib

import numpy as np
import pytest
import torch

import list_cases as LC
import poison as P
import rect_cases as RC
from test_gpu_parity import _case as parity_case
from util import rel_l2, small_case

pytestmark = pytest.mark.gpu

ORDER_TOL = 1e-5      # two device evaluations of the same sums, order of the additions only (tests/test_gpu_aux_channels.py)
CHAIN_TOL = 1e-4      # the same behind the chain rule (tests/test_gpu_parity.py: test_hit_masks_hand_over)
BG = (0.3, 0.6, 0.9)
WALK = ("means2D", "conic", "opacities", "colors")
CHAIN = ("means3D", "scales", "rotations")
EXACT = ("radii_mismatch", "rec_bits_mismatch", "offsets_mismatch", "list_mismatch", "n_contrib_mismatch",
         "image_bits_mismatch", "final_T_bits_mismatch")

# What the comparisons leave out, each with the sentence of include/lograst.h that declares it unspecified -- nothing else is.
EXEMPT = [
    dict(region="bwd_rows after a backward (the dL/dconic introspection of rows with point_weight == 0 in the touched-only regime "
                "included: compared where point_weight > 0)",
         header="whatever the caller finds in bwd_rows after lograst_backward is unspecified",
         how="gpu_util.hip_backward zeroes conic where point_weight == 0; no other slot of the rows is read"),
    dict(region="geom records of Gaussians with radii == 0",
         header="Records of Gaussians with radii == 0 are undefined: a view that owns a band of tile rows does not write them",
         how="records are compared on the rows the oracle's radii make visible"),
    dict(region="point_list tails of lazily ordered lists before lograst_finish_lists",
         header="those entries are unspecified until lograst_finish_lists has run",
         how="gpu_util.hip_forward finishes the lists before it returns them; the ordered prefix is checked to stay as it was"),
    dict(region="the outputs of an overflowed call",
         header="the outputs of such a call are undefined",
         how="no forward here overflows; the failed speculative attempt of tests/test_gpu_poison_packages.py is repeated"),
    dict(region="child rows of a LOGRAST_MOVE_SKIP key after lograst_densify_move_rows",
         header="Rows d >= num_keep of a LOGRAST_MOVE_SKIP key are not written here: they are unspecified until the kernel that "
                "owns the children has run",
         how="tests/test_gpu_poison_modules.py: test_densify_move_rows compares such a key below num_keep; the recorded densify "
             "round compares the children once lograst_densify_split_uniform has written them"),
    dict(region="a packed segment of the row-sparse exchange: the order of its rows, and its value rows and index words "
                "behind the rows it holds",
         header="Value rows and index words j >= min(count, kmax) of a segment are unspecified: nothing reads them",
         how="tests/test_gpu_poison_modules.py: canonical_segments compares the header's count and the held rows sorted by their "
             "index (the header: `those rows, in no particular order`); everything the unpack writes is compared in full"),
    dict(region="k-NN output for fewer than four points",
         header="p < 4: a point has fewer than three other points and out[i] is unspecified",
         how="the k-NN scenarios of tests/test_gpu_poison_modules.py have 257 and 1025 points"),
]

FWD_PARTS = {"geom", "state", "final_T", "n_contrib"}
BWD_PARTS = {"rot", "means3D", "scales", "colors", "opac"}


class Scenario:
    """One forward (+ backwards) through gpu_util.  scene: () -> (cam, sc); path "plain" / "training" (scratch_floats = 16);
    fwd_form None / "rows" / "quadrant"; hit_masks None (the default: on) / False; bwd: the reverse-walk forms of the backwards
    over the one forward, in order ("same" / "other" relative to the forward's, None = the package's choice); knobs; band =
    (first, end) tile rows; ints: poison.poisoned's (0 where the scenario has fewer than two rows or pixels)."""

    def __init__(self, id, scene, flavour="wodilate", path="training", fwd_form=None, hit_masks=None, bwd=("same",), knobs=None,
                 band=None, ints=None, ref_key=None):
        self.id, self.scene, self.flavour, self.path, self.fwd_form, self.hit_masks = id, scene, flavour, path, fwd_form, hit_masks
        self.bwd, self.knobs, self.band, self.ints = tuple(bwd), dict(knobs or {}), band, ints
        self.ref_key = (ref_key or id, flavour, band)


def _scenarios():
    out = []
    for name in ("tiny", "ragged", "big_splats", "mid_rects", "dense_tile", "flat_depth_3000"):
        sc = (lambda n: (lambda: parity_case(n)))(name)
        for fl in ("wodilate", "upstream"):
            kw = dict(flavour=fl, ref_key=name)
            out.append(Scenario("%s-%s-plain" % (name, fl), sc, path="plain", bwd=(None,), **kw))
            # a training forward in each compositing form; its masked reverse walk, then a second backward in the other form
            out.append(Scenario("%s-%s-training-rows" % (name, fl), sc, fwd_form="rows", bwd=("same", "other"), **kw))
            out.append(Scenario("%s-%s-training-quadrant" % (name, fl), sc, fwd_form="quadrant", bwd=("same", "other"), **kw))
    for name in ("ragged", "big_splats"):
        sc = (lambda n: (lambda: parity_case(n)))(name)
        for form in ("rows", "quadrant"):
            out.append(Scenario("%s-no-masks-%s" % (name, form), sc, fwd_form=form, hit_masks=False, bwd=("same",), ref_key=name))
    # LOGRAST_HELPER_MIN_N below the 2000 Gaussians: the touched-only regime of the 5-tuple flavour, the large-input clears
    ragged = lambda: parity_case("ragged")
    for min_n in (1000, 0):
        for fl in ("wodilate", "upstream"):
            out.append(Scenario("ragged-%s-min_n-%d" % (fl, min_n), ragged, flavour=fl, bwd=("same", "other"),
                                knobs={"LOGRAST_HELPER_MIN_N": min_n}, ref_key="ragged"))
    for cid in ("spread-63", "spread-64", "spread-65", "spread-4097", "spread-8193", "spread-8193-closed"):
        out.append(Scenario("list-" + cid, (lambda c: (lambda: LC.BY_ID[c].scene()[:2]))(cid)))
    out.append(Scenario("adjacent-tiles", lambda: LC.adjacent_tiles(LC.ADJACENT[1])[:2], fwd_form="rows"))
    out.append(Scenario("ragged-band", ragged, band=(2, 5), ref_key="ragged"))
    band = RC.BY_ID["band-partial-tail"]
    out.append(Scenario("rect-" + band.id, band.scene, band=tuple(band.band), knobs=band.knobs))
    for W, H in ((1, 1), (15, 17), (33, 5)):
        out.append(Scenario("image-%dx%d" % (W, H), (lambda w, h: (lambda: _tiny_image(w, h)))(W, H), path="plain", bwd=(None,),
                            ints=0 if W * H < 2 else None))
    return out


def _tiny_image(W, H):
    from log_amd import scenes
    return scenes.orbit_cameras(1, W=W, H=H, focal=max(W, H) * 1.2)[0], scenes.random_scene(300, seed=25, opacity=None, smax=0.3)


SCENARIOS = _scenarios()


@contextlib.contextmanager
def _knobs(kv):
    from log_amd import tune
    tune.reset_knobs()
    for k, v in kv.items():
        tune.set_knob(k, v)
    try:
        yield
    finally:
        tune.reset_knobs()


def _flavour(name):
    from log_amd import rasterizer as R
    return {"wodilate": R.WODILATE, "upstream": R.UPSTREAM}[name]


_refs = {}


def _reference(oracle_mod, s, cam, sc):
    """The oracle's forward, dL/dimage and backward of a (scene, flavour, band): computed once, shared, left unchanged."""
    import gpu_util as G
    if s.ref_key not in _refs:
        v, of = G.oracle_forward(oracle_mod, cam, sc, BG, flavour=_flavour(s.flavour), tile_rows=s.band)
        dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
        _refs[s.ref_key] = (of, dL, oracle_mod.backward(v, of, dL))
    return _refs[s.ref_key]


FWD_BITS = ("image", "final_T", "point_weight_pixel", "point_weight")
FWD_INTS = ("radii", "tile_offsets", "point_list", "n_contrib", "point_id_pixel")


def _run(s, cam, sc, dL):
    import gpu_util as G
    from log_amd import rasterizer as R
    # (an unpinned forward takes its compositing form from the resolution's history: every run starts without one)
    R.capacity_stats(reset=True)
    with _knobs(s.knobs), (R.tile_rows(*s.band) if s.band else contextlib.nullcontext()):
        hf = G.hip_forward(cam, sc, BG, flavour=_flavour(s.flavour), scratch_floats=16 if s.path == "training" else 0,
                           fwd_form=s.fwd_form, hit_masks=s.hit_masks)
        grads = []
        for b in s.bwd:
            form = {None: None, "same": hf["fwd_form"], "other": "rows" if hf["fwd_form"] == "quadrant" else "quadrant"}[b]
            grads.append(G.hip_backward(hf, dL, bwd_form=form))
    return hf, grads


def _assert_forward(s, runs, of):
    import gpu_util as G
    base = runs[None][0]
    vis = of["radii"] > 0
    for fill, (hf, _) in runs.items():
        what = (s.id, fill)
        st = G.compare_forward(hf, of)                              # the base tests' rule, under every fill
        for k in EXACT + (("pid_mismatch",) if "pid_mismatch" in st else ()):
            assert st[k] == 0, (what, k, st)
        if "pwp_max_abs" in st:
            assert st["pwp_max_abs"] == 0.0 and st["pw_max_abs"] == 0.0, (what, st)
        for k in FWD_BITS:
            if k in base:
                assert np.array_equal(hf[k].view(np.uint32), base[k].view(np.uint32)), (what, k)
                assert np.isfinite(hf[k]).all(), (what, k)
        for k in FWD_INTS:
            if k in base:
                assert np.array_equal(hf[k], base[k]), (what, k)
        assert hf["I"] == base["I"] and hf["fwd_form"] == base["fwd_form"], what
        assert np.array_equal(hf["rec"][: len(vis)][vis].view(np.uint32), base["rec"][: len(vis)][vis].view(np.uint32)), what
        # (where a streamed list's first window ends depends on the arrival order of its keys -- the sort samples them --: the
        # base test, tests/test_gpu_list_boundaries.py, bounds it; which lists stay partly ordered does not)
        assert hf["lazy_lists"] == base["lazy_lists"], what
        assert np.array_equal(hf["ordered_len"] < np.diff(hf["tile_offsets"].astype(np.int64))[: len(hf["ordered_len"])],
                              base["ordered_len"] < np.diff(base["tile_offsets"].astype(np.int64))[: len(base["ordered_len"])]), what
        if hf["lazy_lists"]:
            print("ORDERED %s %s: %s" % (s.id, fill, hf["ordered_len"][hf["ordered_len"] > 4096].tolist()))


def _assert_gradients(s, runs, og):
    base = runs[None][1]
    for fill, (_, grads) in runs.items():
        for nth, (g, g0) in enumerate(zip(grads, base)):
            what = (s.id, fill, nth)
            assert g["bwd_form"] == g0["bwd_form"] and g["bwd_masks"] == g0["bwd_masks"], what
            for k in WALK + CHAIN:
                assert np.isfinite(g[k]).all(), (what, k, int((~np.isfinite(g[k])).sum()))
                dead = ~og[k].reshape(len(og[k]), -1).any(axis=1)
                assert not g[k].reshape(len(dead), -1)[dead].any(), (what, k)          # exactly 0.0 where the oracle's row is
                e = rel_l2(g[k], g0[k])
                assert e < (ORDER_TOL if k in WALK else CHAIN_TOL), (what, k, e)
            assert not g["means2D"][:, 2].any(), what


@pytest.mark.parametrize("s", SCENARIOS, ids=lambda s: s.id)
def test_scenario_under_every_fill(oracle_mod, s):
    cam, sc = s.scene()
    of, dL, og = _reference(oracle_mod, s, cam, sc)
    assert of["I"] > 0
    want = FWD_PARTS | ({"bwd_scratch"} if s.path == "training" else set()) | BWD_PARTS
    runs, parts = P.run_fills(lambda: _run(s, cam, sc, dL), ints=s.ints, sync=torch.cuda.synchronize, parts=want)
    for fill, census in parts.items():
        assert census.part_dtypes()["final_T"] == "float32" and census.part_dtypes()["n_contrib"] == "int32"
    print("CENSUS %s: %s; fills %s" % (s.id, parts["nan"].summary(), ", ".join(P.FILLS)))
    if s.path == "training":
        base = runs[None][1]
        assert base[0]["bwd_masks"] == (s.hit_masks is not False), s.id
        if len(base) > 1:
            assert not base[1]["bwd_masks"] and base[1]["bwd_form"] != base[0]["bwd_form"], s.id
    _assert_forward(s, runs, of)
    _assert_gradients(s, runs, og)
    assert any(np.abs(runs[None][1][0][k]).sum() > 0 for k in WALK), s.id


def test_lazily_ordered_scenarios_really_leave_a_tail():
    """The closed 8193 list stays ordered up to its first window (the tail is the exempt region), the open one parks and resumes."""
    import gpu_util as G
    for cid, lazy in (("spread-8193-closed", 1), ("spread-8193", 0)):
        cam, sc = LC.BY_ID[cid].scene()[:2]
        with P.poisoned("huge"):
            hf = G.hip_forward(cam, sc, BG, scratch_floats=16)
        assert hf["lazy_lists"] == lazy and hf["lazy_prefix_mismatch"] == 0 and hf["walk_beyond_ordered"] == 0, cid
        assert (hf["open_words"][LC.MAIN_TILE] != 0) == (lazy == 0), cid


@pytest.mark.parametrize("kind", ["empty", "all_culled"])
def test_nothing_to_draw(oracle_mod, kind):
    """N = 0 and a view that culls every Gaussian: the image is the background's bits, every map is defined, every gradient 0."""
    import gpu_util as G
    cam, sc = small_case(n=150, W=48, H=40, seed=0)
    if kind == "empty":
        sc = {k: v[:0] for k, v in sc.items()}
    else:
        sc = dict(sc, xyz=(sc["xyz"] + 3.0 * cam["camera_center"][None]).astype(np.float32))    # behind the camera
    bg = (0.1, 0.2, 0.3)
    H, W = cam["image_height"], cam["image_width"]
    want = np.broadcast_to(np.asarray(bg, np.float32)[:, None, None], (3, H, W))
    for fill in (None,) + P.FILLS:
        # (no row at all: 1 is no valid index -- integers are filled with 0)
        ctx = P.poisoned(fill, ints=0 if kind == "empty" else None) if fill else contextlib.nullcontext()
        with ctx as census:
            hf = G.hip_forward(cam, sc, bg, scratch_floats=16)
            # (the base test, test_gpu_parity.py: test_empty_and_all_culled, differentiates the culled view only)
            hg = G.hip_backward(hf, np.ones((3, H, W), np.float32)) if kind == "all_culled" else {}
        if fill:
            assert FWD_PARTS <= census.parts(), (kind, fill, census.parts())
        what = (kind, fill)
        assert hf["I"] == 0 and not hf["radii"].any() and not hf["tile_offsets"].any(), what
        assert np.array_equal(hf["image"].view(np.uint32), want.view(np.uint32)), what
        assert not hf["n_contrib"].any() and (hf["point_id_pixel"] == -1).all(), what
        assert (hf["final_T"] == 1.0).all() and not hf["point_weight_pixel"].any() and not hf["point_weight"].any(), what
        for k, g in hg.items():
            assert g.shape[0] == len(sc["xyz"]) and not g.any() and np.isfinite(g).all(), (what, k)

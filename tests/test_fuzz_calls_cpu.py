"""The draws behind the fixed slice of `tools/fuzz_parity.py --mode calls` (tests/test_gpu_fuzz.py::test_random_calls), held
without a GPU: what the forty seeds cover, the camera pre-pass's cap on every camera seed, and that draw_case still draws what
it drew (three seeds of the older slice, pinned as literals)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# the drawn knobs and their defaults (include/lograst.h; a literal table: this file asserts on draws and needs no built library)
KNOB_DEFAULTS = {"LOGRAST_LAZY_SORT": 1, "LOGRAST_MID_RANK": 1, "LOGRAST_MID_COOP": 16, "LOGRAST_FILL_STAGED": 2,
                 "LOGRAST_BATCH_SLOTS": 256, "LOGRAST_DEFER_TILES": 16, "LOGRAST_PBWD_LIST": 1, "LOGRAST_HUGE_CHUNK": 256,
                 "LOGRAST_PROJECT_BLOCKS": 512}
PLANTS = ("dup", "zero_scale", "zero_opacity", "needle", "giant", "unnormalised")

PINNED = [
    dict(seed=100003, n=1, W=1631, H=33, focal=1838.3, radius=1.5, scene="random", opacity="uniform", degenerate=[],
         flavour="upstream", training=False, fwd_form="quadrant", bwd_form=None, hit_masks=True, use_filter=True,
         scale_modifier=0.5, bg=(0.59, 0.35, 0.78),
         knobs={"LOGRAST_MID_COOP": 16, "LOGRAST_PBWD_LIST": 1, "LOGRAST_PROJECT_BLOCKS": 64}),
    dict(seed=200005, n=283585, W=8, H=6, focal=17.4, radius=1.5, scene="random", opacity="mixed", degenerate=[],
         flavour="wodilate", training=True, fwd_form="quadrant", bwd_form=None, hit_masks=True, use_filter=True,
         scale_modifier=0.5, bg=(0.1, 0.98, 0.34),
         knobs={"LOGRAST_BATCH_SLOTS": 256, "LOGRAST_DEFER_TILES": 4, "LOGRAST_PBWD_LIST": 2, "LOGRAST_PROJECT_BLOCKS": 4096}),
    dict(seed=300239, n=670, W=1, H=11, focal=1.0, radius=1.5, scene="trained", opacity="uniform", degenerate=[],
         flavour="wodilate", training=True, fwd_form="rows", bwd_form="rows", hit_masks=True, use_filter=True,
         scale_modifier=1.0, bg=(0.17, 0.09, 0.13), knobs={"LOGRAST_MID_RANK": 1, "LOGRAST_BATCH_SLOTS": 1024}),
]


@pytest.fixture(scope="module")
def draws():
    import fuzz_parity as F
    from test_gpu_fuzz import CALL_SEEDS
    return {seed: F.draw_call(seed) for seeds in CALL_SEEDS.values() for seed in seeds}


def test_draw_case_draws_what_it_drew():
    import fuzz_parity as F
    from test_gpu_fuzz import SEEDS
    for want in PINNED:
        assert want["seed"] in SEEDS
        assert F.draw_case(want["seed"])[0] == want
    # and draw_call is draw_case plus a stream of its own: the case underneath is the same
    desc, cam, sc, opt = F.draw_case(100005)
    d2, cam2, sc2, opt2, call = F.draw_call(100005)
    assert opt2 == opt and all(d2[k] == v for k, v in desc.items()) and all(np.array_equal(sc[k], sc2[k]) for k in sc)
    assert call["kind"] in F.KINDS and call["capacity"] in F.CAPACITIES


def test_the_slice_is_forty_seeds_in_blocks_of_eight_by_kind(draws):
    import fuzz_parity as F
    from test_gpu_fuzz import CALL_SEEDS
    assert tuple(CALL_SEEDS) == F.KINDS and all(len(v) == 8 for v in CALL_SEEDS.values()) and len(draws) == 40
    for kind, seeds in CALL_SEEDS.items():
        assert {draws[s][4]["kind"] for s in seeds} == {kind}


def test_the_fixed_seeds_cover_every_kind_mode_and_edge(draws):
    import fuzz_parity as F
    ds = [d[0] for d in draws.values()]
    for kind in F.KINDS:                                   # every kind under both flavours and every capacity mode
        mine = [d for d in ds if d["kind"] == kind]
        assert {d["flavour"] for d in mine} == {"wodilate", "upstream"}, kind
        assert {d["capacity"] for d in mine} == set(F.CAPACITIES), kind
    assert {d["hit_masks"] for d in ds} == {True, False}
    assert {d["fwd_form"] for d in ds} == {None, "rows", "quadrant"} and {d["bwd_form"] for d in ds} == {None, "rows", "quadrant"}
    assert any(d["W"] < 16 and d["H"] < 16 for d in ds)
    assert {p for d in ds for p in d["degenerate"]} == set(PLANTS)
    assert {d["use_filter"] for d in ds} == {True, False} and {d["scale_modifier"] for d in ds} == {1.0, 0.5, 2.3}
    assert {d["sh_degree"] for d in ds if d["kind"] == "shs"} == {0, 1, 2, 3}
    assert any(d["mapped"] for d in ds)                    # a refused combination, mapped and recorded
    for knob, default in KNOB_DEFAULTS.items():
        assert any(d["knobs"].get(knob, default) != default for d in ds), knob


def test_a_guess_that_is_too_small_exists_for_every_kind(draws):
    """speculative_too_small is mapped to speculative on a view below the guess's floor (4096 instances, 256 entries): every
    kind has a seed of that mode whose rect-rule numbers are far above the floor."""
    import fuzz_parity as F
    for kind in F.KINDS:
        big = []
        for desc, cam, sc, opt, call in draws.values():
            if call["kind"] == kind and call["capacity"] == "speculative_too_small":
                instances, longest = F.rect_lists(cam, sc, opt["flavour"], call["use_filter"], opt["scale_modifier"])
                big.append(instances > 30000 or longest > 1000)
        assert any(big), kind


def test_a_lazily_ordered_long_fog_list_is_in_the_slice(draws):
    import fuzz_parity as F
    found = []
    for desc, cam, sc, opt, call in draws.values():
        if desc["opacity"] == "fog" and opt["knobs"].get("LOGRAST_LAZY_SORT", 1) != 0:
            found.append(F.rect_lists(cam, sc, opt["flavour"], call["use_filter"], opt["scale_modifier"])[1])
    assert found and max(found) > 4096 + 3584, found       # beyond the first window of a lazily ordered list (7680)


def test_instance_counts_stay_far_below_the_oracles_limit(draws):
    import fuzz_parity as F
    for desc, cam, sc, opt, call in draws.values():
        instances, _ = F.rect_lists(cam, sc, opt["flavour"], call["use_filter"], opt["scale_modifier"])
        assert instances <= F.MAX_INSTANCES // 20, (desc["seed"], instances)
        if call["kind"] == "second_pass":
            assert instances > 0, desc["seed"]             # (a view without instances cannot be recomposited)


def test_camera_prepass_cap_on_every_camera_seed(draws):
    """The float64 reference of the isolated chain rule takes the fp32 forward's decisions; rows where fp32 and float64 decide
    differently (or too close to call) get no upstream gradient on either side: at most 1 % of a case's live rows."""
    import fuzz_parity as F
    seen = 0
    for desc, cam, sc, opt, call in draws.values():
        if call["kind"] != "camera":
            continue
        pre = F.camera_prepass(cam, sc, opt["flavour"], opt["use_filter"], opt["scale_modifier"])
        assert pre["dropped"] <= F.CAMERA_DROP_CAP * pre["live"], (desc["seed"], pre["dropped"], pre["live"])
        assert pre["drop"].shape == (desc["n"],) and pre["drop"].dtype == bool
        seen += 1
    assert seen == 8


def test_prepass_drops_a_row_between_the_fp32_and_the_float64_limit():
    """A Gaussian whose t.x / t.z sits on the clamp limit: undecidable in fp32, so dropped; its neighbours well inside and well
    outside are kept."""
    import fuzz_parity as F
    from log_amd import scenes
    from util import cam_tan
    cam = scenes.orbit_cameras(1, W=64, H=64, focal=40.0, radius=2.5)[0]
    V = np.asarray(cam["world_view_transform"], np.float64)
    tfx, _ = cam_tan(cam)
    inv = np.linalg.inv(V)

    def world(tx_over_tz, tz=2.0):
        return (np.array([tx_over_tz * tz, 0.0, tz, 1.0]) @ inv)[:3]
    lim = 1.3 * tfx
    xyz = np.stack([world(0.5 * lim), world(lim), world(1.2 * lim)]).astype(np.float32)
    sc = dict(xyz=xyz, scaling=np.full((3, 3), 0.5, np.float32),      # (wide enough to reach the screen)
 rotation=np.tile(np.array([1, 0, 0, 0], np.float32), (3, 1)))
    pre = F.camera_prepass(cam, sc, "upstream", True, 1.0)          # (upstream: no |ndc| cull, the far row stays live)
    assert pre["decisions"]["live"].all()
    assert list(pre["drop"]) == [False, True, False]
    assert list(pre["decisions"]["cx"][[0, 2]]) == [False, True]


def test_the_twin_of_a_sum_adds_the_addends_units():
    """_sum_f64: two backwards whose fp32 evaluation errors point against each other (seed 700579's one row: 4.1e-5 and
    2.8e-5 of the row, 2.5e-5 left in the signed sum).  The unit gradient_anchor_stats builds for the sum must be the sum of
    the addends' units, whatever cancels: in the values (row 1) or in the evaluation errors (row 0)."""
    import fuzz_parity as F
    eps = F.EPS32
    keys = ("means3D", "scales", "rotations")

    def twin(g, dev, cond):
        g = np.asarray(g, np.float64)
        return dict({k: g.copy() for k in keys}, means2D=np.zeros((2, 3)), cond=np.full((2, 3), cond),
                    chain32={k: (g + np.asarray(dev, np.float64)).astype(np.float64) for k in keys})
    f1 = twin([[1.0, 0, 0], [1.0, 0, 0]], [[4.1e-5, 0, 0], [1e-7, 0, 0]], 10.0)
    f2 = twin([[0.7, 0, 0], [-0.999, 0, 0]], [[-2.8e-5, 0, 0], [1e-7, 0, 0]], 20.0)
    s = F._sum_f64([f1, f2])
    for j, k in enumerate(keys):
        assert np.allclose(s[k], f1[k] + f2[k])
        y = np.linalg.norm(s[k], axis=1)
        unit = eps * np.maximum(s["cond"][:, j], 1.0) * y + np.linalg.norm(s["chain32"][k] - s[k], axis=1)   # gpu_util's unit
        want = sum(eps * f["cond"][:, j] * np.linalg.norm(f[k], axis=1) + np.linalg.norm(f["chain32"][k] - f[k], axis=1)
                   for f in (f1, f2))
        assert np.allclose(unit, want, rtol=1e-9), (k, unit, want)
        assert unit[0] / y[0] > 500 * eps          # row 0 is NOT one fp32 can know to 3e-5 ...
        assert np.linalg.norm((f1["chain32"][k] + f2["chain32"][k] - s[k])[0]) / y[0] < 500 * eps   # ... though the signed sum says so
    zero = F._sum_f64([twin([[1.0, 0, 0], [0, 0, 0]], [[0, 0, 0]] * 2, 5.0), twin([[-1.0, 0, 0], [0, 0, 0]], [[0, 0, 0]] * 2, 5.0)])
    assert np.isfinite(zero["cond"]).all()         # rows that sum to zero carry no unit, and no inf

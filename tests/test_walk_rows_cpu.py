"""The row-by-row rule of the reverse walk's sums (tests/gpu_util.py: walk_row_stats / assert_walk_rows) on the CPU, with the
fp32 oracle standing in for the device:

* it ACCEPTS the two fp32 references -- the oracle itself and its restatement with the kernels' freedoms
  (oracle.backward_alt), each with two orders of the commits -- on every scene of tests/walk_rows_scenes.py, and the floor
  those ask for, times four, is within WALK_ROW_FLOOR, which is within the chain rule's ROW_FLOOR;
* it REJECTS every planted fault below -- among them the one the aggregate relative-L2 rule accepts, on record here.

No device result enters anything in this file."""
import math

import numpy as np
import pytest

import gpu_util as G
import list_cases as LC
import walk_rows_scenes as WS
from util import rel_l2

NINE = ("means2D", "conic", "opacities", "colors")


def _copy(g):
    return {k: np.array(a, copy=True) for k, a in g.items()}


def _rejected(faulted, ref, what):
    st = G.walk_row_stats(faulted, ref["og"], ref["g64"])
    print("%s: %d violations %s, worst excess %.1f units at %s" % (what, st["violations"], st["violations_by_slot"],
                                                                   st["worst_excess_units"], st.get("worst")))
    with pytest.raises(AssertionError):
        G.assert_walk_rows(st)
    assert st["violations"] > 0 and st["nonfinite"] == 0
    return st


def _aggregate_accepts(faulted, ref, keys):
    """The rule the suite had for the walk's outputs: rel_l2_hip <= max(1e-4, 1.25 rel_l2_oracle) over the whole array."""
    fig = {k: (rel_l2(faulted[k], ref["g64"][k].reshape(faulted[k].shape)), rel_l2(ref["og"][k], ref["g64"][k].reshape(ref["og"][k].shape)))
           for k in keys}
    return all(e <= max(1e-4, 1.25 * o) for e, o in fig.values()), fig


def _main_ids(of):
    offs = of["tile_offsets"].astype(np.int64)
    return of["point_list"][offs[LC.MAIN_TILE]:offs[LC.MAIN_TILE + 1]].astype(np.int64)


# ---- what must pass -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", WS.NAMES)
def test_both_references_are_accepted(oracle_mod, name):
    ref = WS.reference(oracle_mod, name)
    assert ref["g64"]["walk_unit"].shape == (ref["fwd"]["N"], 11)
    for dev in ("og", "og16", "alt", "alt16"):
        for anchor in ("og", "og16"):
            st = G.walk_row_stats(ref[dev], ref[anchor], ref["g64"])
            assert st["slots"] == 11
            G.assert_walk_rows(st)
    # the nine-slot form every ordinary backward goes through: the same rule without the two absolute sums
    nine = lambda g: {k: g[k] for k in NINE}
    st = G.walk_row_stats(nine(ref["alt"]), nine(ref["og"]), ref["g64"])
    assert st["slots"] == 9
    G.assert_walk_rows(st)


def test_floor_is_the_measured_one(oracle_mod):
    """WALK_ROW_FLOOR = the floor the two references ask for between them (both commit orders, all scenes), times 4, rounded up
    to a power of two -- and no more than the chain rule's ROW_FLOOR."""
    asked = {name: WS.floor_asked(G, WS.reference(oracle_mod, name)) for name in WS.NAMES}
    worst = max(asked, key=asked.get)
    print("floor asked: %.3f on %s; WALK_FLOOR_MEASURED %.3f, WALK_ROW_FLOOR %g" % (asked[worst], worst, G.WALK_FLOOR_MEASURED, G.WALK_ROW_FLOOR))
    assert G.WALK_ROW_FLOOR == 2.0 ** math.ceil(math.log2(4.0 * G.WALK_FLOOR_MEASURED))
    assert G.WALK_ROW_FLOOR <= G.ROW_FLOOR
    # (the 16-thread commit order differs from run to run: what is asked today stays within the rounding up to a power of two)
    assert 4.0 * asked[worst] <= G.WALK_ROW_FLOOR, asked[worst]


def test_units_do_not_move_the_twin(oracle_mod):
    """walk_unit is a separate output: with it, with the absolute sums' columns, with or without cond, the twin's gradients
    and the chain rule's cond / chain32 keep their bits (one thread: the twin's sums are then in one order)."""
    ref = WS.reference(oracle_mod, "small_case")
    before = oracle_mod.set_threads(1)
    try:
        a = oracle_mod.backward_f64(ref["view"], ref["fwd"], ref["dL"])
        b = oracle_mod.backward_f64(ref["view"], ref["fwd"], ref["dL"], cond=False)
        c = oracle_mod.backward_f64(ref["view"], ref["fwd"], ref["dL"], abs_sums=True)
    finally:
        oracle_mod.set_threads(before)
    assert a["walk_unit"].shape[1] == 9 and c["walk_unit"].shape[1] == 11 and "cond" not in b
    assert (a["walk_unit"] == b["walk_unit"]).all() and (a["walk_unit"] == c["walk_unit"][:, :9]).all()
    for k in ("means2D", "conic", "opacities", "colors", "means3D", "scales", "rotations"):
        assert (a[k] == b[k]).all() and (a[k] == c[k]).all(), k
    assert (a["cond"] == c["cond"]).all()
    for k in a["chain32"]:
        assert (a["chain32"][k].view(np.uint32) == c["chain32"][k].view(np.uint32)).all(), k
    assert (a["walk_unit"] >= 0).all() and np.isfinite(a["walk_unit"]).all()
    assert (a["walk_unit"][G.walk_matrix(a) != 0] > 0).all()          # a non-zero sum has a unit
    # the absolute sums dominate the signed ones, and share their unit
    assert (c["absgrad"] >= np.abs(c["means2D"][:, :2]) * (1 - 1e-12)).all()
    assert (c["walk_unit"][:, 9:] == c["walk_unit"][:, :2]).all()


# ---- what must fail -----------------------------------------------------------------------------------------------------

def test_last_list_entry_lost(oracle_mod):
    """The commit of the main list's LAST entry (deepest: T is smallest there) lost in all nine slots, on offc-4097: every one
    of the nine slots is a violation.  (On THIS scene the aggregate rule sees the dL/dmeans2D and dL/dconic part too, printed
    below: all 4097 rows weigh about the same by construction, so one of them is 1e-3 of the array.  Where it is blind --
    rows that are small next to the rest -- is the next test.)"""
    ref = WS.reference(oracle_mod, "offc-4097")
    last = int(_main_ids(ref["fwd"])[-1])
    bad = _copy(ref["og"])
    for k in NINE:
        assert np.any(ref["g64"][k][last])
        bad[k][last] = 0
    st = _rejected(bad, ref, "last list entry lost")
    assert st["violations"] == 9 and len(st["violations_by_slot"]) == 9
    ok, fig = _aggregate_accepts(bad, ref, ("means2D", "conic"))
    print("the aggregate rule on the same fault (rel L2 faulted, oracle):", {k: "%.2e %.2e" % v for k, v in fig.items()}, "accepts:", ok)


@pytest.mark.parametrize("name", ["small_case", "trained_like_scene", "random_scene"])
def test_deepest_row_lost_and_the_aggregate_rule_accepts_it(oracle_mod, name):
    """The gap, on record: the commits of the Gaussian that lies deepest in its lists (the smallest blending weight anywhere
    among those that contribute) lost in all nine slots.  The aggregate rule -- relative L2 over the whole array within
    max(1e-4, 1.25 x the oracle's) -- accepts that for all four outputs; the row rule rejects it."""
    ref = WS.reference(oracle_mod, name)
    pw = ref["fwd"]["point_weight"]
    r = G.walk_matrix(ref["g64"])
    whole = (r != 0).all(axis=1)                             # all nine sums live
    row = int(np.argmin(np.where(whole & (pw > 0), pw, np.inf)))
    assert whole[row]
    bad = _copy(ref["og"])
    for k in NINE:
        bad[k][row] = 0
    st = _rejected(bad, ref, "%s: deepest row %d (weight %.2e) lost" % (name, row, pw[row]))
    assert st["violations"] >= 9
    ok, fig = _aggregate_accepts(bad, ref, NINE)
    print("the aggregate rule on the same fault (rel L2 faulted, oracle):", {k: "%.2e %.2e" % v for k, v in fig.items()})
    assert ok, fig                                           # the old rule does not see it


def test_one_block_missing(oracle_mod):
    """One 4x4 block's contribution missing: the walk with dL zeroed in that block, against the twin of the full dL."""
    ref = WS.reference(oracle_mod, "small_case")
    H, W = ref["fwd"]["n_contrib"].shape
    nc = ref["fwd"]["n_contrib"]
    by, bx = max(((int(nc[y:y + 4, x:x + 4].sum()), y, x) for y in range(0, H - 3, 4) for x in range(0, W - 3, 4)))[1:]
    dL = ref["dL"].copy()
    dL[:, by:by + 4, bx:bx + 4] = 0
    _rejected(oracle_mod.backward(ref["view"], ref["fwd"], dL), ref, "block (%d, %d) missing" % (bx, by))


def test_last_contributor_of_one_pixel_dropped(oracle_mod):
    ref = WS.reference(oracle_mod, "small_case")
    nc = ref["fwd"]["n_contrib"]
    y, x = np.unravel_index(int(np.argmax(nc)), nc.shape)
    fwd = dict(ref["fwd"], n_contrib=nc.copy())
    fwd["n_contrib"][y, x] -= 1
    _rejected(oracle_mod.backward(ref["view"], fwd, ref["dL"]), ref, "n_contrib - 1 at pixel (%d, %d)" % (x, y))


@pytest.mark.parametrize("key, a, b", [("conic", 0, 2), ("colors", 0, 2)], ids=["conic-A-C", "colour-r-b"])
def test_slots_swapped_on_one_row(oracle_mod, key, a, b):
    ref = WS.reference(oracle_mod, "small_case")
    m = np.abs(ref["g64"][key])
    row = int(np.argmax(np.minimum(m[:, a], m[:, b]) * (np.abs(m[:, a] - m[:, b]) > 0.1 * np.maximum(m[:, a], m[:, b]))))
    bad = _copy(ref["og"])
    bad[key][row, [a, b]] = bad[key][row, [b, a]]
    st = _rejected(bad, ref, "%s columns %d and %d swapped on row %d" % (key, a, b, row))
    assert st["violations"] == 2


def test_neighbouring_entries_exchanged(oracle_mod):
    """The rows of two entries next to each other in a list take each other's sums."""
    ref = WS.reference(oracle_mod, "offc-4097")
    ids = _main_ids(ref["fwd"])
    i, j = int(ids[2048]), int(ids[2049])
    bad = _copy(ref["og"])
    for k in NINE:
        bad[k][[i, j]] = bad[k][[j, i]]
    _rejected(bad, ref, "rows %d and %d exchanged" % (i, j))


def test_three_digit_error_on_a_tenth(oracle_mod):
    """A relative error of 2^-10 on a tenth of the components the rule holds to three digits: every one of them whose bound is
    below the planted error is a violation."""
    ref = WS.reference(oracle_mod, "trained_like_scene")
    clean = G.walk_row_stats(ref["og"], ref["og"], ref["g64"])
    assert clean["held_3_digits"] > 0.5, clean
    unit = ref["g64"]["walk_unit"][:, :9]
    r, o = G.walk_matrix(ref["g64"]), G.walk_matrix(ref["og"])
    bound = 2.0 * np.abs(o - r) + G.WALK_ROW_FLOOR * G.EPS32 * unit
    held = (unit > 0) & (bound <= 1e-3 * np.abs(r))
    pick = held & (np.random.default_rng(0).random(held.shape) < 0.1)
    m = o * np.where(pick, 1.0 + 2.0 ** -10, 1.0)
    bad = dict(means2D=np.concatenate([m[:, 0:2], np.zeros((len(m), 1))], 1), conic=np.concatenate([m[:, 2:5], np.zeros((len(m), 1))], 1),
               opacities=m[:, 5:6], colors=m[:, 6:9])
    st = _rejected(bad, ref, "2^-10 on %d of %d held components" % (pick.sum(), held.sum()))
    # |planted - f64| >= 2^-10 |oracle| - |oracle - f64|: a violation wherever that exceeds the bound
    sure = pick & (2.0 ** -10 * np.abs(o) - np.abs(o - r) > bound)
    assert sure.sum() > 0.5 * pick.sum(), (int(sure.sum()), int(pick.sum()))
    assert st["violations"] >= sure.sum()
    assert st["violations"] <= pick.sum()                    # and nothing that was left alone


# ---- the device tests' scenes (tests/test_gpu_walk_rows.py), checked here through the oracle ------------------------------

def test_device_scenes_are_what_they_say(oracle_mod):
    import test_gpu_walk_rows as D
    cam, sc, v, of, dL, og, g64 = D._reference(oracle_mod, G, D.every_lane, D.BG)
    # every lane: each splat contributes at exactly one pixel, each pixel of the tile has exactly one contributor, nothing
    # outside the tile, and all nine sums of every row are live
    tile = (slice(16, 32), slice(16, 32))
    assert (of["point_weight"] > 0).all() and len(np.unique(of["point_id_pixel"][tile])) == 256
    outside = of["n_contrib"].copy()
    outside[tile] = 0
    assert not outside.any() and (of["n_contrib"][tile] > 0).all()
    assert (np.abs(of["final_T"][tile] - 1.0) < 0.006).all()                    # ONE faint contributor each
    assert (G.walk_matrix(g64) != 0).all()
    # pair parity: one list of 70, the stack of 64 is its first chunk, every stack is walked to its end
    cam, sc, v, of, dL, og, g64 = D._reference(oracle_mod, G, D.pair_parity, D.BG)
    offs = of["tile_offsets"].astype(np.int64)
    assert offs[5] - offs[4] == 70
    assert (of["point_list"][offs[4]:offs[4] + 64] < 64).all() and (of["point_weight"] > 0).all()
    pos = 64
    for bx, by, n in D.PAIR_STACKS[1:]:
        pos += n
        assert of["n_contrib"][by + 2, bx + 1] == pos, (bx, by, n)               # the pixel under the stack: to its last entry
    assert of["n_contrib"][30, 29] == 64
    # opaque stacks: the 0.99 clamp is reached in front of the veil and behind it
    cam, sc, v, of, dL, og, g64 = D._reference(oracle_mod, G, D.opaque_stacks, D.BG)
    ids, w = of["point_id_pixel"], of["point_weight_pixel"]
    front = np.isin(ids, np.nonzero(sc["xyz"][:70, 2] < 2.0)[0])
    behind = np.isin(ids, np.nonzero(sc["xyz"][:70, 2] > 2.0)[0])
    assert (w[front] >= 0.98).any() and (w[behind] > 0.5).any() and of["point_weight"][70] > 0
    g = g64["walk_unit"][:, 6] / np.maximum(np.abs(g64["colors"][:, 0]), 1e-300)
    assert np.nanmax(np.where(g64["colors"][:, 0] != 0, g, 0)) > 100.0           # the amplification is in the unit


@pytest.mark.parametrize("bg", [(0.3, 0.6, 0.9), (0.0, 0.0, 0.0)], ids=["bg", "bg0"])
def test_device_scenes_accept_both_references(oracle_mod, bg):
    import test_gpu_walk_rows as D
    for make in D.SCENES:
        cam, sc, v, of, dL, og, g64 = D._reference(oracle_mod, G, make, bg)
        alt = oracle_mod.backward_alt(v, of, dL, abs_sums=True)
        for dev in (og, alt):
            st = G.walk_row_stats(dev, og, g64)
            assert st["live"] > 0 and st["slots"] == 11
            G.assert_walk_rows(st, name=None)
        print(make.__name__, "alt: worst excess %.2f units, held to 3 digits %.3f" % (st["worst_excess_units"], st["held_3_digits"]))

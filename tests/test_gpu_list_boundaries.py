"""Tile lists ON the boundaries between the regimes of the per-tile sort (log_amd/csrc/sort.hip), the lazy first-window
protocol and the compositing walk (log_amd/csrc/blend.hip), instead of wherever a random scene lands:

  sort.hip    8/9 keys in a bucket (registers / whole-wave ranking), 32/33 (LR_BUCKET_MAX: second map or network), 1024/1025
              (256-thread / 1024-thread workgroup), 4096/4097 (LR_LONG_LIST: LDS-resident / streamed), 7680/7681 (one window /
              two: the first length with sorted[tile] < L), 8192/8193 (LR_SORT_BLOCK: the network's second block and its first
              global pass), 16384/16385/24577 (three and four blocks under P2 = 32768: the `l < L` guards are live);
  blend.hip   64-entry chunks, `ordered = s >= L ? s : s & ~63`, LR_MBUF_CHUNKS = 4096 entries between mask flushes, mask
              slot (offsets[tile] >> 6) + tile + chunk.

The scenes (tests/list_cases.py) have ONE list of exactly L keys with exact depth ties, beginning at list offset 37; what
sort path each takes is declared there and asserted on the CPU (tests/test_list_cases_cpu.py), and the device's own record
of it -- how far the first pass ordered the list, whether waves parked -- is asserted here.  Every case: lists, image,
final_T, n_contrib and the per-pixel maps bit for bit the oracle's; the reverse walk on the forward's hit masks within
GRAD_TOL of the oracle and no further from the float64 twin than the oracle is; two forwards give the same list."""
import json

import numpy as np
import pytest

import list_cases as LC
from util import rel_l2

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4   # relative L2 against the oracle (BASELINE.json)
BG = (0.3, 0.6, 0.9)
EXACT = ("radii_mismatch", "rec_bits_mismatch", "offsets_mismatch", "list_mismatch", "n_contrib_mismatch",
         "image_bits_mismatch", "final_T_bits_mismatch", "pid_mismatch")
WALK = ("means2D", "conic", "opacities", "colors")
T4 = LC.MAIN_TILE


def _assert_exact(G, hf, of, lens):
    assert hf["I"] == of["I"]                                   # (compare_forward's entry-for-entry branch)
    assert np.diff(hf["tile_offsets"].astype(np.int64)).tolist() == lens
    st = G.compare_forward(hf, of)
    for k in EXACT:
        assert st[k] == 0, (k, st)
    assert st["pwp_max_abs"] == 0.0 and st["pw_max_abs"] == 0.0, st


def _same_bits(a, b):
    for k in ("image", "final_T", "point_weight_pixel", "point_weight"):
        assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), k
    for k in ("radii", "tile_offsets", "point_list", "n_contrib", "point_id_pixel"):
        assert (a[k] == b[k]).all(), k


def _assert_gradients(name, g, og, g64):
    """Against the fp32 oracle: rel-L2 < GRAD_TOL.  Against the float64 twin: the rule of gpu_util.assert_gradients_anchored
    for the reverse walk's outputs -- within the tolerance, or no further from it than 1.25 x the fp32 oracle's own distance --
    and gpu_util.assert_walk_rows for every row and slot of them."""
    assert g["bwd_masks"]
    fig = {}
    for k in WALK:
        ref = g64[k].reshape(g[k].shape)
        fig[k] = (rel_l2(g[k], og[k]), rel_l2(g[k], ref), rel_l2(og[k], ref))
    print("LISTCASE " + json.dumps({"case": name, **{k: ["%.3e" % x for x in v] for k, v in fig.items()}}))
    for k, (e, e64, o64) in fig.items():
        assert e < GRAD_TOL, (k, e)
        assert e64 <= max(1e-4, 1.25 * o64), (k, e64, o64)
    # ... and row by row, slot by slot (gpu_util.walk_row_stats): an aggregate does not see one entry of 8193
    import gpu_util as G
    G.assert_walk_rows(G.walk_row_stats(g, og, g64), name="list_" + name)


def _reference(oracle_mod, G, cam, sc):
    v, of = G.oracle_forward(oracle_mod, cam, sc, BG)
    dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
    return of, dL, oracle_mod.backward(v, of, dL), oracle_mod.backward_f64(v, of, dL, cond=False)


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.id)
def test_list_on_a_boundary(oracle_mod, case):
    import gpu_util as G
    cam, sc, lens = case.scene()
    of, dL, og, g64 = _reference(oracle_mod, G, cam, sc)
    hf = G.hip_forward(cam, sc, BG, scratch_floats=16)
    again = G.hip_forward(cam, sc, BG, scratch_floats=16)
    assert (hf["point_list"] == again["point_list"]).all()      # run to run
    assert lens[T4] == case.L
    _assert_exact(G, hf, of, lens)
    nc = hf["n_contrib"][16:32, 16:32]
    assert (nc.max() == case.L) if case.open else (nc.max() < LC.N_FRONT)
    _assert_gradients(case.id, G.hip_backward(hf, dL, bwd_form=hf["fwd_form"]), og, g64)
    # which way the list went, by the device's own record
    L, first, opened = case.L, int(hf["first_window"][T4]), int(hf["open_words"][T4])
    print("%s: first window %d, ordered %d, open %#x, LR_HDR_OPEN %d" % (case.id, first, hf["ordered_len"][T4], opened, hf["hdr_open"]))
    assert not np.delete(hf["open_words"], T4).any()
    if L <= LC.LONG_WIN:                                        # one window (or no window at all): ordered to its end, nobody parks
        assert first == L and hf["ordered_len"][T4] == L and hf["lazy_lists"] == 0 and opened == 0 and hf["hdr_open"] == 0
    elif case.regime == "network":                              # the network orders the whole list in the first pass
        assert first == L and hf["ordered_len"][T4] == L and hf["lazy_lists"] == 0 and opened == 0 and hf["hdr_open"] == 0
    elif case.regime is not None and case.open:                 # the first pass stopped at its window, the open pixels asked for the rest
        assert LC.LONG_WIN - LC.BUCKET_MAX < first <= LC.LONG_WIN < L     # (windows end at a bucket's end: <= 32 keys short)
        assert opened != 0 and hf["hdr_open"] == 1 and hf["ordered_len"][T4] == L and hf["lazy_lists"] == 0
    elif case.regime is not None:                               # closed: nobody asked, the tail stays as the fill left it
        assert LC.LONG_WIN - LC.BUCKET_MAX < first <= LC.LONG_WIN < L
        assert opened == 0 and hf["hdr_open"] == 0 and hf["ordered_len"][T4] == first and hf["lazy_lists"] == 1


@pytest.mark.parametrize("form", ["rows", "quadrant"])
@pytest.mark.parametrize("L", LC.KNOB_LENGTHS)
def test_forms_and_knobs(oracle_mod, L, form):
    """Both compositing forms; LOGRAST_LAZY_SORT=0 gives the same bits; without the forward's hit masks the reverse walk finds
    the same visits itself."""
    import gpu_util as G
    from log_amd import tune
    case = LC.BY_ID["spread-%d" % L]
    cam, sc, lens = case.scene()
    of, dL, og, g64 = _reference(oracle_mod, G, cam, sc)
    hf = G.hip_forward(cam, sc, BG, scratch_floats=16, fwd_form=form)
    _assert_exact(G, hf, of, lens)
    assert hf["n_contrib"].max() == L
    g = G.hip_backward(hf, dL, bwd_form=form)
    _assert_gradients("%s-%s" % (case.id, form), g, og, g64)
    assert (int(hf["first_window"][T4]) < L) == (L > LC.LONG_WIN) == (hf["open_words"][T4] != 0)
    tune.set_knob("LOGRAST_LAZY_SORT", 0)
    try:
        hf0 = G.hip_forward(cam, sc, BG, scratch_floats=16, fwd_form=form)
        assert hf0["lazy_lists"] == 0 and hf0["first_window"][T4] == L and not hf0["open_words"].any()
        _same_bits(hf0, hf)
        g0 = G.hip_backward(hf0, dL, bwd_form=form)
    finally:
        tune.reset_knobs()
    hf1 = G.hip_forward(cam, sc, BG, scratch_floats=16, fwd_form=form, hit_masks=False)
    _same_bits(hf1, hf)
    g1 = G.hip_backward(hf1, dL, bwd_form=form)
    assert g0["bwd_masks"] and not g1["bwd_masks"]
    for k in WALK:
        assert rel_l2(g0[k], g[k]) < 1e-5, (k, rel_l2(g0[k], g[k]))
        assert rel_l2(g1[k], g[k]) < 1e-5, (k, rel_l2(g1[k], g[k]))


@pytest.mark.parametrize("lengths", LC.ADJACENT, ids=lambda l: "-".join(map(str, l)))
def test_adjacent_tiles(oracle_mod, lengths):
    """Six lists of chosen lengths one behind the other: their mask slots (offsets[tile] >> 6) + tile + chunk are neighbours,
    and a list may begin in the 64-entry chunk of the list buffer its predecessor ends in.  Every tile's last chunk, whole or
    partial, has the visits of the pixel that walked to the list's end."""
    import gpu_util as G
    from log_amd import rasterizer as R
    cam, sc, lens = LC.adjacent_tiles(lengths)
    of, dL, og, g64 = _reference(oracle_mod, G, cam, sc)
    prev_zero, R._zero_hit_masks = R._zero_hit_masks, True
    try:
        hf = G.hip_forward(cam, sc, BG, scratch_floats=16, fwd_form="rows")
        again = G.hip_forward(cam, sc, BG, scratch_floats=16, fwd_form="rows")
    finally:
        R._zero_hit_masks = prev_zero
    assert (hf["point_list"] == again["point_list"]).all()
    _assert_exact(G, hf, of, lens)
    vis = G.visits(hf)
    offs = hf["tile_offsets"].astype(np.int64)
    for t, n in enumerate(lens):
        x0, y0 = 16 * (t % LC.GX), 16 * (t // LC.GX)
        assert hf["n_contrib"][y0:y0 + 16, x0:x0 + 16].max() == n
        last_chunk = vis[offs[t] + ((n - 1) & ~63):offs[t + 1]]
        assert last_chunk.any(), (t, n)
        assert vis[offs[t + 1] - 1].any(), (t, n)               # the last entry itself: the pixel under it accumulated it
    _assert_gradients("adjacent-" + "-".join(map(str, lengths)), G.hip_backward(hf, dL, bwd_form="rows"), og, g64)
    for form in ("quadrant",):
        hq = G.hip_forward(cam, sc, BG, scratch_floats=16, fwd_form=form)
        _assert_exact(G, hq, of, lens)
        _assert_gradients("adjacent-%s-%s" % ("-".join(map(str, lengths)), form), G.hip_backward(hq, dL, bwd_form=form), og, g64)

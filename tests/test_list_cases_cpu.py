"""The scenes of tests/list_cases.py are what they declare -- through the oracle, without a device: exact list lengths,
exact depth ties, the (depth bits, id) order, a pixel that walks to the list's end, and the sort path sort.hip takes for
the list (tests/list_cases.py: regime_lds / regime_streamed).  tests/test_gpu_list_boundaries.py runs the same table on the
device; a regime it relies on is asserted here."""
import numpy as np
import pytest

import list_cases as LC
from util import oracle_view

BG = (0.3, 0.6, 0.9)
_CACHE = {}


def _forward(oracle_mod, key, make):
    if key not in _CACHE:
        cam, sc, lens = make()
        v = oracle_view(oracle_mod, cam, BG)
        of = oracle_mod.forward(v, sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["colors"])
        _CACHE[key] = (sc, lens, of)
    return _CACHE[key]


def _tile_pixels(a, tile):
    x0, y0 = 16 * (tile % LC.GX), 16 * (tile // LC.GX)
    return a[y0:y0 + 16, x0:x0 + 16]


def _main_depths(of, lens):
    """Depth bits of the main list's keys, in the oracle's list order."""
    offs = of["tile_offsets"].astype(np.int64)
    ids = of["point_list"][offs[LC.MAIN_TILE]:offs[LC.MAIN_TILE + 1]].astype(np.int64)
    return ids, of["rec"][ids, 9].view(np.uint32)


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.id)
def test_case_is_what_it_declares(oracle_mod, case):
    sc, lens, of = _forward(oracle_mod, case.id, case.scene)
    offs = of["tile_offsets"].astype(np.int64)
    assert np.diff(offs).tolist() == lens and lens[LC.MAIN_TILE] == case.L
    assert offs[LC.MAIN_TILE] == 37                                             # not 64-aligned
    vis = of["radii"] > 0
    assert vis.all()
    assert (of["rec"][:, 9].view(np.uint32) == sc["xyz"][:, 2].view(np.uint32)).all()    # view depth = z, bit for bit
    ids, zb = _main_depths(of, lens)
    # the list is the (depth bits, id) order of the Gaussians built for it (everything behind tile 0's own)
    nf = LC.N_FRONT if case.front else 0
    n0 = lens[0] - nf
    mine = np.arange(n0, len(sc["xyz"]))
    assert len(mine) == case.L
    want = mine[np.lexsort((mine, sc["xyz"][mine, 2].view(np.uint32)))]
    assert (ids == want).all()
    if case.tie is not None:
        assert np.unique(zb, return_counts=True)[1].max() == case.tie
    nc = _tile_pixels(of["n_contrib"], LC.MAIN_TILE)
    if case.open:
        assert nc.max() == case.L, nc.max()                                       # some pixel walks to the end
    else:
        # every pixel stops at once: the last front splat (alpha > 0.9 all over the tile) contributed to none of them, so each
        # was done when it met it (a pixel is done, without accumulating, at the entry that would take T below 1e-4)
        assert nc.max() < LC.N_FRONT and _tile_pixels(of["final_T"], LC.MAIN_TILE).max() < 0.011


@pytest.mark.parametrize("case", [c for c in LC.CASES if c.regime is not None], ids=lambda c: c.id)
def test_declared_regime(oracle_mod, case):
    sc, lens, of = _forward(oracle_mod, case.id, case.scene)
    ids, zb = _main_depths(of, lens)
    z = zb.view(np.float32)
    if case.L <= LC.LONG_LIST:
        got = LC.regime_lds(z)
        print(case.id, got)
        assert got[0] == case.regime, got
        if case.pattern == "tie32":
            assert got[1] == 32                                                   # a bucket of exactly LR_BUCKET_MAX keys
        return
    # streamed: the keys reach the oracle's binning in id order; the device's fill has an order of its own, so the declared
    # regime has to hold in id order and in any shuffle of it.  (Not in EVERY order: arriving sorted by depth, the pieces of
    # the sample miss the list's far end by L / npieces keys, which then share the last bucket -- the network.)
    ids = np.sort(ids)
    z = of["rec"][ids, 9]
    rng = np.random.default_rng(case.L)
    seen = [LC.regime_streamed(z)] + [LC.regime_streamed(z[rng.permutation(case.L)]) for _ in range(20)]
    print(case.id, sorted(set(seen), key=str))
    assert all(r[0] == case.regime for r in seen), seen
    if case.pattern.startswith("tie") and case.regime == "linear":
        assert all(r[1] == case.tie for r in seen), seen                          # the group is a bucket of its own, and the largest


@pytest.mark.parametrize("L", LC.OFFC_LENGTHS)
def test_off_centre_lists_have_live_mean_and_conic_sums(oracle_mod, L):
    """The `offc` family exists so that the long-list regimes exercise ALL nine sums of the reverse walk: at least 99 % of the
    main list's entries have a non-zero dL/dmeans2D and a non-zero dL/dconic row in the float64 twin (one tile, declared
    regime: test_case_is_what_it_declares / test_declared_regime above, through LC.CASES)."""
    case = LC.BY_ID["offc-%d" % L]
    assert case.regime == "linear" and case.open
    sc, lens, of = _forward(oracle_mod, case.id, case.scene)
    assert np.diff(of["tile_offsets"].astype(np.int64)).tolist() == lens      # each splat in ONE tile's list
    ids, _ = _main_depths(of, lens)
    cx, cy = of["rec"][ids, 0].astype(np.float64), of["rec"][ids, 1].astype(np.float64)
    ox, oy = LC.OFF_CENTRE
    tol = LC.OFF_JITTER + 1e-4                                                   # every centre off its pixel on both axes
    assert np.abs((cx - np.floor(cx)) - ox).max() < tol and np.abs((cy - np.floor(cy)) - (1.0 + oy)).max() < tol
    dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
    g64 = oracle_mod.backward_f64(oracle_view(oracle_mod, LC.camera(), BG), of, dL, cond=False)
    mean_live = (g64["means2D"][ids, :2] != 0).all(axis=1)
    conic_live = (g64["conic"][ids, :3] != 0).all(axis=1)
    print(case.id, "live mean rows %.4f, live conic rows %.4f" % (mean_live.mean(), conic_live.mean()))
    assert mean_live.mean() >= 0.99 and conic_live.mean() >= 0.99


def test_every_size_class_has_every_regime():
    have = {(c.size_class, c.regime) for c in LC.CASES if c.open}
    for cls in ("small", "lds", "streamed"):
        for regime in ("linear", "equalised", "network"):
            assert (cls, regime) in have, (cls, regime)
    assert {c.L for c in LC.CASES if c.pattern == "spread" and c.open} >= set(LC.LENGTHS)


def test_restatement_on_known_lists():
    """What the restatements say about lists whose path follows from sort.hip by hand."""
    rng = np.random.default_rng(0)
    for L in (1, 7, 8, 9, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 4095, 4096):
        r = LC.regime_lds(LC.depths(L, "spread", rng))
        assert r[0] == "linear" and r[1] <= 8, (L, r)
        r = LC.regime_lds(LC.depths(L, "flat", rng))                              # one bucket for all: range 0
        assert r[0] == ("linear" if L <= 32 else "network") and r[1] == L, (L, r)
        if L >= 64:
            assert LC.regime_lds(LC.depths(L, "tie32", rng))[:2] == ("linear", 32), L
            r = LC.regime_lds(LC.depths(L, "tie33", rng))
            assert r[0] == "network" and r[1] == 33 and r[2] == 33, (L, r)
        if L >= 1023:
            r = LC.regime_lds(LC.depths(L, "cells", rng))
            assert r[0] == "equalised" and r[1] > 32, (L, r)
    for L in (4097, 8193, 24577):
        assert LC.regime_streamed(LC.depths(L, "flat", rng)) == ("network", L, L)
        assert LC.regime_streamed(LC.depths(L, "spread", rng))[0] == "linear"


@pytest.mark.parametrize("lengths", LC.ADJACENT, ids=lambda l: "-".join(map(str, l)))
def test_adjacent_tiles(oracle_mod, lengths):
    sc, lens, of = _forward(oracle_mod, ("adjacent",) + tuple(lengths), lambda: LC.adjacent_tiles(lengths))
    offs = of["tile_offsets"].astype(np.int64)
    assert np.diff(offs).tolist() == list(lengths) == lens
    for t, n in enumerate(lengths):
        assert _tile_pixels(of["n_contrib"], t).max() == n                        # every tile's last entry is walked
    # mask slots (offsets[tile] >> 6) + tile + chunk: some tile begins in the chunk its neighbour's list ends in
    if lengths == LC.ADJACENT[1]:
        assert sum(1 for t, n in enumerate(lengths) if offs[t] % 64 + n % 64 > 64) >= 2

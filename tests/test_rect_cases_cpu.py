"""The scenes of tests/rect_cases.py are what they declare -- through the oracle, without a device: the rect words of every
live Gaussian, fillers without a rect, the class counts and flagged chunks that follow from the rects, the rect-rule
instance count, no list near the sort's 1024-key class, and the plan arithmetic.  tests/test_gpu_binning_boundaries.py runs
the same table on the device; a wrong scene is caught here."""
import numpy as np
import pytest

import rect_cases as RC
from util import oracle_view

BG = (0.3, 0.6, 0.9)
_CACHE = {}


def forward(oracle_mod, case, filter_mode=RC.FILTER_CLAMP, ndc_cull=1):
    key = (case.id, filter_mode)
    if key not in _CACHE:
        cam, sc = case.scene(filter_mode)
        v = oracle_view(oracle_mod, cam, BG, filter_mode=filter_mode, ndc_cull=ndc_cull)
        of = oracle_mod.forward(v, sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["colors"])
        if case.N > 100000:                                    # (the large cases: keep what the checks read)
            of = {k: of[k] for k in ("radii", "tile_offsets", "point_list", "I")} | {"rec": of["rec"][:, 9:12].copy()}
            of["_rec_cols"] = 9
        _CACHE.clear()
        _CACHE[key] = (sc, of)
    return _CACHE[key]


def rects_of(of, idx):
    c0 = 10 - of.get("_rec_cols", 0)
    r0, r1 = of["rec"][idx, c0].view(np.uint32), of["rec"][idx, c0 + 1].view(np.uint32)
    x0, y0, x1, y1 = r0 & 0xffff, r0 >> 16, r1 & 0xffff, r1 >> 16
    return np.stack([x0, y0, x1 - x0, y1 - y0], 1).astype(np.int64)


def check_declaration(case, of, decl):
    live = np.array([d["i"] for d in decl["live"]])
    assert (of["radii"][live] > 0).all()
    assert rects_of(of, live).tolist() == [list(d["rect"]) for d in decl["live"]]
    filler = np.ones(case.N, bool)
    filler[live] = False
    assert not of["radii"][filler].any()                                     # all fillers have radius 0
    assert of["I"] == decl["n_rect"] == sum(d["rect"][2] * d["rect"][3] for d in decl["live"])
    assert np.diff(of["tile_offsets"].astype(np.int64)).max() < 1024         # this test is not about the sort
    # depths distinct: the list order is unambiguous
    c9 = 9 - of.get("_rec_cols", 0)
    assert len(np.unique(of["rec"][live, c9].view(np.uint32))) == len(live)


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.id)
def test_case_is_what_it_declares(oracle_mod, case):
    sc, of = forward(oracle_mod, case)
    decl = case.declaration()
    check_declaration(case, of, decl)
    B = decl["batch"]
    for d in decl["live"]:                                                   # class, position: from the rect and the index
        nt = d["rect"][2] * d["rect"][3]
        assert d["nt"] == nt
        assert (d["cls"] == "small") == (nt <= RC.RANKED_TILES)
        assert (d["cls"] == "deferred") == (nt > RC.COOP_TILES)
        assert d["i"] == d["batch"] * B + d["chunk"] * 256 + (d["i"] % 256) and d["i"] % 64 == d["lane"]
        if d["partial"]:
            assert d["cls"] != "mid-ranked" and d["cls"] != "mid"
    mids = {}
    for d in decl["live"]:
        if d["cls"] in ("mid", "mid-ranked"):
            mids[d["batch"]] = mids.get(d["batch"], 0) + 1
    assert decl["rows"] == {b: min(n, B // 4) for b, n in mids.items()}
    assert decl["flagged"] == {(d["i"] // B, (d["i"] % B) // 256) for d in decl["live"] if d["nt"] > RC.COOP_TILES}


@pytest.mark.parametrize("case", [c for c in RC.CASES if c.flavours], ids=lambda c: c.id)
def test_upstream_flavour_has_the_same_rects(oracle_mod, case):
    """The other package's low-pass (+0.3 instead of max(., 0.3)) and no ndc cull: the scene is solved for it."""
    sc, of = forward(oracle_mod, case, RC.FILTER_DILATE, ndc_cull=0)
    check_declaration(case, of, case.declaration())


@pytest.mark.parametrize("case", [c for c in RC.CASES if c.cov3d], ids=lambda c: c.id)
def test_cov3d_form_has_the_same_rects(oracle_mod, case):
    cam, sc = case.scene()
    v = oracle_view(oracle_mod, cam, BG)
    of = oracle_mod.forward(v, sc["xyz"], None, None, sc["opacity"], sc["colors"], cov3d=RC.cov3d_of(sc))
    check_declaration(case, of, case.declaration())


@pytest.mark.parametrize("case", RC.BAND_CASES, ids=lambda c: c.id)
def test_band_case_is_what_it_declares(oracle_mod, case):
    """oracle.forward(tile_rows=...): the survivors are the declared ones, with the declared clipped rects, and every wave's
    share of every workgroup holds the declared number of them."""
    cam, sc = case.scene()
    v = oracle_view(oracle_mod, cam, BG)
    of = oracle_mod.forward(v, sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["colors"], tile_rows=case.band)
    decl = case.band_declaration()
    assert decl["batch"] == 4096 and decl["span"] == RC.BAND_SPAN
    surv = np.nonzero(of["radii"] > 0)[0]
    want = [d for d in decl["live"] if d["survivor"]]
    assert surv.tolist() == [d["i"] for d in want]
    assert rects_of(of, surv).tolist() == [list(d["rect"]) for d in want]
    assert any(not d["survivor"] for d in decl["live"])                      # a rect outside the band
    share = {}
    for i in surv:
        key = (int(i) // decl["span"], (int(i) % decl["span"]) % 1024 // 64)
        share[key] = share.get(key, 0) + 1
    assert share == decl["share"]
    assert of["I"] == decl["n_rect"] and np.diff(of["tile_offsets"].astype(np.int64)).max() < 1024
    for wg, slots in decl["slots"].items():
        if slots is not None:                                                # ring order = (step, lane) order = index order
            steps = [(i % decl["span"]) // 1024 * 64 + i % 64 for i in slots]
            assert steps == sorted(steps)


def test_band_ring_states():
    """What the ring of the declared wave holds after each step (the kernel: add the step's survivors, fire 64 when 64 or
    more are pending): the table reaches 63, 64, 65 and 127 pending, fires with exactly 64 and leaves 0, 1 and 63 behind."""
    pending, left = set(), set()
    for case in RC.BAND_CASES:
        decl = case.band_declaration()
        for wg, slots in decl["slots"].items():
            if not slots:
                continue
            per_step = np.bincount([(i % decl["span"]) // 1024 for i in slots], minlength=16)
            n = 0
            for c in per_step:
                n += int(c)
                pending.add(n)
                if n >= 64:
                    n -= 64
                    left.add(n)
    assert {0, 1, 63, 64, 65, 127} <= pending and max(pending) == 127 and {0, 1, 63} <= left
    assert {sum(c.band_declaration()["share"].get((0, 3), 0) for c in [k]) for k in RC.BAND_CASES} >= {0, 1, 63, 64, 127, 129}
    flagged = RC.BY_ID["band-300-two-slot-chunks"].band_declaration()["flagged"]
    assert flagged == {(0, 0), (0, 1)}


def test_knobs_move_the_classes():
    """LOGRAST_DEFER_TILES 4 / 100 and LOGRAST_MID_RANK 0 on the class scenes: the same rects, other classes."""
    for cid in ("classes-rows", "classes-columns", "classes-square"):
        case = RC.BY_ID[cid]
        d16, d4, d100 = case.declaration(), case.declaration(defer_tiles=4), case.declaration(defer_tiles=100)
        for a, b, c in zip(d16["live"], d4["live"], d100["live"]):
            nt = a["nt"]
            assert b["cls"] == ("small" if nt <= 4 else "deferred")
            assert c["cls"] == ("small" if nt <= 4 else "mid-ranked" if nt <= 16 else "mid-cursor" if nt <= 100 else "deferred")
        assert {d["cls"] for d in d16["live"]} == {"small", "mid-ranked", "deferred"}
        assert any(d["cls"] == "mid-cursor" for d in d100["live"]) and not d4["rows"]
        assert all(d["cls"] != "mid-ranked" for d in case.declaration(mid_rank=0)["live"])


def test_table_covers_the_boundaries():
    """Every boundary of the issue has a case on each side; the ids in RC.BOUNDARIES exist."""
    for name, ids in RC.BOUNDARIES.items():
        for i in ids:
            assert i in RC.BY_ID, (name, i)
    nts = {cid: sorted(d["nt"] for d in RC.BY_ID[cid].declaration()["live"]) for cid in ("classes-rows", "classes-columns", "classes-square")}
    for cid in ("classes-rows", "classes-columns"):
        assert {4, 5, 16, 17} <= set(nts[cid]) and max(nts[cid]) == 25               # 25 = the whole grid
    assert {1, 2, 3, 4, 5, 6, 9, 16, 25, 64, 65, 625} <= set(nts["classes-square"])
    sq = {d["rect"][2:] for d in RC.BY_ID["classes-square"].declaration()["live"]}
    assert {(1, 1), (2, 1), (1, 2), (3, 1), (1, 3), (4, 1), (1, 4), (2, 2)} <= sq     # every order of the ranked class
    # mid rects per wave
    for K in (1, 4, 5, 16, 17, 64):
        d = RC.BY_ID["mid-wave-%d" % K].declaration()
        assert sum(1 for x in d["live"] if x["wave"] == 1 and x["cls"] == "mid-ranked") == K
    # rank rows
    for K in (1023, 1024, 1025):
        d = RC.BY_ID["rank-rows-%d" % K].declaration()
        assert d["batch"] == 4096 and d["rows"] == {0: min(K, 1024), 1: 3}
        assert ({x["cls"] for x in d["live"] if x["batch"] == 0} == {"mid"}) == (K > 1024)
    # deferred rects per chunk
    assert RC.BY_ID["huge-8-in-chunk"].declaration()["direct"] == {(0, 1): True}
    assert RC.BY_ID["huge-9-in-chunk"].declaration()["direct"] == {(0, 1): False}
    assert RC.BY_ID["huge-batch-ends"].declaration()["flagged"] == {(0, 15), (1, 0)}
    d = RC.BY_ID["huge-chunks-31-32"].declaration()
    assert d["batch"] == 10240 and d["flagged"] == {(1, 31), (1, 32), (1, 39)}
    # array ends
    for N in (1, 63, 64, 65, 4095, 4096, 4097, 4160):
        d = RC.BY_ID["n-%d" % N].declaration()
        last = d["live"][0]
        assert last["i"] == N - 1 and last["partial"] == (N % 64 != 0)
        assert last["cls"] == ("mid-cursor" if N % 64 else "mid-ranked")
    d = RC.BY_ID["n-4097"].declaration()
    assert d["live"][0]["batch"] == 1 and d["rows"] == {}
    assert RC.BY_ID["n-4097-deferred"].declaration()["flagged"] == {(0, 0), (1, 0)}
    assert RC.BY_ID["n-4160"].declaration()["rows"] == {1: 1}
    # the plan
    assert RC.plan(4097, 400, 400) == (4096, 1, 2)
    d = RC.BY_ID["plan-batch-6144"].declaration()
    assert (d["batch"], d["planes"], d["staged_k"]) == (6144, 1, 2) and RC.plan(393216, 400, 400, 64, 3)[2] == 3
    assert {x["batch"] for x in d["live"]} == {0, 1, 63}
    d = RC.BY_ID["plan-two-planes"].declaration()
    assert (d["batch"], d["planes"]) == (18432, 2)
    assert {x["batch"] for x in d["live"]} == {0, 1, 2, 3}                            # both planes of workgroups 0 and 1

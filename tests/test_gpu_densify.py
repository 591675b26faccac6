"""The device densification (log_amd/densify.py -> log_amd/csrc/densify.hip) against the fixtures recorded from the
reference's own plumbing (tests/golden/densify_*.npz) and the numpy restatement tests/densify_ref.py (held to those fixtures
by tests/test_densify_cpu.py).  No test here reads the reference tree: the three drop-ins run on stand-in objects that carry
the attributes the reference's TensorTree / GaussianPoint / SparseOptimizer / Counter / Splitter carry.

Integers and every copied row must match bit for bit.  The children's xyz and raw scaling follow the criterion of the step
kernels (tests/test_gpu_fuzz_step.py):  |hip - ref64| <= 8 * (|ref32 - ref64| + 2^-24 * S)  per element, ref32 the fixture,
ref64 the restatement, S its condition scale (S_xyz = |xyz_parent| + sum of 0.5 * scale[axis], S_scaling = 1 + |raw|)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import densify_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = 2.0 ** -24
TREE_KEYS = ("node_index", "index_parent", "local_index", "depth", "tree")
_FIXTURES = {}


def fixture(name):
    if name not in _FIXTURES:
        _FIXTURES[name] = D.load_fixture(name)
    return _FIXTURES[name]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


class _Buffers:
    """A BufferDict stand-in (LoG/model/sparse_optimizer.py:95-119)."""

    def __init__(self, d):
        self.keys = list(d)
        for k, v in d.items():
            setattr(self, k, v)

    @property
    def device(self):
        return getattr(self, self.keys[0]).device

    def items(self):
        for k in self.keys:
            yield k, getattr(self, k)


class TensorTree:      # the class name appears in the drop-in's count print, as the reference's does
    def __init__(self, t, max_child, max_level):
        for k in TREE_KEYS:
            setattr(self, k, dev(t[k]))
        self.max_child, self.max_level, self.min_resolution_pixel = max_child, max_level, 3


class Splitter:
    def __init__(self, n):
        self.N, self.split_method, self.scaling_factor = n, "uniform", 0.7


def stand_ins(meta, r):
    """The round's BEFORE state on the device: (tree or None, splitter, gaussian, optimizer, counter)."""
    c = r["copied"]
    g = types.SimpleNamespace(
        keys=[k for k in D.MODEL_KEYS if k in ("xyz", "scaling") or k in c],
        activation=types.SimpleNamespace(scaling_activation=torch.exp, scaling_inverse_activation=torch.log,
                                         rotation_activation=torch.nn.functional.normalize))
    for k in g.keys:
        setattr(g, k, dev(r[k] if k in ("xyz", "scaling") else c[k]))
    opt = types.SimpleNamespace(state_keys=list(D.STATE_KEYS))
    for sk in D.STATE_KEYS:
        setattr(opt, sk, _Buffers({k: dev(c[f"{sk}.{k}"]) for k in g.keys}))
    opt.steps = _Buffers({k: torch.zeros(r["p"], dtype=torch.int32, device=DEV) for k in g.keys})
    counter = types.SimpleNamespace(**{k: dev(c[k]) for k in D.COUNTER_KEYS})
    tree = TensorTree(r["tree_before"], meta["children"], meta["max_level"]) if meta["has_tree"] else None
    return tree, Splitter(meta["children"]), g, opt, counter


def densify(meta, r, tree, splitter, g, opt, counter, flags=None):
    """LoG.update_depth_stage's triple (level_of_gaussian.py:509-514) or update_init_stage's pair (:444-445) through the
    drop-ins; -> (masked split, masked remove, num_keep)."""
    from log_amd import densify as dd
    fs, fr = flags if flags is not None else (dev(r["flag_split"]), dev(r["flag_remove"]))
    remove_split = not meta["has_tree"]
    if tree is not None:
        fs, fr = dd.tree_split_and_remove(tree, fs, fr)
    nk = dd.split_and_remove(splitter, g, opt, fs, fr, remove_split=remove_split)
    dd.split_and_remove_other(splitter, counter, list(D.COUNTER_KEYS), fs, fr, remove_split=remove_split)
    return fs, fr, int(nk)


def check_tree(tree, r, where):
    for k in TREE_KEYS:
        got = getattr(tree, k).cpu().numpy()
        assert got.dtype == r["after_" + k].dtype and got.shape == r["after_" + k].shape, (where, k)
        assert np.array_equal(got, r["after_" + k]), (where, k, int((got != r["after_" + k]).sum()))


def check_children(meta, r, g, where):
    """-> the worst ratio of |hip - ref64| to the bound, for the record."""
    children, nk, ns = meta["children"], int(r["num_keep"]), int(r["num_split"])
    parents = r["src_row"][nk::children]
    r64 = D.split_uniform(r["xyz"][parents], r["scaling"][parents], r["copied"]["rotation"][parents], children)
    worst = 0.0
    for k in ("xyz", "scaling"):
        got = getattr(g, k)[nk:].cpu().numpy().astype(np.float64)
        assert got.shape == (ns * children, 3), (where, k)
        bound = 8.0 * (np.abs(r["child_" + k].astype(np.float64) - r64[k]) + ULP * r64["S_" + k])
        err = np.abs(got - r64[k])
        ratio = float((err / bound).max(initial=0.0))
        print(where, k, "worst |hip - ref64| / bound: %.3f" % ratio)
        assert np.isfinite(got).all() and (err <= bound).all(), (where, k, ratio)
        worst = max(worst, ratio)
    # the axis that each round halved, from the raw scales themselves: exact, tie rows included
    halved = np.rint((np.repeat(r["scaling"][parents].astype(np.float64), children, axis=0)
                      - getattr(g, "scaling")[nk:].cpu().numpy()) / np.log(2.0)).astype(np.int64)
    want = np.stack([(r64["axes"] == a).sum(axis=1) for a in range(3)], axis=1)
    assert np.array_equal(halved, np.repeat(want, children, axis=0)), (where, "axis choice")
    # ... and the ORDER of the rounds, from the centres: the children on the + side of round r minus those on its - side
    # are scale_r[axis_r] * R[:, axis_r] apart (the other rounds cancel), so the rotation column that carries the
    # difference names the axis of that round -- on the tie rows 0, then 1, then 2
    # (off-axis part: fp32 rounding of centres up to 2.1 in size, a few 2^-24 * 2.1 = 5e-7, against steps of at least
    # 0.01 * 0.25 = 2.5e-3: below 1e-3 of the step)
    rounds = r64["axes"].shape[1]
    if ns:
        kids = getattr(g, "xyz")[nk:].cpu().numpy().astype(np.float64).reshape(ns, children, 3)
        R = D.rotation_matrix(r["copied"]["rotation"][parents])
        side = (np.arange(children)[None, :] >> (rounds - 1 - np.arange(rounds)[:, None])) & 1          # [rounds, children]
        for rd in range(rounds):
            diff = kids[:, side[rd] == 1].mean(axis=1) - kids[:, side[rd] == 0].mean(axis=1)           # [ns, 3]
            along = np.abs(np.einsum("nij,ni->nj", R, diff))                                           # per rotation column
            assert np.array_equal(np.argmax(along, axis=1), r64["axes"][:, rd]), (where, "axis of round", rd)
            assert (np.sort(along, axis=1)[:, 1] <= 1e-3 * along.max(axis=1)).all(), (where, "off-axis offset", rd)
    return worst


@pytest.mark.parametrize("name", D.fixture_names())
def test_every_recorded_round_replays_on_the_device(name):
    meta, rounds = fixture(name)
    for i, r in enumerate(rounds):
        where = f"{name} round {i}"
        tree, splitter, g, opt, counter = stand_ins(meta, r)
        objects = {k: getattr(g, k) for k in g.keys}
        old_ptr = {k: v.data_ptr() for k, v in objects.items()}
        steps = {k: v.clone() for k, v in opt.steps.items()}
        fs, fr, nk = densify(meta, r, tree, splitter, g, opt, counter)
        src_row, num_new = r["src_row"], r["src_row"].shape[0]
        assert nk == int(r["num_keep"]), where
        assert fs.dtype == torch.bool and fr.dtype == torch.bool
        assert np.array_equal(fs.cpu().numpy(), r["masked_split"]) and np.array_equal(fr.cpu().numpy(), r["masked_remove"]), where
        if tree is not None:
            check_tree(tree, r, where)
        c = r["copied"]
        for k in g.keys:
            t = getattr(g, k)
            assert t is objects[k] and t.shape[0] == num_new and t.is_contiguous(), (where, k)      # identity kept
            assert num_new == 0 or r["p"] == 0 or t.data_ptr() != old_ptr[k], (where, k)                 # storage replaced
            before = r[k] if k in ("xyz", "scaling") else c[k]
            rows = slice(0, nk) if k in ("xyz", "scaling") else slice(None)
            assert np.array_equal(t.cpu().numpy()[rows], before[src_row][rows]), (where, k)
        for sk in D.STATE_KEYS:
            for k, v in getattr(opt, sk).items():
                assert np.array_equal(v.cpu().numpy(), D.move_rows(c[f"{sk}.{k}"], src_row, nk, D.ZERO)), (where, sk, k)
        for k, v in opt.steps.items():
            assert torch.equal(v, steps[k]), (where, "steps", k)            # not touched, as in the reference
        for k in D.COUNTER_KEYS:
            got = getattr(counter, k).cpu().numpy()
            assert got.dtype == r["after_" + k].dtype and np.array_equal(got, r["after_" + k]), (where, k)
        check_children(meta, r, g, where)


def test_parameter_keys_are_resized_in_place():
    """Model keys that are nn.Parameters (splitter.py:156-178 reads them through .data and calls set_ on the key itself):
    the Parameter object stays, requires grad, and holds the new rows like every other key."""
    meta, rounds = fixture("densify_init4")
    r = rounds[0]
    _, splitter, g, opt, counter = stand_ins(meta, r)
    params = {}
    for k in ("xyz", "opacity", "shs"):
        params[k] = torch.nn.Parameter(getattr(g, k))
        setattr(g, k, params[k])
    fs, fr, nk = densify(meta, r, None, splitter, g, opt, counter)
    src_row = r["src_row"]
    assert nk == int(r["num_keep"])
    for k in g.keys:
        t = getattr(g, k)
        assert t.shape[0] == src_row.shape[0], (k, tuple(t.shape))
        if k in params:
            assert t is params[k] and isinstance(t, torch.nn.Parameter) and t.requires_grad and t.is_leaf, k
        before = r[k] if k in ("xyz", "scaling") else r["copied"][k]
        rows = slice(0, nk) if k in ("xyz", "scaling") else slice(None)
        assert np.array_equal(t.detach().cpu().numpy()[rows], before[src_row][rows]), k
    assert opt.exp_avg.shs.shape == g.shs.shape and counter.create_steps.shape[0] == g.xyz.shape[0]
    check_children(meta, r, types.SimpleNamespace(xyz=g.xyz.detach(), scaling=g.scaling), "parameter keys")


@pytest.mark.parametrize("name", ["densify_tree2", "densify_tree4", "densify_tree8"])
def test_tree_rounds_chained_on_the_device(name):
    """Each round on the device's own output: integers stay exact through round 3 (float state is loaded per round, as the
    generator did; the children's xyz / scaling stay the device's own)."""
    meta, rounds = fixture(name)
    tree = splitter = g = opt = counter = None
    for i, r in enumerate(rounds):
        fresh = stand_ins(meta, r)
        if i == 0:
            tree, splitter, g, opt, counter = fresh
        else:
            assert g.xyz.shape[0] == r["p"]
            for k in D.COPIED_KEYS:                      # what the generator reloaded between rounds
                if k in g.keys:
                    getattr(g, k).set_(getattr(fresh[2], k))
            opt, counter = fresh[3], fresh[4]
        fs, fr, nk = densify(meta, r, tree, splitter, g, opt, counter)
        assert nk == int(r["num_keep"]) and np.array_equal(fs.cpu().numpy(), r["masked_split"])
        check_tree(tree, r, f"{name} chained round {i}")
        assert g.xyz.shape[0] == r["src_row"].shape[0] == counter.create_steps.shape[0]
        assert np.array_equal(counter.create_steps.cpu().numpy(), r["after_create_steps"])


def test_traverse_on_a_densified_tree_matches_the_oracle(oracle_mod):
    """log_amd.lod.traverse on the tree the device built (the depth hint is cached on depth.data_ptr(), which every
    densification replaces) against the oracle on the same arrays, before and after a round."""
    sys.path.append(os.path.join(HERE, "golden"))
    import make_golden_lod as G
    from log_amd import lod
    meta, rounds = fixture("densify_tree4")
    _, rast = G.camera_and_rasterizer(320, 240, 300.0, radius=6.0)
    rs = rast.raster_settings
    fx, fy = rs.image_width / (2 * rs.tanfovx), rs.image_height / (2 * rs.tanfovy)
    rast_dev = types.SimpleNamespace(raster_settings=rs._replace(
        bg=rs.bg.to(DEV), viewmatrix=rs.viewmatrix.to(DEV), projmatrix=rs.projmatrix.to(DEV), campos=rs.campos.to(DEV)))
    roots = np.arange(meta["n"], dtype=np.int64)
    tree, splitter, g, opt, counter = stand_ins(meta, rounds[0])
    tree.max_level = 30
    deepest = 0
    for i in range(2):
        r = rounds[i]
        if i:
            for k in D.COPIED_KEYS:
                getattr(g, k).set_(dev(r["copied"][k]))
            opt, counter = stand_ins(meta, r)[3:]
        densify(dict(meta, max_level=30), r, tree, splitter, g, opt, counter, flags=(dev(r["masked_split"]), dev(r["masked_remove"])))
        check_tree(tree, r, f"traverse round {i}")
        arrays = [x.cpu().numpy() for x in (tree.node_index, tree.tree, g.xyz, g.scaling, g.rotation)]
        for min_px in (0.5, 3.0):
            tree.min_resolution_pixel = min_px
            want = oracle_mod.lod_traverse(*arrays, roots, rs.projmatrix.numpy(), rs.viewmatrix.numpy(), fx, fy, rs.tanfovx,
                                           rs.tanfovy, min_px, tree.max_level, 1000)
            got = lod.traverse(tree, g, dev(roots), rast_dev, max_depth=1000).cpu().numpy()
            np.testing.assert_array_equal(got, want)
            deepest = max(deepest, int(tree.depth.cpu().numpy()[got].max()))
        assert tree._lograst_depth[0][0] == tree.depth.data_ptr() and tree._lograst_depth[1] == i + 1
    assert deepest == 2          # the selection reached the children of the second round


def test_one_host_synchronisation_per_call():
    """The smallest fixture through the drop-ins: each call reads back once (the plan's counts) and none falls back."""
    from log_amd import densify as dd
    meta, (r,) = fixture("densify_firstsplit")
    tree, splitter, g, opt, counter = stand_ins(meta, r)
    dd.reset_stats()
    fs, fr = dd.tree_split_and_remove(tree, dev(r["flag_split"]), dev(r["flag_remove"]))
    assert dd.stats() == {"calls": {"tree_split_and_remove": 1}, "fallbacks": {}, "readbacks": {"tree_split_and_remove": 1}}
    dd.reset_stats()
    nk = dd.split_and_remove(splitter, g, opt, fs, fr, remove_split=False)
    assert dd.stats() == {"calls": {"split_and_remove": 1}, "fallbacks": {}, "readbacks": {"split_and_remove": 1}}
    assert int(nk) == int(r["num_keep"]) and g.xyz.shape[0] == r["src_row"].shape[0]
    check_tree(tree, r, "firstsplit")


# ---- the row move alone ----------------------------------------------------------------------------------------------

def _plan(p, seed, children=4, remove_split=False, ps=0.05, pr=0.1):
    from log_amd import densify as dd
    rng = np.random.default_rng(seed)
    fr = rng.random(p) < pr
    fs = (rng.random(p) < ps) & ~fr
    plan = dd.Plan(dev(fs), dev(fr), remove_split, children)
    keep_dest, src_row, nk, ns, _ = D.plan(fs, fr, remove_split, children)
    assert (plan.num_keep, plan.num_split, plan.overlap) == (nk, ns, 0)
    assert np.array_equal(plan.keep_dest.cpu().numpy(), keep_dest) and np.array_equal(plan.src_row.cpu().numpy(), src_row)
    return rng, plan, src_row, nk


@pytest.mark.parametrize("p", [1, 255, 1024, 1025, 5000])
def test_move_rows_of_every_width_and_type(p):
    """f32 rows of 1, 3, 4, 9 and 45 columns (4 to 180 bytes; 4 columns and 16 x int32 take the 16-byte loads), int32, int16
    and int8 columns, every child mode, in 9 keys = two launches."""
    from log_amd import _lib
    rng, plan, src_row, nk = _plan(p, 100 + p)
    srcs = [rng.standard_normal((p, c)).astype(np.float32) for c in (1, 3, 4, 9, 45)]
    srcs += [rng.integers(-2 ** 31, 2 ** 31, (p, 16), dtype=np.int64).astype(np.int32),
             rng.integers(-2 ** 15, 2 ** 15, (p, 3)).astype(np.int16), rng.integers(-128, 128, p).astype(np.int8),
             rng.integers(-128, 128, (p, 5)).astype(np.int8)]
    modes = [D.COPY_PARENT, D.ZERO, D.COPY_PARENT, D.SKIP, D.COPY_PARENT, D.ZERO, D.COPY_PARENT, D.ZERO, D.SKIP]
    assert len(srcs) == 9 and (_lib.MOVE_COPY_PARENT, _lib.MOVE_ZERO, _lib.MOVE_SKIP) == (D.COPY_PARENT, D.ZERO, D.SKIP)
    outs = plan.move([(dev(s), m) for s, m in zip(srcs, modes)])
    for s, m, o in zip(srcs, modes, outs):
        got, want = o.cpu().numpy(), D.move_rows(s, src_row, nk, m)
        rows = slice(0, nk) if m == D.SKIP else slice(None)              # SKIP: the children belong to another kernel
        assert got.dtype == s.dtype and got.shape == want.shape and np.array_equal(got[rows], want[rows]), (s.shape, s.dtype, m)


def test_move_rows_leaves_skipped_children_alone_and_takes_strided_input():
    from log_amd import _lib
    from log_amd import rasterizer as R
    p = 3000
    rng, plan, src_row, nk = _plan(p, 7, children=2, ps=0.3)
    assert plan.num_new > nk
    wide = rng.standard_normal((p, 6)).astype(np.float32)
    strided = dev(wide)[:, ::2]                                           # not contiguous: made contiguous by move()
    assert not strided.is_contiguous()
    out, = plan.move([(strided, D.COPY_PARENT)])
    assert np.array_equal(out.cpu().numpy(), wide[:, ::2][src_row])
    # SKIP writes nothing behind row num_keep, not even the rest of the 16-byte word that holds the last kept row
    src = dev(rng.standard_normal((p, 3)).astype(np.float32))
    dst = torch.full((plan.num_new, 3), 7.0, device=DEV)
    key = (_lib.LograstMoveKey * 1)()
    key[0].src, key[0].dst, key[0].elem_size, key[0].columns, key[0].child_mode = src.data_ptr(), dst.data_ptr(), 4, 3, D.SKIP
    _lib.check(_lib.lib().lograst_densify_move_rows(nk, plan.num_new, p, R._ptr(plan.src_row), 1, key, R._stream_ptr(dst.device)))
    got = dst.cpu().numpy()
    assert np.array_equal(got[:nk], src.cpu().numpy()[src_row[:nk]]) and (got[nk:] == 7.0).all()


def test_scan_second_level():
    """P = 1024 * 1024 + 77: 1025 chunks of 1024 rows, the smallest size at which the chunk scan takes a second round."""
    p = 1024 * 1024 + 77
    rng, plan, src_row, nk = _plan(p, 11, children=8, remove_split=True, ps=0.02, pr=0.05)
    a = rng.integers(-128, 128, p).astype(np.int8)
    b = rng.standard_normal(p).astype(np.float32)
    oa, ob = plan.move([(dev(a), D.COPY_PARENT), (dev(b), D.ZERO)])
    assert np.array_equal(oa.cpu().numpy(), D.move_rows(a, src_row, nk)) and np.array_equal(ob.cpu().numpy(), D.move_rows(b, src_row, nk, D.ZERO))


def test_overlap_falls_back_and_counts():
    """Rows flagged for both while remove_split is off: the plan reports them and the drop-in refuses (the reference leaves
    the case undefined); with remove_split on they are simply split."""
    from log_amd import _dropin, densify as dd
    fs = np.zeros(2000, bool)
    fr = np.zeros(2000, bool)
    fs[[3, 1500]] = True
    fr[[3, 1999]] = True
    with pytest.raises(_dropin.Fallback, match="both split and remove"):
        dd.Plan(dev(fs), dev(fr), False, 2)
    plan = dd.Plan(dev(fs), dev(fr), True, 2)
    assert (plan.num_keep, plan.num_split, plan.overlap) == (1997, 2, 0)

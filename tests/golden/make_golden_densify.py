"""Generates tests/golden/densify_*.npz by RUNNING the reference's own densification plumbing on the CPU (build container
only: needs the reference checkout; the fixtures are committed and travel to the GPU box).

What is pinned: TensorTree.split_and_remove, Splitter.split_and_remove and Splitter.split_and_remove_other -- unmodified --
on the reference's LoG model (GaussianPoint, TensorTree, Counter, SparseOptimizer, Splitter), set up as
tests/test_log_plumbing_cpu.py::_log_model does, in the order of LoG.update_depth_stage (level_of_gaussian.py:509-514; the
init-stage case: :444-445).  Before every round the buffers are loaded from densify_ref.initial_geometry / copied_state,
so a fixture stores only: the packed flags, the reference's masked flags, the integer results, src_row (a row id carried
through colors[:, 0]), the children's xyz and raw scaling, and the reference's own fp32 error K against the float64
restatement.  Asserted here, on the CPU: every copied key of the reference equals before[src_row], the moments end in zeros,
the restatement reproduces the integers, and no parent has two different scales within 1e-6 of each other in any round.

    python tests/golden/make_golden_densify.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("LOG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (REF, ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import densify_ref as D                      # noqa: E402
from make_golden_lod import reference_env, save_lzma   # noqa: E402

TREE_KEYS = ("node_index", "index_parent", "local_index", "depth", "tree")
EPS = 2.0 ** -24


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def cpu_shims():
    """create_from_point calls distCUDA2(xyz.cuda()): `.cuda()` becomes the identity, the 3-NN distance comes from scipy."""
    from scipy.spatial import cKDTree

    def dist2(points):
        p = points.detach().cpu().numpy().astype(np.float64)
        d, _ = cKDTree(p).query(p, k=4)
        return torch.from_numpy((d[:, 1:] ** 2).mean(axis=1).astype(np.float32))
    mod = types.ModuleType("simple_knn._C")
    mod.distCUDA2 = dist2
    sys.modules["simple_knn._C"] = mod
    torch.Tensor.cuda = lambda self, *a, **k: self


def log_model(seed, n, max_child, max_level, sh_degree):
    from LoG.model.level_of_gaussian import LoG
    from log_amd import scenes
    sc = scenes.random_scene(max(n, 8), seed=seed, smax=0.08)
    cfg_opt = _Cfg(optimize_keys=["xyz", "colors", "scaling", "opacity", "rotation"] + (["shs"] if sh_degree else []),
                   opt_all_levels=True,
                   lr_dict={"xyz": 0.00016, "xyz_final": 0.0000016, "colors": 0.0025, "shs": 0.000125, "scaling": 0.005,
                            "opacity": 0.05, "rotation": 0.001, "max_steps": 300})
    model = LoG(gaussian=_Cfg(init_ply=dict(filename={"xyz": sc["xyz"], "colors": sc["colors"]}, scale3d=1.0,
                                            init_opacity=0.3), sh_degree=sh_degree, xyz_scale=1.0),
                tree=_Cfg(max_child=max_child, max_level=max_level), optimizer=cfg_opt, densify_and_remove=_Cfg())
    model.base_iter = 1
    model.set_stage("tree")
    return model


def load_state(model, xyz, scaling, copied):
    """The round's BEFORE state into the model's own buffers (set_, as the reference's methods do)."""
    g = model.gaussian
    p = xyz.shape[0]
    g.xyz.set_(torch.from_numpy(xyz.copy()))
    g.scaling.set_(torch.from_numpy(scaling.copy()))
    for k in D.COPIED_KEYS:
        if k in copied:
            getattr(g, k).set_(torch.from_numpy(copied[k].copy()))
    g.colors[:, 0] = torch.arange(p, dtype=torch.float32)          # the row id that becomes src_row
    for sk in D.STATE_KEYS:
        state = getattr(model.optimizer, sk)
        for k, val in state.items():
            val.set_(torch.from_numpy(copied[f"{sk}.{k}"].copy()))
    for k in D.COUNTER_KEYS:
        getattr(model.counter, k).set_(torch.from_numpy(copied[k].copy()))


def run_round(model, meta, i, xyz, scaling, tree_before, flag_split, flag_remove, worst):
    """One update_depth_stage triple (or the init-stage pair) of the reference; -> (round arrays, xyz, scaling after)."""
    seed, children, sh = meta["seed"], meta["children"], meta["sh_degree"]
    p = xyz.shape[0]
    assert p < 2 ** 24
    copied = D.copied_state(seed, i, p, sh)
    load_state(model, xyz, scaling, copied)
    before = {k: getattr(model.gaussian, k).numpy().copy() for k in D.MODEL_KEYS if hasattr(model.gaussian, k)}
    fs, fr = torch.from_numpy(flag_split), torch.from_numpy(flag_remove)
    out = {"flag_split": np.packbits(flag_split), "flag_remove": np.packbits(flag_remove)}
    if meta["has_tree"]:
        ms, mr = model.tree.split_and_remove(fs, fr)
        remove_split = False
    else:
        ms, mr = fs, fr
        remove_split = True
    num_keep = model.splitter.split_and_remove(model.gaussian, model.optimizer, ms, mr, remove_split=remove_split)
    model.splitter.split_and_remove_other(model.counter, list(D.COUNTER_KEYS), ms, mr, remove_split=remove_split)
    ms, mr = ms.numpy(), mr.numpy()
    out["masked_split"], out["masked_remove"] = np.packbits(ms), np.packbits(mr)
    num_keep = int(num_keep)
    after = {k: getattr(model.gaussian, k).numpy().copy() for k in before}
    src_row = after["colors"][:, 0].astype(np.int32)
    num_new = src_row.shape[0]
    # the restatement's plan is the reference's
    keep_dest, src_ref, nk, ns, overlap = D.plan(ms, mr, remove_split, children)
    assert overlap == 0 and nk == num_keep and np.array_equal(src_ref, src_row), "plan"
    assert num_new == nk + children * ns
    # every copied key equals before[src_row]; moments are cat(kept, zeros); the counter rule
    for k in D.COPIED_KEYS:
        if k in before:
            assert np.array_equal(after[k], before[k][src_row]), k
    for k in ("xyz", "scaling"):
        assert np.array_equal(after[k][:nk], before[k][src_row[:nk]]), k
    for sk in D.STATE_KEYS:
        for k, val in getattr(model.optimizer, sk).items():
            assert np.array_equal(val.numpy(), D.move_rows(copied[f"{sk}.{k}"], src_row, nk, D.ZERO)), (sk, k)
    for k in D.COUNTER_KEYS:
        got = getattr(model.counter, k).numpy()
        assert np.array_equal(got, D.counter_rule(k, copied[k], src_row, nk)), k
        out["after_" + k] = got.copy()
    if meta["has_tree"]:
        want = D.tree_update(tree_before, ms, mr, children)
        for k in TREE_KEYS:
            got = getattr(model.tree, k).numpy()
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
            out["after_" + k] = got.copy()
    # the children against the float64 restatement: the reference's own fp32 error in units of 2^-24 * S
    parents = src_row[nk::children]
    r64 = D.split_uniform(xyz[parents], scaling[parents], copied["rotation"][parents], children)
    if ns:
        if r64["min_gap"] < 1e-6:
            raise _Redraw(f"two scales of one parent within {r64['min_gap']:.2e}")
        for k in ("xyz", "scaling"):
            ratio = np.abs(after[k][nk:].astype(np.float64) - r64[k]) / (EPS * r64["S_" + k])
            worst[k] = max(worst[k], float(ratio.max()))
    out.update(num_keep=np.int64(nk), num_split=np.int64(ns), src_row=src_row, child_xyz=after["xyz"][nk:],
               child_scaling=after["scaling"][nk:])
    tree_after = {k: out["after_" + k] for k in TREE_KEYS} if meta["has_tree"] else None
    return out, after["xyz"], after["scaling"], tree_after


class _Redraw(Exception):
    pass


def tree_flags(rng, tree, rnd, plant):
    """Random flags as update_depth_stage could hand them over, plus rows the tree's masks must reject (parents, roots, the
    depth limit); never both flags on one row.  plant (round >= 1): one node loses ALL its children, another one some."""
    p = tree["node_index"].shape[0]
    leaf = tree["node_index"] == -1
    flag_remove = (rng.random(p) < (0.25 if rnd else 0.05))          # most hit roots / parents and are masked off
    flag_split = (rng.random(p) < 0.6 / tree["tree"].shape[1]) & ~flag_remove
    if plant and tree["tree"].shape[0] >= 2:
        full = np.nonzero((tree["tree"] >= 0).all(axis=1) & leaf[np.maximum(tree["tree"], 0)].all(axis=1))[0]
        assert full.size >= 2, "no two nodes with all children present and leaves"
        a, b = tree["tree"][full[0]], tree["tree"][full[-1]]
        flag_remove[a] = True
        flag_remove[b] = False
        flag_remove[b[0]] = True
        flag_split[a] = False
        flag_split[b] = False
    return flag_split, flag_remove


def tree_case(name, seed, children, n=5000, max_level=2, sh_degree=1, rounds=3):
    meta = dict(seed=seed, n=n, children=children, max_level=max_level, sh_degree=sh_degree, isotropic=0, has_tree=1,
                rounds=rounds)
    model = log_model(seed, n, children, max_level, sh_degree)
    xyz, scaling = D.initial_geometry(seed, n)
    load_geometry_and_setup(model, xyz, scaling, seed, sh_degree)
    model.upgrade_tree()
    tree = D.initial_tree(n, children)
    for k in TREE_KEYS:
        assert np.array_equal(getattr(model.tree, k).numpy(), tree[k]), k
    rng = np.random.default_rng([seed, 0xF1])
    arrays, worst = {}, {"xyz": 0.0, "scaling": 0.0}
    for i in range(rounds):
        fs, fr = tree_flags(rng, tree, i, plant=i >= 1)
        out, xyz, scaling, tree = run_round(model, meta, i, xyz, scaling, tree, fs, fr, worst)
        arrays.update({f"r{i}_{k}": v for k, v in out.items()})
        print(name, "round", i, "rows", fs.shape[0], "->", xyz.shape[0], "split", int(out["num_split"]),
              "nodes", tree["tree"].shape[0], "orphan rows", int((tree["tree"] < 0).all(axis=1).sum()))
    # the planted nodes: one lost all its children (its parent is a leaf again), one lost only some
    if rounds >= 2:
        lost = (tree["tree"] < 0).sum(axis=1)
        assert (lost == children).any() and ((lost > 0) & (lost < children)).any(), "plants"
    finish(name, meta, arrays, worst)


def load_geometry_and_setup(model, xyz, scaling, seed, sh_degree):
    """Resize the model's buffers to the case's rows before the optimizer and the counter take their sizes from them."""
    n = xyz.shape[0]
    copied = D.copied_state(seed, 0, n, sh_degree)
    g = model.gaussian
    g.xyz.set_(torch.from_numpy(xyz.copy()))
    g.scaling.set_(torch.from_numpy(scaling.copy()))
    for k in D.COPIED_KEYS:
        if k in copied:
            getattr(g, k).set_(torch.from_numpy(copied[k].copy()))
    from LoG.model.counter import Counter
    model.counter = Counter(num_points=n)
    model.training_setup()


def flat_case(name, seed, children, n, flags, sh_degree=1, isotropic=1):
    """No tree, remove_split=True: LoG.update_init_stage's pair (level_of_gaussian.py:444-445).  flags: a list of
    (flag_split, flag_remove) makers, one per round, called with (rng, p)."""
    meta = dict(seed=seed, n=n, children=children, max_level=0, sh_degree=sh_degree, isotropic=isotropic, has_tree=0,
                rounds=len(flags))
    model = log_model(seed, n, children, 20, sh_degree)
    xyz, scaling = D.initial_geometry(seed, n, bool(isotropic))
    load_geometry_and_setup(model, xyz, scaling, seed, sh_degree)
    rng = np.random.default_rng([seed, 0xF2])
    arrays, worst = {}, {"xyz": 0.0, "scaling": 0.0}
    for i, make in enumerate(flags):
        fs, fr = make(rng, xyz.shape[0])
        out, xyz, scaling, _ = run_round(model, meta, i, xyz, scaling, None, fs, fr, worst)
        arrays.update({f"r{i}_{k}": v for k, v in out.items()})
        print(name, "round", i, "rows", fs.shape[0], "->", xyz.shape[0], "split", int(out["num_split"]))
    finish(name, meta, arrays, worst)


def finish(name, meta, arrays, worst):
    meta = dict(meta, k_xyz=worst["xyz"], k_scaling=worst["scaling"])
    arrays.update({"meta_" + k: np.asarray(v) for k, v in meta.items()})
    path = os.path.join(HERE, f"densify_{name}.npz")
    save_lzma(path, arrays)
    print(f"{name}: K_xyz {worst['xyz']:.2f} K_scaling {worst['scaling']:.2f}  {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


def _rand(ps, pr):
    return lambda rng, p: (rng.random(p) < ps, rng.random(p) < pr)


def _none(rng, p):
    return np.zeros(p, bool), np.zeros(p, bool)


def _all_removed(rng, p):
    return np.zeros(p, bool), np.ones(p, bool)


def _all_split(rng, p):
    return np.ones(p, bool), np.zeros(p, bool)


def _ends(rng, p):
    fs, fr = np.zeros(p, bool), np.zeros(p, bool)
    fs[0] = fr[-1] = True
    return fs, fr


def _ends_swapped(rng, p):
    fs, fr = np.zeros(p, bool), np.zeros(p, bool)
    fr[0] = fs[-1] = True
    return fs, fr


def with_redraw(fn, name, seed, *args, **kw):
    for attempt in range(20):
        try:
            return fn(name, seed + 1000 * attempt, *args, **kw)
        except _Redraw as why:
            print(name, "seed", seed + 1000 * attempt, "redrawn:", why)
    raise SystemExit(f"{name}: no seed without near-equal scales")


def main():
    reference_env()
    cpu_shims()
    for children in (2, 4, 8):
        with_redraw(tree_case, f"tree{children}", 40 + children, children)
    # the init stage: isotropic scalings tie three ways, then two ways; flags may name a row for both (remove_split)
    with_redraw(flat_case, "init8", 51, 8, 3000, [_rand(0.2, 0.1), _rand(0.1, 0.3)])
    with_redraw(flat_case, "init4", 52, 4, 2500, [_rand(0.2, 0.1)], sh_degree=3, isotropic=0)
    # edges: nothing flagged, first / last row flagged (both ways), everything split, everything removed, then P = 0
    with_redraw(flat_case, "edges", 53, 2, 1100, [_none, _ends, _ends_swapped, _all_split, _all_removed, _none, _all_split])
    # an empty tree's first split, on a handful of points
    with_redraw(tree_case, "firstsplit", 54, 4, n=37, max_level=20, rounds=1)


if __name__ == "__main__":
    main()

"""numpy restatement of the decisions of LoG.update_depth_stage / update_init_stage (LoG/model/level_of_gaussian.py:400-427,
:454-508, :516-519): integers exact, statistics in float64.  Held to the reference by tests/golden/decide_*.npz
(tests/test_decide_cpu.py) and the yardstick of the device path (tests/test_gpu_decide.py).  Also what the fixture generator
(tests/golden/make_golden_decide.py) and the tests share: the counter inputs that are regenerated from a seed instead of
stored.

Every comparison is on stored values or on one correctly rounded fp32 division, which numpy's float32 reproduces bit for
bit -- except `weights_max < sigmoid(opacity) * 0.1` of the init stage, for which the generator keeps a margin (see there)
and the fixture carries the reference's activated values."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32
COUNTER_INPUTS = ("create_steps", "grad_sum", "area_sum", "radii_max_max", "weights_max", "visible_count", "radius3d_min",
                  "radius3d_max")
TREE_KEYS = ("node_index", "index_parent", "local_index", "depth", "tree")
DEPTH_CFG = dict(min_steps_split=100, split_grad_thres=0.0002, radius2d_thres=6, remove_weights_thres=0.005,
                 max_split_points=100, scaling_decay=0.9, sort_method="radii")
INIT_CFG = dict(init_split_method="split_by_2d", init_radius_min=4, init_radius_split=16, init_weight_min=0.1, min_steps=50,
                split_grad_thres=0.0002)


# ---- statistics ------------------------------------------------------------------------------------------------------

def stat64(x):
    """Counter.str_min_mean_max's numbers of an fp32 population, mean and unbiased std in float64."""
    x = np.asarray(x, f32)
    d = x.astype(np.float64)
    n = d.size
    return {"count": n, "min": f32(x.min()) if n else f32(np.inf), "max": f32(x.max()) if n else f32(-np.inf),
            "mean": float(d.mean()) if n else float("nan"), "std": float(d.std(ddof=1)) if n > 1 else float("nan"),
            "S": float(np.abs(d).max()) if n else 0.0}


def sigmoid64(raw):
    return 1.0 / (1.0 + np.exp(-np.asarray(raw, np.float64)))


def ratio64(raw_scaling):
    e = np.sort(np.exp(np.asarray(raw_scaling, np.float64)), axis=1)
    return e[:, 2] / e[:, 1]


def gradmean(c):
    """Counter.get_gradmean: one fp32 division."""
    return (c["grad_sum"].astype(f32) / np.maximum(c["area_sum"], 1).astype(f32)).astype(f32)


# ---- the depth stage -------------------------------------------------------------------------------------------------

def top_k_cut(cand, radii, k):
    """:496-499 -> (cut value, flag): the k-th largest radii among the candidates; rows whose fp32 radii reach it stay."""
    vals = np.sort(radii[cand].astype(np.int64))[::-1]
    cut = int(vals[k - 1])
    return cut, cand & (radii.astype(f32) >= f32(cut))


def depth_stage(node_index, depth, c, cfg, current_depth, max_level):
    """-> dict: flag_split (cut applied), flag_remove, candidates, counts, num_max_split, need_cut, cut_value, the depth
    histograms and the exact populations (grad, radii over is_parent; 'parent' = the mask for the activated ones)."""
    grad = gradmean(c)
    rmm = c["radii_max_max"]
    rmm_f = rmm.astype(f32)
    leaf = node_index == -1
    lt = depth < current_depth
    parent = leaf & lt
    sg = grad > f32(cfg["split_grad_thres"])
    sr = rmm_f > f32(cfg["radius2d_thres"])
    remove = leaf & (depth > 0) & (c["weights_max"] < f32(cfg["remove_weights_thres"])) & (c["visible_count"] > 1)
    cand = sg & sr & parent & (c["create_steps"] > cfg["min_steps_split"]) & ~remove
    k = min(int(f32(int(lt.sum())) * f32(0.05)), int(cfg["max_split_points"]))
    need = int(cand.sum()) > k
    split, cut = cand, None
    if need and k > 0:
        cut, split = top_k_cut(cand, rmm, k)
    bins = lambda m: np.bincount(depth[m].astype(np.int64) + 128, minlength=256)
    return {"flag_split": split, "flag_remove": remove, "candidates": cand, "parent": parent,
            "counts": {"split_grad": int(sg.sum()), "split_radii": int(sr.sum()), "candidates": int(cand.sum()),
                       "removed": int(remove.sum()), "depth_lt": int(lt.sum())},
            "num_max_split": max(k, 0), "need_cut": need, "cut_value": cut,
            "depth_all": bins(np.ones_like(leaf)), "depth_split": bins(split & (depth < max_level)), "depth_remove": bins(remove),
            "pop": {"grad": grad[parent], "radii": rmm_f[parent]}}


def depth_after(r, children):
    """Rows per depth after the resize, as the closing lines of update_depth_stage print them (bin = depth + 128)."""
    out = r["depth_all"].astype(np.int64) - r["depth_remove"]
    out[1:] += children * r["depth_split"][:-1]
    return out


def child_radius_max(raw_scaling, flag_split, children, decay):
    """:516-519 in float64: scaling_decay * max(exp(scaling)) of every split row, `children` times."""
    e = np.exp(np.asarray(raw_scaling, np.float64)[flag_split]).max(axis=1)
    return np.repeat(float(f32(decay)) * e, children)


# ---- the init stage --------------------------------------------------------------------------------------------------

def init_stage(opacity_act, c, rand, cfg, scale, children):
    """'split_by_2d' (:401-427); opacity_act: sigmoid(opacity) as fp32 (the fixture's, or the float64 one rounded)."""
    grad = gradmean(c)
    rmm_f = c["radii_max_max"].astype(f32)
    wmax = c["weights_max"]
    rw = wmax < f32(cfg["init_weight_min"])
    nonmax = wmax < np.asarray(opacity_act, f32) * f32(0.1)
    small = rmm_f < f32((cfg["init_radius_min"] * scale) ** 2)
    remove = (small & (rand > f32(0.5))) | rw | nonmax
    act = (c["create_steps"] > cfg["min_steps"]) & (rmm_f > 0)
    by_grad = (grad > f32(10 * cfg["split_grad_thres"])) & (rmm_f > f32(cfg["init_radius_min"] * scale * 8))
    by_radii = rmm_f > f32((cfg["init_radius_split"] * scale) ** 2)
    split = act & (by_radii | by_grad) & ~remove
    after_min = np.concatenate([c["radius3d_min"][~(remove | split)], np.repeat(c["radius3d_min"][split], children)])
    return {"flag_split": split, "flag_remove": remove,
            "counts": {"remove_weight": int(rw.sum()), "nonmax": int(nonmax.sum()), "remove_small": int(small.sum()),
                       "split_grad": int(by_grad.sum()), "split_radii": int(by_radii.sum())},
            "pop": {"radii_max_act": rmm_f[act], "grad": grad, "radii_split": rmm_f[split], "radius3d_min": after_min}}


def nonmax_margin_ulp(opacity_raw, weights_max):
    """The smallest distance, in fp32 ulp of the product, between weights_max and sigmoid(opacity) * 0.1."""
    prod = sigmoid64(opacity_raw) * float(f32(0.1))
    return float((np.abs(weights_max.astype(np.float64) - prod) / np.spacing(prod.astype(f32)).astype(np.float64)).min(initial=np.inf))


# ---- the inputs that are regenerated instead of stored ---------------------------------------------------------------

def counter_inputs(seed, rnd, p, depth=None, few=False, wide=False):
    """What a stretch of training leaves in the Counter, drawn from (seed, round): radii_max_max with many ties (pixel
    counts), area_sum with zeros, a tenth of the leaves below the removal threshold.  few: about 1 % of the rows pass the
    gradient threshold instead of a third; wide: radii over [0, 1600) and gradients up to 0.003 (the init stage's thresholds are 16 to 1024 pixels and 0.002)."""
    g = np.random.default_rng([seed, rnd, 0xDEC1])
    area = g.integers(0, 40, p).astype(np.int32) * (g.random(p) < 0.9)
    gmean = g.random(p) * (0.000202 if few else (0.003 if wide else 0.0006))
    out = {"opacity": g.standard_normal((p, 1)).astype(f32),
           "create_steps": g.integers(0, 400, p).astype(np.int32),
           "area_sum": area.astype(np.int32),
           "grad_sum": (gmean * np.maximum(area, 1)).astype(f32),
           "radii_max_max": (g.integers(0, 1600, p) if wide else np.minimum(g.geometric(0.04, p), 400)).astype(np.int32),
           "weights_max": np.where(g.random(p) < 0.1, g.random(p) * 0.005, g.random(p) * 0.9 + 0.005).astype(f32),
           "visible_count": g.integers(0, 6, p).astype(np.int16),
           "radius3d_min": (g.random(p) * 0.01 + 1e-4).astype(f32),
           "radius3d_max": (g.random(p) * 0.5 + 0.1).astype(f32)}
    return out


def initial_scaling(seed, n):
    g = np.random.default_rng([seed, 0xDEC2])
    return np.log(g.random((n, 3)) * 0.06 + 0.01).astype(f32)


# ---- fixtures --------------------------------------------------------------------------------------------------------

def fixture_names(kind=None):
    names = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("decide_") and f.endswith(".npz"))
    return [n for n in names if kind is None or n.startswith("decide_" + kind)]


def load_fixture(name):
    """-> (meta, [round dict]): every round with its inputs attached ('p', 'scaling', 'c' = counter_inputs of the round,
    'opacity', and for the depth stage 'tree_before')."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    rounds = []
    tree = None
    if meta["stage"] == "depth":
        import densify_ref as D
        tree = D.initial_tree(meta["n"], meta["children"])
    for i in range(meta["rounds"]):
        r = {k[len(f"r{i}_"):]: z[k] for k in z.files if k.startswith(f"r{i}_")}
        p = r["scaling"].shape[0]
        c = counter_inputs(meta["seed"], i, p, few=bool(meta["few"]), wide=meta["stage"] == "init")
        r.update(p=p, c=c, opacity=c["opacity"], tree_before=tree)
        for k in ("flag_split", "flag_remove"):
            r[k] = np.unpackbits(r[k])[:p].astype(bool)
        rounds.append(r)
        if tree is not None:
            tree = {k: r["after_" + k] for k in TREE_KEYS}
    return meta, rounds

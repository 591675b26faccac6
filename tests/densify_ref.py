"""numpy restatement of LoG's densification (LoG/model/tensor_tree.py:65-129, LoG/model/splitter.py:5-31, :95-220):
integers exact, floats in float64.  Held to the reference by tests/golden/densify_*.npz (tests/test_densify_cpu.py) and
the yardstick of the device path (tests/test_gpu_densify.py).  Also the helpers that the fixture generator
(tests/golden/make_golden_densify.py) and the tests share: the state that is regenerated from a seed instead of stored."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_KEYS = ("scaling", "colors", "xyz", "opacity", "rotation", "shs")   # GaussianPoint.keys (level_of_gaussian.py:156-159)
COPIED_KEYS = ("colors", "opacity", "rotation", "shs")                    # children copy the parent (splitter.py:168-173)
STATE_KEYS = ("exp_avg", "exp_avg_sq")
COUNTER_KEYS = ("create_steps", "radius3d_min", "radius3d_max")
COPY_PARENT, ZERO, SKIP = 0, 1, 2


# ---- plan ------------------------------------------------------------------------------------------------------------

def mask_flags(flag_split, flag_remove, node_index, index_parent, depth, max_level):
    """tensor_tree.py:121-122."""
    leaf = node_index == -1
    return flag_split & leaf & (depth < max_level), flag_remove & leaf & (index_parent != -1)


def plan(flag_split, flag_remove, remove_split, children):
    """-> keep_dest i32[P] (the reference's left_index on kept rows, -1 on the others), src_row i32[num_new], num_keep,
    num_split, overlap.  The flags are the masked ones."""
    flag_split, flag_remove = np.asarray(flag_split, bool), np.asarray(flag_remove, bool)
    gone = flag_remove | flag_split if remove_split else flag_remove
    keep = ~gone
    keep_dest = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    kept_rows = np.nonzero(keep)[0]
    split_rows = np.nonzero(flag_split)[0]
    src_row = np.concatenate([kept_rows, np.repeat(split_rows, children)]).astype(np.int32)
    overlap = 0 if remove_split else int((flag_split & flag_remove).sum())
    return keep_dest, src_row, int(kept_rows.size), int(split_rows.size), overlap


def move_rows(src, src_row, num_keep, child_mode=COPY_PARENT):
    """The row move: dst[d] = src[src_row[d]]; rows >= num_keep by child_mode (SKIP leaves zeros here)."""
    out = np.asarray(src)[src_row]
    if child_mode != COPY_PARENT:
        out[num_keep:] = 0
    return out


def counter_rule(key, old, src_row, num_keep):
    """splitter.py:207-220: children get zero, those of radius3d_min copy the parent."""
    return move_rows(old, src_row, num_keep, COPY_PARENT if key == "radius3d_min" else ZERO)


# ---- tree ------------------------------------------------------------------------------------------------------------

def initial_tree(n, max_child):
    """TensorTree.initialize (tensor_tree.py:32-43)."""
    return {"node_index": np.full(n, -1, np.int32), "index_parent": np.full(n, -1, np.int32),
            "local_index": np.full(n, -1, np.int8), "depth": np.zeros(n, np.int8),
            "tree": np.zeros((0, max_child), np.int32)}


def tree_update(t, flag_split, flag_remove, children):
    """split followed by remove (tensor_tree.py:65-118) on masked flags: -> the five new arrays."""
    keep_dest, src_row, num_keep, num_split, _ = plan(flag_split, flag_remove, False, children)
    num_nodes = t["tree"].shape[0]
    kept = src_row[:num_keep]
    parents = src_row[num_keep::children]
    node_index = t["node_index"].copy()
    node_index[parents] = num_nodes + np.arange(num_split, dtype=np.int32)
    ip = t["index_parent"][kept]
    new = {
        "node_index": np.concatenate([node_index[kept], np.full(num_split * children, -1, np.int32)]),
        "index_parent": np.concatenate([np.where(ip >= 0, keep_dest[np.maximum(ip, 0)], -1).astype(np.int32),
                                        np.repeat(keep_dest[parents], children)]),
        "local_index": np.concatenate([t["local_index"][kept], np.tile(np.arange(children, dtype=np.int8), num_split)]),
        "depth": np.concatenate([t["depth"][kept], np.repeat(t["depth"][parents] + 1, children).astype(np.int8)]),
    }
    old = t["tree"]
    tree = np.concatenate([np.where(old >= 0, keep_dest[np.maximum(old, 0)], -1).astype(np.int32),
                           (num_keep + np.arange(num_split * children, dtype=np.int32)).reshape(num_split, children)])
    has_node = new["node_index"] >= 0
    empty = (tree[new["node_index"][has_node]] < 0).all(axis=1)
    new["node_index"][np.nonzero(has_node)[0][empty]] = -1
    new["tree"] = tree
    return new


# ---- uniform split -----------------------------------------------------------------------------------------------------

def rotation_matrix(q):
    """geometry.py:4-25 in float64: the raw quaternion divided by its norm."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def split_uniform(xyz, raw_scaling, rotation, children, scaling_factor=0.5):
    """split_by_uniform (splitter.py:95-130) for the parents given, in float64.
    -> dict: xyz [n * children, 3], scaling (raw) [n * children, 3], the per-element condition scales S_xyz = |xyz_parent| +
    sum over rounds of 0.5 * scale[axis] and S_scaling = 1 + |raw|, axes [n, rounds] and min_gap = the smallest relative
    distance between two DIFFERENT current scales of one parent in any round (how safe the axis choice is)."""
    xyz, raw = np.asarray(xyz, np.float64), np.asarray(raw_scaling, np.float64)
    n = xyz.shape[0]
    rounds = {2: 1, 4: 2, 8: 3}[children]
    R = rotation_matrix(rotation)
    scale = np.exp(raw)
    centre = xyz[:, None, :]                                  # [n, 2^r, 3]
    reach = np.zeros(n)
    axes = np.zeros((n, rounds), np.int64)
    rows = np.arange(n)
    min_gap = np.inf
    for r in range(rounds):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            d = np.abs(scale[:, a] - scale[:, b]) / np.maximum(scale[:, a], scale[:, b])
            if (d > 0).any():
                min_gap = min(min_gap, float(d[d > 0].min()))
        axis = np.argmax(scale, axis=1)                       # the first of equal maxima: the lowest axis
        axes[:, r] = axis
        off = 0.5 * scale[rows, axis]
        step = R[rows, :, axis] * off[:, None]                # [n, 3]
        centre = np.stack([centre - step[:, None, :], centre + step[:, None, :]], axis=2).reshape(n, 2 * centre.shape[1], 3)
        reach += off
        scale = scale.copy()
        scale[rows, axis] *= scaling_factor
    out_scaling = np.repeat(np.log(scale), children, axis=0)
    return {"xyz": centre.reshape(-1, 3), "scaling": out_scaling,
            "S_xyz": np.repeat(np.abs(xyz) + reach[:, None], children, axis=0),
            "S_scaling": 1.0 + np.abs(out_scaling), "axes": axes, "min_gap": min_gap}


# ---- the state that is regenerated instead of stored ---------------------------------------------------------------------

def initial_geometry(seed, n, isotropic=False):
    """xyz f32[n, 3] and raw scaling f32[n, 3] of a case's first round; isotropic: three equal scales per row, as
    GaussianPoint.register_by_pointcloud creates them (level_of_gaussian.py:126)."""
    g = np.random.default_rng([seed, 0xD5])
    xyz = ((g.random((n, 3)) - 0.5) * 4.0).astype(np.float32)
    s = np.log(g.random((n, 1 if isotropic else 3)) * 0.06 + 0.01).astype(np.float32)
    return xyz, np.ascontiguousarray(np.broadcast_to(s, (n, 3)))


def copied_state(seed, rnd, p, sh_degree):
    """Everything a round only copies (or zeroes): rotation, opacity, colors, shs, both moments of every key and the three
    counter arrays, p rows each, drawn from (seed, round)."""
    g = np.random.default_rng([seed, rnd, 0xC0])
    f32 = lambda *shape: g.standard_normal(shape).astype(np.float32)
    widths = {"scaling": (3,), "colors": (3,), "xyz": (3,), "opacity": (1,), "rotation": (4,),
              "shs": ((sh_degree + 1) ** 2 - 1, 3)}
    if sh_degree == 0:
        del widths["shs"]
    out = {k: f32(p, *widths[k]) for k in COPIED_KEYS if k in widths}
    for sk in STATE_KEYS:
        for k, w in widths.items():
            out[f"{sk}.{k}"] = f32(p, *w)
    out["create_steps"] = g.integers(0, 1000, p).astype(np.int32)
    out["radius3d_min"] = (g.random(p) * 0.01 + 1e-4).astype(np.float32)
    out["radius3d_max"] = (g.random(p) * 0.5 + 0.1).astype(np.float32)
    return out


# ---- fixtures ----------------------------------------------------------------------------------------------------------

def fixture_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("densify_") and f.endswith(".npz"))


def unpack_flags(packed, p):
    return np.unpackbits(np.asarray(packed, np.uint8))[:p].astype(bool)


def load_fixture(name):
    """-> (meta dict, [round dict]) with the flags unpacked and every round's BEFORE state attached: 'p', 'xyz', 'scaling'
    (chained through the stored children), 'tree_before' (a dict, or None), 'copied' (copied_state of the round)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    xyz, scaling = initial_geometry(meta["seed"], meta["n"], bool(meta["isotropic"]))
    tree = initial_tree(meta["n"], meta["children"]) if meta["has_tree"] else None
    rounds = []
    for i in range(meta["rounds"]):
        r = {k[len(f"r{i}_"):]: z[k] for k in z.files if k.startswith(f"r{i}_")}
        p = xyz.shape[0]
        for k in ("flag_split", "flag_remove", "masked_split", "masked_remove"):
            r[k] = unpack_flags(r[k], p)
        r.update(p=p, xyz=xyz, scaling=scaling, tree_before=tree, copied=copied_state(meta["seed"], i, p, meta["sh_degree"]))
        rounds.append(r)
        nk = int(r["num_keep"])
        xyz = np.concatenate([xyz[r["src_row"][:nk]], r["child_xyz"]])
        scaling = np.concatenate([scaling[r["src_row"][:nk]], r["child_scaling"]])
        if tree is not None:
            tree = {k: r["after_" + k] for k in ("node_index", "index_parent", "local_index", "depth", "tree")}
    return meta, rounds

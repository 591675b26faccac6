"""Generates tests/golden/lod_*.npz by RUNNING the reference's own level-of-detail code (build container only:
needs /root/reference; the fixtures are committed and travel to the GPU box).

What is pinned: TensorTree.initialize / split / remove build the tree buffers, TensorTree.traverse +
_query_tree_torch (LoG/model/tensor_tree.py:131-185) select the points, Gaussian.compute_radius
(LoG/model/level_of_gaussian.py:65-88) gathers and activates (torch.exp, F.normalize) -- all unmodified
reference code.  The only stand-in is compute_radius_module (the CUDA extension, not buildable here), for
which the oracle's A0 is used (itself pinned against LoG/model/geometry.py by make_golden.py).

    python tests/golden/make_golden_lod.py
"""
import math
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("LOG_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (REF, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def reference_env():
    """Stubs for host-only deps + the LoG.cuda drop-in backed by the oracle (CPU)."""
    from log_amd import rasterizer as R
    from log_amd.compute_radius import compute_radius_module
    import oracle_backend
    from oracle_backend import OracleBackend
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    drop = types.ModuleType("LoG.cuda.compute_radius")
    drop.compute_radius_module = compute_radius_module
    sys.modules["LoG.cuda.compute_radius"] = drop
    oracle_backend.install(OracleBackend())


def build_case(seed, n_roots, n_levels, max_child, split_prob=0.7, remove_prob=0.04, extent=1.0, record=None):
    """A tree grown with the reference's TensorTree, parameters of children derived from their parent.  record (a list):
    receives the candidate lists the tree handed out, from which replay_case() draws the same parameters."""
    from LoG.model.tensor_tree import TensorTree
    tree = TensorTree(max_child=max_child, max_level=30)
    return (tree,) + _grow(_Grown(tree, record), seed, n_roots, n_levels, max_child, split_prob, remove_prob, extent)


def replay_case(seed, n_roots, n_levels, max_child, cands, split_prob=0.7, remove_prob=0.04, extent=1.0):
    """The parameters build_case() draws, from the candidate lists it recorded (no tree needed): (xyz, scaling, rotation)."""
    return _grow(_Replayed(cands), seed, n_roots, n_levels, max_child, split_prob, remove_prob, extent)


class _Grown:
    """The tree operations of _grow() on a reference TensorTree, recording every candidate list."""

    def __init__(self, tree, record):
        self.tree, self.record = tree, record if record is not None else []

    def initialize(self, xyz):
        self.tree.initialize(xyz)

    def split_candidates(self, level):
        return self._note(torch.where((self.tree.node_index == -1) & (self.tree.depth == level))[0])

    def split(self, parent):
        self.tree.split(parent)

    def remove_candidates(self):
        return self._note(torch.where((self.tree.node_index == -1) & (self.tree.index_parent > -1))[0])

    def remove(self, rem):
        self.tree.remove(rem)

    def _note(self, cand):
        self.record.append(cand.clone())
        return cand


class _Replayed:
    """The same operations, handing back recorded candidate lists."""

    def __init__(self, cands):
        self.cands = [torch.as_tensor(c).long() for c in cands]

    def initialize(self, xyz):
        pass

    def split_candidates(self, level):
        return self.cands.pop(0)

    def split(self, parent):
        pass

    def remove_candidates(self):
        return self.cands.pop(0)

    def remove(self, rem):
        pass


def _grow(ops, seed, n_roots, n_levels, max_child, split_prob, remove_prob, extent):
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(n_roots, 3, generator=g) - 0.5) * extent
    scaling = torch.log(torch.rand(n_roots, 3, generator=g) * 0.06 + 0.01)
    rotation = torch.randn(n_roots, 4, generator=g)
    ops.initialize(xyz)
    for level in range(n_levels):
        cand = ops.split_candidates(level)
        parent = cand[torch.rand(cand.shape[0], generator=g) < split_prob]
        if parent.numel() == 0:
            break
        ops.split(parent)
        rep = parent[:, None].repeat(1, max_child).reshape(-1)
        sig = torch.exp(scaling[rep]).max(dim=-1, keepdim=True).values
        xyz = torch.cat([xyz, xyz[rep] + torch.randn(rep.shape[0], 3, generator=g) * sig])
        scaling = torch.cat([scaling, scaling[rep] - math.log(1.6) + 0.2 * torch.randn(rep.shape[0], 3, generator=g)])
        rotation = torch.cat([rotation, rotation[rep] + 0.3 * torch.randn(rep.shape[0], 4, generator=g)])
    # holes: remove some non-root leaves (tensor_tree.py:92-119); the caller drops the same rows of the parameters
    cand = ops.remove_candidates()
    rem = cand[torch.rand(cand.shape[0], generator=g) < remove_prob]
    keep = torch.ones(xyz.shape[0], dtype=torch.bool)
    keep[rem] = False
    ops.remove(rem)
    xyz, scaling, rotation = xyz[keep], scaling[keep], rotation[keep]
    if isinstance(ops, _Grown):
        assert xyz.shape[0] == ops.tree.num_points
    return xyz.contiguous(), scaling.contiguous(), rotation.contiguous()


def camera_and_rasterizer(W, H, focal, theta=30.0, radius=2.5):
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    from log_amd import scenes
    cam = scenes.orbit_cameras(8, W=W, H=H, focal=focal, radius=radius)[int(theta // 45) % 8]
    tfx, tfy = math.tan(cam["FoVx"] * 0.5), math.tan(cam["FoVy"] * 0.5)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=tfx, tanfovy=tfy, bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=torch.tensor(cam["world_view_transform"]), projmatrix=torch.tensor(cam["full_proj_transform"]),
        sh_degree=0, campos=torch.tensor(cam["camera_center"]), prefiltered=False, debug=False)
    return cam, GaussianRasterizer(raster_settings=rs)


def random_tree_case(seed, cands=None, record=None):
    """Case `seed` of tests/test_lod_cpu.py::test_oracle_and_dropin_follow_reference_on_random_trees: a tree of random
    arity, depth and removal rate grown by the reference's TensorTree (cands=None; `record` receives its candidate lists)
    or its parameters replayed from those lists (cands), and a random camera.  -> (rng, tree or None, xyz, scaling,
    rotation, rast); rng goes on with the draws of the roots and the queries."""
    rng = np.random.default_rng(seed)
    mc = int(rng.choice([2, 3, 4, 8]))
    args = (100 + seed, int(rng.integers(50, 400)), int(rng.integers(1, 5)), mc)
    kw = dict(split_prob=float(rng.uniform(0.3, 0.95)), remove_prob=float(rng.uniform(0.0, 0.3)))
    if cands is None:
        tree, xyz, scaling, rotation = build_case(*args, record=record, **kw)
    else:
        tree, (xyz, scaling, rotation) = None, replay_case(*args, cands, **kw)
    cam, rast = camera_and_rasterizer(320, 240, float(rng.uniform(150, 500)), theta=float(rng.integers(0, 8) * 45))
    return rng, tree, xyz, scaling, rotation, rast


def random_tree_queries(rng, root_index):
    """The roots handed over (a random 85 %) and three (min_px, max_depth) queries of a random_tree_case()."""
    roots = root_index[torch.from_numpy(rng.random(root_index.shape[0]) < 0.85)]
    queries = []
    for _ in range(3):
        min_px = float(rng.choice([0.5, 2.0, 3.0, 6.0, 20.0]))
        queries.append((min_px, int(rng.choice([0, 1, 2, 3, 1000]))))
    return roots, queries


def reference_traverse(tree, xyz, scaling, rotation, root_index, rast, min_px, max_depth):
    from LoG.model.level_of_gaussian import Gaussian
    g = Gaussian()
    g.xyz, g.scaling, g.rotation = xyz, scaling, rotation
    tree.min_resolution_pixel = min_px
    return tree.traverse(g, root_index, rast, max_depth=max_depth)


CASES = [dict(name="a", seed=3, n_roots=300, n_levels=4, max_child=4, W=640, H=480, focal=600.0, theta=45.0),
         dict(name="b", seed=4, n_roots=1500, n_levels=3, max_child=2, W=400, H=400, focal=445.0, theta=180.0)]
QUERIES = [(3.0, 1000), (3.0, 2), (3.0, 0), (3.0, 1), (8.0, 1000), (0.5, 1000), (1e9, 1000)]


def main():
    reference_env()
    for c in CASES:
        tree, xyz, scaling, rotation = build_case(c["seed"], c["n_roots"], c["n_levels"], c["max_child"])
        cam, rast = camera_and_rasterizer(c["W"], c["H"], c["focal"], c["theta"])
        g = torch.Generator().manual_seed(c["seed"] + 100)
        roots = tree.root_index.long()
        roots = roots[torch.rand(roots.shape[0], generator=g) < 0.9]       # LoG.prepare hands over a subset
        out = {"node_index": tree.node_index.numpy(), "tree": tree.tree.numpy(), "depth": tree.depth.numpy(),
               "xyz": xyz.numpy(), "scaling": scaling.numpy(), "rotation": rotation.numpy(),
               "root_index": roots.numpy(), "max_level": np.int32(tree.max_level),
               "viewmatrix": np.asarray(cam["world_view_transform"], np.float32),
               "projmatrix": np.asarray(cam["full_proj_transform"], np.float32),
               "wh": np.array([c["W"], c["H"]], np.int32),
               "tanfov": np.array([rast.raster_settings.tanfovx, rast.raster_settings.tanfovy], np.float64),
               "queries": np.array(QUERIES, np.float64)}
        for qi, (min_px, max_depth) in enumerate(QUERIES):
            idx = reference_traverse(tree, xyz, scaling, rotation, roots, rast, min_px, int(max_depth))
            out[f"index_{qi}"] = idx.numpy().astype(np.int64)
            print(c["name"], "min_px", min_px, "max_depth", max_depth, "->", idx.shape[0], "of", tree.num_points,
                  "points; mean depth", float(tree.depth[idx].float().mean()))
        save_lzma(os.path.join(HERE, f"lod_{c['name']}.npz"), out)


def save_lzma(path, arrays):
    """np.savez with LZMA members (np.load reads them like deflated ones): lod_a stays below 1 MiB, which deflate misses."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asanyarray(a))
            z.writestr(name + ".npy", buf.getvalue())


if __name__ == "__main__":
    main()

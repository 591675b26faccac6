"""Generates tests/golden/lodrand_<seed>.npz by RUNNING the reference's own TensorTree (initialize / split / remove /
traverse, LoG/model/tensor_tree.py) and Gaussian.compute_radius on the random trees of
tests/test_lod_cpu.py::test_oracle_and_dropin_follow_reference_on_random_trees (build container only: needs the
reference tree).  Stored: the tree buffers, the candidate lists the tree handed out while it grew (the parameters are
replayed from them: make_golden_lod.replay_case), the roots, and the reference's selection for each query.

    python tests/golden/make_golden_lod_random.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_lod as G   # noqa: E402

SEEDS = range(8)


def main():
    G.reference_env()
    for seed in SEEDS:
        rec = []
        rng, tree, xyz, scaling, rotation, rast = G.random_tree_case(seed, record=rec)
        root_index = tree.root_index.long()
        roots, queries = G.random_tree_queries(rng, root_index)
        out = {"node_index": tree.node_index.numpy(), "tree": tree.tree.numpy(), "depth": tree.depth.numpy(),
               "max_level": np.int32(tree.max_level), "root_index": root_index.numpy(), "n_cands": np.int32(len(rec)),
               "queries": np.array(queries, np.float64)}
        for i, c in enumerate(rec):
            out["cand_%d" % i] = c.numpy().astype(np.int32)
        for q, (min_px, max_depth) in enumerate(queries):
            out["index_%d" % q] = G.reference_traverse(tree, xyz, scaling, rotation, roots, rast, min_px, max_depth).numpy()
        path = os.path.join(HERE, "lodrand_%d.npz" % seed)
        G.save_lzma(path, out)
        print(path, os.path.getsize(path), "points", tree.num_points, "selected", [len(out["index_%d" % q]) for q in range(3)])


if __name__ == "__main__":
    main()

"""Synthetic level-of-detail trees in the buffer layout TensorTree keeps (LoG/model/tensor_tree.py:57-90): see
log_amd.scenes.synth_tree (shared with bench.py's C3 leg)."""
from log_amd.scenes import synth_tree  # noqa: F401


def check_random_tree_case(seed, device, oracle_mod):
    """Case `seed` of the reference's recorded random trees (tests/golden/lodrand_<seed>.npz, written by
    tests/golden/make_golden_lod_random.py: the tree buffers, the reference's lists, and the candidate lists from which the
    parameters are drawn again here): the oracle and the drop-in on `device` (whatever backend is installed there does the
    work) return the list the reference's traverse returned.  One body for the CPU test and the GPU test."""
    import os
    import sys
    import types
    import numpy as np
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    if os.path.join(here, "golden") not in sys.path:
        sys.path.append(os.path.join(here, "golden"))
    import make_golden_lod as G
    from log_amd import lod
    ref = np.load(os.path.join(here, "golden", "lodrand_%d.npz" % seed))
    cands = [ref["cand_%d" % i] for i in range(int(ref["n_cands"]))]
    rng, _, xyz, scaling, rotation, rast = G.random_tree_case(seed, cands=cands)
    assert xyz.shape[0] == ref["node_index"].shape[0]
    tree = types.SimpleNamespace(node_index=torch.from_numpy(ref["node_index"]).to(device),
                                 tree=torch.from_numpy(ref["tree"]).to(device),
                                 depth=torch.from_numpy(ref["depth"]).to(device), max_level=int(ref["max_level"]))
    roots, queries = G.random_tree_queries(rng, torch.from_numpy(ref["root_index"]))
    np.testing.assert_array_equal(np.array(queries, np.float64), ref["queries"])
    rs = rast.raster_settings
    fx, fy = rs.image_width / (2 * rs.tanfovx), rs.image_height / (2 * rs.tanfovy)
    rast_dev = types.SimpleNamespace(raster_settings=rs._replace(
        bg=rs.bg.to(device), viewmatrix=rs.viewmatrix.to(device), projmatrix=rs.projmatrix.to(device),
        campos=rs.campos.to(device)))
    g = types.SimpleNamespace(xyz=xyz.to(device), scaling=scaling.to(device), rotation=rotation.to(device),
                              activation=types.SimpleNamespace(scaling_activation=torch.exp,
                                                               rotation_activation=torch.nn.functional.normalize))
    for q, (min_px, max_depth) in enumerate(queries):
        want = ref["index_%d" % q]
        got = oracle_mod.lod_traverse(ref["node_index"], ref["tree"], xyz.numpy(), scaling.numpy(), rotation.numpy(),
                                      roots.numpy(), rs.projmatrix.numpy(), rs.viewmatrix.numpy(), fx, fy, rs.tanfovx,
                                      rs.tanfovy, min_px, tree.max_level, max_depth)
        np.testing.assert_array_equal(got, want)
        tree.min_resolution_pixel = min_px
        np.testing.assert_array_equal(lod.traverse(tree, g, roots.to(device), rast_dev, max_depth=max_depth).cpu().numpy(), want)

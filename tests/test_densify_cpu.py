"""CPU checks of the device densification (log_amd/densify.py, log_amd/csrc/densify.hip): the numpy restatement
(tests/densify_ref.py) against the fixtures recorded from the reference (tests/golden/densify_*.npz), the new entry points
of the C ABI, their argument validation, and the drop-ins' fall-back to the reference's own methods."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import densify_ref as D
from test_log_plumbing_cpu import REF, _log_model, cpu_cuda_shims, log_env   # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
NEW_SYMBOLS = ("lograst_densify_scratch_bytes", "lograst_densify_plan", "lograst_densify_read", "lograst_densify_src_rows",
               "lograst_densify_move_rows", "lograst_densify_split_uniform", "lograst_densify_tree")
TREE_KEYS = ("node_index", "index_parent", "local_index", "depth", "tree")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")


def test_fixture_set_is_complete():
    names = D.fixture_names()
    assert {"densify_tree2", "densify_tree4", "densify_tree8", "densify_init8", "densify_edges",
            "densify_firstsplit"} <= set(names)
    for n in names:
        assert os.path.getsize(os.path.join(D.GOLDEN, n + ".npz")) < 1_000_000


@pytest.mark.parametrize("name", D.fixture_names())
def test_restatement_reproduces_fixture(name):
    """Integers exactly; the children within twice the reference's own fp32 error (K, measured by the generator and stored
    in the fixture) of the float64 restatement: K * 2^-24 * S per element."""
    meta, rounds = D.load_fixture(name)
    children = meta["children"]
    print(name, "K_xyz", meta["k_xyz"], "K_scaling", meta["k_scaling"])
    assert 0 < meta["k_xyz"] < 16 and 0 < meta["k_scaling"] < 16       # a reference that is itself fp32-accurate
    for i, r in enumerate(rounds):
        ms, mr = r["flag_split"], r["flag_remove"]
        if meta["has_tree"]:
            t = r["tree_before"]
            ms, mr = D.mask_flags(ms, mr, t["node_index"], t["index_parent"], t["depth"], meta["max_level"])
        assert np.array_equal(ms, r["masked_split"]) and np.array_equal(mr, r["masked_remove"]), i
        keep_dest, src_row, nk, ns, overlap = D.plan(ms, mr, not meta["has_tree"], children)
        assert overlap == 0 and nk == int(r["num_keep"]) and ns == int(r["num_split"]), i
        assert src_row.dtype == np.int32 and np.array_equal(src_row, r["src_row"]), i
        kept = keep_dest >= 0
        assert np.array_equal(keep_dest[kept], np.arange(nk)) and np.array_equal(np.nonzero(kept)[0], src_row[:nk])
        if meta["has_tree"]:
            new = D.tree_update(r["tree_before"], ms, mr, children)
            for k in TREE_KEYS:
                assert new[k].dtype == r["after_" + k].dtype and np.array_equal(new[k], r["after_" + k]), (i, k)
        for k in D.COUNTER_KEYS:
            assert np.array_equal(D.counter_rule(k, r["copied"][k], src_row, nk), r["after_" + k]), (i, k)
        parents = src_row[nk::children]
        r64 = D.split_uniform(r["xyz"][parents], r["scaling"][parents], r["copied"]["rotation"][parents], children)
        assert ns == 0 or r64["min_gap"] >= 1e-6
        for k in ("xyz", "scaling"):
            err = np.abs(r["child_" + k].astype(np.float64) - r64[k])
            bound = 2.0 * meta["k_" + k] * EPS * r64["S_" + k]
            assert err.shape == (ns * children, 3) and (err <= bound).all(), (i, k, float((err / bound).max(initial=0)))


def test_isotropic_rows_split_the_lowest_axis_first():
    """The tie rule: three equal scales split axis 0, then 1, then 2 (what the CPU torch of the fixtures did)."""
    meta, rounds = D.load_fixture("densify_init8")
    r = rounds[0]
    parents = r["src_row"][int(r["num_keep"])::8]
    assert (r["scaling"][parents][:, 0] == r["scaling"][parents][:, 1]).all()
    r64 = D.split_uniform(r["xyz"][parents], r["scaling"][parents], r["copied"]["rotation"][parents], 8)
    assert (r64["axes"] == np.array([0, 1, 2])).all()
    halved = np.rint((np.repeat(r["scaling"][parents], 8, axis=0) - r["child_scaling"]) / np.log(2.0))
    assert (halved == 1).all()


def test_symbols_are_declared_exported_and_bound():
    from log_amd import _lib
    header = open(os.path.join(ROOT, "include", "lograst.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    assert ctypes.sizeof(_lib.LograstMoveKey) == 32
    assert _lib.lib().lograst_version() == 4 and _lib.lib().lograst_knob_count() == 22


def test_move_key_matches_the_header(tmp_path):
    import shutil
    import subprocess
    from log_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    names = [f[0] for f in _lib.LograstMoveKey._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "lograst.h"', 'int main(void) {',
            '  printf("%zu", sizeof(lograst_move_key));']
    prog += [f'  printf(" %zu", offsetof(lograst_move_key, {n}));' for n in names]
    prog += ['  printf(" %d %d %d\\n", LOGRAST_MOVE_COPY_PARENT, LOGRAST_MOVE_ZERO, LOGRAST_MOVE_SKIP);', '  return 0;', '}']
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text("\n".join(prog))
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == ctypes.sizeof(_lib.LograstMoveKey)
    assert out[1:1 + len(names)] == [getattr(_lib.LograstMoveKey, n).offset for n in names]
    assert out[-3:] == [_lib.MOVE_COPY_PARENT, _lib.MOVE_ZERO, _lib.MOVE_SKIP] == [D.COPY_PARENT, D.ZERO, D.SKIP]


def test_argument_validation_needs_no_gpu():
    from log_amd import _lib
    L = _lib.lib()
    err = lambda: L.lograst_last_error().decode()
    assert L.lograst_densify_scratch_bytes(0) >= 16
    assert L.lograst_densify_scratch_bytes(2 ** 31 - 1) >= 16 + 2 * 4 * (2 ** 21)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    plan = lambda n, children, scratch, nbytes: L.lograst_densify_plan(n, p, p, 0, children, None, None, None, 0, p, p, p,
                                                                      scratch, nbytes, None)
    assert plan(-1, 4, p, 4096) == -1 and "negative" in err()
    for children in (0, 1, 3, 5, 16):
        assert plan(8, children, p, 4096) == -1 and "children must be 2, 4 or 8" in err()
    assert plan(8, 4, p, 8) == -1 and "scratch too small" in err()
    assert plan(8, 4, None, 4096) == -1 and "scratch too small" in err()
    assert L.lograst_densify_plan(8, p, p, 0, 4, p, None, None, 0, p, p, p, p, 4096, None) == -1 and "go together" in err()
    assert L.lograst_densify_src_rows(8, 3, 0, p, p, 1, 1, p, p, None) == -1 and "children" in err()
    assert L.lograst_densify_src_rows(8, 4, 0, p, p, -1, 1, p, p, None) == -1 and "negative" in err()
    assert L.lograst_densify_src_rows(8, 4, 0, p, p, 9, 0, p, p, None) == -1 and "more kept or split rows" in err()
    assert L.lograst_densify_split_uniform(0, 1, 6, 0.5, 8, p, p, p, p, p, p, None) == -1 and "children" in err()
    assert L.lograst_densify_split_uniform(-1, 1, 4, 0.5, 8, p, p, p, p, p, p, None) == -1 and "negative" in err()
    assert L.lograst_densify_tree(-1, 0, 4, 0, 0, *([p] * 13), None) == -1 and "negative" in err()
    assert L.lograst_densify_tree(8, 0, 7, 0, 0, *([p] * 13), None) == -1 and "children" in err()
    keys = (_lib.LograstMoveKey * 9)()
    for k in keys:
        k.src, k.dst, k.elem_size, k.columns, k.child_mode = p.value, p.value & ~15, 4, 3, 0
    move = lambda nk, nn, n: L.lograst_densify_move_rows(nk, nn, 8, p, n, keys, None)
    assert move(1, 2, 9) == -1 and "at most 8 keys" in err()
    assert move(-1, 2, 1) == -1 and "negative" in err()
    assert move(3, 2, 1) == -1 and "num_keep exceeds" in err()
    for bad in (0, 3, 8):
        keys[0].elem_size = bad
        assert move(1, 2, 1) == -1 and "element size must be 1, 2 or 4" in err()
    keys[0].elem_size, keys[0].child_mode = 4, 3
    assert move(1, 2, 1) == -1 and "child mode" in err()
    keys[0].child_mode, keys[0].columns = 0, 0
    assert move(1, 2, 1) == -1 and "row size" in err()
    keys[0].columns, keys[0].dst = 3, (p.value & ~15) + 4
    assert move(1, 2, 1) == -1 and "16-byte aligned" in err()
    # nothing to do is not an error, and touches no device
    keys[0].dst = p.value & ~15
    assert move(0, 0, 1) == 0 and L.lograst_densify_split_uniform(4, 0, 4, 0.5, 8, p, p, p, p, p, p, None) == 0


def _state(model):
    out = {"tree." + k: getattr(model.tree, k).clone() for k in TREE_KEYS}
    out.update({"g." + k: getattr(model.gaussian, k).detach().clone() for k in model.gaussian.keys})
    for sk in model.optimizer.state_keys:
        out.update({f"{sk}.{k}": v.clone() for k, v in getattr(model.optimizer, sk).items()})
    out.update({"c." + k: getattr(model.counter, k).clone() for k in D.COUNTER_KEYS})
    return out


@needs_reference
def test_dropins_fall_back_to_the_reference_on_cpu_tensors(cpu_cuda_shims, caplog):
    """Tensors that are not on the GPU go to the reference's own methods: a model grown through the installed drop-ins on
    the CPU is the model the reference grows."""
    from LoG.model.splitter import Splitter
    from LoG.model.tensor_tree import TensorTree
    from log_amd import densify
    saved = (TensorTree.split_and_remove, Splitter.split_and_remove, Splitter.split_and_remove_other)
    want = _state(_log_model(0, 400))
    try:
        assert densify.install() is Splitter
        assert TensorTree.split_and_remove is densify.tree_split_and_remove
        assert Splitter.split_and_remove is densify.split_and_remove
        assert Splitter.split_and_remove_other is densify.split_and_remove_other
        densify.dropins.logged.clear()
        densify.reset_stats()
        with caplog.at_level("WARNING", logger="log_amd"):
            got = _state(_log_model(0, 400))
        densify.uninstall()
        assert (TensorTree.split_and_remove, Splitter.split_and_remove, Splitter.split_and_remove_other) == saved
    finally:
        TensorTree.split_and_remove, Splitter.split_and_remove, Splitter.split_and_remove_other = saved
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    logged = [r.getMessage() for r in caplog.records if "log_amd.densify" in r.getMessage()]
    assert len(logged) == 3 and all("not on the GPU" in m for m in logged), logged      # once per method, not per call
    st = densify.stats()
    methods = ("tree_split_and_remove", "split_and_remove", "split_and_remove_other")
    assert set(st["calls"]) == set(methods) and min(st["calls"].values()) >= 1 and st["readbacks"] == {}
    assert st["fallbacks"] == {(m, "tensors are not on the GPU"): st["calls"][m] for m in methods}       # every call fell back


@needs_reference
def test_install_all_without_the_flag_leaves_densification_alone(cpu_cuda_shims):
    from LoG.model.counter import Counter
    from LoG.model.level_of_gaussian import LoG
    from LoG.model.sparse_optimizer import SparseOptimizer
    from LoG.model.splitter import Splitter
    from LoG.model.tensor_tree import TensorTree
    import LoG.render.renderer as ref_renderer
    import log_amd
    densify_methods = (TensorTree.split_and_remove, Splitter.split_and_remove, Splitter.split_and_remove_other)
    saved = (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
             ref_renderer.torch)
    try:
        patched = log_amd.install_all()
        assert [c.__name__ for c in patched] == ["LoG", "TensorTree", "Counter", "SparseOptimizer"]
        assert (TensorTree.split_and_remove, Splitter.split_and_remove, Splitter.split_and_remove_other) == densify_methods
        patched = log_amd.install_all(device_densify=True)
        assert patched[-1] is Splitter and Splitter.split_and_remove is log_amd.densify.split_and_remove
        log_amd.densify.uninstall()
        assert (TensorTree.split_and_remove, Splitter.split_and_remove, Splitter.split_and_remove_other) == densify_methods
    finally:
        (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
         ref_renderer.torch) = saved
        TensorTree.split_and_remove, Splitter.split_and_remove, Splitter.split_and_remove_other = densify_methods
        if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
            del SparseOptimizer._lograst_load_state_dict

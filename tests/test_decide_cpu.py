"""CPU checks of the device decision layer (log_amd/decide.py, log_amd/csrc/decide.hip): the numpy restatement
(tests/decide_ref.py) against the fixtures recorded from the reference's own update_depth_stage / update_init_stage
(tests/golden/decide_*.npz), the new entry points of the C ABI and their argument validation, the ctypes mirrors of the new
structs, and the drop-ins' fall-back to the reference's methods on CPU tensors."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import decide_ref as R
from test_log_plumbing_cpu import REF, _Cfg, _log_model, cpu_cuda_shims, log_env   # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")
DEPTH_LINES = ("opacity", "ratio", "grad", "radii")
INIT_LINES = ("radii_max_act", "grad", "radii_split", "radius3d_min")
ULP = 2.0 ** -23          # spacing of fp32 relative to a value in [1, 2)


def test_fixture_set_is_complete():
    names = R.fixture_names()
    assert {"decide_depth2", "decide_depth4", "decide_depth8", "decide_depth_few", "decide_depth_exact", "decide_init_scale1",
            "decide_init_scale2"} <= set(names)
    for n in names:
        assert os.path.getsize(os.path.join(R.GOLDEN, n + ".npz")) < 1_000_000


def _line_agrees(pop, line, where):
    s = R.stat64(pop)
    assert s["count"] == line[0] and float(s["min"]) == line[1] and float(s["max"]) == line[2], where
    assert abs(s["mean"] - line[3]) <= 1e-12 * abs(line[3]) and abs(s["std"] - line[4]) <= 1e-12 * abs(line[4]), where


@pytest.mark.parametrize("name", R.fixture_names("depth"))
def test_restatement_reproduces_depth_fixture(name):
    meta, rounds = R.load_fixture(name)
    cfg = dict(R.DEPTH_CFG)
    saw_cut = saw_removal = False
    for i, r in enumerate(rounds):
        where = f"{name} round {i}"
        cfg["max_split_points"] = int(r["max_split_points"])
        t = r["tree_before"]
        w = R.depth_stage(t["node_index"], t["depth"], r["c"], cfg, meta["current_depth"], meta["max_level"])
        assert np.array_equal(w["flag_split"], r["flag_split"]) and np.array_equal(w["flag_remove"], r["flag_remove"]), where
        assert w["num_max_split"] == int(r["num_max_split"]) and w["need_cut"] == bool(r["need_cut"]), where
        assert (w["cut_value"] if w["cut_value"] is not None else -1) == int(r["cut_value"]), where
        assert np.array_equal(R.depth_after(w, meta["children"]), r["depth_after"]), where
        # the two lines whose data is exact, from the raw inputs; the two behind an activation from the recorded data, which
        # the float64 activation of the raw inputs must meet: sigmoid within 1 ulp, the ratio max / (sum - max - min) within
        # (2 + 3 * ratio) ulp -- sum, max and min carry half an ulp of `max` each into a difference of size `mid`
        _line_agrees(w["pop"]["grad"], r["line_grad"], where)
        _line_agrees(w["pop"]["radii"], r["line_radii"], where)
        _line_agrees(r["pop_opacity"], r["line_opacity"], where)
        _line_agrees(r["pop_ratio"], r["line_ratio"], where)
        o64 = R.sigmoid64(r["opacity"][:, 0])[w["parent"]]
        assert (np.abs(r["pop_opacity"] - o64) <= ULP * o64).all(), where
        q64 = R.ratio64(r["scaling"])[w["parent"]]
        assert (np.abs(r["pop_ratio"] - q64) <= ULP * q64 * (2 + 3 * q64)).all(), where
        saw_cut |= w["need_cut"] and int(w["flag_split"].sum()) > w["num_max_split"]          # ties survive the cut
        saw_removal |= int(w["flag_remove"].sum()) > 0
        if name == "decide_depth_few":
            assert 0 < w["counts"]["candidates"] < w["num_max_split"] and not w["need_cut"]
        if name == "decide_depth_exact":
            assert w["counts"]["candidates"] == w["num_max_split"] > 0 and not w["need_cut"]
    if meta["rounds"] == 3:
        assert saw_cut and saw_removal, name


@pytest.mark.parametrize("name", R.fixture_names("init"))
def test_restatement_reproduces_init_fixture(name):
    meta, (r,) = R.load_fixture(name)
    c = r["c"]
    assert R.nonmax_margin_ulp(c["opacity"][:, 0], c["weights_max"]) > 64
    act = R.sigmoid64(c["opacity"][:, 0]).astype(np.float32)
    w = R.init_stage(act, c, r["rand"], R.INIT_CFG, meta["scale"], meta["children"])
    assert np.array_equal(w["flag_split"], r["flag_split"]) and np.array_equal(w["flag_remove"], r["flag_remove"])
    assert [w["counts"][k] for k in ("remove_weight", "nonmax", "remove_small", "split_grad", "split_radii")] == list(r["counts"])
    assert min(r["counts"]) > 0 and w["flag_split"].any() and w["flag_remove"].any()
    for k in INIT_LINES:
        _line_agrees(w["pop"][k], r["line_" + k], k)
    assert int(r["num_points_after"]) == w["pop"]["radius3d_min"].size


def test_top_k_cut_keeps_ties_and_compares_in_fp32():
    radii = np.array([5, 9, 9, 9, 2, 2 ** 24 + 1, 2 ** 24, 7], np.int32)
    cand = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    cut, keep = R.top_k_cut(cand, radii, 3)
    assert cut == 9 and keep.tolist() == [False, True, True, True, False, True, True, False]
    cut, keep = R.top_k_cut(cand, radii, 1)          # 2^24 + 1 rounds to 2^24 in fp32: the reference keeps both
    assert cut == 2 ** 24 + 1 and int(keep.sum()) == 2


def test_sizing_helper_and_argument_checks_work_without_gpu():
    from log_amd import _lib
    L = _lib.lib()
    err = lambda: L.lograst_last_error().decode()
    assert L.lograst_version() == 4
    nbytes = L.lograst_decide_scratch_bytes(1000)
    assert ctypes.sizeof(_lib.LograstDecideRecord) < nbytes < (1 << 20) and nbytes == L.lograst_decide_scratch_bytes(30_000_000)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    p.value = (p.value + 15) & ~15
    da, ia = _lib.LograstDecideDepthArgs(), _lib.LograstDecideInitArgs()
    assert L.lograst_decide_depth(-1, ctypes.byref(da), p, nbytes, None) < 0 and "negative" in err()
    assert L.lograst_decide_init(-1, ctypes.byref(ia), p, nbytes, None) < 0 and "negative" in err()
    assert L.lograst_decide_depth(8, None, p, nbytes, None) < 0 and "args is NULL" in err()
    assert L.lograst_decide_depth(8, ctypes.byref(da), p, 8, None) < 0 and "scratch too small" in err()
    assert L.lograst_decide_init(8, ctypes.byref(ia), None, nbytes, None) < 0 and "scratch too small" in err()
    assert L.lograst_decide_depth(8, ctypes.byref(da), p.value + 4, nbytes, None) < 0 and "16-byte aligned" in err()
    assert L.lograst_decide_depth(8, ctypes.byref(da), p, nbytes, None) < 0 and "NULL pointer" in err()
    assert L.lograst_decide_init(8, ctypes.byref(ia), p, nbytes, None) < 0 and "NULL pointer" in err()
    for name, _ in da._fields_:
        if getattr(_lib.LograstDecideDepthArgs, name).size == 8:
            setattr(da, name, p.value)
    assert L.lograst_decide_depth(8, ctypes.byref(da), p, nbytes, None) < 0 and "their own storage" in err()
    da.flag_remove = p.value + 16
    da.current_depth = 300
    assert L.lograst_decide_depth(8, ctypes.byref(da), p, nbytes, None) < 0 and "current_depth" in err()
    for name, _ in ia._fields_:
        if getattr(_lib.LograstDecideInitArgs, name).size == 8:
            setattr(ia, name, p.value)
    ia.flag_remove = p.value + 16
    for children in (0, 9):
        ia.children = children
        assert L.lograst_decide_init(8, ctypes.byref(ia), p, nbytes, None) < 0 and "children" in err()
    rec = _lib.LograstDecideRecord()
    assert L.lograst_decide_read(None, ctypes.byref(rec), ctypes.sizeof(rec), None) < 0 and "NULL" in err()
    assert L.lograst_decide_read(p, ctypes.byref(rec), ctypes.sizeof(rec) - 8, None) < 0 and "record_bytes" in err()
    assert L.lograst_decide_child_radius_max(-1, 0, p, p, 0.9, p, None) < 0 and "negative" in err()
    assert L.lograst_decide_child_radius_max(4, 5, p, p, 0.9, p, None) < 0 and "more children" in err()
    assert L.lograst_decide_child_radius_max(4, 2, None, p, 0.9, p, None) < 0 and "NULL" in err()
    assert L.lograst_decide_child_radius_max(4, 0, None, None, 0.9, None, None) == 0      # nothing to do touches no device


def test_ctypes_mirrors_of_the_decide_structs_match_the_header(tmp_path):
    from log_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    structs = {"lograst_decide_stat": _lib.LograstDecideStat, "lograst_decide_record": _lib.LograstDecideRecord,
               "lograst_decide_depth_args": _lib.LograstDecideDepthArgs, "lograst_decide_init_args": _lib.LograstDecideInitArgs}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "lograst.h"', 'int main(void) {']
    for st, cls in structs.items():
        prog.append(f'  printf("{st} %zu", sizeof({st}));')
        prog += [f'  printf(" %zu", offsetof({st}, {f[0]}));' for f in cls._fields_]
        prog.append('  printf("\\n");')
    prog += ['  return 0;', '}']
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text("\n".join(prog))
    subprocess.check_call([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    for line, (st, cls) in zip(out, structs.items()):
        parts = line.split()
        assert parts[0] == st and int(parts[1]) == ctypes.sizeof(cls), line
        assert [int(x) for x in parts[2:]] == [getattr(cls, f[0]).offset for f in cls._fields_], line
    assert _lib.DECIDE_DEPTH_BINS == 256


def _state(model):
    out = {"tree." + k: getattr(model.tree, k).clone() for k in R.TREE_KEYS}
    out.update({"g." + k: getattr(model.gaussian, k).detach().clone() for k in model.gaussian.keys})
    for sk in model.optimizer.state_keys:
        out.update({f"{sk}.{k}": v.clone() for k, v in getattr(model.optimizer, sk).items()})
    out.update({"c." + k: getattr(model.counter, k).clone() for k in R.COUNTER_INPUTS})
    return out


def _events(seed):
    """A depth-stage event on a two-level model, then an init-stage event on it (the reference's methods, or whatever is
    installed in their place); -> the model's state after each."""
    model = _log_model(seed, 400)
    states = []
    for stage, cfg in (("depth", R.DEPTH_CFG), ("init", R.INIT_CFG)):
        model.densify_and_remove = _Cfg(cfg, max_split_points=10)
        c = R.counter_inputs(seed, 0, model.num_points, wide=stage == "init")
        for k in R.COUNTER_INPUTS:
            getattr(model.counter, k).set_(torch.from_numpy(c[k].copy()))
        model.gaussian.opacity.data.copy_(torch.from_numpy(c["opacity"]))
        torch.manual_seed(seed)
        if stage == "depth":
            model.update_depth_stage(12)
        else:
            model.update_init_stage(scale=1)
        states.append(_state(model))
    return states


@needs_reference
def test_install_all_with_the_flag_falls_back_on_cpu_tensors(cpu_cuda_shims):
    """install_all(device_decide=True) on a CPU model: both drop-ins hand over to the reference's methods, count the reason,
    and leave the model the unpatched methods leave."""
    from LoG.model.counter import Counter
    from LoG.model.level_of_gaussian import LoG
    from LoG.model.sparse_optimizer import SparseOptimizer
    from LoG.model.tensor_tree import TensorTree
    import LoG.render.renderer as ref_renderer
    import log_amd
    from log_amd import decide
    ours = (LoG.update_depth_stage, LoG.update_init_stage)
    saved = (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
             ref_renderer.torch)
    want = _events(3)
    try:
        patched = log_amd.install_all()
        assert (LoG.update_depth_stage, LoG.update_init_stage) == ours            # default off
        patched = log_amd.install_all(device_decide=True)
        assert patched[-1] is LoG and LoG.update_depth_stage is decide.update_depth_stage
        assert LoG.update_init_stage is decide.update_init_stage
        decide.reset_stats()
        got = _events(3)
        st = decide.stats()
        decide.uninstall()
        assert (LoG.update_depth_stage, LoG.update_init_stage) == ours
    finally:
        (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
         ref_renderer.torch) = saved
        LoG.update_depth_stage, LoG.update_init_stage = ours
        if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
            del SparseOptimizer._lograst_load_state_dict
    assert st["calls"] == {"update_depth_stage": 1, "update_init_stage": 1} and st["readbacks"] == {}
    assert st["fallbacks"] == {("update_depth_stage", "tensors are not on the GPU"): 1,
                               ("update_init_stage", "tensors are not on the GPU"): 1}
    for a, b in zip(want, got):
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert want[0]["g.xyz"].shape[0] != want[1]["g.xyz"].shape[0] != 0

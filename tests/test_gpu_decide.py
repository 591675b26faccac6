"""The device decision layer (log_amd/decide.py -> log_amd/csrc/decide.hip) against the fixtures recorded from the
reference's own LoG.update_depth_stage / update_init_stage (tests/golden/decide_*.npz) and the numpy restatement
tests/decide_ref.py (held to those fixtures by tests/test_decide_cpu.py).  No test here reads the reference tree: the drop-ins
run on stand-in objects that carry the attributes the reference's LoG / TensorTree / Counter / Splitter carry.

Flags, counts, num_max_split, the threshold and the depth histograms must match bit for bit; min / max of grad and radii
exactly, min / max of opacity and ratio within 2 fp32 ulp (the activation); mean and std by the criterion of the step kernels
(tests/test_gpu_fuzz_step.py):  |hip - ref64| <= 8 * (|ref32 - ref64| + 2^-24 * S),  ref32 the reference's own fp32 result,
ref64 the float64 statistic of the same data, S = max |x| of the population."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decide_ref as R  # noqa: E402
import densify_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -24
DEPTH_LINES = ("opacity", "ratio", "grad", "radii")
INIT_LINES = ("radii_max_act", "grad", "radii_split", "radius3d_min")
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = R.load_fixture(name)
    return _CACHE[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counter_of(c):
    return types.SimpleNamespace(**{k: dev(c[k]) for k in R.COUNTER_INPUTS})


def run_depth(node_index, depth, scaling, c, cfg, current_depth, max_level):
    from log_amd import decide
    fs, fr, rec = decide.decide_depth(dev(c["opacity"]), dev(scaling), dev(node_index), dev(depth), counter_of(c), current_depth,
                                      max_level, cfg["min_steps_split"], cfg["split_grad_thres"], cfg["radius2d_thres"],
                                      cfg["remove_weights_thres"], cfg["max_split_points"])
    assert fs.dtype == torch.bool and fr.dtype == torch.bool and fs.device.type == "cuda"
    return fs.cpu().numpy(), fr.cpu().numpy(), rec


def hist(d):
    out = np.zeros(256, np.int64)
    for k, v in d.items():
        out[k + 128] = v
    return out


def check_exact(rec, fs, fr, w, where):
    from log_amd import decide
    assert np.array_equal(fs, w["flag_split"]), (where, "flag_split", int((fs != w["flag_split"]).sum()))
    assert np.array_equal(fr, w["flag_remove"]), (where, "flag_remove")
    assert {k: rec.counts[i] for k, i in decide.C.items()} == w["counts"], where
    assert rec.num_max_split == w["num_max_split"] and rec.need_cut == w["need_cut"], (where, rec.num_max_split, rec.need_cut)
    if w["cut_value"] is not None:
        assert rec.cut_value == w["cut_value"] and rec.cut_thres == float(np.float32(w["cut_value"])), (where, rec.cut_value)
    for k in ("depth_all", "depth_split", "depth_remove"):
        assert np.array_equal(hist(getattr(rec, k)), w[k]), (where, k)


def check_line(st, line, where, ulp_minmax=0):
    """line: [count, min, max, mean64, std64, mean32, std32, S] of the fixture."""
    n, mn, mx, m64, s64, m32, s32, S = [float(v) for v in line]
    tol_min, tol_max = ulp_minmax * float(np.spacing(np.float32(abs(mn)))), ulp_minmax * float(np.spacing(np.float32(abs(mx))))
    bm, bs = 8 * (abs(m32 - m64) + EPS * S), 8 * (abs(s32 - s64) + EPS * S)
    print(where, "count", st.count, "min", st.min - mn, "max", st.max - mx, "mean err / bound %.3g" % (abs(st.mean - m64) / bm),
          "std err / bound %.3g" % (abs(st.std - s64) / bs))
    assert st.count == n, where
    assert abs(st.min - mn) <= tol_min and abs(st.max - mx) <= tol_max, (where, st.min, mn, st.max, mx)
    assert abs(st.mean - m64) <= bm and abs(st.std - s64) <= bs, (where, st.mean, m64, st.std, s64)


# ---- the fixtures ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.fixture_names("depth"))
def test_depth_fixture_decisions_on_the_device(name):
    meta, rounds = fixture(name)
    cfg = dict(R.DEPTH_CFG)
    for i, r in enumerate(rounds):
        where = f"{name} round {i}"
        cfg["max_split_points"] = int(r["max_split_points"])
        t = r["tree_before"]
        w = R.depth_stage(t["node_index"], t["depth"], r["c"], cfg, meta["current_depth"], meta["max_level"])
        assert np.array_equal(w["flag_split"], r["flag_split"])            # the restatement is the fixture (test_decide_cpu)
        fs, fr, rec = run_depth(t["node_index"], t["depth"], r["scaling"], r["c"], cfg, meta["current_depth"], meta["max_level"])
        check_exact(rec, fs, fr, w, where)
        assert np.array_equal(fs, r["flag_split"]) and np.array_equal(fr, r["flag_remove"]), where
        assert rec.num_max_split == int(r["num_max_split"]) and rec.need_cut == bool(r["need_cut"]), where
        assert np.array_equal(hist(rec.depth_after(meta["children"])), r["depth_after"]), where
        for j, k in enumerate(DEPTH_LINES):
            check_line(rec.stats[j], r["line_" + k], f"{where} {k}", ulp_minmax=2 if k in ("opacity", "ratio") else 0)


@pytest.mark.parametrize("name", R.fixture_names("init"))
def test_init_fixture_decisions_on_the_device(name):
    from log_amd import decide
    meta, (r,) = fixture(name)
    c, cfg = r["c"], R.INIT_CFG
    fs, fr, rec = decide.decide_init(dev(c["opacity"]), counter_of(c), meta["children"], cfg["init_weight_min"],
                                     cfg["init_radius_min"], cfg["init_radius_split"], cfg["split_grad_thres"], cfg["min_steps"],
                                     meta["scale"], dev(r["rand"]))
    assert np.array_equal(fs.cpu().numpy(), r["flag_split"]) and np.array_equal(fr.cpu().numpy(), r["flag_remove"])
    assert [rec.counts[decide.CI[k]] for k in ("remove_weight", "nonmax", "remove_small", "split_grad", "split_radii")] == list(r["counts"])
    for j, k in enumerate(INIT_LINES):
        check_line(rec.stats[j], r["line_" + k], f"{name} {k}")


# ---- sizes at which the kernels can go wrong -------------------------------------------------------------------------

def synthetic(p, seed):
    """A tree-shaped input of p rows: three depths, a third of the rows inner nodes; scales within a factor 2.7 of each
    other, so that no ratio exceeds e."""
    if ("syn", p, seed) not in _CACHE:
        g = np.random.default_rng([seed, p])
        c = R.counter_inputs(seed, 0, p)
        depth = g.integers(0, 3, p).astype(np.int8)
        node_index = np.where(g.random(p) < 0.33, g.integers(0, max(p, 1), p), -1).astype(np.int32)
        scaling = (np.log(0.02) + g.random((p, 3))).astype(np.float32)
        _CACHE[("syn", p, seed)] = (node_index, depth, scaling, c)
    return _CACHE[("syn", p, seed)]


def check_stat64(st, pop, where, extra=1.0):
    """Against the float64 statistic of a population that is itself exact (extra = 1), or whose elements the kernel may
    form with a relative error of extra * 2^-24."""
    s = R.stat64(pop)
    assert st.count == s["count"], where
    if s["count"] == 0:
        assert st.min == np.inf and st.max == -np.inf and st.sum == 0.0
        return
    bound = 8 * EPS * s["S"] * extra
    assert abs(st.mean - s["mean"]) <= bound, (where, st.mean, s["mean"])
    if s["count"] > 1:
        assert abs(st.std - s["std"]) <= bound, (where, st.std, s["std"])
    else:
        assert np.isnan(st.std)
    if extra == 1.0:
        assert st.min == float(s["min"]) and st.max == float(s["max"]), where


@pytest.mark.parametrize("p", [0, 1, 1023, 1024, 1025, 1024 * 1024 + 1])
def test_depth_stage_at_the_edges_of_chunks_and_partials(p):
    """1024 rows a chunk, 2048 workgroups at the most: 1024 * 1024 + 1 rows is past one round of chunk partials."""
    node_index, depth, scaling, c = synthetic(p, 5)
    cfg = dict(R.DEPTH_CFG, max_split_points=max(p // 200, 1))
    w = R.depth_stage(node_index, depth, c, cfg, 2, 20)
    fs, fr, rec = run_depth(node_index, depth, scaling, c, cfg, 2, 20)
    check_exact(rec, fs, fr, w, f"p = {p}")
    if p >= 1023:
        assert w["need_cut"] and w["flag_remove"].any() and 0 < w["flag_split"].sum() < w["counts"]["candidates"]
    par = w["parent"]
    check_stat64(rec.stats[2], w["pop"]["grad"], "grad")
    check_stat64(rec.stats[3], w["pop"]["radii"], "radii")
    # sigmoid: two roundings and an exp of 1 ulp; ratio = max / ((e0 + e1) + e2 - max - min) <= e: every term of the
    # difference carries 2^-24 * max, the quotient amplifies by max / mid -> (2 + 3 * e) * e < 28 units of 2^-24
    check_stat64(rec.stats[0], R.sigmoid64(c["opacity"][:, 0])[par], "opacity", extra=4.0)
    check_stat64(rec.stats[1], R.ratio64(scaling)[par], "ratio", extra=28.0)


@pytest.mark.parametrize("p", [0, 1, 1023, 1024, 1025, 1024 * 1024 + 1])
def test_init_stage_at_the_edges_of_chunks_and_partials(p):
    from log_amd import decide
    g = np.random.default_rng([9, p])
    c = R.counter_inputs(9, 0, p, wide=True)
    rand = g.random(p).astype(np.float32)
    act = R.sigmoid64(c["opacity"][:, 0]).astype(np.float32)
    near = np.abs(c["weights_max"].astype(np.float64) - act.astype(np.float64) * float(np.float32(0.1))) <= 64 * np.spacing(act * np.float32(0.1))
    c["weights_max"][near] = 0.5                      # the one comparison behind an activation keeps its margin
    cfg = R.INIT_CFG
    w = R.init_stage(act, c, rand, cfg, 1, 4)
    fs, fr, rec = decide.decide_init(dev(c["opacity"]), counter_of(c), 4, cfg["init_weight_min"], cfg["init_radius_min"],
                                     cfg["init_radius_split"], cfg["split_grad_thres"], cfg["min_steps"], 1, dev(rand))
    assert np.array_equal(fs.cpu().numpy(), w["flag_split"]) and np.array_equal(fr.cpu().numpy(), w["flag_remove"])
    assert {k: rec.counts[i] for k, i in decide.CI.items()} == w["counts"]
    for j, k in enumerate(INIT_LINES):
        check_stat64(rec.stats[j], w["pop"][k], k)


# ---- the cut ---------------------------------------------------------------------------------------------------------

def all_candidates(radii, cand=None):
    """Rows that all pass every test but the ones `cand` clears (through create_steps)."""
    p = radii.shape[0]
    c = {"opacity": np.zeros((p, 1), np.float32), "create_steps": np.full(p, 1000, np.int32),
         "area_sum": np.ones(p, np.int32), "grad_sum": np.ones(p, np.float32), "radii_max_max": radii.astype(np.int32),
         "weights_max": np.ones(p, np.float32), "visible_count": np.zeros(p, np.int16),
         "radius3d_min": np.ones(p, np.float32), "radius3d_max": np.ones(p, np.float32)}
    if cand is not None:
        c["create_steps"][~cand] = 0
    return np.full(p, -1, np.int32), np.zeros(p, np.int8), np.zeros((p, 3), np.float32), c


def cut_case(radii, k, cand=None, where=""):
    node_index, depth, scaling, c = all_candidates(radii, cand)
    cfg = dict(R.DEPTH_CFG, max_split_points=k, radius2d_thres=-1)
    w = R.depth_stage(node_index, depth, c, cfg, 20, 20)
    fs, fr, rec = run_depth(node_index, depth, scaling, c, cfg, 20, 20)
    check_exact(rec, fs, fr, w, where)
    return w, rec


def test_cut_with_k_and_k_plus_one_candidates_and_with_ties():
    p, k = 3000, 40                                   # int(3000 * 0.05) = 150 > k: the cap is max_split_points
    g = np.random.default_rng(1)
    radii = g.permutation(p).astype(np.int32) + 10
    cand = np.zeros(p, bool)
    cand[g.choice(p, k, replace=False)] = True
    w, _ = cut_case(radii, k, cand, "k candidates")
    assert not w["need_cut"] and w["flag_split"].sum() == k
    extra = np.nonzero(~cand)[0][7]
    cand[extra] = True
    w, rec = cut_case(radii, k, cand, "k + 1 candidates")
    assert w["need_cut"] and w["flag_split"].sum() == k and rec.num_split == k
    w, rec = cut_case(np.full(p, 77, np.int32), k, None, "one value")
    assert w["need_cut"] and w["cut_value"] == 77 and w["flag_split"].all() and rec.num_split == p


@pytest.mark.parametrize("kind", ["digit3", "digit2", "digit1", "digit0", "spread", "pixels_4k", "top"])
def test_cut_threshold_in_every_radix_digit(kind):
    """The candidates differ only in one 8-bit digit of the select (so that pass decides), or are spread over all of
    [0, 2^31 - 1], or are pixel counts of a 3840 x 2160 view; `top`: the largest values sit at 2^31 - 1."""
    p = 5000
    g = np.random.default_rng(list(kind.encode()))
    if kind.startswith("digit"):
        shift = 8 * int(kind[5])
        radii = (0x12345678 & ~(0xFF << shift)) | (g.integers(0, 128 if shift == 24 else 256, p) << shift)
    elif kind == "spread":
        radii = g.integers(0, 2 ** 31, p)
    elif kind == "pixels_4k":
        radii = g.integers(0, 3840 * 2160 + 1, p)
    else:
        radii = np.where(g.random(p) < 0.01, 2 ** 31 - 1, g.integers(0, 2 ** 31, p))
    for k in (1, 100, 250):
        w, rec = cut_case(radii.astype(np.int32), k, None, f"{kind} k = {k}")
        assert w["need_cut"] and rec.num_max_split == k and rec.num_split == int(w["flag_split"].sum()) >= k


def test_cut_with_candidates_only_in_the_last_chunk():
    p = 3 * 1024 + 500
    radii = np.random.default_rng(3).integers(0, 1000, p).astype(np.int32)
    cand = np.arange(p) >= 3 * 1024
    w, rec = cut_case(radii, 20, cand, "last chunk")
    assert w["need_cut"] and 20 <= w["flag_split"].sum() < 500 and not w["flag_split"][:3 * 1024].any()


def test_two_runs_give_the_same_bits():
    node_index, depth, scaling, c = synthetic(1024 * 1024 + 1, 5)
    cfg = dict(R.DEPTH_CFG, max_split_points=5000)
    a = run_depth(node_index, depth, scaling, c, cfg, 2, 20)
    b = run_depth(node_index, depth, scaling, c, cfg, 2, 20)
    assert a[2].raw == b[2].raw and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2].need_cut and a[2].stats[0].count > 100000 and a[2].stats[1].std > 0


# ---- composition with the resize -------------------------------------------------------------------------------------

class _Buffers:
    def __init__(self, d):
        self.keys = list(d)
        for k, v in d.items():
            setattr(self, k, v)

    def items(self):
        for k in self.keys:
            yield k, getattr(self, k)


class Counter:
    def __init__(self, c):
        for k in R.COUNTER_INPUTS + ("weights_sum", "radii_max"):
            setattr(self, k, dev(c[k]) if k in c else torch.zeros(c["area_sum"].shape[0], device=DEV))
        self.resets = []

    def reset(self, num_points):                      # LoG/model/counter.py:27-31
        self.resets.append(num_points)
        for key in ['weights_max', 'weights_sum', 'radii_max', 'radii_max_max', 'area_sum', 'grad_sum', 'visible_count']:
            data = getattr(self, key)
            data.set_(torch.zeros((num_points,), device=data.device, dtype=data.dtype))


class TensorTree:
    def __init__(self, t, max_child, max_level):
        for k in R.TREE_KEYS:
            setattr(self, k, dev(t[k]))
        self.max_child, self.max_level = max_child, max_level


class Splitter:
    def __init__(self, n):
        self.N, self.split_method = n, "uniform"


def _reference_shaped(seen):
    """The three resize methods as torch / numpy code of the reference's shape (boolean flags in, row moves by index): the
    tree by densify_ref.tree_update, the rows by densify_ref.plan.  Children copy their parent in every model key (what the
    split does to xyz and scaling is not looked at here)."""
    def tree_sr(self, fs, fr):
        seen.append((fs.cpu().numpy().copy(), fr.cpu().numpy().copy()))
        t = {k: getattr(self, k).cpu().numpy() for k in R.TREE_KEYS}
        ms, mr = D.mask_flags(seen[-1][0], seen[-1][1], t["node_index"], t["index_parent"], t["depth"], self.max_level)
        for k, v in D.tree_update(t, ms, mr, self.max_child).items():
            getattr(self, k).set_(dev(v))
        return dev(ms), dev(mr)

    def rows(fs, fr, remove_split, n):
        _, src_row, nk, _, _ = D.plan(fs.cpu().numpy(), fr.cpu().numpy(), remove_split, n)
        return dev(src_row.astype(np.int64)), nk

    def model_sr(self, model, optimizer, fs, fr, remove_split=True):
        seen.append((fs.cpu().numpy().copy(), fr.cpu().numpy().copy()))
        src, nk = rows(fs, fr, remove_split, self.N)
        for k in model.keys:
            getattr(model, k).set_(getattr(model, k)[src].contiguous())
        for sk in optimizer.state_keys:
            for _, v in getattr(optimizer, sk).items():
                new = v[src].contiguous()
                new[nk:] = 0
                v.set_(new)
        return torch.tensor(nk, device=DEV)

    def other_sr(self, model, keys, fs, fr, remove_split=True):
        src, nk = rows(fs, fr, remove_split, self.N)
        for k in keys:
            new = getattr(model, k)[src].contiguous()
            if k != "radius3d_min":
                new[nk:] = 0
            getattr(model, k).set_(new)
    return tree_sr, model_sr, other_sr


def _clamp_scale(self, index):                       # LoG.clamp_scale (level_of_gaussian.py:367-377)
    scaling = self.gaussian.scaling[index]
    hi = torch.log(self.counter.radius3d_max[index][:, None].expand(-1, 3))
    lo = torch.log(self.counter.radius3d_min[index][:, None].expand(-1, 3))
    self.gaussian.scaling[index] = torch.clamp(scaling, lo, hi)


def log_stand_in(meta, r, cfg, mode, seen):
    """An object with what LoG.update_depth_stage / update_init_stage touch; mode 'device': log_amd.densify's methods,
    'reference': _reference_shaped."""
    from log_amd import densify as dd
    p, c = r["p"], r["c"]
    g = np.random.default_rng(p)
    gaussian = types.SimpleNamespace(
        keys=["scaling", "colors", "xyz", "opacity", "rotation"], xyz_scale=1.0,
        activation=types.SimpleNamespace(opacity_activation=torch.sigmoid, scaling_activation=torch.exp,
                                         scaling_inverse_activation=torch.log, rotation_activation=torch.nn.functional.normalize),
        scaling=dev(r["scaling"]), opacity=dev(c["opacity"]), xyz=dev(g.standard_normal((p, 3)).astype(np.float32)),
        colors=dev(g.random((p, 3)).astype(np.float32)), rotation=dev(g.standard_normal((p, 4)).astype(np.float32)))
    opt = types.SimpleNamespace(state_keys=["exp_avg", "exp_avg_sq"])
    for sk in opt.state_keys:
        setattr(opt, sk, _Buffers({k: torch.ones_like(getattr(gaussian, k)) for k in gaussian.keys}))
    if mode == "device":
        tree_sr, model_sr, other_sr = dd.tree_split_and_remove, dd.split_and_remove, dd.split_and_remove_other
    else:
        tree_sr, model_sr, other_sr = _reference_shaped(seen)
    tree_cls = type("TensorTree", (TensorTree,), {"split_and_remove": tree_sr})
    split_cls = type("Splitter", (Splitter,), {"split_and_remove": model_sr, "split_and_remove_other": other_sr})
    log_cls = type("LoG", (), {"num_points": property(lambda self: self.gaussian.xyz.shape[0]), "clamp_scale": _clamp_scale})
    log = log_cls()
    log.gaussian, log.optimizer, log.counter, log.splitter = gaussian, opt, Counter(c), split_cls(meta["children"])
    log.tree = tree_cls(r["tree_before"], meta["children"], meta.get("max_level", 20)) if r["tree_before"] is not None else None
    log.densify_and_remove = types.SimpleNamespace(**cfg)
    log.current_depth = meta.get("current_depth", 0)
    return log


@pytest.mark.parametrize("mode", ["device", "reference"])
@pytest.mark.parametrize("name", ["decide_depth2", "decide_depth4", "decide_depth8"])
def test_depth_stage_composed_with_the_resize(name, mode):
    """The drop-in on a stand-in LoG, every recorded round: the end state is the fixture's -- tree and counters exactly, the
    radius3d_max of the new children within 2 ulp (one expf) -- and the reference-shaped methods see the fixture's flags."""
    from log_amd import decide
    meta, rounds = fixture(name)
    decide.reset_stats()
    for i, r in enumerate(rounds):
        where = f"{name} round {i} ({mode})"
        seen = []
        log = log_stand_in(meta, r, dict(R.DEPTH_CFG, max_split_points=int(r["max_split_points"])), mode, seen)
        decide.update_depth_stage(log, 100 + i)
        if mode == "reference":
            assert np.array_equal(seen[0][0], r["flag_split"]) and np.array_equal(seen[0][1], r["flag_remove"]), where
        for k in R.TREE_KEYS:
            assert np.array_equal(getattr(log.tree, k).cpu().numpy(), r["after_" + k]), (where, k)
        for k in ("create_steps", "radius3d_min"):
            assert np.array_equal(getattr(log.counter, k).cpu().numpy(), r["after_" + k]), (where, k)
        got, want = log.counter.radius3d_max.cpu().numpy(), r["after_radius3d_max"]
        n_new = meta["children"] * int(r["flag_split"].sum())
        assert n_new > 0 and np.array_equal(got[:-n_new], want[:-n_new]), where
        err = np.abs(got[-n_new:].astype(np.float64) - want[-n_new:]) / np.spacing(want[-n_new:])
        print(where, "radius3d_max tail: worst %.1f ulp" % err.max())
        assert err.max() <= 2, where
        assert log.counter.resets == [want.shape[0]] and log.counter.weights_max.shape[0] == log.num_points == want.shape[0]
    st = decide.stats()
    assert st["calls"] == {"update_depth_stage": 3} and st["readbacks"] == {"update_depth_stage": 3} and st["fallbacks"] == {}


@pytest.mark.parametrize("mode", ["device", "reference"])
@pytest.mark.parametrize("name", R.fixture_names("init"))
def test_init_stage_composed_with_the_resize(name, mode):
    from log_amd import decide
    meta, (r,) = fixture(name)
    seen = []
    log = log_stand_in(meta, r, R.INIT_CFG, mode, seen)
    decide.reset_stats()
    real = torch.rand_like
    torch.rand_like = lambda t, **kw: dev(r["rand"])            # the fixture's draw
    try:
        decide.update_init_stage(log, scale=meta["scale"])
    finally:
        torch.rand_like = real
    if mode == "reference":
        assert np.array_equal(seen[0][0], r["flag_split"]) and np.array_equal(seen[0][1], r["flag_remove"])
    n = int(r["num_points_after"])
    assert log.num_points == n == log.counter.create_steps.shape[0] == log.counter.weights_max.shape[0]
    assert log.counter.resets == [n] and bool((log.counter.radius3d_max == 0.2).all())
    scale = torch.exp(log.gaussian.scaling)
    assert bool((scale <= 0.2 * (1 + 1e-6)).all())                # clamp_scale ran on every row
    assert decide.stats()["fallbacks"] == {} and decide.stats()["readbacks"] == {"update_init_stage": 1}


# ---- fall-backs ------------------------------------------------------------------------------------------------------

def test_every_fallback_reason_is_counted_and_leaves_the_model_alone():
    from log_amd import decide
    meta, rounds = fixture("decide_depth4")
    r = rounds[1]
    imeta, (ir,) = fixture("decide_init_scale1")
    calls = []
    decide.reset_stats()

    def depth(change, **cfg):
        log = log_stand_in(meta, r, dict(R.DEPTH_CFG, **cfg), "device", [])
        change(log)
        before = {k: (getattr(log.tree, k).data_ptr(), getattr(log.tree, k).shape) for k in R.TREE_KEYS}
        before["xyz"] = (log.gaussian.xyz.data_ptr(), log.gaussian.xyz.shape)
        decide.update_depth_stage(log, 3)
        after = {k: (getattr(log.tree, k).data_ptr(), getattr(log.tree, k).shape) for k in R.TREE_KEYS}
        after["xyz"] = (log.gaussian.xyz.data_ptr(), log.gaussian.xyz.shape)
        assert before == after and log.counter.resets == []

    def init(change, **cfg):
        log = log_stand_in(imeta, ir, dict(R.INIT_CFG, **cfg), "device", [])
        change(log)
        decide.update_init_stage(log, scale=1)
        assert log.num_points == ir["p"] and log.counter.resets == []
    with decide.dropins.substituted(update_depth_stage=lambda self, it: calls.append(("depth", it)),
                                    update_init_stage=lambda self, scale=1: calls.append(("init", scale))):
        depth(lambda log: setattr(log.gaussian, "scaling", log.gaussian.scaling.cpu()))
        depth(lambda log: setattr(log.counter, "visible_count", log.counter.visible_count.int()))
        depth(lambda log: setattr(log.gaussian.activation, "scaling_activation", torch.nn.functional.softplus))
        depth(lambda log: None, sort_method="opacity")
        depth(lambda log: setattr(log, "current_depth", 0))               # no is_parent row
        depth(lambda log: None, max_split_points=0)                        # a cut to nothing
        init(lambda log: None, init_split_method="split_by_3d")
        init(lambda log: None, init_radius_split=-1)
        init(lambda log: setattr(log.counter, "weights_max", log.counter.weights_max.cpu()))
        init(lambda log: setattr(log.gaussian.activation, "opacity_activation", torch.tanh))
    assert calls == [("depth", 3)] * 6 + [("init", 1)] * 4
    reasons = decide.stats()["fallbacks"]
    assert set(reasons.values()) == {1} and len(reasons) == 10, reasons
    text = " | ".join(f"{k[0]}: {k[1]}" for k in reasons)
    for want in ("not on the GPU", "visible_count", "sigmoid / exp", "sort_method = 'opacity'", "no is_parent row",
                 "num_max_split == 0", "split_by_3d", "== -1"):
        assert want in text, (want, text)

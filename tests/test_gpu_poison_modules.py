"""Every other module whose Python layer allocates with torch.empty -- the loss family, the depth loss, the evaluation, view
preparation, the densification decisions and moves, the initialisation pass, the pose table, the exchange kernels -- and the
modules whose tests hand over buffers of their own (SH, get_all and the fused step, multi-view accumulation, the counter and the
id histogram, sparse Adam, k-NN, the LoD traverse), at one or two of the smallest edge shapes of each module's own GPU test,
with every hooked allocation filled first (tests/poison.py): once unpoisoned, once under each of the four fills.

Two forms.
  * Where the module's rule is a tolerance against a restatement (losses, evaluation, pose, k-NN): the restatement is computed and
    the unpoisoned result held to it once, by the helpers of the module's own test; the result under every fill must then be
    bit-identical to the unpoisoned one (these kernels use no float atomics: their own tests assert run-to-run identical bits).
  * The other modules (prepare, decide, densify, the initialisation pass, the exchange kernels, get_all, the fused step,
    multi-view sums, counter, id histogram, LoD): a case of the module's own test is run with every call it makes into the
    library's Python layer recorded (poison.spied: what each call returned, and what it left in its arguments).  The unpoisoned
    run is held to the reference by that test's rule; the record under every fill must be the unpoisoned run's bit for bit.
Every poisoned run must have made hooked allocations.  The calls that make none (they work in place on the caller's tensors:
scale clamp, pose step, multi-view step, sparse Adam, the SH entry points on the test's own buffers) are listed in
NO_UNINITIALISED with the reason, and held to making none."""
import importlib

import numpy as np
import pytest
import torch

import poison as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _five(call, ints=None):
    """call() unpoisoned and under each fill -> ({fill: result}, the census of the `nan` run)."""
    out, census = P.run_fills(call, ints=ints, sync=torch.cuda.synchronize)
    return out, census["nan"]


def _identical(what, out):
    bad = P.differing(out)
    assert bad == [], (what, bad)


def _record(what, census):
    print("CENSUS %s: %s; fills %s" % (what, census.summary(), ", ".join(P.FILLS)))


# ---- the loss family ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C,H,W,with_l1", [(1, 3, 11, 11, False), (1, 3, 43, 42, False), (2, 4, 33, 75, True)])
def test_loss(B, C, H, W, with_l1):
    import test_gpu_loss as T
    render, gt = T._pair(B, C, H, W, 10 * B + C)
    rl = (render * 1.03 + 0.01).contiguous() if with_l1 else None
    checked = T._check_against_restatement("B=%d C=%d %dx%d" % (B, C, H, W), render, gt, rl)      # (scalars, grad, grad_l1)
    out, census = _five(lambda: T._run(render, gt, rl)[:3])
    _record("loss-%dx%dx%dx%d%s" % (B, C, H, W, "-render_l1" if with_l1 else ""), census)
    _identical("loss", out)
    assert P.same_bits(list(out[None]), list(checked))


def test_masked_loss_with_a_mask_and_a_gain():
    import masked_loss_ref as mref
    import test_gpu_masked_loss as T
    render, gt, g = T._smooth_pair(2, 37, 53, 11)
    mask = torch.rand(2, 37, 53, device=DEV, generator=g)
    mask[:, 5:20, 10:30] = 1.0
    gain = torch.tensor([[1.1, 0.93, 1.04], [0.9, 1.02, 1.2]], device=DEV)
    fg, bg = (torch.rand(2, 37, 53, device=DEV, generator=g) > 0.3).float(), torch.tensor([0.2, 0.5, 0.8], device=DEV)
    for tag, args in (("gain + mask", (mask, None, None, None, gain)), ("gain + mask + composite", (mask, None, fg, bg, gain))):
        got = T._masked(render, gt, *args)
        T._check_against_restatement(tag, got, mref.masked_loss(render, gt, args[0], args[2], args[3], gain=gain),
                                     mref.masked_loss(render, gt, args[0], args[2], args[3], gain=gain, dtype=torch.float32), render)
        out, census = _five(lambda: [list(x) if isinstance(x, tuple) else x for x in T._masked(render, gt, *args)])
        _record("masked-loss-" + tag.replace(" + ", "-"), census)
        _identical(tag, out)
        assert P.same_bits(out[None], [list(x) if isinstance(x, tuple) else x for x in got])


@pytest.mark.parametrize("n", [1, 3])
def test_depth_loss(n):
    import test_gpu_depth_loss as T
    pred, gt, acc = T._maps(65, 65, 1)
    rows, cols = T._t([0, 1, 0][:n]), T._t([0, 1, 1][:n])
    loss, grad = T._check_against_restatement("65x65 n=%d" % n, pred, gt, acc, rows, cols)
    out, census = _five(lambda: T._run(pred, gt, acc, rows, cols)[1:])
    _record("depth-loss-65x65-n%d" % n, census)
    _identical("depth loss", out)
    assert P.same_bits(out[None][0], grad) and float(out[None][1]) == loss


def test_evaluate():
    import test_gpu_evaluate as T
    from evaluate_ref import evaluate_ref, to_bgr8
    from log_amd import evaluate
    pred, gt = T._random_pair(3, 45, 70, 103)
    dp, dg = pred.to(DEV), gt.to(DEV)

    def call():
        m = evaluate.validation_metrics(dp, dg, fit_gain=True, ssim=True, corrected=True, bgr8=True)
        return dict(record=m.record.cpu().numpy().copy(), corrected=m.corrected.cpu().numpy(), bgr8=np.array(m.bgr8_host()),
                    image=np.array(evaluate.image_to_bgr8(dp))), m.read()

    out, census = _five(call)
    _record("evaluate-3x45x70", census)
    _identical("evaluate", {f: r[0] for f, r in out.items()})
    r64 = evaluate_ref(pred.numpy(), gt.numpy(), fit_gain=True, ssim=True)
    r32 = evaluate_ref(pred.numpy(), gt.numpy(), fit_gain=True, ssim=True, dtype=np.float32)
    res, read = out[None]
    T._check_scalars("C=3", read, r64, r32, True, True)
    T._check_corrected("C=3", res["corrected"], r64, r32)
    assert np.array_equal(res["bgr8"], to_bgr8(np.concatenate([res["corrected"], gt.numpy()], axis=1)))
    assert np.array_equal(res["image"], to_bgr8(pred.numpy()))


def test_pose_camera_and_row_gradient():
    import pose_ref
    import test_gpu_pose as T
    from util import rel_l2
    V, Pm = T._matrices()
    rng = np.random.default_rng(5)
    w = [torch.tensor(rng.standard_normal(s), dtype=torch.float32, device=DEV) for s in ((4, 4), (4, 4), (3,))]

    def call():
        pose = T._table()
        pose.table[2] = torch.tensor(T.XIS["series"], device=DEV)
        Vn, Pn, cp = pose.camera(2, V, Pm)
        sum((a * b).sum() for a, b in zip((Vn, Pn, cp), w)).backward()
        return [Vn.detach(), Pn.detach(), cp.detach(), pose.grad.clone()]

    out, census = _five(call)
    _record("pose-camera", census)
    _identical("pose", out)
    xi = torch.tensor(T.XIS["series"], dtype=torch.float32).double().requires_grad_(True)
    ref = pose_ref.camera(xi, V, Pm)
    want, = torch.autograd.grad(sum((a * b.cpu().double()).sum() for a, b in zip(ref, w)), xi)
    for got, r in zip(out[None][:3], ref):
        assert rel_l2(got.cpu().numpy(), r.detach().numpy()) < T.ROUND_TOL
    assert rel_l2(out[None][3][2].cpu().numpy(), want.numpy()) < T.ROUND_TOL and not out[None][3][[0, 1, 3]].any()


@pytest.mark.parametrize("n", [257, 1025])
def test_knn(n):
    import test_gpu_knn as T
    from simple_knn._C import distCUDA2
    pts = T._box(np.random.default_rng(11 + n), n)
    d = torch.tensor(pts, device=DEV)
    out, census = _five(lambda: distCUDA2(d))
    _record("knn-%d" % n, census)
    _identical("knn", out)
    got, ref = out[None].cpu().numpy(), T._brute(pts)
    assert np.isfinite(got).all() and (np.abs(got - ref) <= T.RTOL * ref).all()


# ---- modules whose own test is bit for bit: its case as it stands, under every fill --------------------------------------------
# (test module, test function, arguments; "oracle" stands for the session's oracle fixture)
BASE_CASES = [
    ("prepare-frustum-65", "test_gpu_prepare", "test_frustum_select_sizes", (65,)),
    ("prepare-frustum-1025", "test_gpu_prepare", "test_frustum_select_sizes", (1025,)),
    ("prepare-frustum-activations", "test_gpu_prepare", "test_frustum_select_activations_and_row_list", ()),
    ("prepare-lod-select", "test_gpu_prepare", "test_lod_select_partition_edges", ()),
    ("decide-depth-1025", "test_gpu_decide", "test_depth_stage_at_the_edges_of_chunks_and_partials", (1025,)),
    ("decide-init-1025", "test_gpu_decide", "test_init_stage_at_the_edges_of_chunks_and_partials", (1025,)),
    ("decide-cut", "test_gpu_decide", "test_cut_with_k_and_k_plus_one_candidates_and_with_ties", ()),
    ("densify-scan", "test_gpu_densify", "test_scan_second_level", ()),
    ("densify-round", "test_gpu_densify", "test_every_recorded_round_replays_on_the_device", ("densify_tree2",)),
    ("init-pass-257x1", "test_gpu_init_pass", "test_radius3d_min_sizes_and_planted_rows", (257, 1)),      # (V = 1: init_radius3d too)
    ("init-pass-257x3", "test_gpu_init_pass", "test_radius3d_min_sizes_and_planted_rows", (257, 3)),
    ("dist-pack-unpack", "test_gpu_dist", "test_pack_and_unpack_rows_kernels", ()),
    ("dist-pack-clear", "test_gpu_dist", "test_pack_and_clear_and_the_zeroing_unpack", ()),
    ("dist-hinted-pack-visible-count", "test_gpu_dist", "test_pack_rows_with_a_hint_and_the_visible_count_kernel", ()),
    ("get-all-K4", "test_gpu_getall", "test_row_lengths_no_reference_configuration_produces", (4, (0, 1))),
    ("get-all-invalid-index", "test_gpu_getall", "test_an_invalid_index_reads_row_zero", (8, 2)),
    ("fused-step-63of65", "test_gpu_train_ops", "test_fused_step_kernel_equals_activation_backward_plus_sparse_adam",
     (2, True, 15, (65, 63), ())),
    ("multi-view-sums-15-2", "test_gpu_multi_view", "test_sums_equal_the_parents_backward_added_by_index",
     (15, 2, False, ("opacity", "rotation"))),
    ("counter", "test_gpu_train_ops", "test_counter_matches_reference_counter_and_oracle", ("oracle",)),
    ("id-histogram-7x13", "test_gpu_train_ops", "test_id_histogram_matches_torch_unique", (5, (7, 13))),
    ("id-histogram-100x100", "test_gpu_train_ops", "test_id_histogram_matches_torch_unique", (70000, (100, 100))),
    ("lod-edge-cases", "test_gpu_lod", "test_traverse_edge_cases", ("oracle",)),
    ("lod-random-tree", "test_gpu_lod", "test_traverse_follows_reference_on_random_trees", (0, "oracle")),
]

# Calls that hand the library no uninitialised memory from the Python layer: they work in place on the caller's tensors (or in
# buffers the test itself fills), so there is nothing to poison.  Held as data: the day one of them starts to allocate with
# torch.empty, the test below fails and asks for a scenario above.
NO_UNINITIALISED = [
    ("prepare-clamp-257", "test_gpu_prepare", "test_clamp_scale_sizes", (257, True), "clamp_scale steps the caller's rows in place"),
    ("pose-step", "test_gpu_pose", "test_step_is_the_corrector_step_at_width_six", (0,),
     "PoseTable.step updates its zero-initialised table, gradient and moments in place"),
    ("sh-edges-M4", "test_gpu_sh_edges", "test_sh_kernels_at_wave_and_workgroup_edges", ("oracle", 4),
     "the test calls lograst_sh_forward / _backward on buffers it fills itself; HipBackend.sh_forward / sh_backward, which "
     "allocate with torch.empty, are poisoned in tests/test_gpu_poison_packages.py: test_native_shs"),
    ("multi-view-step", "test_gpu_multi_view", "test_step_equals_the_parents_sparse_adam_over_all_rows", (15, 2, True, True, None),
     "accumulated_adam steps parameters and moments in place from zero-initialised sums"),
    ("sparse-adam", "test_gpu_train_ops", "test_sparse_adam_matches_reference_optimizer_and_oracle", ("adam_a.npz", "oracle"),
     "the sparse Adam step updates the caller's parameters and moments in place"),
]


@pytest.mark.parametrize("name,module,function,args,why", NO_UNINITIALISED, ids=[c[0] for c in NO_UNINITIALISED])
def test_calls_without_uninitialised_memory_still_make_none(oracle_mod, name, module, function, args, why):
    fn = getattr(importlib.import_module(module), function)
    with P.poisoned("zero") as census:
        fn(*tuple(oracle_mod if a == "oracle" else a for a in args))
        torch.cuda.synchronize()
    assert len(census) == 0, (name, census.entries[:4], "this call now allocates uninitialised memory: give it a poisoned scenario")


def canonical_segments(packed, groups, kmax):
    """A packed buffer of the row-sparse exchange (include/lograst.h: header [16] | values [kmax][16] | index
    [roundup(kmax, 16)] per group) -> (per segment [count, the held rows' indices sorted, their values in that order], did a
    segment overflow): the rows come "in no particular order", what lies behind the held rows is unspecified (EXEMPT), and of a
    group with more than kmax rows WHICH rows were dropped is the arrival order's ("the outputs of an overflowed call": only
    the counts are compared then).  The host form of the buffer (a CPU tensor: kmax rows of values + index) -> as it is."""
    flat = np.asarray(packed, np.float32).reshape(-1)
    if groups == 0 or flat.size % groups or flat.size // groups < 16 + 17 * kmax:
        return flat, False
    seg = flat.reshape(groups, -1)
    counts = [int(s[:1].view(np.int32)[0]) for s in seg]
    if max(counts) > kmax:
        return counts, True
    out = []
    for s, k in zip(seg, counts):
        idx = s[16 + 16 * kmax: 16 + 16 * kmax + k].view(np.int32)
        order = np.argsort(idx, kind="stable")
        out.append([k, idx[order].copy(), s[16: 16 + 16 * kmax].reshape(kmax, 16)[:k][order].copy()])
    return out, False


def _normalise(entry):
    """A recorded call with the exchange's packed buffers in canonical form (in the return value of _pack_segments, in the
    arguments of _unpack_segments).  Of a group with more than kmax rows the pack keeps -- and, packing and clearing, clears --
    whichever kmax arrive first: what such a pack left in `rows` and what an unpack of its buffer wrote follow that choice and
    are left out (the base test holds them: a subset of the rows, each intact).  Every other call as recorded."""
    name, ret, (args, kwargs) = entry
    if name == "log_amd.dist._pack_segments" and isinstance(ret, list):
        canon, overflowed = canonical_segments(ret[0], args[0].shape[0], int(args[1]))
        ret = [canon, ret[1]]
        if overflowed:
            args = [None] + list(args[1:])
    elif name == "log_amd.dist._unpack_segments":
        args = list(args)
        args[1], overflowed = canonical_segments(args[1], int(args[2]), int(args[3]))
        if overflowed:
            args[0], ret = None, None
    return [name, ret, [args, kwargs]]


def _spy_targets():
    """The library's Python layer as the base cases call it: every public function and method of these is recorded."""
    from log_amd import (counter, decide, densify, dist, get_all, init_pass, lod, multi_view, prepare, rasterizer as R,
                         sparse_optimizer)
    return (prepare, lod, decide, densify, init_pass, dist, get_all, counter, sparse_optimizer, multi_view, R.HipBackend)


@pytest.mark.parametrize("name,module,function,args", BASE_CASES, ids=[c[0] for c in BASE_CASES])
def test_base_case_under_every_fill(oracle_mod, name, module, function, args):
    """The base test's case with every call it makes into the library's Python layer recorded: what each call returned and what
    it left in its arguments.  The unpoisoned run is held to the reference by the base test's own rule; the record of every
    poisoned run must be the unpoisoned run's, call for call and bit for bit -- whatever the base test's rule tolerates, and
    whether or not its reference is another path of the library that saw the same fill."""
    fn = getattr(importlib.import_module(module), function)
    args = tuple(oracle_mod if a == "oracle" else a for a in args)

    def call():
        with P.spied(*_spy_targets()) as log:
            fn(*args)
            torch.cuda.synchronize()
        return log

    logs, census = P.run_fills(call)
    _record(name, census["nan"])
    base = logs[None]
    assert len(base) > 0, name
    for fill in P.FILLS:
        assert [e[0] for e in logs[fill]] == [e[0] for e in base], (name, fill)
        for i, (e, e0) in enumerate(zip(map(_normalise, logs[fill]), map(_normalise, base))):
            assert P.same_bits(e[1], e0[1]), (name, fill, i, e[0], "returned")
            assert P.same_bits(e[2], e0[2]), (name, fill, i, e[0], "left in its arguments")
    print("CALLS %s: %s" % (name, ", ".join(sorted({e[0] for e in base}))))


def test_densify_move_rows():
    """Plan.move at 1025 rows, nine keys of every width, type and child mode (tests/test_gpu_densify.py).  The child rows of a
    LOGRAST_MOVE_SKIP key belong to another kernel (EXEMPT of tests/test_gpu_poison_rasterizer.py): compared below num_keep."""
    import densify_ref as D
    import test_gpu_densify as T
    p = 1025
    rng, plan, src_row, nk = T._plan(p, 100 + p)
    srcs = [rng.standard_normal((p, c)).astype(np.float32) for c in (1, 3, 4, 9, 45)]
    srcs += [rng.integers(-2 ** 31, 2 ** 31, (p, 16), dtype=np.int64).astype(np.int32),
             rng.integers(-2 ** 15, 2 ** 15, (p, 3)).astype(np.int16), rng.integers(-128, 128, p).astype(np.int8),
             rng.integers(-128, 128, (p, 5)).astype(np.int8)]
    modes = [D.COPY_PARENT, D.ZERO, D.COPY_PARENT, D.SKIP, D.COPY_PARENT, D.ZERO, D.COPY_PARENT, D.ZERO, D.SKIP]
    want = [D.move_rows(s, src_row, nk, m) for s, m in zip(srcs, modes)]
    dsrc = [T.dev(s) for s in srcs]
    rows = [slice(0, nk) if m == D.SKIP else slice(None) for m in modes]

    def call():
        fresh = T._plan(p, 100 + p)[1]                           # (the plan's own keep_dest / src_row are torch.empty too)
        return [fresh.keep_dest, fresh.src_row] + [o.cpu().numpy()[r] for o, r in zip(fresh.move(list(zip(dsrc, modes))), rows)]

    out, census = _five(call)
    _record("densify-move-1025", census)
    _identical("densify move", out)
    assert 0 < nk < plan.num_new
    for got, w, r in zip(out[None][2:], want, rows):
        assert got.dtype == w.dtype and np.array_equal(got, w[r])

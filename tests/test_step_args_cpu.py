"""The argument surface of the row-step entry points (lograst_gather_activate, lograst_activate_backward, its _adam and
_accumulate forms, lograst_sparse_adam, lograst_accumulated_adam; log_amd/csrc/api.hip), pinned as a literal table:
(entry point, one fault) -> return code and a fragment of the message.  Every row fails a check before any device work -- or
returns at the empty input -- so the pointers are never dereferenced and the table runs without a GPU.  A call that passes
every check would launch, so the table has no such row: what is no fault (a key that is left out, whatever its other fields
say) is shown by a row that plants one fault behind it.

Throughout: 5 rows of a model of 9, 3 SH coefficients stored, degree 1 active."""
import ctypes

import pytest

OK, ERR_ARG = 0, -1
P, Q = 0x1000, 0x2000                                        # never dereferenced, 16-byte aligned
N, NUM_POINTS, K, DEG = 5, 9, 3, 1
WIDTHS = (3, 3, 1, 4, 3, 3 * K)                              # xyz, scaling, opacity, rotation, colors, shs
KEY_NAMES = ("xyz", "scaling", "opacity", "rotation", "colors", "shs")


def adam_keys(count=6, widths=WIDTHS, **change):
    """`count` keys with every pointer set; change: k<i>=dict(field=value) for key i."""
    from log_amd import _lib
    keys = (_lib.LograstAdamKey * count)()
    for i, k in enumerate(keys):
        k.model_param, k.param, k.grad, k.exp_avg, k.exp_avg_sq, k.max_exp_avg_sq = P, Q, Q, P, P, None
        k.width, k.step_size = widths[i % 6], 1e-3
    for name, fields in change.items():
        for f, v in fields.items():
            setattr(keys[int(name[1:])], f, v)
    return keys


def targets(**change):
    """six targets, rows exactly their width apart; change: t<i>=dict(field=value)."""
    from log_amd import _lib
    t = (_lib.LograstAccTarget * 6)()
    for i, s in enumerate(t):
        s.base, s.row_stride_floats = P, WIDTHS[i]
    for name, fields in change.items():
        for f, v in fields.items():
            setattr(t[int(name[1:])], f, v)
    return t


def strides(*v):
    return (ctypes.c_int32 * 6)(*(v or WIDTHS))


_RAW = "n raw_xyz raw_scaling raw_opacity raw_rotation sh_coeffs active_degree camera_center "
_UPS = "dl_dact_scaling dl_dact_opacity dl_dact_rotation dl_dact_colors "
_ADAM = "beta1 beta2 bc2_sqrt eps "
# per entry point: the parameters in the order of the C signature
ORDER = {
    "gather_activate": "n num_points index xyz scaling opacity rotation colors shs sh_coeffs active_degree camera_center "
                       "out_xyz out_scaling out_opacity out_rotation out_colors out_shs act_scaling act_opacity act_rotation "
                       "act_colors stream",
    "activate_backward": _RAW + _UPS + "dl_dscaling dl_dopacity dl_drotation dl_dcolors dl_dshs stream",
    "activate_backward_adam": _RAW + "dl_dact_xyz " + _UPS + "num_points index radii keys " + _ADAM + "stream",
    "activate_backward_accumulate": _RAW + "dl_dact_xyz " + _UPS + "num_points index radii targets seen stream",
    "sparse_adam": "m num_points index flag_vis num_keys keys " + _ADAM + "stream",
    "accumulated_adam": "num_points seen keys grad_strides " + _ADAM + "moved_out stream",
}
SCALARS = dict(n=N, m=N, num_points=NUM_POINTS, sh_coeffs=K, active_degree=DEG, num_keys=6, beta1=0.9, beta2=0.999,
               bc2_sqrt=0.07, eps=1e-15, stream=None, moved_out=None)
STRUCTS = ("keys", "targets", "grad_strides")                # built per call (the library must be loaded first)
POINTERS = {e: tuple(p for p in ORDER[e].split() if p not in SCALARS and p not in STRUCTS) for e in ORDER}

ALL = tuple(ORDER)
GA = ("gather_activate", "activate_backward", "activate_backward_adam", "activate_backward_accumulate")   # lr_ga_check
ROWS_OF_MODEL = ("activate_backward_adam", "activate_backward_accumulate")
STEPS = ("activate_backward_adam", "sparse_adam", "accumulated_adam")                                     # lograst_adam_key

ALIGN = {
    "gather_activate": (("rotation", "out_rotation", "act_rotation"),
                        b"rotation / raw_rotation / act_rotation must be 16-byte aligned"),
    "activate_backward": (("raw_rotation", "dl_dact_rotation", "dl_drotation"),
                          b"raw_rotation / dl_dact_rotation / dl_drotation must be 16-byte aligned"),
    "activate_backward_adam": (("raw_rotation", "dl_dact_rotation"), b"raw_rotation / dl_dact_rotation must be 16-byte aligned"),
    "activate_backward_accumulate": (("raw_rotation", "dl_dact_rotation"),
                                     b"raw_rotation / dl_dact_rotation must be 16-byte aligned"),
}
# pointers that may be NULL (or have a message of their own) in a call that is good otherwise
NOT_IN_NULL_CLASS = {"gather_activate": ("shs", "out_shs", "camera_center"), "activate_backward": ("dl_dshs", "camera_center"),
                     "activate_backward_adam": ("camera_center",), "activate_backward_accumulate": ("camera_center",),
                     "sparse_adam": (), "accumulated_adam": ()}
ADAM_WIDTHS = b"lograst_activate_backward_adam: key widths are 3, 3, 1, 4, 3, 3 * sh_coeffs (xyz, scaling, opacity, rotation, colors, shs)"
STEP_WIDTHS = b"lograst_accumulated_adam: key widths are 3, 3, 1, 4, 3, 3 * sh_coeffs (xyz, scaling, opacity, rotation, colors, shs)"
TARGET_STRIDE = (b"lograst_activate_backward_accumulate: a target's row stride is smaller than its key's width "
                 b"(3, 3, 1, 4, 3, 3 * sh_coeffs)")
GRAD_STRIDE = b"lograst_accumulated_adam: a gradient row stride is smaller than its key's width"
EVERYTHING_NULL = {e: {p: None for p in POINTERS[e] + tuple(s for s in STRUCTS if s in ORDER[e].split())} for e in ORDER}

# (entry points, the fault, what the row changes in the good call, return code, message fragment or None)
TABLE = [
    # ---- counts and SH geometry (lr_ga_check), before anything else
    (GA, "negative n", dict(n=-1), ERR_ARG, b"negative row count"),
    (GA, "sh_coeffs 16", dict(sh_coeffs=16), ERR_ARG, b"sh_coeffs must be 0..15 (degree <= 3)"),
    (GA, "sh_coeffs -1", dict(sh_coeffs=-1), ERR_ARG, b"sh_coeffs must be 0..15 (degree <= 3)"),
    (GA, "degree 4", dict(sh_coeffs=15, active_degree=4), ERR_ARG, b"active SH degree must be 0..3"),
    (GA, "degree -1", dict(active_degree=-1), ERR_ARG, b"active SH degree must be 0..3"),
    (GA, "degree 2 with sh_coeffs 3", dict(active_degree=2), ERR_ARG, b"shs holds fewer coefficients than the active degree needs"),
    (GA, "degree 3 with sh_coeffs 14", dict(sh_coeffs=14, active_degree=3), ERR_ARG,
     b"shs holds fewer coefficients than the active degree needs"),
    (GA, "camera_center NULL at degree 1", dict(camera_center=None), ERR_ARG, b"camera_center is NULL"),
    (GA, "no rows, camera_center NULL at degree 1", dict(n=0, camera_center=None), ERR_ARG, b"camera_center is NULL"),
    (("sparse_adam",), "negative m", dict(m=-1), ERR_ARG, b"negative count"),
    (("sparse_adam", "accumulated_adam"), "negative num_points", dict(num_points=-1), ERR_ARG, b"negative count"),
    (("gather_activate",), "num_points 0 with rows", dict(num_points=0), ERR_ARG, b"rows requested from an empty model"),
    (ROWS_OF_MODEL, "num_points 0 with rows", dict(num_points=0), ERR_ARG, b"rows of an empty model"),
    (("sparse_adam",), "num_keys 9", dict(num_keys=9), ERR_ARG, b"at most 8 keys per call"),
    (("sparse_adam",), "num_keys -1", dict(num_keys=-1), ERR_ARG, b"at most 8 keys per call"),
    # ---- nothing to do: returns before a pointer is looked at
    (GA, "no rows, everything NULL", dict(n=0, sh_coeffs=0, active_degree=0, num_points=0), OK, None),
    (GA, "no rows, degree 0 of 15, everything NULL", dict(n=0, sh_coeffs=15, active_degree=0), OK, None),
    (("sparse_adam",), "no rows, everything NULL", dict(m=0), OK, None),
    (("sparse_adam",), "no keys, everything NULL", dict(num_keys=0), OK, None),
    (("accumulated_adam",), "empty model, everything NULL", dict(num_points=0), OK, None),
    # ---- the SH blocks of the gather have a message of their own
    (("gather_activate",), "shs NULL", dict(shs=None), ERR_ARG, b"NULL shs pointer"),
    (("gather_activate",), "raw shs NULL", dict(out_shs=None), ERR_ARG, b"NULL shs pointer"),
    # ---- the key and target lists
    (STEPS, "keys NULL", dict(keys=None), ERR_ARG, b"NULL pointer"),
    (("activate_backward_accumulate",), "targets NULL", dict(targets=None), ERR_ARG, b"NULL pointer"),
    (("accumulated_adam",), "gradient strides NULL", dict(grad_strides=None), ERR_ARG, b"NULL pointer"),
    (("sparse_adam",), "width 0", dict(keys=("adam_keys", dict(k2=dict(width=0)))), ERR_ARG, b"key width must be >= 1"),
    (("sparse_adam",), "eighth key, width -3", dict(num_keys=8, keys=("adam_keys", dict(count=8, k7=dict(width=-3)))), ERR_ARG,
     b"key width must be >= 1"),
    (("activate_backward_adam",), "shs key at degree 0", dict(active_degree=0, camera_center=None), ERR_ARG,
     b"shs key without active SH coefficients"),
    (("activate_backward_adam",), "shs key without coefficients",
     dict(sh_coeffs=0, active_degree=0, keys=("adam_keys", dict(k5=dict(width=0)))), ERR_ARG,
     b"shs key without active SH coefficients"),
    (("activate_backward_accumulate",), "shs target without coefficients", dict(sh_coeffs=0, active_degree=0), ERR_ARG,
     b"shs target without SH coefficients"),
    (("accumulated_adam",), "shs width 48", dict(keys=("adam_keys", dict(k5=dict(width=48))), grad_strides=(3, 3, 1, 4, 3, 48)),
     ERR_ARG, STEP_WIDTHS),
    (("accumulated_adam",), "shs width 0", dict(keys=("adam_keys", dict(k5=dict(width=0)))), ERR_ARG, STEP_WIDTHS),
    (("accumulated_adam",), "shs width 10", dict(keys=("adam_keys", dict(k5=dict(width=10))), grad_strides=(3, 3, 1, 4, 3, 10)),
     ERR_ARG, STEP_WIDTHS),
    # ... a key that is left out is not looked at: the call goes on to the next fault
    (("activate_backward_adam",), "key left out with a wrong width and NULLs, raw_rotation misaligned",
     dict(keys=("adam_keys", dict(k1=dict(model_param=None, width=99, param=None, exp_avg=None))), raw_rotation=P + 4), ERR_ARG,
     ALIGN["activate_backward_adam"][1]),
    (("activate_backward_accumulate",), "target left out with stride 0, raw_rotation misaligned",
     dict(targets=("targets", dict(t3=dict(base=None, row_stride_floats=0))), raw_rotation=P + 4), ERR_ARG,
     ALIGN["activate_backward_accumulate"][1]),
    (("accumulated_adam",), "key left out with a wrong width and stride 0, next key's stride short",
     dict(keys=("adam_keys", dict(k0=dict(model_param=None, width=99, grad=None))), grad_strides=(0, 2, 1, 4, 3, 9)), ERR_ARG,
     GRAD_STRIDE),
    # ... and so is max_exp_avg_sq, the grad of the fused step and the param of the accumulated one
    (("activate_backward_adam",), "grad NULL and amsgrad are no fault, dl_dact_rotation misaligned",
     dict(keys=("adam_keys", dict(k0=dict(grad=None, max_exp_avg_sq=Q))), dl_dact_rotation=P + 8), ERR_ARG,
     ALIGN["activate_backward_adam"][1]),
    (("accumulated_adam",), "param NULL and amsgrad are no fault, stride short",
     dict(keys=("adam_keys", dict(k0=dict(param=None, max_exp_avg_sq=Q))), grad_strides=(3, 3, 1, 4, 3, 8)), ERR_ARG,
     GRAD_STRIDE),
]
# ---- each NULL pointer class and each misaligned quaternion block
for _e in ALL:
    for _p in POINTERS[_e]:
        if _p not in NOT_IN_NULL_CLASS[_e]:
            TABLE.append(((_e,), _p + " NULL", {_p: None}, ERR_ARG, b"NULL pointer"))
for _e, (_ptrs, _words) in ALIGN.items():
    for _p in _ptrs:
        TABLE.append(((_e,), _p + " misaligned by 4", {_p: P + 4}, ERR_ARG, _words))
        TABLE.append(((_e,), _p + " misaligned by 8", {_p: Q + 8}, ERR_ARG, _words))
# ---- per key: wrong width, NULL inside the key, strides below the width
for _i, _k in enumerate(KEY_NAMES):
    _w = WIDTHS[_i]
    for _wrong in (_w - 1, _w + 1):
        TABLE.append((("activate_backward_adam",), f"{_k} width {_wrong}", dict(keys=("adam_keys", {f"k{_i}": dict(width=_wrong)})),
                      ERR_ARG, ADAM_WIDTHS))
        if _k != "shs":                                      # (any multiple of 3 up to 45 is a width of shs there)
            TABLE.append((("accumulated_adam",), f"{_k} width {_wrong}",
                          dict(keys=("adam_keys", {f"k{_i}": dict(width=_wrong)}), grad_strides=(9,) * 6), ERR_ARG, STEP_WIDTHS))
    for _entry, _fields in (("sparse_adam", ("model_param", "param", "grad", "exp_avg", "exp_avg_sq")),
                            ("activate_backward_adam", ("param", "exp_avg", "exp_avg_sq")),
                            ("accumulated_adam", ("grad", "exp_avg", "exp_avg_sq"))):
        for _f in _fields:
            TABLE.append(((_entry,), f"{_k} {_f} NULL", dict(keys=("adam_keys", {f"k{_i}": {_f: None}})), ERR_ARG,
                          b"NULL pointer in key"))
    TABLE.append((("activate_backward_accumulate",), f"{_k} target stride {_w - 1}",
                  dict(targets=("targets", {f"t{_i}": dict(row_stride_floats=_w - 1)})), ERR_ARG, TARGET_STRIDE))
    TABLE.append((("accumulated_adam",), f"{_k} gradient stride {_w - 1}",
                  dict(grad_strides=tuple(w - (j == _i) for j, w in enumerate(WIDTHS))), ERR_ARG, GRAD_STRIDE))
ROWS = [(entry, fault, change, rc, words) for entries, fault, change, rc, words in TABLE for entry in entries]
_MAKE = {"adam_keys": adam_keys, "targets": targets}


def _call(L, entry, fault, change):
    names = ORDER[entry].split()
    args = {**SCALARS, **{p: P for p in POINTERS[entry]}, "keys": ("adam_keys", {}), "targets": ("targets", {}), "grad_strides": ()}
    if "everything NULL" in fault:
        args.update(EVERYTHING_NULL[entry])
    assert set(change) <= set(args), change
    args.update({k: v for k, v in change.items() if k in names})
    for s in ("keys", "targets"):
        if isinstance(args[s], tuple):
            args[s] = _MAKE[args[s][0]](**args[s][1])
    if isinstance(args["grad_strides"], tuple):
        args["grad_strides"] = strides(*args["grad_strides"])
    return getattr(L, "lograst_" + entry)(*(args[n] for n in names))


def test_the_table_covers_every_entry_point_and_every_pointer():
    assert {e for entries, *_ in TABLE for e in entries} == set(ALL)
    from log_amd import _lib
    for e in ALL:
        assert len(ORDER[e].split()) == len(_lib._SIGNATURES["lograst_" + e][1]), e
        nulled = {next(iter(c)) for entries, f, c, *_ in TABLE if e in entries and f.endswith(" NULL") and len(c) == 1}
        assert nulled >= set(POINTERS[e]) - set(NOT_IN_NULL_CLASS[e]), e
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("entry,fault,change,rc,words", ROWS, ids=[f"{r[0]}-{r[1]}".replace(" ", "_") for r in ROWS])
def test_one_fault_one_message(entry, fault, change, rc, words):
    from log_amd import _lib
    L = _lib.lib()
    got = _call(L, entry, fault, change)
    assert got == rc, (got, L.lograst_last_error())
    if words is not None:
        assert words in L.lograst_last_error(), L.lograst_last_error()

"""The argument checks of the six backward entry points, without a GPU: lograst_backward, _aux, _camera, _abs and
lograst_project_backward, _camera.

Every call carries fake 64-byte-aligned addresses and exactly one fault, so it is refused before any launch; each row holds
the return code and the WHOLE text of lograst_last_error.  The rows cover every check of the two bodies behind the entry
points (api.hip: lr_backward, lr_project_backward) on every entry point that reaches it: the view, the count, each pointer of
the NULL lists, the three alignments, LOGRAST_BWD_CONIC_TOUCHED_ONLY and LOGRAST_BWD_SCRATCH_ZEROED without point_weight, the
rules of the row-major sink, and the list of each extra (aux channels, camera gradients, absolute sums).  n == 0 is
LOGRAST_OK on the four entry points that launch nothing for it (the two camera ones clear their matrices)."""
import ctypes

import pytest

OK, ERR_ARG = 0, -1
PTR = 0x10000                 # never dereferenced; 64-byte aligned
N = 2000
ZEROED, ACCUMULATE, TOUCHED_ONLY, ACCUMULATE_ROWS = 1, 2, 4, 8

COMMON = ["means3d", "scales", "rotations", "radii", "geom", "tile_state", "point_list", "final_t", "n_contrib", "dl_dimage",
          "dl_dmeans2d", "bwd_rows", "dl_dopacities", "dl_dcolors", "dl_dmeans3d", "dl_dscales", "dl_drotations", "point_weight",
          "flags"]
CAMERA = ["dl_dviewmatrix", "dl_dprojmatrix", "camera_scratch", "camera_scratch_bytes"]
PROJECT = ["means3d", "scales", "rotations", "radii", "dl_dmeans2d", "dl_dconic", "dl_dmeans3d", "dl_dscales", "dl_drotations"]
PARAMS = {   # behind (view, n), in front of the stream: include/lograst.h
    "lograst_backward": COMMON,
    "lograst_backward_aux": COMMON[:9] + ["aux_colors", "dl_dimage", "dl_daux_image", "dl_dmeans2d", "bwd_rows", "bwd_row_floats",
                                          "dl_dopacities", "dl_dcolors", "dl_daux_colors"] + COMMON[14:],
    "lograst_backward_camera": COMMON + CAMERA,
    "lograst_backward_abs": COMMON + ["dl_dmeans2d_abs"],
    "lograst_project_backward": PROJECT,
    "lograst_project_backward_camera": PROJECT + CAMERA,
}
BACKWARD = [e for e in PARAMS if "project" not in e]
BOTH_PROJECT = [e for e in PARAMS if "project" in e]
EVERY = list(PARAMS)


def _call(entry, view=None, n=N, **over):
    """-> (return code, lograst_last_error): `entry` with a sound view and sound fake arguments, but for `view` (fields of
    the view) and `over` (arguments by name; view=False: a NULL view)."""
    from log_amd import _lib
    L = _lib.lib()
    v = _lib.LograstView()
    v.width, v.height, v.tanfovx, v.tanfovy, v.scale_modifier = 64, 64, 0.5, 0.5, 1.0
    v.filter_mode, v.ndc_cull, v.extras = 2, 1, 1
    v.viewmatrix = v.projmatrix = v.bg = PTR
    for k, val in (view or {}).items():
        setattr(v, k, val)
    values = {"flags": ZEROED, "bwd_row_floats": 16, "camera_scratch_bytes": L.lograst_camera_scratch_bytes(n)}
    unknown = set(over) - set(PARAMS[entry])
    assert not unknown, unknown
    values.update(over)
    args = [values.get(name, PTR) for name in PARAMS[entry]]
    rc = getattr(L, entry)(None if view is False else ctypes.byref(v), n, *args, None)
    return rc, L.lograst_last_error()


COV3D = dict(cov3d_precomp=PTR, dl_dcov3d=PTR)
BAND = dict(tile_row_begin=1, tile_row_end=3)
ROWS_SINK = ZEROED | ACCUMULATE_ROWS
NULL_POINTER = b"NULL pointer"
AUX_FRESH = b"lograst_backward_aux writes fresh gradients (no LOGRAST_BWD_ACCUMULATE / _ROWS form)"
CAM_FRESH = b"camera gradients come with fresh gradients only (no LOGRAST_BWD_ACCUMULATE / _ROWS form)"
ABS_FRESH = b"lograst_backward_abs writes fresh gradients (no LOGRAST_BWD_ACCUMULATE / _ROWS form)"
CAM_SCRATCH = b"camera scratch is NULL or smaller than lograst_camera_scratch_bytes(n)"

# (what, the entry points it is run on, fields of the view, arguments, the error text)
ROWS = [
    ("view NULL", EVERY, False, {}, b"view is NULL"),
    ("negative count", EVERY, {}, dict(n=-1), b"negative Gaussian count"),
    # the NULL lists
    *[(name + " NULL", BACKWARD, {}, {name: None}, NULL_POINTER)
      for name in ("means3d", "radii", "geom", "tile_state", "final_t", "n_contrib", "dl_dmeans2d", "bwd_rows", "dl_dmeans3d",
                   "dl_dopacities", "dl_dcolors", "scales", "rotations", "dl_dscales", "dl_drotations")],
    ("dl_dimage NULL", [e for e in BACKWARD if e != "lograst_backward_aux"], {}, dict(dl_dimage=None), NULL_POINTER),
    *[(name + " NULL", BOTH_PROJECT, {}, {name: None}, NULL_POINTER) for name in PROJECT],
    ("cov3d_precomp without dl_dcov3d", ["lograst_backward", "lograst_project_backward"], dict(cov3d_precomp=PTR), {},
     b"cov3d_precomp is set but dl_dcov3d is NULL"),
    # the three alignments
    ("rotations misaligned", BACKWARD, {}, dict(rotations=PTR + 4), b"rotations / dl_drotations must be 16-byte aligned"),
    ("dl_drotations misaligned", BACKWARD, {}, dict(dl_drotations=PTR + 8), b"rotations / dl_drotations must be 16-byte aligned"),
    ("bwd_rows misaligned", BACKWARD, {}, dict(bwd_rows=PTR + 16), b"bwd_rows must be 64-byte aligned (one accumulator row per line)"),
    *[(name + " misaligned", BOTH_PROJECT, {}, {name: PTR + 4}, b"rotations / dl_dconic / dl_drotations must be 16-byte aligned")
      for name in ("rotations", "dl_dconic", "dl_drotations")],
    # the flags that need point_weight
    ("touched-only without point_weight", BACKWARD, {}, dict(flags=ZEROED | TOUCHED_ONLY, point_weight=None),
     b"LOGRAST_BWD_CONIC_TOUCHED_ONLY needs point_weight"),
    # the row-major sink (lograst_backward alone: the extras refuse the flag)
    ("sink rows: cov3d_precomp", ["lograst_backward"], COV3D, dict(flags=ROWS_SINK), b"LOGRAST_BWD_ACCUMULATE_ROWS has no cov3d_precomp form"),
    ("sink rows: scales NULL", ["lograst_backward"], {}, dict(flags=ROWS_SINK, scales=None), b"scales / rotations are NULL"),
    ("sink rows: rotations NULL", ["lograst_backward"], {}, dict(flags=ROWS_SINK, rotations=None), b"scales / rotations are NULL"),
    ("sink rows: rows misaligned", ["lograst_backward"], {}, dict(flags=ROWS_SINK, dl_dmeans3d=PTR + 16),
     b"LOGRAST_BWD_ACCUMULATE_ROWS: the gradient rows must be 64-byte aligned"),
    ("sink rows: rotations misaligned", ["lograst_backward"], {}, dict(flags=ROWS_SINK, rotations=PTR + 4), b"rotations must be 16-byte aligned"),
    ("sink rows: dl_dmeans3d NULL", ["lograst_backward"], {}, dict(flags=ROWS_SINK, dl_dmeans3d=None), NULL_POINTER),
    # aux channels
    ("aux: band view", ["lograst_backward_aux"], BAND, {}, b"aux channels render whole images only (tile_row_begin / tile_row_end)"),
    ("aux: cov3d_precomp", ["lograst_backward_aux"], COV3D, {}, b"aux channels have no cov3d_precomp form"),
    ("aux: aux_colors NULL", ["lograst_backward_aux"], {}, dict(aux_colors=None), b"aux_colors / dl_daux_colors are NULL"),
    ("aux: dl_daux_colors NULL", ["lograst_backward_aux"], {}, dict(dl_daux_colors=None), b"aux_colors / dl_daux_colors are NULL"),
    ("aux: both image gradients NULL", ["lograst_backward_aux"], {}, dict(dl_dimage=None, dl_daux_image=None),
     b"dl_dimage and dl_daux_image are both NULL"),
    ("aux: short rows", ["lograst_backward_aux"], {}, dict(bwd_row_floats=9),
     b"bwd_rows must hold LOGRAST_BWD_ROW_FLOATS (16) floats per Gaussian (dL/daux_colors: slots 9..11)"),
    ("aux: running sums", ["lograst_backward_aux"], {}, dict(flags=ZEROED | ACCUMULATE), AUX_FRESH),
    ("aux: row-major running sums", ["lograst_backward_aux"], {}, dict(flags=ROWS_SINK), AUX_FRESH),
    # camera gradients
    ("camera: running sums", ["lograst_backward_camera"], {}, dict(flags=ZEROED | ACCUMULATE), CAM_FRESH),
    ("camera: row-major running sums", ["lograst_backward_camera"], {}, dict(flags=ROWS_SINK), CAM_FRESH),
    *[(what, ["lograst_backward_camera", "lograst_project_backward_camera"], view, over, text) for what, view, over, text in (
        ("camera: cov3d_precomp", COV3D, {}, b"camera gradients have no cov3d_precomp form"),
        ("camera: band view", BAND, {}, b"camera gradients are summed over whole images only (tile_row_begin / tile_row_end)"),
        ("camera: dl_dviewmatrix NULL", {}, dict(dl_dviewmatrix=None), b"dl_dviewmatrix / dl_dprojmatrix are NULL"),
        ("camera: dl_dprojmatrix NULL", {}, dict(dl_dprojmatrix=None), b"dl_dviewmatrix / dl_dprojmatrix are NULL"),
        ("camera: scratch NULL", {}, dict(camera_scratch=None), CAM_SCRATCH),
        ("camera: scratch one row short", {}, dict(camera_scratch_bytes=96 + 64 * 24 * 8), CAM_SCRATCH),
        ("camera: scratch misaligned", {}, dict(camera_scratch=PTR + 4), b"camera scratch must be 8-byte aligned"))],
    # absolute sums
    ("abs: dl_dmeans2d_abs NULL", ["lograst_backward_abs"], {}, dict(dl_dmeans2d_abs=None), b"dl_dmeans2d_abs is NULL"),
    ("abs: dl_dmeans2d_abs NULL, n == 0", ["lograst_backward_abs"], {}, dict(n=0, dl_dmeans2d_abs=None), b"dl_dmeans2d_abs is NULL"),
    ("abs: running sums", ["lograst_backward_abs"], {}, dict(flags=ZEROED | ACCUMULATE), ABS_FRESH),
    ("abs: row-major running sums", ["lograst_backward_abs"], {}, dict(flags=ROWS_SINK), ABS_FRESH),
    ("abs: cov3d_precomp", ["lograst_backward_abs"], COV3D, {}, b"lograst_backward_abs has no cov3d_precomp form"),
    ("abs: band view", ["lograst_backward_abs"], BAND, {}, b"lograst_backward_abs: whole images only (tile_row_begin / tile_row_end)"),
]
CASES = [(entry, what, view, over, text) for what, entries, view, over, text in ROWS for entry in entries]


@pytest.mark.parametrize("entry,what,view,over,text", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_one_fault_is_refused_with_its_text(entry, what, view, over, text):
    rc, msg = _call(entry, view, **over)
    assert (rc, msg) == (ERR_ARG, text)


@pytest.mark.parametrize("entry", BACKWARD)
def test_zeroed_scratch_of_a_large_input_needs_point_weight(entry):
    """LOGRAST_BWD_SCRATCH_ZEROED after a forward with extras on a large input: only the contributing Gaussians' rows were
    cleared.  LOGRAST_HELPER_MIN_N lowered, so that N is a large input; at the default the same call passes this check (and
    would go on to the launches: not made here)."""
    from log_amd import _lib
    L = _lib.lib()
    assert L.lograst_set_knob(b"LOGRAST_HELPER_MIN_N", N) == OK
    try:
        rc, msg = _call(entry, point_weight=None)
    finally:
        assert L.lograst_reset_knobs() == OK
    assert (rc, msg) == (ERR_ARG, b"LOGRAST_BWD_SCRATCH_ZEROED after a forward with view.extras and n >= LOGRAST_HELPER_MIN_N: "
                                  b"dL/dconic is cleared for contributing Gaussians only, pass point_weight "
                                  b"(+ LOGRAST_BWD_CONIC_TOUCHED_ONLY)")


@pytest.mark.parametrize("entry", [e for e in EVERY if "camera" not in e])
def test_no_gaussians_is_ok_and_launches_nothing(entry):
    rc, msg = _call(entry, n=0)
    assert rc == OK, msg

"""CPU checks of the drop-in boundary: the C-ABI library loads without a GPU, exports every symbol that
include/lograst.h declares, the ctypes binding covers all of them, and the product path refuses to run on CPU
tensors (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "lograst.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lograst_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from log_amd import _lib
    names = _declared()
    assert len(names) >= 15
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/lograst.h but not exported by liblograst.so"
    assert set(names) == set(_lib.EXPORTS), set(names) ^ set(_lib.EXPORTS)


def test_sizing_helpers_and_error_text_work_without_gpu():
    from log_amd import _lib
    L = _lib.lib()
    assert L.lograst_version() == 4
    tiles = 120 * 68
    assert L.lograst_tile_state_bytes(1920, 1080, 1000000) >= 4 * (tiles + 1)
    # records + fill records + an index each (band views), rounded up to 64 bytes, + the rank rows of the 5..16-tile rects
    # (8 bytes per Gaussian of the padded batches: round 5)
    assert L.lograst_geom_bytes(10) == (10 * (64 + 16 + 4) + 63) // 64 * 64 + 8 * 10 + 8 * 32768
    assert L.lograst_geom_bytes(30_000_000) < 30_000_000 * 93 + (1 << 20)
    assert L.lograst_keys_bytes(7) == 2 * 56 and L.lograst_list_bytes(7) == 28   # keys + the sort scratch half
    # argument validation happens before any device work
    rc = L.lograst_compute_radius(-1, None, None, None, None, None, 1.0, 1.0, 1.0, 1.0, None, None)
    assert rc < 0 and b"negative" in L.lograst_last_error()
    assert [L.lograst_kernel_name(i) for i in range(3)] == [b"compute_radius", b"project", b"scan_tiles"]


def test_product_path_has_no_cpu_fallback():
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    from log_amd import _lib
    from log_amd.compute_radius import compute_radius_module
    from simple_knn._C import distCUDA2
    rs = GaussianRasterizationSettings(image_height=32, image_width=32, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3),
                                       scale_modifier=1., viewmatrix=torch.eye(4), projmatrix=torch.eye(4),
                                       sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False)
    r = GaussianRasterizer(raster_settings=rs)
    z = torch.zeros
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        r(means3D=z(2, 3), means2D=z(2, 3), shs=None, colors_precomp=z(2, 3), opacities=z(2, 1), scales=z(2, 3) + 1,
          rotations=z(2, 4) + 1, cov3D_precomp=None)
    with pytest.raises(_lib.LograstError):
        compute_radius_module.compute_radius(z(2, 3), z(2, 3), z(2, 4), torch.eye(4), torch.eye(4), 1., 1., 1., 1.)
    with pytest.raises(_lib.LograstError):
        distCUDA2(z(8, 3))
    # the product package does not import the oracle
    import sys
    import log_amd.rasterizer  # noqa: F401
    src = "".join(open(os.path.join(ROOT, "log_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "log_amd"))
                  if f.endswith(".py"))
    assert "import oracle" not in src and "from oracle" not in src
    del sys


def test_reference_error_strings():
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(32, 32, 0.5, 0.5, torch.zeros(3), 1., torch.eye(4), torch.eye(4), 0,
                                       torch.zeros(3), False, False)
    r = GaussianRasterizer(raster_settings=rs)
    z = torch.zeros
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=z(2, 3), means2D=z(2, 3), opacities=z(2, 1), scales=z(2, 3), rotations=z(2, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=z(2, 3), means2D=z(2, 3), opacities=z(2, 1), colors_precomp=z(2, 3))


def test_header_is_plain_c(tmp_path):
    """include/lograst.h is the drop-in boundary for hosts that are not Python: it must compile as C99 on its own."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        import pytest
        pytest.skip("no gcc")
    src = tmp_path / "h.c"
    src.write_text('#include "lograst.h"\nint main(void) { lograst_view v; lograst_adam_key k; (void)v; (void)k; return 0; }\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)])


def test_ctypes_structs_match_the_header(tmp_path):
    """The ctypes mirrors in log_amd/_lib.py have the size and field offsets the C compiler gives the header's structs."""
    import shutil
    import subprocess
    from log_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = {"lograst_view": [f[0] for f in _lib.LograstView._fields_],
              "lograst_adam_key": [f[0] for f in _lib.LograstAdamKey._fields_]}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "lograst.h"', 'int main(void) {']
    for st, names in fields.items():
        prog.append(f'  printf("{st} %zu", sizeof({st}));')
        for n in names:
            prog.append(f'  printf(" %zu", offsetof({st}, {n}));')
        prog.append('  printf("\\n");')
    prog += ['  return 0;', '}']
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text("\n".join(prog))
    inc = os.path.join(ROOT, "include")
    subprocess.check_call([gcc, "-std=c99", "-I", inc, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).strip().splitlines()
    for line, (st, cls) in zip(out, (("lograst_view", _lib.LograstView), ("lograst_adam_key", _lib.LograstAdamKey))):
        parts = line.split()
        assert parts[0] == st and int(parts[1]) == ctypes.sizeof(cls), line
        assert [int(x) for x in parts[2:]] == [getattr(cls, f[0]).offset for f in cls._fields_], line


def test_ctypes_signatures_match_the_header_prototypes():
    """Every prototype in include/lograst.h against log_amd/_lib.py: same number of parameters and the same C class
    (pointer / 32-bit int / 64-bit int / float / double / size_t) in every position."""
    from log_amd import _lib
    src = open(os.path.join(ROOT, "include", "lograst.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\b(lograst_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src))
    assert set(protos) == set(_lib.EXPORTS)

    def c_class(param):
        p = param.strip()
        if "*" in p:
            return "ptr"
        base = p.rsplit(" ", 1)[0] if " " in p else p
        return {"int32_t": "i32", "uint32_t": "i32", "int": "i32", "float": "f32", "double": "f64", "size_t": "size",
                "int64_t": "i64"}[base.replace("const ", "").strip()]

    def py_class(t):
        if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
            return "ptr"
        return {ctypes.c_int32: "i32", ctypes.c_uint32: "i32", ctypes.c_int: "i32", ctypes.c_float: "f32",
                ctypes.c_double: "f64", ctypes.c_size_t: "size", ctypes.c_int64: "i64"}[t]

    for name, params in protos.items():
        want = [] if params.strip() in ("", "void") else [c_class(p) for p in params.split(",")]
        got = [py_class(t) for t in _lib._SIGNATURES[name][1]]
        assert got == want, (name, got, want)


def _knob_table(L):
    """[(name, default, lo, hi)] as lograst_knob_info enumerates it."""
    rows = []
    for i in range(L.lograst_knob_count()):
        name, what = ctypes.c_char_p(), ctypes.c_char_p()
        d, lo, hi = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert L.lograst_knob_info(i, ctypes.byref(name), ctypes.byref(d), ctypes.byref(lo), ctypes.byref(hi),
                                   ctypes.byref(what)) == 0
        rows.append((name.value.decode(), d.value, lo.value, hi.value))
    return rows


def test_every_tunable_knob_is_documented():
    """The knob table of the library (api.hip: kKnobs -- what lograst_knob_info enumerates) against INTEGRATION.md: a knob
    a host can move must be described where a host looks."""
    from log_amd import _lib
    names = [row[0] for row in _knob_table(_lib.lib())]
    assert len(names) >= 20 and all(re.fullmatch(r"LOGRAST_[A-Z_]+", n) for n in names)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert [n for n in names if n not in doc] == []


_KNOB_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from log_amd import _lib
L = _lib.lib()
def get(name):
    v = ctypes.c_int32(-12345)
    rc = L.lograst_get_knob(name, ctypes.byref(v))
    return [rc, v.value]
out = {"env": get(b"LOGRAST_MID_COOP")}
out["set_rc"] = L.lograst_set_knob(b"LOGRAST_MID_COOP", 32)
out["set"] = get(b"LOGRAST_MID_COOP")
out["range_rc"] = L.lograst_set_knob(b"LOGRAST_MID_COOP", 65)
out["range_err"] = L.lograst_last_error().decode()
out["after_range"] = get(b"LOGRAST_MID_COOP")
out["unknown_rc"] = L.lograst_set_knob(b"LOGRAST_NOPE", 1)
out["unknown_err"] = L.lograst_last_error().decode()
out["reset_rc"] = L.lograst_reset_knobs()
out["reset"] = get(b"LOGRAST_MID_COOP")
out["all"] = []
for i in range(L.lograst_knob_count()):
    name, d = ctypes.c_char_p(), ctypes.c_int32()
    assert L.lograst_knob_info(i, ctypes.byref(name), ctypes.byref(d), None, None, None) == 0
    out["all"].append([name.value.decode(), d.value] + get(name.value))
print(json.dumps(out))
"""


def test_knob_precedence_override_environment_default():
    """lograst_get_knob answers what the next launch reads: a lograst_set_knob override, else the environment variable of
    the knob's name (read in a child process that starts with it), else the default that lograst_knob_info reports."""
    import json
    import subprocess
    import sys
    from log_amd import _lib
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LOGRAST_") or k == "LOGRAST_LIB"}

    def child(**env):
        text = subprocess.check_output([sys.executable, "-c", _KNOB_CHILD, ROOT], env=dict(clean, **env), text=True)
        return json.loads(text.strip().splitlines()[-1])
    out = child(LOGRAST_MID_COOP="8")
    assert out["env"] == [0, 8]
    assert out["set_rc"] == 0 and out["set"] == [0, 32]
    assert out["range_rc"] == -1 and out["range_err"] == "LOGRAST_MID_COOP: value out of range"
    assert out["after_range"] == [0, 32]          # a refused value changes nothing
    assert out["unknown_rc"] == -1 and out["unknown_err"] == "unknown knob: LOGRAST_NOPE"
    assert out["reset_rc"] == 0 and out["reset"] == [0, 8]
    # a clean environment: every knob at the default that lograst_knob_info reports
    out = child()
    assert len(out["all"]) == 22 and out["env"] == [0, 16] and out["reset"] == [0, 16]
    for name, dflt, rc, value in out["all"]:
        assert rc == 0 and value == dflt, (name, value, dflt)


def test_backward_form_is_the_written_out_table():
    """lograst_backward_form (the reverse walk's form, as lr_launch_blend_bwd decides it) over knob LOGRAST_BWD_ROWS x the
    view's walk_form x n on either side of LOGRAST_HELPER_MIN_N: 1 = row-split, 2 = quadrant.  The view's pointers are fake
    (never dereferenced, as with lograst_forward_form); a NULL view or a walk_form outside the enumeration is an error code,
    not a form."""
    from log_amd import _lib
    L = _lib.lib()
    v = _lib.LograstView()
    v.width, v.height, v.tanfovx, v.tanfovy, v.scale_modifier = 64, 48, 0.5, 0.5, 1.0
    v.filter_mode, v.ndc_cull, v.extras = _lib.FILTER_CLAMP, 1, 1
    v.viewmatrix, v.projmatrix, v.bg = 0x1000, 0x2000, 0x3000
    min_n = ctypes.c_int32(-1)
    assert L.lograst_get_knob(b"LOGRAST_HELPER_MIN_N", ctypes.byref(min_n)) == 0 and min_n.value >= 1
    small, big = min_n.value - 1, min_n.value
    AUTO, ROWS, QUAD = _lib.FORM_AUTO, _lib.FORM_ROWS, 2
    expected = {  # (knob, walk_form, n) -> form
        (0, AUTO, small): 2, (0, AUTO, big): 2, (0, ROWS, small): 2, (0, ROWS, big): 2, (0, QUAD, small): 2, (0, QUAD, big): 2,
        (1, AUTO, small): 1, (1, AUTO, big): 1, (1, ROWS, small): 1, (1, ROWS, big): 1, (1, QUAD, small): 1, (1, QUAD, big): 1,
        (2, AUTO, small): 2, (2, AUTO, big): 1, (2, ROWS, small): 1, (2, ROWS, big): 1, (2, QUAD, small): 2, (2, QUAD, big): 2,
    }
    assert len(expected) == 18
    try:
        for (knob, form, n), want in expected.items():
            assert L.lograst_set_knob(b"LOGRAST_BWD_ROWS", knob) == 0
            v.walk_form = form
            assert L.lograst_backward_form(ctypes.byref(v), n) == want, (knob, form, n)
        v.walk_form = 3
        assert L.lograst_backward_form(ctypes.byref(v), big) == -1 and b"walk_form" in L.lograst_last_error()
        assert L.lograst_backward_form(None, big) == -1 and b"view" in L.lograst_last_error()
    finally:
        assert L.lograst_reset_knobs() == 0


def test_gather_and_activate_family_refuses_misaligned_quaternion_blocks():
    """include/lograst.h: the rotation blocks of lograst_gather_activate, lograst_activate_backward and
    lograst_activate_backward_adam move one quaternion (16 bytes) at a time and must be 16-byte aligned.  A pointer 4, 8 or
    12 bytes past a boundary is refused with LOGRAST_ERR_ARG before any device work -- on a machine without a GPU, with
    made-up addresses nobody dereferences.  Every other pointer of the calls below sits 4 bytes past a boundary and is not
    what the refusal names."""
    import torch  # noqa: F401
    from log_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p
    A = 0x10000                                     # addresses are A * slot (+ offset): aligned unless made otherwise
    keys = (_lib.LograstAdamKey * 6)()

    def gather(rotation=3 * A, raw_rotation=13 * A, act_rotation=18 * A):
        return L.lograst_gather_activate(8, 100, P(1 * A), P(2 * A + 4), P(4 * A + 4), P(5 * A + 4), P(rotation), P(6 * A + 4),
                                         P(7 * A + 4), 15, 3, P(8 * A + 4), P(9 * A + 4), P(10 * A + 4), P(11 * A + 4),
                                         P(raw_rotation), P(14 * A + 4), P(15 * A + 4), P(16 * A + 4), P(17 * A + 4),
                                         P(act_rotation), P(19 * A + 4), None)

    def backward(raw_rotation=4 * A, dl_dact_rotation=8 * A, dl_drotation=12 * A):
        return L.lograst_activate_backward(8, P(1 * A + 4), P(2 * A + 4), P(3 * A + 4), P(raw_rotation), 15, 3, P(5 * A + 4),
                                           P(6 * A + 4), P(7 * A + 4), P(dl_dact_rotation), P(9 * A + 4), P(10 * A + 4),
                                           P(11 * A + 4), P(dl_drotation), P(13 * A + 4), P(14 * A + 4), None)

    def fused(raw_rotation=4 * A, dl_dact_rotation=9 * A):
        return L.lograst_activate_backward_adam(8, P(1 * A + 4), P(2 * A + 4), P(3 * A + 4), P(raw_rotation), 15, 3, P(5 * A + 4),
                                                P(6 * A + 4), P(7 * A + 4), P(8 * A + 4), P(dl_dact_rotation), P(10 * A + 4),
                                                100, P(11 * A), P(12 * A + 4), keys, 0.9, 0.999, 1.0, 1e-15, None)

    for call, names in ((gather, ("rotation", "raw_rotation", "act_rotation")),
                        (backward, ("raw_rotation", "dl_dact_rotation", "dl_drotation")),
                        (fused, ("raw_rotation", "dl_dact_rotation"))):
        for name in names:
            for off in (4, 8, 12):
                default = call.__defaults__[call.__code__.co_varnames.index(name)]
                assert call(**{name: default + off}) == -1, (call.__name__, name, off)
                msg = L.lograst_last_error()
                assert b"16-byte aligned" in msg and name.encode() in msg, (call.__name__, name, off, msg)

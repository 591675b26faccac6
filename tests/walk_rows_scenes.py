"""The scenes on which the row-by-row rule of the reverse walk (tests/gpu_util.py: walk_row_stats) is calibrated and shown to
have teeth, with their CPU references computed once: the fp32 oracle, the fp32 walk restated with the kernels' freedoms
(oracle.backward_alt) and the float64 twin.  Nothing here needs a device.  tests/test_walk_rows_cpu.py asserts on them,
tools/walk_rows_md.py writes profiles/walk_rows_tests.md from them."""
import numpy as np

import list_cases as LC
from log_amd import scenes
from util import oracle_view, small_case

BG = (0.3, 0.6, 0.9)
LIST_MAX = 8193                                # every list case up to this many entries
THREADS = (1, 16)                              # two orders of the oracles' commits


def _small():
    return small_case(n=2000, W=96, H=80, focal=110.0, seed=3)


def _trained():
    return scenes.orbit_cameras(3, W=256, H=192, focal=280.0, radius=2.5)[1], scenes.trained_like_scene(20000, seed=1)


def _stacks():                                 # dense near-opaque stacks: 1 / (1 - alpha) up to 1000 on long runs
    return scenes.orbit_cameras(3, W=256, H=192, focal=280.0, radius=2.5)[1], scenes.random_scene(20000, seed=2, opacity=0.999, smax=0.05)


SCENES = {"small_case": _small, "trained_like_scene": _trained, "random_scene": _stacks}
for _c in LC.CASES:
    if _c.L <= LIST_MAX:
        SCENES[_c.id] = (lambda c: lambda: c.scene()[:2])(_c)
NAMES = list(SCENES)

_CACHE = {}


def reference(oracle, name):
    """-> dict(view, fwd, dL, og, alt, g64; og16, alt16: the same two with the other thread count).  Computed once per
    process; callers must not write into it."""
    if name not in _CACHE:
        cam, sc = SCENES[name]()
        v = oracle_view(oracle, cam, BG)
        of = oracle.forward(v, sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["colors"])
        dL = np.random.default_rng(4).standard_normal(of["image"].shape).astype(np.float32)
        ref = dict(view=v, fwd=of, dL=dL, g64=oracle.backward_f64(v, of, dL, cond=False, abs_sums=True))
        before = oracle.set_threads(THREADS[0])
        try:
            ref["og"], ref["alt"] = oracle.backward(v, of, dL, abs_sums=True), oracle.backward_alt(v, of, dL, abs_sums=True)
            oracle.set_threads(THREADS[1])
            ref["og16"], ref["alt16"] = oracle.backward(v, of, dL, abs_sums=True), oracle.backward_alt(v, of, dL, abs_sums=True)
        finally:
            oracle.set_threads(before)
        _CACHE[name] = ref
    return _CACHE[name]


def floor_asked(G, ref):
    """The largest (|alt - f64| - 2 |oracle - f64|) / (6e-8 unit) of this scene over both thread counts, either way round."""
    worst = 0.0
    for a in ("alt", "alt16"):
        for o in ("og", "og16"):
            worst = max(worst, G.walk_row_stats(ref[a], ref[o], ref["g64"])["worst_excess_units"])
    return worst

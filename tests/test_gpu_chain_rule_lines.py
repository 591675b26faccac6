"""GPU tests of the chain rule's large-input running-sum route (log_amd/csrc/project_bwd.hip: STAGE): every workgroup
builds its 1024-row slice of dL/dmeans2D in LDS -- zeros, then the live rows' values -- and writes it out as whole lines;
no zero pass runs in front of the kernel.  The reference is the same backward through the small-input route
(LOGRAST_HELPER_MIN_N at its default: the slice is cleared in memory, live rows overwrite theirs with 12-byte stores), handed
the SAME accumulator rows: the rows of one reverse walk are copied, and every compared backward runs on a copy of them with
dL/dimage = 0 (its own reverse walk then adds nothing), so the order of the reverse walk's float atomics does not enter and
the comparison is bit for bit.

Rows per block of 1024, by N: 5 / 1023: one partial block, sparse; 1024: one block, entirely live; 1025: an entirely live
block + a last block of one dead row; 3000: sparse, entirely live, entirely dead (952 rows); 4097: sparse, entirely live,
entirely dead, sparse, a last block of one live row."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W = H = 64
SIZES = [5, 1023, 1024, 1025, 3000, 4097]
SCRATCH_ZEROED, ACCUMULATE_ROWS = 1, 8      # include/lograst.h: LOGRAST_BWD_*


def block_kinds(n):
    nb = (n + 1023) // 1024
    return {1: ["live" if n == 1024 else "sparse"], 2: ["live", "dead"], 3: ["sparse", "live", "dead"],
            5: ["sparse", "live", "dead", "sparse", "live"]}[nb]


def scene(n, cam, seed=21):
    """A seeded random scene whose opacities make the blocks of 1024 rows sparse (a third of the rows can contribute),
    entirely dead (opacity 0) or entirely live (two-pixel Gaussians in front of everything else, translucent enough that none
    of the 1024 hides another)."""
    from log_amd import scenes
    sc = scenes.random_scene(n, seed=seed, opacity=None, smax=0.05)
    rng = np.random.default_rng(seed + 1)
    to_cam = np.asarray(cam["camera_center"], np.float32).reshape(3)
    to_cam = to_cam / np.linalg.norm(to_cam)
    for b, kind in enumerate(block_kinds(n)):
        r = slice(1024 * b, min(1024 * b + 1024, n))
        k = r.stop - r.start
        if kind == "dead":
            sc["opacity"][r] = 0.0
        elif kind == "sparse":
            sc["opacity"][r] = np.where(rng.random((k, 1)) < 0.33, sc["opacity"][r], 0.0).astype(np.float32)
        else:
            sc["opacity"][r] = 0.15
            sc["scaling"][r] = 0.05 + 0.01 * rng.random((k, 3), dtype=np.float32)
            sc["xyz"][r] = sc["xyz"][r] * np.float32(0.9) + to_cam * np.float32(1.2)
    return sc


class Case:
    """One forward and one reverse walk of a view (small-input route); the chain rule then runs on copies of its rows."""

    def __init__(self, n, cam, sc, flavour, dl_seed=5):
        import gpu_util as G
        from log_amd import rasterizer as R
        self.n, self.dev = n, torch.device(DEV)
        self.hf = G.hip_forward(cam, sc, (0.1, 0.2, 0.3), flavour=flavour, scratch_floats=0)
        self.rs, self.flavour, self.use_filter, self.m, self.s, self.r, self.saved = self.hf["_torch"]
        self.pw = self.saved.get("point_weight")
        dl = torch.tensor(np.random.default_rng(dl_seed).random((3, H, W), dtype=np.float32), device=self.dev)
        self.zero_image = torch.zeros_like(dl)
        rows = torch.zeros(n, 16, device=self.dev)
        sink = torch.zeros(n, 16, device=self.dev)
        self.call(dl, rows, sink, torch.empty(n, 3, device=self.dev))
        self.rows = rows.clone()                      # what the reverse walk summed (slots 0-8)
        assert float(self.rows[:, :9].abs().sum()) > 0
        self.R = R

    def call(self, dl_dimage, rows, sink, m2d):
        from log_amd import _lib, rasterizer as R
        L = R._backend.require(self.dev)
        view, keep = R._backend.make_view(self.rs, self.flavour, self.use_filter, self.dev)
        view.tile_row_begin, view.tile_row_end = self.saved["tile_rows"]
        view.walk_form = _lib.FORM_QUADRANT           # one reverse-walk kernel on both sides of the threshold
        assert rows.data_ptr() % 64 == 0 and sink.data_ptr() % 64 == 0
        sv, P = self.saved, R._ptr
        with torch.cuda.device(self.dev):
            _lib.check(L.lograst_backward(ctypes.byref(view), self.n, P(self.m), P(self.s), P(self.r), P(sv["radii"]),
                                          P(sv["geom"]), P(sv["state"]), P(sv["plist"]), P(sv["final_T"]), P(sv["n_contrib"]),
                                          P(dl_dimage), ctypes.c_void_p(m2d.data_ptr()), P(rows), P(None), P(None), P(sink),
                                          P(None), P(None), P(self.pw), SCRATCH_ZEROED | ACCUMULATE_ROWS,
                                          R._stream_ptr(self.dev)))
        torch.cuda.synchronize()
        del keep

    def chain_rule(self, big, sink0, m2d=None):
        """The chain rule on a copy of the reverse walk's rows -> (dL/dmeans2D, sink rows).  big: through the large-input
        route (LOGRAST_HELPER_MIN_N = 0 for the call, restored afterwards); else the knob's default."""
        from log_amd import tune
        rows, sink = self.rows.clone(), sink0.clone()
        if m2d is None:
            m2d = torch.full((self.n, 3), float("nan"), device=self.dev)
        prev = tune.get_knob("LOGRAST_HELPER_MIN_N")
        assert self.n < prev
        if big:
            tune.set_knob("LOGRAST_HELPER_MIN_N", 0)
        try:
            self.call(self.zero_image, rows, sink, m2d)
        finally:
            tune.set_knob("LOGRAST_HELPER_MIN_N", prev)
        assert torch.equal(rows[:, :12].view(torch.int32), self.rows[:, :12].view(torch.int32))   # the walk added nothing
        return m2d, sink


def bits(t):
    return t.contiguous().view(torch.int32)


def sink_start(n, dev, seed=9):
    """Running sums that are already under way (random), slots 14-15 a guard value."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    s = torch.randn(n, 16, generator=g).to(dev)
    s[:, 14:] = 7.0
    return s


def cameras():
    from log_amd import scenes
    return scenes.orbit_cameras(3, W=W, H=H, focal=70.0)


_cases = {}


def case(n, flavour_name="wodilate", view=0):
    """One forward + reverse walk per (n, flavour, view), shared by the tests and left unchanged."""
    from log_amd import rasterizer as R
    key = (n, flavour_name, view)
    if key not in _cases:
        cams = cameras()
        sc = scene(n, cams[0])
        _cases[key] = (Case(n, cams[view], sc, R.WODILATE if flavour_name == "wodilate" else R.UPSTREAM), sc)
    return _cases[key]


def check_live_pattern(n, c):
    pw = c.pw.cpu().numpy()
    for b, kind in enumerate(block_kinds(n)):
        live = pw[1024 * b: min(1024 * b + 1024, n)] > 0
        print("N=%d block %d (%s): %d of %d rows live" % (n, b, kind, int(live.sum()), len(live)))
        if kind == "dead":
            assert not live.any()
        elif kind == "live":
            assert live.all()
        elif len(live) > 16:
            assert 0 < live.sum() < len(live)


@pytest.mark.parametrize("n", SIZES)
def test_staged_slice_equals_the_small_input_route(n):
    """dL/dmeans2D (dead rows and the array's tail included: the output starts as NaN) and the sink rows, bit for bit."""
    c, _ = case(n)
    check_live_pattern(n, c)
    s0 = sink_start(n, c.dev)
    m_ref, s_ref = c.chain_rule(False, s0)
    m_big, s_big = c.chain_rule(True, s0)
    assert not torch.isnan(m_ref).any()
    dead = (c.pw == 0)
    assert bool((bits(m_big)[dead] == 0).all())                     # exactly +0.0f in every dead row
    assert bool((m_big[:, 2] == 0).all())
    assert torch.equal(bits(m_big), bits(m_ref))
    assert float(m_big.abs().sum()) > 0
    assert torch.equal(bits(s_big[:, :10]), bits(s_ref[:, :10]))    # dL/dmeans3D, dL/dscales, dL/drotations
    assert torch.equal(bits(s_big), bits(s_ref))                    # ... and opacity, colour, the two guard slots
    assert bool((s_big[:, 14:] == 7.0).all())
    assert not torch.equal(bits(s_big[~dead][:, :10]), bits(s0[~dead][:, :10]))
    assert torch.equal(bits(s_big[dead]), bits(s0[dead]))           # nothing is added to a dead row


@pytest.mark.parametrize("n", [1025, 3000])
def test_radii_as_the_live_flag(n):
    """The flavour without point_weight: radii > 0 is the live flag (the kernel's other instantiation)."""
    c, _ = case(n, "upstream")
    assert c.pw is None
    s0 = sink_start(n, c.dev)
    m_ref, s_ref = c.chain_rule(False, s0)
    m_big, s_big = c.chain_rule(True, s0)
    assert float(m_big.abs().sum()) > 0 and not torch.isnan(m_big).any()
    assert torch.equal(bits(m_big), bits(m_ref)) and torch.equal(bits(s_big), bits(s_ref))


@pytest.mark.parametrize("n", [5, 1025, 3000, 4097])
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_output_at_a_four_byte_offset(n, offset):
    """dl_dmeans2d handed at 4, 8 or 12 bytes past a 16-byte boundary (the C ABI asks for 4-byte alignment only): the
    scalar head and tail of every block's slice.  The floats in front of and behind the array keep their guard value."""
    c, _ = case(n)
    s0 = sink_start(n, c.dev)
    m_ref, s_ref = c.chain_rule(False, s0)
    buf = torch.full((offset + 3 * n + 37,), 7.0, device=c.dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset: offset + 3 * n]
    assert out.data_ptr() % 16 == 4 * offset
    _, s_big = c.chain_rule(True, s0, m2d=out)
    assert bool((buf[:offset] == 7.0).all()) and bool((buf[offset + 3 * n:] == 7.0).all())
    assert torch.equal(bits(out.reshape(n, 3)), bits(m_ref))
    assert torch.equal(bits(s_big), bits(s_ref))


@pytest.mark.parametrize("n", [3000, 4097])
def test_two_views_into_one_sink(n):
    """Two different views added into one sink bucket: the sums equal the small-input route's bit for bit."""
    a, _ = case(n, view=0)
    b, _ = case(n, view=1)
    assert not torch.equal(a.rows, b.rows)
    s0 = torch.zeros(n, 16, device=a.dev)
    res = {}
    for big in (False, True):
        m_a, s = a.chain_rule(big, s0)
        m_b, s = b.chain_rule(big, s)
        res[big] = (m_a, m_b, s)
    for x, y in zip(res[False], res[True]):
        assert torch.equal(bits(x), bits(y))
    both = (a.pw > 0) & (b.pw > 0)
    assert int(both.sum()) > 0 and float(res[True][2][both][:, :10].abs().sum()) > 0

"""The native `shs=` kernels (log_amd/csrc/sh.hip: lr_sh_fwd_kernel, lr_sh_bwd_kernel) through the C entry points
lograst_sh_forward / lograst_sh_backward, with buffers this file owns, at the edges of the wave-staged layout
(tests/sh_edge_cases.py: N around a wave and a workgroup, both copy paths, M above the active degree, M no perfect square),
against the C oracle, which tests/test_sh_edges_cpu.py holds to the float64 twin at the same shapes.  Every output lies
between guard values that must survive the call."""
import ctypes

import numpy as np
import pytest
import torch

import sh_edge_cases as E
from util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 61            # guard elements on either side of every output (odd: the tail is no multiple of a float4)
GUARD_F, GUARD_B = -7.25, 0xA5
WORST = {}            # criterion -> largest figure seen (printed by the tests, for the note in profiles/)


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


class Guarded:
    """`count` elements at `offset` elements past a 16-byte boundary, GUARD elements of guard value in front and behind."""

    def __init__(self, count, dtype=torch.float32, offset=0, fill=None):
        self.value = GUARD_F if dtype == torch.float32 else GUARD_B
        head = 64 + offset                                    # 64 elements: a multiple of 16 bytes for either type
        self.buf = torch.full((head + count + GUARD,), self.value, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[head: head + count]
        self.head, self.count = head, count
        if dtype == torch.float32:
            assert self.t.data_ptr() % 16 == (4 * offset) % 16
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill, dtype=dtype).reshape(-1).to(DEV))

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def read(self, shape):
        """The payload on the host, after checking every guard element."""
        host = self.buf.cpu()
        assert bool((host[:self.head] == self.value).all()), "guard in front of the output was written"
        assert bool((host[self.head + self.count:] == self.value).all()), "guard behind the output was written"
        return host[self.head: self.head + self.count].numpy().reshape(shape).copy()


def _dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return t, ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _forward(L, n, M, degree, means, campos, shs_ptr):
    from log_amd import _lib
    colors, clamped = Guarded(3 * n), Guarded(3 * n, torch.uint8)
    _lib.check(L.lograst_sh_forward(n, degree, M, means, campos, shs_ptr, colors.ptr(), clamped.ptr(), _stream()))
    torch.cuda.synchronize()
    return colors.read((n, 3)), clamped.read((n, 3))


def _backward(L, n, M, degree, means, campos, shs_ptr, clamped, g, g_shs, g_means, accumulate):
    from log_amd import _lib
    _lib.check(L.lograst_sh_backward(n, degree, M, means, campos, shs_ptr, clamped, g, g_shs.ptr(), g_means.ptr(),
                                     accumulate, _stream()))
    torch.cuda.synchronize()
    return g_shs.read((n, M, 3)), g_means.read((n, 3))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _within_ulps(got, want64, ulps):
    """|got - want64| <= ulps * ulp(fp32(want64)), element by element."""
    ulp = np.spacing(np.abs(want64.astype(np.float32))).astype(np.float64)
    return bool((np.abs(got.astype(np.float64) - want64) <= ulps * ulp).all())


@pytest.mark.parametrize("M", E.MS)
def test_sh_kernels_at_wave_and_workgroup_edges(oracle_mod, M):
    from log_amd import _lib
    L = _lib.lib()
    for n, _, degree in E.cases(M):
        tag = (n, M, degree)
        means, campos, shs, g = E.inputs(n, M, degree)
        nk = (degree + 1) ** 2
        (_m, d_means), (_c, d_campos), (_s, d_shs), (_g, d_g) = _dev(means), _dev(campos), _dev(shs), _dev(g)

        # ---- forward: colours and clamp mask bit for bit the oracle's
        ocol, ocl = oracle_mod.sh_forward(means, campos, shs, degree)
        if degree > 0:
            assert ocl.any() and not ocl.all(), tag
        col, cl = _forward(L, n, M, degree, d_means, d_campos, d_shs)
        assert (cl == ocl).all(), tag
        assert (_bits(col) == _bits(ocol)).all(), tag
        _cl, d_cl = _dev(cl)

        # ---- backward, accumulate = 0: every element of dl_dshs overwritten, zeros above the active degree
        ogs, ogm = oracle_mod.sh_backward(means, campos, shs, degree, ocl, g)
        g_shs = Guarded(3 * M * n, fill=np.full(3 * M * n, np.nan, np.float32))
        g_means = Guarded(3 * n, fill=np.zeros(3 * n, np.float32))
        gs0, gm0 = _backward(L, n, M, degree, d_means, d_campos, d_shs, d_cl, d_g, g_shs, g_means, 0)
        assert not np.isnan(gs0).any(), tag
        assert (gs0[:, nk:] == 0.0).all(), tag
        e_s, e_m = rel_l2(gs0, ogs), rel_l2(gm0, ogm)
        _note("backward rel_l2 dl_dshs", e_s)
        _note("backward rel_l2 dl_dmeans3d", e_m)
        assert e_s < 1e-6 and e_m < 1e-5, (tag, e_s, e_m)
        assert np.abs(gs0[:, :nk]).sum() > 0

        # ---- backward, accumulate = 1: prefill + the result above, the rest of every row untouched
        rng = np.random.default_rng(1000 + n + M + degree)
        pre_s = (rng.random((n, M, 3), dtype=np.float32) + 0.5) * np.where(rng.random((n, M, 3)) < 0.5, -1, 1).astype(np.float32)
        pre_m = (rng.random((n, 3), dtype=np.float32) + 0.5) * np.where(rng.random((n, 3)) < 0.5, -1, 1).astype(np.float32)
        g_shs, g_means = Guarded(3 * M * n, fill=pre_s), Guarded(3 * n, fill=pre_m)
        gs1, gm1 = _backward(L, n, M, degree, d_means, d_campos, d_shs, d_cl, d_g, g_shs, g_means, 1)
        assert _within_ulps(gs1, pre_s.astype(np.float64) + gs0.astype(np.float64), 2), tag
        assert _within_ulps(gm1, pre_m.astype(np.float64) + gm0.astype(np.float64), 2), tag
        assert (_bits(gs1[:, nk:]) == _bits(pre_s[:, nk:])).all(), tag
        ulp = np.spacing(np.abs((pre_s.astype(np.float64) + gs0).astype(np.float32))).astype(np.float64)
        _note("accumulate: ulps from prefill + result", (np.abs(gs1 - (pre_s.astype(np.float64) + gs0)) / ulp).max())
    print("M = %d: %s" % (M, {k: "%.3g" % v for k, v in sorted(WORST.items())}))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_shs_and_dl_dshs_at_a_four_byte_offset(offset):
    """shs and dl_dshs handed at 4, 8 and 12 bytes past a 16-byte boundary (include/lograst.h asks for 4-byte alignment): the
    wave copy must leave its float4 path, and the results are bit for bit those of the aligned call; the floats in front of
    and behind dl_dshs keep their guard value."""
    from log_amd import _lib
    L = _lib.lib()
    for M in (4, 16):
        for n in (65, 257):
            degree = E.degrees(M)[-1]
            means, campos, shs, g = E.inputs(n, M, degree)
            (_m, d_means), (_c, d_campos), (_g, d_g) = _dev(means), _dev(campos), _dev(g)
            pre = np.random.default_rng(offset).random((n, M, 3), dtype=np.float32) + 0.5
            res = {}
            for off in (0, offset):
                d_shs = Guarded(3 * M * n, offset=off, fill=shs)
                col, cl = _forward(L, n, M, degree, d_means, d_campos, d_shs.ptr())
                assert (_bits(d_shs.read((n, M, 3))) == _bits(shs)).all()
                _cl, d_cl = _dev(cl)
                out = [col, cl]
                for accumulate in (0, 1):
                    g_shs = Guarded(3 * M * n, offset=off, fill=pre if accumulate else np.full(3 * M * n, np.nan, np.float32))
                    g_means = Guarded(3 * n, fill=np.zeros(3 * n, np.float32))
                    out += list(_backward(L, n, M, degree, d_means, d_campos, d_shs.ptr(), d_cl, d_g, g_shs, g_means, accumulate))
                res[off] = out
            names = ("colors", "clamped", "dl_dshs", "dl_dmeans3d", "dl_dshs accumulated", "dl_dmeans3d accumulated")
            for name, a, b in zip(names, res[0], res[offset]):
                assert not np.isnan(a.astype(np.float64)).any()
                differ = _bits(a.astype(np.float32)) != _bits(b.astype(np.float32))
                assert not differ.any(), (name, M, n, offset, int(differ.sum()), a[differ][:4], b[differ][:4])
            # the case has what tells the two paths apart: gradients that are a negative basis value times a cut channel
            assert (res[0][1] != 0).any() and (res[0][2] == 0).any()
            assert np.abs(res[0][2]).sum() > 0 and not (_bits(res[0][4]) == _bits(pre)).all()

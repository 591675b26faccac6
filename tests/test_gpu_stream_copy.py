"""lograst_stream_copy (log_amd/csrc/project.hip) is bench.py's measured roof: every *_frac_of_measured_stream_copy divides
by 2 * nbytes / time.  Here every one of its five forms has to COPY nbytes: random bits into a 16-byte-aligned slice inside
a sentinel buffer, the slice bit for bit the source afterwards, every byte around it and the source itself unchanged --
at sizes around a workgroup, around one unrolled pass of the whole grid (U x stride) and with a tail behind two passes,
and with the very argument list the benchmark issues."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A
PAD = 4 * 37                                                # int32 words around the destination slice (a multiple of 16 bytes)
UNROLL = {0: 4, 2: 8, 3: 4}                                 # the grid-stride forms and their loads in flight per lane
FLAT = (1, 4)                                               # one access per lane, grid = n16 / 256
DEFAULT_BLOCKS = 4096
ERR_ARG = -1                                                # LOGRAST_ERR_ARG


def _native():
    from log_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


_SOURCE = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_sources():
    """The sources live for this file only: nothing stays on the device for the tests that run after it."""
    yield
    _SOURCE.clear()
    torch.cuda.empty_cache()


def _source(n16):
    """n16 x 16 bytes of random bits (NaN patterns and all), drawn once per size class and cut to length, with a copy to
    hold the source against afterwards."""
    cap = 1 << max(n16 - 1, 1).bit_length()
    if cap not in _SOURCE:
        for big in [c for c in _SOURCE if c > (1 << 20) and cap > (1 << 20)]:   # one large source at a time
            del _SOURCE[big]
        gen = torch.Generator(device=DEV).manual_seed(cap)
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (4 * cap,), dtype=torch.int32, device=DEV, generator=gen)
        src[:8] = torch.tensor([0x7FC00000, -1, 0x7F800001, -0x80000000, 0, 1, 0x7F800000, SENTINEL], dtype=torch.int32)
        _SOURCE[cap] = (src, src.clone())
    src, keep = _SOURCE[cap]
    return src[:4 * n16], keep[:4 * n16]


def _copy_and_check(n16, arg):
    _lib, L = _native()
    src, keep = _source(n16)
    buf = torch.full((4 * n16 + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    dst = buf[PAD:PAD + 4 * n16]
    assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    _lib.check(L.lograst_stream_copy(dst.data_ptr(), src.data_ptr(), 16 * n16, arg, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(dst, src), (n16, hex(arg))
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + 4 * n16:] == SENTINEL).all()), (n16, hex(arg))
    assert torch.equal(src, keep), (n16, hex(arg))


def _cases():
    out = []
    for form, U in UNROLL.items():
        for blocks in (1, 2, 3):
            S = 256 * blocks
            for n16 in (1, 255, 256, 257, U * S - 1, U * S, U * S + 1, 2 * U * S + S + 5):
                out.append((form, blocks, n16))
        S = 256 * DEFAULT_BLOCKS                                        # blocks = 0: one size each side of U x 4096 x 256 x 16 bytes
        for n16 in (1, 255, 256, 257, U * S - 1, U * S + 1):
            out.append((form, 0, n16))
    for form in FLAT:
        for n16 in (1, 255, 256, 257, 65537):
            out.append((form, 0, n16))
    return out


def test_the_forms_under_test_are_the_benchmark_s():
    import bench
    assert tuple(sorted(bench.COPY_FORMS)) == tuple(sorted(list(UNROLL) + list(FLAT))) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("form,blocks,n16", _cases())
def test_every_form_copies_every_byte(form, blocks, n16):
    _copy_and_check(n16, (form << 20) | blocks)


def test_stream_copy_edges_of_the_argument():
    _lib, L = _native()
    src, keep = _source(1024)
    buf = torch.full((4 * 1024 + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    dst = buf[PAD:PAD + 4096]
    # nothing to copy: nothing happens
    _lib.check(L.lograst_stream_copy(dst.data_ptr(), src.data_ptr(), 0, 0, _stream()))
    # a size, a destination or a source off the 16-byte grid: the argument error, and no launch
    for d_off, s_off, nbytes in ((0, 0, 16 * 100 + 8), (1, 0, 1600), (0, 2, 1600), (0, 0, 4)):
        rc = L.lograst_stream_copy(dst[d_off:].data_ptr(), src[s_off:].data_ptr(), nbytes, 0, _stream())
        assert rc == ERR_ARG and b"16" in L.lograst_last_error(), (d_off, s_off, nbytes, rc)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and torch.equal(src, keep)
    # a form number nobody defined runs the default kernel; the packing (form << 20) | blocks takes all 20 bits of blocks
    for arg in ((5 << 20) | 2, (9 << 20), (0 << 20) | 0xFFFFF, (2 << 20) | 0xFFFFF, (3 << 20) | 0xFFFFF):
        for n16 in (257, 2 * 8 * 512 + 512 + 5):
            _copy_and_check(n16, arg)


def test_the_benchmark_s_calls_copy_everything():
    """The argument list of bench.py's measured_stream_copy_bandwidth (every form of bench.COPY_FORMS; the grid-stride ones
    with 1024 ... 16384 workgroups, the flat ones with 0), on 64 MB of random bits."""
    import bench
    n16 = (64 << 20) // 16
    calls = 0
    for form in bench.COPY_FORMS:
        for blocks in ((0,) if form in FLAT else (1024, 2048, 4096, 8192, 16384)):
            _copy_and_check(n16, (form << 20) | blocks)
            calls += 1
    assert calls == 17

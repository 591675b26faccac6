"""The exchange's device side (log_amd/csrc/exchange.hip) at its block, bound and form edges, against the restatement of
the segment format in tests/exchange_ref.py (proved against the torch formulation on the CPU: test_exchange_ref_cpu.py).
Every comparison is exact, on int32 views: pack and unpack move bits, and the summing unpack adds the segments in order,
((s0 + s1) + s2) + ... in fp32.  The C entry points are called directly, into buffers the test owns and has filled with a
sentinel, and through log_amd.dist._pack_segments / _unpack_segments."""
import pytest
import torch

import exchange_ref as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64                                                  # sentinel floats behind the last segment
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _native():
    from log_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _pack(bucket, kmax, clear=False, hint=None, hint_rows=None, flag=True):
    """One pack through the C ABI into a sentinel-filled buffer of the test's own -> (packed with GUARD floats behind the
    segments, overflow flag or None when `flag` is False: the NULL pointer the ABI allows)."""
    _lib, L = _native()
    G, R, _ = bucket.shape
    seg = X.segment_floats(kmax)
    assert seg == int(L.lograst_sparse_segment_floats(kmax)) and bucket.is_contiguous()
    packed = X.sentinel(G * seg + GUARD, DEV)
    over = torch.zeros(1, dtype=torch.int32, device=DEV) if flag else None
    op = over.data_ptr() if flag else None
    if hint is not None:
        assert hint.is_contiguous() and hint.element_size() == 4
        n = int(hint.numel()) if hint_rows is None else int(hint_rows)
        assert n <= hint.numel()
        _lib.check(L.lograst_pack_rows_hinted(bucket.data_ptr(), G, R, kmax, packed.data_ptr(), op, 1 if clear else 0,
                                              hint.data_ptr(), n, _stream()))
    else:
        fn = L.lograst_pack_rows_clear if clear else L.lograst_pack_rows
        _lib.check(fn(bucket.data_ptr(), G, R, kmax, packed.data_ptr(), op, _stream()))
    torch.cuda.synchronize()
    return packed, (bool(over.item()) if flag else None)


def _check_pack(rows, sel, kmax, packed, over, bucket, clear):
    """Everything a pack promises, on host copies.  rows: the input (CPU); sel: the rows it had to take; packed / over: what
    it gave; bucket: `rows` as the pack left it."""
    G, R, _ = rows.shape
    rb = X.bits(rows)
    counts = sel.sum(1).tolist()
    p = packed.cpu()
    got = X.decode(p, G, kmax)
    assert [h for h, _, _ in got] == counts                              # the header is the true count, kept or not
    if over is not None:
        assert over == any(c > kmax for c in counts)
    want, _ = X.expect(rows, sel, kmax)
    kept = torch.zeros(G, R, dtype=torch.bool)
    for g in range(G):
        h, idx, vals = got[g]
        if counts[g] <= kmax:
            assert torch.equal(idx, want[g][1]) and torch.equal(vals, want[g][2]), g
        else:                                                           # any kmax of the selected rows, distinct, each intact
            assert idx.numel() == kmax and idx.unique().numel() == kmax, g
            assert int(idx.min()) >= 0 and int(idx.max()) < R and bool(sel[g, idx.long()].all()), g
            assert torch.equal(vals, rb[g, idx.long()]), g
        kept[g, idx.long()] = True
    if p.numel() > G * X.segment_floats(kmax):                           # (a buffer of the test's own)
        assert X.untouched_outside(p, G, kmax, counts) == 0
    # the bucket: untouched without clear; with it exactly the kept rows are +0.0, every other row keeps its bits
    left = torch.where(kept[:, :, None], torch.zeros((), dtype=torch.int32), rb) if clear else rb
    assert torch.equal(X.bits(bucket.cpu()), left)


def _bounds(sel, R):
    longest = max(int(sel.sum(1).max()), 1)
    return longest, [longest] + ([longest - 1] if longest >= 2 else []) + ([17, 1] if R in (65, 1025) else [])


# ---- the scanning pack ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R", X.SCAN_SHAPES)
@pytest.mark.parametrize("density", X.DENSITIES)
def test_scanning_pack(G, R, density):
    """lograst_pack_rows / _clear with R at, below and above a wave (64), a round (256) and a workgroup (1024), planted rows
    on both sides of every such edge, special values (NaN, inf, denormal: non-zero; -0.0: zero), and kmax exactly full, one
    short, 17 and 1."""
    from log_amd import dist as D
    rows, special = X.planted(G, R, density)
    sel = X.select(rows)
    rows_d = rows.to(DEV)
    assert torch.equal(X.select(rows_d).cpu(), sel)
    longest, ks = _bounds(sel, R)
    for kmax in ks:
        for clear in (False, True):
            bucket = rows_d.clone()
            packed, over = _pack(bucket, kmax, clear=clear)
            assert over == (kmax < longest)
            _check_pack(rows, sel, kmax, packed, over, bucket, clear)
            bucket = rows_d.clone()
            flat, flag = D._pack_segments(bucket, kmax, clear=clear)
            assert flat.numel() == G * X.segment_floats(kmax)
            _check_pack(rows, sel, kmax, flat, bool(flag), bucket, clear)
    if longest >= 2:                                                    # overflow = NULL with a bound that is too small
        bucket = rows_d.clone()
        packed, _ = _pack(bucket, 1, flag=False)
        _check_pack(rows, sel, 1, packed, None, bucket, False)


# ---- the hinted pack at the small shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R", X.SCAN_SHAPES)
@pytest.mark.parametrize("density", X.DENSITIES)
def test_hinted_pack_with_a_truthful_hint(G, R, density):
    """A hint that names exactly the non-zero rows gives the scanning pack's segments (after the sort), clear on and off."""
    from log_amd import dist as D
    rows, _ = X.planted(G, R, density)
    sel = X.select(rows)
    hint = X.hint_for(sel).to(DEV)
    rows_d = rows.to(DEV)
    longest, ks = _bounds(sel, R)
    for kmax in ks:
        for clear in (False, True):
            bucket = rows_d.clone()
            packed, over = _pack(bucket, kmax, clear=clear, hint=hint)
            _check_pack(rows, sel, kmax, packed, over, bucket, clear)
            if kmax == longest:
                scan, _ = _pack(rows_d.clone(), kmax, clear=clear)
                assert X.same_groups(X.decode(packed.cpu(), G, kmax), X.decode(scan.cpu(), G, kmax)) == []
                bucket = rows_d.clone()
                flat, flag = D._pack_segments(bucket, kmax, clear=clear, hint=hint)
                _check_pack(rows, sel, kmax, flat, bool(flag), bucket, clear)


@pytest.mark.parametrize("G,R", [(G, R) for G, R in X.SCAN_SHAPES if R in (5, 65, 1025, 2049)])
def test_hinted_pack_follows_the_hint_alone(G, R):
    """The hint's rules: a word of -0.0 (and any other non-zero bits) selects; a hinted all-zero row is packed with its zeros
    and its index; a non-zero row without a hint is neither packed nor cleared; rows from hint_rows on have no hint, with
    hint_rows at the end, in the middle of a group and in the middle of a 1024-row block."""
    from log_amd import dist as D
    rows, _ = X.planted(G, R, "half")
    rows_d = rows.to(DEV)
    gen = torch.Generator().manual_seed(R)
    hint = X.hint_for(torch.rand(G, R, generator=gen) < 0.3, seed=1)
    assert X.NEG_ZERO in hint.tolist()
    nz = X.select(rows).view(-1)
    hinted = hint != 0
    assert bool((hinted & ~nz).any()) and bool((~hinted & nz).any())
    hint_d = hint.to(DEV)
    for n in (G * R, (G - 1) * R + R // 2, min(G * R, 1030)):
        sel = X.select(rows, hint, hint_rows=n)
        for kmax in _bounds(sel, R)[1]:
            for clear in (False, True):
                bucket = rows_d.clone()
                packed, over = _pack(bucket, kmax, clear=clear, hint=hint_d, hint_rows=n)   # (the words behind n are there, and set)
                _check_pack(rows, sel, kmax, packed, over, bucket, clear)
        bucket = rows_d.clone()
        kmax = _bounds(sel, R)[0]
        flat, flag = D._pack_segments(bucket, kmax, clear=True, hint=hint_d[:n])
        _check_pack(rows, sel, kmax, flat, bool(flag), bucket, True)


# ---- the hinted pack at the block sizes production runs -------------------------------------------------------------------
def _big_hinted(G, R, kmax, hinted, hint_rows, need_bytes):
    """Rows (every float non-zero: X.pattern_of), hints and checks all on the device, no host copy of the bucket.  hinted:
    bool [G * R], the words that are set; rows from hint_rows on have no hint all the same.  kmax None: the longest list."""
    _lib, L = _native()
    free, _ = torch.cuda.mem_get_info(0)
    print("hinted pack %d x %d: %.2f GB free, %.2f GB needed" % (G, R, free / 1e9, need_bytes / 1e9))
    if free < need_bytes:
        pytest.skip("less than %.1f GB of device memory free" % (need_bytes / 1e9))
    torch.cuda.reset_peak_memory_stats(0)
    N, CH = G * R, 1 << 20
    rows = torch.empty(G, R, 16, dtype=torch.int32, device=DEV)
    flat = rows.view(N, 16)
    for a in range(0, N, CH):
        flat[a:a + CH] = X.pattern_rows(a, min(CH, N - a), DEV)
    words = torch.tensor(X.HINT_WORDS, dtype=torch.int32, device=DEV)[torch.arange(N, device=DEV) % len(X.HINT_WORDS)]
    hint = torch.where(hinted, words, torch.zeros((), dtype=torch.int32, device=DEV))
    del words
    sel = (hinted & (torch.arange(N, device=DEV) < hint_rows)).view(G, R)
    counts = sel.sum(1)
    if kmax is None:
        kmax = int(counts.max())
    assert int(counts.max()) <= kmax
    seg = X.segment_floats(kmax)
    live = torch.nonzero(counts).reshape(-1).tolist()
    for clear in (False, True):
        packed = X.sentinel(G * seg + GUARD, DEV)
        over = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.check(L.lograst_pack_rows_hinted(rows.data_ptr(), G, R, kmax, packed.data_ptr(), over.data_ptr(), 1 if clear else 0,
                                              hint.data_ptr(), int(hint_rows), _stream()))
        torch.cuda.synchronize()
        pb = X.bits(packed)
        body = pb[:G * seg].view(G, seg)
        assert int(over.item()) == 0
        assert torch.equal(body[:, 0].to(torch.int64), counts)
        assert bool((pb[G * seg:] == X.SENTINEL).all())
        for g in live:                                                  # the groups that hold hints, one by one
            h, idx, vals = X.decode_group(packed, g, kmax)
            m = int(counts[g])
            want = torch.nonzero(sel[g]).reshape(-1)
            assert h == m and torch.equal(idx.to(torch.int64), want), g
            assert torch.equal(vals, X.pattern_of(want + g * R)), g
            assert bool((body[g, 16 + 16 * m:16 + 16 * kmax] == X.SENTINEL).all()), g
            assert bool((body[g, 16 + 16 * kmax + m:16 + 17 * kmax] == X.SENTINEL).all()), g
        empty = counts == 0                                             # every other segment: nothing but its header
        for a in range(0, G, 128):
            clean = (body[a:a + 128, 16:16 + 17 * kmax] == X.SENTINEL).all(1)
            assert bool(clean[empty[a:a + 128]].all()), a
        sf = sel.view(N)
        for a in range(0, N, CH):                                       # the bucket: hinted rows +0.0 after a clear, all else as it was
            want = X.pattern_rows(a, min(CH, N - a), DEV)
            if clear:
                want[sf[a:a + CH]] = 0
            assert torch.equal(flat[a:a + CH], want), (clear, a)
        if clear:
            flat[sf] = X.pattern_of(torch.nonzero(sf).reshape(-1))      # (the bucket as it was)
        del packed, pb, body
    print("hinted pack %d x %d: %d rows per block x %d, kmax %d, peak device memory %.2f GB"
          % ((G, R) + X.hinted_rows_per_block(G, R) + (kmax, torch.cuda.max_memory_allocated(0) / 1e9)))
    return counts


def test_hinted_pack_1280_rows_per_block_one_group():
    """G = 1, R = 4096 * 1024 + 1: 1280 rows per block (3277 blocks, the last of 1025 rows: a fifth trip of the listing loop
    with one live lane).  Block 0 hinted entirely (1280 list entries: beyond 1023), block 1 not at all, block 2 only its last
    row, the last block only row R - 1, 2 % at random elsewhere; kmax the exact count."""
    G, R = 1, 4096 * 1024 + 1
    rpb, blocks = X.hinted_rows_per_block(G, R)
    assert (rpb, blocks, R - (blocks - 1) * rpb) == (1280, 3277, 1025)
    gen = torch.Generator(device=DEV).manual_seed(41)
    hinted = torch.rand(R, device=DEV, generator=gen) < 0.02
    hinted[:rpb] = True
    hinted[rpb:3 * rpb] = False
    hinted[3 * rpb - 1] = True
    hinted[(blocks - 1) * rpb:] = False
    hinted[R - 1] = True
    counts = _big_hinted(G, R, None, hinted, R, 16 * 4 * R * 2 + (1 << 30))
    assert int(counts[0]) > 0.015 * R


def test_hinted_pack_1280_rows_per_block_64_groups():
    """G = 64, R = 65537: 1280 rows per block, 52 blocks per group, the last of 257 rows.  3 % at random plus both rows at
    every block edge of groups 0 and 63; the hint ends at 40 R + 100, so group 40 has 100 hinted rows at most and groups 41
    to 63 none, whatever their words say."""
    G, R = 64, 65537
    rpb, blocks = X.hinted_rows_per_block(G, R)
    assert (rpb, blocks, R - (blocks - 1) * rpb) == (1280, 52, 257)
    gen = torch.Generator(device=DEV).manual_seed(42)
    hinted = (torch.rand(G * R, device=DEV, generator=gen) < 0.03).view(G, R)
    edges = torch.tensor(sorted({0, R - 1} | {b * rpb - 1 for b in range(1, blocks)} | {b * rpb for b in range(1, blocks)}), device=DEV)
    hinted[0, edges] = True
    hinted[63, edges] = True
    counts = _big_hinted(G, R, None, hinted.view(-1), 40 * R + 100, 16 * 4 * G * R * 2 + (1 << 30))
    assert int(counts[0]) > 2 * blocks and int(counts[41:].sum()) == 0 and 0 < int(counts[40]) <= 100


def test_hinted_pack_16384_rows_per_block():
    """G = 2049, R = 16400: the cap of 16384 rows per block, two blocks per group, the second of 16 rows; kmax = 16384.  Group
    0: all of block 0, every slot of the 16-bit list up to 16383.  Group 1: rows 16383, 16384 and 16399.  Group 2048: the
    last row.  Twenty seeded groups: 1 % at random.  Every other group has no hint: header 0, segment and rows untouched."""
    G, R, kmax = 2049, 16400, 16384
    assert X.hinted_rows_per_block(G, R) == (16384, 2)
    gen = torch.Generator(device=DEV).manual_seed(43)
    hinted = torch.zeros(G, R, dtype=torch.bool, device=DEV)
    some = (torch.randperm(G - 3, generator=torch.Generator().manual_seed(43))[:20] + 2).tolist()
    for g in some:
        hinted[g] = torch.rand(R, device=DEV, generator=gen) < 0.01
    hinted[0, :16384] = True
    hinted[1, [16383, 16384, 16399]] = True
    hinted[2048, R - 1] = True
    need = 16 * 4 * G * R + 4 * G * X.segment_floats(kmax) + (1 << 30)
    counts = _big_hinted(G, R, kmax, hinted.view(-1), G * R, need)
    assert int(counts[0]) == 16384 and int(counts[1]) == 3 and int(counts[2048]) == 1 and int((counts > 0).sum()) == 23


# ---- the unpack, on hand-built segments ------------------------------------------------------------------------------------
def _unpack(dest, packed, segments, kmax, rows_per_group, dest_group_rows, mode):
    _lib, L = _native()
    _lib.check(L.lograst_unpack_rows(dest.data_ptr(), packed.data_ptr(), segments, kmax, rows_per_group, dest_group_rows, mode,
                                     _stream()))
    torch.cuda.synchronize()


def _guarded(rows, fill=None, guard=3):
    """-> (buffer [guard + rows + guard, 16] of sentinel floats on the host, the slice of the middle rows)."""
    buf = X.sentinel((rows + 2 * guard) * 16).view(-1, 16).clone()
    if fill is not None:
        buf[guard:guard + rows] = fill
    return buf, slice(guard, guard + rows)


def _hand_segments(kmax, R, gen):
    """Six segments: empty; full; three with the indices -1, R and INT32_MAX among good ones (at entry 0 in turn, so that
    kmax = 1 has each of them); and, last in its allocation, one whose header says kmax + 5.  No entry names row R // 2:
    that is the index planted in everything the format leaves unspecified -- the entries behind the empty segment's count
    and every segment's index padding kmax .. roundup(kmax, 16), the only entries a launch of roundup(kmax, 16) lanes
    could reach behind kmax (none at kmax = 16) -- so that a reader that passes the count, or the clamp of the header to
    kmax, WRITES into a row that must keep the sentinel."""
    bad = (-1, R, INT32_MAX)
    spare = R // 2
    groups = [(0, [], torch.zeros(0, 16))]
    for s in range(5):
        idx = [r + (r >= spare) for r in torch.randperm(R - 1, generator=gen)[:kmax].tolist()]
        if 1 <= s <= 3:
            for j in range(0, kmax, 4):
                idx[j] = bad[(s - 1 + j // 4) % 3]
        vals = torch.randn(kmax, 16, generator=gen) * (10.0 ** torch.randint(-3, 4, (kmax, 1), generator=gen).float())
        groups.append((kmax + 5 if s == 4 else kmax, idx, vals))
    return X.build_segments(groups, kmax, beyond=(R // 2, 123.0)), len(groups)


@pytest.mark.parametrize("kmax", [1, 15, 16, 17, 33])
def test_unpack_guards_and_modes(kmax):
    """lograst_unpack_rows on hand-built segments: header 0, = kmax and kmax + 5 (the segment ends its allocation; without
    the clamp to kmax the lanes kmax .. roundup(kmax, 16) would take the index padding, which names a row here, for an
    entry: caught at kmax 1, 15, 17, 33; at 16 no lane is behind kmax);
    corrupt indices are skipped and the good rows beside them arrive; every row of the destination nobody named, the 7 gap
    rows per segment of a wider destination and the guard rows around it keep the sentinel; mode 2 zeroes exactly what mode 0
    wrote; mode 1 adds in segment order."""
    from log_amd import dist as D
    R = 50
    gen = torch.Generator().manual_seed(100 + kmax)
    segs, S = _hand_segments(kmax, R, gen)
    assert segs.numel() == S * X.segment_floats(kmax)
    segs_d = torch.empty(segs.numel(), dtype=torch.float32, device=DEV)     # exactly the segments: the last one ends the allocation
    segs_d.copy_(segs)
    for dgr in (R, R + 7):
        buf, mid = _guarded(S * dgr)
        want = buf.clone()
        X.unpack_expect(want[mid], segs, S, kmax, R, dgr, 0)
        wrote = X.bits(want) != X.SENTINEL
        assert int(wrote.sum()) > 0 and not bool(wrote[mid].view(S, dgr, 16)[:, R:].any()) and not bool(wrote[mid][:dgr].any())
        assert not bool(wrote[mid].view(S, dgr, 16)[:, R // 2].any())     # the row every unspecified index names: nobody's
        dev = buf.to(DEV)
        _unpack(dev[mid], segs_d, S, kmax, R, dgr, 0)
        assert torch.equal(X.bits(dev.cpu()), X.bits(want)), dgr
        X.unpack_expect(want[mid], segs, S, kmax, R, dgr, 2)
        assert torch.equal(X.bits(want) == 0, wrote)
        _unpack(dev[mid], segs_d, S, kmax, R, dgr, 2)
        assert torch.equal(X.bits(dev.cpu()), X.bits(want)), dgr
    # through the package: the own-range store and its clear
    buf, mid = _guarded(S * R)
    want = buf.clone()
    X.unpack_expect(want[mid], segs, S, kmax, R, R, 0)
    dev = buf.to(DEV)
    D._unpack_segments(dev[mid], segs_d, S, kmax, per_segment_rows=R)
    torch.cuda.synchronize()
    assert torch.equal(X.bits(dev.cpu()), X.bits(want))
    X.unpack_expect(want[mid], segs, S, kmax, R, R, 2)
    D._unpack_segments(dev[mid], segs_d, S, kmax, per_segment_rows=R, zero=True)
    torch.cuda.synchronize()
    assert torch.equal(X.bits(dev.cpu()), X.bits(want))
    # the sum: every segment into the same R rows, in order, on top of what is there
    start = torch.randn(R, 16, generator=gen)
    for through_package in (False, True):
        buf, mid = _guarded(R, fill=start)
        want = buf.clone()
        X.unpack_expect(want[mid], segs, S, kmax, R, 0, 1)
        dev = buf.to(DEV)
        if through_package:
            D._unpack_segments(dev[mid], segs_d, S, kmax)
            torch.cuda.synchronize()
        else:
            _unpack(dev[mid], segs_d, S, kmax, R, 0, 1)
        assert torch.equal(X.bits(dev.cpu()), X.bits(want)), through_package


def test_summing_unpack_is_the_left_to_right_sum():
    """Mode 1 over five segments naming 33 of the same 40 rows each, magnitudes from 1e-3 to 1e3: the fp32 sum ((s0 + s1) +
    s2) + ... bit for bit, three runs.  Rows of NaN and of infinities propagate as IEEE addition says (inf + -inf is NaN;
    which NaN is not IEEE's business: the NaN entries are compared as NaN, all others as bits)."""
    R, kmax, S = 40, 33, 5
    gen = torch.Generator().manual_seed(77)
    groups = []
    for s in range(S):
        rest = [r for r in torch.randperm(R, generator=gen).tolist() if r not in (3, 5, 8)][:kmax - 3]
        idx = [(rest + [3, 5, 8])[j] for j in torch.randperm(kmax, generator=gen).tolist()]   # rows 3, 5 and 8 are in every segment
        vals = torch.randn(kmax, 16, generator=gen) * (10.0 ** torch.randint(-3, 4, (kmax, 1), generator=gen).float())
        if s == 2:
            vals[idx.index(3)] = float("nan")
        vals[idx.index(5)] = float("inf") if s % 2 == 0 else float("-inf")
        vals[idx.index(8), ::2] = float("inf")
        groups.append((kmax, idx, vals))
    segs = X.build_segments(groups, kmax)
    want = X.unpack_expect(torch.zeros(R, 16), segs, S, kmax, R, 0, 1)
    dense = torch.zeros(R, 16)                                            # the same sum, written as the formula
    for _, idx, vals in groups:
        d = torch.zeros(R, 16)
        d[idx] = vals
        dense = dense + d
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(dense), nan) and torch.equal(X.bits(dense)[~nan], X.bits(want)[~nan])
    assert bool(nan.any()) and bool(torch.isinf(want).any()) and not bool(nan.all(1)[[r for r in range(R) if r not in (3, 5)]].any())
    segs_d = segs.to(DEV)
    for _ in range(3):
        buf, mid = _guarded(R, fill=torch.zeros(R, 16))
        dev = buf.to(DEV)
        _unpack(dev[mid], segs_d, S, kmax, R, 0, 1)
        got = dev.cpu()
        assert bool((X.bits(got[:mid.start]) == X.SENTINEL).all()) and bool((X.bits(got[mid.stop:]) == X.SENTINEL).all())
        assert torch.equal(torch.isnan(got[mid]), nan) and torch.equal(X.bits(got[mid])[~nan], X.bits(want)[~nan])


@pytest.mark.parametrize("G,R", X.SCAN_SHAPES)
def test_round_trip_and_the_cpu_formulation(G, R):
    """unpack(pack(rows)) into a zeroed own-range destination is `rows` (a row of only -0.0 is not sent: +0.0), and both that
    and the sum over the groups are what the torch formulation gives for the same input on the CPU."""
    from log_amd import dist as D
    for density in ("half", "all"):
        rows, _ = X.planted(G, R, density)
        sel = X.select(rows)
        kmax = max(int(sel.sum(1).max()), 1)
        packed, over = _pack(rows.to(DEV), kmax)
        assert not over
        back = torch.zeros(G * R, 16, device=DEV)
        _unpack(back, packed, G, kmax, R, R, 0)
        want = torch.where(sel.view(-1)[:, None], X.bits(rows).view(-1, 16), torch.zeros((), dtype=torch.int32))
        assert torch.equal(X.bits(back.cpu()), want)
        cpu_packed, _ = D._pack_segments(rows.clone(), kmax)
        cpu_back = D._unpack_segments(torch.zeros(G * R, 16), cpu_packed, G, kmax, per_segment_rows=R)
        nan = torch.isnan(cpu_back)
        assert torch.equal(torch.isnan(back.cpu()), nan) and torch.equal(X.bits(back.cpu())[~nan], X.bits(cpu_back)[~nan])
        acc = torch.zeros(R, 16, device=DEV)
        _unpack(acc, packed, G, kmax, R, 0, 1)
        cpu_acc = torch.zeros(R, 16)
        for g in range(G):                                              # (segment after segment: the order the device promises)
            D._unpack_segments(cpu_acc, cpu_packed.view(G, -1)[g].contiguous(), 1, kmax)
        nan = torch.isnan(cpu_acc)
        assert torch.equal(torch.isnan(acc.cpu()), nan) and torch.equal(X.bits(acc.cpu())[~nan], X.bits(cpu_acc)[~nan])


# ---- seen += radii > 0 ---------------------------------------------------------------------------------------------------------
def _radii(n, gen, first):
    r = torch.randint(-5, 6, (n,), generator=gen, dtype=torch.int32)
    edge = torch.tensor([0, -1, INT32_MIN, INT32_MAX, 1], dtype=torch.int32).roll(first)
    r[:min(n, 5)] = edge[:min(n, 5)]
    return r


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_add_visible_counts_exactly(n):
    """lograst_add_visible and lograst_add_visible_n (k = 1, 15, 16 views) with n at, below and above a workgroup, radii 0,
    -1, INT32_MIN and INT32_MAX among them, counts that start non-zero: the exact integer sum, and nothing behind entry n."""
    _lib, L = _native()
    gen = torch.Generator().manual_seed(n)
    pad = 5
    for k in (0, 1, 15, 16):                                            # 0: the one-view entry point
        for first in range(5 if n == 1 else 1):
            views = [_radii(n, gen, first + j) for j in range(max(k, 1))]
            start = torch.randint(0, 100, (n,), generator=gen).float()
            buf = X.sentinel(n + 2 * pad).clone()
            buf[pad:pad + n] = start
            dev = buf.to(DEV)
            seen = dev[pad:pad + n]
            views_d = [v.to(DEV) for v in views]
            if k == 0:
                _lib.check(L.lograst_add_visible(seen.data_ptr(), views_d[0].data_ptr(), n, _stream()))
            else:
                table = torch.tensor([v.data_ptr() for v in views_d], dtype=torch.int64)
                _lib.check(L.lograst_add_visible_n(seen.data_ptr(), table.data_ptr(), k, n, _stream()))
            torch.cuda.synchronize()
            want = buf.clone()
            want[pad:pad + n] = start + sum((v > 0).float() for v in views)
            assert torch.equal(X.bits(dev.cpu()), X.bits(want)), (k, first)

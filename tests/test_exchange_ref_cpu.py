"""tests/exchange_ref.py (the restatement of the exchange's segment format that tests/test_gpu_exchange_edges.py holds the
kernels against) held against the torch formulation the gloo tests run -- log_amd.dist._pack_segments / _unpack_segments
on CPU tensors -- at every small shape of the device tests, special values included, and the facts about what a
"non-zero row" is.  The torch form's segment is [kmax][16 values | index], ascending, zero-padded, without a header; the
device's is header | values | index in any order: both decode to the same (count, index, values)."""
import pytest
import torch

import exchange_ref as X
from log_amd import dist as D


def _decode_torch_form(flat, G, kmax, counts):
    out = []
    seg = flat.view(G, kmax, D.SPARSE_FLOATS)
    for g in range(G):
        m = min(int(counts[g]), kmax)
        assert not X.bits(seg[g, m:]).any(), "the torch form pads with all-zero rows of index 0"
        out.append((int(counts[g]), X.bits(seg[g, :m, 16]), X.bits(seg[g, :m, :16])))
    return out


def _bounds(rows, sel, R):
    longest = max(int(sel.sum(1).max()), 1)
    ks = [longest] + ([longest - 1] if longest >= 2 else []) + ([17, 1] if R in (65, 1025) else [])
    return longest, ks


def test_what_a_non_zero_row_is():
    rows = torch.zeros(1, 8, 16)
    rows[0, 1] = float("nan")
    rows[0, 2] = float("inf")
    rows[0, 3] = X.DENORMAL
    rows[0, 4] = -0.0
    rows[0, 5, 15] = 1.0
    rows[0, 6, 0] = -1.0
    assert float(rows[0, 3, 0]) != 0.0 and X.bits(rows)[0, 4, 0].item() == X.NEG_ZERO       # (neither flushed away)
    want = [False, True, True, True, False, True, True, False]
    assert X.select(rows)[0].tolist() == want
    assert (rows != 0).any(2)[0].tolist() == want                      # IEEE comparison says the same
    assert (torch.count_nonzero(rows, dim=2) > 0)[0].tolist() == want   # ... and so does the torch form's count
    packed, counts, over = D._pack_rows(rows, 8)
    assert counts.tolist() == [5] and not bool(over)
    got = _decode_torch_form(packed.reshape(-1), 1, 8, counts)
    assert X.same_groups(got, X.expect(rows, X.select(rows), 8)[0]) == []
    assert got[0][1].tolist() == [1, 2, 3, 5, 6]
    # a hint word is tested as BITS: -0.0 is set; the hinted rows are taken whatever they hold, the others are not
    hint = torch.zeros(8)
    hint[0], hint[4], hint[7] = -0.0, 2.0, float("nan")
    assert X.select(rows, hint)[0].tolist() == [True, False, False, False, True, False, False, True]
    packed, counts, _ = D._pack_rows(rows, 8, hint=hint)
    assert counts.tolist() == [3]
    got = _decode_torch_form(packed.reshape(-1), 1, 8, counts)
    assert X.same_groups(got, X.expect(rows, X.select(rows, hint), 8)[0]) == [] and got[0][1].tolist() == [0, 4, 7]
    # rows behind the hint's end have none
    assert X.select(rows, hint[:5])[0].tolist() == [True, False, False, False, True, False, False, False]
    assert X.select(rows, hint, hint_rows=4)[0].tolist() == [True] + [False] * 7
    assert D._pack_rows(rows, 8, hint=hint[:5])[1].tolist() == [2]


@pytest.mark.parametrize("G,R", X.SCAN_SHAPES)
def test_planted_shapes_hold_what_they_promise(G, R):
    for density in X.DENSITIES:
        rows, special = X.planted(G, R, density)
        sel = X.select(rows)
        assert torch.equal(sel, (rows != 0).any(2))
        for g in range(G):
            for r in {0, R - 1} | {e for e in X.EDGES if e < R}:
                assert bool(sel[g, r])
        for name, where in special.items():
            for g, r in where:
                assert bool(sel[g, r]) == (name != "neg_zero"), (name, g, r)
                if name == "neg_zero":
                    assert (X.bits(rows)[g, r] == X.NEG_ZERO).all()
        if R >= 63:
            assert all(len(w) == G for w in special.values())
        if G * R >= 6:
            assert all(len(w) >= 1 for w in special.values())
        if density == "none":
            assert int(sel.sum()) <= G * 14
        if density == "all":
            assert int(sel.sum()) == G * R - len(special["neg_zero"])


@pytest.mark.parametrize("G,R", X.SCAN_SHAPES)
@pytest.mark.parametrize("density", X.DENSITIES)
def test_restatement_against_the_torch_formulation(G, R, density):
    rows, _ = X.planted(G, R, density)
    sel = X.select(rows)
    longest, ks = _bounds(rows, sel, R)
    for kmax in ks:
        want, over_want = X.expect(rows, sel, kmax)
        for clear in (False, True):
            bucket = rows.clone()
            flat, over = D._pack_segments(bucket, kmax, clear=clear)
            _, counts, _ = D._pack_rows(rows.clone(), kmax)
            assert bool(over) == over_want == (kmax < longest)
            got = _decode_torch_form(flat, G, kmax, counts)
            assert X.same_groups(got, want) == [], (kmax, clear)
            kept = torch.zeros(G, R, dtype=torch.bool)
            for g, (_, idx, _) in enumerate(want):
                kept[g, idx.long()] = True
            left = torch.where(kept[:, :, None], torch.zeros(()).int(), X.bits(rows)) if clear else X.bits(rows)
            assert torch.equal(X.bits(bucket), left), (kmax, clear)       # cleared rows are +0.0, every other row keeps its bits
        # the unpack, from the SAME lists in the device's format: own-range store, its clear, and the sum over groups
        mine = X.build_segments([(c, i.tolist(), v.view(torch.float32)) for c, i, v in want], kmax)
        assert X.same_groups(X.decode(mine, G, kmax), want) == []
        assert X.untouched_outside(mine, G, kmax, [c for c, _, _ in want]) == 0
        a = D._unpack_segments(torch.zeros(G * R, 16), flat, G, kmax, per_segment_rows=R)
        b = X.unpack_expect(torch.zeros(G * R, 16), mine, G, kmax, R, R, 0)
        nan = torch.isnan(b)
        assert torch.equal(torch.isnan(a), nan) and torch.equal(X.bits(a)[~nan], X.bits(b)[~nan])
        if kmax == longest:                                               # the round trip: -0.0-only rows come back as +0.0
            back = torch.where(sel.view(-1)[:, None], X.bits(rows).view(-1, 16), torch.zeros(()).int())
            assert torch.equal(X.bits(b), back)
        if G <= 3:
            a = D._unpack_segments(torch.zeros(R, 16), flat, G, kmax)
            b = X.unpack_expect(torch.zeros(R, 16), mine, G, kmax, R, 0, 1)
            nan = torch.isnan(b)
            assert torch.equal(torch.isnan(a), nan) and torch.equal(X.bits(a)[~nan], X.bits(b)[~nan])
        c = X.unpack_expect(X.unpack_expect(X.sentinel(G * R * 16).view(G * R, 16), mine, G, kmax, R, R, 0), mine, G, kmax, R, R, 2)
        assert int((X.bits(c) != X.SENTINEL).sum()) == 16 * sum(i.numel() for _, i, _ in want) and not c[X.bits(c) != X.SENTINEL].any()


@pytest.mark.parametrize("G,R", [(G, R) for G, R in X.SCAN_SHAPES if R in (5, 65, 1025, 2049)])
def test_restatement_with_hints(G, R):
    rows, _ = X.planted(G, R, "half")
    truthful = X.hint_for(X.select(rows))
    assert torch.equal(X.select(rows, truthful), X.select(rows))
    assert set(truthful.tolist()) >= set(X.HINT_WORDS) or G * R < 20
    gen = torch.Generator().manual_seed(R)
    other = X.hint_for(torch.rand(G, R, generator=gen) < 0.3, seed=1)   # hides non-zero rows, names all-zero ones
    for hint, n in ((truthful, G * R), (other, G * R), (other, (G - 1) * R + R // 2), (other, min(G * R, 1030))):
        sel = X.select(rows, hint, hint_rows=n)
        assert int(sel.view(-1)[n:].sum()) == 0
        kmax = max(int(sel.sum(1).max()), 1)
        want, _ = X.expect(rows, sel, kmax)
        for clear in (False, True):
            bucket = rows.clone()
            packed, counts, over = D._pack_rows(bucket, kmax, clear=clear, hint=hint[:n])
            assert not bool(over)
            assert X.same_groups(_decode_torch_form(packed.reshape(-1), G, kmax, counts), want) == []
            left = torch.where(sel[:, :, None], torch.zeros(()).int(), X.bits(rows)) if clear else X.bits(rows)
            assert torch.equal(X.bits(bucket), left)


def test_the_restatement_s_own_tools():
    assert [X.segment_floats(k) for k in (1, 15, 16, 17, 33)] == [48, 272, 288, 320, 592]
    vals = torch.arange(48.0).view(3, 16)
    seg = X.build_segments([(3, [7, -1, 2], vals), (9, [], vals[:0])], 5, beyond=(4, 123.0))
    assert seg.numel() == 2 * X.segment_floats(5)
    h, idx, v = X.decode_group(seg, 0, 5)
    assert h == 3 and idx.tolist() == [-1, 2, 7] and torch.equal(v.view(torch.float32), vals[[1, 2, 0]])
    h, idx, v = X.decode_group(seg, 1, 5)                                # a header above kmax: kmax entries are read
    assert h == 9 and idx.tolist() == [4] * 5 and (v.view(torch.float32) == 123.0).all()
    pad = X.bits(seg).view(2, -1)[:, 16 + 17 * 5:]                       # the index padding names the same row: entries 5 .. 15
    assert pad.shape == (2, 11) and bool((pad == 4).all())
    buf = X.sentinel(2 * X.segment_floats(5) + 32)
    assert X.untouched_outside(buf, 2, 5, [3, 9]) == 0
    X.bits(buf)[16 + 16 * 3] = 0                                          # a value behind the count
    X.bits(buf)[X.segment_floats(5) + 15] = 0                             # a header word: not held
    X.bits(buf)[-1] = 0                                                   # behind the last segment
    assert X.untouched_outside(buf, 2, 5, [3, 9]) == 2
    d = X.unpack_expect(torch.ones(12, 16), seg, 1, 5, 6, 6, 0)           # index 7 >= 6 rows and -1: skipped
    assert torch.equal(d[2], vals[2]) and float(d.sum()) == 11 * 16 + float(vals[2].sum())
    p = X.pattern_rows(5, 100, "cpu")
    assert p.shape == (100, 16) and bool((p > 0).all()) and torch.equal(p[10:20], X.pattern_rows(15, 10, "cpu"))
    assert p.unique().numel() > 1500

"""A plain restatement of the row-sparse exchange's segment format (log_amd/csrc/exchange.hip:1-12, include/lograst.h) that
tests/test_gpu_exchange_edges.py holds the kernels against, and tests/test_exchange_ref_cpu.py holds against the torch
formulation the gloo tests run.  Written from the format alone: nothing here calls log_amd.dist.

A segment of bound kmax:  header [16] (word 0: the rows found, may exceed kmax) | values [kmax][16] | index [roundup(kmax, 16)]
(int32 bits, the row inside its group).  Everything is compared as int32 BITS, so NaN payloads and -0.0 count.  All
functions work on tensors of any device and keep their results there."""
import torch

ROW = 16
SENTINEL = 0x5A5A5A5A                     # the bits of every float a test owns and the kernels must not touch (1.5e16 as a float)
NEG_ZERO = -0x80000000                    # the int32 value of the bits of -0.0
DENORMAL = 1e-42


def segment_floats(kmax):
    return 16 + 16 * kmax + (kmax + 15) // 16 * 16


def bits(t):
    """The int32 view of a 4-byte tensor."""
    return t if t.dtype == torch.int32 else t.contiguous().view(torch.int32)


def sentinel(n, device="cpu"):
    """n floats whose bits are SENTINEL."""
    return torch.full((int(n),), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def select(rows, hint=None, hint_rows=None):
    """rows float32 [G, R, 16] -> bool [G, R]: the rows a pack takes.
    Without a hint: a row with an entry that differs from zero by IEEE comparison -- any bit besides the sign set, so NaN,
    inf and denormals select and -0.0 does not (written on the bits: no flush-to-zero mode can change the answer).
    With a hint (one 4-byte word per row of all groups in order): the rows whose word is non-zero AS BITS and whose flat
    position is below hint_rows (default: the hint's length), whatever the rows hold."""
    G, R, _ = rows.shape
    if hint is None:
        return ((bits(rows) & 0x7FFFFFFF) != 0).any(dim=2)
    n = int(hint.numel()) if hint_rows is None else int(hint_rows)
    n = min(n, G * R, int(hint.numel()))
    sel = torch.zeros(G * R, dtype=torch.bool, device=rows.device)
    sel[:n] = bits(hint).reshape(-1)[:n] != 0
    return sel.view(G, R)


def decode_group(packed, g, kmax):
    """One segment of a flat buffer of back-to-back segments -> (header count, index int32 [m], values int32 bits [m, 16]),
    m = min(header, kmax), sorted by index.  Nothing behind entry m is read."""
    seg = segment_floats(kmax)
    p = bits(packed)[g * seg:(g + 1) * seg]
    header = int(p[0].item())
    m = min(max(header, 0), kmax)
    idx = p[16 + 16 * kmax:16 + 16 * kmax + m]
    idx, order = torch.sort(idx, stable=True)
    return header, idx, p[16:16 + 16 * m].view(m, ROW)[order]


def decode(packed, G, kmax):
    return [decode_group(packed, g, kmax) for g in range(G)]


def expect_group(rows, sel, g, kmax):
    """What decode_group gives for group g of a pack of `rows` that took the rows `sel`: every selected row in ascending
    order (when there are more than kmax the kernels keep ANY kmax of them; this lists the first kmax)."""
    r = torch.nonzero(sel[g]).reshape(-1)
    count = int(r.numel())
    r = r[:kmax]
    return count, r.to(torch.int32), bits(rows)[g, r]


def expect(rows, sel, kmax):
    """-> (per group (count, index, values), overflow flag = any(count > kmax))."""
    out = [expect_group(rows, sel, g, kmax) for g in range(rows.shape[0])]
    return out, any(c > kmax for c, _, _ in out)


def same_groups(got, want):
    """decode(...) == expect(...)[0], bit for bit -> the list of groups that differ (empty = equal)."""
    bad = []
    for g, ((h, i, v), (c, wi, wv)) in enumerate(zip(got, want)):
        if h != c or i.shape != wi.shape or not torch.equal(i, wi) or not torch.equal(v, wv):
            bad.append(g)
    return bad


def untouched_outside(packed, G, kmax, counts):
    """Did every float of a sentinel-filled buffer of G segments keep the sentinel -- outside each segment's header, its
    values and indices below min(count, kmax), and the padding of its index block (kmax .. roundup(kmax, 16))?  Floats
    behind the last segment (guard room the caller added) must keep it too.  -> the number of floats that did not."""
    seg = segment_floats(kmax)
    p = bits(packed)
    free = torch.ones(p.numel(), dtype=torch.bool, device=p.device)
    body = free[:G * seg].view(G, seg)
    body[:, :16] = False
    body[:, 16 + 17 * kmax:] = False
    for g in range(G):
        m = min(int(counts[g]), kmax)
        body[g, 16:16 + 16 * m] = False
        body[g, 16 + 16 * kmax:16 + 16 * kmax + m] = False
    return int(((p != SENTINEL) & free).sum().item())


def build_segments(groups, kmax, beyond=None):
    """Hand-built segments for the unpack: groups = [(header, index list, values float32 [n, 16])], n <= kmax entries each.
    Every float the format leaves unspecified (header words 1-15, entries behind n, the index padding) is the sentinel, or
    -- entries behind n, the index padding kmax .. roundup(kmax, 16) included -- what beyond = (index, value) says: a
    reader that went too far, past n or past kmax, then WRITES somewhere a test looks."""
    seg = segment_floats(kmax)
    out = bits(sentinel(len(groups) * seg)).clone()
    for g, (header, idx, vals) in enumerate(groups):
        s = out[g * seg:(g + 1) * seg]
        n = len(idx)
        assert n <= kmax
        if beyond is not None:
            s[16 + 16 * n:16 + 16 * kmax] = bits(torch.tensor([beyond[1]], dtype=torch.float32))[0]
            s[16 + 16 * kmax + n:] = int(beyond[0])
        s[0] = int(header)
        if n:
            s[16:16 + 16 * n] = bits(torch.as_tensor(vals, dtype=torch.float32)).reshape(-1)
            s[16 + 16 * kmax:16 + 16 * kmax + n] = torch.tensor(idx, dtype=torch.int64).to(torch.int32)
    return out.view(torch.float32)


def unpack_expect(dest, packed, segments, kmax, rows_per_group, dest_group_rows, mode):
    """The unpack, row by row on the host.  dest float32 [rows, 16] (changed in place and returned).  mode 0: segment s's
    rows stored into rows s * dest_group_rows + index; 2: zeros stored there; 1: all segments added into rows `index`, in
    segment order, one fp32 addition each.  A header above kmax counts as kmax; an index outside [0, rows_per_group) is
    skipped."""
    d = dest
    for s in range(segments):
        header, idx, vals = decode_group(packed, s, kmax)
        vals = vals.view(torch.float32)
        for j in range(idx.numel()):
            r = int(idx[j])
            if r < 0 or r >= rows_per_group:
                continue
            if mode == 1:
                d[r] = d[r] + vals[j]
            elif mode == 2:
                d[s * dest_group_rows + r] = 0.0
            else:
                d[s * dest_group_rows + r] = vals[j]
    return d


# ---- the planted shapes (shared by the CPU and the device tests) --------------------------------------------------------
SCAN_R = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)   # the scanning pack: 1024 rows per workgroup, rounds of 256, waves of 64
SCAN_SHAPES = [(G, R) for G in (1, 3) for R in SCAN_R] + [(300, 5)]   # 300 groups: a second workgroup of the header clear
DENSITIES = ("none", "all", "half")
EDGES = (63, 64, 255, 256, 1023, 1024)
SPECIALS = ("nan", "neg_zero", "denormal", "inf", "col0", "col15")


def _mixed(n, gen):
    """n rows of non-zero floats of mixed magnitude."""
    v = torch.randn(n, ROW, generator=gen) * (10.0 ** torch.randint(-3, 4, (n, 1), generator=gen).float())
    return torch.where(v == 0, torch.ones_like(v), v)


def planted(G, R, density, seed=0):
    """-> (rows float32 [G, R, 16], special {name: [(g, r)]}).  Density "none" / "all" / "half" fills no, every or a random
    half of the rows; then the first and last row of every group and both rows at 63|64, 255|256, 1023|1024 (those that
    exist) are made non-zero, and as many of the special rows as the group has free rows are planted, group g starting the
    list at its g-th name: only NaN, only -0.0 (NOT a non-zero row), only a denormal, only +inf, only column 0, only column
    15."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * G + R + DENSITIES.index(density))
    rows = torch.zeros(G, R, ROW)
    if density == "all":
        rows.view(-1, ROW)[:] = _mixed(G * R, gen)
    elif density == "half":
        take = torch.rand(G, R, generator=gen) < 0.5
        rows[take] = _mixed(int(take.sum()), gen)
    fixed = sorted({0, R - 1} | {e for e in EDGES if e < R})
    special = {name: [] for name in SPECIALS}
    for g in range(G):
        rows[g, fixed] = _mixed(len(fixed), gen)
        free = [int(r) for r in torch.randperm(R, generator=gen) if int(r) not in fixed][:len(SPECIALS)]
        for k, r in enumerate(free):
            name = SPECIALS[(g + k) % len(SPECIALS)]
            row = torch.zeros(ROW)
            if name == "nan":
                row[:] = float("nan")
            elif name == "neg_zero":
                row[:] = -0.0
            elif name == "denormal":
                row[:] = DENORMAL
            elif name == "inf":
                row[:] = float("inf")
            elif name == "col0":
                row[0] = 0.75
            else:
                row[15] = -3.0
            rows[g, r] = row
            special[name].append((g, r))
    return rows, special


HINT_WORDS = (0x3F800000, NEG_ZERO, 1, 0x7FC00000, -1)      # 1.0, -0.0, a denormal, NaN, all ones: every one is "set"


def hint_for(sel, seed=0):
    """An int32 hint word per row (flat, all groups) that is non-zero exactly on `sel`, cycling through HINT_WORDS."""
    flat = sel.reshape(-1)
    words = torch.tensor(HINT_WORDS, dtype=torch.int64)[(torch.arange(flat.numel()) + seed) % len(HINT_WORDS)].to(torch.int32)
    return torch.where(flat.cpu(), words, torch.zeros_like(words)).to(sel.device)


def pattern_of(flat_rows):
    """The rows `flat_rows` (int64 [n], positions in the flat array of all groups) of an endless array in which EVERY float
    is non-zero: int32 bits [n, 16], a function of the flat element index alone -- a large bucket is filled and checked
    chunk by chunk, and its packed rows are known, without a second copy of it."""
    e = flat_rows.to(torch.int64)[:, None] * ROW + torch.arange(ROW, dtype=torch.int64, device=flat_rows.device)
    return ((((e * 2654435761 + 12345) >> 9) & 0x7FFFFFFF) | 1).to(torch.int32)


def pattern_rows(first_row, n, device):
    return pattern_of(torch.arange(first_row, first_row + n, dtype=torch.int64, device=device))


def hinted_rows_per_block(G, R):
    """The hinted pack's launch rule (lx_launch_pack_rows), restated: about 4096 workgroups in all, each owning a multiple
    of 256 rows of one group, 1024 at least and 16384 (the 16-bit list in LDS) at most -> (rows per block, blocks per group)."""
    per = max(4096 // G, 1)
    rpb = min(max((-(-R // per) + 255) // 256 * 256, 1024), 16384)
    return rpb, -(-R // rpb)

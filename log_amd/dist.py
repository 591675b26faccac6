"""View-sharded data parallelism for the rasterizer path (new design; the reference is single-GPU,
SURVEY.md 2.2 / 8e).

One process per GPU.  Gaussian attributes are replicated; rank r renders views {v : v % world == r};
each view's backward accumulates into ONE flat fp32 gradient buffer per rank (every attribute's ``.grad``
is a view into it), so a step needs exactly one exchange.  Two forms:

  * ``GradientBucket.reduce()``: sum of the whole buffer across ranks, issued as reduce-scatter + all-gather over
    the Gaussian dimension (RCCL over xGMI on the MI355X node; ``gloo`` for the CPU tests) -- every rank then holds
    every gradient and steps its own replica;
  * owner-computes (``OwnerAdam``): after the reduce-scatter rank r owns rows
    [r P/world, (r+1) P/world) of every attribute; it alone runs the sparse Adam of
    /root/reference/LoG/model/sparse_optimizer.py:41-78,163-196 on them (the HIP kernel behind
    ``lograst_sparse_adam``), with moments that exist for ITS rows only -- optimizer state and optimizer work are
    divided by world -- and the updated attribute rows are all-gathered (same bytes as the gradient all-gather they
    replace).  The reference updates only the rows seen this step (``flag_vis``, sparse_optimizer.py:167): the bucket
    carries a per-row ``seen`` count next to the gradients for exactly that.

Three refinements of the exchange, each optional and each leaving the result unchanged:

  * **touched-row blocks** (``block_rows`` > 0, ``compact=True``): a level-of-detail step touches a fraction of the model's
    rows, and a row no view saw has an exactly zero gradient and does not move.  The ranks first agree on which
    ``block_rows``-row blocks anyone touched (a max-reduce of world x nb flags: P / block_rows bytes), then only those
    blocks travel: owner r receives the sum of ITS touched blocks, and publishes only those after the update.  Every rank
    derives the same block lists from the same bitmap, padded per owner to the longest list with UNTOUCHED blocks of that
    owner (zero gradients / unchanged attributes: sending them is a no-op, so there is no mask and no variable-size
    collective).  Falls back to the dense form when most blocks are touched;
  * **row-sparse** (``sparse=True``, row-major buckets): with an opaque scene a view's gradients live in the few per cent
    of the rows that composited somewhere (30 M Gaussians, 8 views of a rank: 24 % of the rows; measured,
    tools/touched_rows.py), and at 4096-row -- even 16-row -- granularity every block holds one.  Only the touched ROWS
    travel: every rank packs (row index, 16 sums) of its touched rows per owner into equal-sized, padded segments (an
    all-to-all with equal splits: no sizes on the wire, no host read-back once the bound is known), the owner adds what it
    receives into its shard, and the closing all-gather moves the shard's non-zero rows the same way;
  * **overlap** (``StepExchange``, ``parts`` > 1): the step's views are split into `parts` groups with a bucket each; the
    reduce-scatter of group g is issued on a side stream as soon as g's last backward is enqueued and runs under the
    rendering of group g + 1.  Only the last group's reduce-scatter and the closing all-gather are exposed.

With world_size == 1 nothing is communicated and results are bit-identical to the single-GPU path.
"""
import contextlib
import math
import os

import torch
import torch.distributed as dist

# per-Gaussian gradient columns: means3D 3, scales 3, rotations 4, opacities 1, colors 3  (14 floats)
LAYOUT = (("means3D", 3), ("scales", 3), ("rotations", 4), ("opacities", 1), ("colors", 3))
COLS = sum(c for _, c in LAYOUT)


ROW_FLOATS = 16            # row-major form: one 64-byte row per Gaussian (include/lograst.h: LOGRAST_GRAD_ROW_FLOATS)
ROW_COLUMNS = {"means3D": (0, 3), "scales": (3, 6), "rotations": (6, 10), "opacities": (10, 11), "colors": (11, 14)}


def layout(sh_coeffs=0, row_major=False):
    """Columns of the exchange: LAYOUT (14 floats) + the SH coefficients [K, 3] when the model has them (SURVEY 8e:
    +9 at degree 1, +45 at degree 3).  row_major: the 14 base columns travel as ONE block of 16-float rows ("rows")."""
    base = (("rows", ROW_FLOATS),) if row_major else LAYOUT
    return base + ((("shs", 3 * int(sh_coeffs)),) if sh_coeffs else ())


def split_rows(grads):
    """dict with a "rows" entry ([n, 16]) -> the same dict with per-attribute (strided) views of it instead."""
    if "rows" not in grads:
        return grads
    out = {k: v for k, v in grads.items() if k != "rows"}
    for name, (a, b) in ROW_COLUMNS.items():
        out[name] = grads["rows"][:, a:b]
    return out


def shard_views(n_views, rank, world):
    """The views of `rank`: view v belongs to rank v % world."""
    return list(range(rank, n_views, world))


def rows_per_rank(num_points, world, block_rows=0):
    """Rows owned by one rank: a whole number of `block_rows`-row blocks when the touched-block exchange is on, and
    always a multiple of 4 rows -- the attribute blocks of `_Flat` sit back to back, a block of c columns is
    P_pad * c * 4 bytes, and the kernels read / write the 4-column blocks (rotations, dL/drotations) as 16-byte rows
    (lograst_forward / lograst_backward reject pointers that are not 16-byte aligned): with P_pad % 4 == 0 every block and
    every rank's slice of it starts on a 16-byte boundary whatever the point count (LoG's changes at every densify)."""
    per = (int(num_points) + max(int(world), 1) - 1) // max(int(world), 1)
    unit = math.lcm(int(block_rows) if block_rows else 1, 4)
    return (per + unit - 1) // unit * unit


def _single_rank_forced():
    """LOGRAST_DIST_SINGLE_RANK=1 (diagnostics; bench.py, tests/test_gpu_dist.py): a world of ONE rank still goes through
    every collective -- on a one-GPU box that runs the RCCL branches below for real (one-rank RCCL calls on the device)."""
    return os.environ.get("LOGRAST_DIST_SINGLE_RANK", "0") == "1"


def _active(world):
    return dist.is_initialized() and (world > 1 or _single_rank_forced())


def _reduce_scatter(out, inp, group=None):
    """out[numel / world] = this rank's slice of the sum of `inp` over ranks.  gloo (the CPU tests) has no
    reduce_scatter_tensor: all_reduce of a copy, then the slice."""
    if dist.get_backend(group) == "gloo":
        tmp = inp.clone()
        dist.all_reduce(tmp, op=dist.ReduceOp.SUM, group=group)
        r, n = dist.get_rank(group), out.numel()
        out.copy_(tmp[r * n:(r + 1) * n])
    else:
        dist.reduce_scatter_tensor(out, inp, op=dist.ReduceOp.SUM, group=group)
    return out


def _all_gather(out, inp, group=None):
    """out[world * numel] = the ranks' `inp` in rank order."""
    if dist.get_backend(group) == "gloo":
        parts = [torch.empty(inp.shape, dtype=inp.dtype, device=inp.device) for _ in range(dist.get_world_size(group))]
        dist.all_gather(parts, inp.contiguous(), group=group)
        out.copy_(torch.cat(parts))
    else:
        dist.all_gather_into_tensor(out, inp.contiguous(), group=group)
    return out


SPARSE_FLOATS = ROW_FLOATS + 1     # a packed row of the row-sparse exchange: 16 running sums | row index (int32 bits)


def _clamp(k, limit):
    """A list length the collectives are sized for: at least one entry (nothing touched: one of padding), at most all."""
    return min(max(int(k), 1), limit)


def _row_bound(rows, kmax, group):
    """Rows per segment of a row-sparse collective over rows [G, R, 16]: the caller's bound `kmax`, or (None) the longest
    list of non-zero rows any group holds on any rank, exactly -- one max-reduce and one device -> host read."""
    if kmax is None:
        cnt = (rows != 0).any(dim=2).sum(1).max().reshape(1)
        dist.all_reduce(cnt, op=dist.ReduceOp.MAX, group=group)
        kmax = cnt.item()
    return _clamp(kmax, rows.shape[1])


def _pack_rows(rows, kmax, clear=False, hint=None):
    """clear: the packed rows are zeroed in `rows` afterwards (pack and clear; rows dropped by an exceeded kmax stay).
    hint: see _pack_segments (the rows to pack are those with a non-zero hint word, whatever they hold).
    rows: float32 [G, R, 16] (G groups of R rows).  -> (packed float32 [G, kmax, 17], counts int64 [G], overflow bool):
    per group the rows with a non-zero entry, in ascending row order, as (16 values | row index inside the group, int32
    bits), padded with all-zero rows of index 0 (adding them is a no-op).  No host synchronisation: kmax is the caller's
    bound; `overflow` (a device flag) is raised when a group holds more than kmax such rows (the excess is dropped)."""
    G, R, C = rows.shape
    dev = rows.device
    if hint is None:
        nz = torch.count_nonzero(rows, dim=2) > 0                 # [G, R]
    else:                             # (a hinted row is packed whatever it holds; the others are not looked at)
        nz = torch.zeros(G * R, dtype=torch.bool, device=dev)
        n = min(int(hint.numel()), G * R)
        nz[:n] = hint.reshape(-1)[:n].view(torch.int32) != 0
        nz = nz.view(G, R)
    csum = torch.cumsum(nz.view(-1).to(torch.int32), 0).view(G, R)
    before = torch.cat([csum.new_zeros(1), csum[:-1, -1]])        # non-zero rows in front of each group
    rank = csum - 1 - before[:, None]                             # position of a non-zero row inside its group's list
    counts = (csum[:, -1] - before).to(torch.int64)
    keep = nz & (rank < kmax)
    # every row is sent somewhere: kept rows to their slot, all others to one scratch slot behind the buffer
    slot = torch.where(keep, torch.arange(G, device=dev)[:, None] * kmax + rank, G * kmax).view(-1).to(torch.int64)
    del nz, csum, rank, keep
    packed = torch.zeros(G * kmax + 1, SPARSE_FLOATS, dtype=torch.float32, device=dev)
    packed[:, :C].index_copy_(0, slot, rows.reshape(G * R, C))
    idx = torch.arange(R, dtype=torch.int32, device=dev).view(torch.float32).repeat(G)
    packed[:, C].index_copy_(0, slot, idx)
    packed[G * kmax].zero_()                                      # (the scratch slot is not part of the result)
    if clear:
        rows.view(G * R, C)[slot < G * kmax] = 0
    return packed[:G * kmax].view(G, kmax, SPARSE_FLOATS), counts, (counts > kmax).any()


def _unpack_add(dest, packed):
    """dest: float32 [R, 16]; packed: [..., 17] rows of (16 values | row index).  dest[index] += values (padding rows
    add zeros to row 0)."""
    flat = packed.reshape(-1, SPARSE_FLOATS)
    dest.index_add_(0, flat[:, ROW_FLOATS].contiguous().view(torch.int32).to(torch.int64), flat[:, :ROW_FLOATS])
    return dest


# ---- the same on the device: lograst_pack_rows / lograst_unpack_rows (log_amd/csrc/exchange.hip) ----------------------
# The torch formulation above is what the CPU tests run (gloo); on a 30 M-row bucket it takes 6 ms to pack, 30 ms to add
# 8 M received rows (index_add_) and 180 ms to put the gathered rows back -- the kernels stream (a segment there is
# header | values | indices, lograst_sparse_segment_floats(kmax) floats: include/lograst.h).
def _native():
    """-> (check, library, _ptr, _stream_ptr): liblograst.so with the error check of its return codes and the rasterizer's
    marshalling of tensors and of the current stream.  Imported on first use: importing this module loads no library."""
    from . import _lib
    from .rasterizer import _ptr, _stream_ptr
    return _lib.check, _lib.lib(), _ptr, _stream_ptr


def _segment_floats(kmax, device):
    if device.type != "cuda":
        return int(kmax) * SPARSE_FLOATS
    return int(_native()[1].lograst_sparse_segment_floats(int(kmax)))


def _pack_segments(rows, kmax, clear=False, hint=None):
    """rows [G, R, 16] -> (flat float32 buffer of G equal segments, overflow: device bool).  clear: every packed row is
    zeroed in `rows` (which must then be the bucket's own contiguous storage: lograst_pack_rows_clear).
    hint: a 4-byte-per-row tensor over the rows of ALL groups in order (fewer entries: the rows behind them have none) whose
    zero words mark rows the caller KNOWS to be zero -- they are not read; rows with a non-zero word are packed whatever they
    hold (lograst_pack_rows_hinted: the pack then knows its rows from the hints alone)."""
    if rows.device.type != "cuda":
        packed, _, over = _pack_rows(rows, kmax, clear=clear, hint=hint)
        return packed.reshape(-1), over
    check, L, ptr, stream_ptr = _native()
    G, R, _ = rows.shape
    assert rows.is_contiguous() or not clear, "pack and clear works on the bucket's own storage"
    rows = rows.contiguous()
    packed = torch.empty(G * _segment_floats(kmax, rows.device), dtype=torch.float32, device=rows.device)
    flag = torch.zeros(1, dtype=torch.int32, device=rows.device)
    with torch.cuda.device(rows.device):
        if hint is not None:
            assert hint.is_contiguous() and hint.element_size() == 4 and hint.device == rows.device
            check(L.lograst_pack_rows_hinted(ptr(rows), G, R, int(kmax), ptr(packed), ptr(flag), 1 if clear else 0,
                                             ptr(hint), int(hint.numel()), stream_ptr(rows.device)))
        else:
            fn = L.lograst_pack_rows_clear if clear else L.lograst_pack_rows
            check(fn(ptr(rows), G, R, int(kmax), ptr(packed), ptr(flag), stream_ptr(rows.device)))
    return packed, flag[0] != 0


def _unpack_segments(dest, packed, segments, kmax, per_segment_rows=0, zero=False):
    """dest [R, 16] += the rows of all `segments` (per_segment_rows = 0), or dest [segments * per_segment_rows, 16]: segment s's
    rows written into its own range (the destination must be zeroed: only non-zero rows arrive).  zero (owner-major form
    only): the rows the segments name are CLEARED instead -- undoes an earlier call with the same `packed`."""
    if dest.device.type != "cuda":
        segs = packed.view(segments, kmax, SPARSE_FLOATS)
        if per_segment_rows and zero:
            for r in range(segments):
                idx = segs[r][:, ROW_FLOATS].contiguous().view(torch.int32).to(torch.int64)
                keep = segs[r][:, :ROW_FLOATS].ne(0).any(dim=1)                   # (padding rows name row 0: not theirs to clear)
                dest[r * per_segment_rows:(r + 1) * per_segment_rows][idx[keep]] = 0
        elif per_segment_rows:
            for r in range(segments):
                _unpack_add(dest[r * per_segment_rows:(r + 1) * per_segment_rows], segs[r])
        else:
            _unpack_add(dest, segs)
        return dest
    check, L, ptr, stream_ptr = _native()
    rows_per_group = int(per_segment_rows) if per_segment_rows else int(dest.shape[0])
    with torch.cuda.device(dest.device):
        check(L.lograst_unpack_rows(ptr(dest), ptr(packed), int(segments), int(kmax), rows_per_group, int(per_segment_rows),
                                    (2 if zero else 0) if per_segment_rows else 1, stream_ptr(dest.device)))
    return dest


def _all_to_all(out, inp, group=None):
    """Equal splits: segment r of `inp` goes to rank r, segment s of `out` comes from rank s.  gloo (the CPU tests, and two
    ranks sharing one GPU in tests/test_gpu_dist.py) has no all-to-all for device tensors: all-gather, then the segments."""
    inp = inp.contiguous()
    if dist.get_backend(group) == "gloo" and inp.is_cuda:
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        parts = [torch.empty(inp.shape, dtype=inp.dtype, device=inp.device) for _ in range(world)]
        dist.all_gather(parts, inp, group=group)
        n = inp.numel() // world
        out.copy_(torch.cat([p[rank * n:(rank + 1) * n] for p in parts]))
    else:
        dist.all_to_all_single(out, inp, group=group)
    return out


def _shape(name, rows, cols):
    return (rows, cols // 3, 3) if name == "shs" else (rows, cols)


class _Flat:
    """One flat fp32 buffer holding every attribute as a contiguous [P_pad, c] block, P_pad = world * ceil(P / world), so
    that rank r's rows [r * Pr, (r + 1) * Pr) are a contiguous slice of every block.  row_major: the 14 base columns are
    ONE block "rows" of 16-float (64-byte) rows -- what the rasterizer's backward adds into with one read-modify-write per
    Gaussian (``sink()``) and what travels as one collective; ``alias[name]`` are strided per-attribute views of it."""

    def __init__(self, num_points, device, world=1, sh_coeffs=0, block_rows=0, row_major=False):
        self.P, self.world = int(num_points), max(int(world), 1)
        self.row_major = bool(row_major)
        self.layout = layout(sh_coeffs, self.row_major)
        self.block_rows = int(block_rows)
        self.Pr = rows_per_rank(self.P, self.world, self.block_rows)
        self.Ppad = self.Pr * self.world
        self.cols = sum(c for _, c in self.layout)
        self.flat = torch.zeros(self.Ppad * self.cols, dtype=torch.float32, device=device)
        self.blocks, self.views, off = {}, {}, 0
        for name, c in self.layout:
            blk = self.flat[off:off + self.Ppad * c]
            self.blocks[name] = blk                                           # [P_pad * c], padding rows included
            self.views[name] = blk[:self.P * c].view(_shape(name, self.P, c))  # what the kernels see
            off += self.Ppad * c
        self.alias = dict(self.views)
        if self.row_major:
            for name, (a, b) in ROW_COLUMNS.items():
                self.alias[name] = self.views["rows"][:, a:b]

    def sink(self):
        """What ``log_amd.rasterizer.accumulate_grads_into`` takes.  A row-major bucket WITH SH coefficients has no
        rasterizer sink (the chain rule's row-major form adds dL/dcolour into the row; with native `shs=` the colour is an
        intermediate): attach the attributes' .grad to ``alias[...]`` instead (autograd route), or build the bucket
        attribute-major (row_major=False), whose sink takes an "shs" entry."""
        if self.row_major and "shs" in self.views:
            raise ValueError("a row-major gradient bucket with SH coefficients has no rasterizer sink: use "
                             "row_major=False (its sink has an 'shs' entry) or attach .grad to bucket.alias[...]")
        return dict(self.views)

    def rows(self, name, rank):
        """Rank `rank`'s rows of attribute `name`: a contiguous [Pr, c] view."""
        c = dict(self.layout)[name]
        return self.blocks[name][rank * self.Pr * c:(rank + 1) * self.Pr * c].view(self.Pr, c)


class TouchedBlocks:
    """Which `block_rows`-row blocks of each owner any rank touched this step, as every rank computes it from the same
    max-reduced bitmap: ``order[r]`` = owner r's block ids, touched ones first (ascending), and ``kmax`` = the length the
    collectives are sized for.  Entries [count_r, kmax) of ``order[r]`` are untouched blocks of owner r -- padding that
    carries zeros / unchanged rows.

    kmax=None: the longest touched list over the owners, exactly -- one small device -> host read per exchange (the
    collectives need their sizes on the host).  kmax=K (a bound the caller keeps from earlier steps, e.g. the warm-up's
    longest list + headroom): NO read-back; ``overflow`` is a device flag that is raised when some owner touched more than
    K blocks (the exchange then dropped gradient rows: the caller checks the flag at a point where it synchronises anyway
    -- ``StepExchange.compact_overflowed()`` -- and repeats the step dense or with a larger bound)."""

    def __init__(self, bitmap, kmax=None):
        self.bitmap = bitmap                                   # bool [world, nb]
        self.world, self.nb = bitmap.shape
        self.counts = bitmap.sum(1)
        self.kmax = _clamp(self.counts.max().item() if kmax is None else kmax, self.nb)
        self.overflow = None if kmax is None else self.counts.max() > self.kmax       # device bool, no synchronisation
        self.bound = kmax
        self.order = torch.argsort((~bitmap).to(torch.uint8), dim=1, stable=True)[:, :self.kmax].contiguous()

    def union(self, other):
        """Blocks touched by either.  Bounded form: the union of two lists of at most K blocks can hold up to 2 K, so the
        union is sized for the SUM of the parts' bounds (sized for max(K, K), an owner whose parts touched disjoint
        blocks would publish only its first K, and the other updated rows would never reach the replicas); its own
        overflow flag (impossible unless a part overflowed) is folded in all the same."""
        out = TouchedBlocks(self.bitmap | other.bitmap,
                            kmax=None if self.bound is None else min(self.kmax + other.kmax, self.nb))
        for o in (self.overflow, other.overflow):
            if o is not None:
                out.overflow = o if out.overflow is None else (out.overflow | o)
        return out

    @property
    def fraction(self):
        """Share of the dense exchange the compact one moves (padding included)."""
        return self.kmax / max(self.nb, 1)


class GradientBucket(_Flat):
    """Flat gradient buffer, attribute-major, with one contiguous view per attribute, and the per-row `seen` count."""
    DENSE_ABOVE = 0.85     # touched-block exchange only when it moves less than this share of the dense one

    def __init__(self, num_points, device, world=1, sh_coeffs=0, block_rows=0, track_seen=True, row_major=False):
        """track_seen=False: no per-row `seen` counts (nothing to exchange for them) -- for a caller that only wants the
        gradient sum, like bench.py; the owner-computes step needs them."""
        super().__init__(num_points, device, world, sh_coeffs, block_rows, row_major)
        self.pad = self.flat.numel() - self.P * self.cols
        self.track_seen = bool(track_seen)
        # views that saw the row this step (one float when not tracked: mark_seen / the touched-block exchange then refuse)
        self._seen = torch.zeros(self.Ppad if self.track_seen else 1, dtype=torch.float32, device=device)
        self._seen_pending = []      # radii tensors of mark_seen(defer=True), not yet counted (see the `seen` property)
        self._seen_dirty = False     # somebody marked the counts since the last reset
        self._seen_reduced = False
        self.touched = None                                   # TouchedBlocks of the last compact exchange (else None)
        self.touch_hint, self._hint_calls = None, 0           # mark_touched
        self.sparse_overflow, self.sparse_kmax = None, 0      # the last row-sparse exchange's device flag and rows per segment

    def attach(self, params):
        """params: dict name -> leaf tensor (requires_grad).  Their .grad become views of the bucket,
        so autograd accumulates every view's gradient in place -- and the rasterizer's backward may add into them directly
        (log_amd.rasterizer.allow_inplace_grad: the caller of attach() owns these leaves and steps them with plain
        ``.backward()`` calls; torch.autograd.grad / backward(inputs=...) on them is not supported)."""
        from .rasterizer import allow_inplace_grad
        for name in (list(ROW_COLUMNS) + [n for n, _ in self.layout if n != "rows"]) if self.row_major else [n for n, _ in self.layout]:
            p = params[name]
            assert p.shape == self.alias[name].shape, (name, p.shape)
            p.grad = self.alias[name]
            allow_inplace_grad(p)

    @property
    def seen(self):
        """float32 [P_pad] (1 without track_seen): how many of this step's views saw each row.  Reading it counts whatever
        ``mark_seen(defer=True)`` left pending -- on the current stream, in one pass over up to 16 views."""
        self._flush_seen()
        return self._seen

    def _flush_seen(self):
        pend, self._seen_pending = self._seen_pending, []
        if not pend:
            return
        check, L, ptr, stream_ptr = _native()
        dev = self._seen.device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            for k0 in range(0, len(pend), 16):
                part = pend[k0:k0 + 16]
                n = min(int(t.numel()) for t in part)
                assert all(int(t.numel()) == n for t in part), "mark_seen(defer=True): views of different lengths in one step"
                if n > int(self._seen.numel()):
                    raise RuntimeError("mark_seen(defer=True): %d radii for a bucket of %d rows" % (n, int(self._seen.numel())))
                for t in part:
                    t.record_stream(stream)
                table = torch.tensor([t.data_ptr() for t in part], dtype=torch.int64)      # host array of addresses, read by the call
                check(L.lograst_add_visible_n(ptr(self._seen), ptr(table), len(part), n, stream_ptr(dev)))

    def reset_step(self, rows):
        """The per-step state back to where a step starts.  rows: the gradient rows are zero-filled as well -- False for a
        caller that knows them zero (the streamed exchange's packs cleared them): then only seen counts that somebody marked
        are zero-filled, and nothing else of the bucket's size is touched."""
        if rows:
            self.flat.zero_()
        self._seen_pending = []
        if rows or (self.track_seen and self._seen_dirty):
            self._seen.zero_()
        self._seen_reduced = False
        self._seen_dirty = False
        self.touched = None
        self._take_hint()

    def zero(self):
        self.reset_step(rows=True)

    def mark_seen(self, radii, index=None, defer=False):
        """Record which rows one view touched: radii > 0 (what the reference's step calls flag_vis,
        /root/reference/LoG/model/counter.py:48,50), for all rows or for the rows `index` a level-of-detail selection
        handed to the rasterizer.
        defer (device buckets, whole-model int32 radii): only remember the tensor; the views of the step are counted together,
        in one pass, when the counts are next read (`seen`: finish() of the streamed exchange, any reduce-scatter) -- 8 views
        of 30 M rows cost 1.1 GB of traffic instead of 2.9.  The tensor must stay alive and unchanged until then."""
        if not self.track_seen:
            raise RuntimeError("this bucket was built with track_seen=False")
        self._seen_dirty = True
        fast = index is None and radii.is_cuda and radii.dtype == torch.int32 and radii.is_contiguous() and self._seen.is_cuda
        if fast and int(radii.numel()) > int(self._seen.numel()):
            # (the kernels write seen[0 .. n): e.g. compact / LoD radii handed over without `index`)
            # RuntimeError: what the torch path below raises for the same mistake
            raise RuntimeError("mark_seen: %d radii for a bucket of %d rows (pass `index` for a selection's radii)"
                               % (int(radii.numel()), int(self._seen.numel())))
        if defer and fast:
            self._seen_pending.append(radii)
            return
        self._flush_seen()
        if fast:
            check, L, ptr, stream_ptr = _native()
            with torch.cuda.device(radii.device):
                check(L.lograst_add_visible(ptr(self._seen), ptr(radii), int(radii.numel()), stream_ptr(radii.device)))
            return
        vis = (radii > 0).to(torch.float32)
        if index is None:
            self.seen[:vis.numel()] += vis
        else:
            self.seen.index_add_(0, index, vis)

    def mark_touched(self, point_weight):
        """Hint for the row-sparse exchange of a bucket that holds ONE view's gradient rows (the streamed exchange, one
        group per view): that view's `point_weight` [n] -- zero exactly for the Gaussians that contributed to no pixel,
        whose gradient rows the backward left untouched.  The pack then reads 4 bytes per row instead of 64 for the rows
        the view did not touch (94 % of them at the 30 M headline).  A second call before the bucket is exchanged (several
        views in one group) withdraws the hint: the pack scans the rows themselves, as without it.  The tensor must stay
        alive and unchanged until the exchange of this bucket has run."""
        usable = self._hint_calls == 0 and point_weight is not None and point_weight.dim() == 1 \
            and point_weight.element_size() == 4 and point_weight.is_contiguous()
        self.touch_hint = point_weight if usable else None
        self._hint_calls += 1

    def _take_hint(self):
        h, self.touch_hint, self._hint_calls = self.touch_hint, None, 0
        return h

    def _sum_seen(self, group):
        if _active(self.world) and not self._seen_reduced and self.track_seen:
            dist.all_reduce(self.seen, op=dist.ReduceOp.SUM, group=group)
        self._seen_reduced = True

    def reduce(self, group=None):
        """Sum across ranks.  reduce-scatter + all-gather: every xGMI link carries 1/world of the buffer."""
        if not _active(self.world):
            return self.flat
        self._sum_seen(group)
        mine = torch.empty(self.flat.numel() // self.world, dtype=self.flat.dtype, device=self.flat.device)
        return _all_gather(self.flat, _reduce_scatter(mine, self.flat, group), group)

    def touched_blocks(self, group=None, kmax=None):
        """The step's TouchedBlocks: local `seen` per block, max-reduced over the ranks (world * nb int32: tiny).
        kmax: see TouchedBlocks (a bound instead of a read-back)."""
        assert self.block_rows > 0, "construct the bucket with block_rows > 0 for the touched-block exchange"
        assert self.track_seen, "the touched-block exchange reads the seen counts"
        nb = self.Pr // self.block_rows
        flags = (self.seen.view(self.world, nb, self.block_rows).amax(-1) > 0).to(torch.int32)
        if _active(self.world):
            dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=group)
        return TouchedBlocks(flags > 0, kmax=kmax)

    def touched_row_fraction(self):
        """Share of this rank's rows with a non-zero gradient (row-major buckets; a device scalar)."""
        return (self.blocks["rows"].view(self.Ppad, ROW_FLOATS) != 0).any(dim=1).float().mean()

    def _own_rows(self, seen=True):
        """What every exchange form delivers in a world without a process group: this rank's own rows of every column
        block and (seen) its own seen counts -- views of the bucket, nothing moves."""
        out = {name: self.rows(name, 0) for name, _ in self.layout}
        if seen and self.track_seen:
            out["seen"] = self.seen[:self.Pr]
        return out

    def _seen_shard(self, counts, group, into=None):
        """The seen counts' exchange: `counts` [P_pad] -> [Pr], this rank's rows of their sum over the ranks -- a dense
        reduce-scatter (4 bytes per row, dense by nature: every visible row counts); without a process group the local
        slice.  Added to the running sums `into`, or returned fresh."""
        active = _active(self.world)
        if active:
            mine = _reduce_scatter(torch.empty(self.Pr, dtype=torch.float32, device=counts.device), counts, group)
        else:
            mine = counts[:self.Pr]
        if into is not None:
            into += mine
            return into
        return mine if active else mine.clone()      # (fresh: never a view of a bucket's own counts, which a reset zeroes)

    def reduce_scatter_rows_sparse(self, rank, group=None, kmax=None, into=None, clear=False, seen_later=False):
        """Row-sparse form of ``reduce_scatter_rows`` (row-major buckets without SH columns): -> the same dict -- "rows"
        [Pr, 16] = the sum over ranks of this rank's rows, "seen" [Pr] -- but only the rows with a non-zero gradient
        travel: packed per owner as (16 sums | row index), padded to `kmax` rows per (sender, owner) pair, one all-to-all
        with equal splits; the owner adds what it receives into a zeroed shard.  The seen counts keep their dense
        reduce-scatter (``_seen_shard``).
        kmax=None: the longest list over all pairs of the whole job, exactly (``_row_bound``); kmax=K: a bound kept from an
        earlier step, no read-back; ``self.sparse_overflow`` (device flag, summed into
        ``StepExchange.compact_overflowed()``) says if some list was longer -- rows were dropped, repeat the step.
        Same addends as the dense form, summed in rank order -- ((r0 + r1) + r2) + ... -- instead of ring order: on the
        device lograst_unpack_rows adds the received segments one after the other with plain read-modify-writes (rows inside
        a segment are unique: no float atomics), on the CPU index_add_ walks them in the same order, so the reduced
        gradients are reproducible run to run on any number of ranks.
        into (the STREAMED exchange of ``StepExchange(parts > 1)``): a dict {"rows": [Pr, 16](, "seen": [Pr])} of running
        sums that this group's received rows (and seen counts) are ADDED to instead of a fresh zeroed shard -- the step's
        shard then holds, row by row, (((0 + g0) + g1) + ...) with every g = ((r0 + r1) + ...) added segment by segment.
        clear: the rows this call packs are zeroed in the bucket ("pack and clear"): the bucket is all zero again and needs
        no zero-fill before the next step (unless a bound was outgrown: then zero() and repeat the step).
        seen_later: the seen counts are NOT exchanged here (StepExchange's streamed form sends them once per step, from
        finish(): a dense 4-byte-per-row reduce-scatter per GROUP moves as many bytes as the packed rows themselves).
        A hint left by ``mark_touched`` is consumed by this call."""
        assert self.row_major and [n for n, _ in self.layout] == ["rows"], "row-sparse exchange: row-major bucket without SH columns"
        self.touched = None
        hint = self._take_hint()
        with_seen = self.track_seen and not seen_later
        if not _active(self.world):
            self.sparse_overflow, self.sparse_kmax = None, 0
            if into is None:
                return self._own_rows()
            own = self.rows("rows", 0)             # streamed: the group's rows join the running sums, the bucket is cleared
            into["rows"] += own
            if clear:
                own.zero_()
            if with_seen:
                self._seen_shard(self.seen, group, into["seen"])
            return into
        rows = self.blocks["rows"].view(self.world, self.Pr, ROW_FLOATS)
        kmax = _row_bound(rows, kmax, group)
        if hint is not None and hint.is_cuda:
            hint.record_stream(torch.cuda.current_stream(hint.device))      # (read here, possibly on a side stream)
        packed, self.sparse_overflow = _pack_segments(rows, kmax, clear=clear, hint=hint)
        self.sparse_kmax = kmax
        recv = torch.empty(packed.shape, dtype=packed.dtype, device=packed.device)
        _all_to_all(recv, packed, group)
        shard = into["rows"] if into is not None else torch.zeros(self.Pr, ROW_FLOATS, dtype=torch.float32, device=self.flat.device)
        out = {"rows": _unpack_segments(shard, recv, self.world, kmax)}
        if with_seen:
            out["seen"] = self._seen_shard(self.seen, group, None if into is None else into["seen"])
        return out

    def _columns(self):
        """(name, [P_pad * c] block, c) of everything that is exchanged: the attribute gradients and the seen counts."""
        return [(name, self.blocks[name], c) for name, c in self.layout] + ([("seen", self.seen, 1)] if self.track_seen else [])

    def reduce_scatter_rows(self, rank, group=None, compact=False, kmax=None):
        """Owner-computes exchange, first half: -> dict name -> [Pr, c] = the sum over ranks of this rank's rows of every
        attribute, plus "seen" -> [Pr] (how many views of all ranks saw each of them).  One reduce-scatter per column
        block, issued back to back.  compact: only the blocks some rank touched travel (TouchedBlocks; needs
        block_rows > 0), the rest of the returned rows are zeros -- which is what their sum is."""
        self.touched = None
        if not _active(self.world):
            return self._own_rows()
        dev, out = self.flat.device, {}
        tb = self.touched_blocks(group, kmax=kmax) if compact and self.block_rows > 0 and self.track_seen else None
        if tb is not None and tb.fraction >= self.DENSE_ABOVE:
            tb = None
        if tb is None:
            for name, blk, c in self._columns():
                mine = torch.empty(self.Pr * c, dtype=torch.float32, device=dev)
                _reduce_scatter(mine, blk, group)
                out[name] = mine.view(self.Pr, c) if name != "seen" else mine
            return out
        self.touched = tb
        B, nb, k = self.block_rows, tb.nb, tb.kmax
        owner = torch.arange(self.world, device=dev)[:, None]
        for name, blk, c in self._columns():
            packed = blk.view(self.world, nb, B * c)[owner, tb.order]            # [world, kmax, B c]: owner-major
            mine = torch.empty(k * B * c, dtype=torch.float32, device=dev)
            _reduce_scatter(mine, packed.reshape(-1), group)
            full = torch.zeros(nb, B * c, dtype=torch.float32, device=dev)
            full[tb.order[rank]] = mine.view(k, B * c)
            out[name] = full.view(self.Pr, c) if name != "seen" else full.view(self.Pr)
        return out


class FlatParams(_Flat):
    """The Gaussian attributes themselves in the bucket's layout (``views[name]`` are the tensors to render from), so
    that the owner-computes step can publish the rows it updated with one all-gather per attribute block."""

    def __init__(self, tensors, device, world=1, block_rows=0):
        k = int(tensors["shs"].shape[1]) if "shs" in tensors else 0
        super().__init__(next(iter(tensors.values())).shape[0], device, world, k, block_rows)
        for name, _ in self.layout:
            self.views[name].copy_(tensors[name].reshape(self.views[name].shape))

    def all_gather_rows(self, rank, group=None, touched=None):
        """Owner-computes exchange, second half: every rank publishes its (updated) rows of every attribute; with
        `touched` (the TouchedBlocks of the gradient exchange) only the blocks that can have moved."""
        if not _active(self.world):
            return
        dev = self.flat.device
        for name, c in self.layout:
            if touched is None:
                _all_gather(self.blocks[name], self.rows(name, rank).reshape(-1).clone(), group)
                continue
            B, nb, k = self.block_rows, touched.nb, touched.kmax
            blocks = self.blocks[name].view(self.world, nb, B * c)
            recv = torch.empty(self.world * k * B * c, dtype=torch.float32, device=dev)
            _all_gather(recv, blocks[rank][touched.order[rank]].reshape(-1), group)
            blocks[torch.arange(self.world, device=dev)[:, None], touched.order] = recv.view(self.world, k, B * c)


class OwnerAdam:
    """Sparse Adam on the rows this rank owns (/root/reference/LoG/model/sparse_optimizer.py:41-78,163-196): same update,
    same ``flag_vis`` rule (only rows seen this step move, and only their moments), eps 1e-15, optional amsgrad; moments
    allocated for Pr = ceil(P / world) rows only.  ``lr``: dict name -> learning rate of this step (the caller runs the
    reference's schedules: xyz / scaling follow ``get_expon_lr_func``, sparse_optimizer.py:6-39,171-177)."""
    BETA1, BETA2, EPS = 0.9, 0.999, 1e-15

    def __init__(self, params, rank, amsgrad=False):
        self.rank, self.steps = int(rank), 0
        z = lambda name, c: torch.zeros(params.Pr, c, dtype=torch.float32, device=params.flat.device)
        self.exp_avg = {name: z(name, c) for name, c in params.layout}
        self.exp_avg_sq = {name: z(name, c) for name, c in params.layout}
        self.max_exp_avg_sq = {name: z(name, c) for name, c in params.layout} if amsgrad else None
        self._index = torch.arange(params.Pr, dtype=torch.int64, device=params.flat.device)

    def step(self, bucket, params, lr, group=None, compact=False):
        """One optimizer step from the gradients accumulated in `bucket` (all views of all ranks): reduce-scatter,
        Adam on the owned rows that some view saw, all-gather of the attributes.  Returns the number of rows of this
        rank that moved (a device tensor; no synchronisation).  compact: touched-block form of both exchanges."""
        grads = bucket.reduce_scatter_rows(self.rank, group, compact=compact)
        return self.step_rows(grads, params, lr, group, touched=bucket.touched)

    def step_rows(self, grads, params, lr, group=None, touched=None):
        """The same step from already reduce-scattered rows (``GradientBucket.reduce_scatter_rows`` /
        ``StepExchange.finish``): dict name -> [Pr, c] and "seen" -> [Pr]."""
        from . import rasterizer as _r
        grads = split_rows(grads)     # (a row-major bucket's "rows" -> per-attribute views)
        if "seen" not in grads:
            raise ValueError("the owner-computes step needs the seen counts (GradientBucket(track_seen=True) + mark_seen)")
        self.steps += 1
        flag = grads["seen"] > 0
        bc1, bc2 = 1 - self.BETA1 ** self.steps, 1 - self.BETA2 ** self.steps
        entries = []
        for name, _ in params.layout:
            if name not in lr:
                continue
            rows = params.rows(name, self.rank)            # updated in place: "model" rows and gathered parameter are the same memory
            entries.append((rows, rows, grads[name], self.exp_avg[name], self.exp_avg_sq[name],
                            self.max_exp_avg_sq[name] if self.max_exp_avg_sq is not None else None, lr[name] / bc1))
        if entries:
            with torch.no_grad():
                _r._backend.sparse_adam(self._index, flag, entries, self.BETA1, self.BETA2, math.sqrt(bc2), self.EPS)
        params.all_gather_rows(self.rank, group, touched=touched)
        return flag.sum()


class StepExchange:
    """The gradient exchange of one training step in `parts` pieces, so that most of it runs under the rendering.

    The step's views are split into `parts` consecutive groups (``bucket_of``), each accumulating into its own
    GradientBucket.  ``launch(g)`` -- called once group g's last backward has been enqueued -- issues g's reduce-scatter:
    on a HIP device it goes to a side stream that waits for the compute stream's work so far, so RCCL moves group g while
    group g + 1 renders; ``finish()`` joins the side stream and sums the groups' shards (P / world rows each).  What stays
    exposed is the last group's reduce-scatter (1 / parts of the bytes) and whatever the caller does with the shard
    (``OwnerAdam.step_rows`` + its all-gather, or ``all_gather_grads`` for replicated optimizers).  Costs parts x the
    bucket memory (30 M Gaussians x 14 columns: 1.7 GB each out of 288).  The sum is the same set of addends as one
    bucket's, grouped by part.

    The STREAMED row-sparse exchange (``launch(g, sparse=True)`` with parts > 1): a dense group exchange is as large as the
    whole step's, so grouping does not pay for views that touch rows all over the model -- but ONE view's gradients live in
    6 % of the rows against the 24 % of a rank's eight views (tools/touched_rows.py).  Per group: the touched rows are packed
    per owner and CLEARED in the bucket (pack and clear: no bucket is ever zero-filled again), one all-to-all moves them
    under the next group's rendering, and the owner adds them straight into the step's ONE running shard -- no per-group
    dense shards, no sum in finish().  Exposed: the last group's all-to-all (1 / parts of the rows a rank touches, counting
    rows several groups touch once per group) and the closing all-gather.  The sum of a row is (((0 + g0) + g1) + ...),
    each g = ((r0 + r1) + ...): fixed by construction, reproducible on any number of ranks."""

    def __init__(self, num_points, device, world=1, rank=0, sh_coeffs=0, parts=1, block_rows=0, group=None,
                 track_seen=True, timing=False, row_major=False):
        """timing: a pair of device events brackets every collective and the join in finish(), so that a run reports how
        much of the exchange ran under the rendering and how much was exposed (``timing_summary``)."""
        self.world, self.rank, self.parts, self.group = max(int(world), 1), int(rank), max(int(parts), 1), group
        self._timing = bool(timing)
        self._ev = {"reduce_scatter": [], "join": [], "all_gather": []}
        self.buckets = [GradientBucket(num_points, device, world, sh_coeffs, block_rows, track_seen, row_major)
                        for _ in range(self.parts)]
        self.device = self.buckets[0].flat.device
        self.side = torch.cuda.Stream(device=self.device) if (self.device.type == "cuda" and (self.world > 1 or _single_rank_forced())) else None
        self._shards = [None] * self.parts
        self.touched = None
        # device flag: a bounded touched-block / row-sparse exchange dropped rows (compact_overflowed).  ONE persistent
        # tensor, OR-ed in place on the stream that produced the addend (a fresh `a | b` issued on the compute stream would
        # read a side-stream temporary without waiting for it, after its block has gone back to the pool)
        self._overflow = torch.zeros((), dtype=torch.bool, device=self.device)
        self._overflow_used = False
        self.gather_kmax = 0           # rows per owner of the last row-sparse all_gather_grads
        self._gathered_prev = None     # (result tensor, received segments, rows per owner) of the last all_gather_grads(into=...)
        self._stream_shard = None      # the streamed sparse exchange's running sums of this step (launch(sparse=True), parts > 1)
        self.streamed = False          # the last step's sparse launches were streamed: buckets cleared by their own packs

    def bucket_of(self, view, n_views):
        """The bucket view `view` of the rank's `n_views` accumulates into (consecutive views share a group)."""
        return self.buckets[min(int(view) * self.parts // max(int(n_views), 1), self.parts - 1)]

    def seen_bucket(self, part, streamed):
        """The bucket whose ``mark_seen`` a caller should use for group `part`: the group's own -- or, when the step's sparse
        exchange is streamed (launch(sparse=True), parts > 1), bucket 0 for every group: the counts then sit in ONE array
        and finish() exchanges them once."""
        return self.buckets[0 if (streamed and self.parts > 1) else part]

    def last_view_of(self, part, n_views):
        return max(v for v in range(n_views) if self.bucket_of(v, n_views) is self.buckets[part])

    def _reset_step(self, rows):
        for b in self.buckets:
            b.reset_step(rows)
        self._shards = [None] * self.parts
        self.touched = None
        self._stream_shard = None

    def zero(self):
        self._reset_step(rows=True)

    def begin_step(self):
        """Between steps of the STREAMED sparse exchange: the buckets' rows were cleared by their own packs, so only the
        small per-step state is reset (the seen counts somebody marked, the shard list) -- instead of zero()'s full
        zero-fill of every bucket."""
        self._reset_step(rows=False)

    @contextlib.contextmanager
    def _timed(self, kind, stream):
        """A pair of timing events on `stream` bracketing the block (nothing unless timing on a HIP device)."""
        if not (self._timing and self.device.type == "cuda"):
            yield
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        try:
            yield
        finally:
            b.record(stream)
            self._ev[kind].append((a, b))

    def reset_timing(self):
        for v in self._ev.values():
            v.clear()

    def timing_summary(self, steps):
        """ms per step (synchronises): `reduce_scatter` = the collectives' own duration on the side stream (mostly hidden
        under the next group's rendering), `exposed_join` = how long the compute stream stood still in finish() waiting
        for the last of them, `all_gather` = the closing all-gather on the compute stream (exposed)."""
        if not self._timing or self.device.type != "cuda":
            return None
        torch.cuda.synchronize(self.device)
        tot = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self._ev.items()}
        n = max(int(steps), 1)
        return {"reduce_scatter_ms_per_step": tot["reduce_scatter"] / n, "exposed_join_ms_per_step": tot["join"] / n,
                "all_gather_ms_per_step": tot["all_gather"] / n, "collectives_timed": len(self._ev["reduce_scatter"])}

    def launch(self, part, compact=False, kmax=None, sparse=False):
        """kmax (compact / sparse): size the collectives from this bound instead of a read-back (TouchedBlocks /
        ``GradientBucket.reduce_scatter_rows_sparse``); check ``compact_overflowed()`` where the step synchronises anyway.
        sparse: the row-sparse form (only rows with a non-zero gradient travel)."""
        b = self.buckets[part]
        self.streamed = bool(sparse) and self.parts > 1
        form = self._streamed_form if self.streamed else self._sparse_form if sparse else self._dense_form
        with self._on_side_stream("reduce_scatter"):
            self._shards[part], over = form(b, compact, kmax)
            self._note_overflow(over)       # on the stream that wrote `over`: in order behind its producer

    # the exchange forms of launch(): -> (this rank's shard of bucket `b`, the device flag of an outgrown bound or None)
    def _dense_form(self, b, compact, kmax):
        shard = b.reduce_scatter_rows(self.rank, self.group, compact=compact, kmax=kmax)
        return shard, None if b.touched is None else b.touched.overflow

    def _sparse_form(self, b, compact, kmax):
        return b.reduce_scatter_rows_sparse(self.rank, self.group, kmax=kmax), b.sparse_overflow

    def _streamed_form(self, b, compact, kmax):
        if self._stream_shard is None:             # first group of the step: the running sums start at zero
            self._stream_shard = {"rows": torch.zeros(b.Pr, ROW_FLOATS, dtype=torch.float32, device=self.device)}
            if b.track_seen:
                self._stream_shard["seen"] = torch.zeros(b.Pr, dtype=torch.float32, device=self.device)
        b.reduce_scatter_rows_sparse(self.rank, self.group, kmax=kmax, into=self._stream_shard, clear=True, seen_later=True)
        return self._stream_shard, b.sparse_overflow

    @contextlib.contextmanager
    def _on_side_stream(self, kind):
        """The block is issued on the side stream, behind the compute stream's work so far, between timing events of
        `kind` (no side stream: where it stands)."""
        if self.side is None:
            yield
            return
        self.side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.side), self._timed(kind, self.side):
            yield

    def _note_overflow(self, over):
        """OR a device flag into the step's persistent overflow flag, on the CURRENT stream (the caller issues this on the
        stream that produced `over`; launch() / finish() / compact_overflowed() order the streams among themselves)."""
        if over is not None:
            self._overflow.logical_or_(over.reshape(()).to(torch.bool))
            self._overflow_used = True

    def compact_overflowed(self, reset=True):
        """Did a bounded touched-block exchange since the last call drop blocks (some owner's touched list was longer than
        the bound)?  One device -> host read: call it where the step synchronises anyway."""
        if not self._overflow_used:
            return False
        if self.side is not None:         # the flag may have been written on the side stream last
            torch.cuda.current_stream(self.device).wait_stream(self.side)
        over = bool(self._overflow.item())
        if reset:
            self._overflow.zero_()
            self._overflow_used = False
        return over

    def finish(self):
        """-> dict name -> [Pr, c] (+ "seen" -> [Pr]): this rank's rows of the sum over all groups and ranks."""
        for g in range(self.parts):
            if self._shards[g] is None:
                self.launch(g)
        if self.side is not None:
            main = torch.cuda.current_stream(self.device)
            with self._timed("join", main):
                main.wait_stream(self.side)
            for sh in self._shards:
                for t in sh.values():
                    t.record_stream(main)
        if self._stream_shard is not None and all(sh is self._stream_shard for sh in self._shards):
            # streamed sparse exchange: the groups' rows were added as they arrived; the step's seen counts travel ONCE, now
            # (the sum over the buckets somebody marked: callers that mark one bucket for the whole step -- seen_bucket() --
            # pay one reduce-scatter of 4 bytes per row per step instead of one per group)
            dirty = [b.seen for b in self.buckets if b._seen_dirty]
            if dirty:
                acc = dirty[0] if len(dirty) == 1 else torch.stack(dirty).sum(0)
                self._stream_shard["seen"] = self.buckets[0]._seen_shard(acc, self.group)
            return dict(self._stream_shard)
        total = dict(self._shards[0])
        if self.parts > 1:
            total = {k: v.clone() for k, v in total.items()} if not _active(self.world) else total
            for sh in self._shards[1:]:
                for k in total:
                    total[k] += sh[k]
        tbs = [b.touched for b in self.buckets]
        self.touched = None
        if all(t is not None for t in tbs):
            self.touched = tbs[0]
            for t in tbs[1:]:
                self.touched = self.touched.union(t)
            if self.parts > 1:               # (parts == 1: launch() noted it already)
                self._note_overflow(self.touched.overflow)
        return total

    def all_gather_grads(self, total, sparse_kmax=None, into=None):
        """Replicated-optimizer form: every rank receives every row of the summed gradients, in buckets[0].
        sparse_kmax (row-major buckets): only the non-zero rows of every owner's shard travel, packed like the row-sparse
        reduce-scatter and padded to `sparse_kmax` rows per owner (0 / "exact": the longest list, one max-reduce + one
        read-back); the bucket is zeroed and the gathered rows added into it.  Overflow: ``compact_overflowed()``.
        into (row-sparse form): a persistent [world * Pr, 16] result tensor of the caller's instead of buckets[0] -- zero on
        the first call; from then on only the rows the PREVIOUS call's segments wrote are cleared before the new ones are
        stored (a third of the writes of a zero-fill at 29 % non-zero rows), and buckets[0] stays all zero for the streamed
        exchange's next step."""
        b0 = self.buckets[0]
        if not _active(self.world):
            for name, own in b0._own_rows(seen=False).items():
                own.copy_(total[name])
            return b0.flat
        main = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        if sparse_kmax is not None and "rows" in total:
            # (only the "rows" block travels here: SH columns would silently stay un-gathered)
            assert [n for n, _ in b0.layout] == ["rows"], "row-sparse all-gather: row-major bucket without SH columns"
            with self._timed("all_gather", main):
                shard = total["rows"].reshape(1, b0.Pr, ROW_FLOATS)
                k = _row_bound(shard, None if not sparse_kmax or sparse_kmax == "exact" else sparse_kmax, self.group)
                packed, over = _pack_segments(shard.contiguous(), k)
                recv = torch.empty(self.world * packed.numel(), dtype=torch.float32, device=self.device)
                _all_gather(recv, packed, self.group)
                self._note_overflow(over)      # (the compute stream, which has joined the side stream in finish())
                self.gather_kmax = k
                if into is None:
                    full = b0.blocks["rows"]
                    full.zero_()
                else:
                    full = into.view(-1)
                    assert full.numel() == self.world * b0.Pr * ROW_FLOATS and full.is_contiguous()
                    prev = self._gathered_prev
                    if prev is not None and prev[0] is into:
                        _unpack_segments(full.view(self.world * b0.Pr, ROW_FLOATS), prev[1], self.world, prev[2],
                                         per_segment_rows=b0.Pr, zero=True)
                    else:
                        full.zero_()
                    self._gathered_prev = (into, recv, k)
                _unpack_segments(full.view(self.world * b0.Pr, ROW_FLOATS), recv, self.world, k, per_segment_rows=b0.Pr)
            return b0.flat if into is None else into
        with self._timed("all_gather", main):
            for name, c in b0.layout:
                _all_gather(b0.blocks[name], total[name].reshape(-1), self.group)
        return b0.flat


# ---- second axis: the image split into bands of tile rows, one band per rank ----------------------
# Every rank keeps all Gaussians and renders only its rows (log_amd.rasterizer.tile_rows clips every rect to the band
# in the projection kernel, so a rank bins, sorts and composites only what reaches its rows); no compositing across
# ranks is needed.  Exchange per view: an all-gather of the bands (3 * H * W * 4 bytes in total) and the same gradient
# sum as above.
def band_rows(rank, world, height):
    """Tile rows [begin, end) owned by `rank`: contiguous, sizes differing by at most one row of tiles."""
    from .rasterizer import TILE
    gy = (int(height) + TILE - 1) // TILE
    return rank * gy // world, (rank + 1) * gy // world


def band_pixels(rank, world, height):
    from .rasterizer import TILE
    b, e = band_rows(rank, world, height)
    return b * TILE, min(e * TILE, int(height))


def band_index(y0, y1, rank, world, height):
    """Indices (ascending, int64) of the Gaussians whose rect reaches `rank`'s band of tile rows, from the per-Gaussian
    row ranges of ``GaussianRasterizer.tile_rows`` (one 44-byte-per-Gaussian pass, the same on every rank): the rank then
    gathers, projects, composites and differentiates only those -- SURVEY 8e "every GPU preprocesses only Gaussians whose
    rect intersects its band".  Rendering the subset inside ``rasterizer.tile_rows(*band_rows(rank, world, H))`` gives the
    band bit for bit as rendering all Gaussians does (same Gaussians, same relative order)."""
    b, e = band_rows(rank, world, height)
    return torch.nonzero((y0 < e) & (y1 > b)).reshape(-1)


def gather_bands(image, rank, world, group=None):
    """image: [C, H, W] with this rank's band rendered (other rows: anything).  Returns the full image on every rank.
    Bands are padded to a common height for the collective (all_gather needs equal shapes)."""
    C, H, W = image.shape
    if not _active(world):
        return image
    rows = [band_pixels(r, world, H) for r in range(world)]
    hmax = max(e - b for b, e in rows)
    b, e = rows[rank]
    mine = torch.zeros(C, hmax, W, dtype=image.dtype, device=image.device)
    mine[:, :e - b] = image[:, b:e]
    parts = [torch.empty(mine.shape, dtype=mine.dtype, device=mine.device) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    out = torch.empty(image.shape, dtype=image.dtype, device=image.device)
    for (rb, re), part in zip(rows, parts):
        out[:, rb:re] = part[:, :re - rb]
    return out

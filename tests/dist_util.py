"""StepExchange steps against plain sums, shared by tests/test_dist_cpu.py and tests/test_gpu_dist.py."""
import numpy as np
import torch


def one_rank_streamed_steps(device, parts, streamed, defer=False, views=8, P=1003):
    """Two steps of a one-rank StepExchange (no process group: the world is inactive) in the order a training step runs
    them -- a group's views accumulate and are marked, its exchange is launched, then the next group -- against plain
    sums: -> per step (seen counts [P_pad], rows [P_pad, 16], the integer sum of radii > 0 over the views [P] from numpy,
    the dense sum of the accumulated rows).
    On a device the radii are int32 device tensors, so mark_seen takes its kernels (defer: the counted-together form)."""
    from log_amd.dist import StepExchange
    ex = StepExchange(P, device, world=1, parts=parts, row_major=True, track_seen=True)
    assert not ex.buckets[0].world > 1 and ex.buckets[0].Pr >= P and P % 4
    rng = np.random.default_rng(7 + parts)
    out = []
    for step in range(2):
        if step:
            # (one group: the exchange is not streamed, nothing cleared the bucket's rows -- the full reset, as a step does)
            ex.begin_step() if parts > 1 else ex.zero()
        radii = [np.where(rng.random(P) < 0.3, rng.integers(1, 40, P), -rng.integers(0, 2, P)).astype(np.int32) for _ in range(views)]
        want_seen = sum((r > 0).astype(np.int64) for r in radii)
        want_rows = torch.zeros(ex.buckets[0].Pr, 16)
        keep = []                                                                # (deferred radii stay alive until they are counted)
        for v in range(views):
            b = ex.bucket_of(v, views)
            part = ex.buckets.index(b)
            touched = torch.from_numpy(rng.permutation(P)[:60])
            vals = torch.from_numpy(rng.integers(-8, 9, (60, 14))).float()       # integer-valued: sums exact in any order
            b.views["rows"][touched.to(device), :14] += vals.to(device)
            want_rows[touched, :14] += vals
            r = torch.from_numpy(radii[v]).to(device)
            keep.append(r)
            ex.seen_bucket(part, streamed).mark_seen(r, **({"defer": True} if defer else {}))
            if v == ex.last_view_of(part, views):
                ex.launch(part, sparse=True)
        total = ex.finish()
        out.append((total["seen"].cpu().clone(), total["rows"].cpu().clone(), want_seen, want_rows))
    return out


# ---- the streamed row-sparse exchange, one group per view, against one group for all views ----------------------------
# (mode, parts, launch() arguments, all_gather_grads() arguments)
STREAMED_MODES = (("one_group", 1, dict(sparse=True), dict(sparse_kmax="exact")),
                  ("stream8", 8, dict(sparse=True), dict(sparse_kmax="exact")),
                  ("stream8_bound", 8, dict(sparse=True, kmax=64), dict(sparse_kmax=500)),
                  # each view's bucket packed from a HINT (the view's point_weight stand-in: non-zero exactly at the rows it
                  # touched) and the seen counts marked in ONE bucket for the step
                  ("stream8_hint", 8, dict(sparse=True), dict(sparse_kmax="exact")))
STREAMED_TOO_SMALL = ("stream8_small", 8, dict(sparse=True, kmax=4), dict(sparse_kmax=500))   # 60 rows per view: outgrown


def streamed_views(rank, P=1003, views=8):
    """Rank `rank`'s synthetic views: per view (60 touched rows -- 6 % of them, overlapping between views --, their
    integer-valued gradients [60, 14] in [-8, 8]: sums exact in any order, a seen mask at 30 % as int32 radii)."""
    out = []
    for v in range(views):
        gen = torch.Generator().manual_seed(5000 + 100 * rank + v)
        touched = torch.randperm(P, generator=gen)[:60]
        out.append((touched, torch.randint(-8, 9, (60, 14), generator=gen).float(),
                    (torch.rand(P, generator=gen) < 0.3).to(torch.int32)))
    return out


def streamed_steps(mode, parts, kw_rs, kw_ag, per_view, device, world, rank, steps=2, P=1003):
    """`steps` steps of one StepExchange over `per_view` (step s accumulates (s + 1) x the views' gradients); the second
    starts from begin_step(), no zero().  With parts > 1 the gathered sum goes into a persistent NaN-filled result (the
    first gather zero-fills it, the later ones clear what the one before wrote).  -> {"<mode>_step<s>": what the step left}."""
    from log_amd.dist import StepExchange
    ex = StepExchange(P, device, world, rank, parts=parts, row_major=True)
    result = torch.full((world * ex.buckets[0].Pr, 16), float("nan"), device=device) if parts > 1 else None
    res = {}
    for step in range(steps):
        if step:
            ex.begin_step()
        keep = []                                                                # (hints and deferred radii stay alive until used)
        for v, (touched, vals, seen) in enumerate(per_view):
            b = ex.bucket_of(v, len(per_view))
            part = ex.buckets.index(b)
            touched, seen = touched.to(device), seen.to(device)
            b.views["rows"][touched, :14] += (vals * (step + 1)).to(device)
            if mode == "stream8_hint":
                hint = torch.zeros(P, device=device)
                hint[touched] = 0.25
                b.mark_touched(hint)
                ex.seen_bucket(part, True).mark_seen(seen, defer=True)           # (counted at once where nothing can defer: CPU)
                keep += [hint, seen]
            else:
                b.mark_seen(seen)
            if v == ex.last_view_of(part, len(per_view)):
                ex.launch(part, **kw_rs)
        total = ex.finish()
        left = [float(b.blocks["rows"].abs().sum()) for b in ex.buckets]
        ex.all_gather_grads(total, into=result, **kw_ag)                         # (streamed: a persistent result, bucket 0 stays clean)
        full = ex.buckets[0].blocks["rows"] if result is None else result.reshape(-1)
        after = [float(b.blocks["rows"].abs().sum()) for b in ex.buckets]
        res["%s_step%d" % (mode, step)] = dict(rows=total["rows"].cpu().clone(), seen=total["seen"].cpu().clone(),
                                               full=full.cpu().clone(), left=left, after=after,
                                               over=ex.compact_overflowed(), streamed=ex.streamed)
        if parts == 1:
            ex.zero()                                                            # (the one-group form keeps its sums: zero-filled as before)
    return res


def streamed_plain_sums(world, step, P=1003):
    """What every rank must hold after step `step` of streamed_steps, from plain torch sums on the CPU: -> (the summed
    rows [world * Pr, 16], the summed seen counts [world * Pr]); rank r's shard is rows [r * Pr, (r + 1) * Pr)."""
    from log_amd.dist import rows_per_rank
    Ppad = world * rows_per_rank(P, world)
    rows, seen = torch.zeros(Ppad, 16), torch.zeros(Ppad)
    for rank in range(world):
        for touched, vals, s in streamed_views(rank, P):
            rows[touched, :14] += vals * (step + 1)
            seen[:P] += (s > 0).float()
    return rows, seen

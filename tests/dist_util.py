"""One-rank StepExchange steps against plain sums, shared by tests/test_dist_cpu.py and tests/test_gpu_dist.py."""
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

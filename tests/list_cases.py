"""Tile lists of EXACT length with EXACT depth ties, and a statement of which sort path each one takes.

A tile's list passes through log_amd/csrc/sort.hip (LDS-resident bucket sort up to 4096 keys, streamed beyond, the
network where no bucket map spreads the depths), the lazy first-window protocol and the compositing walk with its 64-entry
chunks and hit masks (log_amd/csrc/blend.hip).  Every one of those has a boundary at some list length; random scenes land
inside the regimes.  The scenes here put one list ON a chosen length:

  camera: R = I, T = 0, focal 60 on a 48x32 image = 3x2 tiles.  The view depth of a Gaussian is then its z coordinate bit
  for bit, so equal z gives equal sort keys up to the id.
  Gaussians: isotropic, about 0.7 px wide, centres on pixels 4.5 ... 11.5 of their tile on both axes -- at least 4 px from
  the tile's edges, so each lands in ONE tile's list and nowhere else.

Nothing here imports the GPU side: tests/test_list_cases_cpu.py checks every case through the oracle (lengths, ties, order,
open pixel, declared regime), tests/test_gpu_list_boundaries.py runs them on the device.
"""
import numpy as np

from log_amd import scenes

W, H, FOCAL = 48, 32, 60.0
GX, GY = 3, 2
MAIN_TILE = 4                                 # (row 1, column 1): pixels 16..31 on both axes
SIGMA_PX = 0.7
BUCKET_MAX = 32                               # LR_BUCKET_MAX
LONG_LIST = 4096                              # LR_LONG_LIST: longer lists are streamed
LONG_WIN = 7680                               # LR_LONG_WIN: list positions of one window of a streamed list
N_FRONT = 3


def camera():
    K = np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1.0]])
    return scenes.make_camera(np.eye(3), np.zeros(3), K, W=W, H=H)


def open_opacity(L):
    """An opacity at which a pixel under L such splats (spread over the tile's inner 8x8 pixels) never stops, and every
    splat still passes the 1/255 alpha floor at its own centre."""
    return float(np.clip(40.0 / max(L, 1), 0.008, 0.5))


# ---- depth patterns: float32 z of the L keys, in id order ------------------------------------------------------------

def _two_sided(n, rng):
    """n distinct depths, evenly spaced over [2.0, 2.4] and [2.6, 3.0] with both ends of the range taken, shuffled."""
    if n <= 0:
        return np.zeros(0, np.float64)
    if n == 1:
        return np.array([2.0])
    lo = (n + 1) // 2
    z = np.concatenate([np.linspace(2.0, 2.4, lo), np.linspace(3.0, 2.6, n - lo)])
    return rng.permutation(z)


def depths(L, pattern, rng):
    """-> float32[L].
    spread   2 + 1e-4 * permutation: all distinct.
    offc     the depths of `spread`; the scene differs (one_tile: every centre (+0.3, -0.2) px off a pixel).
    flat     one depth: the order is the id order.
    tie<k>   one isolated group of exactly k equal depths (2.5) in the gap of an evenly spread rest: the group has a bucket of
             any linear map to itself.  32 / 33: a bucket holds LR_BUCKET_MAX keys and not one more.  8 / 9 (streamed lists,
             whose buckets lr_emit_bucket orders): eight keys are sorted in registers, nine are ranked by the whole wave.
    cells    L <= 4096: two clusters, each one cell (1/64 of the depth range) wide, the range's ends pinned at 2.0 and 3.0
             by one key each.  The linear map has 1/64 of its buckets for half the list; the equalised one spreads it.
             L > 4096: the streamed sort takes its range and its cell histogram from a SAMPLE, so the range's ends are
             pinned by 96 keys each over 0.3 cells (inside the first / last cell of the 1 % widened map), and the two
             clusters begin a quarter of a cell behind a cell's edge: no cell holds a sliver of a group -- a few dozen keys
             for which the sample earns the cell a handful of buckets, all in one of them -- whatever the sample.
    strays   99.5 % in [2, 2.001], the rest uniform in [1, 4] (a surface seen head-on plus strays)."""
    if pattern in ("spread", "offc"):
        z = 2.0 + 1e-4 * rng.permutation(L)
    elif pattern == "flat":
        z = np.full(L, 2.5)
    elif pattern.startswith("tie"):
        k = int(pattern[3:])
        assert L >= k
        z = np.concatenate([np.full(k, 2.5), _two_sided(L - k, rng)])
        z = z[rng.permutation(L)]
    elif pattern == "cells" and L <= LONG_LIST:
        n = L - 2
        a = n // 2
        cell = 1.0 / 64
        z = np.concatenate([[2.0, 3.0], 2.0 + cell * (10 + np.linspace(0.02, 0.98, a)),
                            2.0 + cell * (40 + np.linspace(0.02, 0.98, n - a))])
        z = z[rng.permutation(L)]
    elif pattern == "cells":
        # cell coordinate of depth d in the streamed map: (d - 2 + 0.01) * 64 / 1.02 for a sampled range of [2, 3]
        cell = 1.02 / 64
        at = lambda c: 2.0 - 0.01 + cell * c
        n = L - 192
        a = n // 2
        z = np.concatenate([np.linspace(2.0, 2.0 + 0.3 * cell, 96), np.linspace(3.0 - 0.3 * cell, 3.0, 96),
                            at(10.25 + np.linspace(0.0, 1.0, a)), at(40.25 + np.linspace(0.0, 1.0, n - a))])
        z = z[rng.permutation(L)]
    elif pattern == "strays":
        n_stray = max(1, L // 200)
        z = np.concatenate([rng.uniform(1.0, 4.0, n_stray), rng.uniform(2.0, 2.001, L - n_stray)])
        z = z[rng.permutation(L)]
    else:
        raise KeyError(pattern)
    return z.astype(np.float32)


# ---- scenes ------------------------------------------------------------------------------------------------------------

def _splats(u, v, z32, sigma_px, opacity, rng):
    """Isotropic Gaussians whose centres project to pixel (u, v) at view depth z32 (float32, kept bit for bit)."""
    n = len(z32)
    z = z32.astype(np.float64)
    xyz = np.stack([(np.asarray(u, np.float64) + 0.5 - W / 2.0) * z / FOCAL,
                    (np.asarray(v, np.float64) + 0.5 - H / 2.0) * z / FOCAL, z], 1).astype(np.float32)
    xyz[:, 2] = z32
    s = np.repeat((np.asarray(sigma_px, np.float64) * z / FOCAL).reshape(n, 1), 3, axis=1)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(xyz=xyz, scaling=s.astype(np.float32), rotation=q.astype(np.float32),
                opacity=np.full((n, 1), opacity, np.float32), colors=rng.random((n, 3), dtype=np.float32))


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


OFF_CENTRE = (0.3, -0.2)                      # `offc`: where every centre lies relative to its pixel ...
OFF_JITTER = 0.05                             # ... give or take this much: no two splats have the same alpha at a pixel


def _tile_list(tile, z32, opacity, rng, off_centre=None):
    """len(z32) splats inside `tile`; the one that sorts LAST (largest depth, then largest id) sits exactly on the tile's
    pixel (8, 8), so that pixel's walk reaches the end of the list if it never stops.
    off_centre=(ox, oy): every centre, the last one's included, lies (ox, oy) px off one of the pixels 5 ... 11, give or take
    OFF_JITTER: no pixel has dx = 0 or dy = 0 to any splat, so no addend of dL/dmean or dL/dconic is zero by construction.
    (The jitter: with hundreds of splats on EXACTLY one centre a pixel sees the same alpha hundreds of times over, and a
    transmittance rebuilt by reciprocal-and-multiply then repeats one rounding error of 1 / (1 - alpha) at every step, in one
    direction -- a scene made of copies, profiles/walk_rows_tests.md.)"""
    n = len(z32)
    x0, y0 = 16 * (tile % GX), 16 * (tile // GX)
    if off_centre is None:
        u, v = x0 + rng.uniform(4.5, 11.5, n), y0 + rng.uniform(4.5, 11.5, n)
    else:
        u = x0 + rng.integers(5, 12, n).astype(np.float64) + off_centre[0] + rng.uniform(-OFF_JITTER, OFF_JITTER, n)
        v = y0 + rng.integers(5, 12, n).astype(np.float64) + off_centre[1] + rng.uniform(-OFF_JITTER, OFF_JITTER, n)
    if n:
        last = np.lexsort((np.arange(n), z32.view(np.uint32)))[-1]
        u[last], v[last] = x0 + 8.0, y0 + 8.0
        if off_centre is not None:
            u[last] += off_centre[0]
            v[last] += off_centre[1]
    return _splats(u, v, z32, SIGMA_PX, opacity, rng)


def one_tile(L, pattern, opacity=None, front=None, beg=37, seed=0):
    """-> (cam, sc, lens): ONE list of exactly L keys with depth pattern `pattern` in tile 4, starting at list offset `beg`
    (37: not 64-aligned) behind a short list in tile 0; lens = the six list lengths this scene is built to have.
    front="closed": N_FRONT opaque splats nearest the camera cover the whole image, so every pixel of tile 4 stops after
    them.  They are entries of every tile's list: L counts them (L - N_FRONT keys follow `pattern`), and the lists of tiles
    0 ... 3 still add up to beg."""
    rng = np.random.default_rng([seed, L, beg])
    opacity = open_opacity(L) if opacity is None else opacity
    cam = camera()
    nf = N_FRONT if front == "closed" else 0
    assert front in (None, "closed") and L >= nf and beg >= 4 * nf
    n0 = beg - 4 * nf
    parts = [_tile_list(0, depths(n0, "spread", rng), open_opacity(n0 + nf), rng),
             _tile_list(MAIN_TILE, depths(L - nf, pattern, rng), opacity, rng, OFF_CENTRE if pattern == "offc" else None)]
    lens = [n0 + nf, nf, nf, nf, L, nf]
    if nf:
        parts.append(_splats(np.full(nf, 24.0), np.full(nf, 24.0), np.array([0.5, 0.51, 0.52], np.float32)[:nf], 60.0, 0.999, rng))
    return cam, _cat(parts), lens


def adjacent_tiles(lengths, seed=0):
    """-> (cam, sc, lens): all six tiles, tile t with a `spread` list of exactly lengths[t] keys whose last entry is walked."""
    assert len(lengths) == GX * GY
    rng = np.random.default_rng([seed] + [int(n) for n in lengths])
    parts = [_tile_list(t, depths(int(n), "spread", rng), open_opacity(int(n)), rng) for t, n in enumerate(lengths)]
    return camera(), _cat(parts), [int(n) for n in lengths]


# ---- which sort path a list takes: restatements of sort.hip's bucket maps in float32 -----------------------------------

_f = np.float32


def _cell_of(d, fmin, cscale, ncells):
    """lr_depth_cell (sort.hip:188-194) -> (cell, frac)."""
    with np.errstate(invalid="ignore", over="ignore"):
        rel = (d - fmin) * cscale                              # nan for every key when the range is 0 (0 * inf)
        ok = rel >= 0
        c = np.where(ok, np.fmin(rel, _f(ncells - 1)), _f(0)).astype(np.uint32)     # below the range / nan -> cell 0
        frac = np.fmin(rel - c.astype(np.float32), _f(0.99999994))                   # fminf(nan, x) = x
        frac = np.where(frac >= 0, frac, _f(0)).astype(np.float32)
    return c, frac


def _table(cellcnt, ncells, sampled, nb, eq):
    """lr_depth_map_build (sort.hip:205-219) -> (first bucket, buckets) per cell."""
    if eq:
        n = 1 + (cellcnt.astype(np.uint64) * np.uint64(nb - ncells)) // np.uint64(max(sampled, 1))
    else:
        n = np.full(ncells, nb // ncells, np.uint64)
    n = n.astype(np.int64)
    return np.cumsum(n) - n, n


def _bucket_counts(d, fmin, cscale, ncells, first, n, nb):
    """lr_depth_bucket (sort.hip:195-200) for every key -> bucket sizes."""
    c, frac = _cell_of(d, fmin, cscale, ncells)
    b = first[c] + np.minimum((frac * n[c].astype(np.float32)).astype(np.int64), n[c] - 1)
    return np.bincount(b, minlength=nb)


def _p2(L):
    p = 8
    while p < L:
        p <<= 1
    return p


def regime_lds(z):
    """The path lr_bucket_tile (sort.hip:284-372) takes for a list with depths z (float32, any order: its range and both
    its cell histograms are over ALL keys) -> (regime, largest bucket of the linear map, of the equalised map).
    `linear`: the first map leaves no bucket above LR_BUCKET_MAX; `equalised`: the second does; `network`: neither."""
    z = np.asarray(z, np.float32)
    L = len(z)
    assert 0 < L <= LONG_LIST
    nb = max(_p2(L) >> 2, 8)                                   # :286
    ncells = min(64, nb >> 1)                                  # :314
    fmin = z.min()
    with np.errstate(divide="ignore"):
        cscale = _f(ncells) / (z.max() - fmin)                 # :315 (inf when the range is 0)
    first, n = _table(None, ncells, L, nb, False)
    m0 = int(_bucket_counts(z, fmin, cscale, ncells, first, n, nb).max())
    if m0 <= BUCKET_MAX:
        return "linear", m0, None
    c, _ = _cell_of(z, fmin, cscale, ncells)                   # :322-328: the histogram of all keys
    first, n = _table(np.bincount(c, minlength=ncells), ncells, L, nb, True)
    m1 = int(_bucket_counts(z, fmin, cscale, ncells, first, n, nb).max())
    return ("equalised" if m1 <= BUCKET_MAX else "network"), m0, m1


def regime_streamed(z):
    """The same for lr_sort_long_list (sort.hip:482-580) and a list whose keys ARRIVE in the order of z: the depth range
    comes from Ls sampled keys (64-key pieces at piece * L / npieces), widened by 1 % on either side, and the equalised
    map's histogram from the first min(Ls, 8192) samples -- so the answer depends on the arrival order, which on the device
    is the fill's and not the oracle's.  (fmin = smin - 0.01 * range is one fused operation on the device and two here:
    one ulp of the range's lower end.)"""
    z = np.asarray(z, np.float32)
    L = len(z)
    assert L > LONG_LIST
    nb = min(4096, _p2(L) >> 1)                                # :484
    Ls = min(L, max(L >> 4, 2048)) & ~63                       # :496
    npieces = Ls >> 6
    j = np.arange(Ls, dtype=np.int64)
    sample = z[(j >> 6) * L // npieces + (j & 63)]             # :498-500
    smin = sample.min()
    srange = sample.max() - smin
    fmin = smin - _f(0.01) * srange                            # :522
    ncells = min(64, nb >> 1)
    with np.errstate(divide="ignore"):
        cscale = _f(ncells) / (_f(1.02) * srange)              # :524
    first, n = _table(None, ncells, L, nb, False)
    m0 = int(_bucket_counts(z, fmin, cscale, ncells, first, n, nb).max())
    if m0 <= BUCKET_MAX:
        return "linear", m0, None
    Lh = min(Ls, 8192)                                         # :535-539
    c, _ = _cell_of(sample[:Lh], fmin, cscale, ncells)
    first, n = _table(np.bincount(c, minlength=ncells), ncells, Lh, nb, True)
    m1 = int(_bucket_counts(z, fmin, cscale, ncells, first, n, nb).max())
    return ("equalised" if m1 <= BUCKET_MAX else "network"), m0, m1


# ---- the case table ----------------------------------------------------------------------------------------------------
# regime: what sort.hip does with the main list (None: not declared -- it depends on the arrival order); tie: the largest
# number of keys with the same depth bits (None: not declared); open: some pixel of tile 4 walks to the list's last entry.

LENGTHS = [1, 8, 9, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 7680, 7681, 7744, 8191, 8192,
           8193, 16384, 16385, 24577]
OFFC_LENGTHS = [65, 4097, 7681, 8193]
STREAMED_CELLS = 8193                                        # the `cells` list of the streamed class


class Case:
    def __init__(self, L, pattern, regime, tie, front=None):
        self.L, self.pattern, self.regime, self.tie, self.front = L, pattern, regime, tie, front
        self.open = front is None
        self.id = "%s-%d%s" % (pattern, L, "-closed" if front else "")

    def scene(self):
        return one_tile(self.L, self.pattern, front=self.front)

    @property
    def size_class(self):
        return "small" if self.L <= 1024 else ("lds" if self.L <= LONG_LIST else "streamed")


def _cases():
    out = [Case(L, "spread", "linear", 1) for L in LENGTHS]
    out += [Case(L, "flat", "linear" if L <= BUCKET_MAX else "network", L) for L in (33, 1024, 1025, 4096, 4097, 8192, 8193, 16385, 24577)]
    for L in (64, 1024, 1025, 4096, 4097, 8193):
        out += [Case(L, "tie32", "linear", 32), Case(L, "tie33", "network", 33)]
    out += [Case(L, "tie%d" % k, "linear", k) for L in (4097, 8193) for k in (8, 9)]
    out += [Case(L, "cells", "equalised", 1) for L in (1024, 1025, 4096, STREAMED_CELLS)]
    # (99.5 % of the keys in 1/48 of ONE cell: beyond what 64 cells of linear buckets spread, in any arrival order)
    out += [Case(L, "strays", "network", None) for L in (4097, 9000, 20000)]
    # every pixel stops at once: the tail of a list left at its first window is never asked for
    # (`spread` only: the front splats' depth, if sampled, moves the range a `cells` list is laid out for)
    out += [Case(L, "spread", "linear", 1, front="closed") for L in (7681, 8193, 20000)]
    # `spread` with every centre off its pixel: a partial second chunk, just past LONG_LIST, just past LONG_WIN, a tail that is
    # ordered on demand -- with all nine of the reverse walk's sums live on (nearly) every entry
    out += [Case(L, "offc", "linear", 1) for L in OFFC_LENGTHS]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
KNOB_LENGTHS = [64, 65, 4096, 4097, 7681, 8193, 16385]          # `spread`: both forms, lazy sort off, no hit masks
ADJACENT = [(63, 1, 64, 65, 127, 130),
            # a streamed list between two short ones; tiles 2 and 3 begin in the 64-entry chunk the list before them ends in
            (37, 4097, 61, 100, 3, 66)]

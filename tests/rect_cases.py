"""Gaussians with EXACT tile rects at EXACT indices, and a statement of which binning path each one takes.

The stage in front of the per-tile sort -- the projection's counting and ranking, lr_count_huge_kernel, the scan and the two
fill kernels (log_amd/csrc/project.hip), planned by lr_pick_batch (log_amd/csrc/api.hip) -- treats a Gaussian by the CLASS
of its rect (tile count nt = w * h) and by WHERE it sits in the array (lane, wave, 256-Gaussian chunk, batch, plane).  Random
scenes land inside the regimes; the scenes here put live rects ON the boundaries:

  camera      R = I, T = 0, focal 60, so a centre at view depth z projects to pixel (u, v) = W/2 - 0.5 + 60 x / z.
  live        axis-aligned, round across the view axis and DEPTH_RATIO as deep along it (a sphere's dL/drotation is zero: no
              reference for the backward), z = 2 + 1e-4 k (distinct depths: the list order is unambiguous), opacity 0.9.
              Its 3-sigma radius in pixels is solved (restatement of lr_ewa_t / lr_radius_from_cov below) so that the rect
              is a square of s x s tiles at a stated tile origin; the image's edges clip the square to rows, columns and
              w x h rects.
  filler      behind the camera (z = -1): culled by `tz > 0.2` in the device code and in the oracle alike, radius 0, no
              rect.  They cost nothing and make N -- and with it the lane, wave, chunk, batch and plane of every live rect --
              free to choose.

Nothing here imports the GPU side: tests/test_rect_cases_cpu.py checks every declaration through the oracle,
tests/test_gpu_binning_boundaries.py runs the table on the device and asserts the device's own record of the path.
"""
import math

import numpy as np

from log_amd import scenes

FOCAL = 60.0
OPACITY = 0.9
# the constants of the stage, next to their names in log_amd/csrc
RANKED_TILES = 4            # LR_RANKED_TILES: rects of up to this many tiles are ranked in the record / fill record
COOP_TILES = 16             # LR_COOP_TILES = the default of LOGRAST_DEFER_TILES: rects above are deferred
MID_ROW = 16                # LR_MID_ROW: ranks per rank row
MID_COOP = 16               # default of LOGRAST_MID_COOP: mid rects per wave up to which the wave expands them together
HUGE_DIRECT = 8             # LR_HUGE_DIRECT: deferred rects per 256-chunk counted without the LDS plane
HUGE_CHUNK = 256            # bit c of a batch's hugemask = its 256-Gaussian chunk c
WAVE = 64
BATCH_THREADS = 1024        # LR_BATCH_THREADS
BATCH_LDS_BYTES = 160 * 1024 - 512      # LR_BATCH_LDS_BYTES
BATCH_SLOTS = 256           # default of LOGRAST_BATCH_SLOTS
MAX_PLANES = 4              # LR_MAX_PLANES = the default of LOGRAST_BATCH_PLANES
FILL_STAGED_ROWS = 1024     # LR_FILL_STAGED_ROWS
RING = 128                  # LR_RING (band form): a wave's survivor ring fires at 64 pending
FILTER_DILATE, FILTER_CLAMP = 1, 2      # include/lograst.h: LOGRAST_FILTER_*
DEPTH_RATIO = 0.6           # a live Gaussian's scale along the view axis over its scale across it (a sphere's dL/drotation is zero)


def mid_cap(B):
    """lr_mid_cap: rank rows per batch."""
    return B // 4


def camera(W, H):
    K = np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1.0]])
    return scenes.make_camera(np.eye(3), np.zeros(3), K, W=W, H=H)


def plan(N, W, H, slots=BATCH_SLOTS, staged=2):
    """lr_pick_batch + lr_fill_staged_k (api.hip) for a full view -> (batch, planes, staged K)."""
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    smax = max(1, min(BATCH_LDS_BYTES // (4 * tiles), MAX_PLANES, 4))
    per_round = slots * 32768 * smax
    rounds = (N + per_round - 1) // per_round
    groups = slots * rounds
    g = (N + groups - 1) // groups
    planes = min(max((g + 32767) // 32768, 1), smax)
    b = ((g + planes - 1) // planes + 2047) // 2048 * 2048
    b = min(max(b, 4096), 32768)
    K = 0
    if staged > 0 and b % FILL_STAGED_ROWS == 0 and tiles <= 12288:
        K = min(staged, 3)
        while K > 1 and (b // FILL_STAGED_ROWS) % K:
            K -= 1
    return b, planes, K


# ---- the radius of a live Gaussian: lr_ewa_t + lr_radius_from_cov in float64 ---------------------------------------

def _radius_px(a2, px, py, filter_mode):
    """3 sqrt(larger eigenvalue) of the 2D covariance a2 (I + DEPTH_RATIO^2 p p^T) after the low-pass: a2 = (focal sigma /
    z)^2, p = the centre's (x / z, y / z) (inside the 1.3 tan(fov) clamp: asserted by the builder)."""
    q = DEPTH_RATIO * DEPTH_RATIO
    a, b, c = a2 * (1 + q * px * px), a2 * q * px * py, a2 * (1 + q * py * py)
    if filter_mode == FILTER_DILATE:
        a, c = a + 0.3, c + 0.3
    elif filter_mode == FILTER_CLAMP:
        a, c = max(a, 0.3), max(c, 0.3)
    mid = 0.5 * (a + c)
    return 3.0 * math.sqrt(mid + math.sqrt(max(0.1, mid * mid - (a * c - b * b))))


def _solve_a2(target, px, py, filter_mode):
    lo, hi = 1e-6, 1e6
    for _ in range(200):
        m = math.sqrt(lo * hi)
        lo, hi = (m, hi) if _radius_px(m, px, py, filter_mode) < target else (lo, m)
    return lo


class Live:
    """One live Gaussian: array index i, a square of s x s tiles with its corner at tile (X0, Y0) of the unbounded grid."""

    def __init__(self, i, X0, Y0, s):
        self.i, self.X0, self.Y0, self.s = int(i), int(X0), int(Y0), int(s)

    def rect(self, gx, gy, rows=None):
        """(x0, y0, w, h) after the image's clip; rows = (begin, end): clipped to that band of tile rows as well (None
        when nothing is left: the Gaussian is no survivor of the band)."""
        x0, x1 = max(self.X0, 0), min(self.X0 + self.s, gx)
        y0, y1 = max(self.Y0, 0), min(self.Y0 + self.s, gy)
        assert x1 > x0 and y1 > y0
        if rows is not None:
            y0, y1 = max(y0, rows[0]), min(y1, rows[1])
            if y1 <= y0:
                return None
        return x0, y0, x1 - x0, y1 - y0


def build(W, H, N, lives, filter_mode=FILTER_CLAMP):
    """-> scene dict.  The ceil'ed radius rf of a live Gaussian is 8 s - 8 (s = 1: 4) around the centre pixel
    8 (X0 + X1): then (mx - rf) / 16 lies half a tile inside tile X0 and (mx + rf + 15) / 16 inside tile X1, and the radius
    itself is solved to rf - 0.5, half a pixel from either neighbouring integer."""
    xyz = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (N, 1))
    scal = np.full((N, 3), 0.01, np.float32)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (N, 1))
    rng = np.random.default_rng([W, H, N % 9973, len(lives)])
    op = np.full((N, 1), 0.5, np.float32)
    col = np.full((N, 3), 0.5, np.float32)
    seen = set()
    for k, lv in enumerate(lives):
        assert 0 <= lv.i < N and lv.i not in seen, lv.i
        seen.add(lv.i)
        z = float(np.float32(2.0 + 1e-4 * k))
        mx, my = 8.0 * (2 * lv.X0 + lv.s), 8.0 * (2 * lv.Y0 + lv.s)
        px, py = (mx + 0.5 - W / 2.0) / FOCAL, (my + 0.5 - H / 2.0) / FOCAL
        assert abs(px) < 1.25 * (W / 2.0) / FOCAL and abs(py) < 1.25 * (H / 2.0) / FOCAL, "centre outside the 1.3 tan(fov) clamp / ndc cull"
        rf = 4 if lv.s == 1 else 8 * lv.s - 8
        a2 = _solve_a2(rf - 0.5, px, py, filter_mode)
        xyz[lv.i] = (px * z, py * z, z)
        scal[lv.i] = math.sqrt(a2) * z / FOCAL
        scal[lv.i, 2] *= DEPTH_RATIO
        op[lv.i] = OPACITY
        col[lv.i] = rng.random(3, dtype=np.float32)
    return dict(xyz=xyz, scaling=scal, rotation=rot, opacity=op, colors=col)


def cov3d_of(sc):
    """cov3D_precomp of the scene: the rotation is the identity, so diag(s^2) in float32."""
    s2 = (sc["scaling"].astype(np.float64) ** 2).astype(np.float32)
    z = np.zeros(len(s2), np.float32)
    return np.stack([s2[:, 0], z, z, s2[:, 1], z, s2[:, 2]], axis=1)


# ---- a case and its declaration ------------------------------------------------------------------------------------------

class Case:
    """id; image; N; the live Gaussians; the knobs the case sets for every run (e.g. LOGRAST_BATCH_SLOTS); `legs`: further
    knob settings that must give the bits of the default run; `backward` / `cov3d` / `flavours`: which extra checks run;
    band = (first tile row, end tile row, first Gaussian, workgroup share) for the band form."""

    def __init__(self, id, W, H, N, lives, knobs=None, legs=(), backward=False, cov3d=False, flavours=False, band=None):
        self.id, self.W, self.H, self.N, self.lives = id, W, H, int(N), list(lives)
        self.knobs, self.legs = dict(knobs or {}), list(legs)
        self.backward, self.cov3d, self.flavours, self.band = backward, cov3d, flavours, band
        self.gx, self.gy = (W + 15) // 16, (H + 15) // 16

    def scene(self, filter_mode=FILTER_CLAMP):
        return camera(self.W, self.H), build(self.W, self.H, self.N, self.lives, filter_mode)

    def declaration(self, defer_tiles=COOP_TILES, mid_rank=1):
        """Everything from indices and constants.  -> dict:
        batch / planes / staged_k   the plan
        live     [dict(i, rect, nt, cls, lane, wave, chunk, batch, partial)], cls one of small / mid-ranked / mid-cursor /
                 deferred, or `mid` where a batch holds more rankable rects than rank rows (which of them get the rows is
                 the device's race; their NUMBER is declared)
        rows     {batch: rank rows used}
        flagged  {(batch, chunk)}: hugemask bits
        direct   {(batch, chunk): lr_count_huge_kernel counts that chunk straight into the global counters}
        n_rect   sum of w h."""
        B, planes, K = plan(self.N, self.W, self.H, self.knobs.get("LOGRAST_BATCH_SLOTS", BATCH_SLOTS),
                            self.knobs.get("LOGRAST_FILL_STAGED", 2))
        first_partial = self.N - self.N % WAVE            # lr_project_one<true>: the one partial wave of the array
        out, rankable = [], {}
        for lv in self.lives:
            x0, y0, w, h = lv.rect(self.gx, self.gy)
            nt = w * h
            partial = lv.i >= first_partial
            cls = "small" if nt <= RANKED_TILES else ("deferred" if nt > defer_tiles else "mid")
            b = lv.i // B
            if cls == "mid":
                if nt <= MID_ROW and mid_rank and not partial:
                    rankable[b] = rankable.get(b, 0) + 1
                    cls = "mid-ranked"
                else:
                    cls = "mid-cursor"
            out.append(dict(i=lv.i, rect=(x0, y0, w, h), nt=nt, cls=cls, lane=lv.i % WAVE, wave=lv.i // WAVE,
                            chunk=(lv.i % B) // HUGE_CHUNK, batch=b, partial=partial))
        rows = {b: min(n, mid_cap(B)) for b, n in rankable.items()}
        for d in out:
            if d["cls"] == "mid-ranked" and rankable[d["batch"]] > mid_cap(B):
                d["cls"] = "mid"
        flagged = {(d["batch"], d["chunk"]) for d in out if d["cls"] == "deferred"}
        per_chunk = {}
        for d in out:
            if d["cls"] == "deferred":
                per_chunk[(d["batch"], d["chunk"])] = per_chunk.get((d["batch"], d["chunk"]), 0) + 1
        direct = {k: n <= HUGE_DIRECT for k, n in per_chunk.items()}
        return dict(batch=B, planes=planes, staged_k=K, live=out, rows=rows, flagged=flagged, direct=direct,
                    n_rect=sum(d["nt"] for d in out))

    def band_declaration(self, defer_tiles=COOP_TILES):
        """The band form (lr_project_band_kernel) on tile rows self.band: a workgroup owns `span` = planes x batch Gaussians,
        its wave w the Gaussians base + 64 w + 1024 k + lane; survivors (a rect inside the band) go through the wave's ring
        to the front of the workgroup's fill-record slots.  -> dict:
        batch, span
        share     {(workgroup, wave): survivors}
        slots     {workgroup: [Gaussian of slot 0, 1, ...]} where one wave holds all of the workgroup's survivors (ring
                  order = index order); None where several waves race for the slots
        live      [dict(i, rect, nt, cls, survivor)], cls small / mid-cursor / deferred (the band form ranks no mid rect)
        flagged   {(batch, chunk)} of the SLOTS of the deferred survivors
        n_rect    sum of w h inside the band."""
        B, _, _ = plan(self.N, self.W, self.H, self.knobs.get("LOGRAST_BATCH_SLOTS", BATCH_SLOTS))
        planes = min(MAX_PLANES, (BAND_LDS_BYTES - BAND_STATIC_LDS) // (4 * (self.band[1] - self.band[0]) * self.gx))
        span = planes * B
        out, share, by_wg = [], {}, {}
        for lv in sorted(self.lives, key=lambda l: l.i):
            r = lv.rect(self.gx, self.gy, self.band)
            d = dict(i=lv.i, rect=r, nt=0, cls=None, survivor=r is not None)
            if r is not None:
                d["nt"] = r[2] * r[3]
                d["cls"] = "small" if d["nt"] <= RANKED_TILES else ("deferred" if d["nt"] > defer_tiles else "mid-cursor")
                wg, wave = lv.i // span, ((lv.i % span) % BATCH_THREADS) // WAVE
                share[(wg, wave)] = share.get((wg, wave), 0) + 1
                by_wg.setdefault(wg, []).append(d)
            out.append(d)
        slots, flagged = {}, set()
        for wg, ds in by_wg.items():
            one_wave = sum(1 for k in share if k[0] == wg) == 1
            slots[wg] = [d["i"] for d in ds] if one_wave else None
            for pos, d in enumerate(ds):
                if d["cls"] == "deferred":
                    assert one_wave, "a deferred survivor's slot is declared only where one wave fills the workgroup's slots"
                    flagged.add((wg * planes + pos // B, (pos % B) // HUGE_CHUNK))
        return dict(batch=B, span=span, share=share, slots=slots, live=out, flagged=flagged, n_rect=sum(d["nt"] for d in out))


BAND_LDS_BYTES = 160 * 1024 - 512                                       # LR_BAND_LDS_BYTES
BAND_STATIC_LDS = (BATCH_THREADS // 64) * RING * (10 + 1) * 4 + 128     # LR_BAND_STATIC_LDS: the rings + the small words

# ---- the table -----------------------------------------------------------------------------------------------------------
SQ, ROW, COL = (400, 400), (400, 16), (16, 400)          # 25x25, 25x1 and 1x25 tiles
DEFER_LEGS = [{"LOGRAST_DEFER_TILES": 4}, {"LOGRAST_DEFER_TILES": 100}]
MID_LEGS = [{"LOGRAST_MID_RANK": 0}, {"LOGRAST_MID_COOP": 0}]
FILL_LEGS = [{"LOGRAST_FILL_STAGED": 0}, {"LOGRAST_FILL_STAGED": 3},
             {"LOGRAST_FILL_STAGED": 0, "LOGRAST_FILL_PER_THREAD": 2}, {"LOGRAST_FILL_STAGED": 0, "LOGRAST_FILL_PER_THREAD": 4},
             {"LOGRAST_HELPER_MIN_N": 0}, {"LOGRAST_HELPER_MIN_N": 0, "LOGRAST_FILL_STAGED": 0}]
HUGE_LEGS = [{"LOGRAST_HUGE_CHUNK": 512}]


def _strip(sizes, column=False, step=37, first=5):
    """Rects of s x 1 (column: 1 x s) tiles on a one-tile-high image, one per size, `step` Gaussians apart (another lane and,
    every other one, another wave), corners cycling over the strip."""
    out = []
    for k, s in enumerate(sizes):
        X0 = (3 * k) % (25 - s + 1)
        Y0 = -(s // 2)                                   # the square's rows straddle the image's one row
        out.append(Live(first + step * k, *((Y0, X0) if column else (X0, Y0)), s))
    return out


def _square_classes():
    """On 25x25 tiles: every order of the ranked class (one row, one column, 2x2), mid rects, and the deferred sizes on
    either side of 64 = one whole-wave pass (8x8 = 64 tiles, 13x5 = 65), 5x13, and a rect over the whole grid."""
    spec = [(3, 3, 1), (5, 5, 2), (7, -1, 2), (-1, 7, 2), (10, -2, 3), (-2, 10, 3), (14, -3, 4), (-3, 14, 4),   # 1x1 2x2 2x1 1x2 3x1 1x3 4x1 1x4
            (19, -4, 5), (-4, 19, 5),                                                                                # 5x1, 1x5
            (8, -1, 3), (-1, 12, 3), (12, 12, 3), (16, 16, 4), (2, 18, 5),                                           # 3x2 2x3 3x3 4x4 5x5
            (15, 2, 8), (1, -8, 13), (-8, 9, 13), (-1, -1, 27)]                                                      # 64, 65, 65, 625
    return [Live(3 + 29 * k, X0, Y0, s) for k, (X0, Y0, s) in enumerate(spec)]


def _with_companions(lives, gx, gy):
    """Behind every rect of 2..16 tiles, in the next lane, a one-tile rect on the rect's SECOND tile (its first if it is a
    column: the one below).  That tile's run then holds two ranks and the rect's other tiles one, so a tile order on which
    projection and fill disagree puts two keys into one slot."""
    out = []
    for lv in lives:
        out.append(lv)
        x0, y0, w, h = lv.rect(gx, gy)
        if 2 <= w * h <= MID_ROW:
            out.append(Live(lv.i + 1, x0 + 1, y0, 1) if w > 1 else Live(lv.i + 1, x0, y0 + 1, 1))
    return out


def _grid_positions(n, s=3, g=25):
    """n corners of s x s rects spread over a g x g grid (no tile under more than a few dozen of them)."""
    span = g - s + 1
    return [((7 * k) % span, (11 * k + (7 * k) // span) % span) for k in range(n)]


def _mids(indices, s=3):
    return [Live(i, X0, Y0, s) for i, (X0, Y0) in zip(indices, _grid_positions(len(indices), s))]


def _wave_case(K):
    """K mid rects (3x3) in wave 1 of 256 Gaussians, lanes spread evenly; one more in wave 3."""
    lanes = [(l * 64) // K for l in range(K)]
    return Case("mid-wave-%d" % K, *SQ, 256, _mids([64 + l for l in lanes] + [200]), legs=MID_LEGS)


def _row_case(K):
    """K rankable rects in batch 0 (cap 1024 rows) of a two-batch input, three in batch 1: a row index one too large would
    land in batch 1's row 0."""
    idx = [(i * 4096) // K for i in range(K)] + [4096, 4096 + 700, 8191]
    return Case("rank-rows-%d" % K, *SQ, 8192, _mids(idx), legs=MID_LEGS[:1] + FILL_LEGS[:1])


def _huge_case(K):
    """K deferred rects (5x5) in chunk 1 of batch 0."""
    pos = _grid_positions(K, 5)
    return Case("huge-%d-in-chunk" % K, *SQ, 1024, [Live(256 + 19 * k, *pos[k], 5) for k in range(K)], legs=HUGE_LEGS)


def _end_case(N, last="mid", suffix=""):
    """A special rect in the LAST Gaussian (3x3: mid, or 5x5: deferred), a deferred one in the first, a 2x2 in the middle."""
    lives = [Live(N - 1, 12, 12, 3 if last == "mid" else 5)]
    if N > 1:
        lives.append(Live(0, 2, 18, 5))
    if N > 2:
        lives.append(Live(N // 2, 5, 5, 2))
    # (n-4095: the partial wave and the last full wave through lr_project_batched_kernel<COV3D = true> as well)
    return Case("n-%d%s" % (N, suffix), *SQ, N, lives, backward=True, legs=FILL_LEGS[:1], cov3d=N == 4095)


def _plan_lives(B, batches):
    """One rect of every class in each of the given batches (at a chunk's last lane, a wave's first, mid-batch)."""
    out = []
    for k, b in enumerate(batches):
        out += [Live(b * B + 255, 3 + k, 3, 1), Live(b * B + 256, 5, 5 + k, 2), Live(b * B + B // 2 + 1, 12 + k, 12, 3),
                Live(b * B + B - 1, 2 + k, 18, 5), Live(b * B + 64 * 7 + 63, 15, 2 + k, 8)]
    return out


BAND_ROWS = (10, 14)                                     # four of the 25 tile rows: 100 tiles, four counter planes per workgroup
BAND_SPAN = 4 * 4096                                     # Gaussians per band workgroup at batch 4096
BAND_DEFERRED = {1, 62, 65, 127, 255, 256}               # ring positions that hold a deferred rect (5x5 clipped to 5x4) ...
BAND_MID = {0, 63, 64, 128, 257}                         # ... and a 3x3 one; everything else one tile
BAND_LEGS = [{"LOGRAST_BAND_SPARSE": 0}]


def _band_live(i, pos):
    if pos in BAND_DEFERRED:
        return Live(i, (3 * pos) % 21, 9, 5)             # rows 9..13, clipped to 10..13
    if pos in BAND_MID:
        return Live(i, (5 * pos) % 23, 10 + pos % 2, 3)
    return Live(i, (7 * pos) % 25, 10 + pos % 4, 1)


def _band_case(steps, wave=3, wg=0, tag=""):
    """steps[k] survivors in the k-th 64 Gaussians of ONE wave's share of workgroup `wg` (lanes spread evenly): the ring
    holds sum(steps[:k + 1]) minus what it fired.  Outside the band: a rect in the next wave's share and one in the LAST
    step of this wave's share (no survivors).  The other workgroup has one survivor."""
    lives, pos = [], 0
    for k, cnt in enumerate(steps):
        for l in range(cnt):
            lives.append(_band_live(wg * BAND_SPAN + 64 * wave + 1024 * k + (l * 64) // cnt, pos))
            pos += 1
    lives.append(Live(wg * BAND_SPAN + 64 * ((wave + 1) % 16) + 5, 4, 2, 3))
    lives.append(Live(wg * BAND_SPAN + 64 * wave + 1024 * 15 + 63, 8, 15, 2))
    lives.append(Live((1 - wg) * BAND_SPAN + 64 * 2 + 7, 6, 12, 2))
    return Case("band-%d%s" % (sum(steps), tag), *SQ, 2 * BAND_SPAN, lives, legs=BAND_LEGS, band=BAND_ROWS)


def _band_cases():
    out = [_band_case([]), _band_case([1]), _band_case([63]), _band_case([64]), _band_case([64, 1], wave=15),
           _band_case([1, 63], tag="-in-two-steps"),           # the firing condition met by the second step
           _band_case([63, 64]),                                # 127 pending: the fullest ring
           _band_case([64, 64], wg=1), _band_case([63, 64, 2]),
           _band_case([64, 64, 64, 64, 44], tag="-two-slot-chunks")]   # deferred survivors in slots 255 and 256
    # every wave of workgroup 0 holds five survivors (one of them 3x3): the waves share the slot cursor
    lives = [(_band_live(64 * w + 1024 * (w % 3) + 11 * l, 2 + l) if l else Live(64 * w + 1024 * (w % 3), w, 10, 3))
             for w in range(16) for l in range(5)]
    lives.append(Live(64 * 5 + 1024 * 7 + 9, 4, 2, 3))           # outside the band
    # the array ends 27 Gaussians into a wave: `mine` masks the rest; the last Gaussian survives (workgroup 1, two planes)
    n = BAND_SPAN + 4096 + 27
    out.append(Case("band-partial-tail", *SQ, n, [Live(64 * 3 + 1, 3, 9, 5), Live(BAND_SPAN + 5, 7, 11, 1), Live(n - 1, 12, 10, 3),
                                                   Live(n - 2, 4, 2, 3)], legs=BAND_LEGS, band=BAND_ROWS))
    out.append(Case("band-all-waves", *SQ, 2 * BAND_SPAN, lives, legs=BAND_LEGS, band=BAND_ROWS))
    return out


def _cases():
    S64 = {"LOGRAST_BATCH_SLOTS": 64}
    out = [
        # 1. rect classes: 4/5 and 16/17 on rows and columns, 64/65 and the whole grid on the square image
        Case("classes-rows", *ROW, 640, _with_companions(_strip([1, 2, 3, 4, 5, 6, 15, 16, 17, 18, 24, 25]), 25, 1), legs=DEFER_LEGS + MID_LEGS + HUGE_LEGS,
             backward=True, cov3d=True, flavours=True),
        Case("classes-columns", *COL, 640, _with_companions(_strip([1, 2, 3, 4, 5, 6, 15, 16, 17, 18, 24, 25], column=True), 1, 25),
             legs=DEFER_LEGS + MID_LEGS, cov3d=True),
        Case("classes-square", *SQ, 640, _with_companions(_square_classes(), 25, 25), legs=DEFER_LEGS + MID_LEGS + HUGE_LEGS + FILL_LEGS[:4], backward=True,
             cov3d=True, flavours=True),
    ]
    # 2. lr_mid_rects: four rects per pass (1, 4, 5, 64 in one wave); LOGRAST_MID_COOP: 16 cooperative, 17 per lane
    out += [_wave_case(K) for K in (1, 4, 5, MID_COOP, MID_COOP + 1, 64)]
    # 3. rank rows: lr_mid_cap(4096) = 1024
    out += [_row_case(K) for K in (1023, 1024, 1025)]
    # 4. lr_count_huge_kernel: LR_HUGE_DIRECT, batch ends, the hugemask word boundary
    out += [_huge_case(K) for K in (8, 9)]
    out.append(Case("huge-batch-ends", *SQ, 8192, [Live(4095, 2, 2, 5), Live(4096, 10, 10, 5), Live(5000, 12, 12, 3)], legs=HUGE_LEGS))
    B10 = 10240
    out.append(Case("huge-chunks-31-32", *SQ, 600000,
                    [Live(B10 + 31 * 256 + 255, 2, 2, 5), Live(B10 + 32 * 256, 10, 10, 5), Live(B10 + 39 * 256 + 17, 15, 2, 8),
                     Live(3, 12, 12, 3), Live(599999, 5, 5, 2)], knobs=S64, legs=HUGE_LEGS + FILL_LEGS[:1]))
    # 5. array and batch ends
    out += [_end_case(N) for N in (1, 63, 64, 65, 4095, 4096, 4097, 4160)]
    out.append(_end_case(4097, "deferred", "-deferred"))
    # 6. the plan: batch 6144 (staged K = 3), two planes per workgroup
    out.append(Case("plan-batch-6144", *SQ, 393216, _plan_lives(6144, (0, 1, 63)), knobs=S64, legs=FILL_LEGS))
    out.append(Case("plan-two-planes", *SQ, 2200000, _plan_lives(18432, (0, 1, 2, 3)), knobs=S64,
                    legs=[FILL_LEGS[0], FILL_LEGS[5]]))
    # 7. the band form: the survivor ring of one wave
    out += _band_cases()
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
# which case ids sit on either side of each boundary (tests/test_rect_cases_cpu.py asserts the table against this list)
BOUNDARIES = {
    "nt 4|5 (LR_RANKED_TILES)": ("classes-rows", "classes-columns", "classes-square"),
    "nt 16|17 (LOGRAST_DEFER_TILES, LR_MID_ROW)": ("classes-rows", "classes-columns"),
    "nt 64|65 (whole-wave pass)": ("classes-square",),
    "mid rects per wave 4|5 (lr_mid_rects pass)": ("mid-wave-4", "mid-wave-5"),
    "mid rects per wave 16|17 (LOGRAST_MID_COOP)": ("mid-wave-16", "mid-wave-17"),
    "rank rows 1024|1025 (lr_mid_cap)": ("rank-rows-1023", "rank-rows-1024", "rank-rows-1025"),
    "deferred per chunk 8|9 (LR_HUGE_DIRECT)": ("huge-8-in-chunk", "huge-9-in-chunk"),
    "flagged chunk at a batch's end|start": ("huge-batch-ends",),
    "hugemask word 31|32": ("huge-chunks-31-32",),
    "N 63|64|65 (ulane clamp, one full wave)": ("n-1", "n-63", "n-64", "n-65"),
    "N 4095|4096|4097 (batch end)": ("n-4095", "n-4096", "n-4097", "n-4097-deferred", "n-4160"),
    "batch 4096|6144|18432, planes 1|2": ("classes-square", "plan-batch-6144", "plan-two-planes"),
    "band ring 63|64|65 pending (fires at 64)": ("band-0", "band-1", "band-63", "band-64", "band-65", "band-64-in-two-steps"),
    "band ring 127|128|129 (LR_RING)": ("band-127", "band-128", "band-129"),
    "band slot chunk 255|256, shared slot cursor": ("band-300-two-slot-chunks", "band-all-waves"),
    "band array end inside a wave": ("band-partial-tail", "band-128"),
}
BAND_CASES = [c for c in CASES if c.band]

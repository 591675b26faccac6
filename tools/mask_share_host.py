"""Host-side estimate of what contribution masks (LOGRAST_HIT_MASKS=1 against 2) remove from the row-split reverse walk: on a sample of tiles of one
tile row of a bench view, the CPU oracle's lists and n_contrib, the compositing recurrence of blend.hip per pixel, and the
support test of common.hpp (lr_support_prepare / lr_support_box, IEEE divisions and square roots instead of the device's
approximate ones) per (entry, 4x4 block).  Counted in front of each block's deepest contributor, as the reverse walk cuts
its masks: support visits, contributing visits, and the passes per (wave, 64-entry chunk) = max over the wave's four blocks
of ceil(visits / 2).  A sample, not the device's own masks: tools/mask_stats.py reads those.
    python tools/mask_share_host.py [--gaussians N] [--opacity X] [--scene random|trained] [--tile-row R] [--tiles K]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def support(r, x0, x1, y0, y1):
    import numpy as np
    f32 = np.float32
    mx, my, A, B, C, op = [f32(r[i]) for i in range(6)]
    if op < 1 / 512:
        return False
    tau = f32(np.log(f32(255) * op)) * f32(1.01) + f32(0.01)
    det = A * C - B * B
    ex2, ey2 = (2 * tau * C / det, 2 * tau * A / det) if det > 0 else (-1.0, -1.0)
    if not (ex2 >= 0 and ey2 >= 0):
        return True                                     # mode 1: cannot cull safely
    ex, ey = np.sqrt(ex2) * f32(1.0001) + f32(0.01), np.sqrt(ey2) * f32(1.0001) + f32(0.01)
    if not ((mx + ex >= x0) and (mx - ex <= x1) and (my + ey >= y0) and (my - ey <= y1)):
        return False
    dx0, dx1, dy0, dy1 = (x0 - 0.01) - mx, (x1 + 0.01) - mx, (y0 - 0.01) - my, (y1 + 0.01) - my
    if dx0 <= 0 and dx1 >= 0 and dy0 <= 0 and dy1 >= 0:
        return True
    dx = dx0 if dx0 > 0 else dx1
    dy = min(dy1, max(dy0, -B * dx / C))
    bv = 0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy
    ey_ = dy0 if dy0 > 0 else dy1
    ex_ = min(dx1, max(dx0, -B * ey_ / A))
    bh = 0.5 * (A * ex_ * ex_ + C * ey_ * ey_) + B * ex_ * ey_
    return not (min(bv, bh) > tau)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=30_000_000)
    ap.add_argument("--opacity", type=float, default=0.999, help="<0: random opacities")
    ap.add_argument("--scene", choices=("random", "trained"), default="random")
    ap.add_argument("--tile-row", type=int, default=33)
    ap.add_argument("--tiles", type=int, default=12, help="tiles sampled between columns 36 and 84 of the row")
    a = ap.parse_args()
    import numpy as np
    from log_amd import scenes
    from oracle import oracle
    import gpu_util as G
    oracle.build()
    f32 = np.float32
    W, H, gx = 1920, 1080, 120
    cam = scenes.orbit_cameras(8)[0]
    sc = scenes.trained_like_scene(a.gaussians, seed=0) if a.scene == "trained" else \
        scenes.random_scene(a.gaussians, seed=0, opacity=(None if a.opacity < 0 else a.opacity))
    _, of = G.oracle_forward(oracle, cam, sc, (0, 0, 0), tile_rows=(a.tile_row, a.tile_row + 1))
    offs, pl, rec, ncimg = of["tile_offsets"].astype(np.int64), of["point_list"], of["rec"], of["n_contrib"]
    blocks = lambda m: m.reshape(2, 2, 4, 2, 2, 4)      # qy, by, iy, qx, bx, ix -> column 4 (qy 2 + qx) + by 2 + bx
    tot_s = tot_e = chunks = passes_s = passes_e = 0
    for t in [a.tile_row * gx + int(x) for x in np.linspace(36, 84, a.tiles)]:
        tx, ty = t % gx, t // gx
        ys, xs = np.mgrid[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        inside = (xs < W) & (ys < H)
        nc = np.zeros((16, 16), np.int64)
        nc[inside] = ncimg[ys[inside], xs[inside]]
        rmax = blocks(nc).max(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(16)
        depth = int(rmax.max())
        T, done = np.ones((16, 16), f32), ~inside
        S, E = np.zeros((depth, 16), bool), np.zeros((depth, 16), bool)
        for p in range(depth):
            r = rec[pl[offs[t] + p]]
            dx, dy = f32(r[0]) - xs.astype(f32), f32(r[1]) - ys.astype(f32)
            pw = (f32(-0.5) * (r[2] * dx * dx + r[4] * dy * dy) - r[3] * dx * dy).astype(f32)
            al = np.minimum(f32(0.99), r[5] * np.exp(pw)).astype(f32)
            ok = (~done) & ~(pw > 0) & ~(al < f32(1 / 255))
            test = T * (1 - al)
            stop = ok & (test < 1e-4)
            acc = ok & ~stop
            T = np.where(acc, test, T)
            done |= stop
            E[p] = blocks(acc).any(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(16)
            for c in range(16):
                if p < rmax[c]:
                    w, b = c >> 2, c & 3
                    x0, y0 = tx * 16 + (w & 1) * 8 + (b & 1) * 4, ty * 16 + (w >> 1) * 8 + (b >> 1) * 4
                    S[p, c] = support(r, x0, x0 + 3, y0, y0 + 3)
        assert not (E & ~S).any(), "a contribution without support"
        tot_s += int(S.sum())
        tot_e += int(E.sum())
        for w in range(4):
            for c in range((int(rmax[4 * w:4 * w + 4].max()) + 63) // 64):
                hs, he = S[64 * c:64 * c + 64, 4 * w:4 * w + 4].sum(0), E[64 * c:64 * c + 64, 4 * w:4 * w + 4].sum(0)
                passes_s += int(((hs + 1) // 2).max())
                passes_e += int(((he + 1) // 2).max())
                chunks += 1
    print("%d %s Gaussians, opacity %s, tile row %d, %d tiles: support visits %d, contributing %d, pruned share %.3f; "
          "visits per chunk %.1f -> %.1f; passes per chunk %.2f -> %.2f"
          % (a.gaussians, a.scene, a.opacity, a.tile_row, a.tiles, tot_s, tot_e, 1 - tot_e / max(tot_s, 1),
             tot_s / max(chunks, 1), tot_e / max(chunks, 1), passes_s / max(chunks, 1), passes_e / max(chunks, 1)))


if __name__ == "__main__":
    main()

"""CPU model of tile lists expanded on demand (csrc/raster_render.hip, LAZY; nothing here touches a GPU).

Under mvi_raster_list_expansion(1) render_forward finds the entries of a tile's list itself: the list of tile (row b, column x)
is the column segments of column x that cover row b, in segment order, and a block walks its column from the column's first
segment until it has the entries of the rounds it composites. This script runs the oracle forward on the bench view (or any
--gaussians / --width / --height), rebuilds the column segments of pass 1 from the oracle's xy, radii and depths (depth order =
stable order of the depth bits; a Gaussian's tile rectangle is one segment (first row, rows) per tile column), checks that the
rebuilt lists are the oracle's (tiles touched, num_rendered, the length of every sampled tile's list and its Gaussians), and
prints for the tiles of a sample of columns:

    segments per column;
    entries staged per tile: whole rounds of 256, up to and including the round in which the tile's last pixel saturates
    (every round where a pixel never does), and what share of the list that is;
    segments scanned per tile, from the column's first segment to the last staged entry, in steps of --step segments as the
    kernel loads them: for the rounds it composites (the shipped walk: just in time) and with one more round looked at ahead.

A pixel counts as saturated when its final T is below 0.01 while its n_contrib is below the list's length (the kernel ends a
pixel when T (1 - alpha) < 1e-4 with alpha <= 0.99); the round that holds entry number n_contrib is the last one it needs.

    python tools/experiments/lazy_list_model.py [--gaussians N --width W --height H --seed S --columns 12 --step 2048]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TILE, ROUND = 16, 256


def column_segments(f, W, H):
    """The output of pass 1 from the oracle's forward: (column of every segment, first row, end row, Gaussian), column-major,
    depth order inside a column; and tiles touched per Gaussian."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    xy, r = f["xy"].astype(np.float32), f["radii"].astype(np.float32)
    t = np.float32(TILE)
    lo = lambda c: np.clip(((c - r) / t).astype(np.int64), 0, None)
    hi = lambda c: np.clip(((c + r + np.float32(TILE - 1)) / t).astype(np.int64), 0, None)
    x0, x1 = np.minimum(gx, lo(xy[:, 0])), np.minimum(gx, hi(xy[:, 0]))
    y0, y1 = np.minimum(gy, lo(xy[:, 1])), np.minimum(gy, hi(xy[:, 1]))
    w, h = np.maximum(x1 - x0, 0), np.maximum(y1 - y0, 0)
    dead = (f["radii"] <= 0) | (w * h == 0)
    w, h = np.where(dead, 0, w), np.where(dead, 0, h)
    order = np.argsort(np.where(dead, 0xFFFFFFFF, f["depths"].astype(np.float32).view(np.uint32)).astype(np.uint64), kind="stable")
    order = order[~dead[order]]
    reps = w[order]
    g = np.repeat(order, reps)                                              # one segment per (Gaussian, column), depth order
    col = np.repeat(x0[order], reps) + (np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps))
    by_col = np.argsort(col, kind="stable")                                 # stable partition by column = pass 1
    g, col = g[by_col], col[by_col]
    return col, y0[g], y1[g], g, w * h, gx, gy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--columns", type=int, default=12, help="tile columns sampled (evenly spaced)")
    ap.add_argument("--step", type=int, default=2048, help="segments the walk loads per step")
    a = ap.parse_args()
    from multiview_inpaint_amd import synthetic as syn
    from oracle import raster_oracle as ro
    ro.build()
    N, W, H, deg = a.gaussians, a.width, a.height, 3
    cam = syn.make_camera(W, H, 50.0)
    sc = syn.make_scene(N, cam, deg, seed=a.seed)
    p = ro.make_params(N, deg, (deg + 1) ** 2, W, H, cam["tanfovx"], cam["tanfovy"], 1.0, cam["viewmatrix"], cam["projmatrix"],
                       cam["campos"], np.zeros(3, np.float32))
    t0 = time.time()
    f = ro.forward(p, sc["means3D"], sc["opacities"], shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    print(f"N = {N}, {W}x{H}, seed {a.seed}: oracle forward {time.time() - t0:.1f} s, num_rendered {f['num_rendered']}")
    col, y0, y1, g, touched, gx, gy = column_segments(f, W, H)
    assert np.array_equal(touched.astype(np.uint32), f["tiles_touched"] * (f["radii"] > 0)), "tile rectangles differ from the oracle's"
    assert int((y1 - y0).sum()) == f["num_rendered"], "the segments do not expand to num_rendered pairs"
    col_start = np.searchsorted(col, np.arange(gx + 1))
    per_col = np.diff(col_start)
    print(f"{len(col)} column segments, {len(col) / max(f['num_rendered'], 1):.3f} per pair; per column: mean {per_col.mean():.0f}, "
          f"min {per_col.min()}, max {per_col.max()}")
    ranges = f["ranges"].astype(np.int64)
    nc = np.zeros((gy * TILE, gx * TILE), np.int64)
    nc[:H, :W] = f["n_contrib"].astype(np.int64).reshape(H, W)
    fT = np.ones((gy * TILE, gx * TILE), np.float32)
    fT[:H, :W] = f["final_T"].reshape(H, W)
    inside = np.zeros((gy * TILE, gx * TILE), bool)
    inside[:H, :W] = True
    cols = np.unique(np.linspace(0, gx - 1, min(a.columns, gx)).round().astype(int))
    length, staged, scan_now, scan_ahead, exact = [], [], [], [], []
    for x in cols:
        c0, c1 = col_start[x], col_start[x + 1]
        sy0, sy1, sg = y0[c0:c1], y1[c0:c1], g[c0:c1]
        first = c0 & ~1                                                      # the walk starts at the aligned word
        for b in range(gy):
            where = np.nonzero((sy0 <= b) & (b < sy1))[0]                    # the tile's list, as positions in the column
            r0, r1 = ranges[b * gx + x]
            assert len(where) == r1 - r0, ("list length", b, x)
            assert np.array_equal(sg[where], f["point_list"][r0:r1]), ("list", b, x)
            n = len(where)
            rounds = (n + ROUND - 1) // ROUND
            sl = (slice(b * TILE, (b + 1) * TILE), slice(x * TILE, (x + 1) * TILE))
            live = inside[sl] & ~((fT[sl] < 0.01) & (nc[sl] < n))            # pixels that never saturate
            need = rounds if live.any() else min(rounds, int(nc[sl].max()) // ROUND + 1)
            length.append(n)
            staged.append(min(n, need * ROUND))

            def scanned(k):                                                  # segments loaded to find the first k entries
                if k <= 0:
                    return 0
                last = c0 + where[min(k, n) - 1] if k <= n else c1 - 1
                return min(((last + 1 - first) + a.step - 1) // a.step * a.step, (c1 - first + 1) // 2 * 2)
            exact.append(where[staged[-1] - 1] + 1 if staged[-1] else 0)     # segments of the column up to the last staged entry
            scan_now.append(scanned(staged[-1]))
            scan_ahead.append(scanned(min(n, (need + 1) * ROUND)))
    length, staged, scan_now, scan_ahead, exact = (np.array(v, np.float64) for v in (length, staged, scan_now, scan_ahead, exact))
    print(f"{len(length)} tiles of {len(cols)} sampled columns: list length mean {length.mean():.0f}; entries staged per tile mean "
          f"{staged.mean():.0f} = {100 * staged.sum() / max(length.sum(), 1):.1f} % of the lists")
    print("\n| segments scanned per tile | mean | p95 | max |\n|---|---|---|---|")
    for name, v in (("up to the last staged entry (no step granularity)", exact), ("the rounds it composites, in steps", scan_now),
                    ("one more round ahead, in steps", scan_ahead)):
        print(f"| {name} | {v.mean():.0f} | {np.percentile(v, 95):.0f} | {v.max():.0f} |")
    print(f"\nper thread of a 256-thread block: {scan_now.mean() / 256:.1f} segments (just in time), {scan_ahead.mean() / 256:.1f} (one round ahead)")


if __name__ == "__main__":
    main()

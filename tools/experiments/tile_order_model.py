"""List-scheduling model of render_backward's tile order (CPU only; nothing here touches a GPU).

A block of render_backward_kernel replays its tile's list up to the tile's largest n_contrib, so that number (plus a fixed
start-up share) is the block's work. The hardware hands the blocks of a launch to each XCD in id order; the kernel maps block
ids to one contiguous band of tiles per XCD (xcd_band_tile). This script runs the oracle forward on the bench scene (or any
--gaussians / --width / --height), takes every tile's largest n_contrib, and simulates each band on its own:

    32 CUs with `slots` resident blocks each; the next block of the band's order starts on the CU with the most free slots as
    soon as one is free; a CU with b resident blocks advances each of them at min(1, b_sat / b) (its throughput saturates at
    b_sat resident blocks; b_sat = slots: no saturation); the launch ends when the slowest band ends.

Orders: plain tile order inside the band; heaviest first by the 16 classes of width 32 the forward records (tile order inside
a class); an exact descending sort. Printed: the scene's statistics, then makespans (in list entries) and the gain of heaviest
first per b_sat. The model knows nothing about memory, atomics or the instruction mix: it only says what the ORDER is worth if
the blocks are otherwise independent.

    python tools/experiments/tile_order_model.py [--gaussians N --width W --height H --seed S]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BANDS, CUS, CLASSES, CLASS_WIDTH, FIXED = 8, 32, 16, 32, 20


def tile_work(N, W, H, seed, deg=3):
    """(largest n_contrib per tile [tiles], list length per tile [tiles], num_rendered) of the bench view, from the oracle"""
    from multiview_inpaint_amd import synthetic as syn
    from oracle import raster_oracle as ro
    ro.build()
    cam = syn.make_camera(W, H, 50.0)
    sc = syn.make_scene(N, cam, deg, seed=seed)
    p = ro.make_params(N, deg, (deg + 1) ** 2, W, H, cam["tanfovx"], cam["tanfovy"], 1.0, cam["viewmatrix"], cam["projmatrix"],
                       cam["campos"], np.zeros(3, np.float32))
    f = ro.forward(p, sc["means3D"], sc["opacities"], shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nc = np.zeros((gy * 16, gx * 16), np.int64)
    nc[:H, :W] = f["n_contrib"].astype(np.int64).reshape(H, W)
    r = f["ranges"].astype(np.int64)
    return nc.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1), r[:, 1] - r[:, 0], int(f["num_rendered"])


def bands_of(tiles):
    q, r = divmod(tiles, BANDS)
    return [np.arange(x * q + min(x, r), x * q + min(x, r) + q + (1 if x < r else 0)) for x in range(BANDS)]


def makespan(costs, slots, b_sat):
    """One band: blocks of `costs` (in dispatch order) over CUS CUs with `slots` resident blocks each."""
    resident = [[] for _ in range(CUS)]
    nxt, n, t = 0, len(costs), 0.0
    while True:
        while nxt < n:
            cu = min(range(CUS), key=lambda c: len(resident[c]))
            if len(resident[cu]) >= slots:
                break
            resident[cu].append(float(costs[nxt]))
            nxt += 1
        busy = [c for c in range(CUS) if resident[c]]
        if not busy:
            return t
        rate = {c: min(1.0, b_sat / len(resident[c])) for c in busy}
        dt = min(min(resident[c]) / rate[c] for c in busy)
        t += dt
        for c in busy:
            step = rate[c] * dt
            resident[c] = [w - step for w in resident[c] if w - step > 1e-9]


def launch(work, order, slots, b_sat):
    spans = []
    for band in bands_of(len(work)):
        w = work[band]
        if order == "classes":
            cls = np.minimum(CLASSES - 1, w // CLASS_WIDTH)
            w = w[np.argsort(-cls, kind="stable")]
        elif order == "sorted":
            w = np.sort(w)[::-1]
        spans.append(makespan(w + FIXED, slots, b_sat))
    return max(spans)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    work, length, D = tile_work(a.gaussians, a.width, a.height, a.seed)
    tiles = len(work)
    band_tot = np.array([work[b].sum() for b in bands_of(tiles)], np.float64)
    corr = float(np.corrcoef(length, work)[0, 1]) if work.std() > 0 and length.std() > 0 else float("nan")
    print(f"N = {a.gaussians}, {a.width}x{a.height}, seed {a.seed}: num_rendered {D}, {tiles} tiles")
    print(f"largest n_contrib per tile: mean {work.mean():.1f}, p5 {np.percentile(work, 5):.0f}, p95 {np.percentile(work, 95):.0f}, "
          f"max {work.max()}, coefficient of variation {work.std() / max(work.mean(), 1e-9):.2f}")
    print(f"band totals max / mean {band_tot.max() / max(band_tot.mean(), 1e-9):.3f}; correlation of list length with largest n_contrib "
          f"{corr:.2f}; blocks per resident slot {tiles / (BANDS * CUS * 10):.2f}")
    total = float((work + FIXED).sum())
    print("\n| slots per CU | b_sat | plain order | heaviest first (16 classes) | exact sort | gain of heaviest first |")
    print("|---|---|---|---|---|---|")
    for slots, b_sat in ((10, 10), (10, 8), (10, 6), (10, 4), (12, 12)):
        plain, cls, srt = (launch(work, o, slots, b_sat) for o in ("plain", "classes", "sorted"))
        eff = total / (BANDS * CUS * b_sat * plain)
        print(f"| {slots} | {b_sat} | {plain:.0f} (efficiency {eff:.2f}) | {cls:.0f} | {srt:.0f} | {100.0 * (plain - cls) / plain:.1f} % |")


if __name__ == "__main__":
    main()

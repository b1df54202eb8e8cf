"""Cost of mask lifting (raster.lift_weights, csrc/raster_lift.hip) on the bench scene of bench.py (1.5 M Gaussians, 1920 x 1080,
SH degree 3, seed 0), one view:

  (a) the lift kernel at C = 1 and at C = 8, into 64-byte rows ([P, 16], what lift_weights allocates) and, as the A/B of the row
      stride, into tight rows ([P, 1 + C]);
  (b) the route a user had without it: rasterize_backward on a colors_precomp forward with the weight image as grad_color
      (dL/dcolors_precomp is the hits, three channels per call; the rows are zeroed by the backward itself);
  (c) the render_backward stage of (b) alone, from the library's stage timers.

(a) and (b) are timed with device events around `--steps` calls, in ALTERNATING repetitions inside one process, after a warm-up
of every shape; (c) in a loop of its own with only that stage bracketed. Before timing, the hits of a C = 3 lift are compared
with dL/dcolors_precomp of (b). Prints one JSON line and writes it to --out.

    python tools/bench_lift.py --out profiles/mask_lift_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(xs):
    s = sorted(xs)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return dict(reps=[round(x, 4) for x in xs], median=round(med, 4), min=round(s[0], 4), max=round(s[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gaussians", type=int, default=1_500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from multiview_inpaint_amd import _lib, raster as R, synthetic as syn
    assert torch.cuda.is_available(), "this benchmark needs the GPU; there is no CPU figure"
    dev = "cuda:0"
    W, H, N, deg = args.width, args.height, args.gaussians, 3
    cam = syn.make_camera(W, H, 50.0)
    sc = syn.make_scene(N, cam, deg, seed=0)
    t = {k: torch.tensor(v, device=dev) for k, v in sc.items() if k != "sh_degree"}
    rs = R.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device=dev),
        projmatrix=torch.tensor(cam["projmatrix"], device=dev), sh_degree=deg, campos=torch.tensor(cam["campos"], device=dev),
        prefiltered=False)
    gen = torch.Generator(dev).manual_seed(0)
    w8 = torch.randn(8, H, W, device=dev, generator=gen)
    w8[0] = (w8[0] > 0.3).float()                                       # channel 0: a binary mask
    w1, w3 = w8[:1].contiguous(), w8[:3].contiguous()
    ckw = dict(scales=t["scales"], rotations=t["rotations"])
    with torch.no_grad():
        _, _, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], shs=t["shs"], **ckw)
    cp = torch.rand(N, 3, device=dev, generator=gen)
    _, _, _, st_b = R.rasterize_forward(rs, t["means3D"], t["opacities"], colors_precomp=cp, prepare_backward=True, **ckw)

    def backward_route():
        return R.rasterize_backward(rs, st_b, w3, t["means3D"], colors_precomp=cp, **ckw)

    # faster and different is not faster: the hits are the colour gradient of the old route, to the order of the float atomics
    hits = R.lift_weights(st, w3)[:, 1:4]
    ref = backward_route()["colors_precomp"]
    err = float((hits - ref).abs().max() / (ref.abs().max() + 1e-30))
    assert err < 1e-4, err

    acc = {("row16", 1): torch.zeros(N, 16, device=dev)[:, :2], ("row16", 8): torch.zeros(N, 16, device=dev)[:, :9],
           ("tight", 1): torch.zeros(N, 2, device=dev), ("tight", 8): torch.zeros(N, 9, device=dev)}
    modes = {f"lift_c{c}_{row}": (lambda a=a, w=(w1 if c == 1 else w8): R.lift_weights(st, w, acc=a)) for (row, c), a in acc.items()}
    modes["backward_route_c3"] = backward_route

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    for fn in modes.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    out = {m: [] for m in modes}
    for _ in range(args.reps):
        for m, fn in modes.items():                                      # alternating
            out[m].append(timed(fn))
    # (c): the render_backward stage alone, bracketed by the library's own events (stage 6), in a loop of its own
    L = _lib.lib()
    stage = next(i for i in range(8) if L.mvi_raster_stage_name(i) == b"render_backward")
    stage_ms = []
    for _ in range(args.reps):
        L.mvi_raster_timing_enable_stages(1 << stage)
        for _ in range(args.steps):
            backward_route()
        torch.cuda.synchronize()
        L.mvi_raster_timing_enable(0)
        ms, calls = (C.c_float * 8)(), (C.c_int32 * 8)()
        _lib.check(L.mvi_raster_timing_read(ms, calls), "timing_read")
        stage_ms.append(ms[stage] / max(1, calls[stage]))

    res = dict(bench="mask_lift", unit="ms per call, one view", gaussians=N, width=W, height=H, steps_per_rep=args.steps,
               num_rendered=int(st.D), evaluated_pairs=int(st.tensor("n_contrib", (H, W), torch.int32).sum()),
               hits_vs_backward_route_max_rel_diff=err)
    for m, xs in out.items():
        res[m] = _stats(xs)
    res["render_backward_stage_c3"] = _stats(stage_ms)
    res["lift_c1_below_render_backward_stage_in_every_repetition"] = all(a < c for a, c in zip(out["lift_c1_row16"], stage_ms))
    for c in (1, 8):
        res[f"tight_minus_row16_c{c}_ms"] = round(res[f"lift_c{c}_tight"]["median"] - res[f"lift_c{c}_row16"]["median"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

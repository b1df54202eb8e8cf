"""Cost of the feature splat (raster.splat_features, csrc/raster_splat.hip) on the bench scene of bench.py (1.5 M Gaussians,
1920 x 1080, SH degree 3, seed 0), one view:

  (a) the splat kernel at C = 1, 3 and 8 on the state of one finished forward;
  (b) the route a user had without it: one complete rasterize_forward(colors_precomp=F[:, 3k : 3k + 3]) per three channels,
      ceil(C / 3) calls (preprocess, sort and binning repeated every time; the column chunks are cut and padded to three
      columns once, outside the timing);
  (c) the render_forward stage of one such forward alone, from the library's stage timers, times ceil(C / 3).

(a) and (b) are timed with device events around `--steps` calls, in ALTERNATING repetitions inside one process, after a warm-up
of every shape; (c) in a loop of its own with only that stage bracketed. Before timing, a C = 3 splat is compared with the colour
image of a zero-background colors_precomp forward: the two must be torch.equal. Prints one JSON line and writes it to --out.

    python tools/bench_splat.py --out profiles/feature_splat_bench.json
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
    F8 = torch.randn(N, 8, device=dev, generator=gen)
    F = {1: F8[:, :1].contiguous(), 3: F8[:, :3].contiguous(), 8: F8}
    ckw = dict(scales=t["scales"], rotations=t["rotations"])
    with torch.no_grad():
        _, _, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], shs=t["shs"], **ckw)

    def chunks(c):
        out = []
        for c0 in range(0, c, 3):
            part = F8[:, c0:min(c, c0 + 3)]
            pad = torch.zeros(N, 3, device=dev)
            pad[:, :part.shape[1]] = part
            out.append(pad)
        return out

    def forward_route(parts):
        with torch.no_grad():
            return [R.rasterize_forward(rs, t["means3D"], t["opacities"], colors_precomp=p, **ckw)[0] for p in parts]

    parts = {c: chunks(c) for c in (1, 3, 8)}
    # faster and different is not faster: the splat of a forward's colours is that forward's colour image, bit for bit
    with torch.no_grad():
        color, _, _, st_c = R.rasterize_forward(rs, t["means3D"], t["opacities"], colors_precomp=F[3], **ckw)
    equal = bool(torch.equal(R.splat_features(st_c, F[3]), color))
    assert equal, "the C = 3 splat differs from the colour image of the colors_precomp forward"
    del st_c, color

    outs = {c: torch.empty(c, H, W, device=dev) for c in (1, 3, 8)}
    modes = {}
    for c in (1, 3, 8):
        modes[f"splat_c{c}"] = lambda c=c: R.splat_features(st, F[c], out=outs[c])
    for c in (1, 3, 8):
        modes[f"forward_route_c{c}"] = lambda c=c: forward_route(parts[c])

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
    # (c): the render_forward stage of one colors_precomp forward alone, bracketed by the library's own events
    L = _lib.lib()
    stage = next(i for i in range(8) if L.mvi_raster_stage_name(i) == b"render_forward")
    stage_ms = []
    for _ in range(args.reps):
        L.mvi_raster_timing_enable_stages(1 << stage)
        for _ in range(args.steps):
            forward_route(parts[1])
        torch.cuda.synchronize()
        L.mvi_raster_timing_enable(0)
        ms, calls = (C.c_float * 8)(), (C.c_int32 * 8)()
        _lib.check(L.mvi_raster_timing_read(ms, calls), "timing_read")
        stage_ms.append(ms[stage] / max(1, calls[stage]))

    res = dict(bench="feature_splat", unit="ms per call, one view", gaussians=N, width=W, height=H, steps_per_rep=args.steps,
               num_rendered=int(st.D), composited_pairs=int(st.tensor("n_contrib", (H, W), torch.int32).sum()),
               splat_c3_equals_colour_image_of_colors_precomp_forward=equal)
    for m, xs in out.items():
        res[m] = _stats(xs)
    res["render_forward_stage_one_call"] = _stats(stage_ms)
    for c in (1, 3, 8):
        k = (c + 2) // 3
        res[f"render_forward_stage_times_{k}_for_c{c}"] = _stats([k * x for x in stage_ms])
        res[f"splat_c{c}_below_render_forward_stage_times_{k}_in_every_repetition"] = all(
            a < k * b for a, b in zip(out[f"splat_c{c}"], stage_ms))
    res["splat_c8_below_forward_route_c8_in_every_repetition"] = all(a < b for a, b in zip(out["splat_c8"], out["forward_route_c8"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

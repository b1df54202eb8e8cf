"""Times the first-stage decode (and encode) of the SVD pipeline at the bench size: 14 frames, 72x128 latents ->
576x1024 RGB, fp32 (the reference disables autocast for the first stage), seeded random weights, on cuda:0.
Prints one JSON object with the per-op HIP kernel times (hipEvents on the launch stream) beside the total.

    python tools/bench_vae.py [--frames 14] [--h 72] [--w 128] [--iters 3] [--dtype fp32|bf16]
    python tools/bench_vae.py --encode-mode both [--pairs 5]

--encode-mode times the ENCODE alone (no decode): "fp32" the library path, "split3" the split-operand walk (svd/vae_split.py encode), "both"
the two alternating in one process — each route with its own warm-up, then --pairs rounds of (fp32, split3), every call between device
events behind a synchronise — with medians, spread, per-kind hip_ops times, peak memory and the routes' difference on the moments.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FULL = dict(attn_type="vanilla", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
            ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0)


def bench_encode(a, eng, g, dev):
    """The encoder's moments (no regularizer draw: that is a host-side randn, the same on both routes) on the library path and / or the
    split walk, alternating."""
    import statistics
    from multiview_inpaint_amd.svd import hip_ops, vae
    routes = ["fp32", "split3"] if a.encode_mode == "both" else [a.encode_mode]
    x = (torch.rand(a.frames, 3, 8 * a.h, 8 * a.w, generator=g) * 2 - 1).to(dev)
    fn = lambda m: vae.encode_first_stage(eng, x, mode=m, unregularized=True)
    res = {r: {"ms": [], "ops": {}, "peak": 0} for r in routes}
    last = {}

    def call(r, record):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        hip_ops.PROFILE = [] if record else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn(r)
        e1.record()
        torch.cuda.synchronize()
        if record:
            res[r]["ms"].append(e0.elapsed_time(e1))
            for k, (c, t, w) in hip_ops.profile_summary().items():
                res[r]["ops"].setdefault(k, []).append((c, t, w))
            res[r]["peak"] = max(res[r]["peak"], torch.cuda.max_memory_allocated())
        hip_ops.PROFILE = None
        return y
    for r in routes:
        print(f"warm-up {r} ...", file=sys.stderr, flush=True)
        call(r, False)
    for _ in range(max(1, a.pairs)):
        for r in routes:
            last[r] = call(r, True)
    out = {"workload": f"first-stage encode (moments), {a.frames} frames of {8 * a.h}x{8 * a.w}, fp32 contract, seeded random weights",
           "device": torch.cuda.get_device_name(0), "pairs": max(1, a.pairs), "timing": "device events around one synchronised call, routes alternating"}
    for r in routes:
        ms = res[r]["ms"]
        ops = {k: {"calls": v[0][0], "ms": round(statistics.median(t for _, t, _ in v), 3),
                   "GBs_or_GFLOPs": round(v[0][2] / statistics.median(t for _, t, _ in v) / 1e6, 1)} for k, v in res[r]["ops"].items()}
        out[r] = {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2),
                  "all_ms": [round(m, 2) for m in ms], "hip_ops": ops, "hip_ops_ms": round(sum(v["ms"] for v in ops.values()), 2),
                  "peak_mem_GB": round(res[r]["peak"] / 1e9, 2), "finite": bool(torch.isfinite(last[r]).all())}
    if len(routes) == 2:
        out["split3_over_fp32_time"] = round(out["split3"]["median_ms"] / out["fp32"]["median_ms"], 3)
        out["moments_rel_max_diff"] = float((last["split3"] - last["fp32"]).abs().max() / last["fp32"].abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--h", type=int, default=72)
    ap.add_argument("--w", type=int, default=128)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--search", action="store_true", help="let MIOpen time its solvers in the warm-up (minutes in fp32)")
    ap.add_argument("--encode-mode", choices=["fp32", "split3", "both"], default=None, help="time the encode alone on this route / both routes")
    ap.add_argument("--pairs", type=int, default=5, help="--encode-mode: timed calls per route")
    a = ap.parse_args()
    from multiview_inpaint_amd.svd import hip_ops, vae
    import svd_helpers as H
    dev = "cuda:0"
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    torch.backends.cudnn.benchmark = a.search
    eng = vae.AutoencodingEngine(encoder_config=vae.Encoder(**FULL),
                                 decoder_config=vae.VideoDecoder(**FULL, video_kernel_size=[3, 1, 1])).eval()
    eng.decoder.load_state_dict(H.seeded_state_dict(eng.decoder, 42))
    eng.encoder.load_state_dict(H.seeded_state_dict(eng.encoder, 41))
    eng = eng.to(dev)                                            # the model stays fp32: --dtype bf16 is decode_first_stage's opt-in copy
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(a.frames, 4, a.h, a.w, generator=g) * 0.18215).to(dev)
    out = {"workload": f"first-stage decode, {a.frames} frames, latent {a.h}x{a.w} -> {8 * a.h}x{8 * a.w}, {a.dtype}, "
                       "seeded random weights", "iters": a.iters}

    def run(fn, arg):
        with torch.no_grad():
            print("warm-up ...", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            y = fn(arg)                                           # warm-up (MIOpen solver search with --search)
            torch.cuda.synchronize()
            print(f"warm-up done in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            hip_ops.PROFILE = []
            t0 = time.perf_counter()
            for _ in range(a.iters):
                y = fn(arg)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.iters
        prof = hip_ops.profile_summary()
        hip_ops.PROFILE = None
        ops = {k: {"calls": c // a.iters, "ms": round(t / a.iters, 3), "GBs_or_GFLOPs": round(w / t / 1e6, 1) if t else None}
               for k, (c, t, w) in prof.items()}
        return y, ms, ops
    if a.encode_mode:
        print(json.dumps(bench_encode(a, eng, g, dev)))
        return
    y, ms, ops = run(lambda t: vae.decode_first_stage(eng, t, dtype=dt), z)
    out["decode"] = {"ms": round(ms, 2), "frames_per_s": round(a.frames / ms * 1e3, 2), "finite": bool(torch.isfinite(y).all()),
                     "out_shape": list(y.shape), "hip_ops": ops, "hip_ops_ms": round(sum(v["ms"] for v in ops.values()), 2)}
    if a.encode:
        x = torch.rand(a.frames, 3, 8 * a.h, 8 * a.w, generator=g).to(dev) * 2 - 1
        zz, ms, ops = run(lambda t: vae.encode_first_stage(eng, t), x)
        out["encode"] = {"ms": round(ms, 2), "finite": bool(torch.isfinite(zz).all()), "hip_ops": ops}
    out["peak_mem_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

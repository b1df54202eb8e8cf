"""Forward + backward time of ops.add_layer_norm under autograd, bf16 and f16, random data, at the token shapes of the three
transformer levels — the reference's training latent (14 frames: 14 x 3072 x 320, 14 x 768 x 640, 14 x 192 x 1280) and the sampling
size (28 x 9216 x 320, 28 x 2304 x 640, 28 x 576 x 1280) — in the three variants the blocks use:
  plain   y = norm(x)                                          (gradient of y)
  add     y, s = norm(x + h), x + h                            (gradients of y and s)
  row     y, s, s_pre with a row per frame and ret_pre         (gradients of all three)
each with every gradient asked for and with the norm frozen (x, h, row only), on
  (i)  the HIP route     ops.LAYERNORM_BACKWARD on  (csrc/token_rows.hip + csrc/layernorm_bwd.hip)
  (ii) the PyTorch route the same call with it off (MVI_LN_BWD=0: adds and F.layer_norm under autograd)
alternating in ONE process, device events around each forward + backward, PAIRS pairs per class after warm-up; medians and the
PyTorch route's own spread (slowest - fastest). Also the HIP route's host time per forward + backward (the enqueue, no synchronise
inside), and at the two level-0 shapes the backward launches' own time (hip_ops.PROFILE's events around them) with the fraction of
the HBM peak by algorithmic bytes (every gradient and s read once, gP written once).

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_layernorm_bwd.py [--out profiles/layernorm_bwd_bench.json]
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, ops  # noqa: E402

SHAPES = [(14, 3072, 320), (14, 768, 640), (14, 192, 1280), (28, 9216, 320), (28, 2304, 640), (28, 576, 1280)]
VARIANTS = ("plain", "add", "row")
PAIRS = 9
PEAK_HBM = 8.0e12             # bytes / s of one MI355X (MI355X_MICROARCH.md)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = []
    for _ in range(PAIRS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    return statistics.median(t)


def kernel_ms(fn):
    hip_ops.PROFILE = []
    try:
        for _ in range(PAIRS):
            fn()
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for kind, a, b, _ in hip_ops.PROFILE if kind == "add_layernorm_bwd")
    finally:
        hip_ops.PROFILE = None


def pairs(hip, lib):
    for _ in range(3):
        hip(), lib()
    torch.cuda.synchronize()
    t_hip, t_lib = [], []
    for _ in range(PAIRS):
        t_hip.append(timed(hip))
        t_lib.append(timed(lib))
    row = dict(pairs=PAIRS, hip_fwd_bwd_ms_median=statistics.median(t_hip), pytorch_fwd_bwd_ms_median=statistics.median(t_lib),
               pytorch_spread_ms=max(t_lib) - min(t_lib), hip_spread_ms=max(t_hip) - min(t_hip))
    row["hip_route_wins"] = row["hip_fwd_bwd_ms_median"] < row["pytorch_fwd_bwd_ms_median"] - row["pytorch_spread_ms"]
    return row


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "layernorm_bwd_bench.json")
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    ops.add_layer_norm_backward_pays = lambda *a: True   # measure the HIP route also where the default routing leaves it out
    rows_out = []
    for tag, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        for B, S, C in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(0)
            x, h, gy, gs, gp = (torch.randn(B, S, C, device="cuda", generator=g).to(dtype) for _ in range(5))
            row = torch.randn(B, 1, C, device="cuda", generator=g).to(dtype)
            norm = torch.nn.LayerNorm(C).to("cuda", dtype)
            for variant in VARIANTS:
                for frozen in (False, True):
                    leaves = [x] + ([h] if variant != "plain" else []) + ([row] if variant == "row" else [])

                    def route(on):
                        def run():
                            ops.LAYERNORM_BACKWARD = on
                            norm.requires_grad_(not frozen)
                            for t in leaves:
                                t.requires_grad_(True)
                                t.grad = None
                            norm.weight.grad = norm.bias.grad = None
                            y, s, p = ops.add_layer_norm(x, norm, h=h if variant != "plain" else None, row=row if variant == "row" else None,
                                                         ret_pre=variant == "row")
                            if variant == "plain":
                                y.backward(gy)
                            elif variant == "add":
                                torch.autograd.backward([y, s], [gy, gs])
                            else:
                                torch.autograd.backward([y, s, p], [gy, gs, gp])
                            del ops.FALLBACKS[:]
                        return run
                    r = dict(dtype=tag, B=B, S=S, C=C, variant=variant, gradients="frozen norm" if frozen else "all",
                             **pairs(route(True), route(False)))
                    r["hip_host_ms_median"] = host_ms(route(True))
                    r["pytorch_host_ms_median"] = host_ms(route(False))
                    if C == 320:
                        n_io = {"plain": 3, "add": 4, "row": 5}[variant]          # s, gy (, gs (, gs_pre)) read, gP written
                        k = kernel_ms(route(True))
                        r["hip_backward_launches_ms"] = k
                        r["backward_hbm_fraction_algorithmic"] = n_io * B * S * C * x.element_size() / (k * 1e-3) / PEAK_HBM
                    rows_out.append(r)
                    print(f"{tag} {B} x {S} x {C} {variant} {r['gradients']}: HIP {r['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                          f"{r['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {r['pytorch_spread_ms']:.3f}); host HIP {r['hip_host_ms_median']:.3f} / "
                          f"PyTorch {r['pytorch_host_ms_median']:.3f} ms" +
                          (f"; backward launches {r['hip_backward_launches_ms']:.3f} ms = {r['backward_hbm_fraction_algorithmic']:.2f} of the HBM peak"
                           if C == 320 else "") + f"; wins: {r['hip_route_wins']}", flush=True)
                    for t in leaves:
                        t.requires_grad_(False)
            del x, h, gy, gs, gp, row
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(dict(peak_hbm_bytes_per_s=PEAK_HBM, device=torch.cuda.get_device_name(0), rows=rows_out), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

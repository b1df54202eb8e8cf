"""Forward + backward time of GEGLU under autograd, bf16 and f16, random data:
  fused        ops.linear_geglu at the level-0 width (K = 320, inner = 1280), rows 14 x 3072 (the reference's training latent, 14 frames),
               28 x 3072 and 14 x 9216 (the sampling size), with only x requiring grad (dx only: frozen weights) and with x, weight and
               bias requiring grad;
  elementwise  ops.geglu on an h that requires grad at the (rows, inner) of levels 1 - 3 of the sampling size and of the training
               latent (the projection in front of it is the same library GEMM on both routes and is left out);
each on
  (i)  the HIP route     ops.FF_GEGLU_BACKWARD on  (csrc/ff_geglu.hip + csrc/ff_geglu_bwd.hip; csrc/geglu.hip)
  (ii) the PyTorch route the same call with it off (MVI_FF_GEGLU_BWD=0: F.linear, chunk, gelu, mul under autograd)
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and the
PyTorch route's own spread (slowest - fastest). Also the fused backward kernel's own time (dx only, hip_ops.PROFILE's events around the
launch) and its fraction of the MFMA peak,
counting the 2 products it executes (recomputation and contraction).

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_geglu_bwd.py [--out profiles/geglu_bwd_bench.json]
       [--dtypes f16,bf16]   the order in which the types are measured (default bf16,f16): what is measured first in a process pays the
                             libraries' first calls in its warm-up
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, ops  # noqa: E402

FUSED = [(14 * 3072, 320, 1280), (28 * 3072, 320, 1280), (14 * 9216, 320, 1280)]
ELEMENTWISE = [(14 * 2304, 2560), (14 * 576, 5120), (14 * 144, 5120), (14 * 768, 2560), (14 * 192, 5120), (14 * 48, 5120)]
PAIRS = 9
PEAK_TFLOPS = 2500.0          # dense bf16 / f16 MFMA peak of one MI355X (MI355X_MICROARCH.md)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def kernel_ms(fn):
    """Median time of the ff_geglu_bwd kernel alone, from hip_ops.PROFILE's device events around the launch (no allocation, no
    wrapper)."""
    for _ in range(3):
        fn()
    hip_ops.PROFILE = []
    try:
        for _ in range(PAIRS):
            fn()
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for kind, a, b, _ in hip_ops.PROFILE if kind == "ff_geglu_bwd")
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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "geglu_bwd_bench.json")
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    rows_out = []

    def lifted(on):                                      # measure the HIP route also where the default routing leaves it out
        ops.FF_GEGLU_BACKWARD = on
        ops.linear_geglu_backward_pays = ops.geglu_backward_pays = lambda *a: True

    order = sys.argv[sys.argv.index("--dtypes") + 1].split(",") if "--dtypes" in sys.argv else ["bf16", "f16"]
    for dtype, tag in (({"bf16": torch.bfloat16, "f16": torch.float16}[t], t) for t in order):
        for rows, K, inner in FUSED:
            g = torch.Generator(device="cuda").manual_seed(0)
            x = torch.randn(rows, K, device="cuda", generator=g).to(dtype).requires_grad_()
            w = (torch.randn(2 * inner, K, device="cuda", generator=g) / K ** 0.5).to(dtype).requires_grad_()
            b = torch.randn(2 * inner, device="cuda", generator=g).to(dtype).requires_grad_()
            dy = torch.randn(rows, inner, device="cuda", generator=g).to(dtype)
            kern = kernel_ms(lambda: hip_ops.ff_geglu_backward(x.detach(), w.detach(), b.detach(), dy, need_dparams=False))
            for need_dparams in (False, True):
                def route(on):
                    def run():
                        lifted(on)
                        w.requires_grad_(need_dparams), b.requires_grad_(need_dparams)
                        x.grad = w.grad = b.grad = None
                        ops.linear_geglu(x, w, b).backward(dy)
                    return run
                row = dict(path="fused", dtype=tag, rows=rows, K=K, inner=inner, gradients="all" if need_dparams else "dx", **pairs(route(True), route(False)))
                row["hip_backward_kernel_dx_only_ms"] = kern
                row["backward_mfma_fraction_2_products"] = 2 * (2.0 * rows * K * 2 * inner) / (kern * 1e-3) / (PEAK_TFLOPS * 1e12)
                rows_out.append(row)
                print(f"fused {tag} rows {rows} {row['gradients']}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                      f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); backward kernel {kern:.3f} ms = "
                      f"{row['backward_mfma_fraction_2_products']:.3f} of peak; wins: {row['hip_route_wins']}", flush=True)
            del x, w, b, dy
        for rows, inner in ELEMENTWISE:
            g = torch.Generator(device="cuda").manual_seed(0)
            h = torch.randn(rows, 2 * inner, device="cuda", generator=g).to(dtype).requires_grad_()
            dy = torch.randn(rows, inner, device="cuda", generator=g).to(dtype)

            def route(on):
                def run():
                    lifted(on)
                    h.grad = None
                    ops.geglu(h).backward(dy)
                return run
            row = dict(path="elementwise", dtype=tag, rows=rows, inner=inner, **pairs(route(True), route(False)))
            rows_out.append(row)
            print(f"elementwise {tag} rows {rows} inner {inner}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                  f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); wins: {row['hip_route_wins']}", flush=True)
            del h, dy
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(dict(peak_tflops=PEAK_TFLOPS, dtype_order=order, device=torch.cuda.get_device_name(0), rows=rows_out), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""Forward + backward time of the four leading conv + SiLU layers of ControlNet.input_hint_block under autograd, bf16 and f16, random data:
7 -> 16 and 16 -> 16 at 14 x 576x1024, 16 -> 32 with stride 2 from 576x1024, 32 -> 32 at 14 x 288x512 (the workload's sizes), the same at
half the hint's height and width, and the four-layer prefix as a whole with torch.cuda.max_memory_allocated of each route. Each on
  (i)  the HIP route      ops.stem_conv3x3_silu (csrc/stem_conv.hip forward, dz epilogue and stride-1 dgrad, csrc/stem_conv_bwd.hip)
  (ii) the PyTorch route  F.silu(F.conv2d(...)) under autograd, what the training path runs today
alternating in ONE process, device events around each forward + backward, PAIRS pairs per class after warm-up; medians and each route's
spread (slowest - fastest). A class wins where the HIP median beats the PyTorch median by more than the PyTorch route's spread. Every
parameter requires grad; the input requires grad except in the first layer (the hint needs none). Also the HIP backward passes' own
times (hip_ops.PROFILE's events around each launch) beside the bytes they have to move.

Usage (GPU box, under its own time limit):  timeout -k 10 900 python tools/bench_stem_bwd.py [--out profiles/stem_bwd_bench.json]
       [--dtypes f16,bf16]   the order in which the types are measured (default bf16,f16)
"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, ops  # noqa: E402

# (C_in, C_out, stride, the input requires grad, divisor of the hint's size at the layer's input)
LAYERS = [(7, 16, 1, False, 1), (16, 16, 1, True, 1), (16, 32, 2, True, 1), (32, 32, 1, True, 2)]
HINT = (14, 576, 1024)
SCALES = (1, 2)               # the workload's hint, and half its height and width
PAIRS = 9
KINDS = ("stem_conv", "stem_conv_dz", "stem_conv_wgrad", "stem_conv_dgrad")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


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


def kernel_ms(fn):
    """Median time of each HIP launch kind over PAIRS runs of fn (events around the launch)."""
    hip_ops.PROFILE = []
    try:
        for _ in range(PAIRS):
            fn()
        torch.cuda.synchronize()
        return {k: statistics.median(a.elapsed_time(b) for kk, a, b, _ in hip_ops.PROFILE if kk == k)
                for k in KINDS if any(p[0] == k for p in hip_ops.PROFILE)}
    finally:
        hip_ops.PROFILE = None


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def make(N, Ci, Co, H, W, stride, need_dx, dtype, g):
    x = torch.randn(N, Ci, H, W, device="cuda", generator=g).to(dtype).requires_grad_(need_dx)
    w = (torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) / (9 * Ci) ** 0.5).to(dtype).requires_grad_()
    b = (0.3 * torch.randn(Co, device="cuda", generator=g)).to(dtype).requires_grad_()
    dy = torch.randn(N, Co, (H - 1) // stride + 1, (W - 1) // stride + 1, device="cuda", generator=g).to(dtype)
    return x, w, b, dy


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "stem_bwd_bench.json")
    ops.STRICT = False
    ops.stem_conv_backward_pays = lambda *a, **k: True   # measure the HIP route whatever the committed routing says
    order = sys.argv[sys.argv.index("--dtypes") + 1].split(",") if "--dtypes" in sys.argv else ["bf16", "f16"]
    rows_out = []

    def dump():                                          # after every class: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(dict(dtype_order=order, device=torch.cuda.get_device_name(0), rows=rows_out), fh, indent=1)
            fh.write("\n")

    N, H0, W0 = HINT
    for dtype, tag in (({"bf16": torch.bfloat16, "f16": torch.float16}[t], t) for t in order):
        for scale in SCALES:
            for Ci, Co, stride, need_dx, div in LAYERS:
                H, W = H0 // (scale * div), W0 // (scale * div)
                g = torch.Generator(device="cuda").manual_seed(0)
                x, w, b, dy = make(N, Ci, Co, H, W, stride, need_dx, dtype, g)
                assert ops.stem_conv_gates(N, Ci, Co, H, W, stride, dtype, need_dx)

                def hip():
                    x.grad = w.grad = b.grad = None
                    ops.stem_conv3x3_silu(x, w, b, silu=True, stride=stride).backward(dy)

                def lib():
                    x.grad = w.grad = b.grad = None
                    F.silu(F.conv2d(x, w, b, stride, 1)).backward(dy)
                row = dict(path="layer", dtype=tag, N=N, H=H, W=W, C_in=Ci, C_out=Co, stride=stride, input_gradient=need_dx, **pairs(hip, lib))
                row["hip_launch_ms"] = kernel_ms(hip)
                e = x.element_size()
                row["bytes_dz_pass"] = (x.numel() + 2 * dy.numel()) * e
                row["bytes_wgrad"] = (x.numel() + dy.numel()) * e
                row["bytes_dgrad"] = 2 * dy.numel() * e if need_dx and stride == 1 else 0
                row["wgrad_workspace_bytes"] = hip_ops.stem_conv3x3_wgrad_workspace_bytes(N, Ci, Co, H, W, stride)
                rows_out.append(row)
                print(f"layer {tag} {N}x{H}x{W} {Ci}->{Co} s{stride}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                      f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); launches "
                      f"{ {k: round(v, 3) for k, v in row['hip_launch_ms'].items()} }; wins: {row['hip_route_wins']}", flush=True)
                del x, w, b, dy
                dump()

            # the four-layer prefix: time and peak memory of each route
            H, W = H0 // scale, W0 // scale
            g = torch.Generator(device="cuda").manual_seed(1)
            hint = torch.randn(N, 7, H, W, device="cuda", generator=g).to(dtype)
            params = [make(1, Ci, Co, 8, 16, stride, False, dtype, g)[1:3] for Ci, Co, stride, _, _ in LAYERS]
            dy = torch.randn(N, 32, H // 2, W // 2, device="cuda", generator=g).to(dtype)

            def prefix(layer):
                def run():
                    for w, b in params:
                        w.grad = b.grad = None
                    h = hint
                    for (w, b), (_, _, stride, _, _) in zip(params, LAYERS):
                        h = layer(h, w, b, stride)
                    h.backward(dy)
                return run
            hip = prefix(lambda h, w, b, s: ops.stem_conv3x3_silu(h, w, b, silu=True, stride=s))
            lib = prefix(lambda h, w, b, s: F.silu(F.conv2d(h, w, b, s, 1)))
            row = dict(path="prefix", dtype=tag, N=N, H=H, W=W, **pairs(hip, lib))
            row["hip_peak_bytes"], row["pytorch_peak_bytes"] = peak_bytes(hip), peak_bytes(lib)
            rows_out.append(row)
            print(f"prefix {tag} {N}x{H}x{W}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch {row['pytorch_fwd_bwd_ms_median']:.3f} ms "
                  f"(spread {row['pytorch_spread_ms']:.3f}); peak memory HIP {row['hip_peak_bytes'] / 2 ** 20:.0f} MiB, PyTorch "
                  f"{row['pytorch_peak_bytes'] / 2 ** 20:.0f} MiB; wins: {row['hip_route_wins']}", flush=True)
            del hint, params, dy
            dump()


if __name__ == "__main__":
    main()

"""Forward + backward time of the 3x3 / padding 1 / stride 1 convolution under autograd, bf16 and f16, random data, at the shapes of the
14-frame 64 x 48 training latent and its CFG pair — (N, H, W, C_in, C_out) for N in {14, 28} at (48, 64, 320, 320), (48, 64, 640, 320),
(24, 32, 640, 640), (24, 32, 1280, 640), (12, 16, 1280, 1280), (12, 16, 2560, 1280), (6, 8, 1280, 1280) — with only the input
requiring grad (dx only: frozen weights) and with input and weight requiring grad, each on
  (i)  the HIP route      ops.conv3x3_tokens on token-major tensors (csrc/linear_n320.hip forward and dgrad, csrc/conv3x3_wgrad.hip)
  (ii) the PyTorch route  F.conv2d under autograd on the NCHW planes the training path hands it today (layers.conv_no_bias)
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and the PyTorch
route's own spread (slowest - fastest). A class wins where the HIP median beats the PyTorch median by more than that spread. Also the
wgrad kernel's own time (hip_ops.PROFILE's events around the launch) and its fraction of the MFMA peak, and one ResBlock line:
layers.ResBlock(320, 1280, 0.0, out_channels=320), 14 x 320 x 48x64, bf16, forward + backward with every parameter trainable, with
layers.RESBLOCK_CONV_BWD on and off.

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_conv_bwd.py [--out profiles/conv3x3_bwd_bench.json]
       [--dtypes f16,bf16]   the order in which the types are measured (default bf16,f16)
"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, layers, ops  # noqa: E402

SHAPES = [(48, 64, 320, 320), (48, 64, 640, 320), (24, 32, 640, 640), (24, 32, 1280, 640), (12, 16, 1280, 1280), (12, 16, 2560, 1280),
          (6, 8, 1280, 1280)]
BATCHES = (14, 28)
PAIRS = 9
PEAK_TFLOPS = 2500.0          # dense bf16 / f16 MFMA peak of one MI355X (MI355X_MICROARCH.md)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def kernel_ms(fn, kind):
    for _ in range(3):
        fn()
    hip_ops.PROFILE = []
    try:
        for _ in range(PAIRS):
            fn()
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for k, a, b, _ in hip_ops.PROFILE if k == kind)
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


def resblock_line():
    dt = torch.bfloat16
    torch.manual_seed(0)
    m = layers.ResBlock(320, 1280, 0.0, out_channels=320)
    with torch.no_grad():
        for p in m.out_layers[3].parameters():               # (zero_module: give the last convolution real weights)
            p.copy_(torch.randn(p.shape) / 54)
    m = m.to("cuda", dt)
    x = torch.randn(14, 320, 48, 64, device="cuda").to(dt).requires_grad_()
    emb = torch.randn(14, 1280, device="cuda").to(dt)
    dy = torch.randn(14, 320, 48, 64, device="cuda").to(dt)

    def route(on):
        def run():
            layers.RESBLOCK_CONV_BWD = on
            ops.CONV3X3_BACKWARD = on
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x, emb).backward(dy)
        return run
    row = dict(path="resblock", dtype="bf16", N=14, H=48, W=64, C_in=320, C_out=320, gradients="all", **pairs(route(True), route(False)))
    layers.RESBLOCK_CONV_BWD = False
    ops.CONV3X3_BACKWARD = True
    return row


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "conv3x3_bwd_bench.json")
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    ops.conv3x3_backward_pays = lambda *a: True          # measure the HIP route also where the default routing leaves it out
    ops.group_norm_backward_pays = lambda *a, **k: True  # (the ResBlock line: both routes on the HIP norms)
    rows_out = []

    def dump():                                          # after every shape: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(dict(peak_tflops=PEAK_TFLOPS, dtype_order=order, device=torch.cuda.get_device_name(0), rows=rows_out), fh, indent=1)
            fh.write("\n")
    order = sys.argv[sys.argv.index("--dtypes") + 1].split(",") if "--dtypes" in sys.argv else ["bf16", "f16"]
    for dtype, tag in (({"bf16": torch.bfloat16, "f16": torch.float16}[t], t) for t in order):
        for N in BATCHES:
            for H, W, Ci, Co in SHAPES:
                if not ops.conv3x3_tokens_gates(N, H, W, Ci, Co, dtype):
                    rows_out.append(dict(path="conv", dtype=tag, N=N, H=H, W=W, C_in=Ci, C_out=Co, gated_out=True))
                    print(f"conv {tag} {N}x{H}x{W} {Ci}->{Co}: outside the kernels' gates", flush=True)
                    continue
                g = torch.Generator(device="cuda").manual_seed(0)
                tok = torch.randn(N, H * W, Ci, device="cuda", generator=g).to(dtype).requires_grad_()
                dy = torch.randn(N, H * W, Co, device="cuda", generator=g).to(dtype)
                w = (torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) / (9 * Ci) ** 0.5).to(dtype).requires_grad_()
                xp = tok.detach().view(N, H, W, Ci).permute(0, 3, 1, 2).contiguous().requires_grad_()      # NCHW planes, as today
                dyp = dy.view(N, H, W, Co).permute(0, 3, 1, 2).contiguous()
                kern = kernel_ms(lambda: hip_ops.conv3x3_wgrad(tok.detach(), dy, H, W), "conv3x3_wgrad")
                flops = 2.0 * N * H * W * 9 * Ci * Co
                for need_dw in (False, True):
                    def hip():
                        w.requires_grad_(need_dw)
                        tok.grad = w.grad = None
                        ops.conv3x3_tokens(tok, w, H, W).backward(dy)

                    def lib():
                        w.requires_grad_(need_dw)
                        xp.grad = w.grad = None
                        F.conv2d(xp, w, None, 1, 1).backward(dyp)
                    row = dict(path="conv", dtype=tag, N=N, H=H, W=W, C_in=Ci, C_out=Co, gradients="all" if need_dw else "dx", **pairs(hip, lib))
                    row["wgrad_kernel_ms"] = kern
                    row["wgrad_mfma_fraction"] = flops / (kern * 1e-3) / (PEAK_TFLOPS * 1e12)
                    row["wgrad_split_workspace_bytes"] = hip_ops.conv3x3_wgrad_workspace_bytes(N, H, W, Ci, Co)
                    rows_out.append(row)
                    print(f"conv {tag} {N}x{H}x{W} {Ci}->{Co} {row['gradients']}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                          f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); wgrad kernel {kern:.3f} ms = "
                          f"{row['wgrad_mfma_fraction']:.3f} of peak; wins: {row['hip_route_wins']}", flush=True)
                del tok, dy, w, xp, dyp
                dump()
    row = resblock_line()
    rows_out.append(row)
    print(f"ResBlock 320 14x48x64 bf16 all gradients: conv backward on HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, parent route "
          f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); wins: {row['hip_route_wins']}", flush=True)
    dump()

if __name__ == "__main__":
    main()

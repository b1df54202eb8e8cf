"""Forward + backward time of the (3, 1, 1) / padding (1, 0, 0) frame convolution of VideoResBlock.time_stack under autograd, bf16 and
f16, random data, at the time-stack shapes of the 14-frame 512 x 384 training clip (48 x 64 latents) — (B, T, S, C) = (1, 14, 3072, 320),
(1, 14, 768, 640), (1, 14, 192, 1280), (1, 14, 48, 1280), C -> C — with only the input requiring grad (dx only: frozen weights) and with
input and weight requiring grad, each on
  (i)  the HIP route      ops.conv3t_tokens on token-major tensors (csrc/linear_n320.hip forward and dgrad, csrc/conv3t_wgrad.hip)
  (ii) the PyTorch route  layers.temporal_conv3_stacked under autograd on an ALREADY channel-stacked [(b T), 3 C, h, w] input, what the
                          training path runs today (the cost of writing the stack and of its gradient is left out: that favours PyTorch)
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and the PyTorch
route's own spread (slowest - fastest). A class wins where the HIP median beats the PyTorch median by more than that spread. Also the
wgrad kernel's own time (hip_ops.PROFILE's events around the launch) and its fraction of the MFMA peak, and one block line:
layers.VideoResBlock(320, 1280, 0.0, out_channels=320) in the networks' configuration, 14 x 320 x 48x64, bf16, forward + backward with
every parameter trainable, with layers.TIME_STACK_CONV_BWD on and off — once with the default routing of the time stack's token-major
norms (ops.group_norm_tok2tok's PyTorch fallback under autograd) and once with their HIP backward taken.

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_conv3t_bwd.py [--out profiles/conv3t_bwd_bench.json]
       [--dtypes f16,bf16]   the order in which the types are measured (default bf16,f16)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, layers, ops  # noqa: E402

SHAPES = [(1, 14, 3072, 320), (1, 14, 768, 640), (1, 14, 192, 1280), (1, 14, 48, 1280)]          # (B, T, S, C)
HW = {3072: (48, 64), 768: (24, 32), 192: (12, 16), 48: (6, 8)}
PAIRS = 9
PEAK_TFLOPS = 2500.0          # dense bf16 / f16 MFMA peak of one MI355X


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


def block_line(hip_norms):
    """hip_norms: ops.group_norm_tok2tok's HIP backward taken for the time stack's norms (its own speed decision lifted) instead of its
    differentiable PyTorch fallback, which is what the default routing gives the token route today."""
    dt = torch.bfloat16
    T = 14
    torch.manual_seed(0)
    m = layers.VideoResBlock(320, 1280, 0.0, video_kernel_size=[3, 1, 1], out_channels=320, merge_strategy="learned_with_images", merge_factor=0.5)
    with torch.no_grad():
        for blk in (m, m.time_stack):                        # (zero_module: give the last convolutions real weights)
            for p in blk.out_layers[3].parameters():
                p.copy_(torch.randn(p.shape) / 54)
    m = m.to("cuda", dt)
    x = torch.randn(T, 320, 48, 64, device="cuda").to(dt).requires_grad_()
    emb = torch.randn(T, 1280, device="cuda").to(dt)
    ind = torch.zeros(1, T, device="cuda")
    dy = torch.randn(T, 320, 48, 64, device="cuda").to(dt)

    def route(on):
        def run():
            layers.TIME_STACK_CONV_BWD = on
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x, emb, T, ind).backward(dy)
        return run
    keep = ops.group_norm_tok2tok_backward_pays
    if hip_norms:
        ops.group_norm_tok2tok_backward_pays = lambda *a, **k: True
    try:
        row = dict(path="video_resblock_hip_norms" if hip_norms else "video_resblock", dtype="bf16", B=1, T=T, S=3072, C_in=320, C_out=320,
                   gradients="all", **pairs(route(True), route(False)))
    finally:
        ops.group_norm_tok2tok_backward_pays = keep
        layers.TIME_STACK_CONV_BWD = False
    return row


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "conv3t_bwd_bench.json")
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    ops.conv3t_backward_pays = lambda *a: True           # measure the HIP route also where the default routing leaves it out
    ops.group_norm_backward_pays = lambda *a, **k: True  # (the block line: both routes on the HIP norms they can reach)
    rows_out = []

    def dump():                                          # after every shape: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(dict(peak_tflops=PEAK_TFLOPS, dtype_order=order, device=torch.cuda.get_device_name(0), rows=rows_out), fh, indent=1)
            fh.write("\n")
    order = sys.argv[sys.argv.index("--dtypes") + 1].split(",") if "--dtypes" in sys.argv else ["bf16", "f16"]
    for dtype, tag in (({"bf16": torch.bfloat16, "f16": torch.float16}[t], t) for t in order):
        for B, T, S, C in SHAPES:
            if not ops.conv3t_tokens_gates(B, T, S, C, C, dtype):
                rows_out.append(dict(path="conv", dtype=tag, B=B, T=T, S=S, C_in=C, C_out=C, gated_out=True))
                print(f"conv3t {tag} {B}x{T}x{S} {C}->{C}: outside the kernels' gates", flush=True)
                continue
            h, w_ = HW[S]
            g = torch.Generator(device="cuda").manual_seed(0)
            tok = torch.randn(B * T, S, C, device="cuda", generator=g).to(dtype).requires_grad_()
            dy = torch.randn(B * T, S, C, device="cuda", generator=g).to(dtype)
            conv = torch.nn.Conv3d(C, C, (3, 1, 1), padding=(1, 0, 0)).to("cuda", dtype)
            w = conv.weight
            x3 = torch.randn(B * T, 3 * C, h, w_, device="cuda", generator=g).to(dtype).requires_grad_()      # the stacked planes, as today
            dyp = dy.view(B * T, h, w_, C).permute(0, 3, 1, 2).contiguous()
            kern = kernel_ms(lambda: hip_ops.conv3t_wgrad(tok.detach(), dy, T), "conv3t_wgrad")
            flops = 2.0 * B * T * S * 3 * C * C
            for need_dw in (False, True):
                def hip():
                    w.requires_grad_(need_dw)
                    tok.grad = w.grad = None
                    ops.conv3t_tokens(tok, w, T).backward(dy)

                def lib():
                    w.requires_grad_(need_dw)
                    x3.grad = w.grad = None
                    layers.temporal_conv3_stacked(x3, conv, with_bias=False).backward(dyp)
                row = dict(path="conv", dtype=tag, B=B, T=T, S=S, C_in=C, C_out=C, gradients="all" if need_dw else "dx", **pairs(hip, lib))
                row["wgrad_kernel_ms"] = kern
                row["wgrad_mfma_fraction"] = flops / (kern * 1e-3) / (PEAK_TFLOPS * 1e12)
                row["wgrad_split_workspace_bytes"] = hip_ops.conv3t_wgrad_workspace_bytes(B, T, S, C, C)
                rows_out.append(row)
                print(f"conv3t {tag} {B}x{T}x{S} {C}->{C} {row['gradients']}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                      f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); wgrad kernel {kern:.3f} ms = "
                      f"{row['wgrad_mfma_fraction']:.3f} of peak; wins: {row['hip_route_wins']}", flush=True)
            del tok, dy, conv, w, x3, dyp
            dump()
    for hip_norms in (False, True):
        row = block_line(hip_norms)
        rows_out.append(row)
        print(f"VideoResBlock 320 14x48x64 bf16 all gradients ({row['path']}): time stack on tokens {row['hip_fwd_bwd_ms_median']:.3f} ms, "
              f"parent route {row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); wins: {row['hip_route_wins']}",
              flush=True)
        dump()


if __name__ == "__main__":
    main()

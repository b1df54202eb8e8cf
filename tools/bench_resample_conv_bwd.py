"""Forward + backward time of the two resampling 3x3 convolutions under autograd, bf16 and f16, random data, at the shapes a ControlNet training
step crosses — N in {14, 28}, C -> C at (H, W, C) = (72, 128, 320), (36, 64, 640), (18, 32, 1280): the Downsample's INPUT size (stride 2,
with only the input requiring grad and with input, weight and bias requiring grad) and the Upsample's OUTPUT size (frozen weight: dx only)
— each on
  (i)  the HIP route      ops.conv3x3_down_tokens / ops.conv3x3_up_tokens on token-major tensors (csrc/linear_n320.hip forward and input
                          gradient, csrc/conv3x3_wgrad.hip's stride-2 form, csrc/token_rows.hip's 2x2 pooling pass)
  (ii) the PyTorch route  F.conv2d(stride 2) / F.conv2d(F.interpolate(x)) under autograd on the NCHW planes the training path hands it today
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and the PyTorch
route's own spread (slowest - fastest). A class wins where the HIP median beats the PyTorch median by more than that spread. Also the
stride-2 wgrad kernel's own time (hip_ops.PROFILE's events around the launch) and its fraction of the MFMA peak (useful FLOPs: the zeros
of the zero-stuffed dy are not counted), the module lines — layers.Downsample(C, True) trainable / layers.Upsample(C, True) frozen on NCHW
planes, N = 14, bf16, with layers.RESAMPLE_CONV_BWD on and off (the layout copies around the op included) — and with every Upsample line the peak
memory of forward + backward with the route on and off, that of Upsample(1280) at 18x32 -> 36x64, N = 14, among them
(--memory-line-only: measure that last line alone and append it to the file named by --out).

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_resample_conv_bwd.py [--out profiles/resample_conv_bwd_bench.json]
"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, layers, ops  # noqa: E402

SHAPES = [(72, 128, 320), (36, 64, 640), (18, 32, 1280)]
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


def say(row, what):
    print(f"{what}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch {row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread "
          f"{row['pytorch_spread_ms']:.3f}); wins: {row['hip_route_wins']}", flush=True)


def down_rows(tag, dtype, N, H, W, C):
    g = torch.Generator(device="cuda").manual_seed(0)
    Ho, Wo = H // 2, W // 2
    tok = torch.randn(N, H * W, C, device="cuda", generator=g).to(dtype).requires_grad_()
    dy = torch.randn(N, Ho * Wo, C, device="cuda", generator=g).to(dtype)
    w = (torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5).to(dtype).requires_grad_()
    b = (0.1 * torch.randn(C, device="cuda", generator=g)).to(dtype).requires_grad_()
    xp = tok.detach().view(N, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_()      # NCHW planes, as today
    dyp = dy.view(N, Ho, Wo, C).permute(0, 3, 1, 2).contiguous()
    kern = kernel_ms(lambda: hip_ops.conv3x3_s2_wgrad(tok.detach(), dy, H, W), "conv3x3_s2_wgrad")
    flops = 2.0 * N * Ho * Wo * 9 * C * C
    out = []
    for need_dw in (False, True):
        def hip():
            w.requires_grad_(need_dw), b.requires_grad_(need_dw)
            tok.grad = w.grad = b.grad = None
            ops.conv3x3_down_tokens(tok, w, b, H, W).backward(dy)

        def lib():
            w.requires_grad_(need_dw), b.requires_grad_(need_dw)
            xp.grad = w.grad = b.grad = None
            F.conv2d(xp, w, b, 2, 1).backward(dyp)
        row = dict(path="down", dtype=tag, N=N, H=H, W=W, C_in=C, C_out=C, gradients="all" if need_dw else "dx", **pairs(hip, lib))
        row["wgrad_kernel_ms"] = kern
        row["wgrad_mfma_fraction"] = flops / (kern * 1e-3) / (PEAK_TFLOPS * 1e12)
        row["wgrad_split_workspace_bytes"] = hip_ops.conv3x3_s2_wgrad_workspace_bytes(N, H, W, C, C)
        out.append(row)
        say(row, f"down {tag} {N}x{H}x{W} {C}->{C} {row['gradients']} (s2 wgrad kernel {kern:.3f} ms = {row['wgrad_mfma_fraction']:.3f} of peak)")
    return out


def up_row(tag, dtype, N, H, W, C):
    g = torch.Generator(device="cuda").manual_seed(0)
    h, w_ = H // 2, W // 2
    tok = torch.randn(N, h * w_, C, device="cuda", generator=g).to(dtype).requires_grad_()
    dy = torch.randn(N, H * W, C, device="cuda", generator=g).to(dtype)
    w = (torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5).to(dtype)
    b = (0.1 * torch.randn(C, device="cuda", generator=g)).to(dtype)
    xp = tok.detach().view(N, h, w_, C).permute(0, 3, 1, 2).contiguous().requires_grad_()
    dyp = dy.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()

    def hip():
        tok.grad = None
        ops.conv3x3_up_tokens(tok, w, b, h, w_).backward(dy)

    def lib():
        xp.grad = None
        F.conv2d(F.interpolate(xp, scale_factor=2, mode="nearest"), w, b, 1, 1).backward(dyp)
    row = dict(path="up", dtype=tag, N=N, H=H, W=W, C_in=C, C_out=C, gradients="dx", **pairs(hip, lib))
    say(row, f"up   {tag} {N}x{h}x{w_}->{H}x{W} {C}->{C} dx")
    return row


def module_line(which, H, W, C, N=14):
    dt = torch.bfloat16
    down = which == "Downsample"
    torch.manual_seed(0)
    m = (layers.Downsample if down else layers.Upsample)(C, True).to("cuda", dt).requires_grad_(down)
    hin, win = (H, W) if down else (H // 2, W // 2)
    hout, wout = (H // 2, W // 2) if down else (H, W)
    x = torch.randn(N, C, hin, win, device="cuda").to(dt).requires_grad_()
    dy = torch.randn(N, C, hout, wout, device="cuda").to(dt)

    def route(on):
        def run():
            layers.RESAMPLE_CONV_BWD = on
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x).backward(dy)
        return run
    row = dict(path="module " + which, dtype="bf16", N=N, H=H, W=W, C_in=C, C_out=C, gradients="all" if down else "dx",
               **pairs(route(True), route(False)))
    if not down:                                                 # peak memory of forward + backward over what is held before it
        for on in (True, False):
            route(on)()
            torch.cuda.synchronize()
            x.grad = None
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            route(on)()
            torch.cuda.synchronize()
            row["peak_bytes_over_base_route_" + ("on" if on else "off")] = torch.cuda.max_memory_allocated() - base
        row["upsampled_tensor_bytes"] = N * C * H * W * 2
    layers.RESAMPLE_CONV_BWD = False
    say(row, f"module {which} bf16 {N}x{H}x{W} {C}" + ("" if down else f" peak bytes on/off {row['peak_bytes_over_base_route_on']}/"
                                                         f"{row['peak_bytes_over_base_route_off']} (4x tensor {row['upsampled_tensor_bytes']})"))
    return row


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "resample_conv_bwd_bench.json")
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    ops.conv3x3_down_backward_pays = lambda *a: True     # measure the HIP route also where the default routing leaves it out
    ops.conv3x3_up_backward_pays = lambda *a: True
    layers.resample_conv_module_pays = lambda *a: True
    rows_out = []
    if "--memory-line-only" in sys.argv:                 # append the 1280-channel Upsample line to an existing file
        with open(out_path) as fh:
            old = json.load(fh)
        old["rows"] = [r for r in old["rows"] if not (r["path"] == "module Upsample" and (r["H"], r["C_in"]) == (36, 1280))]
        old["rows"].append(module_line("Upsample", 36, 64, 1280))
        with open(out_path, "w") as fh:
            json.dump(old, fh, indent=1)
            fh.write("\n")
        return

    def dump():                                          # after every shape: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(dict(peak_tflops=PEAK_TFLOPS, device=torch.cuda.get_device_name(0), rows=rows_out), fh, indent=1)
            fh.write("\n")
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        for N in BATCHES:
            for H, W, C in SHAPES:
                if ops.conv3x3_down_tokens_gates(N, H, W, C, C, dtype):
                    rows_out += down_rows(tag, dtype, N, H, W, C)
                else:
                    rows_out.append(dict(path="down", dtype=tag, N=N, H=H, W=W, C_in=C, C_out=C, gated_out=True))
                if ops.conv3x3_up_tokens_gates(N, H // 2, W // 2, C, C, dtype):
                    rows_out.append(up_row(tag, dtype, N, H, W, C))
                else:
                    rows_out.append(dict(path="up", dtype=tag, N=N, H=H, W=W, C_in=C, C_out=C, gated_out=True))
                dump()
    for H, W, C in SHAPES:
        for which in ("Downsample", "Upsample"):
            rows_out.append(module_line(which, H, W, C))
            dump()
    rows_out.append(module_line("Upsample", 36, 64, 1280))       # the UNet decoder's 1280-channel Upsample, 18x32 -> 36x64: its peak memory
    dump()
    assert not [f for f in ops.FALLBACKS if f[0].startswith("conv3x3_")], "the HIP side of a pair took the PyTorch substitute"


if __name__ == "__main__":
    main()

"""Forward + backward time of the transformer projections (ops.linear) under autograd, bf16 and f16, random data, at the shapes of the
14-frame 64 x 48 training latent and its CFG pair — rows = 14 and 28 x {9216, 2304, 576} tokens, each token count with the (N, K)
pairs of its level: (320, 320), (960, 320), (320, 1280) | (640, 640), (1920, 640), (640, 2560) | (1280, 1280), (3840, 1280),
(1280, 5120) — with only the input requiring grad (dx only: frozen weights) and with input, weight and bias requiring grad, each on
  (i)  the HIP route      ops.linear with ops.LINEAR_BACKWARD on (forward and dgrad on csrc/linear_n320.hip / csrc/ff_geglu.hip's
                          plain epilogue, weight + bias gradient on csrc/linear_wgrad.hip)
  (ii) the PyTorch route  F.linear under autograd: what ops.linear runs with the switch off
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and the PyTorch
route's own spread (slowest - fastest). A class wins where the HIP median beats the PyTorch median by more than that spread. A shape
outside ops.linear_gates (the forward itself is the library's there) is listed as gated out. For every shape, gated or not: the wgrad
kernel's own time (hip_ops.PROFILE's events around the launch) and its fraction of the MFMA peak.

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_linear_bwd.py [--out profiles/linear_bwd_bench.json]
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

LEVELS = [(9216, [(320, 320), (960, 320), (320, 1280)]), (2304, [(640, 640), (1920, 640), (640, 2560)]),
          (576, [(1280, 1280), (3840, 1280), (1280, 5120)])]          # tokens per frame, (N, K) pairs
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


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "linear_bwd_bench.json")
    ops.STRICT = False
    ops.LINEAR_BACKWARD = True
    ops.linear_backward_pays = lambda *a: True           # measure the HIP route also where the default routing leaves it out
    rows_out = []
    order = sys.argv[sys.argv.index("--dtypes") + 1].split(",") if "--dtypes" in sys.argv else ["bf16", "f16"]

    def dump():                                          # after every shape: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(dict(peak_tflops=PEAK_TFLOPS, dtype_order=order, device=torch.cuda.get_device_name(0), rows=rows_out), fh, indent=1)
            fh.write("\n")
    for dtype, tag in (({"bf16": torch.bfloat16, "f16": torch.float16}[t], t) for t in order):
        for B in BATCHES:
            for tokens, nk in LEVELS:
                rows = B * tokens
                for N, K in nk:
                    g = torch.Generator(device="cuda").manual_seed(0)
                    x = torch.randn(B, tokens, K, device="cuda", generator=g).to(dtype).requires_grad_()
                    dy = torch.randn(B, tokens, N, device="cuda", generator=g).to(dtype)
                    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(dtype).requires_grad_()
                    b = (torch.randn(N, device="cuda", generator=g) * 0.3).to(dtype).requires_grad_()
                    kern = kernel_ms(lambda: hip_ops.linear_wgrad(x.detach(), dy, True), "linear_wgrad")
                    base = dict(path="linear", dtype=tag, rows=rows, N=N, K=K, wgrad_kernel_ms=kern,
                                wgrad_mfma_fraction=2.0 * rows * K * N / (kern * 1e-3) / (PEAK_TFLOPS * 1e12),
                                wgrad_split_workspace_bytes=hip_ops.linear_wgrad_workspace_bytes(rows, K, N))
                    if not ops.linear_gates(rows, K, N, dtype):
                        rows_out.append(dict(base, gated_out=True))
                        print(f"linear {tag} {rows} x {K} -> {N}: outside ops.linear_gates; wgrad kernel {kern:.3f} ms = "
                              f"{base['wgrad_mfma_fraction']:.3f} of peak", flush=True)
                        continue
                    for need_dp in (False, True):
                        def run(fn):
                            w.requires_grad_(need_dp)
                            b.requires_grad_(need_dp)
                            x.grad = w.grad = b.grad = None
                            fn(x, w, b).backward(dy)
                        row = dict(base, gradients="all" if need_dp else "dx", **pairs(lambda: run(ops.linear), lambda: run(F.linear)))
                        rows_out.append(row)
                        print(f"linear {tag} {rows} x {K} -> {N} {row['gradients']}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                              f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); wgrad kernel {kern:.3f} ms = "
                              f"{row['wgrad_mfma_fraction']:.3f} of peak; wins: {row['hip_route_wins']}", flush=True)
                    del x, dy, w, b
                    dump()
    dump()


if __name__ == "__main__":
    main()

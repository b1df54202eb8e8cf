"""Forward + backward time of attention under autograd at the training shapes of the reference's ControlNet run (latent 64 x 48, 14
frames: (H, S) = (5, 3072), (10, 768), (20, 192), (20, 48)) and at the sampling size (5, 9216), bf16 and f16, random data:
  (i)  the HIP route    ops.attention with ops.ATTENTION_BACKWARD on  (csrc/attn_bwd.hip)
  (ii) the PyTorch route the same call with it off (MVI_ATTN_BWD=0: scaled_dot_product_attention under autograd, with the
       [B, S, H, D] <-> [B, H, S, D] copies it needs)
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and the
PyTorch route's own spread (slowest - fastest). Also the two HIP kernels' own times and the achieved fraction of the MFMA peak,
counting the 7 tile products executed and the 5 algorithmic ones.

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_attention_bwd.py [--out profiles/attention_bwd_bench.json]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, ops  # noqa: E402

SHAPES = [(14, 5, 3072), (14, 10, 768), (14, 20, 192), (14, 20, 48), (14, 5, 9216)]
D = 64
PAIRS = 9
PEAK_TFLOPS = 2500.0          # dense bf16 / f16 MFMA peak of one MI355X (MI355X_MICROARCH.md), as tools/bench_attention.py's fractions use


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "attention_bwd_bench.json")
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    min_scores = ops.ATTENTION_BACKWARD_MIN_SCORES
    rows = []
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        for B, H, S in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(0)
            q, k, v, dy = (torch.randn(B, S, H * D, device="cuda", generator=g).to(dtype) for _ in range(4))
            qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))

            def route(on):
                def run():
                    ops.ATTENTION_BACKWARD = on
                    ops.ATTENTION_BACKWARD_MIN_SCORES = 0          # measure the HIP route also where the default routing leaves it out
                    qa.grad = ka.grad = va.grad = None
                    ops.attention(qa, ka, va, H).backward(dy)
                return run
            hip, lib = route(True), route(False)
            for _ in range(3):
                hip(), lib()
            torch.cuda.synchronize()
            t_hip, t_lib = [], []
            for _ in range(PAIRS):
                t_hip.append(timed(hip))
                t_lib.append(timed(lib))
            # the kernels on their own
            o, lse = hip_ops.attention_forward_lse(q, k, v, H)
            fwd = statistics.median(timed(lambda: hip_ops.attention_forward_lse(q, k, v, H)) for _ in range(PAIRS))
            bwd = statistics.median(timed(lambda: hip_ops.attention_backward(q, k, v, o, dy, lse, H)) for _ in range(PAIRS))
            product = 2.0 * B * H * S * S * D             # FLOPs of one Sq x Sk x D tile product over the whole problem
            row = dict(dtype=tag, B=B, H=H, S=S, pairs=PAIRS,
                       hip_fwd_bwd_ms_median=statistics.median(t_hip), pytorch_fwd_bwd_ms_median=statistics.median(t_lib),
                       pytorch_spread_ms=max(t_lib) - min(t_lib), hip_spread_ms=max(t_hip) - min(t_hip),
                       hip_forward_lse_kernel_ms=fwd, hip_backward_kernels_ms=bwd,
                       backward_mfma_fraction_7_products=7 * product / (bwd * 1e-3) / (PEAK_TFLOPS * 1e12),
                       backward_mfma_fraction_5_products=5 * product / (bwd * 1e-3) / (PEAK_TFLOPS * 1e12),
                       forward_variant=hip_ops.attention_kernel_variant(S, S, D, dtype))
            row["hip_route_kept"] = row["hip_fwd_bwd_ms_median"] <= row["pytorch_fwd_bwd_ms_median"] + row["pytorch_spread_ms"]
            ops.ATTENTION_BACKWARD_MIN_SCORES = min_scores
            row["routed_by_default"] = bool(ops.attention_backward_pays(B, S, S, H, dtype))
            rows.append(row)
            print(f"{tag} B{B} H{H} S{S}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch {row['pytorch_fwd_bwd_ms_median']:.3f} ms "
                  f"(spread {row['pytorch_spread_ms']:.3f}); kernels fwd {fwd:.3f} + bwd {bwd:.3f} ms, backward at "
                  f"{row['backward_mfma_fraction_7_products']:.3f} (7 products) / {row['backward_mfma_fraction_5_products']:.3f} (5) of peak; "
                  f"keep: {row['hip_route_kept']}", flush=True)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(dict(peak_tflops=PEAK_TFLOPS, device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""Forward + backward time of GroupNorm(+SiLU, + embedding bias) under autograd at the training shapes of the reference's ControlNet run
(latent 64 x 48, 14 frames, 32 groups; N = 14 and 28), bf16 and f16, random data, in the three layouts the training path uses
(planes: ops.group_norm; stack3: ops.group_norm_frames(T = 14, stack3 = True); tokens: ops.group_norm_tokens without SiLU / bias):
  (i)  the HIP route      ops.GROUPNORM_BACKWARD on   (csrc/groupnorm_silu.hip kStats forward + csrc/groupnorm_bwd.hip)
  (ii) the PyTorch route  the same call with it off (MVI_GN_BWD=0: the code path before the HIP backward existed)
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and each route's
spread (slowest - fastest). Also the HIP forward and backward calls on their own, and the algorithmic bytes (forward 3, backward 3
tensor passes in the I/O type) over those times as a fraction of 8 TB/s, the inference forward's own fraction beside it. Last: the
package's ResBlock / VideoResBlock (320 -> 320, 14 x 48x64, bf16) under checkpoint, new route against parent route.

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_groupnorm_bwd.py [--out profiles/groupnorm_bwd_bench.json]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, ops  # noqa: E402

SHAPES = [(320, 48, 64), (960, 48, 64), (640, 24, 32), (1920, 24, 32), (1280, 12, 16), (1280, 6, 8), (2560, 6, 8)]
PAIRS = 9
PEAK_TBS = 8.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ab(hip, lib):
    for _ in range(3):
        hip(), lib()
    torch.cuda.synchronize()
    t_hip, t_lib = [], []
    for _ in range(PAIRS):
        t_hip.append(timed(hip))
        t_lib.append(timed(lib))
    return dict(hip_fwd_bwd_ms_median=statistics.median(t_hip), pytorch_fwd_bwd_ms_median=statistics.median(t_lib),
                hip_spread_ms=max(t_hip) - min(t_hip), pytorch_spread_ms=max(t_lib) - min(t_lib))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "groupnorm_bwd_bench.json")
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    line = ops.GROUPNORM_BACKWARD_MIN_ELEMENTS
    rows = []
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        for N in (14, 28):
            for C, Hh, Ww in SHAPES:
                for layout in ("planes", "stack3", "tokens"):
                    g = torch.Generator(device="cuda").manual_seed(0)
                    x = (torch.randn(N, C, Hh, Ww, device="cuda", generator=g) * 1.5 + 0.3).to(dtype)
                    w, b = (torch.randn(C, device="cuda", generator=g).requires_grad_() for _ in range(2))
                    e = None if layout == "tokens" else torch.randn(N, C, device="cuda", generator=g).requires_grad_()
                    xa = x.clone().requires_grad_()

                    def call():
                        if layout == "tokens":
                            return ops.group_norm_tokens(xa, 32, w, b, 1e-6)
                        if layout == "stack3":
                            return ops.group_norm_frames(xa, 14, 32, w, b, 1e-5, silu=True, chan_bias=e, stack3=True)
                        return ops.group_norm(xa, 32, w, b, 1e-5, silu=True, chan_bias=e)
                    with torch.no_grad():
                        dy = torch.randn_like(call())

                    def route(on):
                        def run():
                            ops.GROUPNORM_BACKWARD = on
                            ops.GROUPNORM_BACKWARD_MIN_ELEMENTS = (0, 0, 0)      # measure the HIP route also where the default routing leaves it out
                            xa.grad = w.grad = b.grad = None
                            if e is not None:
                                e.grad = None
                            call().backward(dy)
                        return run
                    row = dict(dtype=tag, N=N, C=C, H=Hh, W=Ww, layout=layout, pairs=PAIRS, **ab(route(True), route(False)))
                    # the calls on their own
                    lay = dict(planes=hip_ops.GN_PLANES, stack3=hip_ops.GN_STACK3, tokens=hip_ops.GN_TOKENS)[layout]
                    T = 14 if layout == "stack3" else 1
                    silu, eps, cb = layout != "tokens", 1e-6 if layout == "tokens" else 1e-5, None if e is None else e.detach()
                    wd, bd = w.detach(), b.detach()
                    fwd = lambda: hip_ops.group_norm_forward_stats(x, T, 32, wd, bd, eps, silu, chan_bias=cb, layout=lay)
                    _, stats = fwd()
                    bwd = lambda: hip_ops.group_norm_backward(dy, x, stats, T, 32, wd, bd, silu, chan_bias=cb, layout=lay, need_dparams=True,
                                                              need_dchan_bias=cb is not None)
                    inf = lambda: call()
                    with torch.no_grad():
                        t_inf = statistics.median(timed(inf) for _ in range(PAIRS))
                    t_fwd = statistics.median(timed(fwd) for _ in range(PAIRS))
                    t_bwd = statistics.median(timed(bwd) for _ in range(PAIRS))
                    three = 3.0 * x.numel() * x.element_size()
                    row.update(hip_forward_stats_ms=t_fwd, hip_backward_ms=t_bwd, hip_inference_forward_ms=t_inf,
                               forward_fraction_of_8tbs=three / (t_fwd * 1e-3) / (PEAK_TBS * 1e12),
                               backward_fraction_of_8tbs=three / (t_bwd * 1e-3) / (PEAK_TBS * 1e12),
                               inference_forward_fraction_of_8tbs=three / (t_inf * 1e-3) / (PEAK_TBS * 1e12))
                    row["hip_route_kept"] = row["hip_fwd_bwd_ms_median"] < row["pytorch_fwd_bwd_ms_median"] - row["pytorch_spread_ms"]
                    ops.GROUPNORM_BACKWARD_MIN_ELEMENTS = line
                    rows.append(row)
                    print(f"{tag} N{N} C{C} {Hh}x{Ww} {layout}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms (spread {row['hip_spread_ms']:.3f}), "
                          f"PyTorch {row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); calls fwd {t_fwd:.3f} + "
                          f"bwd {t_bwd:.3f} ms = {row['forward_fraction_of_8tbs']:.3f} / {row['backward_fraction_of_8tbs']:.3f} of 8 TB/s "
                          f"(inference fwd {row['inference_forward_fraction_of_8tbs']:.3f}); keep: {row['hip_route_kept']}", flush=True)
    modules = []
    from torch.utils.checkpoint import checkpoint
    from multiview_inpaint_amd.svd import layers
    for kind in ("ResBlock", "VideoResBlock"):
        torch.manual_seed(1)
        m = getattr(layers, kind)(320, 1280, 0.0, out_channels=320)
        with torch.no_grad():
            for p in m.parameters():
                if p.ndim > 1:
                    p.normal_(0, p[0].numel() ** -0.5)
        m = m.to("cuda", torch.bfloat16)
        xg = torch.randn(14, 320, 48, 64, device="cuda").bfloat16().requires_grad_()
        emb, dy = torch.randn(14, 1280, device="cuda").bfloat16(), torch.randn(14, 320, 48, 64, device="cuda").bfloat16()
        args = (14,) if kind == "VideoResBlock" else ()

        def route(on):
            def run():
                ops.GROUPNORM_BACKWARD = on
                ops.GROUPNORM_BACKWARD_MIN_ELEMENTS = (0, 0, 0)          # every norm of the block on the HIP route
                m.zero_grad(set_to_none=True)
                xg.grad = None
                checkpoint(m, xg, emb, *args, use_reentrant=False).backward(dy)
            return run
        r = dict(module=kind, shape=[14, 320, 48, 64], dtype="bf16", pairs=PAIRS, **ab(route(True), route(False)))
        modules.append(r)
        print(f"{kind} under checkpoint: HIP norms {r['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch norms {r['pytorch_fwd_bwd_ms_median']:.3f} ms "
              f"(spread {r['pytorch_spread_ms']:.3f})", flush=True)
    ops.GROUPNORM_BACKWARD_MIN_ELEMENTS = line
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(dict(peak_tbs=PEAK_TBS, device=torch.cuda.get_device_name(0), rows=rows, modules=modules), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

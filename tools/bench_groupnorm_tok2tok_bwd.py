"""Forward + backward time of the ResBlock's middle norm — GroupNorm + SiLU with the embedding bias, token-major input [N, H W, C] from
one convolution and token-major output for the next — under autograd at the ResBlock shapes of the training latent (64 x 48, 32 groups;
N = 14 and 28), bf16 and f16, random data, on three routes:
  (a) hip     ops.group_norm_tok2tok on ops._GroupNormFn (csrc/groupnorm_tokens.hip forward with the statistics kept +
              csrc/groupnorm_bwd.hip gn_bwd_tok_*)
  (b) torch   the same call with ops.GROUPNORM_TOK2TOK_BACKWARD off: the PyTorch fallback, this op's behaviour before the HIP backward
  (c) planes  the ResBlock middle before it: a transposing copy to planes + ops.group_norm_tokens on its HIP backward
alternating in ONE process, device events around each forward + backward, PAIRS rounds per shape after warm-up; medians and each
route's spread (slowest - fastest), with every gradient asked for and with dx only. A class wins where the hip median beats the faster
of (b) and (c) by more than that route's spread. Also the HIP calls on their own (hip_ops.PROFILE's events): the algorithmic bytes of
the backward (5 tensor passes) and of the inference forward (3) over their times — the backward's two tensor kernels should hold
at least half the rate the forward's do. Last, one ResBlock line: layers.ResBlock(320, 1280, 0.0, out_channels=320), 14 x 320 x 48x64,
bf16, forward + backward with every parameter trainable and layers.RESBLOCK_CONV_BWD on, the new middle against the parent middle.

Usage (GPU box, under its own time limit):
    timeout -k 10 600 python tools/bench_groupnorm_tok2tok_bwd.py [--out profiles/groupnorm_tok2tok_bwd_bench.json]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiview_inpaint_amd.svd import hip_ops, layers, ops  # noqa: E402

LEVELS = [(48, 64, 320), (24, 32, 640), (12, 16, 1280), (6, 8, 1280)]
BATCHES = (14, 28)
PAIRS = 9
ROUTES = ("hip", "torch", "planes")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def rounds(fns):
    """{route: (median, spread)} of the routes run in turn, PAIRS rounds after three warm-up rounds."""
    for _ in range(3):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(PAIRS):
        for k, f in fns.items():
            t[k].append(timed(f))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in t.items()}


def verdict(res):
    rival = min(("torch", "planes"), key=lambda k: res[k][0])
    return rival, res["hip"][0] < res[rival][0] - res[rival][1]


def profiled_ms(fn, kinds):
    for _ in range(3):
        fn()
    hip_ops.PROFILE = []
    try:
        for _ in range(PAIRS):
            fn()
        torch.cuda.synchronize()
        return {kind: statistics.median(a.elapsed_time(b) for k, a, b, _ in hip_ops.PROFILE if k == kind) for kind in kinds}
    finally:
        hip_ops.PROFILE = None


def middle_rows(dtype, tag, N, Hh, Ww, C):
    S = Hh * Ww
    g = torch.Generator(device="cuda").manual_seed(0)
    t = (torch.randn(N, S, C, device="cuda", generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(N, S, C, device="cuda", generator=g).to(dtype)
    out = []
    for grads in ("all", "dx"):
        ta = t.clone().requires_grad_()
        w, b = (torch.randn(C, device="cuda", generator=g).requires_grad_(grads == "all") for _ in range(2))
        e = torch.randn(N, C, device="cuda", generator=g).requires_grad_(grads == "all")

        def run(route):
            def f():
                ops.GROUPNORM_TOK2TOK_BACKWARD = route == "hip"
                ta.grad = w.grad = b.grad = e.grad = None
                if route == "planes":
                    hp = ta.transpose(1, 2).reshape(N, C, Hh, Ww)
                    y = ops.group_norm_tokens(hp, 32, w, b, 1e-5, silu=True, chan_bias=e)
                else:
                    y = ops.group_norm_tok2tok(ta, 32, w, b, 1e-5, silu=True, chan_bias=e)
                y.backward(dy)
            return f
        res = rounds({k: run(k) for k in ROUTES})
        rival, wins = verdict(res)
        row = dict(dtype=tag, N=N, H=Hh, W=Ww, C=C, gradients=grads, pairs=PAIRS, rival=rival, hip_route_wins=wins)
        for k in ROUTES:
            row[k + "_fwd_bwd_ms_median"], row[k + "_spread_ms"] = res[k]
        bwd_kind = "groupnorm_tok2tok_bwd_params" if grads == "all" else "groupnorm_tok2tok_bwd"
        ms = profiled_ms(run("hip"), ("groupnorm_tok2tok_stats_fwd", bwd_kind))
        with torch.no_grad():
            ms.update(profiled_ms(lambda: ops.group_norm_tok2tok(t, 32, w, b, 1e-5, silu=True, chan_bias=e), ("groupnorm_tok2tok",)))
        nbytes = t.numel() * t.element_size()
        row.update(hip_forward_stats_call_ms=ms["groupnorm_tok2tok_stats_fwd"], hip_backward_call_ms=ms[bwd_kind],
                   hip_inference_forward_call_ms=ms["groupnorm_tok2tok"],
                   backward_call_tbs=5.0 * nbytes / (ms[bwd_kind] * 1e-3) / 1e12,
                   inference_forward_call_tbs=3.0 * nbytes / (ms["groupnorm_tok2tok"] * 1e-3) / 1e12)
        print(f"{tag} N{N} {Hh}x{Ww} C{C} {grads}: hip {res['hip'][0]:.3f} ({res['hip'][1]:.3f}), torch {res['torch'][0]:.3f} "
              f"({res['torch'][1]:.3f}), planes {res['planes'][0]:.3f} ({res['planes'][1]:.3f}) ms; calls: fwd+stats "
              f"{row['hip_forward_stats_call_ms']:.3f}, bwd {row['hip_backward_call_ms']:.3f} ms = {row['backward_call_tbs']:.2f} TB/s "
              f"(inference fwd {row['inference_forward_call_tbs']:.2f} TB/s); wins over {rival}: {wins}", flush=True)
        out.append(row)
    return out


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
    layers.RESBLOCK_CONV_BWD = True

    def route(on):
        def run():
            ops.GROUPNORM_TOK2TOK_BACKWARD = on
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x, emb).backward(dy)
        return run
    res = rounds({"tok2tok_middle": route(True), "planes_middle": route(False)})
    layers.RESBLOCK_CONV_BWD = False
    row = dict(path="resblock", dtype="bf16", N=14, H=48, W=64, C_in=320, C_out=320, gradients="all", pairs=PAIRS)
    for k, (med, spread) in res.items():
        row[k + "_fwd_bwd_ms_median"], row[k + "_spread_ms"] = med, spread
    row["tok2tok_middle_wins"] = res["tok2tok_middle"][0] < res["planes_middle"][0] - res["planes_middle"][1]
    return row


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "groupnorm_tok2tok_bwd_bench.json")
    ops.STRICT = False                                            # the PyTorch route is a recorded fallback, not an error, here
    ops.group_norm_tok2tok_backward_pays = lambda *a, **k: True   # measure the HIP route also where the default routing leaves it out
    ops.group_norm_backward_pays = lambda *a, **k: True           # route (c) and the ResBlock line: the planes norms on their HIP backward
    ops.conv3x3_backward_pays = lambda *a: True
    rows = []

    def dump():                                                   # after every shape: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)
            fh.write("\n")
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        for N in BATCHES:
            for Hh, Ww, C in LEVELS:
                rows.extend(middle_rows(dtype, tag, N, Hh, Ww, C))
                del ops.FALLBACKS[:]
                dump()
    row = resblock_line()
    rows.append(row)
    print(f"ResBlock 320 14x48x64 bf16 all gradients: token-major middle {row['tok2tok_middle_fwd_bwd_ms_median']:.3f} ms "
          f"(spread {row['tok2tok_middle_spread_ms']:.3f}), parent middle {row['planes_middle_fwd_bwd_ms_median']:.3f} ms "
          f"(spread {row['planes_middle_spread_ms']:.3f}); wins: {row['tok2tok_middle_wins']}", flush=True)
    dump()
    ops.GROUPNORM_TOK2TOK_BACKWARD = True


if __name__ == "__main__":
    main()

"""Forward + backward time of the block tails under autograd, bf16 and f16, random data, at the shapes of the 14-frame 64 x 48 training
latent and its CFG pair — N = 14 and 28 samples of (C, S) = (320, 9216), (640, 2304), (1280, 576), (1280, 144) — for
  planes_add    ops.tokens_to_planes_add(tok, x_in, bias)                 (ResBlock exit, SpatialTransformer exit)
  planes_blend  ops.tokens_blend_to_planes(tok, base, bias, alpha, hw)    (VideoResBlock tail)
  add_lerp      ops.add_lerp(x, h, base, alpha) on N S rows of C          (SpatialVideoTransformer)
  to_tokens     ops.planes_to_tokens(x)                                    (VideoResBlock's temporal entry)
with every input requiring grad ("all") and with bias and alpha frozen ("frozen"), each on
  (i)  the HIP route      ops.BLOCK_TAILS_BACKWARD on: the inference kernel forward, csrc/block_tails_bwd.hip backward
  (ii) the PyTorch route  what runs with the switch off (for planes_blend: the transposing copy + bias add + skip add + torch.lerp of
                          layers.VideoResBlock._time_stack_tokens_autograd)
alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians and the PyTorch
route's own spread (slowest - fastest). A class wins where the HIP median beats the PyTorch median by more than that spread. Also: the
new kernels' own time (hip_ops.PROFILE's events) and achieved TB/s over the bytes the algorithm needs, the planes kernel with a walk of
1 beside the rule's walk, and the peak memory of one VideoResBlock forward + backward at (14, 320, 72 x 128), switch on against off.

Usage (GPU box, under its own time limit):  timeout -k 10 600 python tools/bench_block_tails_bwd.py [--out profiles/block_tails_bwd_bench.json]
       python tools/bench_block_tails_bwd.py --routing RUN1.json RUN2.json ...    prints ops.BLOCK_TAILS_BACKWARD_ROUTED for these runs (no GPU)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CLASSES = [(320, 96, 96), (640, 48, 48), (1280, 24, 24), (1280, 12, 12)]          # (C, H, W): S = 9216, 2304, 576, 144
BATCHES = (14, 28)
KINDS = ("planes_add", "planes_blend", "add_lerp", "to_tokens")
PAIRS = 9


def routing(paths):
    """{(kind, C, S, need_dparams): smallest N_or_R from which every measured size won in both dtypes in every run}."""
    wins = {}
    for p in paths:
        with open(p) as fh:
            for r in json.load(fh)["rows"]:
                if "hip_route_wins" in r:
                    wins.setdefault((r["kind"], r["C"], r["S"], r["gradients"] == "all"), {}).setdefault(r["N_or_R"], []).append(bool(r["hip_route_wins"]))
    table = {}
    for key, by_n in sorted(wins.items()):
        lo = None
        for n in sorted(by_n, reverse=True):
            if not all(by_n[n]):
                break
            lo = n
        if lo is not None:
            table[key] = lo
    return table


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


def kernel_stats(hip_ops, fn, kinds):
    """{kind: (median ms, bytes)} of the PROFILE records of fn()."""
    for _ in range(3):
        fn()
    hip_ops.PROFILE = []
    try:
        for _ in range(PAIRS):
            fn()
        torch.cuda.synchronize()
        out = {}
        for kind in kinds:
            recs = [(a.elapsed_time(b), w) for k, a, b, w in hip_ops.PROFILE if k == kind]
            if recs:
                out[kind] = (statistics.median(t for t, _ in recs), recs[0][1])
        return out
    finally:
        hip_ops.PROFILE = None


def main():
    if "--routing" in sys.argv:
        table = routing(sys.argv[sys.argv.index("--routing") + 1:])
        print("BLOCK_TAILS_BACKWARD_ROUTED = {" + ", ".join(f"{k!r}: {v}" for k, v in table.items()) + "}")
        return
    from multiview_inpaint_amd import _lib
    from multiview_inpaint_amd.svd import hip_ops, layers, ops
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "block_tails_bwd_bench.json")
    ops.STRICT = False
    ops.block_tails_backward_pays = lambda *a: True      # measure the HIP route also where the default routing leaves it out
    rows_out, extra = [], {}
    order = sys.argv[sys.argv.index("--dtypes") + 1].split(",") if "--dtypes" in sys.argv else ["bf16", "f16"]
    L = _lib.lib()

    def dump():                                          # after every shape: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(dict(dtype_order=order, device=torch.cuda.get_device_name(0), rows=rows_out, **extra), fh, indent=1)
            fh.write("\n")

    def blend_today(tok, x, bias, alpha):                # layers.VideoResBlock._time_stack_tokens_autograd with the switch off
        h = tok.transpose(1, 2).reshape(x.shape).contiguous()
        xt = h + bias.to(h.dtype).reshape(1, -1, 1, 1) + x
        return torch.lerp(xt, x, alpha.reshape(-1, 1, 1, 1).to(x.dtype))

    for dtype, tag in (({"bf16": torch.bfloat16, "f16": torch.float16}[t], t) for t in order):
        for N in BATCHES:
            for C, H, W in CLASSES:
                S = H * W
                g = torch.Generator(device="cuda").manual_seed(0)
                rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(dtype)
                tok, base, hh = rnd(N, S, C).requires_grad_(), rnd(N, S, C).requires_grad_(), rnd(N, S, C).requires_grad_()
                x_in, dy = rnd(N, C, H, W).requires_grad_(), rnd(N, C, H, W)
                dyr = rnd(N, S, C)
                bias = (rnd(C) * 0.3).requires_grad_()
                alpha32 = torch.rand(N, device="cuda", generator=g).requires_grad_()
                alpha16 = alpha32.detach().to(dtype).requires_grad_()
                leaves = (tok, base, hh, x_in, bias, alpha32, alpha16)
                # the kernels alone: time and achieved bandwidth over the bytes the algorithm needs (hip_ops counts them)
                d, t_, b_, h_, a32 = dy.detach(), tok.detach(), base.detach(), hh.detach(), alpha32.detach()
                calls = {"planes_add all": lambda: hip_ops.planes_tail_backward(d, need_dtok=True, need_dbias=True),
                         "planes_blend all": lambda: hip_ops.planes_tail_backward(d, alpha=a32, tok=t_, bias=bias.detach(), need_dtok=True, need_dbase=True, need_dbias=True),
                         "planes_blend frozen": lambda: hip_ops.planes_tail_backward(d, alpha=a32, need_dtok=True, need_dbase=True),
                         "add_lerp all": lambda: hip_ops.rows_tail_backward(dyr, a32, x=t_, h=h_, base=b_),
                         "add_lerp frozen": lambda: hip_ops.rows_tail_backward(dyr, a32)}
                kern = {}
                for name, fn in calls.items():
                    for walk in ((0, 1) if name.startswith("planes") else (0,)):
                        L.mvi_planes_tail_backward_set_walk(walk)
                        st = kernel_stats(hip_ops, fn, ("planes_tail_bwd", "rows_tail_bwd", "tails_reduce"))
                        for kind, (ms, nbytes) in st.items():
                            kern[f"{name}{' walk1' if walk else ''} {kind}"] = dict(ms=ms, bytes=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12)
                    L.mvi_planes_tail_backward_set_walk(0)
                rows_out.append(dict(kernels=True, dtype=tag, N=N, C=C, S=S, walk=int(L.mvi_planes_tail_backward_walk(S)), stats=kern))
                print(f"kernels {tag} N={N} C={C} S={S}: " + "; ".join(f"{k} {v['ms']:.3f} ms {v['tb_per_s']:.2f} TB/s" for k, v in kern.items()), flush=True)
                for kind in KINDS:
                    for need_dp in ((True, False) if kind != "to_tokens" else (False,)):
                        def run(on):
                            ops.BLOCK_TAILS_BACKWARD = on
                            bias.requires_grad_(need_dp), alpha32.requires_grad_(need_dp), alpha16.requires_grad_(need_dp)
                            for l in leaves:
                                l.grad = None
                            if kind == "planes_add":
                                ops.tokens_to_planes_add(tok, x_in, bias).backward(dy)
                            elif kind == "planes_blend":
                                (ops.tokens_blend_to_planes(tok, base, bias, alpha32, (H, W)) if on else blend_today(tok, x_in, bias, alpha32)).backward(dy)
                            elif kind == "add_lerp":
                                ops.add_lerp(tok, hh, base, alpha16).backward(dyr)
                            else:
                                ops.planes_to_tokens(x_in).backward(dyr)
                        row = dict(kind=kind, dtype=tag, N=N, C=C, S=S, N_or_R=N * S if kind == "add_lerp" else N,
                                   gradients="all" if need_dp or kind == "to_tokens" else "frozen", **pairs(lambda: run(True), lambda: run(False)))
                        if kind == "to_tokens":
                            row["gradients"] = "frozen"                  # (no parameter: the table's need_dparams = False)
                        rows_out.append(row)
                        print(f"{kind} {tag} N={N} C={C} S={S} {row['gradients']}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms, PyTorch "
                              f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); wins: {row['hip_route_wins']}", flush=True)
                ops.BLOCK_TAILS_BACKWARD = False
                del tok, base, hh, x_in, dy, dyr, leaves, d, t_, b_, h_, calls
                dump()
    # peak memory of one VideoResBlock forward + backward at (14, 320, 72 x 128), every parameter trainable, both convolution routes on
    # and their speed decisions lifted so that the block runs on tokens either way; switch on against off
    try:
        for name in ("conv3t_backward_pays", "conv3x3_backward_pays", "group_norm_backward_pays", "group_norm_tok2tok_backward_pays"):
            setattr(ops, name, lambda *a, **k: True)
        layers.TIME_STACK_CONV_BWD = layers.RESBLOCK_CONV_BWD = True
        peak = {}
        for tag, dtype in (("bf16", torch.bfloat16),):
            m = layers.VideoResBlock(320, 1280, 0.0, video_kernel_size=[3, 1, 1], out_channels=320, merge_strategy="learned_with_images",
                                     merge_factor=0.5).to("cuda", dtype)
            x = torch.randn(14, 320, 72, 128, device="cuda").to(dtype).requires_grad_()
            emb = torch.randn(14, 1280, device="cuda").to(dtype)
            dy = torch.randn(14, 320, 72, 128, device="cuda").to(dtype)
            ind = torch.zeros(1, 14, device="cuda")
            for on in (True, False, True, False):
                ops.BLOCK_TAILS_BACKWARD = on
                del ops.FALLBACKS[:]
                x.grad = None
                m.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                m(x, emb, 14, ind).backward(dy)
                torch.cuda.synchronize()
                peak[f"{tag} {'on' if on else 'off'}"] = dict(peak_bytes_above_start=torch.cuda.max_memory_allocated() - before,
                                                             fallbacks=sorted({f[0] for f in ops.FALLBACKS}))
        extra["video_resblock_14x320x72x128_peak_memory"] = peak
        print("VideoResBlock peak memory:", peak, flush=True)
    except Exception as e:                                   # the figure is a record, not a gate: say what stood in the way
        extra["video_resblock_14x320x72x128_peak_memory"] = dict(error=repr(e))
        print("VideoResBlock peak memory: not measured:", repr(e), flush=True)
    ops.BLOCK_TAILS_BACKWARD = False
    dump()


if __name__ == "__main__":
    main()

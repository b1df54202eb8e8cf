"""Temporal attention at 25 frames (the svd_xt checkpoint of the reference's stock sampler), the three attention levels of a 576 x 1024
step at CFG batch 2: (Bo, T, S, H) = (2, 25, 9216, 5), (2, 25, 2304, 10), (2, 25, 576, 20), D = 64, bf16, random data.

Forward: the MFMA kernel of csrc/attn_temporal32.hip against the fp32-math kernel of csrc/attn_rowtile.hip — the SAME library with
  MVI_ATTN_TEMPORAL_MFMA=0. The switch is read once per process, so every repetition of either arm is a fresh child process; the
  arms alternate (mfma, rowtile, mfma, ...). A child asserts from mvi_attention_temporal_kernel_kind which kernel it is timing, warms
  every shape up, then times ITERS back-to-back calls of hip_ops.attention_temporal_packed between two device events. The fraction
  of the HBM roof uses hip_ops's own byte count for the call (q, k, v read and the output written once) over the 8.0 TB/s peak.
  Acceptance: at every shape EVERY repetition of the MFMA arm is below EVERY repetition of the rowtile arm.
Backward: forward + backward of ops.attention_temporal under autograd,
  (i)  the HIP route     _AttentionTemporalFn (the forward above, the frame-cap-32 backward of csrc/attn_bwd.hip)
  (ii) the PyTorch route  the same call with ops.ATTENTION_BACKWARD off: q, k, v regrouped to (b s) t c by three transposing copies,
       the spatial attention route (scaled_dot_product_attention under autograd at 25 keys), one copy back
  alternating in ONE process, device events around each forward + backward, PAIRS pairs per shape after warm-up; medians, spreads,
  and the two HIP kernels' own times.

Usage (GPU box, under its own time limit):  timeout -k 10 900 python tools/bench_attn_temporal.py [--out profiles/attn_temporal32_bench.json]
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = [(2, 25, 9216, 5), (2, 25, 2304, 10), (2, 25, 576, 20)]
D = 64
REPS = 3                      # child processes per arm of the forward comparison
ITERS = 200                   # calls per timed window
PAIRS = 9
PEAK_HBM = 8.0e12             # bytes / s of one MI355X (MI355X_MICROARCH.md)
CHILD_TIMEOUT = 240


def timed(fn, iters=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def forward_child(want_kind):
    """One repetition of one arm: [{Bo, T, S, H, ms, bytes}] as a JSON line on stdout."""
    import torch
    from multiview_inpaint_amd import _lib
    from multiview_inpaint_amd.svd import hip_ops
    dtype = torch.bfloat16
    rows = []
    for Bo, T, S, H in SHAPES:
        kind = _lib.lib().mvi_attention_temporal_kernel_kind(T, H, D, 1, 3 * H * D, H * D)
        assert kind == want_kind, (kind, want_kind)
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(Bo * T, S, 3 * H * D, device="cuda", generator=g).to(dtype)
        run = lambda: hip_ops.attention_temporal_packed(qkv, H, T)
        hip_ops.PROFILE = []
        run()
        torch.cuda.synchronize()
        nbytes = hip_ops.PROFILE[0][3]
        hip_ops.PROFILE = None
        timed(run, 5)
        rows.append(dict(Bo=Bo, T=T, S=S, H=H, ms=timed(run, ITERS), bytes=nbytes))
        del qkv
    print("FORWARD_ROWS " + json.dumps(rows), flush=True)


def forward_parent():
    arms = {"mfma": ("1", 32), "rowtile": ("0", 0)}
    reps = {a: [] for a in arms}
    for r in range(REPS):
        for arm, (switch, kind) in arms.items():
            env = dict(os.environ, MVI_ATTN_TEMPORAL_MFMA=switch)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-child", str(kind)], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            if p.returncode != 0:                            # a fault ends the whole measurement: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"forward child ({arm}, repetition {r}) ended with status {p.returncode}")
            line = [l for l in p.stdout.splitlines() if l.startswith("FORWARD_ROWS ")][-1]
            reps[arm].append(json.loads(line[len("FORWARD_ROWS "):]))
            print(f"forward repetition {r} {arm}: " + ", ".join(f"{x['ms']:.4f}" for x in reps[arm][-1]) + " ms", flush=True)
    rows = []
    for i, (Bo, T, S, H) in enumerate(SHAPES):
        mfma = [rep[i]["ms"] for rep in reps["mfma"]]
        rowtile = [rep[i]["ms"] for rep in reps["rowtile"]]
        nbytes = reps["mfma"][0][i]["bytes"]
        row = dict(Bo=Bo, T=T, S=S, H=H, dtype="bf16", repetitions=REPS, calls_per_repetition=ITERS, bytes_hip_ops=nbytes,
                   mfma_ms=mfma, rowtile_ms=rowtile,
                   mfma_hbm_fraction=[nbytes / (t * 1e-3) / PEAK_HBM for t in mfma],
                   rowtile_hbm_fraction=[nbytes / (t * 1e-3) / PEAK_HBM for t in rowtile],
                   every_mfma_repetition_below_every_rowtile_repetition=max(mfma) < min(rowtile))
        rows.append(row)
        print(f"forward Bo{Bo} T{T} S{S} H{H}: MFMA {min(mfma):.4f} .. {max(mfma):.4f} ms ({max(row['mfma_hbm_fraction']):.2f} of the HBM "
              f"roof at best), rowtile {min(rowtile):.4f} .. {max(rowtile):.4f} ms ({max(row['rowtile_hbm_fraction']):.2f}); "
              f"accepted: {row['every_mfma_repetition_below_every_rowtile_repetition']}", flush=True)
    return rows


def backward_rows():
    import torch
    from multiview_inpaint_amd.svd import hip_ops, ops
    ops.STRICT = False                                   # the PyTorch route is a recorded fallback, not an error, here
    dtype = torch.bfloat16
    rows = []
    for Bo, T, S, H in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        q, k, v, dy = (torch.randn(Bo * T, S, H * D, device="cuda", generator=g).to(dtype) for _ in range(4))
        qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))

        def route(on):
            def run():
                ops.ATTENTION_BACKWARD = on
                qa.grad = ka.grad = va.grad = None
                ops.attention_temporal(qa, ka, va, H, T).backward(dy)
            return run
        hip, lib = route(True), route(False)
        for _ in range(3):
            hip(), lib()
        torch.cuda.synchronize()
        t_hip, t_lib = [], []
        for _ in range(PAIRS):
            t_hip.append(timed(hip))
            t_lib.append(timed(lib))
        ops.ATTENTION_BACKWARD = True
        fwd = statistics.median(timed(lambda: hip_ops.attention_temporal(q, k, v, H, T)) for _ in range(PAIRS))
        bwd = statistics.median(timed(lambda: hip_ops.attention_temporal_backward(q, k, v, dy, H, T)) for _ in range(PAIRS))
        es = q.element_size()
        row = dict(Bo=Bo, T=T, S=S, H=H, dtype="bf16", pairs=PAIRS,
                   hip_fwd_bwd_ms=t_hip, pytorch_fwd_bwd_ms=t_lib,
                   hip_fwd_bwd_ms_median=statistics.median(t_hip), pytorch_fwd_bwd_ms_median=statistics.median(t_lib),
                   hip_spread_ms=max(t_hip) - min(t_hip), pytorch_spread_ms=max(t_lib) - min(t_lib),
                   hip_forward_kernel_ms=fwd, hip_backward_kernel_ms=bwd,
                   backward_hbm_fraction=7.0 * q.numel() * es / (bwd * 1e-3) / PEAK_HBM)
        row["hip_route_at_least_as_fast"] = row["hip_fwd_bwd_ms_median"] <= row["pytorch_fwd_bwd_ms_median"]
        rows.append(row)
        print(f"backward Bo{Bo} T{T} S{S} H{H}: HIP {row['hip_fwd_bwd_ms_median']:.3f} ms (spread {row['hip_spread_ms']:.3f}), PyTorch "
              f"{row['pytorch_fwd_bwd_ms_median']:.3f} ms (spread {row['pytorch_spread_ms']:.3f}); kernels fwd {fwd:.3f} + bwd {bwd:.3f} ms "
              f"({row['backward_hbm_fraction']:.2f} of the HBM roof); HIP at least as fast: {row['hip_route_at_least_as_fast']}", flush=True)
        del q, k, v, dy, qa, ka, va
    return rows


def main():
    if "--forward-child" in sys.argv:
        return forward_child(int(sys.argv[sys.argv.index("--forward-child") + 1]))
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join("profiles", "attn_temporal32_bench.json")
    forward = forward_parent()                           # (before this process opens the GPU itself)
    import torch
    backward = backward_rows()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(dict(peak_hbm_bytes_per_s=PEAK_HBM, device=torch.cuda.get_device_name(0), forward=forward, backward=backward), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""GPU implementations of multiview_inpaint_amd.svd.ops through the C-ABI HIP library
(include/mvi_unet_ops.h). Importing this module without libmvi_hip.so raises."""
import collections
import ctypes as C
import math

import torch

from .. import _lib
from .derived import derived1

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
_ws = {}

# Optional per-op timing for bench.py: when PROFILE is a list, every op appends
# (kind, start_event, end_event, work) with events recorded on the stream the kernel runs on. GroupNorm under autograd shows as
# "groupnorm_stats_fwd" and "groupnorm_bwd" ("groupnorm_bwd_params" when the call also launched the dweight / dbias kernel), the
# token-major norm as "groupnorm_tok2tok_stats_fwd" and "groupnorm_tok2tok_bwd" / "groupnorm_tok2tok_bwd_params",
# GEGLU under autograd as "ff_geglu" + "ff_geglu_bwd" (the kernel alone) + "ff_geglu_dparams" (for trainable parameters: the library's
# dweight GEMM and the dbias sum on the kernel's dh), or "geglu" + "geglu_bwd"; a projection under autograd (ops._LinearFn) as its forward kind +
# "linear_dgrad_n320" / "linear_dgrad_k320" (the forward kernels on the transposed weight) + "linear_wgrad" (dweight and dbias, one kind);
# the block tails under autograd (ops.BLOCK_TAILS_BACKWARD) as their forward kind + "planes_tail_bwd" / "rows_tail_bwd", and "tails_reduce"
# (the finishing kernel) when a sum (dbias, dalpha) was asked for.
PROFILE = None
# When a list: every attention call appends (kernel variant, Sq, Sk) — 0 rowtile, 4 / 16 = the 4- / 8-wave MFMA kernel
# (mvi_attention_kernel_variant, the function the C dispatch itself uses). The parity tests assert from it WHICH kernel ran
# inside a module graph.
ATTN_VARIANTS = None


class _Timed:
    def __init__(self, kind, work, dev):
        self.on = PROFILE is not None
        if self.on:
            self.kind, self.work = kind, work
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.st = torch.cuda.current_stream(dev)

    def __enter__(self):
        if self.on:
            self.a.record(self.st)

    def __exit__(self, *exc):
        if self.on:
            self.b.record(self.st)
            PROFILE.append((self.kind, self.a, self.b, self.work))


def profile_summary():
    """{kind: (calls, total_ms, total_work)} of the recorded ops; call after torch.cuda.synchronize()."""
    out = {}
    for kind, a, b, work in PROFILE or []:
        c, ms, w = out.get(kind, (0, 0.0, 0.0))
        out[kind] = (c + 1, ms + a.elapsed_time(b), w + work)
    return out


def _check(rc, what):
    if rc != 0:
        msg = _lib.lib().mvi_unet_last_error().decode(errors="replace")
        raise (Exception if rc == -1 else RuntimeError)(f"{what} failed ({rc}): {msg}")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _workspace(dev, nbytes):
    """Per-device grow-only scratch (stream-ordered reuse: every op runs on the current stream)."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    w = _ws.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _ws[key] = w
    return w


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


def _aligned(t):
    """t contiguous at a 16-byte aligned address (the kernels read 16-byte vectors); a copy only where it is not."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _ptr(t):
    return None if t is None else t.data_ptr()


_gn_sync = {}


def _groupnorm_sync(dev):
    """Zeroed once per (device, stream): the counters of the one-launch cluster GroupNorm (include/mvi_unet_ops.h,
    mvi_groupnorm_forward) — the kernels leave them zeroed, and launches that share a stream never overlap."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    b = _gn_sync.get(key)
    if b is None:
        b = torch.zeros(_lib.lib().mvi_groupnorm_sync_bytes(), dtype=torch.uint8, device=dev)
        _gn_sync[key] = b
    return b


def groupnorm_cluster_timeouts(dev=None):
    """Non-zero if a cluster GroupNorm block ever gave up waiting for its group on any stream of `dev` (sticky flag)."""
    tot = 0
    for (di, _), b in _gn_sync.items():
        if dev is None or di == torch.device(dev).index:
            tot += int(b.view(torch.int32)[2 * 65536].item())     # [arrived, departed] x 65536 groups, then the flag
    return tot


def check_groupnorm_cluster(dev=None):
    """Raises if a block of the one-launch cluster GroupNorm ever ran out of its bounded wait (the statistics of that call
    were then merged from stale partners). Cannot happen while the device makes progress (csrc/groupnorm_silu.hip: places are
    drawn as tickets in start order); called at the end of every SVDInpaintEngine.sample() and benchmark run."""
    n = groupnorm_cluster_timeouts(dev)
    if n:
        raise RuntimeError("cluster GroupNorm: a block gave up waiting for its group (device wedged?); results of this run "
                           "are not valid. MVI_GN_CLUSTER_KB=-1 selects the two-launch kernels.")


def _to_f32(p):
    return p.detach().float().contiguous()


def _f32(p):
    """fp32 contiguous copy of a (small) parameter, cached per parameter object (svd/derived.py): the kernels take their affine
    parameters in fp32, the bf16-weights model stores them in bf16, and converting on every call costs a launch."""
    if p.dtype == torch.float32 and p.is_contiguous():
        return p.detach()
    return derived1("f32", p, _to_f32)


def _chan_bias(what, chan_bias, N, C_):
    """The per-(sample, channel) bias of a norm as the kernels read it: fp32 contiguous [N, C], or None."""
    if chan_bias is None:
        return None
    cb = chan_bias.detach().float().contiguous()
    if cb.shape != (N, C_):
        raise ValueError(f"{what}: chan_bias must be [{N}, {C_}], got {tuple(cb.shape)}")
    return cb


GN_PLANES, GN_STACK3, GN_TOKENS = 0, 1, 2      # MVI_GN_DY_*: the layout the forward writes y in = the layout dy arrives in


def _gn_args(what, x, chan_bias):
    if x.dtype not in _DT:
        raise TypeError(f"{what}: unsupported dtype {x.dtype}")
    xc = _contig(x)
    N, Cc = xc.shape[0], xc.shape[1]
    S = xc.numel() // max(N * Cc, 1)
    return xc, N, Cc, S, _chan_bias(what, chan_bias, N, Cc)


def _gn_forward(x, T, num_groups, weight, bias, eps, silu, chan_bias, layout, want_stats, kind):
    """The one forward of x [N = videos * T, C, *spatial] (mvi_groupnorm_forward): (y in `layout`, stats), stats the fp32 (mean, rstd)
    table [N / T * groups, 2] when want_stats, else None — the same kernels and the same y either way."""
    L = _lib.lib()
    what = "group_norm_forward_stats" if want_stats else "group_norm"
    xc, N, Cc, S, cb = _gn_args(what, x, chan_bias)
    shape = (N, S, Cc) if layout == GN_TOKENS else (N, 3 * Cc, *xc.shape[2:]) if layout == GN_STACK3 else xc.shape
    y = torch.empty(shape, dtype=x.dtype, device=x.device)
    stats = torch.empty((N // T * num_groups, 2), dtype=torch.float32, device=x.device) if want_stats else None
    ws = _workspace(xc.device, L.mvi_groupnorm_workspace_bytes(N, Cc, S, num_groups))
    sync = None if layout == GN_TOKENS else _groupnorm_sync(xc.device)      # token-major output has no cluster form: nothing allocated
    work = (2.0 + 2.0 * (layout == GN_STACK3)) * xc.numel() * xc.element_size()
    with torch.cuda.device(xc.device), _Timed(kind, work, xc.device):
        _check(L.mvi_groupnorm_forward(xc.data_ptr(), y.data_ptr(), _f32(weight).data_ptr(), _f32(bias).data_ptr(), _ptr(cb), _ptr(stats),
                                       N // T, int(T), Cc, S, num_groups, float(eps), int(bool(silu)), int(layout), _DT[x.dtype], ws.data_ptr(),
                                       ws.numel(), _ptr(sync), 0 if sync is None else sync.numel(), _stream(xc.device)),
               "group_norm_tokens" if kind == "groupnorm_tokens" else what)
    return y, stats


def group_norm_silu(x, num_groups, weight, bias, eps, silu, chan_bias=None):
    return _gn_forward(x, 1, num_groups, weight, bias, eps, silu, chan_bias, GN_PLANES, False, "groupnorm")[0]


def group_norm_silu_tokens(x, num_groups, weight, bias, eps, silu, chan_bias=None):
    """GroupNorm(+SiLU) of x [N, C, *spatial] returned token-major [N, prod(spatial), C]."""
    return _gn_forward(x, 1, num_groups, weight, bias, eps, silu, chan_bias, GN_TOKENS, False, "groupnorm_tokens")[0]


def group_norm_silu_frames(x, T, num_groups, weight, bias, eps, silu, chan_bias=None, stack3=False):
    """x [(b T), C, *spatial] contiguous; statistics per (video, group) over all T frames."""
    return _gn_forward(x, int(T), num_groups, weight, bias, eps, silu, chan_bias, GN_STACK3 if stack3 else GN_PLANES, False, "groupnorm")[0]


def group_norm_forward_stats(x, T, num_groups, weight, bias, eps, silu, chan_bias=None, layout=GN_PLANES):
    """The forward of group_norm_silu / _frames (layout GN_PLANES, GN_STACK3) or group_norm_silu_tokens (GN_TOKENS) — same kernels, y
    bit-identical — that also returns the fp32 (mean, rstd) of every (video, group) [N / T * groups, 2] for group_norm_backward."""
    return _gn_forward(x, T, num_groups, weight, bias, eps, silu, chan_bias, layout, True, "groupnorm_stats_fwd")


def group_norm_backward_supported(N, C, S, num_groups, T, dtype, layout=GN_PLANES):
    """Whether group_norm_forward_stats / group_norm_backward compute x [N = videos * T, C, S] (mvi_groupnorm_backward_supported, a
    host-only function)."""
    if dtype not in _DT or T <= 0 or N % T != 0 or num_groups <= 0 or C % num_groups != 0:
        return False
    return bool(_lib.lib().mvi_groupnorm_backward_supported(int(N // T), int(T), int(C), int(S), int(num_groups), int(layout), _DT[dtype]))


def _tok2tok_args(what, t, chan_bias, frames=1):
    if t.dtype not in _DT:
        raise TypeError(f"{what}: unsupported dtype {t.dtype}")
    if t.dim() != 3:
        raise ValueError(f"{what}: token-major [N, S, C] expected, got {tuple(t.shape)}")
    tc = _contig(t)
    N, S, Cc = tc.shape
    if frames < 1 or N % frames:
        raise ValueError(f"{what}: {N} samples are not whole videos of {frames} frames")
    return tc, N, Cc, S, _chan_bias(what, chan_bias, N, Cc)


# One family of the backward: its names in messages and in PROFILE, the decode of x into (xc, N, C, S, chan_bias), dy's shape, the C
# entry with its workspace function, and how each takes the shape (T = the frames that share statistics).
_GnBackward = collections.namedtuple("_GnBackward", "what forward kind decode dy_shape entry workspace ws_dims dims")
_GN_BACKWARD = {
    "planes": _GnBackward(
        "group_norm_backward", "group_norm_forward_stats", "groupnorm_bwd", lambda what, x, cb, T: _gn_args(what, x, cb),
        lambda xc, N, Cc, S, layout: (N, S, Cc) if layout == GN_TOKENS else (N, (3 if layout == GN_STACK3 else 1) * Cc, *xc.shape[2:]),
        "mvi_groupnorm_backward", "mvi_groupnorm_backward_workspace_bytes",
        lambda N, T, Cc, S, G, dt: (N // T, T, Cc, S, G), lambda N, T, Cc, S, G, silu, layout, dt: (N // T, T, Cc, S, G, silu, layout, dt)),
    "tok2tok": _GnBackward(
        "group_norm_tok2tok_backward", "group_norm_tok2tok_forward_stats", "groupnorm_tok2tok_bwd", _tok2tok_args,
        lambda tc, N, Cc, S, layout: tuple(tc.shape),
        "mvi_groupnorm_tok2tok_backward", "mvi_groupnorm_tok2tok_backward_workspace_bytes",
        lambda N, T, Cc, S, G, dt: (N, T, Cc, S, G, dt), lambda N, T, Cc, S, G, silu, layout, dt: (N, T, Cc, S, G, silu, dt)),
}


def _gn_backward(family, dy, x, stats, T, num_groups, weight, bias, silu, chan_bias, layout, need_dx, need_dparams, need_dchan_bias):
    L, f = _lib.lib(), _GN_BACKWARD[family]
    xc, N, Cc, S, cb = f.decode(f.what, x, chan_bias, T)
    want = f.dy_shape(xc, N, Cc, S, layout)
    if dy.dtype != x.dtype or tuple(dy.shape) != want or not dy.is_contiguous():
        raise ValueError(f"{f.what}: dy must be contiguous {x.dtype} {want}, got {dy.dtype} {tuple(dy.shape)}")
    if stats.dtype != torch.float32 or tuple(stats.shape) != (N // T * num_groups, 2) or not stats.is_contiguous():
        raise ValueError(f"{f.what}: stats must be the fp32 [videos * groups, 2] table of {f.forward}")
    if need_dchan_bias and cb is None:
        raise ValueError(f"{f.what}: dchan_bias asked for without chan_bias")
    nbytes = int(getattr(L, f.workspace)(*f.ws_dims(N, int(T), Cc, S, num_groups, _DT[x.dtype])))
    if nbytes == 0 and xc.numel():
        raise ValueError(f"{f.what}: unsupported shape {tuple(x.shape)} / {num_groups} groups")
    f32 = dict(dtype=torch.float32, device=x.device)
    dx = torch.empty_like(xc) if need_dx else None
    dw = torch.empty(Cc, **f32) if need_dparams else None
    db = torch.empty(Cc, **f32) if need_dparams else None
    dcb = torch.empty((N, Cc), **f32) if need_dchan_bias else None
    ws = _workspace(x.device, nbytes)
    nd = 3 if layout == GN_STACK3 else 1                 # dy blocks read per element
    work = ((1.0 + nd) + (2.0 + nd) * bool(need_dx)) * xc.numel() * xc.element_size()     # reduce pass (+ apply pass) bytes
    with torch.cuda.device(x.device), _Timed(f.kind + "_params" if need_dparams else f.kind, work, x.device):
        _check(getattr(L, f.entry)(xc.data_ptr(), dy.data_ptr(), stats.data_ptr(), _f32(weight).data_ptr(), _f32(bias).data_ptr(), _ptr(cb),
                                   _ptr(dx), _ptr(dw), _ptr(db), _ptr(dcb),
                                   *f.dims(N, int(T), Cc, S, num_groups, int(bool(silu)), int(layout), _DT[x.dtype]),
                                   ws.data_ptr(), ws.numel(), _stream(x.device)), f.what)
    return dx, dw, db, dcb


def group_norm_backward(dy, x, stats, T, num_groups, weight, bias, silu, chan_bias=None, layout=GN_PLANES, need_dx=True,
                        need_dparams=False, need_dchan_bias=False):
    """(dx, dweight, dbias, dchan_bias) of the GroupNorm(+SiLU) whose forward returned `stats` (csrc/groupnorm_bwd.hip): dx in x's dtype
    and shape, the others fp32; outputs not asked for are None and cost nothing (need_dparams adds one small launch; the PROFILE kind
    is then "groupnorm_bwd_params" instead of "groupnorm_bwd"). dy: contiguous, x's dtype, in the layout the forward wrote y in.
    Deterministic."""
    return _gn_backward("planes", dy, x, stats, T, num_groups, weight, bias, silu, chan_bias, layout, need_dx, need_dparams, need_dchan_bias)


def _check_qkv(what, q, k, v, shapes=True):
    if q.dtype not in _DT or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"{what}: q/k/v must share a dtype in {list(_DT)} (got {q.dtype}, {k.dtype}, {v.dtype})")
    if shapes and (q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2]):
        raise ValueError(f"{what}: q [B,Sq,H*D], k/v [B,Sk,H*D] expected (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")


def _attn_prologue(what, q, k, v, heads, shapes=False, packed=False, kind=None):
    """The head of attention, attention_packed (q = k = v = the packed tensor) and attention_forward_lse: one supported dtype (and, with
    `shapes`, operands that line up), the sizes, the PROFILE kind — that of the kernel the C dispatch takes unless `kind` names it —
    and the ATTN_VARIANTS record. -> (B, Sq, Sk, D, kind)."""
    L = _lib.lib()
    _check_qkv(what, q, k, v, shapes)
    B, Sq, HD = q.shape
    Sk = k.shape[1]
    D = (HD // 3 if packed else HD) // heads
    if kind is None:
        kind = "attention_mfma" if L.mvi_attention_kernel_kind(Sq, Sk, D, _DT[q.dtype]) == 1 else "attention_rowtile"
    if ATTN_VARIANTS is not None:
        ATTN_VARIANTS.append((int(L.mvi_attention_kernel_variant(Sq, Sk, D, _DT[q.dtype])), Sq, Sk))
    return B, Sq, Sk, D, kind


def attention(q, k, v, heads):
    """q [B,Sq,H*D], k/v [B,Sk,H*D] -> [B,Sq,H*D]; scale = D**-0.5 (sgm/modules/attention.py:271)."""
    L = _lib.lib()
    B, Sq, Sk, D, kind = _attn_prologue("attention", q, k, v, heads)
    q, k, v = (_contig(t) for t in (q, k, v))
    out = torch.empty_like(q)
    with torch.cuda.device(q.device), _Timed(kind, 4.0 * B * heads * Sq * Sk * D, q.device):
        _check(L.mvi_attention_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, heads, Sq, Sk, D,
                                       float(D) ** -0.5, _DT[q.dtype], _stream(q.device)), "attention")
    return out


def attention_packed(qkv, heads, q_log2=False):
    """Self-attention on ONE packed projection qkv [B, S, 3*H*D] = (q | k | v) -> [B, S, H*D]: the kernels read q, k, v in
    place with a token stride of 3*H*D (mvi_attention_forward_strided), so the three projections are one GEMM.
    q_log2: q carries D^-1/2 log2(e) from its projection's weights (mvi_attention_forward_strided_qlog2)."""
    L = _lib.lib()
    if qkv.dtype not in _DT or not qkv.is_contiguous():
        raise TypeError("attention_packed: contiguous fp32/bf16/f16 [B, S, 3*H*D] expected")
    B, S, _, D, kind = _attn_prologue("attention_packed", qkv, qkv, qkv, heads, packed=True)
    C3 = qkv.shape[2]
    HD = C3 // 3
    out = torch.empty(B, S, HD, dtype=qkv.dtype, device=qkv.device)
    es = qkv.element_size()
    p = qkv.data_ptr()
    with torch.cuda.device(qkv.device), _Timed(kind, 4.0 * B * heads * S * S * D, qkv.device):
        if q_log2:
            rc = L.mvi_attention_forward_strided_qlog2(p, p + HD * es, p + 2 * HD * es, out.data_ptr(), B, heads, S, S, D, _DT[qkv.dtype],
                                                       C3, C3, HD, _stream(qkv.device))
        else:
            rc = L.mvi_attention_forward_strided(p, p + HD * es, p + 2 * HD * es, out.data_ptr(), B, heads, S, S, D,
                                                 float(D) ** -0.5, _DT[qkv.dtype], C3, C3, HD, _stream(qkv.device))
        _check(rc, "attention (packed)")
    return out


def attention_temporal_packed(qkv, heads, T, q_log2=False):
    """attention_temporal on a packed projection qkv [(bo*T), S, 3*H*D] -> [(bo*T), S, H*D]."""
    L = _lib.lib()
    if qkv.dtype not in _DT or not qkv.is_contiguous():
        raise TypeError("attention_temporal_packed: contiguous fp32/bf16/f16 [(bo T), S, 3*H*D] expected")
    BT, S, C3 = qkv.shape
    HD = C3 // 3
    D = HD // heads
    out = torch.empty(BT, S, HD, dtype=qkv.dtype, device=qkv.device)
    es = qkv.element_size()
    p = qkv.data_ptr()
    # HBM-bound (T = 14 keys per query): work = algorithmic bytes, q + k + v read and the output written once
    with torch.cuda.device(qkv.device), _Timed("attention_temporal", 4.0 * BT * S * HD * es, qkv.device):
        if q_log2:
            rc = L.mvi_attention_temporal_strided_qlog2(p, p + HD * es, p + 2 * HD * es, out.data_ptr(), BT // T, T, S, heads, D,
                                                        _DT[qkv.dtype], C3, HD, _stream(qkv.device))
        else:
            rc = L.mvi_attention_temporal_strided(p, p + HD * es, p + 2 * HD * es, out.data_ptr(), BT // T, T, S, heads, D,
                                                  float(D) ** -0.5, _DT[qkv.dtype], C3, HD, _stream(qkv.device))
        _check(rc, "attention_temporal (packed)")
    return out


def softmax_rows_(x, scale):
    """x [..., cols] contiguous: softmax(scale * x) over the last axis, in place."""
    L = _lib.lib()
    if x.dtype not in _DT or not x.is_contiguous():
        raise TypeError("softmax_rows_: contiguous fp32/bf16/f16 tensor expected")
    cols = x.shape[-1]
    rows = x.numel() // cols
    with torch.cuda.device(x.device), _Timed("softmax_rows", 2.0 * x.numel() * x.element_size(), x.device):
        _check(L.mvi_softmax_rows(x.data_ptr(), rows, cols, float(scale), _DT[x.dtype], _stream(x.device)), "softmax_rows")
    return x


_WIDE_SCORE_BYTES = 8 << 30        # scores held at once (of 288 GB)


def attention_wide(q, k, v):
    """Single-head attention with a wide head (D = C, e.g. 512 in the first-stage autoencoder's mid block): q [B,Sq,D],
    k/v [B,Sk,D] -> [B,Sq,D], scale D**-0.5. The D-deep contractions are library GEMMs (like the convolutions and
    Linear layers); the scores of a chunk of frames stay in HBM and are normalised in place by the HIP softmax."""
    B, Sq, D = q.shape
    Sk = k.shape[1]
    out = torch.empty_like(q)
    # Reduced-precision I/O (the opt-in bf16 / f16 first-stage decode): the scores and the probabilities stay fp32 — a D = 512 logit
    # rounded to bf16 before the softmax carries an error of |logit| 2^-9, which alone put the bf16 decode at 1.7 x the reference's own
    # bf16-autocast error (its scaled_dot_product_attention keeps the scores in fp32). 2 x 2 B Sq Sk D FLOPs on the fp32 matrix path:
    # ~25 ms of a 270 ms decode at 14 x 576x1024.
    wide = q.dtype != torch.float32
    per = Sq * Sk * (4 if wide else q.element_size())
    step = max(1, min(B, _WIDE_SCORE_BYTES // max(per, 1)))
    kt = k.transpose(1, 2)
    for b0 in range(0, B, step):
        if wide:
            s = torch.bmm(q[b0:b0 + step].float(), kt[b0:b0 + step].float())
            softmax_rows_(s, float(D) ** -0.5)
            out[b0:b0 + step] = torch.bmm(s, v[b0:b0 + step].float())
        else:
            s = torch.bmm(q[b0:b0 + step], kt[b0:b0 + step])
            softmax_rows_(s, float(D) ** -0.5)
            torch.bmm(s, v[b0:b0 + step], out=out[b0:b0 + step])
    return out


def attention_temporal(q, k, v, heads, T):
    """q/k/v [(bo*T), S, H*D] -> same; softmax over the T frames of each (video, token, head)."""
    L = _lib.lib()
    if q.dtype not in _DT or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"attention_temporal: q/k/v must share a dtype in {list(_DT)}")
    BT, S, HD = q.shape
    D = HD // heads
    q, k, v = (_contig(t) for t in (q, k, v))
    out = torch.empty_like(q)
    with torch.cuda.device(q.device), _Timed("attention_temporal", 4.0 * BT * S * HD * q.element_size(), q.device):
        _check(L.mvi_attention_temporal(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), BT // T, T, S, heads, D,
                                        float(D) ** -0.5, _DT[q.dtype], _stream(q.device)), "attention_temporal")
    return out


def attention_backward_supported(Sq, Sk, D, dtype):
    """Whether attention_forward_lse / attention_backward compute this shape (mvi_attention_backward_supported, a host-only function:
    bf16 / f16, D = 64, Sk > 32 — the domain of the MFMA forward kernels)."""
    return dtype in _DT and bool(_lib.lib().mvi_attention_backward_supported(int(Sq), int(Sk), int(D), _DT[dtype]))


def attention_forward_lse(q, k, v, heads):
    """attention(q, k, v, heads) — the same kernel, bit-identical output — plus the fp32 log-sum-exp of the scaled scores
    [B, H, Sq] that attention_backward needs. Returns (out, lse)."""
    L = _lib.lib()
    B, Sq, Sk, D, kind = _attn_prologue("attention_forward_lse", q, k, v, heads, shapes=True, kind="attention_mfma_lse")
    q, k, v = (_contig(t) for t in (q, k, v))
    out = torch.empty_like(q)
    lse = torch.empty(B, heads, Sq, dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device), _Timed(kind, 4.0 * B * heads * Sq * Sk * D, q.device):
        _check(L.mvi_attention_forward_lse(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B, heads, Sq, Sk, D,
                                           float(D) ** -0.5, _DT[q.dtype], _stream(q.device)), "attention_forward_lse")
    return out, lse


def attention_backward(q, k, v, out, dout, lse, heads, need_dq=True, need_dkv=True):
    """(dq, dk, dv) of out = attention(q, k, v, heads) for the upstream gradient dout; out and lse from attention_forward_lse.
    Deterministic (no atomics). need_dkv False skips the dK/dV kernel; need_dq False skips dq's stores (the dQ kernel also produces
    the delta the dK/dV kernel uses, so dk and dv are the same bits either way). None is returned in place of what was not asked for."""
    L = _lib.lib()
    _check_qkv("attention_backward", q, k, v)
    B, Sq, HD = q.shape
    Sk = k.shape[1]
    D = HD // heads
    if out.shape != q.shape or dout.shape != q.shape or out.dtype != q.dtype or dout.dtype != q.dtype:
        raise ValueError("attention_backward: out and dout must have q's shape and dtype")
    if tuple(lse.shape) != (B, heads, Sq) or lse.dtype != torch.float32:
        raise ValueError(f"attention_backward: lse must be fp32 [B, H, Sq] = {(B, heads, Sq)}")
    q, k, v, out, dout, lse = (_contig(t) for t in (q, k, v, out, dout, lse))
    dq = torch.empty_like(q) if need_dq else None
    dk = torch.empty_like(k) if need_dkv else None
    dv = torch.empty_like(v) if need_dkv else None
    if not (need_dq or need_dkv):
        return None, None, None
    nbytes = int(L.mvi_attention_backward_workspace_bytes(B, heads, Sq, Sk, D, _DT[q.dtype]))
    ws = _workspace(q.device, nbytes)
    # algorithmic FLOPs: five Sq x Sk x D products (S, dP, dV, dK, dQ); the two kernels execute seven (S and dP twice)
    work = 2.0 * B * heads * Sq * Sk * D * (5 if need_dq and need_dkv else 3 if need_dq else 4)
    with torch.cuda.device(q.device), _Timed("attention_mfma_bwd", work, q.device):
        _check(L.mvi_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), _ptr(dq), _ptr(dk),
                                        _ptr(dv), B, heads, Sq, Sk, D, float(D) ** -0.5, _DT[q.dtype], ws.data_ptr(), ws.numel(), _stream(q.device)),
                                        "attention_backward")
    return dq, dk, dv


def attention_temporal_backward(q, k, v, dout, heads, T):
    """(dq, dk, dv) of attention_temporal(q, k, v, heads, T): q/k/v/dout [(bo*T), S, H*D], nothing regrouped."""
    L = _lib.lib()
    _check_qkv("attention_temporal_backward", q, k, v)
    if k.shape != q.shape or dout.shape != q.shape or dout.dtype != q.dtype:
        raise ValueError("attention_temporal_backward: q, k, v and dout must share shape and dtype")
    BT, S, HD = q.shape
    if BT % T:
        raise ValueError(f"attention_temporal_backward: {BT} rows are not a multiple of T = {T}")
    D = HD // heads
    q, k, v, dout = (_contig(t) for t in (q, k, v, dout))
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    with torch.cuda.device(q.device), _Timed("attention_temporal_bwd", 7.0 * BT * S * HD * q.element_size(), q.device):
        _check(L.mvi_attention_temporal_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                                 dv.data_ptr(), BT // T, T, S, heads, D, float(D) ** -0.5, _DT[q.dtype],
                                                 _stream(q.device)), "attention_temporal_backward")
    return dq, dk, dv


def geglu(h):
    L = _lib.lib()
    if h.dtype not in _DT:
        raise TypeError(f"geglu: unsupported dtype {h.dtype}")
    hc = _contig(h)
    inner = hc.shape[-1] // 2
    rows = hc.numel() // (2 * inner)
    out = torch.empty(*hc.shape[:-1], inner, dtype=h.dtype, device=h.device)
    with torch.cuda.device(h.device), _Timed("geglu", 3.0 * rows * inner * h.element_size(), h.device):
        _check(L.mvi_geglu(hc.data_ptr(), out.data_ptr(), rows, inner, _DT[h.dtype], _stream(h.device)), "geglu")
    return out


def _rows_operands(x, weight, bias, clone_misaligned_weight):
    """The operands of a row GEMM x [..., K] . weight [N, K]^T as the MFMA kernels read them: (x as [rows, K] — the kernels read 16-byte
    vectors: a misaligned view is copied —, the contiguous weight — cloned to an aligned address for the kernels that vector-load it too —,
    the fp32 bias or None, rows, the rows of the output buffer: whole 256-row blocks are stored)."""
    xc = x.reshape(-1, x.shape[-1])
    if xc.stride(1) != 1 or xc.stride(0) % 8 or xc.data_ptr() % 16:
        xc = xc.contiguous()
    if clone_misaligned_weight:
        wc = _aligned(weight)
    else:
        wc = _contig(weight)
    rows = xc.shape[0]
    return xc, wc, (None if bias is None else _f32(bias)), rows, int(_lib.lib().mvi_ff_geglu_out_rows(rows))


def ff_geglu_supported(K, inner, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_ff_geglu_supported(int(K), int(inner), _DT[dtype]))


def ff_geglu(x, weight, bias):
    """GEGLU(x) = (x W_v^T + b_v) * gelu(x W_g^T + b_g) in one kernel: x [..., K], weight [2 inner, K], bias [2 inner] or None."""
    L = _lib.lib()
    K, inner = x.shape[-1], weight.shape[0] // 2
    xc, wc, b, rows, cap = _rows_operands(x, weight, bias, True)
    full = torch.empty(cap, inner, dtype=x.dtype, device=x.device)
    out = full[:rows]
    # algorithmic bytes: x once, W once, out once; flops priced separately by the caller
    with torch.cuda.device(x.device), _Timed("ff_geglu", 4.0 * rows * K * inner, x.device):
        _check(L.mvi_ff_geglu(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), rows, cap, K, inner, xc.stride(0), full.stride(0), _DT[x.dtype],
                              _stream(x.device)), "ff_geglu")
    return out.reshape(*x.shape[:-1], inner)


def geglu_backward(h, dy):
    """dh [..., 2 inner] of y = geglu(h) for the upstream gradient dy [..., inner] (csrc/geglu.hip, mvi_geglu_backward): fp32 math,
    one pass, deterministic."""
    L = _lib.lib()
    if h.dtype not in _DT or dy.dtype != h.dtype:
        raise TypeError(f"geglu_backward: h and dy must share a dtype in {list(_DT)} (got {h.dtype}, {dy.dtype})")
    inner = h.shape[-1] // 2
    if tuple(dy.shape) != (*h.shape[:-1], inner):
        raise ValueError(f"geglu_backward: dy must be {(*h.shape[:-1], inner)} (got {tuple(dy.shape)})")
    hc = _contig(h)
    dyc = _contig(dy)
    rows = hc.numel() // max(2 * inner, 1)
    dh = torch.empty_like(hc)
    with torch.cuda.device(h.device), _Timed("geglu_bwd", 5.0 * rows * inner * h.element_size(), h.device):
        _check(L.mvi_geglu_backward(hc.data_ptr(), dyc.data_ptr(), dh.data_ptr(), rows, inner, _DT[h.dtype], _stream(h.device)),
               "geglu_backward")
    return dh


def ff_geglu_backward_supported(K, inner, dtype):
    """Whether ff_geglu_backward computes this shape (mvi_ff_geglu_backward_supported, host-only: the shapes of ff_geglu_supported)."""
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_ff_geglu_backward_supported(int(K), int(inner), _DT[dtype]))


def _ff_geglu_backward(x, weight, bias, dy, need_dx, need_dweight, need_dbias):
    """ff_geglu_backward's body: (dx, dweight, dbias, dh), dh being the transient [rows, 2 inner] buffer the kernel stored (None where
    no parameter gradient was asked for). The public wrapper drops dh; tests/test_geglu_bwd_gpu.py reads it for bit identity."""
    L = _lib.lib()
    K, inner = x.shape[-1], weight.shape[0] // 2
    if dy.dtype != x.dtype or weight.dtype != x.dtype or tuple(dy.shape) != (*x.shape[:-1], inner):
        raise ValueError(f"ff_geglu_backward: dy must be {(*x.shape[:-1], inner)} in x's dtype, weight in x's dtype")
    need_dbias = need_dbias and bias is not None
    need_dh = need_dweight or need_dbias
    if not (need_dx or need_dh):
        return None, None, None, None
    xc, wc, b, rows, _ = _rows_operands(x, weight, bias, True)
    dyc = dy.reshape(-1, inner)
    if dyc.stride(1) != 1 or dyc.stride(0) % 4 or dyc.data_ptr() % 8:
        dyc = dyc.contiguous()
    dx = torch.empty(rows, K, dtype=x.dtype, device=x.device) if need_dx else None      # NULL: the kernel skips the contraction
    dh = torch.empty(rows, 2 * inner, dtype=x.dtype, device=x.device) if need_dh else None
    # the products the kernel executes (recomputation, and the contraction where dx is asked for), 2 rows K 2 inner each
    with torch.cuda.device(x.device), _Timed("ff_geglu_bwd", (8.0 if need_dx else 4.0) * rows * K * inner, x.device):
        _check(L.mvi_ff_geglu_backward(xc.data_ptr(), wc.data_ptr(), _ptr(b), dyc.data_ptr(), _ptr(dx), _ptr(dh), rows, K, inner, xc.stride(0),
                                       dyc.stride(0), K, 2 * inner, _DT[x.dtype], _stream(x.device)), "ff_geglu_backward")
    dw = db = None
    if need_dh:                                                  # the library's share, timed as a kind of its own
        with torch.cuda.device(x.device), _Timed("ff_geglu_dparams", (4.0 * rows * K * inner) if need_dweight else 0.0, x.device):
            if need_dweight:
                dw = dh.t() @ xc
            if need_dbias:
                db = dh.sum(0, dtype=torch.float32)
    return (None if dx is None else dx.reshape(x.shape)), dw, db, dh


def ff_geglu_backward(x, weight, bias, dy, need_dx=True, need_dparams=True, need_dweight=None, need_dbias=None):
    """(dx, dweight, dbias) of y = ff_geglu(x, weight, bias) for the upstream gradient dy [..., inner] (csrc/ff_geglu_bwd.hip): the
    projection is recomputed tile by tile, gated in registers and contracted into dx — no [rows, 2 inner] tensor unless a parameter
    gradient is asked for, which has the kernel store dh in the I/O type for dweight = dh^T x (one library GEMM, fp32 accumulation,
    rounded to x.dtype) and dbias = the fp32 column sums of dh (bias given). need_dparams asks for both; need_dweight / need_dbias
    override it one by one (only the bias trainable: no GEMM). Without need_dx the kernel skips the contraction and writes dh only.
    dh is freed on return. dx and dbias are run-to-run identical; dweight is the library GEMM's. None is returned in place of what
    was not asked for. PROFILE kinds: ff_geglu_bwd (the kernel), ff_geglu_dparams (the GEMM and the column sum)."""
    need_dweight = need_dparams if need_dweight is None else need_dweight
    need_dbias = need_dparams if need_dbias is None else need_dbias
    return _ff_geglu_backward(x, weight, bias, dy, bool(need_dx), bool(need_dweight), bool(need_dbias))[:3]


def ff_geglu_n320_supported(K, inner, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_ff_geglu_n320_supported(int(K), int(inner), _DT[dtype]))


def ff_geglu_n320(x, weight, bias):
    """ff_geglu for a long contraction (K = 640 / 1280: the level-1 / level-2 FeedForward layers) on csrc/linear_n320.hip's GEGLU
    form (mvi_ff_geglu_n320): x [..., K], weight [2 inner, K], bias [2 inner] or None."""
    L = _lib.lib()
    K, inner = x.shape[-1], weight.shape[0] // 2
    xc, wc, b, rows, cap = _rows_operands(x, weight, bias, True)
    full = torch.empty(cap, inner, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _Timed("ff_geglu_n320", 4.0 * rows * K * inner, x.device):
        _check(L.mvi_ff_geglu_n320(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), rows, cap, K, inner, xc.stride(0), full.stride(0),
                                   _DT[x.dtype], _stream(x.device)), "ff_geglu_n320")
    return full[:rows].reshape(*x.shape[:-1], inner)


def linear_k320_supported(K, out_features, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_linear_k320_supported(int(K), int(out_features), _DT[dtype]))


def linear_k320(x, weight, bias, kind="linear_k320"):
    """F.linear(x, weight, bias) for K = 320 on the MFMA kernel of ff_geglu (plain epilogue): x [..., 320], weight [N, 320]. `kind`
    names the launch in PROFILE (linear_dgrad: the same kernel as an input gradient)."""
    L = _lib.lib()
    K, N = x.shape[-1], weight.shape[0]
    xc, wc, b, rows, cap = _rows_operands(x, weight, bias, True)
    full = torch.empty(cap, N, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _Timed(kind, float(rows) * (K + N) * x.element_size(), x.device):
        _check(L.mvi_linear_k320(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), rows, cap, K, N, xc.stride(0), full.stride(0), _DT[x.dtype],
                                 _stream(x.device)), "linear_k320")
    return full[:rows].reshape(*x.shape[:-1], N)


def linear_n320_supported(K, out_features, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_linear_n320_supported(int(K), int(out_features), _DT[dtype]))


def linear_n320(x, weight, bias, kind="linear_n320"):
    """F.linear(x, weight, bias) for 320 outputs and K a multiple of 64 (csrc/linear_n320.hip): x [..., K], weight [320, K]. `kind`
    names the launch in PROFILE (linear_dgrad: the same kernel as an input gradient)."""
    L = _lib.lib()
    K, N = x.shape[-1], weight.shape[0]
    xc, wc, b, rows, cap = _rows_operands(x, weight, bias, False)
    full = torch.empty(cap, N, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _Timed(kind, 2.0 * rows * K * N, x.device):
        _check(L.mvi_linear_n320(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), rows, cap, K, N, xc.stride(0), full.stride(0), _DT[x.dtype],
                                 _stream(x.device)), "linear_n320")
    return full[:rows].reshape(*x.shape[:-1], N)


# ---- the projections under autograd (ops._LinearFn): dgrad on the forward kernels, wgrad + dbias in csrc/linear_wgrad.hip --------------

N320_GROUP_WIDTHS = (640, 1280)                 # ops.linear prefers linear_n320 into these widths (its measured classes)


def linear_dgrad_kernel(K, out_features, dtype):
    """Which forward kernel computes dx = dy . W for a forward with W [out_features, K] — a projection with weight W^T [K, out_features],
    contraction out_features, K outputs — in ops.linear's order of preference: 'n320' into 640 / 1280 channels and for 320 -> 320,
    then 'k320', then 'n320'; None where neither takes the shape."""
    n320 = linear_n320_supported(out_features, K, dtype)
    if n320 and (K in N320_GROUP_WIDTHS or (K == 320 and out_features == 320)):
        return "n320"
    if linear_k320_supported(out_features, K, dtype):
        return "k320"
    return "n320" if n320 else None


def linear_dgrad(dy, weight_t, bias=None):
    """dx [..., K] of y = F.linear(x, W) for the upstream gradient dy [..., N]: the forward kernel on weight_t = W^T [K, N] (contiguous).
    PROFILE kind linear_dgrad_n320 / linear_dgrad_k320 (linear_dgrad_kernel's choice); raises where neither kernel takes the shape."""
    if weight_t.dim() != 2 or weight_t.shape[1] != dy.shape[-1] or weight_t.dtype != dy.dtype:
        raise ValueError("linear_dgrad: dy [..., N] and weight_t [K, N] of one dtype expected")
    which = linear_dgrad_kernel(weight_t.shape[0], weight_t.shape[1], dy.dtype)
    if which is None:
        raise ValueError(f"linear_dgrad: no kernel for a contraction of {weight_t.shape[1]} into {weight_t.shape[0]} outputs in {dy.dtype}")
    if which == "n320":
        return linear_n320(dy, weight_t, bias, kind="linear_dgrad_n320")
    return linear_k320(dy, weight_t, bias, kind="linear_dgrad_k320")


def linear_wgrad_supported(K, out_features, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_linear_wgrad_supported(int(K), int(out_features), _DT[dtype]))


def linear_wgrad_workspace_bytes(rows, K, out_features):
    """> 0: csrc/linear_wgrad.hip splits the row axis of this shape over blocks (a pure host function of the shape)."""
    return int(_lib.lib().mvi_linear_wgrad_workspace_bytes(int(rows), int(K), int(out_features)))


def _rows16(t):
    """t [..., C] as [rows, C] with unit column stride, rows 16-byte aligned at a stride linear_wgrad.hip takes; a copy only otherwise."""
    t2 = t.reshape(-1, t.shape[-1])
    if t2.stride(1) != 1 or t2.stride(0) % 8 or t2.stride(0) < t2.shape[1] or t2.stride(0) >= 1 << 24 or t2.data_ptr() % 16:
        t2 = t2.contiguous()
        if t2.data_ptr() % 16:
            t2 = t2.clone()
    return t2


def linear_wgrad(x, dy, need_dbias, split=True):
    """(dweight fp32 [N, K], dbias fp32 [N] or None) of y = F.linear(x, W, b) from x [..., K] and the output gradient dy [..., N] (one
    16-bit dtype; row-strided views such as a third of the packed q | k | v output are read in place): csrc/linear_wgrad.hip, one
    launch for both (plus the fixed-order sum of the row slices), deterministic. split = False withholds the workspace (the unsplit
    launch). PROFILE kind linear_wgrad."""
    L = _lib.lib()
    if x.dtype != dy.dtype or x.shape[:-1] != dy.shape[:-1]:
        raise ValueError("linear_wgrad: x [..., K] and dy [..., N] of one dtype and the same leading shape expected")
    xc, dc = _rows16(x), _rows16(dy)
    rows, K = xc.shape
    N = dc.shape[1]
    dw = torch.empty(N, K, dtype=torch.float32, device=x.device)
    db = torch.empty(N, dtype=torch.float32, device=x.device) if need_dbias else None
    ws_bytes = int(L.mvi_linear_wgrad_workspace_bytes(rows, K, N)) if split else 0
    ws = _workspace(x.device, ws_bytes) if ws_bytes else None
    with torch.cuda.device(x.device), _Timed("linear_wgrad", 2.0 * rows * K * N, x.device):
        _check(L.mvi_linear_wgrad(xc.data_ptr(), dc.data_ptr(), dw.data_ptr(), _ptr(db), rows, K, N, xc.stride(0), dc.stride(0),
                                  _DT.get(x.dtype, -1), _ptr(ws), ws_bytes, _stream(x.device)), "linear_wgrad")
    return dw, db


def linear_n320_add_layer_norm(x, weight, bias, ln_weight, ln_bias, eps, resid=None, row=None, ret_pre=False):
    """add_layer_norm(resid, h=F.linear(x, weight, bias), row=row) with the projection in the same kernel (mvi_linear_n320_add_layernorm):
    x [..., K], weight [320, K]; resid [..., 320] or None (then the sum starts from h); row [G, 320] / [G, 1, 320] or None.
    Returns (y, s, s_pre) like add_layer_norm: s the residual stream after the adds (h itself without resid and row), s_pre = resid + h
    only with ret_pre."""
    L = _lib.lib()
    K, N = x.shape[-1], weight.shape[0]
    xc, wc, b, rows, cap = _rows_operands(x, weight, bias, False)
    rc, rowc, row_div = None, None, 1
    if resid is not None:
        if resid.shape[-1] != N or resid.numel() != rows * N or resid.dtype != x.dtype:
            raise ValueError("linear_n320_add_layer_norm: resid must be [rows, 320] of x's dtype")
        rc = resid.reshape(rows, N)
        rc = rc if rc.is_contiguous() and rc.data_ptr() % 16 == 0 else rc.contiguous()
    if row is not None:
        if row.dtype != x.dtype or row.shape[-1] != N:
            raise ValueError("linear_n320_add_layer_norm: row must be [G, 320] / [G, 1, 320] of x's dtype")
        rowc = _aligned(row.reshape(-1, N))
        G = rowc.shape[0]
        if G == 0 or rows % G:
            raise ValueError(f"linear_n320_add_layer_norm: {rows} rows do not split into {G} equal runs")
        row_div = rows // G
    y = torch.empty(cap, N, dtype=x.dtype, device=x.device)
    s = torch.empty(cap, N, dtype=x.dtype, device=x.device)
    s_pre = torch.empty(cap, N, dtype=x.dtype, device=x.device) if (ret_pre and rowc is not None) else None
    # the 320 -> 320 projections (to_out, proj_in / proj_out: 53 GFLOP around ~0.7 GB of rows) are HBM-bound like linear_k320 and are
    # reported against that roof (VERDICT r5 "weak" 7): work = algorithmic bytes (x read; resid read; s, y and s_pre written)
    n_tensors = 2 + (rc is not None) + (s_pre is not None)
    kind, work = ("linear_n320_ln_k320", float(rows) * (K + N * n_tensors) * x.element_size()) if K <= N else ("linear_n320_ln", 2.0 * rows * K * N)
    with torch.cuda.device(x.device), _Timed(kind, work, x.device):
        _check(L.mvi_linear_n320_add_layernorm(xc.data_ptr(), wc.data_ptr(), _ptr(b), rows, cap, K, xc.stride(0), _ptr(rc), _ptr(rowc), row_div,
                                               _f32(ln_weight).data_ptr(), _f32(ln_bias).data_ptr(), float(eps), _ptr(s_pre), s.data_ptr(),
                                               y.data_ptr(), N, _DT[x.dtype], _stream(x.device)), "linear_n320_add_layer_norm")
    shape = (*x.shape[:-1], N)
    s = s[:rows].reshape(shape)
    if ret_pre:
        s_pre = s if s_pre is None else s_pre[:rows].reshape(shape)
    return y[:rows].reshape(shape), s, s_pre


def conv3x3_n320_supported(C_in, C_out, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_conv3x3_n320_supported(int(C_in), int(C_out), _DT[dtype]))


def conv3x3_k_order():
    """The contraction order csrc/linear_n320.hip reads 3x3 weights in (mvi_conv3x3_n320_k_order, a process-global switch read again at
    every launch): 1 = [C_in / 64][9 taps][64 channels], 0 = tap-major. Part of the signature of every cached packed weight, so a switch
    after the first forward re-packs instead of silently mis-convolving."""
    return int(_lib.lib().mvi_conv3x3_n320_k_order(-1))


def conv3x3_n320_weight(weight):
    """conv.weight [C_out, C_in, 3, 3] in the kernel's order (mvi_conv3x3_n320_k_order): [C_out][C_in / 64][9 taps (ky, kx)][64
    channels] — or, order 0, [C_out][9][C_in], tap-major."""
    Co, Ci = weight.shape[0], weight.shape[1]
    taps = weight.permute(0, 2, 3, 1).reshape(Co, 9, Ci)                       # [Co, tap, c]
    if conv3x3_k_order() == 1 and Ci % 64 == 0:
        return taps.reshape(Co, 9, Ci // 64, 64).permute(0, 2, 1, 3).reshape(Co, -1).contiguous()
    return taps.reshape(Co, -1).contiguous()


def conv3t_n320_weight(weight):
    """Conv3d weight [C_out, C_in, 3, 1, 1] in the kernel's order: [C_out][3 C_in], tap-major (kt, c)."""
    return weight[:, :, :, 0, 0].permute(0, 2, 1).reshape(weight.shape[0], -1).contiguous()


class GnPartials:
    """Statistics a producer kernel left for the GroupNorm behind it: `part` [samples * chunks * groups, 3] fp32 (count, mean, M2),
    `chunks` per sample, for `groups` groups and the per-sample channel bias `chan_bias` (the object, or None) they were taken with."""
    __slots__ = ("part", "chunks", "groups", "chan_bias")

    def __init__(self, part, chunks, groups, chan_bias):
        self.part, self.chunks, self.groups, self.chan_bias = part, int(chunks), int(groups), chan_bias


def conv_n320_gnstats_supported(rows, taps, C_in, C_out, spatial, groups, stride=1):
    return bool(_lib.lib().mvi_conv_n320_gnstats_supported(int(rows), int(taps), int(stride), int(C_in), int(C_out), int(spatial), int(groups)))


def _conv_taps_n320(kind, tok, weight_taps, bias, N, H, W, taps, stride=1, split=True, gn=None, up2=False):
    """tok: token-major activations of N images of H x W pixels (or, taps = 3, N videos of H frames of W pixels).
    gn = (groups, chan_bias [samples, C_out] fp32 or None): also leave the statistics of the GroupNorm that follows
    (mvi_conv3x3_n320_gnstats / mvi_conv3t_n320_gnstats) — returns (out, GnPartials); the caller asked
    conv_n320_gnstats_supported first."""
    L = _lib.lib()
    C = tok.shape[-1]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if up2:                                    # tok holds the H x W source of the 2x upsampled image the convolution runs over
        if taps != 9 or stride != 1 or gn is not None:
            raise ValueError(f"{kind}: upsampling goes with the plain 3x3 / stride 1 form")
        Ho, Wo = 2 * H, 2 * W
    rows = N * Ho * Wo
    if tok.numel() != N * H * W * C or weight_taps.shape[1] != taps * C or weight_taps.dtype != tok.dtype:
        raise ValueError(f"{kind}: token-major activations [.., C_in] of N H W rows and weight [C_out, {taps} C_in] of one dtype expected")
    xc = _aligned(tok)
    wc = _contig(weight_taps)
    Co = wc.shape[0]
    cap = int(L.mvi_ff_geglu_out_rows(rows))
    full = torch.empty(cap, Co, dtype=tok.dtype, device=tok.device)
    b = None if bias is None else _f32(bias)
    # > 0: a small image, K split over several blocks per tile
    ws_bytes = 0 if not split or up2 else int(L.mvi_conv3x3_n320_workspace_bytes(N, H, W, C, Co, stride) if taps == 9
                                              else L.mvi_conv3t_n320_workspace_bytes(N, H, W, C, Co))      # (the upsampling form never splits)
    ws = _workspace(tok.device, ws_bytes) if ws_bytes else None
    wsp = _ptr(ws)
    if gn is not None:
        groups, cb = gn
        samples, spatial = (N, H * W) if taps == 9 else (N * H, W)
        if cb is not None and (cb.dtype != torch.float32 or not cb.is_contiguous() or tuple(cb.shape) != (samples, Co)):
            raise ValueError(f"{kind}: gn chan_bias must be contiguous fp32 [{samples}, {Co}]")
        nb = int(L.mvi_conv_n320_gnstats_bytes(samples, spatial, int(groups)))
        part = torch.empty(nb // 4, dtype=torch.float32, device=tok.device)
        fn = L.mvi_conv3x3_n320_gnstats if taps == 9 else L.mvi_conv3t_n320_gnstats
        with torch.cuda.device(tok.device), _Timed(kind, 2.0 * rows * taps * C * Co, tok.device):
            _check(fn(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), N, H, W, C, Co, cap, full.stride(0), _DT[tok.dtype], _ptr(cb),
                      int(groups), part.data_ptr(), nb, _stream(tok.device)), kind + " (gn stats)")
        return full[:rows], GnPartials(part, spatial // 256, groups, cb)
    with torch.cuda.device(tok.device), _Timed(kind, 2.0 * rows * taps * C * Co, tok.device):
        if up2:
            rc = L.mvi_conv3x3_up2_n320(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), N, H, W, C, Co, cap, full.stride(0), _DT[tok.dtype],
                                        wsp, ws_bytes, _stream(tok.device))
        elif taps == 9:
            rc = L.mvi_conv3x3_n320(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), N, H, W, C, Co, stride, cap, full.stride(0),
                                    _DT[tok.dtype], wsp, ws_bytes, _stream(tok.device))
        else:
            rc = L.mvi_conv3t_n320(xc.data_ptr(), wc.data_ptr(), _ptr(b), full.data_ptr(), N, H, W, C, Co, cap, full.stride(0), _DT[tok.dtype], wsp,
                                   ws_bytes, _stream(tok.device))
        _check(rc, kind)
    return full[:rows]


# The forms of the implicit-GEMM convolution launch: form -> (stride, whether csrc/linear_n320.hip K-splits it). "up2" (the convolution
# of the nearest-2x upsampled image) and "s2_dgrad" (the zero-stuffed input gradient of the stride-2 form) are instantiations of their
# own that never split (conv_taps_n320 sets cg.ksplit = 1 for them); "t3" is the (3,1,1) frame form with (N, H, W) = (B, T, S).
_CONV_N320_FORMS = {"s1": (1, True), "s2": (2, True), "up2": (1, False), "s2_dgrad": (1, False), "t3": (1, True)}


def conv_n320_launch_ok(form, N, H, W, C_in, C_out, dtype, min_blocks, ksplit_counts=None):
    """Does csrc/linear_n320.hip take this convolution launch and fill the chip? THE routing gate of every caller in ops.py and layers.py.
    N images of H x W pixels with C_in channels as the launch's wrapper is handed them — "up2": the SOURCE of the upsampled image;
    "s2_dgrad": the full-size H x W image dx has, C_in the channels of dy; "t3": B videos of T frames of S pixels. True when
      * the kernel's channel / dtype gate passes (mvi_conv3x3_n320_supported),
      * there is at least one output row,
      * the image the kernel addresses stays within 32-bit byte offsets (conv_taps_n320: N H W C_in 2 <= 0xFFFFFFFF, H x W doubled
        for "up2"),
      * its 256-row x 320-channel blocks number min_blocks or more, or the form K-splits and the library would split this shape
        (its *_workspace_bytes is positive).
    ksplit_counts overrides the form's own answer to "can it split" (one caller: layers.Upsample)."""
    stride, splits = _CONV_N320_FORMS[form]
    if not conv3x3_n320_supported(C_in, C_out, dtype):      # (first: the library's split policy divides by the block count)
        return False
    if form == "up2":
        H, W = 2 * H, 2 * W
    rows = N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    if rows <= 0 or N * H * W * C_in * 2 > 0xFFFFFFFF:
        return False
    if -(-rows // 256) * (C_out // 320) >= min_blocks:
        return True
    if not (splits if ksplit_counts is None else ksplit_counts):
        return False
    L = _lib.lib()
    return int(L.mvi_conv3t_n320_workspace_bytes(N, H, W, C_in, C_out) if form == "t3"
               else L.mvi_conv3x3_n320_workspace_bytes(N, H, W, C_in, C_out, stride)) > 0


def conv3x3_n320(tok, weight_taps, bias, H, W, stride=1, split=True, gn=None, up2=False, kind="conv3x3_n320"):
    """3x3 / padding 1 convolution (stride 1 or 2) to a multiple of 320 output channels of token-major activations tok [N, H W, C_in]
    (csrc/linear_n320.hip in its implicit-GEMM mode) -> [N, Ho Wo, C_out]; weight_taps from conv3x3_n320_weight.
    gn = (groups, chan_bias): -> (out, GnPartials) for the GroupNorm that follows (see _conv_taps_n320).
    up2: the convolution of the nearest-neighbour 2x upsampled image (mvi_conv3x3_up2_n320) -> [N, (2 H)(2 W), C_out].
    kind: the PROFILE kind of the launch ("conv3x3_dgrad" when it computes an input gradient, conv3x3_dgrad below)."""
    N, S, C = tok.shape
    if S != H * W:
        raise ValueError("conv3x3_n320: tok [N, H W, C_in] expected")
    r = _conv_taps_n320(kind, tok, weight_taps, bias, N, H, W, 9, stride, split, gn=gn, up2=up2)
    if gn is not None:
        return r[0].view(N, -1, weight_taps.shape[0]), r[1]
    return r.view(N, -1, weight_taps.shape[0])


# ---- the 3x3 convolution under autograd (ops._ConvTokensFn "s1"): dgrad on the forward kernel, wgrad in csrc/conv3x3_wgrad.hip ---------

CONV3X3_WGRAD_MAX_W = 256                       # csrc/conv3x3_wgrad.hip: the x chunk with its two halo rows has to fit in LDS


def conv3x3_transposed_weight(weight):
    """The weight whose 3x3 / padding 1 / stride 1 convolution of dy is the input gradient of conv(x, weight):
    W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx], as a view [C_in, C_out, 3, 3]. Pure torch; loads no library."""
    return weight.flip(2, 3).transpose(0, 1)


def conv3x3_dgrad(dy_tok, weight_t_taps, H, W, split=True):
    """dx [N, H W, C_in] of the 3x3 / padding 1 / stride 1 convolution from dy [N, H W, C_out]: the forward kernel on the packed
    transposed weight (conv3x3_n320_weight(conv3x3_transposed_weight(weight))), channel roles swapped. PROFILE kind conv3x3_dgrad."""
    return conv3x3_n320(dy_tok, weight_t_taps, None, H, W, split=split, kind="conv3x3_dgrad")


def _conv_wgrad(entry, workspace_bytes, dims, tok, dy_tok, out_shape, kind, flops, split):
    """The launch of the three convolution weight gradients: entry(x, dy, dweight, *dims, dtype, workspace, workspace_bytes, stream) on
    aligned operands, with the workspace workspace_bytes(*dims) asks for unless split is False. -> dweight, fp32 [*out_shape]."""
    xc, dc = _aligned(tok), _aligned(dy_tok)
    dw = torch.empty(out_shape, dtype=torch.float32, device=tok.device)
    ws_bytes = int(workspace_bytes(*dims)) if split else 0
    ws = _workspace(tok.device, ws_bytes) if ws_bytes else None
    with torch.cuda.device(tok.device), _Timed(kind, flops, tok.device):
        _check(entry(xc.data_ptr(), dc.data_ptr(), dw.data_ptr(), *dims, _DT.get(tok.dtype, -1), _ptr(ws), ws_bytes, _stream(tok.device)), kind)
    return dw


def conv3x3_wgrad_supported(C_in, C_out, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_conv3x3_wgrad_supported(int(C_in), int(C_out), _DT[dtype]))


def conv3x3_wgrad_workspace_bytes(N, H, W, C_in, C_out):
    """> 0: csrc/conv3x3_wgrad.hip splits the pixel axis of this shape over blocks (a pure host function of the shape)."""
    return int(_lib.lib().mvi_conv3x3_wgrad_workspace_bytes(int(N), int(H), int(W), int(C_in), int(C_out)))


def conv3x3_wgrad(tok, dy_tok, H, W, split=True):
    """dweight, fp32 [C_out, C_in, 3, 3], of the 3x3 / padding 1 / stride 1 convolution from its input tok [N, H W, C_in] and the output
    gradient dy_tok [N, H W, C_out] (one 16-bit dtype): csrc/conv3x3_wgrad.hip, deterministic. split = False withholds the workspace
    (the unsplit launch). PROFILE kind conv3x3_wgrad."""
    L = _lib.lib()
    if tok.dim() != 3 or dy_tok.dim() != 3 or tok.shape[:2] != dy_tok.shape[:2] or tok.shape[1] != H * W or tok.dtype != dy_tok.dtype:
        raise ValueError("conv3x3_wgrad: tok [N, H W, C_in] and dy_tok [N, H W, C_out] of one dtype expected")
    N, S, C = tok.shape
    Co = dy_tok.shape[2]
    return _conv_wgrad(L.mvi_conv3x3_wgrad, L.mvi_conv3x3_wgrad_workspace_bytes, (N, H, W, C, Co), tok, dy_tok, (Co, C, 3, 3),
                       "conv3x3_wgrad", 2.0 * N * S * 9 * C * Co, split)


# ---- the stride-2 and the upsampling 3x3 convolution under autograd (ops._ConvTokensFn "s2" / "up2") ------------------------------------

def conv3x3_s2_dgrad_supported(C_in, C_out, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_conv3x3_s2_dgrad_supported(int(C_in), int(C_out), _DT[dtype]))


def conv3x3_s2_dgrad(dy_tok, weight_t_taps, H, W):
    """dx [N, H W, C_in] of the 3x3 / padding 1 / STRIDE 2 convolution of an H x W image (both even) from dy [N, (H / 2)(W / 2), C_out]:
    the forward kernel on the packed transposed weight (conv3x3_n320_weight(conv3x3_transposed_weight(weight)), the packing of
    conv3x3_dgrad) reading dy as the zero-stuffed H x W image it never builds (mvi_conv3x3_s2_dgrad). PROFILE kind conv3x3_s2_dgrad."""
    L = _lib.lib()
    if dy_tok.dim() != 3 or H % 2 or W % 2 or dy_tok.shape[1] != (H // 2) * (W // 2):
        raise ValueError("conv3x3_s2_dgrad: dy_tok [N, (H / 2)(W / 2), C_out] with even H and W expected")
    N, _, Co = dy_tok.shape
    if weight_t_taps.dim() != 2 or weight_t_taps.shape[1] != 9 * Co or weight_t_taps.dtype != dy_tok.dtype:
        raise ValueError("conv3x3_s2_dgrad: packed transposed weight [C_in, 9 C_out] of dy's dtype expected")
    dc = _aligned(dy_tok)
    wc = _contig(weight_t_taps)
    Ci = wc.shape[0]
    rows = N * H * W
    cap = int(L.mvi_ff_geglu_out_rows(rows))
    full = torch.empty(cap, Ci, dtype=dy_tok.dtype, device=dy_tok.device)
    with torch.cuda.device(dy_tok.device), _Timed("conv3x3_s2_dgrad", 2.0 * rows * 9 * Ci * Co / 4, dy_tok.device):
        _check(L.mvi_conv3x3_s2_dgrad(dc.data_ptr(), wc.data_ptr(), full.data_ptr(), N, H, W, Ci, Co, cap, full.stride(0),
                                      _DT.get(dy_tok.dtype, -1), _stream(dy_tok.device)), "conv3x3_s2_dgrad")
    return full[:rows].view(N, H * W, Ci)


def conv3x3_s2_wgrad_supported(C_in, C_out, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_conv3x3_s2_wgrad_supported(int(C_in), int(C_out), _DT[dtype]))


def conv3x3_s2_wgrad_workspace_bytes(N, H, W, C_in, C_out):
    """> 0: the stride-2 form of csrc/conv3x3_wgrad.hip splits the pixel axis of this shape over blocks (a pure host function of the shape)."""
    return int(_lib.lib().mvi_conv3x3_s2_wgrad_workspace_bytes(int(N), int(H), int(W), int(C_in), int(C_out)))


def conv3x3_s2_wgrad(tok, dy_tok, H, W, split=True):
    """dweight, fp32 [C_out, C_in, 3, 3], of the 3x3 / padding 1 / STRIDE 2 convolution from its input tok [N, H W, C_in] and the output
    gradient dy_tok [N, (H / 2)(W / 2), C_out] (one 16-bit dtype; H, W even): csrc/conv3x3_wgrad.hip's stride-2 form (x staged as four
    parity planes), deterministic. split = False withholds the workspace (the unsplit launch). PROFILE kind conv3x3_s2_wgrad."""
    L = _lib.lib()
    if tok.dim() != 3 or dy_tok.dim() != 3 or tok.shape[0] != dy_tok.shape[0] or tok.shape[1] != H * W or tok.dtype != dy_tok.dtype \
            or dy_tok.shape[1] != ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1):
        raise ValueError("conv3x3_s2_wgrad: tok [N, H W, C_in] and dy_tok [N, (H / 2)(W / 2), C_out] of one dtype expected")
    N, S, C = tok.shape
    Co = dy_tok.shape[2]
    return _conv_wgrad(L.mvi_conv3x3_s2_wgrad, L.mvi_conv3x3_s2_wgrad_workspace_bytes, (N, H, W, C, Co), tok, dy_tok, (Co, C, 3, 3),
                       "conv3x3_s2_wgrad", 2.0 * N * dy_tok.shape[1] * 9 * C * Co, split)


def pool2x2_sum(g_tok, h, w):
    """g_tok [N, (2 h)(2 w), C] -> [N, h w, C]: the sum over every 2x2 cell in fp32, rounded once (mvi_rows_pool2x2_sum) — the adjoint of the
    nearest-neighbour 2x upsampling. C a multiple of 8, bf16 / f16. PROFILE kind pool2x2_sum."""
    L = _lib.lib()
    if g_tok.dim() != 3 or g_tok.shape[1] != 4 * h * w:
        raise ValueError("pool2x2_sum: g_tok [N, (2 h)(2 w), C] expected")
    N, _, C = g_tok.shape
    gc = _aligned(g_tok)
    out = torch.empty(N, h * w, C, dtype=g_tok.dtype, device=g_tok.device)
    with torch.cuda.device(g_tok.device), _Timed("pool2x2_sum", 3.0 * N * h * w * C, g_tok.device):
        _check(L.mvi_rows_pool2x2_sum(gc.data_ptr(), out.data_ptr(), N, h, w, C, _DT.get(g_tok.dtype, -1), _stream(g_tok.device)), "pool2x2_sum")
    return out


def conv3x3_up2_dgrad(dy_tok, weight_t_taps, h, w):
    """dx [N, h w, C_in] of the convolution of the nearest-2x upsampled h x w image from dy [N, (2 h)(2 w), C_out]: conv3x3_dgrad at
    2 h x 2 w, then pool2x2_sum."""
    return pool2x2_sum(conv3x3_dgrad(dy_tok, weight_t_taps, 2 * h, 2 * w), h, w)


def conv3t_n320(tok, weight_taps, bias, T, split=True, gn=None, kind="conv3t_n320"):
    """(3, 1, 1) / padding (1, 0, 0) convolution over the frame axis of token-major activations tok [(b T), S, C_in] (frames of a video
    consecutive) -> [(b T), S, C_out]; weight_taps from conv3t_n320_weight. gn: as conv3x3_n320 (a sample = a frame).
    kind: the PROFILE kind of the launch ("conv3t_dgrad" when it computes an input gradient, conv3t_dgrad below)."""
    BT, S, C = tok.shape
    if BT % T:
        raise ValueError("conv3t_n320: tok [(b T), S, C_in] expected")
    r = _conv_taps_n320(kind, tok, weight_taps, bias, BT // T, T, S, 3, 1, split, gn=gn)
    if gn is not None:
        return r[0].view(BT, S, -1), r[1]
    return r.view(BT, S, -1)


# ---- the (3,1,1) frame convolution under autograd (ops._ConvTokensFn "t3"): dgrad on the forward kernel, wgrad in csrc/conv3t_wgrad.hip --

CONV3T_WGRAD_CHUNK = 64                         # csrc/conv3t_wgrad.hip (kKc): pixels of one video a block stages per frame


def conv3t_transposed_weight(weight):
    """The weight whose (3, 1, 1) / padding (1, 0, 0) convolution of dy is the input gradient of conv(x, weight):
    W'[ci, co, kt] = W[co, ci, 2 - kt], as a view [C_in, C_out, 3, 1, 1]. Pure torch; loads no library."""
    return weight.flip(2).transpose(0, 1)


def conv3t_dgrad(dy_tok, weight_t_taps, T, split=True):
    """dx [(b T), S, C_in] of the frame convolution from dy [(b T), S, C_out]: the forward kernel on the packed transposed weight
    (conv3t_n320_weight(conv3t_transposed_weight(weight))), channel roles swapped. PROFILE kind conv3t_dgrad."""
    return conv3t_n320(dy_tok, weight_t_taps, None, T, split=split, kind="conv3t_dgrad")


def conv3t_wgrad_supported(C_in, C_out, dtype):
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_conv3t_wgrad_supported(int(C_in), int(C_out), _DT[dtype]))


def conv3t_wgrad_workspace_bytes(B, T, S, C_in, C_out):
    """> 0: csrc/conv3t_wgrad.hip splits the (video, pixel chunk) units of this shape over blocks (a pure host function of the shape)."""
    return int(_lib.lib().mvi_conv3t_wgrad_workspace_bytes(int(B), int(T), int(S), int(C_in), int(C_out)))


def conv3t_wgrad(tok, dy_tok, T, split=True):
    """dweight, fp32 [C_out, C_in, 3, 1, 1], of the (3, 1, 1) / padding (1, 0, 0) frame convolution from its input tok [(b T), S, C_in]
    and the output gradient dy_tok [(b T), S, C_out] (one 16-bit dtype): csrc/conv3t_wgrad.hip, deterministic. split = False withholds
    the workspace (the unsplit launch). PROFILE kind conv3t_wgrad."""
    L = _lib.lib()
    T = int(T)
    if tok.dim() != 3 or dy_tok.dim() != 3 or tok.shape[:2] != dy_tok.shape[:2] or tok.dtype != dy_tok.dtype or T < 1 or tok.shape[0] % T:
        raise ValueError("conv3t_wgrad: tok [(b T), S, C_in] and dy_tok [(b T), S, C_out] of one dtype expected")
    BT, S, C = tok.shape
    B = BT // T
    Co = dy_tok.shape[2]
    return _conv_wgrad(L.mvi_conv3t_wgrad, L.mvi_conv3t_wgrad_workspace_bytes, (B, T, S, C, Co), tok, dy_tok, (Co, C, 3, 1, 1),
                       "conv3t_wgrad", 2.0 * BT * S * 3 * C * Co, split)


def stem_conv3x3_supported(conv, x):
    """A 3x3 / padding 1 Conv2d of the shapes csrc/stem_conv.hip builds (stride 1: <= 16 -> 16, <= 32 -> 32; stride 2: <= 16 -> 32) on a
    contiguous NCHW half tensor."""
    return (x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float16) and x.is_contiguous() and conv.weight.dtype == x.dtype
            and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) in ((1, 1), (2, 2)) and tuple(conv.padding) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
            and bool(_lib.lib().mvi_stem_conv3x3_supported(int(conv.in_channels), int(conv.out_channels), int(x.shape[3]), int(conv.stride[0]),
                                                           _DT[x.dtype])))


def _stem_packed_weight(weight, W, stride):
    """The weight in the kernel's fragment order (mvi_stem_conv3x3_pack), once per parameter version and stride."""
    def pack(weight):
        L = _lib.lib()
        Co, Ci = weight.shape[0], weight.shape[1]
        wc = weight.detach().contiguous()
        packed = torch.empty(int(L.mvi_stem_conv3x3_packed_bytes(Ci, Co, int(stride))), dtype=torch.uint8, device=weight.device)
        with torch.cuda.device(weight.device):
            _check(L.mvi_stem_conv3x3_pack(wc.data_ptr(), packed.data_ptr(), Ci, Co, int(W), int(stride), _DT[weight.dtype], _stream(weight.device)),
                   "stem_conv3x3_pack")
        return packed
    return derived1(("stem_packed", int(stride)), weight, pack)


def stem_conv3x3_silu(x, weight, bias, silu=True, stride=1):
    """silu(conv2d(x, weight, bias, stride, padding=1)) in one kernel; x [N, C_in, H, W], weight [C_out, C_in, 3, 3]."""
    L = _lib.lib()
    N, Cin, H, W = x.shape
    wc = _stem_packed_weight(weight, W, stride)
    b = None if bias is None else _f32(bias)
    y = torch.empty(N, weight.shape[0], (H - 1) // stride + 1, (W - 1) // stride + 1, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _Timed("stem_conv", float(x.numel() + y.numel()) * x.element_size(), x.device):
        _check(L.mvi_stem_conv3x3_silu(x.data_ptr(), wc.data_ptr(), _ptr(b), y.data_ptr(), N, Cin, weight.shape[0], H, W, int(stride),
                                       int(bool(silu)), _DT[x.dtype], _stream(x.device)), "stem_conv3x3_silu")
    return y


# ---- the hint-stem layers under autograd (ops._StemConvSiluFn): dz on the forward kernel's second epilogue, wgrad + dbias in
# csrc/stem_conv_bwd.hip, the stride-1 C -> C input gradient on the forward kernel with the transposed weight --------------------------

def stem_conv3x3_bwd_supported(C_in, C_out, W, stride, dtype):
    """The shapes csrc/stem_conv.hip's dz epilogue and csrc/stem_conv_bwd.hip take: the forward's 16- and 32-output forms."""
    return dtype in (torch.bfloat16, torch.float16) and bool(
        _lib.lib().mvi_stem_conv3x3_bwd_supported(int(C_in), int(C_out), int(W), int(stride), _DT[dtype]))


def stem_conv3x3_transposed_weight(weight):
    """The weight whose 3x3 / padding 1 / stride 1 convolution of dz is the input gradient of conv(x, weight):
    W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx], as a view [C_in, C_out, 3, 3]. Pure torch; loads no library."""
    return weight.flip(2, 3).transpose(0, 1)


def _stem_out_shape(x, weight, stride):
    N, _, H, W = x.shape
    return N, weight.shape[0], (H - 1) // stride + 1, (W - 1) // stride + 1


def stem_conv3x3_dz(x, weight, bias, dy, silu=True, stride=1, with_y=False):
    """dz = dy * silu'(conv2d(x, weight, bias, stride, padding=1)) with z recomputed in the forward kernel (silu=False: dz = dy);
    x [N, C_in, H, W], dy [N, C_out, H_out, W_out] -> dz like dy. with_y: (dz, y), y the forward's output from the same launch.
    PROFILE kind stem_conv_dz."""
    L = _lib.lib()
    N, Cin, H, W = x.shape
    if dy.dtype != x.dtype or tuple(dy.shape) != _stem_out_shape(x, weight, stride):
        raise ValueError("stem_conv3x3_dz: dy [N, C_out, H_out, W_out] in x's dtype expected")
    wc = _stem_packed_weight(weight, W, stride)
    b = None if bias is None else _f32(bias)
    xc, dc = _aligned(x), _aligned(dy)
    dz = torch.empty_like(dc)
    y = torch.empty_like(dc) if with_y else None
    with torch.cuda.device(x.device), _Timed("stem_conv_dz", float(x.numel() + 2 * dz.numel()) * x.element_size(), x.device):
        _check(L.mvi_stem_conv3x3_dz(xc.data_ptr(), wc.data_ptr(), _ptr(b), dc.data_ptr(), dz.data_ptr(), _ptr(y), N, Cin, weight.shape[0], H, W,
                                     int(stride), int(bool(silu)), _DT.get(x.dtype, -1), _stream(x.device)), "stem_conv3x3_dz")
    return (dz, y) if with_y else dz


def stem_conv3x3_wgrad_workspace_bytes(N, C_in, C_out, H, W, stride=1):
    """Bytes of fp32 partials csrc/stem_conv_bwd.hip writes for this shape: a pure host function of the shape, bounded by its grid."""
    return int(_lib.lib().mvi_stem_conv3x3_wgrad_workspace_bytes(int(N), int(C_in), int(C_out), int(H), int(W), int(stride)))


def stem_conv3x3_wgrad(x, dz, stride=1, need_dbias=True):
    """(dweight fp32 [C_out, C_in, 3, 3], dbias fp32 [C_out] or None) of conv2d(x, weight, bias, stride, padding=1) from its input
    x [N, C_in, H, W] and the pre-activation gradient dz [N, C_out, H_out, W_out] (one 16-bit dtype): csrc/stem_conv_bwd.hip,
    deterministic. PROFILE kind stem_conv_wgrad."""
    L = _lib.lib()
    if x.dim() != 4 or dz.dim() != 4 or x.dtype != dz.dtype or x.shape[0] != dz.shape[0]:
        raise ValueError("stem_conv3x3_wgrad: x [N, C_in, H, W] and dz [N, C_out, H_out, W_out] of one dtype expected")
    N, Cin, H, W = x.shape
    Co = dz.shape[1]
    if tuple(dz.shape[2:]) != ((H - 1) // stride + 1, (W - 1) // stride + 1):
        raise ValueError("stem_conv3x3_wgrad: dz does not have the convolution's output size")
    xc, dc = _aligned(x), _aligned(dz)
    dw = torch.empty(Co, Cin, 3, 3, dtype=torch.float32, device=x.device)
    db = torch.empty(Co, dtype=torch.float32, device=x.device) if need_dbias else None
    ws_bytes = int(L.mvi_stem_conv3x3_wgrad_workspace_bytes(N, Cin, Co, H, W, int(stride)))
    ws = _workspace(x.device, ws_bytes) if ws_bytes else None
    with torch.cuda.device(x.device), _Timed("stem_conv_wgrad", float(x.numel() + dz.numel()) * x.element_size(), x.device):
        _check(L.mvi_stem_conv3x3_wgrad(xc.data_ptr(), dc.data_ptr(), dw.data_ptr(), _ptr(db), N, Cin, Co, H, W, int(stride), _DT.get(x.dtype, -1),
                                        _ptr(ws), ws_bytes, _stream(x.device)), "stem_conv3x3_wgrad")
    return dw, db


def stem_conv3x3_dgrad(dz, weight):
    """dx [N, C, H, W] of the stride-1 convolution with C_in == C_out = C in (16, 32) from dz [N, C, H, W]: the forward kernel on the
    packed transposed weight, no bias, no SiLU. The packed weight is kept in svd/derived.py's table while the weight is frozen and built
    from the live tensor while it trains. PROFILE kind stem_conv_dgrad."""
    L = _lib.lib()
    N, C_, H, W = dz.shape
    if tuple(weight.shape) != (C_, C_, 3, 3) or C_ not in (16, 32) or weight.dtype != dz.dtype:
        raise ValueError("stem_conv3x3_dgrad: dz [N, C, H, W] and weight [C, C, 3, 3] of one dtype, C in (16, 32), expected")

    def pack(w):
        wt = stem_conv3x3_transposed_weight(w.detach()).contiguous()
        packed = torch.empty(int(L.mvi_stem_conv3x3_packed_bytes(C_, C_, 1)), dtype=torch.uint8, device=w.device)
        with torch.cuda.device(w.device):
            _check(L.mvi_stem_conv3x3_pack(wt.data_ptr(), packed.data_ptr(), C_, C_, int(W), 1, _DT[w.dtype], _stream(w.device)), "stem_conv3x3_pack")
        return packed
    wp = pack(weight) if weight.requires_grad else derived1(("stem_packed_transposed", 1), weight, pack)
    dc = _aligned(dz)
    dx = torch.empty_like(dc)
    with torch.cuda.device(dz.device), _Timed("stem_conv_dgrad", 2.0 * dz.numel() * dz.element_size(), dz.device):
        _check(L.mvi_stem_conv3x3_silu(dc.data_ptr(), wp.data_ptr(), None, dx.data_ptr(), N, C_, C_, H, W, 1, 0, _DT.get(dz.dtype, -1),
                                       _stream(dz.device)), "stem_conv3x3_dgrad")
    return dx


def bias_residual_add(h, bias, x):
    L = _lib.lib()
    if h.dtype not in _DT:
        raise TypeError(f"bias_residual_add: unsupported dtype {h.dtype}")
    hc = _contig(h)
    xc = None
    if x is not None:
        if x.shape != h.shape or x.dtype != h.dtype:
            raise ValueError("bias_residual_add: x must match h in shape and dtype")
        xc = _contig(x)
    N, Cc = hc.shape[0], hc.shape[1]
    S = hc.numel() // max(N * Cc, 1)
    b = None if bias is None else _f32(bias)
    out = torch.empty_like(hc)
    with torch.cuda.device(h.device), _Timed("bias_residual", (2.0 + (x is not None)) * hc.numel() * hc.element_size(), h.device):
        _check(L.mvi_bias_residual_add(hc.data_ptr(), _ptr(xc), _ptr(b), out.data_ptr(), N, Cc, S, _DT[h.dtype], _stream(h.device)),
                                       "bias_residual_add")
    return out


def concat_add(h, skip, ctrl):
    """cat([h, skip + ctrl], dim=1) in one pass; ctrl may be None. All operands contiguous [N, C, *spatial], one dtype."""
    L = _lib.lib()
    if h.dtype not in _DT or skip.dtype != h.dtype or (ctrl is not None and ctrl.dtype != h.dtype):
        raise TypeError("concat_add: operands must share a supported dtype")
    if skip.shape[0] != h.shape[0] or skip.shape[2:] != h.shape[2:] or (ctrl is not None and ctrl.shape != skip.shape):
        raise ValueError("concat_add: shapes do not line up")
    if not (h.is_contiguous() and skip.is_contiguous() and (ctrl is None or ctrl.is_contiguous())):
        raise ValueError("concat_add: operands must be contiguous")
    N, C1, C2 = h.shape[0], h.shape[1], skip.shape[1]
    S = h.numel() // max(N * C1, 1) if C1 else skip.numel() // max(N * C2, 1)
    out = torch.empty((N, C1 + C2, *h.shape[2:]), dtype=h.dtype, device=h.device)
    nbytes = (2.0 * h.numel() + (2.0 + (ctrl is not None)) * skip.numel()) * h.element_size()
    with torch.cuda.device(h.device), _Timed("concat_add", nbytes, h.device):
        _check(L.mvi_concat_add(h.data_ptr(), skip.data_ptr(), _ptr(ctrl), out.data_ptr(), N, C1, C2, S, _DT[h.dtype], _stream(h.device)),
                                "concat_add")
    return out


def bias_residual_blend(h, bias, x, alpha):
    """x + (1 - alpha[n]) * (h + bias[c]); alpha: [N] (any float dtype), one blend factor per sample of h [N, C, *spatial]."""
    L = _lib.lib()
    if h.dtype not in _DT:
        raise TypeError(f"bias_residual_blend: unsupported dtype {h.dtype}")
    if x.shape != h.shape or x.dtype != h.dtype:
        raise ValueError("bias_residual_blend: x must match h in shape and dtype")
    if alpha.numel() != h.shape[0]:
        raise ValueError(f"bias_residual_blend: alpha has {alpha.numel()} entries for {h.shape[0]} samples")
    hc = _contig(h)
    xc = _contig(x)
    N, Cc = hc.shape[0], hc.shape[1]
    S = hc.numel() // max(N * Cc, 1)
    b = None if bias is None else _f32(bias)
    a = alpha.detach().reshape(-1).float().contiguous()
    out = torch.empty_like(hc)
    with torch.cuda.device(h.device), _Timed("bias_residual", 3.0 * hc.numel() * hc.element_size(), h.device):
        _check(L.mvi_bias_residual_blend(hc.data_ptr(), xc.data_ptr(), _ptr(b), a.data_ptr(), out.data_ptr(), N, Cc, S, _DT[h.dtype],
                                         _stream(h.device)), "bias_residual_blend")
    return out


def bias_silu(h, bias):
    """silu(h + bias[c]) for h [N, C, *spatial], in place on h's (contiguous) memory."""
    L = _lib.lib()
    if h.dtype not in _DT:
        raise TypeError(f"bias_silu: unsupported dtype {h.dtype}")
    hc = _contig(h)
    N, Cc = hc.shape[0], hc.shape[1]
    S = hc.numel() // max(N * Cc, 1)
    b = None if bias is None else _f32(bias)
    with torch.cuda.device(h.device), _Timed("bias_silu", 2.0 * hc.numel() * hc.element_size(), h.device):
        _check(L.mvi_bias_silu(hc.data_ptr(), _ptr(b), hc.data_ptr(), N, Cc, S, _DT[h.dtype], _stream(h.device)), "bias_silu")
    return hc


def layernorm_supported(C_, dtype):
    return dtype in _DT and bool(_lib.lib().mvi_layernorm_supported(int(C_), _DT[dtype]))


def add_layer_norm(x, weight, bias, eps, h=None, row=None, ret_pre=False):
    """x [..., C] contiguous; returns (y, s, s_pre): s_pre = x + h, s = s_pre + row (broadcast over equal runs of
    rows), y = LayerNorm(s). s is None when neither h nor row is given; s_pre only when ret_pre and h."""
    L = _lib.lib()
    if x.dtype not in _DT:
        raise TypeError(f"add_layer_norm: unsupported dtype {x.dtype}")
    Cc = x.shape[-1]
    xc = _contig(x)
    R = xc.numel() // Cc
    hc = rc = None
    row_div = 1
    if h is not None:
        if h.shape != x.shape or h.dtype != x.dtype:
            raise ValueError("add_layer_norm: h must match x in shape and dtype")
        hc = _contig(h)
    if row is not None:
        if row.dtype != x.dtype or row.shape[-1] != Cc:
            raise ValueError("add_layer_norm: row must be [G, C] / [G, 1, C] of x's dtype")
        rc = row.reshape(-1, Cc)
        rc = _contig(rc)
        G = rc.shape[0]
        if G == 0 or R % G:
            raise ValueError(f"add_layer_norm: {R} rows do not split into {G} equal runs")
        row_div = R // G
    y = torch.empty_like(xc)
    s = torch.empty_like(xc) if (hc is not None or rc is not None) else None
    s_pre = torch.empty_like(xc) if (ret_pre and hc is not None and rc is not None) else None
    n_io = 2 + (hc is not None) + (s is not None) + (s_pre is not None)
    with torch.cuda.device(x.device), _Timed("add_layernorm", float(n_io) * xc.numel() * xc.element_size(), x.device):
        _check(L.mvi_add_layernorm(xc.data_ptr(), _ptr(hc), _ptr(rc), row_div, _f32(weight).data_ptr(), _f32(bias).data_ptr(), _ptr(s_pre), _ptr(s),
                                   y.data_ptr(), R, Cc, float(eps), _DT[x.dtype], _stream(x.device)), "add_layer_norm")
    if ret_pre and s_pre is None:                  # no separate buffer needed: s_pre coincides with x or with s
        s_pre = xc if hc is None else s
    return y, s, s_pre


LNB_GRAD, LNB_PARAMS, LNB_DROW = 1, 2, 4       # MVI_LNB_* of include/mvi_unet_ops.h


def add_layer_norm_backward_supported(C_, dtype):
    """Whether add_layer_norm_backward computes this width (mvi_add_layernorm_backward_supported, host-only: layernorm_supported's gate)."""
    return dtype in _DT and bool(_lib.lib().mvi_add_layernorm_backward_supported(int(C_), _DT[dtype]))


def add_layer_norm_backward_workspace_bytes(R, C_, row_div, need_dparams, need_drow):
    """Bytes of the fp32 partial rows add_layer_norm_backward needs for these outputs (0 without column sums)."""
    flags = LNB_GRAD | (LNB_PARAMS if need_dparams else 0) | (LNB_DROW if need_drow else 0)
    return int(_lib.lib().mvi_add_layernorm_backward_workspace_bytes(int(R), int(C_), int(row_div), flags))


def add_layer_norm_backward(s, weight, eps, gy=None, gs=None, gs_pre=None, row_groups=None, need_dx=True, need_dparams=True):
    """(g, dweight, dbias, drow) of (y, s, s_pre) = add_layer_norm(x, weight, bias, eps, h, row) for the upstream gradients gy, gs,
    gs_pre of its three outputs, each optional (csrc/layernorm_bwd.hip). s [..., C]: the forward's s (x for the plain norm). g, in
    s's dtype and shape, is the gradient of x AND of h (one tensor); dweight, dbias fp32 [C]; drow fp32 [row_groups, C], asked for by
    giving row_groups (the G of the forward's row). Outputs not asked for are None and cost nothing. Deterministic."""
    L = _lib.lib()
    if s.dtype not in _DT:
        raise TypeError(f"add_layer_norm_backward: unsupported dtype {s.dtype}")
    Cc = s.shape[-1]
    sc = _contig(s)
    R = sc.numel() // Cc
    grads = []
    for name, g in (("gy", gy), ("gs", gs), ("gs_pre", gs_pre)):
        if g is not None:
            if g.shape != s.shape or g.dtype != s.dtype:
                raise ValueError(f"add_layer_norm_backward: {name} must match s in shape and dtype")
            g = _contig(g)
        grads.append(g)
    row_div = 1
    if row_groups is not None:
        if row_groups <= 0 or R % row_groups:
            raise ValueError(f"add_layer_norm_backward: {R} rows do not split into {row_groups} equal runs")
        row_div = R // row_groups
    f32 = dict(dtype=torch.float32, device=s.device)
    g_out = torch.empty_like(sc) if need_dx else None
    dw = torch.empty(Cc, **f32) if need_dparams else None
    db = torch.empty(Cc, **f32) if need_dparams else None
    drow = torch.empty((row_groups, Cc), **f32) if row_groups is not None else None
    if R == 0 or not (need_dx or need_dparams or drow is not None):
        for t in (dw, db, drow):
            if t is not None:
                t.zero_()
        return g_out, dw, db, drow
    flags = (LNB_GRAD if need_dx else 0) | (LNB_PARAMS if need_dparams else 0) | (LNB_DROW if drow is not None else 0)
    nbytes = int(L.mvi_add_layernorm_backward_workspace_bytes(R, Cc, row_div, flags))
    ws = _workspace(s.device, nbytes) if nbytes else None
    n_io = 1 + sum(g is not None for g in grads) + bool(need_dx)
    with torch.cuda.device(s.device), _Timed("add_layernorm_bwd", float(n_io) * sc.numel() * sc.element_size(), s.device):
        _check(L.mvi_add_layernorm_backward(_ptr(grads[0]), sc.data_ptr(), _ptr(grads[1]), _ptr(grads[2]), _f32(weight).data_ptr(), row_div,
                                            float(eps), _ptr(g_out), _ptr(dw), _ptr(db), _ptr(drow), _ptr(ws), 0 if ws is None else ws.numel(), R, Cc,
                                            _DT[s.dtype], _stream(s.device)), "add_layer_norm_backward")
    return g_out, dw, db, drow


def add_lerp(x, h, base, alpha):
    """lerp(x + h, base, alpha) with alpha [G] fp32 broadcast over equal runs of the rows of x [..., C]."""
    L = _lib.lib()
    if x.dtype not in _DT or base.dtype != x.dtype or base.shape != x.shape:
        raise TypeError("add_lerp: x and base must share shape and a supported dtype")
    Cc = x.shape[-1]
    xc = _contig(x)
    bc = _contig(base)
    hc = None
    if h is not None:
        if h.shape != x.shape or h.dtype != x.dtype:
            raise ValueError("add_lerp: h must match x in shape and dtype")
        hc = _contig(h)
    R = xc.numel() // Cc
    al = alpha.detach().reshape(-1).float().contiguous()
    G = al.numel()
    if G == 0 or R % G:
        raise ValueError(f"add_lerp: {R} rows do not split into {G} equal runs")
    out = torch.empty_like(xc)
    with torch.cuda.device(x.device), _Timed("add_lerp", (3.0 + (hc is not None)) * xc.numel() * xc.element_size(), x.device):
        _check(L.mvi_add_lerp(xc.data_ptr(), _ptr(hc), bc.data_ptr(), al.data_ptr(), R // G, out.data_ptr(), R, Cc, _DT[x.dtype], _stream(x.device)),
                              "add_lerp")
    return out


def tokens_to_planes_add(tok, x_in, bias=None, spatial=None):
    """tok [N, S, C] (+ bias[c]) + x_in [N, C, *spatial] -> [N, C, *spatial]; x_in None: the layout change alone, into `spatial`."""
    L = _lib.lib()
    if tok.dtype not in _DT or (x_in is not None and x_in.dtype != tok.dtype):
        raise TypeError("tokens_to_planes_add: tok and x_in must share a supported dtype")
    N, S, Cc = tok.shape
    if x_in is None:
        if spatial is None or math.prod(int(v) for v in spatial) != S:
            raise ValueError("tokens_to_planes_add: without x_in, `spatial` must be given and multiply to the token count")
        xc, out = None, torch.empty(N, Cc, *spatial, dtype=tok.dtype, device=tok.device)
    else:
        if x_in.shape[0] != N or x_in.shape[1] != Cc or x_in.numel() != tok.numel():
            raise ValueError(f"tokens_to_planes_add: tok {tuple(tok.shape)} does not match x_in {tuple(x_in.shape)}")
        xc = _contig(x_in)
        out = torch.empty_like(xc)
    tc = _contig(tok)
    xp = _ptr(xc)
    with torch.cuda.device(tok.device), _Timed("tokens_to_planes_add", (2.0 + (xc is not None)) * tc.numel() * tc.element_size(), tok.device):
        if bias is None:
            _check(L.mvi_tokens_to_planes_add(tc.data_ptr(), xp, out.data_ptr(), N, Cc, S, _DT[tok.dtype],
                                              _stream(tok.device)), "tokens_to_planes_add")
        else:
            _check(L.mvi_tokens_to_planes_add_bias(tc.data_ptr(), xp, _f32(bias).data_ptr(), out.data_ptr(), N, Cc, S,
                                                   _DT[tok.dtype], _stream(tok.device)), "tokens_to_planes_add")
    return out


def planes_add_to_tokens(x, tok, bias=None):
    """x [N, C, *spatial] + tok [N, S, C] (+ bias[c]) -> tokens [N, S, C]: a ResBlock's last add, result token-major."""
    L = _lib.lib()
    if x.dtype not in _DT or tok.dtype != x.dtype:
        raise TypeError("planes_add_to_tokens: x and tok must share a supported dtype")
    N, S, Cc = tok.shape
    if x.shape[0] != N or x.shape[1] != Cc or x.numel() != tok.numel():
        raise ValueError(f"planes_add_to_tokens: x {tuple(x.shape)} does not match tok {tuple(tok.shape)}")
    xc = _contig(x)
    tc = _contig(tok)
    out = torch.empty_like(tc)
    with torch.cuda.device(x.device), _Timed("planes_add_to_tokens", 3.0 * tc.numel() * tc.element_size(), x.device):
        _check(L.mvi_planes_add_to_tokens(xc.data_ptr(), tc.data_ptr(), None if bias is None else _f32(bias).data_ptr(), out.data_ptr(), N, Cc, S,
                                          _DT[x.dtype], _stream(x.device)), "planes_add_to_tokens")
    return out


def tokens_blend_to_planes(tok, base, bias, alpha, spatial):
    """base + (1 - alpha[n]) * (tok + bias[c]) for token-major tok, base [N, S, C] -> [N, C, *spatial]; alpha [N]."""
    L = _lib.lib()
    if tok.dtype not in _DT or base.dtype != tok.dtype or base.shape != tok.shape:
        raise TypeError("tokens_blend_to_planes: tok and base must share shape and a supported dtype")
    N, S, Cc = tok.shape
    if math.prod(int(v) for v in spatial) != S or alpha.numel() != N:
        raise ValueError("tokens_blend_to_planes: `spatial` must multiply to the token count and alpha hold one value per sample")
    tc = _contig(tok)
    bc = _contig(base)
    a = alpha.detach().reshape(N).float().contiguous()
    out = torch.empty(N, Cc, *spatial, dtype=tok.dtype, device=tok.device)
    with torch.cuda.device(tok.device), _Timed("tokens_blend_to_planes", 3.0 * tc.numel() * tc.element_size(), tok.device):
        _check(L.mvi_tokens_blend_to_planes(tc.data_ptr(), bc.data_ptr(), None if bias is None else _f32(bias).data_ptr(), a.data_ptr(),
                                            out.data_ptr(), N, Cc, S, _DT[tok.dtype], _stream(tok.device)), "tokens_blend_to_planes")
    return out


def planes_to_tokens(x, upsample=1):
    """x [N, C, H, W] -> tokens [N, H W, C]; upsample = 2: nearest-neighbour 2x upsampling folded in -> [N, (2H)(2W), C]."""
    L = _lib.lib()
    if x.dtype not in _DT or x.dim() != 4:
        raise TypeError("planes_to_tokens: [N, C, H, W] of a supported dtype expected")
    N, Cc, H, W = x.shape
    xc = _contig(x)
    out = torch.empty(N, H * W * upsample * upsample, Cc, dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _Timed("planes_to_tokens", float(xc.numel() + out.numel()) * x.element_size(), x.device):
        _check(L.mvi_planes_to_tokens(xc.data_ptr(), out.data_ptr(), N, Cc, H, W, int(upsample), _DT[x.dtype], _stream(x.device)),
               "planes_to_tokens")
    return out


# ---- the block tails under autograd (ops._TokensToPlanesAddFn, _TokensBlendToPlanesFn, _AddLerpFn): csrc/block_tails_bwd.hip --------------
TAILS_DTOK, TAILS_DBASE, TAILS_DBIAS, TAILS_DALPHA = 1, 2, 4, 8


def block_tails_backward_supported(C, S, dtype):
    """Whether planes_tail_backward takes dy [N, C, S] (rows_tail_backward: dy [R, C], any S that is a multiple of 8, e.g. 8): the
    forward tails' own conditions in bf16 / f16 (host-only)."""
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().mvi_block_tails_backward_supported(int(C), int(S), _DT[dtype]))


def planes_tail_backward_workspace_bytes(N, C, S, flags):
    return int(_lib.lib().mvi_planes_tail_backward_workspace_bytes(int(N), int(C), int(S), int(flags)))


def planes_tail_backward(dy, alpha=None, tok=None, bias=None, need_dtok=True, need_dbase=False, need_dbias=False):
    """(d_tok, d_base, dbias, dalpha) of out = tokens_to_planes_add(tok, x_in, bias) (alpha None) or of
    out = tokens_blend_to_planes(tok, base, bias, alpha, spatial) for the upstream gradient dy [N, C, *spatial] (a 16-bit dtype):
    d_tok [N, S, C] = (1 - alpha[n]) dy^T, d_base [N, S, C] = dy^T (with alpha only), dbias fp32 [C] = sum_n (1 - alpha[n]) sum_p dy,
    dalpha fp32 [N] = -sum dy (tok + bias) — computed when tok [N, S, C] is given (bias, optional, is read only there). Outputs not
    asked for are None and cost nothing; the gradient of x_in is dy itself. Deterministic. PROFILE kinds planes_tail_bwd, and
    tails_reduce when a sum was asked for."""
    L = _lib.lib()
    if dy.dtype not in (torch.bfloat16, torch.float16) or dy.dim() < 3:
        raise TypeError("planes_tail_backward: dy [N, C, *spatial] in bf16 or f16 expected")
    N, Cc = int(dy.shape[0]), int(dy.shape[1])
    S = math.prod(int(v) for v in dy.shape[2:])
    if need_dbase and alpha is None:
        raise ValueError("planes_tail_backward: d_base belongs to the blend (alpha)")
    if tok is not None and (alpha is None or tok.dtype != dy.dtype or tuple(tok.shape) != (N, S, Cc)):
        raise ValueError("planes_tail_backward: dalpha needs alpha and tok [N, S, C] in dy's dtype")
    if alpha is not None and alpha.numel() != N:
        raise ValueError("planes_tail_backward: alpha must hold one value per sample")
    dc = _contig(dy)
    tc = None if tok is None else _contig(tok)
    al = None if alpha is None else alpha.detach().reshape(N).float().contiguous()
    bf = None if (bias is None or tok is None) else _f32(bias)
    f32 = dict(dtype=torch.float32, device=dy.device)
    d_tok = torch.empty(N, S, Cc, dtype=dy.dtype, device=dy.device) if need_dtok else None
    d_base = torch.empty(N, S, Cc, dtype=dy.dtype, device=dy.device) if need_dbase else None
    dbias = torch.empty(Cc, **f32) if need_dbias else None
    dalpha = torch.empty(N, **f32) if tok is not None else None
    flags = (TAILS_DTOK if need_dtok else 0) | (TAILS_DBASE if need_dbase else 0) | (TAILS_DBIAS if need_dbias else 0) \
        | (TAILS_DALPHA if tok is not None else 0)
    if N == 0 or S == 0 or not flags:
        for t in (dbias, dalpha):
            if t is not None:
                t.zero_()
        return d_tok, d_base, dbias, dalpha
    nbytes = int(L.mvi_planes_tail_backward_workspace_bytes(N, Cc, S, flags))
    ws = _workspace(dy.device, nbytes) if nbytes else None
    n_io = 1 + bool(need_dtok) + bool(need_dbase) + (tok is not None)
    sums = flags & (TAILS_DBIAS | TAILS_DALPHA)
    with torch.cuda.device(dy.device):
        with _Timed("planes_tail_bwd", float(n_io) * dc.numel() * dc.element_size() + nbytes, dy.device):
            _check(L.mvi_planes_tail_backward(dc.data_ptr(), _ptr(al), _ptr(tc), _ptr(d_tok), _ptr(d_base), sums, _ptr(ws), nbytes, N, Cc, S,
                                              _DT[dy.dtype], _stream(dy.device)), "planes_tail_backward")
        if sums:
            with _Timed("tails_reduce", float(nbytes) + 4.0 * (Cc * (1 + (bf is not None)) + 2 * N), dy.device):
                _check(L.mvi_planes_tail_reduce(ws.data_ptr(), nbytes, _ptr(al), _ptr(bf), _ptr(dbias), _ptr(dalpha), N, Cc, S, _stream(dy.device)),
                       "planes_tail_reduce")
    return d_tok, d_base, dbias, dalpha


def rows_tail_backward_workspace_bytes(R, C, row_div, need_dalpha=True):
    return int(_lib.lib().mvi_rows_tail_backward_workspace_bytes(int(R), int(C), int(row_div), TAILS_DALPHA if need_dalpha else 0))


def rows_tail_backward(dy, alpha, x=None, h=None, base=None, need_dt=True, need_dbase=True):
    """(d_t, d_base, dalpha) of out = add_lerp(x, h, base, alpha) for the upstream gradient dy [..., C] (a 16-bit dtype), alpha [G]
    over equal runs of rows: d_t = (1 - alpha[g]) dy (the gradient of x AND of h, one tensor), d_base = alpha[g] dy, dalpha fp32 [G] =
    sum dy (base - round(x + h)) — computed when x and base are given (h optional). Outputs not asked for are None. Deterministic.
    PROFILE kinds rows_tail_bwd, and tails_reduce with dalpha."""
    L = _lib.lib()
    if dy.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("rows_tail_backward: dy in bf16 or f16 expected")
    Cc = int(dy.shape[-1])
    dc = _contig(dy)
    R = dc.numel() // Cc if Cc else 0
    al = alpha.detach().reshape(-1).float().contiguous()
    G = al.numel()
    if G == 0 or R % G:
        raise ValueError(f"rows_tail_backward: {R} rows do not split into {G} equal runs")
    want_da = x is not None and base is not None
    ins = []
    for name, t in (("x", x), ("h", h), ("base", base)):
        if t is not None and want_da:
            if t.shape != dy.shape or t.dtype != dy.dtype:
                raise ValueError(f"rows_tail_backward: {name} must match dy in shape and dtype")
            t = _contig(t)
        ins.append(t if want_da else None)
    d_t = torch.empty_like(dc) if need_dt else None
    d_base = torch.empty_like(dc) if need_dbase else None
    dalpha = torch.empty(G, dtype=torch.float32, device=dy.device) if want_da else None
    if R == 0 or not (need_dt or need_dbase or want_da):
        if dalpha is not None:
            dalpha.zero_()
        return d_t, d_base, dalpha
    row_div = R // G
    nbytes = int(L.mvi_rows_tail_backward_workspace_bytes(R, Cc, row_div, TAILS_DALPHA if want_da else 0))
    ws = _workspace(dy.device, nbytes) if nbytes else None
    n_io = 1 + bool(need_dt) + bool(need_dbase) + sum(t is not None for t in ins)
    sums = TAILS_DALPHA if want_da else 0
    with torch.cuda.device(dy.device):
        with _Timed("rows_tail_bwd", float(n_io) * dc.numel() * dc.element_size() + nbytes, dy.device):
            _check(L.mvi_rows_tail_backward(dc.data_ptr(), al.data_ptr(), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(d_t), _ptr(d_base),
                                            sums, _ptr(ws), nbytes, R, Cc, row_div, _DT[dy.dtype], _stream(dy.device)), "rows_tail_backward")
        if sums:
            with _Timed("tails_reduce", float(nbytes) + 4.0 * G, dy.device):
                _check(L.mvi_rows_tail_reduce(ws.data_ptr(), nbytes, dalpha.data_ptr(), R, Cc, row_div, _stream(dy.device)), "rows_tail_reduce")
    return d_t, d_base, dalpha


def group_norm_tok2tok_supported(N, C_, S, groups, dtype):
    """Whether group_norm_silu_tok2tok takes t [N, S, C] with `groups` groups: the kernel has geometry limits of its own (rows per launch,
    groups, its row pass in LDS)."""
    return _lib.lib().mvi_groupnorm_tok2tok_workspace_bytes(int(N), int(C_), int(S), int(groups), _DT[dtype]) != 0


def _gn_tok2tok_forward(what, t, num_groups, weight, bias, eps, silu, chan_bias, frames, want_stats, kind, work, partials=None):
    """The one forward of token-major t [N, S, C] (mvi_groupnorm_tok2tok_forward; with `partials`, mvi_groupnorm_silu_tok2tok_pre):
    (y, stats), stats the fp32 (mean, rstd) table [N / frames * groups, 2] when want_stats, else None — the same launches and y either way."""
    L = _lib.lib()
    tc, N, Cc, S, cb = _tok2tok_args(what, t, chan_bias, frames)
    nbytes = L.mvi_groupnorm_tok2tok_workspace_bytes(N, Cc, S, num_groups, _DT[t.dtype])
    if nbytes == 0:
        raise ValueError(f"{what}: unsupported shape {tuple(t.shape)} / {num_groups} groups")
    y = torch.empty_like(tc)
    stats = torch.empty((N // frames * num_groups, 2), dtype=torch.float32, device=t.device) if want_stats else None
    ws = _workspace(tc.device, nbytes)
    head = (tc.data_ptr(), y.data_ptr(), _f32(weight).data_ptr(), _f32(bias).data_ptr(), _ptr(cb))
    dims = (N, int(frames), Cc, S, num_groups, float(eps), int(bool(silu)), _DT[t.dtype])
    with torch.cuda.device(tc.device), _Timed(kind, work * tc.numel() * tc.element_size(), tc.device):
        if partials is None:
            _check(L.mvi_groupnorm_tok2tok_forward(*head, _ptr(stats), *dims, ws.data_ptr(), ws.numel(), _stream(tc.device)), what)
        else:
            _check(L.mvi_groupnorm_silu_tok2tok_pre(*head, *dims, partials.part.data_ptr(), partials.chunks, ws.data_ptr(), ws.numel(),
                                                    _stream(tc.device)), what + " (pre)")
    return y, stats


def group_norm_silu_tok2tok(t, num_groups, weight, bias, eps, silu, chan_bias=None, frames=1, partials=None):
    """GroupNorm(+SiLU) of token-major t [N, S, C] -> [N, S, C] (csrc/groupnorm_tokens.hip); frames > 1: statistics over the `frames`
    consecutive samples of a video (the temporal ResBlock's norm), chan_bias still per sample. partials (GnPartials): the statistics
    the producer of t left (same groups, same chan_bias object) — no statistics pass (mvi_groupnorm_silu_tok2tok_pre)."""
    if partials is not None and (partials.groups != num_groups or (partials.chan_bias is None) != (chan_bias is None)
                                 or partials.part.numel() != t.shape[0] * partials.chunks * num_groups * 3):
        raise ValueError("group_norm_tok2tok: the producer's statistics do not belong to this norm")
    return _gn_tok2tok_forward("group_norm_tok2tok", t, num_groups, weight, bias, eps, silu, chan_bias, frames, False, "groupnorm_tok2tok", 2.0,
                               partials)[0]


def group_norm_tok2tok_backward_supported(N, C_, S, num_groups, frames, dtype):
    """Whether group_norm_tok2tok_forward_stats / group_norm_tok2tok_backward compute t [N, S, C] with statistics over videos of
    `frames` samples (mvi_groupnorm_tok2tok_backward_supported, a host-only function; the 16-byte alignment is checked at the call)."""
    if dtype not in _DT or frames <= 0 or num_groups <= 0:
        return False
    return bool(_lib.lib().mvi_groupnorm_tok2tok_backward_supported(int(N), int(frames), int(C_), int(S), int(num_groups), _DT[dtype]))


def group_norm_tok2tok_forward_stats(t, num_groups, weight, bias, eps, silu, chan_bias=None, frames=1):
    """The forward of group_norm_silu_tok2tok (same kernels, y bit-identical) that also returns the fp32 (mean, rstd) of every
    (video, group) [N / frames * groups, 2] for group_norm_tok2tok_backward."""
    return _gn_tok2tok_forward("group_norm_tok2tok_forward_stats", t, num_groups, weight, bias, eps, silu, chan_bias, frames, True,
                               "groupnorm_tok2tok_stats_fwd", 3.0)


def group_norm_tok2tok_backward(dy, t, stats, num_groups, weight, bias, silu, chan_bias=None, frames=1, need_dx=True, need_dparams=False,
                                need_dchan_bias=False):
    """(dx, dweight, dbias, dchan_bias) of the token-major GroupNorm(+SiLU) whose forward returned `stats` (csrc/groupnorm_bwd.hip,
    gn_bwd_tok_*): dx in t's dtype and shape, the others fp32; outputs not asked for are None and cost nothing (need_dparams adds one
    small launch; the PROFILE kind is then "groupnorm_tok2tok_bwd_params" instead of "groupnorm_tok2tok_bwd"). dy: contiguous, t's dtype
    and shape. Deterministic."""
    return _gn_backward("tok2tok", dy, t, stats, frames, num_groups, weight, bias, silu, chan_bias, GN_PLANES, need_dx, need_dparams,
                        need_dchan_bias)


def attention_kernel_variant(Sq, Sk, D, dtype):
    """0 = fp32-math rowtile kernel, 4 / 16 = the 4- / 8-wave MFMA kernel (the function the C dispatch itself uses)."""
    return int(_lib.lib().mvi_attention_kernel_variant(int(Sq), int(Sk), int(D), _DT[dtype]))


def attention_kernel_kind(Sq, Sk, D, dtype):
    return int(_lib.lib().mvi_attention_kernel_kind(Sq, Sk, D, _DT[dtype]))


# ---- Round 6: split-operand convolutions at fp32 accuracy (the first-stage decoder; csrc/linear_n320.hip, mvi_conv3x3_split3_f32) ------

def split_hi_lo(v):
    """fp32 -> (hi, lo) bf16 with hi + lo = v to 16 mantissa bits."""
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


_OPERANDS = {"split3": (3, torch.bfloat16, 0), "bf16": (1, torch.bfloat16, 1), "f16": (1, torch.float16, 2)}    # mode -> (terms, dtype, GN out_mode)


def split3_weight(weight, mode="split3"):
    """A convolution weight ([C_out, C_in, 3, 3] or [C_out, C_in, 3, 1, 1], any float type) for mvi_conv3x3_split3_f32 / mvi_conv3t_split3_f32:
    [C_out padded to whole column groups][taps x terms C_in] in the kernel's contraction order, padding rows zero. mode "split3": bf16
    with the logical channel axis (w_hi | w_lo | w_hi); "bf16" / "f16": the weight rounded once to that type (terms = 1)."""
    terms, dt, _ = _OPERANDS[mode]
    w = weight.detach().float()
    if terms == 3:
        hi, lo = split_hi_lo(w)
        w3 = torch.cat([hi, lo, hi], dim=1)
    else:
        w3 = w.to(dt)
    packed = conv3x3_n320_weight(w3) if w.dim() == 4 else conv3t_n320_weight(w3)
    Co = packed.shape[0]
    group = int(_lib.lib().mvi_conv_split3_group(Co))
    pad = -Co % group
    if pad:
        packed = torch.cat([packed, packed.new_zeros(pad, packed.shape[1])])
    return packed.contiguous()


def group_norm_split(x, num_groups, weight, bias, eps, silu, chan_bias=None, frames=1, mode="split3"):
    """GroupNorm(+SiLU) of fp32 token-major x [N, S, C] -> the operand of conv_split3 in `mode`: split bf16 [N, S, 2 C] = (hi | lo)
    ("split3") or one rounded value per element [N, S, C] ("bf16" / "f16") (mvi_groupnorm_silu_tok2tok_split).
    num_groups = 0: no normalisation, the plain split / rounding."""
    L = _lib.lib()
    terms, dt, out_mode = _OPERANDS[mode]
    if x.dtype != torch.float32 or x.dim() != 3:
        raise TypeError("group_norm_split: fp32 [N, S, C] expected")
    xc = _contig(x)
    N, S, Cc = xc.shape
    y2 = torch.empty(N, S, (2 if terms == 3 else 1) * Cc, dtype=dt, device=x.device)
    ws, nbytes, cb = None, 0, None
    if num_groups:
        nbytes = L.mvi_groupnorm_tok2tok_workspace_bytes(N, Cc, S, num_groups, 0)
        if nbytes == 0:
            raise ValueError(f"group_norm_split: unsupported shape {tuple(x.shape)} / {num_groups} groups")
        ws = _workspace(x.device, nbytes)
        cb = _chan_bias("group_norm_split", chan_bias, N, Cc)
    with torch.cuda.device(x.device), _Timed("groupnorm_split", 2.0 * xc.numel() * 4, x.device):
        _check(L.mvi_groupnorm_silu_tok2tok_split(xc.data_ptr(), y2.data_ptr(), None if not num_groups else _f32(weight).data_ptr(),
                                                  None if not num_groups else _f32(bias).data_ptr(), _ptr(cb), N, int(frames), Cc, S, int(num_groups),
                                                  float(eps), int(bool(silu)), out_mode, _ptr(ws), nbytes, _stream(x.device)), "group_norm_split")
    return y2


def conv_split3(x2, w3, N, H, W, C_out, taps=9, mode="split3", _max_bytes=0xFFFFFFFF):
    """x . w at fp32 accuracy on the bf16 matrix pipe (mode "split3": x2 [N H W, 2 C] split bf16 from group_norm_split, w3 from
    split3_weight) — or with ONE rounded value per operand, fp32 accumulate (modes "bf16" / "f16": x2 [N H W, C]) -> fp32 [N H W, C_out],
    no bias. taps = 9: 3x3 / padding 1 over N images of H x W tokens; taps = 3: (3,1,1) / padding (1,0,0) over N videos of H frames of W
    tokens. The batch is cut so that every launch stays inside the kernel's 32-bit activation offsets."""
    L = _lib.lib()
    terms, dt, _ = _OPERANDS[mode]
    Cx = x2.shape[-1]
    C = Cx // 2 if terms == 3 else Cx
    rows = N * H * W
    if x2.dtype != dt or not x2.is_contiguous() or x2.numel() != rows * Cx or w3.shape[1] != taps * terms * C or w3.dtype != dt:
        raise ValueError(f"conv_split3 ({mode}): x2 contiguous {dt} [N H W, {'2 C' if terms == 3 else 'C'}] and w3 [C_out padded, taps {terms} C] expected")
    x2 = x2.reshape(rows, Cx)
    per = H * W * Cx * 2                                       # bytes of one image / video
    if per > _max_bytes and taps == 3 and W > 1:
        # one video alone exceeds the offsets (e.g. 25 frames of 576 x 1024 at 128 channels): the (3,1,1) convolution is independent
        # per pixel, so the pixel axis is cut (contiguous copies of the slices in, strided copies out: two extra passes, rare)
        parts = -(-per // _max_bytes)
        step = -(-W // parts)
        res = torch.empty(N, H, W, C_out, dtype=torch.float32, device=x2.device)
        xv = x2.view(N, H, W, Cx)
        for w0 in range(0, W, step):
            w1 = min(W, w0 + step)
            res[:, :, w0:w1] = conv_split3(xv[:, :, w0:w1].contiguous().view(-1, Cx), w3, N, H, w1 - w0, C_out, taps=3, mode=mode,
                                           _max_bytes=_max_bytes).view(N, H, w1 - w0, C_out)
        return res.view(rows, C_out)
    n_max = max(1, (_max_bytes // per))
    if per > 0xFFFFFFFF:
        raise ValueError("conv_split3: one image exceeds the kernel's 32-bit activation offsets")
    cap = int(L.mvi_conv_split3_out_rows(rows)) + 256
    out = torch.empty(cap, C_out, dtype=torch.float32, device=x2.device)
    fn = L.mvi_conv3x3_split3_f32 if taps == 9 else L.mvi_conv3t_split3_f32
    with torch.cuda.device(x2.device), _Timed("conv_split3", 2.0 * rows * taps * terms * C * C_out, x2.device):
        for n0 in range(0, N, n_max):
            n = min(n_max, N - n0)
            r0 = n0 * H * W
            _check(fn(x2[r0:].data_ptr(), w3.data_ptr(), out[r0:].data_ptr(), n, H, W, C, C_out, terms, _DT[dt], cap - r0, _stream(x2.device)),
                   "conv_split3")
    return out[:rows]


def conv_split3_s2_plan(N, H, W, row_bytes, max_bytes=0xFFFFFFFF):
    """(Ho, Wo, images per launch) of conv_split3_s2 — pure arithmetic, no device. Ho, Wo: the output of a 3x3 / stride 2 convolution over
    F.pad(x, (0, 1, 0, 1)); the batch is cut by INPUT image bytes (H W row_bytes each: the kernel's 32-bit offsets span the input tensor)."""
    if H < 2 or W < 2:
        raise ValueError("conv_split3_s2: H, W >= 2 expected")
    per = H * W * row_bytes
    if per > 0xFFFFFFFF:
        raise ValueError("conv_split3_s2: one image exceeds the kernel's 32-bit activation offsets")
    return (H - 2) // 2 + 1, (W - 2) // 2 + 1, max(1, min(N, max_bytes // per))


def conv_split3_s2(x2, w3, N, H, W, C_out, mode="split3", _max_bytes=0xFFFFFFFF):
    """Downsample.conv of the first-stage encoder (3x3, stride 2, padding 0 over F.pad(x, (0, 1, 0, 1))) on the operands of conv_split3:
    x2 [N H W, 2 C] (or [N H W, C] in modes "bf16" / "f16"), w3 from split3_weight -> fp32 [N Ho Wo, C_out], no bias
    (mvi_conv3x3_s2_split3_f32). The batch is cut by input bytes; the output advances by Ho Wo rows per image."""
    L = _lib.lib()
    terms, dt, _ = _OPERANDS[mode]
    Cx = x2.shape[-1]
    C = Cx // 2 if terms == 3 else Cx
    if x2.dtype != dt or not x2.is_contiguous() or x2.numel() != N * H * W * Cx or w3.shape[1] != 9 * terms * C or w3.dtype != dt:
        raise ValueError(f"conv_split3_s2 ({mode}): x2 contiguous {dt} [N H W, {'2 C' if terms == 3 else 'C'}] and w3 [C_out padded, 9 {terms} C] expected")
    Ho, Wo, n_max = conv_split3_s2_plan(N, H, W, Cx * 2, _max_bytes)
    x2 = x2.reshape(N * H * W, Cx)
    rows = N * Ho * Wo
    cap = int(L.mvi_conv_split3_out_rows(rows)) + 256
    out = torch.empty(cap, C_out, dtype=torch.float32, device=x2.device)
    with torch.cuda.device(x2.device), _Timed("conv_split3_s2", 2.0 * rows * 9 * terms * C * C_out, x2.device):
        for n0 in range(0, N, n_max):
            n = min(n_max, N - n0)
            r0 = n0 * Ho * Wo
            _check(L.mvi_conv3x3_s2_split3_f32(x2[n0 * H * W:].data_ptr(), w3.data_ptr(), out[r0:].data_ptr(), n, H, W, C, C_out, terms, _DT[dt],
                                               cap - r0, _stream(x2.device)), "conv_split3_s2")
    return out[:rows]


def conv_in_f32_tokens_supported(conv, x):
    """A 3x3 / stride 1 / padding 1 fp32 Conv2d of at most 4 input channels on a contiguous fp32 GPU tensor (csrc/stem_conv_f32.hip)."""
    return (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and conv.weight.dtype == torch.float32
            and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros" and x.shape[1] == conv.in_channels
            and bool(_lib.lib().mvi_conv3x3_small_cin_f32_tokens_supported(int(conv.in_channels), int(conv.out_channels))))


def conv_in_f32_tokens(x, conv):
    """conv(x) for fp32 planes x [N, C_in <= 4, H, W] as token-major fp32 [N, H W, C_out], bias included: exact fp32 FMA chains, the
    output written once in the layout the split-operand walk reads (mvi_conv3x3_small_cin_f32_tokens)."""
    L = _lib.lib()
    if not conv_in_f32_tokens_supported(conv, x):
        raise ValueError(f"conv_in_f32_tokens: unsupported convolution / input {tuple(x.shape)} {x.dtype}")
    xc = _contig(x)
    N, Cin, H, W = xc.shape
    Co = conv.out_channels
    wc = _contig(conv.weight.detach())
    b = None if conv.bias is None else _contig(conv.bias.detach())
    out = torch.empty(N, H * W, Co, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _Timed("conv_in_f32_tokens", float(xc.numel() + out.numel()) * 4, x.device):
        _check(L.mvi_conv3x3_small_cin_f32_tokens(xc.data_ptr(), wc.data_ptr(), _ptr(b), out.data_ptr(), N, Cin, H, W, Co, _stream(x.device)),
               "conv_in_f32_tokens")
    return out


def rows_axpb(a, b, bias, alpha=1.0, out=None):
    """a + alpha * (b + bias[c]) for fp32 token-major a, b [..., C] in one pass (mvi_rows_axpb_f32); out may be a or b (default: b)."""
    L = _lib.lib()
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise TypeError("rows_axpb: contiguous fp32 tensors of one shape expected")
    out = b if out is None else out
    Cc = a.shape[-1]
    R = a.numel() // Cc
    bf = None if bias is None else _f32(bias)
    with torch.cuda.device(a.device), _Timed("rows_axpb", 3.0 * a.numel() * 4, a.device):
        _check(L.mvi_rows_axpb_f32(a.data_ptr(), b.data_ptr(), _ptr(bf), float(alpha), out.data_ptr(), R, Cc, _stream(a.device)), "rows_axpb")
    return out


# ---- Round 6: block tails on token-major tensors with the next GroupNorm's statistics (csrc/groupnorm_tokens.hip gt_fused_kernel) -------

def rows_gnstats_supported(N, C, S, groups, dtype):
    return dtype in _DT and int(_lib.lib().mvi_rows_gnstats_bytes(int(N), int(C), int(S), int(groups), _DT[dtype])) > 0


def rows_fused(a, b=None, bias=None, base=None, alpha=None, groups=0, concat=False):
    """Token-major [N, S, C] tensors of one dtype. base None: a + b + bias[c] (b, bias optional) — the ResBlock's skip add, the
    transformer's `x + x_in`. base and alpha given: base + (1 - alpha[n]) * (a + bias[c]) — the temporal skip add + AlphaBlender (alpha [N]
    fp32). concat: channels (a | b + base) -> [N, S, Ca + Cb], base optional — the decoder's cat([h, skip + control], dim=1).
    groups > 0: also returns GnPartials of GroupNorm(groups) of the result (no chan_bias) for group_norm_silu_tok2tok(partials=...), None
    where the statistics kernel's geometry does not take the shape."""
    L = _lib.lib()
    if a.dim() != 3 or a.dtype not in _DT:
        raise TypeError("rows_fused: token-major [N, S, C] fp32 / bf16 / f16 expected")
    N, S, Ca = a.shape
    ts = [t for t in (a, b, base) if t is not None]
    if any(t.dtype != a.dtype or not t.is_contiguous() or t.shape[:2] != a.shape[:2] for t in ts):
        raise ValueError("rows_fused: a, b, base must be contiguous [N, S, .] tensors of one dtype")
    if concat:
        if b is None or bias is not None or alpha is not None or (base is not None and base.shape != b.shape):
            raise ValueError("rows_fused: concat takes a, b (and base shaped like b), no bias / alpha")
        mode, Cc = 2, Ca + b.shape[2]
    else:
        if any(t.shape != a.shape for t in ts):
            raise ValueError("rows_fused: a, b, base must share one shape")
        mode, Cc = (0 if base is None else 1), Ca
        if mode == 1 and (alpha is None or alpha.numel() != N):
            raise ValueError(f"rows_fused: alpha must be [{N}]")
    out = torch.empty(N, S, Cc, dtype=a.dtype, device=a.device)
    part, nb = None, 0
    if groups:
        nb = int(L.mvi_rows_gnstats_bytes(N, Cc, S, int(groups), _DT[a.dtype]))
        if nb == 0:
            groups = 0
        else:
            part = torch.empty(nb // 4, dtype=torch.float32, device=a.device)
    ch = C.c_int32(0)
    al = None if alpha is None else alpha.detach().float().contiguous()
    bf = None if bias is None else _f32(bias)
    kind = ("rows_add", "rows_blend", "rows_concat")[mode]
    nbytes = float(sum(t.numel() for t in ts) + out.numel()) * a.element_size()
    with torch.cuda.device(a.device), _Timed(kind, nbytes, a.device):
        _check(L.mvi_rows_fused_gnstats(mode, a.data_ptr(), _ptr(b), _ptr(base), _ptr(bf), _ptr(al), out.data_ptr(), N, Cc, Ca, S, int(groups),
                                        _DT[a.dtype], _ptr(part), nb, C.byref(ch), _stream(a.device)), "rows_fused")
    if not groups:
        return out, None
    chunks = int(ch.value)
    return out, GnPartials(part[:N * chunks * int(groups) * 3], chunks, int(groups), None)

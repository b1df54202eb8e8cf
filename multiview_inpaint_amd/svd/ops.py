"""Device ops of the denoise loop. On a GPU tensor these run the hand-written HIP kernels through
the C-ABI library (include/mvi_unet_ops.h) and raise if it is missing — there is no silent
PyTorch substitute on the GPU inference path. On a CPU tensor they are plain PyTorch: that is
BASELINE.json configs[0] ("sgm VideoUNet single denoise step ... fp32 on CPU PyTorch"), the
reference's own CPU-runnable case, not a fallback for the GPU.

Under autograd (ControlNet training — SURVEY.md §2 row 21) attention stays on the HIP path, forward and backward
(csrc/attn_bwd.hip: `attention` for bf16 / f16 with D = 64 and more than 32 keys, `attention_temporal` up to 32 frames in every
type and head dim its forward takes), and so do GroupNorm(+SiLU) (csrc/groupnorm_bwd.hip: `group_norm`, `group_norm_frames`, `group_norm_tokens`, and the
token-major `group_norm_tok2tok` where `group_norm_tok2tok_backward_pays` says so) and GEGLU
(csrc/ff_geglu_bwd.hip: `linear_geglu` at K = 320 in bf16 / f16, the projection recomputed, never stored; csrc/geglu.hip: `geglu`;
from the sizes at which they were measured faster, `linear_geglu_backward_pays` / `geglu_backward_pays`), and the residual add(s) +
LayerNorm of the transformer blocks (csrc/layernorm_bwd.hip: `add_layer_norm` for every width its forward takes, where
`add_layer_norm_backward_pays` says so).
The 3x3 convolution of token-major activations has a HIP backward too (`conv3x3_tokens`: the input gradient on the forward's
implicit-GEMM kernel with the transposed weight, the weight gradient on csrc/conv3x3_wgrad.hip), where `conv3x3_backward_pays` says
so; the ResBlock reaches it through the opt-in layers.RESBLOCK_CONV_BWD. So has the (3,1,1) frame convolution of the temporal
ResBlocks (`conv3t_tokens`: the same kernel's three-tap form for forward and input gradient, csrc/conv3t_wgrad.hip for the weight
gradient), where `conv3t_backward_pays` says so; VideoResBlock reaches it through the opt-in layers.TIME_STACK_CONV_BWD. And so have the
resampling forms (`conv3x3_down_tokens`: the zero-stuffed input gradient on the forward kernel, the stride-2 form of the weight-gradient
kernel; `conv3x3_up_tokens` with a frozen convolution: the stride-1 input gradient at the upsampled size + csrc/token_rows.hip's 2x2 sum),
where `conv3x3_down_backward_pays` / `conv3x3_up_backward_pays` say so; Downsample / Upsample reach them through the opt-in
layers.RESAMPLE_CONV_BWD. These four are forms of one op and share their plumbing: hip_ops.conv_n320_launch_ok is the one "does the kernel
take this launch?" gate (each `*_tokens_gates` is calls of it plus the weight-gradient kernel's own test), `_ConvTokensFn` the one
autograd.Function, `_conv_tokens_route` the one triage, `conv_packed_weight` / `conv_packed_weight_transposed` the one pair of cached weights.
The 16- / 32-channel conv + SiLU layers of the ControlNet hint stem have one as well (`stem_conv3x3_silu`: dz on csrc/stem_conv.hip's second
epilogue, weight / bias gradient on csrc/stem_conv_bwd.hip), where `stem_conv_backward_pays` says so; ControlNet._hint_stem reaches it
through the opt-in unet.HINT_STEM_BWD.
The projections have one behind a switch that is off by default (`linear` with MVI_LINEAR_BWD=1: the forward on the kernel inference
launches, the input gradient on the forward kernels with the transposed weight, weight and bias gradient on csrc/linear_wgrad.hip),
where `linear_gates` and `linear_backward_pays` say so; `linear_module` and `linear_add_layer_norm` under grad reach it through `linear`.
The block tails have one behind another switch that is off by default (`tokens_to_planes_add`, `tokens_blend_to_planes`, `add_lerp`,
`planes_to_tokens` with MVI_BLOCK_TAILS_BWD=1: the forward on the inference kernel, the backward on csrc/block_tails_bwd.hip,
deterministic dbias / dalpha), where `block_tails_backward_pays` says so.
Every other kernel is forward-only: a GPU tensor that requires grad goes through PyTorch-ROCm's differentiable ops there
(the projections without that switch or outside its classes, the cross-attention projections of the context —
`linear_add_layer_norm` under grad is `linear_module` + `add_layer_norm` —, the tails without their switch).

Reference ops: GroupNorm32 + SiLU (sgm/modules/diffusionmodules/util.py:259-276,
openaimodel.py:257-261,292-305), Normalize (sgm/modules/attention.py:125-128),
softmax(QK^T d^-1/2)V (sgm/modules/attention.py:332-336, :427-439).
"""
import collections
import os

import torch
import torch.nn.functional as F

# A GPU tensor leaves the HIP path for one of two reasons, treated differently:
#   * it requires grad and the op has no HIP backward (everything but attention, GroupNorm, GEGLU and add_layer_norm): PyTorch-ROCm's
#     differentiable ops run — the documented path;
#   * a shape / contiguity gate of a kernel fails under no_grad: that RAISES by default (STRICT_GATES; since round 3) — an
#     inference call never silently runs PyTorch ops in place of the kernels. MVI_STRICT=0 allows the substitute again
#     (recorded in FALLBACKS).
# Strict mode proper (MVI_STRICT=1, or ops.STRICT = True) raises in BOTH cases. The GPU tests and bench_svd.run_gpu run with
# it, so "the full-size step took the HIP branch everywhere" is asserted, not assumed.
STRICT = os.environ.get("MVI_STRICT", "") == "1"
STRICT_GATES = os.environ.get("MVI_STRICT", "") != "0"
FALLBACKS = []          # (op, reason) of every GPU-tensor fallback taken when not strict (diagnostics)


class HipPathError(RuntimeError):
    pass


def _fallback(t, op, reason):
    """Called right before a PyTorch substitute runs. CPU tensors: that IS the CPU path. GPU tensors: raise in strict
    mode, otherwise record."""
    if t is not None and t.is_cuda:
        if STRICT or (STRICT_GATES and reason != "requires grad"):
            raise HipPathError(f"{op}: GPU tensor left the HIP path ({reason}); set MVI_STRICT=0 to allow the PyTorch substitute")
        if len(FALLBACKS) < 4096:
            FALLBACKS.append((op, reason))


def _needs_autograd(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _why(*ts):
    return "requires grad" if _needs_autograd(*ts) else "shape / layout gate"


def _stack3(y, T):
    """[(b T), C, ...] -> [(b T), 3C, ...]: frame t-1 | frame t | frame t+1 on the channel axis (zeros at the ends)."""
    bt, c = y.shape[:2]
    yv = y.reshape(bt // T, T, c, *y.shape[2:])
    out = y.new_zeros(bt // T, T, 3 * c, *y.shape[2:])
    out[:, 1:, :c] = yv[:, :-1]
    out[:, :, c:2 * c] = yv
    out[:, :-1, 2 * c:] = yv[:, 1:]
    return out.reshape(bt, 3 * c, *y.shape[2:])


# The HIP backward of GroupNorm(+SiLU) (csrc/groupnorm_bwd.hip). MVI_GN_BWD=0 (or ops.GROUPNORM_BACKWARD = False): the three norms
# below take PyTorch-ROCm's differentiable ops under autograd again.
GROUPNORM_BACKWARD = os.environ.get("MVI_GN_BWD", "1") != "0"
GROUPNORM_BACKWARD_MIN_ELEMENTS = (1 << 24, 0, 1 << 23)      # per dy layout: planes, stack3, token-major


def group_norm_backward_pays(N, C, S, T, dtype, layout=0):
    """Whether forward + backward on the HIP kernels is faster than the PyTorch-ROCm route for this shape class — the routing's second
    question after hip_ops.group_norm_backward_supported. Set from tools/bench_groupnorm_bwd.py (profiles/groupnorm_bwd_bench.json;
    DESIGN.md 'GroupNorm under autograd'): a class goes to HIP where the HIP route's median beat the PyTorch route's by more than that
    route's spread. The HIP route costs 0.22 - 0.27 ms of host time per forward + backward whatever the size (its kernels: 0.06 - 0.29 ms),
    the PyTorch route 0.21 ms at its smallest. stack3 (the temporal ResBlock: 0.26 - 0.41 against 0.43 - 2.7 ms) wins at every shape;
    planes win from 20.6 M elements up (14 x 1920 x 24x32: 0.24 against 0.39 ms) and tie or lose at 13.8 M and below (14 x 320 x 48x64:
    0.247 against 0.244); token-major wins at 13.8 M (0.23 against 0.32) and loses at 3.4 M and below. The lines sit between."""
    return N * C * S >= GROUPNORM_BACKWARD_MIN_ELEMENTS[layout]


_GN_TOK2TOK = 3      # beside hip_ops.GN_PLANES / GN_STACK3 / GN_TOKENS (y's layout, x in planes): token-major in AND out, T carries `frames`


class _GroupNormFn(torch.autograd.Function):
    """GroupNorm(+SiLU) on the HIP kernels with a deterministic HIP backward, behind group_norm, group_norm_tokens, group_norm_frames
    and (layout _GN_TOK2TOK) group_norm_tok2tok. Holds x, weight, bias, chan_bias and the (mean, rstd) table — not y, nothing
    tensor-sized in fp32; nothing is cached outside ctx, so torch.utils.checkpoint may re-run the forward."""

    @staticmethod
    def forward(ctx, x, weight, bias, chan_bias, num_groups, eps, silu, T, layout):
        from . import hip_ops
        xc = x if x.is_contiguous() else x.contiguous()
        if layout == _GN_TOK2TOK:
            y, stats = hip_ops.group_norm_tok2tok_forward_stats(xc, num_groups, weight, bias, eps, silu, chan_bias=chan_bias, frames=T)
        else:
            y, stats = hip_ops.group_norm_forward_stats(xc, T, num_groups, weight, bias, eps, silu, chan_bias=chan_bias, layout=layout)
        ctx.save_for_backward(xc, weight, bias, chan_bias, stats)
        ctx.cfg = (num_groups, bool(silu), T, layout)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        x, weight, bias, chan_bias, stats = ctx.saved_tensors
        num_groups, silu, T, layout = ctx.cfg
        n = ctx.needs_input_grad
        need = dict(chan_bias=chan_bias, need_dx=n[0], need_dparams=n[1] or n[2], need_dchan_bias=n[3])
        if layout == _GN_TOK2TOK:
            dx, dw, db, dcb = hip_ops.group_norm_tok2tok_backward(dy.contiguous(), x, stats, num_groups, weight, bias, silu, frames=T, **need)
        else:
            dx, dw, db, dcb = hip_ops.group_norm_backward(dy.contiguous(), x, stats, T, num_groups, weight, bias, silu, layout=layout, **need)
        return (dx, dw.to(weight.dtype) if n[1] else None, db.to(bias.dtype) if n[2] else None,
                dcb.to(chan_bias.dtype).reshape(chan_bias.shape) if n[3] else None, None, None, None, None, None)


def _gn_hip_autograd(x, T, num_groups, weight, bias, chan_bias, layout):
    """Under autograd: does this norm run _GroupNormFn? (switch on, kernels compute the shape, and it pays; the token-major family also
    wants a contiguous tensor 16-byte aligned — one that is not contiguous is copied by the Function, and the copy is aligned)"""
    tok = layout == _GN_TOK2TOK
    switch = GROUPNORM_TOK2TOK_BACKWARD if tok else GROUPNORM_BACKWARD
    if not (x.is_cuda and switch and (x.dim() == 3 if tok else x.dim() >= 2) and x.numel() > 0):
        return False
    from . import hip_ops
    N, C = x.shape[0], x.shape[2 if tok else 1]
    S = x.numel() // (N * C)
    if chan_bias is not None and tuple(chan_bias.shape) != (N, C):
        return False
    if tok:
        if T < 1 or (x.is_contiguous() and x.data_ptr() % 16 != 0):
            return False
        return (hip_ops.group_norm_tok2tok_backward_supported(N, C, S, num_groups, T, x.dtype)
                and group_norm_tok2tok_backward_pays(N, C, S, T, x.dtype))
    return (hip_ops.group_norm_backward_supported(N, C, S, num_groups, T, x.dtype, layout)
            and group_norm_backward_pays(N, C, S, T, x.dtype, layout))


def group_norm(x, num_groups, weight, bias, eps, silu=False, chan_bias=None):
    """GroupNorm over (C/G, *spatial) with fp32 statistics, optional fused SiLU; output dtype = x.dtype.
    chan_bias [N, C] (optional) is added to x first (the ResBlock's timestep-embedding bias)."""
    if x.is_cuda and not _needs_autograd(x, weight, bias, chan_bias):
        from . import hip_ops
        return hip_ops.group_norm_silu(x, num_groups, weight, bias, eps, silu, chan_bias=chan_bias)
    if _gn_hip_autograd(x, 1, num_groups, weight, bias, chan_bias, 0):
        return _GroupNormFn.apply(x, weight, bias, chan_bias, num_groups, eps, silu, 1, 0)
    _fallback(x, "group_norm", _why(x, weight, bias, chan_bias))
    xf = x.float()
    if chan_bias is not None:
        xf = xf + chan_bias.float().reshape(*chan_bias.shape, *([1] * (x.ndim - 2)))
    y = F.group_norm(xf, num_groups, weight.float(), bias.float(), eps).type(x.dtype)
    return F.silu(y) if silu else y


def group_norm_tokens(x, num_groups, weight, bias, eps, silu=False, chan_bias=None):
    """group_norm(...) returned token-major: [N, C, *spatial] -> [N, prod(spatial), C] ("b c h w -> b (h w) c"
    fused into the normalisation's write)."""
    S = x[0, 0].numel()
    if x.is_cuda and not _needs_autograd(x, weight, bias, chan_bias):
        from . import hip_ops
        if x.shape[1] % 8 == 0 and S % 8 == 0:
            return hip_ops.group_norm_silu_tokens(x, num_groups, weight, bias, eps, silu, chan_bias=chan_bias)
        # odd channel / token counts: the plain HIP GroupNorm, then PyTorch's transpose copy (small tensors only)
        return hip_ops.group_norm_silu(x, num_groups, weight, bias, eps, silu, chan_bias=chan_bias).flatten(2).transpose(1, 2).contiguous()
    if x.shape[1] % 8 == 0 and S % 8 == 0 and x.data_ptr() % 16 == 0 and _gn_hip_autograd(x, 1, num_groups, weight, bias, chan_bias, 2):
        return _GroupNormFn.apply(x, weight, bias, chan_bias, num_groups, eps, silu, 1, 2)
    if _gn_hip_autograd(x, 1, num_groups, weight, bias, chan_bias, 0):
        # odd channel / token counts: the planes form, then PyTorch's transpose copy (autograd provides its backward)
        return _GroupNormFn.apply(x, weight, bias, chan_bias, num_groups, eps, silu, 1, 0).flatten(2).transpose(1, 2).contiguous()
    _fallback(x, "group_norm_tokens", _why(x, weight, bias, chan_bias))
    return group_norm(x, num_groups, weight, bias, eps, silu=silu, chan_bias=chan_bias).flatten(2).transpose(1, 2).contiguous()


# The HIP backward of the token-major GroupNorm(+SiLU) (csrc/groupnorm_bwd.hip, gn_bwd_tok_*). MVI_GN_TOK2TOK_BWD=0 (or
# ops.GROUPNORM_TOK2TOK_BACKWARD = False): group_norm_tok2tok takes PyTorch-ROCm's differentiable ops under autograd again.
GROUPNORM_TOK2TOK_BACKWARD = os.environ.get("MVI_GN_TOK2TOK_BWD", "1") != "0"
GROUPNORM_TOK2TOK_BACKWARD_MIN_ELEMENTS = None      # None: no class has been measured faster yet, nothing is routed by default


def group_norm_tok2tok_backward_pays(N, C, S, frames, dtype):
    """Whether forward + backward of the token-major norm on the HIP kernels is faster than the routes it replaces — the routing's second
    question after hip_ops.group_norm_tok2tok_backward_supported. The rule (tools/bench_groupnorm_tok2tok_bwd.py ->
    profiles/groupnorm_tok2tok_bwd_bench.json; DESIGN.md 'GroupNorm under autograd'): a class goes to HIP only where the HIP route's
    median beats the faster of the PyTorch fallback and the ResBlock's transposing-copy + ops.group_norm_tokens middle by more than
    that route's spread. The bench has NOT been run on a GPU yet (profiles/HISTORY.md says what is owed), so no class has won and the
    line is None: every shape stays on the route it had. The tests lift the decision (a line of 0 elements)."""
    line = GROUPNORM_TOK2TOK_BACKWARD_MIN_ELEMENTS
    return line is not None and N * C * S >= line


def group_norm_tok2tok_hip_autograd(t, num_groups, chan_bias=None, frames=1):
    """Under autograd: does group_norm_tok2tok run _GroupNormFn for this tensor? (switch on, kernels compute the shape, 16-byte
    aligned, and it pays) — layers asks before it keeps the ResBlock's middle token-major."""
    return _gn_hip_autograd(t, frames, num_groups, None, None, chan_bias, _GN_TOK2TOK)


def group_norm_tok2tok(t, num_groups, weight, bias, eps, silu=False, chan_bias=None, frames=1, partials=None):
    """GroupNorm(+SiLU) of token-major t [N, S, C] with token-major output (statistics per sample and group over (S, C/G));
    chan_bias [N, C] is added first. The norm between two convolutions that run on channels-last tensors. frames > 1: the temporal
    layers' norm — statistics over the `frames` consecutive samples of a video (video_model.py:71-75), chan_bias still per sample.
    Under autograd `partials` is ignored: the norm runs its own statistics pass."""
    if t.is_cuda and not _needs_autograd(t, weight, bias, chan_bias):
        from . import hip_ops
        return hip_ops.group_norm_silu_tok2tok(t, num_groups, weight, bias, eps, silu, chan_bias=chan_bias, frames=frames, partials=partials)
    if group_norm_tok2tok_hip_autograd(t, num_groups, chan_bias, frames):
        return _GroupNormFn.apply(t, weight, bias, chan_bias, num_groups, eps, silu, int(frames), _GN_TOK2TOK)
    _fallback(t, "group_norm_tok2tok", _why(t, weight, bias, chan_bias))
    N, S, C = t.shape
    if t.dtype == torch.float64:
        # fp64 (validation on the CPU) stays fp64: group_norm below computes in fp32
        u = t if chan_bias is None else t + chan_bias.to(t.dtype).reshape(N, 1, C)
        y = F.group_norm(u.reshape(N // frames, frames * S, C).transpose(1, 2), num_groups, weight.to(t.dtype), bias.to(t.dtype), eps)
        return (F.silu(y) if silu else y).transpose(1, 2).reshape(N, S, C).contiguous()
    tf = t.float() if chan_bias is None else t.float() + chan_bias.float().reshape(N, 1, C)
    y = group_norm(tf.reshape(N // frames, frames * S, C).transpose(1, 2), num_groups, weight, bias, eps, silu=silu)
    return y.transpose(1, 2).reshape(N, S, C).to(t.dtype).contiguous()


def group_norm_frames(x, T, num_groups, weight, bias, eps, silu=False, chan_bias=None, stack3=False):
    """GroupNorm of the temporal layers — statistics over (C/G, T, H, W) per video — evaluated on the
    frame-major tensor x [(b T), C, H, W] the spatial layers produce (the reference permutes to
    b c t h w first: video_model.py:71-75). chan_bias [(b T), C] is added first; stack3 returns the
    result as [(b T), 3C, H, W] = (previous | own | next frame), the input of a (3,1,1) temporal
    convolution evaluated as one 1x1 convolution."""
    if x.is_cuda and not _needs_autograd(x, weight, bias, chan_bias):
        from . import hip_ops
        return hip_ops.group_norm_silu_frames(x, T, num_groups, weight, bias, eps, silu, chan_bias=chan_bias, stack3=stack3)
    if x.shape[0] % T == 0 and _gn_hip_autograd(x, int(T), num_groups, weight, bias, chan_bias, 1 if stack3 else 0):
        return _GroupNormFn.apply(x, weight, bias, chan_bias, num_groups, eps, silu, int(T), 1 if stack3 else 0)
    _fallback(x, "group_norm_frames", _why(x, weight, bias, chan_bias))
    bt, c = x.shape[:2]
    xf = x.float()
    if chan_bias is not None:
        xf = xf + chan_bias.float().reshape(bt, c, *([1] * (x.ndim - 2)))
    x5 = xf.reshape(bt // T, T, c, *x.shape[2:]).transpose(1, 2)              # b c t h w
    y = F.group_norm(x5, num_groups, weight.float(), bias.float(), eps).type(x.dtype)
    if silu:
        y = F.silu(y)
    y = y.transpose(1, 2).reshape(x.shape)
    return _stack3(y, T) if stack3 else y


# The HIP backward of attention (csrc/attn_bwd.hip). MVI_ATTN_BWD=0 (or ops.ATTENTION_BACKWARD = False): attention under autograd
# takes PyTorch-ROCm's scaled_dot_product_attention again, as every other op does.
ATTENTION_BACKWARD = os.environ.get("MVI_ATTN_BWD", "1") != "0"


def attention_backward_pays(B, Sq, Sk, heads, dtype):
    """Whether forward + backward on the HIP kernels is at least as fast as the PyTorch-ROCm route for this shape class — the
    routing's second question after hip_ops.attention_backward_supported (what the kernels compute correctly). Set from
    tools/bench_attention_bwd.py (profiles/attention_bwd_bench.json; DESIGN.md 'Attention under autograd'): at B = 14 the route wins
    at (H, S) = (5, 9216), (5, 3072), (10, 768) — 7.6 / 1.04 / 0.29 ms against 13.0 / 1.72 / 0.36 in bf16 — and loses in bf16 at
    (20, 192) and (20, 48) — 0.230 / 0.228 ms against 0.189 / 0.184 — where the kernels take 0.08 / 0.05 ms and both routes are
    bound by their host side. The line is drawn in score elements between the two groups (82.6 M and 10.3 M)."""
    return B * heads * Sq * Sk >= ATTENTION_BACKWARD_MIN_SCORES


ATTENTION_BACKWARD_MIN_SCORES = 1 << 25


class _AttentionFn(torch.autograd.Function):
    """softmax(q k^T D^-1/2) v on the MFMA kernels with a deterministic HIP backward. Holds q, k, v, out and the row log-sum-exp;
    nothing is cached outside ctx, so torch.utils.checkpoint may re-run the forward."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        from . import hip_ops
        out, lse = hip_ops.attention_forward_lse(q, k, v, heads)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.heads = heads
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        from . import hip_ops
        q, k, v, out, lse = ctx.saved_tensors
        need_dq = ctx.needs_input_grad[0]
        need_dkv = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dq, dk, dv = hip_ops.attention_backward(q, k, v, out, dout.contiguous(), lse, ctx.heads, need_dq=need_dq, need_dkv=need_dkv)
        return (dq if need_dq else None, dk if ctx.needs_input_grad[1] else None, dv if ctx.needs_input_grad[2] else None, None)


class _AttentionTemporalFn(torch.autograd.Function):
    """attention_temporal with its HIP backward (the softmax over T <= 32 frames is recomputed: only q, k, v are held). The forward is
    the inference entry: the MFMA kernels up to 16 and up to 32 frames where they apply (bf16 / f16, D = 64), else the fp32-math kernel."""

    @staticmethod
    def forward(ctx, q, k, v, heads, T):
        from . import hip_ops
        ctx.save_for_backward(q, k, v)
        ctx.heads, ctx.T = heads, T
        return hip_ops.attention_temporal(q, k, v, heads, T)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        from . import hip_ops
        q, k, v = ctx.saved_tensors
        dq, dk, dv = hip_ops.attention_temporal_backward(q, k, v, dout.contiguous(), ctx.heads, ctx.T)
        n = ctx.needs_input_grad
        return (dq if n[0] else None, dk if n[1] else None, dv if n[2] else None, None, None)


def _temporal_backward_supported(q, k, v, heads, T):
    D = q.shape[-1] // max(heads, 1)
    return (q.dtype in (torch.float32, torch.bfloat16, torch.float16) and k.dtype == q.dtype and v.dtype == q.dtype
            and q.shape == k.shape == v.shape and D in (16, 32, 64) and D * heads == q.shape[-1] and 0 < T <= 32 and q.shape[0] % T == 0)


def attention(q, k, v, heads):
    """q [B,Sq,H*D], k/v [B,Sk,H*D] token-major as the Linear layers produce them -> [B,Sq,H*D]."""
    B, Sq, HD = q.shape
    Sk = k.shape[1]
    if q.is_cuda and not _needs_autograd(q, k, v):
        from . import hip_ops
        return hip_ops.attention(q, k, v, heads)
    if q.is_cuda and ATTENTION_BACKWARD and k.dtype == q.dtype and v.dtype == q.dtype and HD % heads == 0:
        from . import hip_ops
        if hip_ops.attention_backward_supported(Sq, Sk, HD // heads, q.dtype) and attention_backward_pays(B, Sq, Sk, heads, q.dtype):
            return _AttentionFn.apply(q, k, v, heads)
    _fallback(q, "attention", _why(q, k, v))
    D = HD // heads
    qh, kh, vh = (t.reshape(B, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qh, kh, vh)
    return o.transpose(1, 2).reshape(B, Sq, HD)


def packed_ok(x, heads, dim_head):
    """Whether the self-attention of x can take the packed-projection path (GPU inference, kernel-supported head dim)."""
    return x.is_cuda and not torch.is_grad_enabled() and dim_head in (16, 32, 64) and (heads * dim_head * x.element_size()) % 16 == 0


def attention_scale_fold_pays(x, dim_head):
    """Whether the self-attention of x [B, S, C] runs the 8-wave MFMA kernel (csrc/attn_flash8m16.hip), whose softmax is bound by
    vector issue: the only kernel for which a q that carries the softmax scale (CrossAttention._packed_qkv_weight(fold=True))
    is faster."""
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 3):
        return False
    from . import hip_ops
    return hip_ops.attention_kernel_variant(x.shape[1], x.shape[1], dim_head, x.dtype) in (8, 16)


def _unfold_q(q, heads, q_log2):
    """q of a packed projection whose q rows carry dim_head^-1/2 * log2(e) (CrossAttention._packed_qkv_weight), for a consumer that
    applies the softmax scale itself."""
    if not q_log2:
        return q
    D = q.shape[-1] // heads
    return (q.float() * (D ** 0.5 * 0.6931471805599453)).to(q.dtype)


def attention_packed(qkv, heads, q_log2=False):
    """Self-attention on one packed projection qkv [B, S, 3*H*D] = (q | k | v) -> [B, S, H*D]. q_log2: the q third already
    carries dim_head^-1/2 * log2(e) (folded into its projection's weights)."""
    if qkv.is_cuda and not _needs_autograd(qkv):
        from . import hip_ops
        return hip_ops.attention_packed(qkv.contiguous(), heads, q_log2=q_log2)
    _fallback(qkv, "attention_packed", _why(qkv))
    q, k, v = qkv.chunk(3, dim=-1)
    return attention(_unfold_q(q, heads, q_log2).contiguous(), k.contiguous(), v.contiguous(), heads)


def attention_temporal_packed(qkv, heads, T, q_log2=False):
    """attention_temporal on a packed projection [(bo*T), S, 3*H*D]."""
    if qkv.is_cuda and not _needs_autograd(qkv):
        from . import hip_ops
        return hip_ops.attention_temporal_packed(qkv.contiguous(), heads, T, q_log2=q_log2)
    _fallback(qkv, "attention_temporal_packed", _why(qkv))
    q, k, v = qkv.chunk(3, dim=-1)
    return attention_temporal(_unfold_q(q, heads, q_log2).contiguous(), k.contiguous(), v.contiguous(), heads, T)


def attention_wide(q, k, v):
    """Single-head attention whose head is the whole channel axis (model.py:180-195: D = C = 512): q [B,Sq,D],
    k/v [B,Sk,D] -> [B,Sq,D]."""
    if q.is_cuda and not _needs_autograd(q, k, v):
        from . import hip_ops
        if q.shape[-1] <= 64 and q.shape[-1] in (16, 32, 64):
            return hip_ops.attention(q, k, v, 1)
        return hip_ops.attention_wide(q.contiguous(), k.contiguous(), v.contiguous())
    _fallback(q, "attention_wide", _why(q, k, v))
    return F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]


def attention_temporal(q, k, v, heads, T):
    """Self-attention over the frame axis without regrouping tokens: q/k/v [(bo*T), S, H*D] ->
    same shape; one softmax per (video, spatial token, head) over its T frames. Equals
    `(b t) s c -> (b s) t c`, attention, and the inverse regrouping of the reference
    (sgm/modules/video_attention.py:115, :136-140)."""
    BT, S, HD = q.shape
    if q.is_cuda and not _needs_autograd(q, k, v):
        from . import hip_ops
        return hip_ops.attention_temporal(q, k, v, heads, T)
    if q.is_cuda and ATTENTION_BACKWARD and _temporal_backward_supported(q, k, v, heads, T):
        return _AttentionTemporalFn.apply(q, k, v, heads, T)
    _fallback(q, "attention_temporal", _why(q, k, v))
    bo = BT // T

    def regroup(t):
        return t.reshape(bo, T, S, HD).transpose(1, 2).reshape(bo * S, T, HD)
    o = attention(regroup(q), regroup(k), regroup(v), heads)
    return o.reshape(bo, S, T, HD).transpose(1, 2).reshape(BT, S, HD)


# The HIP backward of GEGLU (csrc/ff_geglu_bwd.hip, csrc/geglu.hip). MVI_FF_GEGLU_BWD=0 (or ops.FF_GEGLU_BACKWARD = False): GEGLU under
# autograd takes PyTorch-ROCm's differentiable ops again (F.linear, chunk, gelu, mul), as every op without a HIP backward does.
FF_GEGLU_BACKWARD = os.environ.get("MVI_FF_GEGLU_BWD", "1") != "0"
# The smallest measured size of each class at which the HIP route won in BOTH bench runs (profiles/geglu_bwd_bench.json, bf16 measured
# first, and profiles/geglu_bwd_bench_f16_first.json); a dtype without an entry was not measured and is not routed.
FF_GEGLU_BACKWARD_MIN_ROWS = {torch.float16: 14 * 3072, torch.bfloat16: 28 * 3072}
GEGLU_BACKWARD_MIN_ELEMENTS = {torch.float16: 10752 * 2560, torch.bfloat16: 10752 * 2560}      # rows * inner


def linear_geglu_backward_pays(rows, K, inner, dtype, need_dparams):
    """Whether ff_geglu forward + the fused backward is faster than the PyTorch-ROCm route (F.linear, chunk, gelu, mul and their
    backward) for this shape class — the routing's second question after hip_ops.ff_geglu_backward_supported. Measured by
    tools/bench_geglu_bwd.py (profiles/geglu_bwd_bench.json; DESIGN.md 'GEGLU under autograd'): forward + backward by device events,
    the two routes alternating in one process, 9 pairs, medians; a class goes to HIP only where its median beats the PyTorch route's
    by more than that route's spread. K = 320, inner = 1280, ms HIP / PyTorch (spread), dx only | all gradients:
      f16   14 x 3072 rows  0.498 / 0.800 (0.116) | 0.773 / 1.096 (0.019)    wins
      f16   28 x 3072       0.741 / 1.561 (0.027) | 1.295 / 2.087 (0.137)    wins
      f16   14 x 9216       0.925 / 2.227 (0.044) | 1.711 / 3.055 (0.412)    wins
      bf16  14 x 3072       0.490 / 0.790 (0.806) | 0.966 / 1.151 (0.491)    ahead by the median, inside the spread: a tie, PyTorch
      bf16  28 x 3072       0.729 / 1.552 (0.103) | 1.239 / 2.079 (0.011)    wins
      bf16  14 x 9216       0.913 / 2.218 (0.031) | 1.663 / 2.994 (0.115)    wins
    A second run on another machine with f16 measured first (profiles/geglu_bwd_bench_f16_first.json) won in every class, bf16 at
    14 x 3072 rows included (0.507 / 0.786 (0.044) | 0.795 / 1.096 (0.066)): the tie above was one slow PyTorch pair in what that process
    measured first, not a property of the kernel (same arithmetic, same bytes in both types). A class is routed where it won in BOTH
    runs, so bf16 at 14 x 3072 rows stays on PyTorch. The dx-only and the all-gradient class have the same verdict at every measured
    size, so need_dparams does not move the line. Nothing below 14 x 3072 rows, nothing between the measured sizes and no other
    inner was measured: the line is the smallest size of the dtype that won twice, and everything below it stays on PyTorch."""
    return rows >= FF_GEGLU_BACKWARD_MIN_ROWS.get(dtype, float("inf"))


def geglu_backward_pays(rows, inner, dtype):
    """The same question for the elementwise pair geglu / geglu_backward (one pass each) against chunk + gelu + mul and their
    backward (three passes each and a cat of the two gradient halves), same bench, same rule. (rows, inner) of levels 1 - 3, ms HIP /
    PyTorch (spread), f16 | bf16:
      32256 x 2560 (82.6 M gated elements)  0.277 / 0.844 (0.021) | 0.266 / 0.840 (0.015)    wins | wins
       8064 x 5120 (41.3 M)                 0.139 / 0.408 (0.004) | 0.177 / 0.424 (0.047)    wins | wins
      10752 x 2560 (27.5 M)                 0.094 / 0.256 (0.005) | 0.139 / 0.272 (0.014)    wins | wins
       2688 x 5120 (13.8 M)                 0.076 / 0.125 (0.004) | 0.133 / 0.137 (0.008)    wins | tie
       2016 x 5120 (10.3 M)                 0.072 / 0.101 (0.007) | 0.149 / 0.124 (0.024)    wins | loses
        672 x 5120 (3.4 M)                  0.072 / 0.065 (0.004) | 0.124 / 0.098 (0.136)    loses | loses
    Small shapes are bound by the Function's host side, and that differs by run, not by type: in the second run (f16 first, another
    machine) the HIP route took 0.15 ms at every small size in BOTH types and lost at 13.8 M (0.153 / 0.132 f16, 0.162 / 0.138 bf16),
    10.3 M and 3.4 M, while 27.5 M and above won again in both (0.154 / 0.259 f16, 0.181 / 0.267 bf16 at 27.5 M). A class is routed
    where it won in BOTH runs: from 27.5 M gated elements in either type. fp32 I/O was not measured and is not routed (its kernel
    is parity-tested and reachable through hip_ops.geglu_backward)."""
    return rows * inner >= GEGLU_BACKWARD_MIN_ELEMENTS.get(dtype, float("inf"))


class _GegluFn(torch.autograd.Function):
    """geglu on the HIP kernel with its one-pass HIP backward. Holds h only; nothing is cached outside ctx."""

    @staticmethod
    def forward(ctx, h):
        from . import hip_ops
        hc = h if h.is_contiguous() else h.contiguous()
        ctx.save_for_backward(hc)
        return hip_ops.geglu(hc)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        (h,) = ctx.saved_tensors
        return hip_ops.geglu_backward(h, dy)


class _LinearGegluFn(torch.autograd.Function):
    """linear_geglu on the fused kernel (csrc/ff_geglu.hip) with the fused HIP backward (csrc/ff_geglu_bwd.hip). Holds x, weight and
    bias only — the [rows, 2 inner] projection exists neither between forward and backward nor, for frozen weights, during the
    backward; nothing is cached outside ctx, so torch.utils.checkpoint may re-run the forward."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import hip_ops
        ctx.save_for_backward(x, weight, bias)
        return hip_ops.ff_geglu(x, weight, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        x, weight, bias = ctx.saved_tensors
        n = ctx.needs_input_grad
        need_db = bias is not None and n[2]
        dx, dw, db = hip_ops.ff_geglu_backward(x, weight, bias, dy.contiguous(), need_dx=n[0], need_dparams=n[1] or need_db,
                                               need_dweight=n[1], need_dbias=need_db)
        return (dx if n[0] else None, dw.to(weight.dtype) if n[1] else None, db.to(bias.dtype) if need_db else None)


def geglu(h):
    """h [..., 2*inner] -> h[..., :inner] * gelu(h[..., inner:]) (sgm/modules/attention.py:93-95)."""
    inner = h.shape[-1] // 2
    if h.is_cuda and not _needs_autograd(h) and inner % 8 == 0:
        from . import hip_ops
        return hip_ops.geglu(h)
    if h.is_cuda and FF_GEGLU_BACKWARD and _needs_autograd(h) and h.dtype in (torch.float32, torch.bfloat16, torch.float16) \
            and inner > 0 and h.shape[-1] == 2 * inner and inner % (4 if h.dtype == torch.float32 else 8) == 0 \
            and geglu_backward_pays(h.numel() // (2 * inner), inner, h.dtype):
        return _GegluFn.apply(h)
    _fallback(h, "geglu", _why(h))
    a, gate = h.chunk(2, dim=-1)
    return a * F.gelu(gate)


FF_GEGLU_MIN_ROWS = 32768       # below, the fused kernel's 256-row blocks do not fill the chip: library GEMM + geglu
K320_KERNELS = os.environ.get("MVI_K320", "1") != "0"      # MVI_K320=0: library GEMMs everywhere (same-box A/B runs)


FF_GEGLU_N320 = os.environ.get("MVI_FF_GEGLU_N320", "1") != "0"
FF_GEGLU_N320_K = (640, 1280)
FF_GEGLU_N320_MIN_ROWS = int(os.environ.get("MVI_FF_GEGLU_N320_MIN_ROWS", "16000"))     # (level 2: 16 128 rows; round 5, with the 16x16x32 kernel: 385 us against 329 + 84)


def linear_geglu(x, weight, bias=None):
    """GEGLU of the reference (sgm/modules/attention.py:87-95): `x, gate = F.linear(x, weight, bias).chunk(2, -1); x * F.gelu(gate)`.
    On the GPU, for the shapes csrc/ff_geglu.hip covers (K = 320 in bf16 / f16: the level-0 FeedForward layers) and enough rows,
    projection and gating run as ONE kernel and the [rows, 2 inner] intermediate never exists; everything else is the library
    GEMM followed by geglu()."""
    if K320_KERNELS and x.is_cuda and not _needs_autograd(x, weight, bias) and x.dtype == weight.dtype:
        from . import hip_ops
        rows = x.numel() // max(x.shape[-1], 1)
        if rows >= FF_GEGLU_MIN_ROWS and hip_ops.ff_geglu_supported(x.shape[-1], weight.shape[0] // 2, x.dtype):
            return hip_ops.ff_geglu(x, weight, bias)
        # K = 640 / 1280 (levels 1 and 2): csrc/linear_n320.hip's GEGLU form, where it was measured faster than the library
        # GEMM + geglu_kernel (FF_GEGLU_N320_MIN_ROWS; MVI_FF_GEGLU_N320=0: library everywhere)
        if FF_GEGLU_N320 and x.shape[-1] in FF_GEGLU_N320_K and rows >= FF_GEGLU_N320_MIN_ROWS \
                and hip_ops.ff_geglu_n320_supported(x.shape[-1], weight.shape[0] // 2, x.dtype):
            return hip_ops.ff_geglu_n320(x, weight, bias)
    if K320_KERNELS and FF_GEGLU_BACKWARD and x.is_cuda and _needs_autograd(x, weight, bias) and x.dtype == weight.dtype \
            and (bias is None or bias.is_cuda) and weight.dim() == 2 and weight.shape[1] == x.shape[-1]:
        from . import hip_ops
        rows = x.numel() // max(x.shape[-1], 1)
        inner = weight.shape[0] // 2
        if hip_ops.ff_geglu_backward_supported(x.shape[-1], inner, x.dtype) \
                and linear_geglu_backward_pays(rows, x.shape[-1], inner, x.dtype, weight.requires_grad or (bias is not None and bias.requires_grad)):
            return _LinearGegluFn.apply(x, weight, bias)
    return geglu(F.linear(x, weight, bias))


N320_KERNEL = os.environ.get("MVI_N320", "1") != "0"          # csrc/linear_n320.hip for [rows, K] x [K, 320] with rows >= FF_GEGLU_MIN_ROWS
# Round 5: the same kernel with 320 g outputs (g column groups per row block) for the projections of levels 1 and 2 INTO 640 / 1280
# channels — FeedForward.net[2] (K = 2560 / 5120) and the attention output projections (K = 640 / 1280) — where it was measured faster
# than the tuned library GEMM (180 / 165 / 55 / 46 us against 215 / 189 / 80 / 57: profiles/round5_n320_groups.txt); the packed q/k/v
# projections (1920 / 3840 outputs) tie and stay with the library, and so does everything whose grid would not fill the chip (level 3).
N320_GROUPS = os.environ.get("MVI_N320_GROUPS", "1") != "0"
N320_GROUP_WIDTHS = (640, 1280)
N320_GROUP_MIN_BLOCKS = 200


def _linear_route(rows, K, N, dtype):
    """The kernel linear() launches WITHOUT autograd for x [rows, K] and weight [N, K] of one 16-bit dtype on the GPU: 'n320', 'k320'
    or None (the library GEMM) — linear()'s own conditions in its own order."""
    if not K320_KERNELS:
        return None
    from . import hip_ops
    if N320_KERNEL and N320_GROUPS and N in N320_GROUP_WIDTHS and (rows + 255) // 256 * (N // 320) >= N320_GROUP_MIN_BLOCKS \
            and hip_ops.linear_n320_supported(K, N, dtype):
        return "n320"
    if rows >= FF_GEGLU_MIN_ROWS:
        n320 = N320_KERNEL and N == 320 and hip_ops.linear_n320_supported(K, N, dtype)
        if n320 and K == 320:
            return "n320"
        if hip_ops.linear_k320_supported(K, N, dtype):
            return "k320"
        if n320:
            return "n320"
    return None


# The projections under autograd: forward on the kernel linear() launches at inference, the input gradient on the forward kernels with
# the transposed weight (dx = dy W is a projection with weight W^T [K, N]), weight and bias gradient on csrc/linear_wgrad.hip —
# deterministic, where the library's split-K GEMMs are not run-to-run reproducible. DEFAULT OFF (MVI_LINEAR_BWD=1 or
# ops.LINEAR_BACKWARD = True turns it on): linear() is called by every transformer block, and off it is exactly the function it was.
LINEAR_BACKWARD = os.environ.get("MVI_LINEAR_BWD", "0") == "1"
# Classes tools/bench_linear_bwd.py showed to win (profiles/linear_bwd_bench.json): {(N, K, need_dweight): the smallest measured row
# count from which every measured size of the class won in both dtypes}. A class that is not listed is not routed.
LINEAR_BACKWARD_ROUTED = {(320, 320, True): 14 * 9216, (320, 320, False): 28 * 9216, (960, 320, True): 14 * 9216, (960, 320, False): 14 * 9216,
                          (320, 1280, True): 14 * 9216, (320, 1280, False): 28 * 9216, (640, 640, True): 14 * 2304, (640, 640, False): 28 * 2304,
                          (1280, 1280, True): 28 * 576}


def linear_backward_pays(rows, K, N, dtype, need_dweight):
    """Whether forward + backward on the HIP kernels is faster than F.linear under autograd for this shape class — the routing's second
    question after linear_gates. Measured by tools/bench_linear_bwd.py (profiles/linear_bwd_bench.json; DESIGN.md 'Projections under
    autograd'): forward + backward by device events, the two routes alternating in one process, 9 pairs, medians; a class goes to HIP
    only where its median beats the F.linear route's by more than that route's spread. ms HIP / PyTorch (spread), dx only | all
    gradients, bf16 (f16: the JSON):
      129024 x  320 ->  320   0.239 / 0.193 (0.006) | 0.300 / 0.618 (0.020)    dx only LOSES, all gradients wins
      258048 x  320 ->  320   0.198 / 0.338 (0.004) | 0.327 / 0.987 (0.011)    wins
      129024 x  320 ->  960   0.271 / 0.338 (0.050) | 0.438 / 0.817 (0.013)    wins
      258048 x  320 ->  960   0.390 / 0.613 (0.041) | 0.679 / 1.528 (0.030)    wins
      129024 x 1280 ->  320   0.334 / 0.365 (0.020) | 0.473 / 0.897 (0.016)    dx only UNSTEADY (lost one of three runs), all gradients wins
      258048 x 1280 ->  320   0.550 / 0.670 (0.014) | 0.920 / 1.793 (0.067)    wins
       32256 x  640 ->  640   0.108 / 0.118 (0.007) | 0.165 / 0.306 (0.008)    dx only UNSTEADY (lost two of three runs), all gradients wins
       64512 x  640 ->  640   0.145 / 0.232 (0.005) | 0.292 / 0.596 (0.045)    wins
       16128 x 1280 -> 1280   0.173 / 0.188 (0.032) | 0.273 / 0.360 (0.052)    dx only LOSES, all gradients wins
    The tool ran three times; a class is routed only if it won every time (the small dx-only classes are bound by the host side of two
    launches and change sides between runs). The other shapes of the list — 640 -> 1920, 2560 -> 640, 1280 -> 3840, 5120 -> 1280 at
    every size and 1280 -> 1280 at 8064 rows — are outside linear_gates (their forward, or the projection that is their input gradient,
    is the library's) and were measured for the wgrad kernel alone. Unmeasured classes are not routed. One machine."""
    lo = LINEAR_BACKWARD_ROUTED.get((N, K, bool(need_dweight)))
    return lo is not None and rows >= lo


def linear_gates(rows, K, N, dtype):
    """Do the launches of _LinearFn take x [rows, K] and weight [N, K]? The forward's conditions (_linear_route: linear()'s own), the same
    with K and N swapped for the input gradient, csrc/linear_wgrad.hip's gate (K and N multiples of 64), and byte offsets of the
    activations inside 32 bits (what the forward kernels address with)."""
    from . import hip_ops
    if dtype not in (torch.bfloat16, torch.float16) or rows <= 0 or K <= 0 or N <= 0 or K % 64 or N % 64:
        return False
    return (rows * max(K, N) * 2 < 2 ** 32 and _linear_route(rows, K, N, dtype) is not None
            and _linear_route(rows, N, K, dtype) is not None and hip_ops.linear_dgrad_kernel(K, N, dtype) is not None
            and hip_ops.linear_wgrad_supported(K, N, dtype))


def _linear_transposed(weight):
    """W^T [K, N], contiguous: the weight of the input gradient. Kept in svd/derived.py's table while the weight is frozen, built from
    the live tensor while it trains (it changes every step)."""
    def build(w):
        return w.detach().t().contiguous()
    if weight.requires_grad:
        return build(weight)
    from .derived import derived1
    return derived1("linear_transposed", weight, build)


class _LinearFn(torch.autograd.Function):
    """linear() on the kernel it launches without autograd (y is bit-identical to inference) with a deterministic HIP backward: dx is a
    forward kernel on the transposed weight, dweight and dbias are one launch of csrc/linear_wgrad.hip, each only where asked for.
    Holds x and weight only; nothing is cached outside ctx, so torch.utils.checkpoint may re-run the forward."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import hip_ops
        ctx.save_for_backward(x, weight)
        ctx.bias_dtype = None if bias is None else bias.dtype
        route = _linear_route(x.numel() // max(x.shape[-1], 1), x.shape[-1], weight.shape[0], x.dtype)
        if route is None:
            raise HipPathError("linear: _LinearFn reached without a forward kernel for this shape")
        return (hip_ops.linear_n320 if route == "n320" else hip_ops.linear_k320)(x, weight, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        x, weight = ctx.saved_tensors
        n = ctx.needs_input_grad
        dx = hip_ops.linear_dgrad(dy, _linear_transposed(weight)) if n[0] else None
        dw = db = None
        if n[1] or n[2]:
            dw, db = hip_ops.linear_wgrad(x, dy, n[2])
            dw = dw.to(weight.dtype) if n[1] else None
            db = db.to(ctx.bias_dtype) if n[2] else None
        return dx, dw, db


def linear(x, weight, bias=None):
    """F.linear(x, weight, bias). On the GPU, the K = 320 projections of the level-0 transformer blocks (packed q/k/v, to_out,
    proj_in / proj_out: output-bound GEMMs around a 20-step loop) take csrc/ff_geglu.hip's plain-epilogue kernel
    (mvi_linear_k320), the level-0 projections INTO 320 channels with a long contraction (FeedForward.net[2], K = 1280) take
    csrc/linear_n320.hip (mvi_linear_n320), and so do the projections into 640 / 1280 channels of levels 1 and 2 (N320_GROUPS above);
    everything else is the library GEMM. Under autograd with LINEAR_BACKWARD on: _LinearFn where the launches take the shape
    (linear_gates) and linear_backward_pays says so; F.linear otherwise, as without the switch."""
    if LINEAR_BACKWARD and x.is_cuda and _needs_autograd(x, weight, bias) and x.dtype == weight.dtype and weight.dim() == 2 \
            and weight.is_cuda and weight.shape[1] == x.shape[-1] and (bias is None or (bias.is_cuda and bias.shape == weight.shape[:1])):
        rows = x.numel() // max(x.shape[-1], 1)
        if linear_gates(rows, x.shape[-1], weight.shape[0], x.dtype) \
                and linear_backward_pays(rows, x.shape[-1], weight.shape[0], x.dtype, weight.requires_grad or (bias is not None and bias.requires_grad)):
            return _LinearFn.apply(x, weight, bias)
    if K320_KERNELS and N320_KERNEL and N320_GROUPS and x.is_cuda and weight.shape[0] in N320_GROUP_WIDTHS and x.dtype == weight.dtype \
            and not _needs_autograd(x, weight, bias):
        rows = x.numel() // max(x.shape[-1], 1)
        if (rows + 255) // 256 * (weight.shape[0] // 320) >= N320_GROUP_MIN_BLOCKS:
            from . import hip_ops
            if hip_ops.linear_n320_supported(x.shape[-1], weight.shape[0], x.dtype):
                return hip_ops.linear_n320(x, weight, bias)
    if K320_KERNELS and x.is_cuda and not _needs_autograd(x, weight, bias) and x.dtype == weight.dtype \
            and x.numel() // max(x.shape[-1], 1) >= FF_GEGLU_MIN_ROWS:
        from . import hip_ops
        n320 = N320_KERNEL and weight.shape[0] == 320 and hip_ops.linear_n320_supported(x.shape[-1], weight.shape[0], x.dtype)
        if n320 and x.shape[-1] == 320:            # 320 -> 320 (to_out, proj_in / proj_out): both kernels apply, this one is 6 % faster (93 / 99 us)
            return hip_ops.linear_n320(x, weight, bias)
        if hip_ops.linear_k320_supported(x.shape[-1], weight.shape[0], x.dtype):
            return hip_ops.linear_k320(x, weight, bias)
        if n320:
            return hip_ops.linear_n320(x, weight, bias)
    return F.linear(x, weight, bias)


def linear_module(mod, x):
    """`mod(x)` for an nn.Linear (or Sequential(Linear, Dropout) at inference) through linear()."""
    lin = _plain_linear(mod)
    return mod(x) if lin is None else linear(x, lin.weight, lin.bias)


def bias_residual_add(h, bias=None, x=None):
    """h [N, C, *spatial] + bias[c] + x in one pass (conv bias and ResBlock skip add, openaimodel.py:354)."""
    if h.is_cuda and not _needs_autograd(h, bias, x):
        from . import hip_ops
        return hip_ops.bias_residual_add(h, bias, x)
    _fallback(h, "bias_residual_add", _why(h, bias, x))
    out = h
    if bias is not None:
        out = out + bias.to(h.dtype).reshape(1, -1, *([1] * (h.ndim - 2)))
    if x is not None:
        out = out + x
    return out


def concat_add(h, skip, ctrl=None):
    """torch.cat([h, skip + ctrl], dim=1) — the decoder's skip concatenation with the ControlNet residual added on the
    way (models/csvd.py:79-91) — as one pass over contiguous NCHW activations."""
    if (h.is_cuda and not _needs_autograd(h, skip, ctrl) and h.dtype == skip.dtype and (ctrl is None or ctrl.dtype == h.dtype)
            and h.is_contiguous() and skip.is_contiguous() and (ctrl is None or (ctrl.is_contiguous() and ctrl.shape == skip.shape))
            and h.shape[0] < 65536):
        from . import hip_ops
        return hip_ops.concat_add(h, skip, ctrl)
    _fallback(h, "concat_add", _why(h, skip, ctrl))
    return torch.cat([h, skip if ctrl is None else skip + ctrl], dim=1)


def bias_residual_blend(h, bias, x, alpha):
    """alpha * x + (1 - alpha) * (x + h + bias[c]) = x + (1 - alpha) * (h + bias[c]) in one pass; alpha [N] per sample
    (the temporal ResBlock's skip add followed by AlphaBlender, video_model.py:67-81, util.py:358-372)."""
    if h.is_cuda and not _needs_autograd(h, bias, x, alpha):
        from . import hip_ops
        return hip_ops.bias_residual_blend(h, bias, x, alpha)
    _fallback(h, "bias_residual_blend", _why(h, bias, x, alpha))
    xt = bias_residual_add(h, bias, x)
    return torch.lerp(xt, x, alpha.reshape(-1, *([1] * (h.ndim - 1))).to(x.dtype))


def bias_silu(h, bias):
    """silu(h + bias[c]) for a convolution output h [N, C, *spatial] whose bias was withheld (one pass; may reuse h)."""
    if h.is_cuda and not _needs_autograd(h, bias) and h.is_contiguous():
        from . import hip_ops
        return hip_ops.bias_silu(h, bias)
    _fallback(h, "bias_silu", _why(h, bias))
    if bias is not None:
        h = h + bias.to(h.dtype).reshape(1, -1, *([1] * (h.ndim - 2)))
    return F.silu(h)


# The HIP backward of add_layer_norm (csrc/layernorm_bwd.hip). MVI_LN_BWD=0 (or ops.LAYERNORM_BACKWARD = False): add_layer_norm under
# autograd takes PyTorch-ROCm's differentiable ops again (two adds and F.layer_norm), as every op without a HIP backward does.
LAYERNORM_BACKWARD = os.environ.get("MVI_LN_BWD", "1") != "0"
# Smallest rows * C of each (dtype, variant) class from which every measured size won, with all gradients and with the norm frozen
# (profiles/layernorm_bwd_bench.json); a class without an entry was not measured or did not win, and is not routed. Variants: "plain"
# (no h, no row), "add" (h only), "row" (anything with a row).
LAYERNORM_BACKWARD_MIN_ELEMENTS = {(torch.bfloat16, "plain"): 28 * 2304 * 640, (torch.bfloat16, "add"): 28 * 2304 * 640,
                                   (torch.bfloat16, "row"): 28 * 2304 * 640, (torch.float16, "plain"): 28 * 2304 * 640,
                                   (torch.float16, "row"): 28 * 2304 * 640}


def add_layer_norm_backward_pays(rows, C, dtype, variant):
    """Whether add_layer_norm forward + the fused HIP backward is faster than the PyTorch-ROCm route (two adds, F.layer_norm and their
    backward) for this shape class — the routing's second question after hip_ops.add_layer_norm_backward_supported. Measured by
    tools/bench_layernorm_bwd.py (profiles/layernorm_bwd_bench.json; DESIGN.md 'Add+LayerNorm under autograd'): forward + backward by
    device events, the two routes alternating in one process, 9 pairs, medians; a class goes to HIP only where its median beats the
    PyTorch route's by more than that route's spread, with all gradients AND with the norm frozen. ms HIP / PyTorch (spread), all
    gradients | frozen norm, bf16 then f16:
      28 x 9216 x 320 (82.6 M elements)  plain 0.321 / 1.057 (0.013) | 0.213 / 0.764 (0.009)    0.410 / 1.063 (0.011) | 0.339 / 0.753 (0.009)    wins, wins
                                         add   0.480 / 1.284 (0.037) | 0.356 / 0.990 (0.009)    0.678 / 1.288 (0.763) | 0.468 / 0.982 (0.011)    wins, TIE (one slow PyTorch pair)
                                         row   0.699 / 1.560 (0.016) | 0.482 / 1.256 (0.010)    0.876 / 1.571 (0.233) | 0.483 / 1.241 (0.010)    wins, wins
      28 x 2304 x 640 (41.3 M)           plain 0.205 / 0.339 (0.010) | 0.133 / 0.275 (0.003)    0.201 / 0.336 (0.008) | 0.133 / 0.269 (0.003)    wins, wins
                                         add   0.373 / 0.477 (0.029) | 0.255 / 0.393 (0.008)    0.282 / 0.455 (0.028) | 0.197 / 0.379 (0.006)    wins, wins
                                         row   0.459 / 0.613 (0.012) | 0.320 / 0.530 (0.003)    0.391 / 0.591 (0.007) | 0.272 / 0.511 (0.009)    wins, wins
      28 x 576 x 1280 (20.6 M)           every variant loses or ties in both types (row, all gradients: 0.351 / 0.307 bf16, 0.273 / 0.267 f16)
      14 x 3072 x 320 (13.8 M)           bf16 add 0.177 / 0.221 and row 0.223 / 0.296 win, plain loses (0.246 / 0.193); f16 loses or ties everywhere
      14 x 768 x 640, 14 x 192 x 1280    lose everywhere (0.08 - 0.29 against 0.05 - 0.22)
    Below 41.3 M the route is bound by the Function's host side (0.07 - 0.28 ms per forward + backward, varying within the process, against
    0.04 - 0.24 for the PyTorch route) and the verdict is not monotone in the size, so the line is the smallest size from which every
    measured size won: 41.3 M elements; f16 "add" tied at 82.6 M and is not routed at all. The training latent's shapes stay on PyTorch."""
    return rows * C >= LAYERNORM_BACKWARD_MIN_ELEMENTS.get((dtype, variant), float("inf"))


def _ln_variant(h, row):
    return "row" if row is not None else ("add" if h is not None else "plain")


class _AddLayerNormFn(torch.autograd.Function):
    """add_layer_norm on its inference kernel with the fused deterministic HIP backward (csrc/layernorm_bwd.hip). Outputs: y, then s
    when there is an h or a row, then s_pre when it is a tensor of its own (ret_pre with both h and row); an input is never returned.
    Holds s (x for the plain norm) and the norm's weight — no statistics, nothing tensor-sized in fp32; nothing is cached outside ctx,
    so torch.utils.checkpoint may re-run the forward. The gradients of x and h are ONE tensor."""

    @staticmethod
    def forward(ctx, x, h, row, weight, bias, eps, ret_pre):
        from . import hip_ops
        y, s, s_pre = hip_ops.add_layer_norm(x, weight, bias, eps, h=h, row=row, ret_pre=ret_pre)
        own_pre = ret_pre and h is not None and row is not None
        ctx.save_for_backward(x if s is None else s, weight)
        ctx.set_materialize_grads(False)
        ctx.cfg = (float(eps), None if row is None else (tuple(row.shape), row.dtype, row.numel() // x.shape[-1]), tuple(x.shape), bias.dtype)
        if s is None:
            return y
        return (y, s, s_pre) if own_pre else (y, s)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gs=None, gs_pre=None):
        from . import hip_ops
        s, weight = ctx.saved_tensors
        eps, row_info, x_shape, bias_dtype = ctx.cfg
        n = ctx.needs_input_grad
        need_g, need_par, need_drow = n[0] or n[1], n[3] or n[4], row_info is not None and n[2]
        if (gy is None and gs is None and gs_pre is None) or not (need_g or need_par or need_drow):
            return (None,) * 7
        g, dw, db, drow = hip_ops.add_layer_norm_backward(s, weight, eps, gy=gy, gs=gs, gs_pre=gs_pre,
                                                          row_groups=row_info[2] if need_drow else None, need_dx=need_g,
                                                          need_dparams=need_par)
        if g is not None:
            g = g.reshape(x_shape)
        return (g if n[0] else None, g if n[1] else None, drow.to(row_info[1]).reshape(row_info[0]) if need_drow else None,
                dw.to(weight.dtype) if n[3] else None, db.to(bias_dtype) if n[4] else None, None, None)


def _ln_hip_autograd(x, norm, h, row):
    """Under autograd: does this add_layer_norm run _AddLayerNormFn? (switch on, affine norm, the kernels compute the width, and it pays)"""
    if not (x.is_cuda and LAYERNORM_BACKWARD and norm.elementwise_affine and x.numel() > 0):
        return False
    from . import hip_ops
    C_ = x.shape[-1]
    if tuple(norm.normalized_shape) != (C_,) or (h is not None and (h.shape != x.shape or h.dtype != x.dtype)) \
            or (row is not None and (row.dtype != x.dtype or row.shape[-1] != C_ or (x.numel() // C_) % max(row.numel() // C_, 1))):
        return False
    return (hip_ops.layernorm_supported(C_, x.dtype) and hip_ops.add_layer_norm_backward_supported(C_, x.dtype)
            and add_layer_norm_backward_pays(x.numel() // C_, C_, x.dtype, _ln_variant(h, row)))


def add_layer_norm(x, norm, h=None, row=None, ret_pre=False):
    """Residual add(s) fused with the next LayerNorm: s_pre = x + h, s = s_pre + row, y = norm(s) for token-major
    x [B, S, C]; `row` [G, 1, C] (G divides B*S) is broadcast over equal runs of rows — the single-token
    cross-attention row or the frame-index embedding. Returns (y, s, s_pre); s is x when h and row are None,
    s_pre is returned only with ret_pre (and is s when row is None). `norm` is the nn.LayerNorm. Under autograd the same kernel
    runs inside _AddLayerNormFn where the HIP backward is supported and pays (add_layer_norm_backward_pays)."""
    C_ = x.shape[-1]
    if x.is_cuda and not _needs_autograd(x, h, row, norm.weight, norm.bias):
        from . import hip_ops
        if norm.elementwise_affine and hip_ops.layernorm_supported(C_, x.dtype):
            y, s, s_pre = hip_ops.add_layer_norm(x, norm.weight, norm.bias, norm.eps, h=h, row=row, ret_pre=ret_pre)
            return y, (x if s is None else s), s_pre
    elif _ln_hip_autograd(x, norm, h, row):
        out = _AddLayerNormFn.apply(x, h, row, norm.weight, norm.bias, norm.eps, bool(ret_pre))
        if h is None and row is None:
            return out, x, (x if ret_pre else None)
        y, s = out[0], out[1]
        return y, s, ((out[2] if len(out) == 3 else (x if h is None else s)) if ret_pre else None)
    _fallback(x, "add_layer_norm", _why(x, h, row, norm.weight, norm.bias))
    s_pre = x if h is None else x + h
    s = s_pre
    if row is not None:
        G = row.reshape(-1, C_).shape[0]
        rows = x.numel() // C_
        s = (s_pre.reshape(G, rows // G, C_) + row.reshape(G, 1, C_)).reshape(x.shape)
    return norm(s), s, (s_pre if ret_pre else None)


LN_EPILOGUE = os.environ.get("MVI_LN_EPILOGUE", "1") != "0"    # MVI_LN_EPILOGUE=0: projection and add + LayerNorm as two kernels (same-box A/B)


def _plain_linear(mod):
    if isinstance(mod, torch.nn.Sequential) and len(mod) == 2 and isinstance(mod[0], torch.nn.Linear) \
            and isinstance(mod[1], torch.nn.Dropout) and not (mod[1].training and mod[1].p > 0):
        return mod[0]
    return mod if type(mod) is torch.nn.Linear else None


def linear_add_layer_norm(lin_in, lin_mod, resid, norm, row=None, ret_pre=False):
    """add_layer_norm(resid, norm, h=lin_mod(lin_in), row=row, ret_pre=ret_pre) — the projection that ends an attention / FeedForward
    layer, the residual add(s) behind it and the LayerNorm of the NEXT layer (attention.py:544-572, video_attention.py:110-141).
    With resid None the sum starts from the projection itself (proj_in followed by norm1). On the GPU at the level-0 width (320
    outputs: a block of csrc/linear_n320.hip holds whole rows) all of it is ONE kernel: the projection's result and its read-back
    never touch memory (hip_ops.linear_n320_add_layer_norm); everywhere else it is linear_module + add_layer_norm."""
    lin = _plain_linear(lin_mod)
    if LN_EPILOGUE and K320_KERNELS and N320_KERNEL and lin is not None and lin_in.is_cuda and lin.out_features == 320 \
            and isinstance(norm, torch.nn.LayerNorm) and norm.elementwise_affine and tuple(norm.normalized_shape) == (320,) \
            and lin_in.dtype == lin.weight.dtype and lin_in.numel() // max(lin_in.shape[-1], 1) >= FF_GEGLU_MIN_ROWS \
            and not _needs_autograd(lin_in, lin.weight, lin.bias, resid, row, norm.weight, norm.bias):
        from . import hip_ops
        if hip_ops.linear_n320_supported(lin_in.shape[-1], 320, lin_in.dtype) and (resid is None or resid.dtype == lin_in.dtype) \
                and (row is None or row.dtype == lin_in.dtype):
            return hip_ops.linear_n320_add_layer_norm(lin_in, lin.weight, lin.bias, norm.weight, norm.bias, norm.eps, resid=resid, row=row,
                                                      ret_pre=ret_pre)
    return finish_add_layer_norm(linear_module(lin_mod, lin_in), dict(resid=resid, norm=norm, row=row, ret_pre=ret_pre))


def finish_add_layer_norm(h, fuse):
    """The unfused form of a `fuse` request ({resid, norm, row, ret_pre}) for a layer output h that already exists."""
    resid, row, ret_pre = fuse.get("resid"), fuse.get("row"), fuse.get("ret_pre", False)
    if resid is None:
        return add_layer_norm(h, fuse["norm"], row=row, ret_pre=ret_pre)
    return add_layer_norm(resid, fuse["norm"], h=h, row=row, ret_pre=ret_pre)


# The block tails under autograd (csrc/block_tails_bwd.hip): tokens_to_planes_add, tokens_blend_to_planes, add_lerp and planes_to_tokens
# keep their one-pass HIP forward when a graph is recorded, with a fused deterministic backward — the transposition of dy, the scaled
# copies and the sums dbias / dalpha (the gradient of time_mixer.mix_factor) without atomics. DEFAULT OFF (MVI_BLOCK_TAILS_BWD=1 or
# ops.BLOCK_TAILS_BACKWARD = True turns it on): off, every function below is exactly the function it was.
BLOCK_TAILS_BACKWARD = os.environ.get("MVI_BLOCK_TAILS_BWD", "0") == "1"
# Classes tools/bench_block_tails_bwd.py showed to win (profiles/block_tails_bwd_bench.json): {(kind, C, S, need_dparams): the smallest
# measured N (add_lerp: row count R, S = rows per alpha) from which every measured size of the class won in both dtypes, in every run of
# the tool}. A class that is not listed is not routed. Kinds: "planes_add" (tokens_to_planes_add), "planes_blend"
# (tokens_blend_to_planes), "add_lerp", "to_tokens" (planes_to_tokens).
BLOCK_TAILS_BACKWARD_ROUTED = {
    ("planes_add", 320, 9216, True): 14, ("planes_add", 320, 9216, False): 14, ("planes_add", 640, 2304, True): 28,
    ("planes_add", 640, 2304, False): 14, ("planes_add", 1280, 576, True): 28, ("planes_add", 1280, 576, False): 28,
    ("planes_blend", 320, 9216, True): 14, ("planes_blend", 320, 9216, False): 14, ("planes_blend", 640, 2304, True): 14,
    ("planes_blend", 640, 2304, False): 14, ("planes_blend", 1280, 576, True): 14, ("planes_blend", 1280, 576, False): 28,
    ("planes_blend", 1280, 144, True): 28, ("planes_blend", 1280, 144, False): 28,
    ("add_lerp", 320, 9216, True): 14 * 9216, ("add_lerp", 320, 9216, False): 28 * 9216, ("add_lerp", 640, 2304, True): 14 * 2304,
    ("add_lerp", 640, 2304, False): 28 * 2304, ("add_lerp", 1280, 576, True): 28 * 576,
    ("to_tokens", 320, 9216, False): 14, ("to_tokens", 640, 2304, False): 14, ("to_tokens", 1280, 576, False): 28}


def block_tails_backward_pays(kind, N_or_R, C, S, dtype, need_dparams):
    """Whether the tail's forward + the HIP backward is faster than the PyTorch-ROCm composition under autograd for this shape class —
    the routing's second question after hip_ops.block_tails_backward_supported. The rule ops.linear_backward_pays documents: a class
    is routed only if it won every time it was measured (tools/bench_block_tails_bwd.py, profiles/block_tails_bwd_bench.json; DESIGN.md
    'Block tails under autograd'), and anything unmeasured is not routed. Forward + backward by device events, the two routes
    alternating in one process, 9 pairs, medians; a win is a HIP median below the PyTorch median by more than that route's spread, in
    bf16 AND f16, in each of three runs of the tool. ms HIP / PyTorch (spread), all gradients | bias and alpha frozen, bf16 of the
    last run (f16: the JSON):
      planes_add    14 x  320 x 9216   0.248 / 0.513 (0.012) | 0.221 / 0.452 (0.006)    wins
                    28 x  320 x 9216   0.300 / 1.129 (0.019) | 0.263 / 1.033 (0.008)    wins
                    14 x  640 x 2304   0.251 / 0.262 (0.013) | 0.205 / 0.232 (0.007)    all gradients UNSTEADY (lost one of three runs), frozen wins
                    28 x  640 x 2304   0.149 / 0.473 (0.012) | 0.126 / 0.436 (0.003)    wins
                    14 x 1280 x  576   0.242 / 0.170 (0.040) | 0.197 / 0.139 (0.007)    LOSES in bf16 (f16 wins)
                    28 x 1280 x  576   0.111 / 0.240 (0.004) | 0.084 / 0.221 (0.004)    wins
                    .. x 1280 x  144   loses at both sizes (0.109 / 0.094 at 28)
      planes_blend  14 x  320 x 9216   0.298 / 0.977 (0.029) | 0.226 / 0.598 (0.010)    wins
                    28 x  320 x 9216   0.347 / 1.838 (0.018) | 0.244 / 1.180 (0.014)    wins
                    14 x  640 x 2304   0.301 / 0.514 (0.007) | 0.234 / 0.324 (0.007)    wins
                    28 x  640 x 2304   0.165 / 0.832 (0.005) | 0.115 / 0.587 (0.012)    wins
                    14 x 1280 x  576   0.290 / 0.301 (0.007) | 0.231 / 0.198 (0.006)    all gradients wins, frozen LOSES in bf16
                    28 x 1280 x  576   0.136 / 0.439 (0.006) | 0.098 / 0.310 (0.004)    wins
                    14 x 1280 x  144   0.288 / 0.263 (0.024) | 0.227 / 0.192 (0.059)    UNSTEADY
                    28 x 1280 x  144   0.174 / 0.220 (0.042) | 0.130 / 0.162 (0.031)    wins
      add_lerp      14 x 9216 x  320   0.308 / 0.524 (0.007) | 0.238 / 0.217 (0.003)    all gradients wins, frozen UNSTEADY
                    28 x 9216 x  320   0.431 / 0.935 (0.011) | 0.333 / 0.390 (0.012)    wins
                    14 x 2304 x  640   0.283 / 0.308 (0.014) | 0.246 / 0.172 (0.008)    all gradients wins, frozen LOSES
                    28 x 2304 x  640   0.214 / 0.402 (0.007) | 0.162 / 0.205 (0.004)    wins
                    14 x  576 x 1280   0.284 / 0.210 (0.067) | 0.246 / 0.170 (0.009)    LOSES
                    28 x  576 x 1280   0.145 / 0.210 (0.006) | 0.110 / 0.108 (0.062)    all gradients wins, frozen TIES
                    .. x  144 x 1280   loses everywhere
      to_tokens     wins at 320 x 9216 and 640 x 2304 at both sizes and at 28 x 1280 x 576; loses in bf16 at 14 x 1280 x 576 and
                    everywhere at 1280 x 144
    The kernels themselves take 8 - 180 us; below about 20 M elements a forward + backward is bound by the host side of the Function
    (0.07 - 0.25 ms, the first type measured in a process — bf16 — slower than the second), which is why the small classes lose or
    change sides and why N = 14 can lose where N = 28 wins. One machine."""
    lo = BLOCK_TAILS_BACKWARD_ROUTED.get((kind, int(C), int(S), bool(need_dparams)))
    return lo is not None and N_or_R >= lo


def _rg(t):
    return t is not None and t.requires_grad


def _tails_planes_route(kind, tok, bias, N, C_, S, need_dparams):
    """Under autograd with the switch on: do the tail's launches take tok [N, S, C] (+ bias [C]), and does the route pay?"""
    from . import hip_ops
    return (tok.dim() == 3 and tok.dtype in (torch.bfloat16, torch.float16) and tok.numel() > 0
            and (bias is None or (bias.is_cuda and tuple(bias.shape) == (C_,)))
            and hip_ops.block_tails_backward_supported(C_, S, tok.dtype)
            and block_tails_backward_pays(kind, N, C_, S, tok.dtype, need_dparams))


class _TokensToPlanesAddFn(torch.autograd.Function):
    """tokens_to_planes_add on its inference kernel; backward: d_x_in is dy itself, d_tok its transposition (the planes_to_tokens kernel
    when the bias is frozen or absent, csrc/block_tails_bwd.hip with dbias otherwise). Saves nothing."""

    @staticmethod
    def forward(ctx, tok, x_in, bias):
        from . import hip_ops
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.set_materialize_grads(False)
        return hip_ops.tokens_to_planes_add(tok, x_in, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        n = ctx.needs_input_grad
        if dy is None:
            return None, None, None
        d_tok = db = None
        if n[2]:
            d_tok, _, db, _ = hip_ops.planes_tail_backward(dy, need_dtok=n[0], need_dbias=True)
            db = db.to(ctx.bias_dtype)
        elif n[0]:
            d_tok = hip_ops.planes_to_tokens(dy.reshape(dy.shape[0], dy.shape[1], 1, -1))
        return d_tok, (dy if n[1] else None), db


class _TokensBlendToPlanesFn(torch.autograd.Function):
    """tokens_blend_to_planes on its inference kernel with the fused backward of csrc/block_tails_bwd.hip (mode B). Saves alpha; tok and
    bias only when alpha requires grad (its gradient is the one that reads an activation)."""

    @staticmethod
    def forward(ctx, tok, base, bias, alpha, spatial):
        from . import hip_ops
        need_da = ctx.needs_input_grad[3]
        ctx.save_for_backward(alpha, *((tok,) if need_da else ()), *((bias,) if need_da and bias is not None else ()))
        ctx.cfg = (None if bias is None else bias.dtype, need_da, bias is not None)
        ctx.set_materialize_grads(False)
        return hip_ops.tokens_blend_to_planes(tok, base, bias, alpha, spatial)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        n = ctx.needs_input_grad
        if dy is None or not any(n[:4]):
            return (None,) * 5
        bias_dtype, saved_tok, has_bias = ctx.cfg
        saved = ctx.saved_tensors                                      # (read once: checkpoint unpacks a tensor a single time)
        alpha = saved[0]
        tok = saved[1] if saved_tok and n[3] else None
        bias = saved[2] if saved_tok and has_bias and n[3] else None
        d_tok, d_base, db, da = hip_ops.planes_tail_backward(dy, alpha=alpha, tok=tok, bias=bias, need_dtok=n[0], need_dbase=n[1],
                                                             need_dbias=n[2] and has_bias)
        return (d_tok, d_base, db.to(bias_dtype) if db is not None else None,
                da.to(alpha.dtype).reshape(alpha.shape) if da is not None else None, None)


class _AddLerpFn(torch.autograd.Function):
    """add_lerp on its inference kernel with the row pass of csrc/block_tails_bwd.hip as backward: one tensor for d_x and d_h, d_base,
    and dalpha in alpha's own shape and dtype. Saves alpha; x, h, base only when alpha requires grad."""

    @staticmethod
    def forward(ctx, x, h, base, alpha):
        from . import hip_ops
        need_da = ctx.needs_input_grad[3]
        ctx.save_for_backward(alpha, *((x, base) if need_da else ()), *((h,) if need_da and h is not None else ()))
        ctx.cfg = (need_da, h is not None)
        ctx.set_materialize_grads(False)
        return hip_ops.add_lerp(x, h, base, alpha)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        n = ctx.needs_input_grad
        if dy is None or not any(n):
            return (None,) * 4
        saved_x, has_h = ctx.cfg
        saved = ctx.saved_tensors                                      # (read once: checkpoint unpacks a tensor a single time)
        alpha = saved[0]
        x = base = h = None
        if saved_x and n[3]:
            x, base = saved[1], saved[2]
            h = saved[3] if has_h else None
        need_dt = n[0] or (has_h and n[1])
        d_t, d_base, da = hip_ops.rows_tail_backward(dy, alpha, x=x, h=h, base=base, need_dt=need_dt, need_dbase=n[2])
        return (d_t if n[0] else None, d_t if has_h and n[1] else None, d_base,
                da.to(alpha.dtype).reshape(alpha.shape) if da is not None else None)


class _PlanesToTokensFn(torch.autograd.Function):
    """x [N, C, H, W] -> tokens [N, H W, C] on the planes_to_tokens kernel; backward: the tokens_to_planes_add kernel without an addend."""

    @staticmethod
    def forward(ctx, x):
        from . import hip_ops
        ctx.spatial = tuple(x.shape[2:])
        return hip_ops.planes_to_tokens(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import hip_ops
        return hip_ops.tokens_to_planes_add(g, None, spatial=ctx.spatial)


def planes_to_tokens_routed(x):
    """Under autograd: does planes_to_tokens(x) run _PlanesToTokensFn? (switch on, the kernels take the shape, the route pays)"""
    return (BLOCK_TAILS_BACKWARD and x.is_cuda and _needs_autograd(x) and x.dim() == 4 and x.dtype in (torch.bfloat16, torch.float16)
            and x.numel() > 0 and x.shape[1] % 8 == 0 and (x.shape[2] * x.shape[3]) % 8 == 0
            and block_tails_backward_pays("to_tokens", x.shape[0], x.shape[1], x.shape[2] * x.shape[3], x.dtype, False))


def planes_to_tokens(x):
    """x [N, C, H, W] -> [N, (H W), C] ("b c h w -> b (h w) c"), one pass through an LDS tile; under autograd with BLOCK_TAILS_BACKWARD
    on, where the kernels take the shape and the route pays, the same kernel with the opposite one as backward."""
    ok = x.dim() == 4 and x.shape[1] % 8 == 0 and (x.shape[2] * x.shape[3]) % 8 == 0
    if x.is_cuda and not _needs_autograd(x):
        if ok:
            from . import hip_ops
            return hip_ops.planes_to_tokens(x)
    elif planes_to_tokens_routed(x):
        return _PlanesToTokensFn.apply(x)
    _fallback(x, "planes_to_tokens", _why(x))
    return x.flatten(2).transpose(1, 2).contiguous()


def tokens_blend_to_planes_routed(tok, base, bias, alpha):
    """Under autograd: does tokens_blend_to_planes run _TokensBlendToPlanesFn for these tensors?"""
    return (BLOCK_TAILS_BACKWARD and tok.is_cuda and _needs_autograd(tok, base, bias, alpha) and tok.dim() == 3 and base.is_cuda
            and alpha.is_cuda and base.shape == tok.shape and base.dtype == tok.dtype and alpha.numel() == tok.shape[0]
            and _tails_planes_route("planes_blend", tok, bias, tok.shape[0], tok.shape[2], tok.shape[1], _rg(bias) or _rg(alpha)))


def tokens_blend_to_planes(tok, base, bias, alpha, spatial):
    """base + (1 - alpha[n]) * (tok + bias[c]) for token-major tok, base [N, S, C] -> [N, C, *spatial]; alpha [N] per sample: the
    temporal ResBlock's skip add followed by AlphaBlender (alpha x + (1 - alpha)(x + h + b), video_model.py:67-81, util.py:358-372)
    evaluated on tokens, in the pass that restores b c h w. Under autograd with BLOCK_TAILS_BACKWARD on: _TokensBlendToPlanesFn where
    the kernels take the shape and the route pays; on the CPU, or otherwise, the differentiable composition."""
    N, S, C_ = tok.shape
    if tok.is_cuda and not _needs_autograd(tok, base, bias, alpha):
        if C_ % 8 == 0 and S % 8 == 0:
            from . import hip_ops
            return hip_ops.tokens_blend_to_planes(tok, base, bias, alpha, spatial)
    elif tokens_blend_to_planes_routed(tok, base, bias, alpha):
        return _TokensBlendToPlanesFn.apply(tok, base, bias, alpha, tuple(int(v) for v in spatial))
    _fallback(tok, "tokens_blend_to_planes", _why(tok, base, bias, alpha))
    t = tok if bias is None else tok + bias.to(tok.dtype)
    out = torch.lerp(base + t, base, alpha.reshape(N, 1, 1).to(tok.dtype))
    return out.transpose(1, 2).reshape(N, C_, *spatial)


def _add_lerp_route(x, h, base, alpha):
    """Under autograd with the switch on: does add_lerp run _AddLerpFn? (the forward's conditions, 16-bit, and it pays)"""
    from . import hip_ops
    C_ = x.shape[-1]
    G = alpha.numel()
    R = x.numel() // max(C_, 1)
    return (x.is_cuda and base.is_cuda and alpha.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.numel() > 0
            and base.shape == x.shape and base.dtype == x.dtype and (h is None or (h.is_cuda and h.shape == x.shape and h.dtype == x.dtype))
            and G > 0 and R % G == 0 and hip_ops.block_tails_backward_supported(C_, 8, x.dtype)
            and block_tails_backward_pays("add_lerp", R, C_, R // G, x.dtype, alpha.requires_grad))


def add_lerp(x, h, base, alpha):
    """lerp(x + h, base, alpha): alpha * base + (1 - alpha) * (x + h) with alpha [G] broadcast over equal runs of
    the rows of x [B, S, C] (AlphaBlender after the temporal block's last residual add). Under autograd with BLOCK_TAILS_BACKWARD on:
    the same kernel inside _AddLerpFn where it takes the shape and block_tails_backward_pays says so."""
    if x.is_cuda and not _needs_autograd(x, h, base, alpha) and x.shape[-1] % 8 == 0:
        from . import hip_ops
        return hip_ops.add_lerp(x, h, base, alpha)
    if BLOCK_TAILS_BACKWARD and _needs_autograd(x, h, base, alpha) and _add_lerp_route(x, h, base, alpha):
        return _AddLerpFn.apply(x, h, base, alpha)
    _fallback(x, "add_lerp", _why(x, h, base, alpha))
    t = x if h is None else x + h
    C_ = x.shape[-1]
    G = alpha.numel()
    a = alpha.reshape(G, 1, 1).to(x.dtype)
    return torch.lerp(t.reshape(G, -1, C_), base.reshape(G, -1, C_), a).reshape(x.shape)


def tokens_to_planes_add_routed(tok, x_in, bias=None):
    """Under autograd: does tokens_to_planes_add run _TokensToPlanesAddFn for these tensors?"""
    return (BLOCK_TAILS_BACKWARD and tok.is_cuda and _needs_autograd(tok, x_in, bias) and x_in is not None and x_in.is_cuda
            and x_in.dtype == tok.dtype and tok.dim() == 3 and x_in.dim() >= 3 and x_in.shape[0] == tok.shape[0]
            and x_in.shape[1] == tok.shape[2] and x_in.numel() == tok.numel()
            and _tails_planes_route("planes_add", tok, bias, tok.shape[0], tok.shape[2], tok.shape[1], _rg(bias)))


def tokens_to_planes_add(tok, x_in, bias=None):
    """tok [B, (h w), C] (+ bias[c]) -> [B, C, h, w] plus x_in, one pass (SpatialTransformer's exit; ResBlock's exit when its
    convolutions ran channels-last). Under autograd with BLOCK_TAILS_BACKWARD on: the same kernel inside _TokensToPlanesAddFn where
    the backward's kernels take the shape and block_tails_backward_pays says so."""
    if tok.is_cuda and not _needs_autograd(tok, x_in, bias):
        from . import hip_ops
        if tok.shape[-1] % 8 == 0 and tok.shape[1] % 8 == 0:
            return hip_ops.tokens_to_planes_add(tok, x_in, bias)
    elif tokens_to_planes_add_routed(tok, x_in, bias):
        return _TokensToPlanesAddFn.apply(tok, x_in, bias)
    _fallback(tok, "tokens_to_planes_add", _why(tok, x_in))
    t = tok if bias is None else tok + bias.to(tok.dtype)
    return t.transpose(1, 2).reshape(x_in.shape) + x_in


# The 3x3 / padding 1 / stride 1 convolution of token-major activations under autograd: forward and input gradient on
# csrc/linear_n320.hip's implicit GEMM, weight gradient on csrc/conv3x3_wgrad.hip. MVI_CONV3X3_BWD=0 (or ops.CONV3X3_BACKWARD = False):
# a convolution that requires grad takes PyTorch-ROCm's F.conv2d again.
CONV3X3_BACKWARD = os.environ.get("MVI_CONV3X3_BWD", "1") != "0"
CONV3X3_MIN_BLOCKS = 128                 # the forward's fill-the-chip line (layers.CONV_N320_MIN_BLOCKS)
CONV3X3_BACKWARD_MIN_ROWS = 14 * 12 * 16          # from here every measured class won (profiles/conv3x3_bwd_bench.json)
CONV3X3_BACKWARD_MIN_ROWS_SMALL = 14 * 6 * 8      # the smallest measured size: bf16, or f16 without the weight gradient


def conv3x3_backward_pays(N, H, W, C_in, C_out, dtype, need_dweight):
    """Whether forward + backward on the HIP kernels is faster than F.conv2d under autograd for this shape class — the routing's
    second question after conv3x3_tokens_gates. Measured by tools/bench_conv_bwd.py (profiles/conv3x3_bwd_bench.json; DESIGN.md
    '3x3 convolution under autograd'): forward + backward by device events, the two routes alternating in one process, 9 pairs, medians;
    a class goes to HIP only where its median beats the PyTorch route's by more than that route's spread. ms HIP / PyTorch (spread),
    dx only | all gradients, bf16 at N = 14 (N = 28 and f16: the JSON; same verdicts except where noted):
      48x64   320 ->  320   0.314 / 0.524 (0.015) | 0.481 / 0.835 (0.023)    wins
      48x64   640 ->  320   0.401 / 0.811 (0.013) | 0.648 / 1.276 (0.054)    wins
      24x32   640 ->  640   0.292 / 0.467 (0.013) | 0.478 / 0.672 (0.034)    wins
      24x32  1280 ->  640   0.385 / 0.701 (0.029) | 0.711 / 1.073 (0.029)    wins
      12x16  1280 -> 1280   0.231 / 0.432 (0.017) | 0.453 / 0.702 (0.035)    wins
      12x16  2560 -> 1280   0.394 / 0.750 (0.044) | 0.837 / 1.263 (0.013)    wins
       6x8   1280 -> 1280   0.154 / 0.331 (0.019) | 0.303 / 0.491 (0.013)    wins in bf16; f16: dx only wins (0.229 / 0.276, N = 28
                                                                             0.242 / 0.292), all gradients LOSES (0.344 / 0.342, 0.439 / 0.408)
    Every class of 14 x 12x16 pixels and more won in both types, both batch sizes and both gradient sets; the 6x8 level won except in
    f16 with the weight gradient. Nothing below 14 x 6x8 rows was measured and nothing there is routed. One run on one machine."""
    rows = N * H * W
    if rows >= CONV3X3_BACKWARD_MIN_ROWS:
        return True
    if rows >= CONV3X3_BACKWARD_MIN_ROWS_SMALL:
        return dtype == torch.bfloat16 or not need_dweight
    return False


def conv3x3_tokens_gates(N, H, W, C_in, C_out, dtype):
    """Do the three launches of the "s1" form under autograd take this shape? The forward's launch gate (hip_ops.conv_n320_launch_ok: the
    kernel's channel gate, 32-bit byte offsets, enough blocks or a K split), the same with the channel roles swapped for the input
    gradient, and csrc/conv3x3_wgrad.hip's gate."""
    from . import hip_ops
    ok, mb = hip_ops.conv_n320_launch_ok, CONV3X3_MIN_BLOCKS
    # (the two byte bounds, rows C_in 2 and rows C_out 2 within 32 bits, are together rows max(C_in, C_out) 2 < 2^32)
    return (ok("s1", N, H, W, C_in, C_out, dtype, mb) and ok("s1", N, H, W, C_out, C_in, dtype, mb)
            and hip_ops.conv3x3_wgrad_supported(C_in, C_out, dtype) and W <= hip_ops.CONV3X3_WGRAD_MAX_W)



# The two resampling forms of that convolution under autograd — stride 2 (Downsample.op) and the convolution of the nearest-neighbour 2x
# upsampled image (Upsample.conv) — on token-major activations: forwards on csrc/linear_n320.hip as at inference; the stride-2 input
# gradient on its zero-stuffed-source form (mvi_conv3x3_s2_dgrad), the stride-2 weight gradient on csrc/conv3x3_wgrad.hip's stride-2
# form, the upsampling form's input gradient as the stride-1 dgrad at 2 h x 2 w + mvi_rows_pool2x2_sum. MVI_RESAMPLE_CONV_BWD=0 (or
# ops.RESAMPLE_CONV_BACKWARD = False): both take PyTorch-ROCm's F.conv2d (F.interpolate + F.conv2d) under autograd again.
RESAMPLE_CONV_BACKWARD = os.environ.get("MVI_RESAMPLE_CONV_BWD", "1") != "0"
RESAMPLE_CONV_MIN_BLOCKS = 128           # the forward's fill-the-chip line (layers.CONV_N320_MIN_BLOCKS); the s2 dgrad has no K split
# Classes tools/bench_resample_conv_bwd.py showed to win (profiles/resample_conv_bwd_bench.json): {(H, W, C, need_dweight): the batch
# sizes N measured ahead, in bf16 AND f16 (the two types had the same verdicts)}; C -> C channels, H x W is the Downsample's input /
# the Upsample's output. Unmeasured classes — any other size, channel count or batch — are not routed.
_B16 = (torch.bfloat16, torch.float16)
CONV3X3_DOWN_BACKWARD_ROUTED = {(72, 128, 320, False): (14, 28), (36, 64, 640, False): (14, 28), (18, 32, 1280, False): (14, 28),
                                (72, 128, 320, True): (14, 28), (18, 32, 1280, True): (14,)}
CONV3X3_UP_BACKWARD_ROUTED = {(72, 128, 320, False): (14, 28), (36, 64, 640, False): (14, 28), (18, 32, 1280, False): (14, 28)}


def conv3x3_down_backward_pays(N, H, W, C_in, C_out, dtype, need_dweight):
    """Whether forward + backward of the stride-2 convolution on the HIP kernels is faster than F.conv2d(stride 2) under autograd on NCHW
    planes (what the training path runs today) for this shape class — the routing's second question after conv3x3_down_tokens_gates.
    The project's standing rule: a class goes to HIP only where tools/bench_resample_conv_bwd.py measured its median ahead of the
    PyTorch route's by more than that route's spread (forward + backward by device events, the two routes alternating in one process,
    9 pairs, medians); unmeasured classes are not routed. ms HIP / PyTorch (spread), dx only | all gradients, bf16, C -> C:
      N = 14  72x128  320   0.359 / 0.522 (0.017) | 0.694 / 0.810 (0.047)    wins | wins
      N = 14  36x64   640   0.331 / 0.422 (0.022) | 0.650 / 0.629 (0.019)    wins | LOSES
      N = 14  18x32  1280   0.484 / 0.786 (0.043) | 0.806 / 1.041 (0.021)    wins | wins
      N = 28  72x128  320   0.523 / 0.960 (0.020) | 1.093 / 1.529 (0.037)    wins | wins
      N = 28  36x64   640   0.526 / 0.666 (0.036) | 1.110 / 0.944 (0.019)    wins | LOSES
      N = 28  18x32  1280   0.525 / 0.702 (0.042) | 1.135 / 1.022 (0.011)    wins | LOSES
    f16 (the JSON): the same verdicts. dx only — the frozen UNet's Downsamples — won everywhere; with the weight gradient the 640-channel
    level and, at N = 28, the 1280-channel level lose: the stride-2 weight-gradient kernel runs at 0.10 of the matrix peak (0.24 ms at
    N = 14 whatever the level) where the library's is faster. One run on one machine."""
    ns = CONV3X3_DOWN_BACKWARD_ROUTED.get((H, W, C_in, bool(need_dweight))) if C_in == C_out and dtype in _B16 else None
    return ns is not None and N in ns


def conv3x3_up_backward_pays(N, h, w, C_in, C_out, dtype):
    """The same question for the upsampling form (frozen weight: dx only) against F.conv2d(F.interpolate(x)) under autograd; h x w is the
    SOURCE size, the table is keyed by the output size 2 h x 2 w. ms HIP / PyTorch (spread), bf16, N = 14 | N = 28 (f16: the JSON, same
    verdicts):
      36x64 -> 72x128  320   0.485 / 1.545 (0.067) | 0.842 / 3.125 (0.052)    wins
      18x32 -> 36x64   640   0.442 / 0.970 (0.041) | 0.811 / 1.774 (0.044)    wins
       9x16 -> 18x32  1280   0.694 / 1.000 (0.036) | 0.750 / 1.689 (0.066)    wins
    Every measured class won: the PyTorch route writes, convolves and keeps the 4x tensor. One run on one machine."""
    ns = CONV3X3_UP_BACKWARD_ROUTED.get((2 * h, 2 * w, C_in, False)) if C_in == C_out and dtype in _B16 else None
    return ns is not None and N in ns


def conv3x3_down_tokens_gates(N, H, W, C_in, C_out, dtype):
    """Do the three launches of the "s2" form under autograd take this shape? Even H and W; the forward's launch gate at stride 2
    (hip_ops.conv_n320_launch_ok: channel gate, 32-bit byte offsets, enough blocks or a K split); the zero-stuffed input gradient's with
    the channel roles swapped (C_in a multiple of 320, C_out of 64: mvi_conv3x3_s2_dgrad_supported is the forward's test on swapped
    channels; it has no K split, so its N H W / 256 row blocks x C_in / 320 column groups alone must reach the line); and the
    weight-gradient kernel's gate."""
    from . import hip_ops
    ok, mb = hip_ops.conv_n320_launch_ok, RESAMPLE_CONV_MIN_BLOCKS
    # (N H W C_in 2 of the forward and N H W C_out 2 of the input gradient within 32 bits: N H W max(C_in, C_out) 2 < 2^32)
    return (H % 2 == 0 and W % 2 == 0 and ok("s2", N, H, W, C_in, C_out, dtype, mb) and ok("s2_dgrad", N, H, W, C_out, C_in, dtype, mb)
            and hip_ops.conv3x3_s2_wgrad_supported(C_in, C_out, dtype) and W <= hip_ops.CONV3X3_WGRAD_MAX_W)


def conv3x3_up_tokens_gates(N, h, w, C_in, C_out, dtype):
    """Do the launches of the "up2" form under autograd take this shape (h x w: the source)? The upsampling forward's launch gate (no K
    split), the stride-1 input gradient's at 2 h x 2 w with the channel roles swapped, and the pooling pass's (C_in a multiple of 8:
    implied)."""
    from . import hip_ops
    ok, mb = hip_ops.conv_n320_launch_ok, RESAMPLE_CONV_MIN_BLOCKS
    # (4 N h w C_in 2 of the forward and 4 N h w C_out 2 of the input gradient within 32 bits: 4 N h w max(C_in, C_out) 2 < 2^32)
    return ok("up2", N, h, w, C_in, C_out, dtype, mb) and ok("s1", N, 2 * h, 2 * w, C_out, C_in, dtype, mb)



# The (3, 1, 1) / padding (1, 0, 0) frame convolution of token-major activations under autograd (VideoResBlock.time_stack): forward and
# input gradient on csrc/linear_n320.hip's three-tap implicit GEMM, weight gradient on csrc/conv3t_wgrad.hip. MVI_CONV3T_BWD=0 (or
# ops.CONV3T_BACKWARD = False): a frame convolution that requires grad takes PyTorch-ROCm's F.conv3d again.
CONV3T_BACKWARD = os.environ.get("MVI_CONV3T_BWD", "1") != "0"
CONV3T_MIN_BLOCKS = 128                  # the forward's fill-the-chip line (layers.CONV_N320_MIN_BLOCKS)
CONV3T_BACKWARD_MIN_ROWS = None          # None: no measured class won (profiles/conv3t_bwd_bench.json), nothing is routed by default


def conv3t_backward_pays(B, T, S, C_in, C_out, dtype, need_dweight):
    """Whether forward + backward on the HIP kernels is faster than the channel-stacked 1x1 library convolution under autograd
    (layers.temporal_conv3_stacked, what the training path runs today) for this shape class — the routing's second question after
    conv3t_tokens_gates. Measured by tools/bench_conv3t_bwd.py (profiles/conv3t_bwd_bench.json; DESIGN.md '(3,1,1) frame convolution
    under autograd'): forward + backward by device events, the two routes alternating in one process, 9 pairs, medians; a class goes to
    HIP only where its median beats the PyTorch route's by more than that route's spread. ms HIP / PyTorch (spread), dx only | all
    gradients, (B, T) = (1, 14), C -> C, the PyTorch side on an already stacked input (its stack's cost left out):
      bf16  S 3072  C  320   0.235 / 0.188 (0.023) | 0.366 / 0.395 (0.029)    loses | inside the spread
      bf16  S  768  C  640   0.255 / 0.186 (0.029) | 0.373 / 0.368 (0.051)    loses | loses
      bf16  S  192  C 1280   0.248 / 0.184 (0.017) | 0.372 / 0.379 (0.030)    loses | inside the spread
      bf16  S   48  C 1280   0.250 / 0.173 (0.019) | 0.334 / 0.329 (0.018)    loses | loses
      f16   S 3072  C  320   0.235 / 0.192 (0.018) | 0.381 / 0.403 (0.032)    loses | inside the spread
      f16   S  768  C  640   0.255 / 0.182 (0.016) | 0.377 / 0.338 (0.080)    loses | loses
      f16   S  192  C 1280   0.252 / 0.186 (0.020) | 0.367 / 0.330 (0.021)    loses | loses
      f16   S   48  C 1280   0.251 / 0.174 (0.020) | 0.332 / 0.322 (0.029)    loses | loses
    No class won: the HIP route's forward + input gradient cost 0.24 - 0.26 ms whatever the shape (two launches of the forward kernel
    whose own work is far shorter: the time is the host's), the library's 0.17 - 0.19; the weight-gradient kernel (0.030 - 0.094 ms)
    takes 0.03 - 0.08 ms less of the step than the library's and does not make up for it by more than the spread. So the line is None and every
    shape stays on the route it had; the tests lift the decision. One run on one machine."""
    line = CONV3T_BACKWARD_MIN_ROWS
    return line is not None and B * T * S >= line


def conv3t_tokens_gates(B, T, S, C_in, C_out, dtype):
    """Do the three launches of the "t3" form under autograd take this shape? The forward's launch gate (hip_ops.conv_n320_launch_ok: the
    kernel's channel gate, 32-bit byte offsets, enough blocks or a K split), the same with the channel roles swapped for the input
    gradient, and csrc/conv3t_wgrad.hip's gate."""
    from . import hip_ops
    ok, mb = hip_ops.conv_n320_launch_ok, CONV3T_MIN_BLOCKS
    # (the two byte bounds, rows C_in 2 and rows C_out 2 within 32 bits, are together rows max(C_in, C_out) 2 < 2^32)
    return (ok("t3", B, T, S, C_in, C_out, dtype, mb) and ok("t3", B, T, S, C_out, C_in, dtype, mb)
            and hip_ops.conv3t_wgrad_supported(C_in, C_out, dtype))


# ---- the four forms of the token-major convolution on csrc/linear_n320.hip: one packed-weight pair, one Function, one route -------------

def conv_packed_weight(w):
    """A convolution weight in the implicit-GEMM kernel's order, [C_out][taps C_in] — 3x3 Conv2d weights ([C_out, C_in, 3, 3] -> 9 taps)
    and (3,1,1) Conv3d weights ([C_out, C_in, 3, 1, 1] -> 3 taps, tap-major) — once per parameter version (svd/derived.py). The packing
    order of the 3x3 weights is a process-global switch of the kernel: part of the signature (hip_ops.conv3x3_k_order)."""
    from . import hip_ops
    from .derived import derived1
    if w.dim() == 5:
        return derived1("tap_major", w, lambda w: hip_ops.conv3t_n320_weight(w.detach()))
    return derived1("tap_major", w, lambda w: hip_ops.conv3x3_n320_weight(w.detach()), hip_ops.conv3x3_k_order())


def conv_packed_weight_transposed(w):
    """The transposed weight of the input gradient (hip_ops.conv3x3_transposed_weight / conv3t_transposed_weight) in the same order:
    kept in svd/derived.py's table while the weight is frozen, built from the live tensor while it trains (it changes every step)."""
    from . import hip_ops
    from .derived import derived1
    if w.dim() == 5:
        build, extra = (lambda w: hip_ops.conv3t_n320_weight(hip_ops.conv3t_transposed_weight(w.detach()))), ()
    else:
        build, extra = (lambda w: hip_ops.conv3x3_n320_weight(hip_ops.conv3x3_transposed_weight(w.detach()))), hip_ops.conv3x3_k_order()
    return build(w) if w.requires_grad else derived1("tap_major_transposed", w, build, extra)


# One form of the op (the key is hip_ops.conv_n320_launch_ok's): the hip_ops forward launch and its keyword arguments, the hip_ops input- and
# weight-gradient launches (wgrad None: not built, the form runs under autograd with a frozen weight and bias only; every form takes a
# bias), and the NAMES of this module's switch, fill-the-chip line, gate and speed decision — looked up when called, so what a test or a
# bench sets on the module holds.
_ConvForm = collections.namedtuple("_ConvForm", "launch kwargs dgrad wgrad switch min_blocks gates pays")
_CONV_FORMS = {
    "s1": _ConvForm("conv3x3_n320", {}, "conv3x3_dgrad", "conv3x3_wgrad",
                    "CONV3X3_BACKWARD", "CONV3X3_MIN_BLOCKS", "conv3x3_tokens_gates", "conv3x3_backward_pays"),
    "s2": _ConvForm("conv3x3_n320", {"stride": 2}, "conv3x3_s2_dgrad", "conv3x3_s2_wgrad",
                    "RESAMPLE_CONV_BACKWARD", "RESAMPLE_CONV_MIN_BLOCKS", "conv3x3_down_tokens_gates", "conv3x3_down_backward_pays"),
    "up2": _ConvForm("conv3x3_n320", {"up2": True}, "conv3x3_up2_dgrad", None,
                     "RESAMPLE_CONV_BACKWARD", "RESAMPLE_CONV_MIN_BLOCKS", "conv3x3_up_tokens_gates", "conv3x3_up_backward_pays"),
    "t3": _ConvForm("conv3t_n320", {}, "conv3t_dgrad", "conv3t_wgrad",
                    "CONV3T_BACKWARD", "CONV3T_MIN_BLOCKS", "conv3t_tokens_gates", "conv3t_backward_pays"),
}


def _conv_launch(f, tok, weight, bias, geom):
    from . import hip_ops
    return getattr(hip_ops, f.launch)(tok, conv_packed_weight(weight), bias, *geom, **f.kwargs)


class _ConvTokensFn(torch.autograd.Function):
    """A token-major convolution on the implicit-GEMM kernel — the inference launch, the bias in its accumulators, so y has the same
    bits — with a deterministic HIP backward: geom is (H, W) of the image the op is handed, or (T,) for "t3".
      dx       the form's input gradient on the forward kernel with the transposed weight (W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx];
               "t3": W'[ci, co, kt] = W[co, ci, 2 - kt]): the same launch ("s1", "t3"), its zero-stuffed form ("s2"), or the stride-1
               launch at 2 h x 2 w summed over every 2x2 cell ("up2": one more rounding than a bare dgrad)
      dweight  csrc/conv3x3_wgrad.hip, its stride-2 form, csrc/conv3t_wgrad.hip
      dbias    the fp32 sum of dy over rows
    each only where needs_input_grad asks. Holds tok and weight — "up2", which has no weight gradient, the weight only: neither its input
    nor the 4x upsampled activation is kept — never y, and nothing is cached outside ctx, so torch.utils.checkpoint may re-run the forward."""

    @staticmethod
    def forward(ctx, form, tok, weight, bias, *geom):
        f = ctx.form = _CONV_FORMS[form]
        ctx.save_for_backward(*((tok, weight) if f.wgrad else (weight,)))
        ctx.geom = geom
        ctx.bias_dtype = None if bias is None else bias.dtype
        return _conv_launch(f, tok, weight, bias, geom)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        f, geom = ctx.form, ctx.geom
        *tok, weight = ctx.saved_tensors
        _, need_dx, need_dw, need_db = ctx.needs_input_grad[:4]
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx = getattr(hip_ops, f.dgrad)(dy, conv_packed_weight_transposed(weight), *geom) if need_dx else None
        dw = getattr(hip_ops, f.wgrad)(tok[0], dy, *geom).to(weight.dtype) if need_dw else None
        db = dy.sum(dim=(0, 1), dtype=torch.float32).to(ctx.bias_dtype) if need_db else None
        return (None, dx, dw, db) + (None,) * len(geom)


def _conv_tokens_route(form, tok, weight, bias, geom, dims):
    """The triage of the four public ops below for a validated call; dims = (N, H, W, C_in, C_out) as the form's gate takes them. Without
    autograd: the kernel where the launch gate passes. Under autograd: _ConvTokensFn where the form's switch is on, its *_tokens_gates
    pass and its *_backward_pays says so (a form without a weight gradient: only with weight and bias frozen). None otherwise: the
    caller records the fallback and runs its PyTorch expression."""
    if not (tok.is_cuda and tok.dtype == weight.dtype):
        return None
    f, g = _CONV_FORMS[form], globals()
    if not _needs_autograd(tok, weight, bias):
        from . import hip_ops
        if hip_ops.conv_n320_launch_ok(form, *dims, tok.dtype, g[f.min_blocks]):
            return _conv_launch(f, tok, weight, bias, geom)
    elif g[f.switch] and (f.wgrad or not _needs_autograd(weight, bias)) and g[f.gates](*dims, tok.dtype) \
            and g[f.pays](*dims, tok.dtype, *((weight.requires_grad,) if f.wgrad else ())):
        return _ConvTokensFn.apply(form, tok, weight, bias, *geom)
    return None


def conv3x3_tokens(tok, weight, H, W):
    """3x3 / padding 1 / stride 1 convolution of token-major activations tok [N, H W, C_in] with weight [C_out, C_in, 3, 3], no bias
    -> [N, H W, C_out]. Without autograd: the implicit-GEMM kernel. Under autograd: _ConvTokensFn where the switch is on, the three
    launches take the shape (conv3x3_tokens_gates) and conv3x3_backward_pays says so; anything else is F.conv2d on the channels-last
    view (a recorded fallback; strict mode raises)."""
    N, S, C = tok.shape
    Co = weight.shape[0]
    if S == H * W and tuple(weight.shape[1:]) == (C, 3, 3):
        y = _conv_tokens_route("s1", tok, weight, None, (H, W), (N, H, W, C, Co))
        if y is not None:
            return y
    _fallback(tok, "conv3x3_tokens", _why(tok, weight))
    x = tok.view(N, H, W, C).permute(0, 3, 1, 2)                  # [N, C, H, W] with channels-last strides: no copy
    y = F.conv2d(x, weight, None, 1, 1)
    return y.permute(0, 2, 3, 1).reshape(N, S, Co)


def conv3x3_down_tokens(tok, weight, bias, H, W):
    """3x3 / padding 1 / STRIDE 2 convolution (Downsample.op) of token-major activations tok [N, H W, C_in] with weight [C_out, C_in, 3, 3]
    and bias [C_out] or None -> [N, Ho Wo, C_out], Ho = (H - 1) // 2 + 1. Without autograd: the implicit-GEMM kernel. Under autograd:
    _ConvTokensFn where the switch is on, the launches take the shape (conv3x3_down_tokens_gates) and conv3x3_down_backward_pays
    says so; anything else is F.conv2d on the channels-last view (a recorded fallback; strict mode raises) — also the CPU path."""
    N, S, C = tok.shape
    Co = weight.shape[0]
    if S != H * W or tuple(weight.shape[1:]) != (C, 3, 3):
        raise ValueError("conv3x3_down_tokens: tok [N, H W, C_in] and weight [C_out, C_in, 3, 3] expected")
    y = _conv_tokens_route("s2", tok, weight, bias, (H, W), (N, H, W, C, Co))
    if y is not None:
        return y
    _fallback(tok, "conv3x3_down_tokens", _why(tok, weight, bias))
    x = tok.view(N, H, W, C).permute(0, 3, 1, 2)                  # [N, C, H, W] with channels-last strides: no copy
    y = F.conv2d(x, weight, bias, 2, 1)
    return y.permute(0, 2, 3, 1).reshape(N, y.shape[2] * y.shape[3], Co)


def conv3x3_up_tokens(tok, weight, bias, h, w):
    """conv3x3(nearest 2x upsampling of x) (Upsample.conv) of token-major activations tok [N, h w, C_in] -> [N, (2 h)(2 w), C_out]. Without
    autograd: the upsampling form of the implicit-GEMM kernel. Under autograd with a FROZEN weight and bias: _ConvTokensFn where the
    switch is on, the launches take the shape (conv3x3_up_tokens_gates) and conv3x3_up_backward_pays says so. Anything else — a
    trainable weight or bias among it: this form's weight gradient is not built, no trained network has an Upsample — is
    F.conv2d(F.interpolate(x)) on the channels-last view (a recorded fallback; strict mode raises) — also the CPU path."""
    N, S, C = tok.shape
    Co = weight.shape[0]
    if S != h * w or tuple(weight.shape[1:]) != (C, 3, 3):
        raise ValueError("conv3x3_up_tokens: tok [N, h w, C_in] and weight [C_out, C_in, 3, 3] expected")
    y = _conv_tokens_route("up2", tok, weight, bias, (h, w), (N, h, w, C, Co))
    if y is not None:
        return y
    _fallback(tok, "conv3x3_up_tokens", _why(tok, weight, bias))
    x = tok.view(N, h, w, C).permute(0, 3, 1, 2)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), weight, bias, 1, 1)
    return y.permute(0, 2, 3, 1).reshape(N, 4 * S, Co)


def conv3x3_up_dgrad(dy, weight, h, w):
    """dx [N, h w, C_in] of conv3x3_up_tokens from dy [N, (2 h)(2 w), C_out] — the "up2" form's backward: the stride-1 input gradient
    at 2 h x 2 w on the forward kernel, then the sum over every 2x2 cell (one more rounding than a bare dgrad)."""
    from . import hip_ops
    dy = dy if dy.is_contiguous() else dy.contiguous()
    return hip_ops.conv3x3_up2_dgrad(dy, conv_packed_weight_transposed(weight), h, w)


def conv3t_tokens(tok, weight, T):
    """(3, 1, 1) / padding (1, 0, 0) convolution over the frame axis of token-major activations tok [(b T), S, C_in] (the T frames of a
    video consecutive) with weight [C_out, C_in, 3, 1, 1], no bias -> [(b T), S, C_out]. Without autograd: the three-tap implicit-GEMM
    kernel. Under autograd: _ConvTokensFn where the switch is on, the three launches take the shape (conv3t_tokens_gates) and
    conv3t_backward_pays says so; anything else is F.conv3d on the b c t s 1 view (a recorded fallback; strict mode raises) — also the
    CPU path."""
    BT, S, C = tok.shape
    T = int(T)
    Co = weight.shape[0]
    if T < 1 or BT % T or tuple(weight.shape[1:]) != (C, 3, 1, 1):
        raise ValueError("conv3t_tokens: tok [(b T), S, C_in] and weight [C_out, C_in, 3, 1, 1] expected")
    B = BT // T
    y = _conv_tokens_route("t3", tok, weight, None, (T,), (B, T, S, C, Co))
    if y is not None:
        return y
    _fallback(tok, "conv3t_tokens", _why(tok, weight))
    x = tok.reshape(B, T, S, C).permute(0, 3, 1, 2).unsqueeze(-1)              # b c t s 1 (a view)
    y = F.conv3d(x, weight, None, 1, (1, 0, 0))
    return y.squeeze(-1).permute(0, 2, 3, 1).reshape(BT, S, Co)


# The 16- / 32-channel 3x3 convolution + SiLU layers of ControlNet.input_hint_block under autograd: forward on csrc/stem_conv.hip, dz on its
# second epilogue (z recomputed from x), weight / bias gradient on csrc/stem_conv_bwd.hip, the stride-1 C -> C input gradient on the forward
# kernel with the transposed weight. MVI_STEM_CONV_BWD=0 (or ops.STEM_CONV_BACKWARD = False): such a layer takes F.conv2d + F.silu under
# autograd again.
STEM_CONV_BACKWARD = os.environ.get("MVI_STEM_CONV_BWD", "1") != "0"
# (stride, C_out, smallest measured N H_o W_o) of every class that won (profiles/stem_bwd_bench.json); nothing below those sizes is routed
STEM_CONV_BACKWARD_ROUTED = ((1, 16, 14 * 288 * 512), (2, 32, 14 * 144 * 256), (1, 32, 14 * 144 * 256))


def stem_conv_backward_pays(N, C_in, C_out, H, W, stride, dtype, need_dx):
    """Whether forward + backward of one stem layer on the HIP kernels is faster than F.silu(F.conv2d(...)) under autograd for this shape
    class — the routing's second question after stem_conv_gates. Measured by tools/bench_stem_bwd.py (profiles/stem_bwd_bench.json;
    DESIGN.md 'Hint stem under autograd'): forward + backward by device events, the two routes alternating in one process, 9 pairs,
    medians; a class goes to HIP only where its median beats the PyTorch route's by more than that route's spread. ms HIP / PyTorch
    (spread), every parameter trainable, the input's gradient too except in the 7 -> 16 layer, N = 14; bf16 | f16:
      576x1024   7 -> 16      0.644 / 1.724 (0.069) | 0.645 / 1.712 (0.038)    wins
      576x1024  16 -> 16      0.991 / 2.843 (0.043) | 1.027 / 2.730 (0.070)    wins
      576x1024  16 -> 32 s2   0.980 / 1.467 (0.052) | 0.844 / 1.254 (0.078)    wins
      288x512   32 -> 32      0.663 / 1.311 (0.075) | 0.605 / 1.235 (0.115)    wins
      288x512    7 -> 16      0.352 / 0.491 (0.045) | 0.316 / 0.466 (0.009)    wins
      288x512   16 -> 16      0.436 / 0.775 (0.031) | 0.345 / 0.697 (0.038)    wins
      288x512   16 -> 32 s2   0.443 / 0.564 (0.042) | 0.310 / 0.501 (0.020)    wins
      144x256   32 -> 32      0.346 / 0.522 (0.018) | 0.244 / 0.471 (0.012)    wins
    Every measured class won in both types, so each class is routed from its smallest measured size (in output pixels N H_o W_o) up.
    Nothing smaller was measured and nothing smaller is routed. One run on one machine.
    A class is (stride, C_out), the kernel form's own split. C_in, dtype and need_dx are deliberately unused: the table holds the widest
    C_in of each class with the input gradient and both types, and a narrower C_in or a layer without an input gradient does less work on
    the HIP route than the measured shape (the arguments stay in the signature for a later table that needs them)."""
    px = N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    return any(stride == s and C_out == co and px >= line for s, co, line in STEM_CONV_BACKWARD_ROUTED)


def stem_conv_gates(N, C_in, C_out, H, W, stride, dtype, need_dx):
    """Do the launches of _StemConvSiluFn take this shape? The forward's and the backward kernels' gate, and for a layer whose input needs
    a gradient one of the two built cases: stride 1 with C_in == C_out in (16, 32) (the forward kernel on the transposed weight), or the
    stride-2 layer (aten's convolution_backward on dz)."""
    from . import hip_ops
    if not (N > 0 and H > 0 and W > 0 and hip_ops.stem_conv3x3_bwd_supported(C_in, C_out, W, stride, dtype)):
        return False
    return not need_dx or stride == 2 or (C_in == C_out and C_in in (16, 32))


class _StemConvSiluFn(torch.autograd.Function):
    """act(conv2d(x, weight, bias, stride, padding=1)), act = SiLU or nothing, on csrc/stem_conv.hip with a deterministic HIP backward. Holds
    x, weight and bias only — z is recomputed by the dz pass, y is never kept — and caches nothing outside ctx, so torch.utils.checkpoint
    may re-run the forward. Without SiLU dy is dz and no dz pass runs."""

    @staticmethod
    def forward(ctx, x, weight, bias, silu, stride):
        from . import hip_ops
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (bool(silu), int(stride))
        return hip_ops.stem_conv3x3_silu(x, weight, bias, silu=silu, stride=stride)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import hip_ops
        x, weight, bias = ctx.saved_tensors
        silu, stride = ctx.cfg
        nx, nw, nb = ctx.needs_input_grad[:3]
        nb = nb and bias is not None
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dz = hip_ops.stem_conv3x3_dz(x, weight, bias, dy, silu=True, stride=stride) if silu else dy
        dx = dw = db = None
        if nw or nb:
            dw, db = hip_ops.stem_conv3x3_wgrad(x, dz, stride=stride, need_dbias=nb)
            dw = dw.to(weight.dtype) if nw else None
            db = db.to(bias.dtype) if nb else None
        if nx:
            if stride == 1:
                dx = hip_ops.stem_conv3x3_dgrad(dz, weight)
            else:
                # the stride-2 input gradient has no HIP kernel yet (four parity classes of 1, 2, 2 and 4 taps): the library's
                dx = torch.ops.aten.convolution_backward(dz, x, weight, None, [stride, stride], [1, 1], [1, 1], False, [0, 0], 1,
                                                         (True, False, False))[0]
        return dx, dw, db, None, None


def stem_conv3x3_silu(x, weight, bias, silu=True, stride=1):
    """act(conv2d(x, weight, bias, stride, padding=1)) for the 16- / 32-output layers of the hint stem; x [N, C_in, H, W] NCHW. Without
    autograd: hip_ops.stem_conv3x3_silu. Under autograd: _StemConvSiluFn where the switch is on, the launches take the shape
    (stem_conv_gates) and stem_conv_backward_pays says so; anything else is F.conv2d (+ F.silu) (a recorded fallback; strict mode
    raises) — also the CPU path."""
    if (x.is_cuda and x.dim() == 4 and x.dtype == weight.dtype and x.is_contiguous() and weight.dim() == 4
            and tuple(weight.shape[1:]) == (x.shape[1], 3, 3) and stride in (1, 2)):
        from . import hip_ops
        N, Ci, H, W = x.shape
        Co = weight.shape[0]
        if not _needs_autograd(x, weight, bias):
            if hip_ops.stem_conv3x3_bwd_supported(Ci, Co, W, stride, x.dtype) and N > 0:
                return hip_ops.stem_conv3x3_silu(x, weight, bias, silu=silu, stride=stride)
        else:
            need_dx = x.requires_grad
            if STEM_CONV_BACKWARD and stem_conv_gates(N, Ci, Co, H, W, stride, x.dtype, need_dx) \
                    and stem_conv_backward_pays(N, Ci, Co, H, W, stride, x.dtype, need_dx):
                return _StemConvSiluFn.apply(x, weight, bias, silu, stride)
    _fallback(x, "stem_conv3x3_silu", _why(x, weight, bias))
    z = F.conv2d(x, weight, bias, stride, 1)
    return F.silu(z) if silu else z

"""Every forward normalisation and pointwise kernel of the UNet path (csrc/groupnorm_silu.hip, csrc/groupnorm_tokens.hip,
csrc/token_rows.hip, csrc/softmax_rows.hip, csrc/bias_residual.hip, csrc/geglu.hip) against an fp64 reference of the same operation, ELEMENT
BY ELEMENT: |got - ref| <= cap + ulp(|ref| + cap) / 2 with the cap derived in tests/norm_exact_helpers.py, torch.equal where fp32 is exact
(cap = 0) and on the constant group, and the same bits from a second call. The data gives every statistics unit its own mean and scale
(tests/test_norm_elementwise_cpu.py shows what the comparison rejects). All calls go through multiview_inpaint_amd.svd.hip_ops; the only
other thing read from the library is geometry (host functions): the token-major kernels' block length and the first multi-chunk shape.

The constant group has ONE right output, act(bias[c]) rounded once, wherever the type leaves one: bf16 / f16, and fp32 without SiLU
(an fp32 evaluation of the sigmoid has no single right bit pattern; those elements stay under the bound).

Every test writes one line per launch through svd_helpers.report: entry point, shape, type, the worst ratio to the bound, the share of
elements whose cap is below a quarter ulp (profiles/norm_elementwise_gpu.txt is that output of a run on an MI355X).

Out of scope here: the GroupNorm statistics left by the convolution epilogue (taken BEFORE the rounding of the convolution's output: another
contract, tests/test_unet_ops_gpu.py and tests/test_gemm_exact_gpu.py hold it), the split hi / lo output of the first stage
(mvi_groupnorm_silu_tok2tok_split: tests/test_split3_exact_gpu.py holds both halves elementwise and the plain split bit for bit;
tests/test_vae_encode_split_gpu.py the encoder walk built on it), and the fused GEGLU projections (tests/test_gemm_exact_gpu.py)."""
import pytest
import torch

import norm_exact_helpers as H
import svd_helpers as SH

pytestmark = pytest.mark.gpu

TAGS = ("f32", "bf16", "f16")
HALF = ("bf16", "f16")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


@pytest.fixture(autouse=True)
def _nothing_runs_on_a_faulted_device():
    """A device fault is sticky: the run ends with the test that met it instead of launching the rest of the module on that device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is launched: {e}", returncode=3)


def dev(v, dtype):
    return None if v is None else v.to(dtype).cuda()


def par(v):
    """An fp32 parameter (weight, bias, chan_bias, alpha) on the device."""
    return None if v is None else v.float().cuda()


def twice(fn):
    """fn() twice: the same bits both times."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        if torch.is_tensor(u):
            assert torch.equal(u, v), "a second call gave other bits"
    return a


def held(what, tag, got, ref, bnd, quarter, note=""):
    """Report, then assert the bound on every element."""
    g = got.detach().double().cpu()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    assert torch.isfinite(g).all(), what
    ratio = float(((g - ref).abs() / bnd).max())
    SH.report(f"{what} {tag}: worst |got - ref| / bound = {ratio:.3f}, cap <= ulp / 4 on {quarter:.3f} of the elements{note}")
    assert ratio <= 1.0, (what, tag, ratio, int(((g - ref).abs() > bnd).sum()), g.numel())
    return ratio


def exact(what, tag, got, want):
    """cap = 0: one right bit pattern."""
    bad = int((got.detach().cpu() != want).sum())
    SH.report(f"{what} {tag}: torch.equal, cap = 0 ({bad} of {want.numel()} elements differ)")
    assert bad == 0, (what, tag, bad)


def const_group(what, c, got_ncs):
    """The constant group: act(bias[c]) rounded once (see the module docstring for fp32 + SiLU)."""
    if c.dtype == torch.float32 and c.silu:
        return
    g = got_ncs.detach().cpu()[c.const]
    bad = int((g != c.want_const).sum())
    assert bad == 0, (what, c.tag, "constant group", bad, g.numel())


def gn_check(what, c, got_ncs, bound_name="bound"):
    bnd = getattr(c, bound_name)
    note = ""
    if c.outlier:
        free = float(((got_ncs.detach().double().cpu() - c.ref).abs() / c.bound).max())
        note = f"; first-token outlier of {c.outlier} scales (D = {c.D:.1f}): ratio to the cancellation-free bound {free:.4f}"
    held(what, c.tag, got_ncs, c.ref, bnd, c.quarter, note)
    const_group(what, c, got_ncs)


# ---- GroupNorm on planes and frames ---------------------------------------------------------------------------------------------------------

def run_planes(ops, c, sp, stack3_too):
    x = dev(c.x, c.dtype).reshape(c.N, c.C, *sp)
    w, b, cb = par(c.w), par(c.b), par(c.cb)
    shape = (c.N, c.C) + tuple(sp)
    if c.T == 1:
        y = twice(lambda: ops.group_norm_silu(x, c.G, w, b, c.eps, c.silu, chan_bias=cb))
        assert y.dtype == c.dtype and y.shape == x.shape
        gn_check(f"group_norm_silu {shape} G={c.G} cb={cb is not None} silu={c.silu}", c, y.reshape(c.N, c.C, c.S))
        return
    y = twice(lambda: ops.group_norm_silu_frames(x, c.T, c.G, w, b, c.eps, c.silu, chan_bias=cb))
    assert y.dtype == c.dtype and y.shape == x.shape
    gn_check(f"group_norm_silu_frames {shape} T={c.T} cb={cb is not None} silu={c.silu}", c, y.reshape(c.N, c.C, c.S))
    if stack3_too:
        y3 = twice(lambda: ops.group_norm_silu_frames(x, c.T, c.G, w, b, c.eps, c.silu, chan_bias=cb, stack3=True))
        assert y3.shape == (c.N, 3 * c.C) + tuple(sp)
        y3 = y3.reshape(c.N, 3, c.C, c.S)
        gn_check(f"group_norm_silu_frames stack3 {shape} T={c.T} cb={cb is not None} silu={c.silu}", c, y3[:, 1])
        # the two copies are the middle one moved by a frame, zeros at the ends of every video
        assert torch.equal(y3.reshape(c.N, 3 * c.C, c.S), H.stack3(y3[:, 1].contiguous(), c.T))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("with_cb,silu", H.GN_VARIANTS)
@pytest.mark.parametrize("N,C,sp,G,T", H.GN_PLANES)
def test_group_norm_planes_and_frames(ops, N, C, sp, G, T, with_cb, silu, tag):
    run_planes(ops, H.gn_case(tag, N, C, H.spatial_size(sp), G, T, with_cb, silu), sp, True)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("with_cb,silu", H.GN_VARIANTS)
def test_group_norm_first_multi_chunk_shape(ops, with_cb, silu, tag):
    """The smallest 64-channel image of 64-wide rows for which mvi_groupnorm_workspace_bytes grows: a group no longer fits one chunk of
    the two-launch kernels, every block merges two partials."""
    L = ops._lib.lib()
    N, C, (rows, W), G, T = H.MULTI_CHUNK
    one = L.mvi_groupnorm_workspace_bytes(N, C, W, G)
    h = next(h for h in range(1, 4 * rows) if L.mvi_groupnorm_workspace_bytes(N, C, h * W, G) > one)
    assert h == rows, "tests/norm_exact_helpers.py MULTI_CHUNK is not the first multi-chunk shape any more"
    run_planes(ops, H.gn_case(tag, N, C, rows * W, G, T, with_cb, silu), (rows, W), False)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("with_cb,silu", H.GN_VARIANTS)
def test_group_norm_cluster_form(ops, with_cb, silu, tag):
    """Four groups of 149 760 elements: up to 8 blocks per group exchange partial moments (gn_cluster_kernel) — a stale partner's moments
    are another unit's here. The counters are zero again after the calls and no block timed out."""
    N, C, sp, G, T = H.CLUSTER
    run_planes(ops, H.gn_case(tag, N, C, H.spatial_size(sp), G, T, with_cb, silu), sp, False)
    torch.cuda.synchronize()
    assert ops.groupnorm_cluster_timeouts() == 0
    assert all(int(buf.view(torch.int32).abs().sum()) == 0 for buf in ops._gn_sync.values())


# ---- GroupNorm with token-major output / input ----------------------------------------------------------------------------------------------

TOKENS_SHAPES = [(2, 64, (2, 4)), (2, 96, (8, 8)), (3, 320, (3, 8))]                # S and C multiples of the 16-byte vector


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("with_cb", [False, True])
@pytest.mark.parametrize("N,C,sp", TOKENS_SHAPES)
def test_group_norm_silu_tokens(ops, N, C, sp, with_cb, tag):
    S = H.spatial_size(sp)
    for outlier in (0, 8, 64):
        c = H.gn_case(tag, N, C, S, 32, 1, with_cb, True, outlier)
        x = dev(c.x, c.dtype).reshape(N, C, *sp)
        y = twice(lambda: ops.group_norm_silu_tokens(x, 32, par(c.w), par(c.b), c.eps, True, chan_bias=par(c.cb)))
        assert y.shape == (N, S, C) and y.dtype == c.dtype
        gn_check(f"group_norm_silu_tokens {(N, C) + tuple(sp)} cb={with_cb} outlier={outlier}", c, y.transpose(1, 2),
                 "bound_out" if outlier else "bound")


def tok_block_rows(ops, C, dtype):
    """Tokens per block of the token-major statistics pass at small sizes (one set of 8 rp rows), read from the host function that sizes
    its partials: the largest S that still has one chunk."""
    L, dt = ops._lib.lib(), ops._DT[dtype]
    one = L.mvi_groupnorm_tok2tok_workspace_bytes(1, C, 1, 32, dt)
    assert one != 0
    return next(s for s in range(1, 4096) if L.mvi_groupnorm_tok2tok_workspace_bytes(1, C, s + 1, 32, dt) != one)


def smallest_supported(ops, N, C, dtype):
    return next(s for s in range(1, 4096) if ops.group_norm_tok2tok_supported(N, C, s, 32, dtype))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("with_cb", [False, True])
@pytest.mark.parametrize("frames", [1, 2, 3])
@pytest.mark.parametrize("C", [64, 96, 320])
def test_group_norm_silu_tok2tok(ops, C, frames, with_cb, tag):
    """The smallest token count the kernel takes, and one that is no multiple of a block's rows (a full block and a ragged one per frame)."""
    dtype = H.DTYPES[tag]
    N = 2 * frames
    rows = tok_block_rows(ops, C, dtype)
    for S in (smallest_supported(ops, N, C, dtype), rows + 37):
        assert ops.group_norm_tok2tok_supported(N, C, S, 32, dtype)
        c = H.gn_case(tag, N, C, S, 32, frames, with_cb, True)
        t = dev(c.x.transpose(1, 2).contiguous(), dtype)
        y = twice(lambda: ops.group_norm_silu_tok2tok(t, 32, par(c.w), par(c.b), c.eps, True, chan_bias=par(c.cb), frames=frames))
        assert y.shape == t.shape and y.dtype == dtype
        gn_check(f"group_norm_silu_tok2tok {(N, S, C)} frames={frames} cb={with_cb}", c, y.transpose(1, 2))


@pytest.mark.parametrize("tag", TAGS)
def test_forward_with_statistics_is_the_inference_forward(ops, tag):
    """One C entry per family serves inference (stats NULL) and autograd (stats kept): y of *_forward_stats is torch.equal — no tolerance —
    to y of the matching inference wrapper on the scalar two-launch, vector, resident, multi-chunk and cluster forms, the stack3 and
    token-major outputs, and the token-major family at frames 1 and 2; the (mean, rstd) table has the same bits on a second call."""
    dtype = H.DTYPES[tag]
    for N, C, sp, G, T in H.GN_PLANES + [H.MULTI_CHUNK, H.CLUSTER]:
        c = H.gn_case(tag, N, C, H.spatial_size(sp), G, T, True, True)
        x, w, b, cb = dev(c.x, dtype).reshape(N, C, *sp), par(c.w), par(c.b), par(c.cb)
        for layout in (ops.GN_PLANES,) if T == 1 else (ops.GN_PLANES, ops.GN_STACK3):
            if T == 1:
                y = ops.group_norm_silu(x, G, w, b, c.eps, True, chan_bias=cb)
            else:
                y = ops.group_norm_silu_frames(x, T, G, w, b, c.eps, True, chan_bias=cb, stack3=layout == ops.GN_STACK3)
            ys, stats = twice(lambda: ops.group_norm_forward_stats(x, T, G, w, b, c.eps, True, chan_bias=cb, layout=layout))
            assert stats.shape == (N // T * G, 2) and stats.dtype == torch.float32
            assert torch.equal(ys, y), ("group_norm_forward_stats", (N, C) + tuple(sp), T, layout, tag)
    torch.cuda.synchronize()                                                         # the cluster shape came last
    assert ops.groupnorm_cluster_timeouts() == 0
    assert all(int(buf.view(torch.int32).abs().sum()) == 0 for buf in ops._gn_sync.values())
    for N, C, sp in TOKENS_SHAPES:
        c = H.gn_case(tag, N, C, H.spatial_size(sp), 32, 1, True, True, 0)
        x, w, b, cb = dev(c.x, dtype).reshape(N, C, *sp), par(c.w), par(c.b), par(c.cb)
        y = ops.group_norm_silu_tokens(x, 32, w, b, c.eps, True, chan_bias=cb)
        ys, stats = twice(lambda: ops.group_norm_forward_stats(x, 1, 32, w, b, c.eps, True, chan_bias=cb, layout=ops.GN_TOKENS))
        assert stats.shape == (N * 32, 2) and torch.equal(ys, y), ("group_norm_forward_stats, token-major output", (N, C) + tuple(sp), tag)
    for C, frames in ((64, 1), (64, 2), (96, 1), (96, 2), (320, 1), (320, 2)):
        N, S = 2 * frames, tok_block_rows(ops, C, dtype) + 37
        c = H.gn_case(tag, N, C, S, 32, frames, True, True)
        t, w, b, cb = dev(c.x.transpose(1, 2).contiguous(), dtype), par(c.w), par(c.b), par(c.cb)
        y = ops.group_norm_silu_tok2tok(t, 32, w, b, c.eps, True, chan_bias=cb, frames=frames)
        ys, stats = twice(lambda: ops.group_norm_tok2tok_forward_stats(t, 32, w, b, c.eps, True, chan_bias=cb, frames=frames))
        assert stats.shape == (N // frames * 32, 2) and torch.equal(ys, y), ("group_norm_tok2tok_forward_stats", (N, S, C), frames, tag)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("D", [8, 64])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("C", [64, 96, 320])
def test_group_norm_silu_tok2tok_outlier_first_token(ops, C, frames, D, tag):
    """The first token of every block of the statistics pass is moved by D scales: the shifted sums of gt_stats_kernel cancel from
    rows D^2 sigma^2 to rows sigma^2. Held to the shifted algebra's own allowance (norm_exact_helpers.outlier_allowance); the ratio to the
    cancellation-free bound is reported."""
    dtype = H.DTYPES[tag]
    N = 2 * frames
    rows = tok_block_rows(ops, C, dtype)
    S = 2 * rows + 37
    c = H.gn_case(tag, N, C, S, 32, frames, True, True, D, rows)
    t = dev(c.x.transpose(1, 2).contiguous(), dtype)
    y = twice(lambda: ops.group_norm_silu_tok2tok(t, 32, par(c.w), par(c.b), c.eps, True, chan_bias=par(c.cb), frames=frames))
    gn_check(f"group_norm_silu_tok2tok {(N, S, C)} frames={frames} block={rows}", c, y.transpose(1, 2), "bound_out")


@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("outlier", [0, 8, 64])
@pytest.mark.parametrize("mode", ["add", "blend", "concat"])
@pytest.mark.parametrize("C", [64, 96, 320])
def test_group_norm_silu_tok2tok_on_rows_fused_partials(ops, C, mode, outlier, tag):
    """rows_fused(..., groups=32) leaves the (count, mean, M2) partials of the NEXT GroupNorm, taken on its ROUNDED output (gt_fused_kernel);
    group_norm_silu_tok2tok(partials=...) then runs merge + apply only. The pointwise result is held to its own bound (torch.equal for the
    concatenation), the norm to the fp64 GroupNorm of what the pointwise pass stored. blend: statistics over videos of two frames."""
    dtype = H.DTYPES[tag]
    N, frames = 4, (2 if mode == "blend" else 1)
    rows = tok_block_rows(ops, C, dtype)
    S = rows + 37
    assert ops.rows_gnstats_supported(N, C, S, 32, dtype)
    c = H.gn_case(tag, N, C, S, 32, frames, False, True, outlier, rows, ident=1)
    g = H.gen(41, C, outlier, ("add", "blend", "concat").index(mode), dtype == torch.float16)
    x = c.x.transpose(1, 2).contiguous()                                             # [N, S, C] with distinct statistics per unit
    what = f"rows_fused {mode} groups=32 {(N, S, C)} outlier={outlier}"
    if mode == "add":
        b = H.q(0.25 * torch.randn(N, S, C, generator=g, dtype=torch.float64), dtype)
        bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
        pc = H.point_case(dtype, x + bias + b, H.pointwise_cap(2, x.abs() + bias.abs() + b.abs()))
        out, part = twice(lambda: ops.rows_fused(dev(x, dtype), dev(b, dtype), bias=par(bias), groups=32))
    elif mode == "blend":
        a = H.q(0.25 * torch.randn(N, S, C, generator=g, dtype=torch.float64), dtype)
        bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
        alpha = H.f32(torch.tensor(H.ALPHAS, dtype=torch.float64))
        pc = H.ref_blend(dtype, x, a, bias, alpha, lambda v: H.samp(v, 3))
        out, part = twice(lambda: ops.rows_fused(dev(a, dtype), bias=par(bias), base=dev(x, dtype), alpha=par(alpha), groups=32))
    else:
        C1 = C // 2
        out, part = twice(lambda: ops.rows_fused(dev(x[..., :C1].contiguous(), dtype), dev(x[..., C1:].contiguous(), dtype), groups=32, concat=True))
    assert part is not None and out.shape == (N, S, C)
    if mode == "concat":
        exact(what, tag, out, x.to(dtype))
    else:
        held(what, tag, out, pc.ref, pc.bound, pc.quarter)
    w, b_ = par(c.w), par(c.b)
    y = twice(lambda: ops.group_norm_silu_tok2tok(out, 32, w, b_, c.eps, True, frames=frames, partials=part))
    stored = out.double().cpu()
    starts = list(range(0, S, rows))
    x5 = stored.transpose(1, 2).reshape(N // frames, frames, 32, C // 32, S)
    A = H.outlier_allowance(x5, (1, 3, 4), starts) if outlier else 1.0
    ref, cap = H.norm_cap(x5, (1, 3, 4), c.w.reshape(1, 1, 32, -1, 1), c.b.reshape(1, 1, 32, -1, 1), c.eps, True, A)
    ref, cap = ref.reshape(N, C, S).transpose(1, 2), cap.reshape(N, C, S).transpose(1, 2)
    note = ""
    if outlier:
        free = H.gn_on(stored, tag, 32, frames, c.w, c.b, None, True, c.eps)
        note = f"; ratio to the cancellation-free bound {float(((y.double().cpu() - free[0]).abs() / free[2]).max()):.4f}"
    held(f"group_norm_silu_tok2tok on partials of {what}", tag, y, ref, H.bound(ref, cap, dtype), H.quarter_share(ref, cap, dtype), note)
    if mode == "concat":
        const_group(what, c, y.transpose(1, 2))
    # and the norm with its own statistics pass agrees to the same bound
    y2 = ops.group_norm_silu_tok2tok(out, 32, w, b_, c.eps, True, frames=frames)
    assert float(((y2.double().cpu() - ref).abs() / H.bound(ref, cap, dtype)).max()) <= 1.0


# ---- LayerNorm rows, softmax rows -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", H.LN_MODES)
@pytest.mark.parametrize("R", H.LN_ROWS)
@pytest.mark.parametrize("C", H.LN_WIDTHS)
def test_add_layer_norm(ops, C, R, mode, tag):
    dtype = H.DTYPES[tag]
    if not ops.layernorm_supported(C, dtype):
        pytest.skip(f"add_layer_norm does not take C = {C} in {tag}")
    c = H.ln_case(tag, R, C, mode)
    w, b = par(c.w), par(c.b)
    y, s, s_pre = twice(lambda: ops.add_layer_norm(dev(c.x, dtype), w, b, c.eps, h=dev(c.h, dtype), row=dev(c.row, dtype), ret_pre=mode == "h_row_pre"))
    what = f"add_layer_norm [{R}, {C}] {mode}"
    if mode == "plain":
        assert s is None
    else:
        exact(what + " s", tag, s, c.s.to(dtype))
    if mode == "h_row_pre":
        exact(what + " s_pre", tag, s_pre, c.s_pre.to(dtype))
    held(what + " y", tag, y, c.ref, c.bound, c.quarter)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("cols", H.SOFTMAX_COLS)
def test_softmax_rows(ops, cols, tag):
    c = H.softmax_case(tag, cols)
    y = twice(lambda: ops.softmax_rows_(dev(c.x, c.dtype).clone(), H.SOFTMAX_SCALE))
    held(f"softmax_rows_ [7, {cols}] scale={H.SOFTMAX_SCALE}", tag, y, c.ref, c.bound, c.quarter)
    if tag != "f32":
        assert torch.equal(y[6].cpu(), torch.full((cols,), 1.0 / cols, dtype=torch.float64).to(c.dtype))   # equal entries: 1 / cols rounded once


# ---- pointwise tails ------------------------------------------------------------------------------------------------------------------------

PLANES = [(4, 64, (6, 8)), (4, 24, (5, 9))]                                          # 16-byte vectors; S odd: the scalar path
TOKENS = [(4, 64, 64), (4, 72, 72)]                                                  # (N, C, S): whole 64 x 64 tiles; ragged tiles both ways
ROWS = [(4, 48, 64), (4, 37, 72)]                                                    # (N, S, C): rows x width, an odd row count


def alphas(n=4):
    return H.f32(torch.tensor([H.ALPHAS[i % 4] for i in range(n)], dtype=torch.float64))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N,C,sp", PLANES)
def test_bias_residual_add_blend_silu_concat(ops, N, C, sp, tag):
    dtype = H.DTYPES[tag]
    g = H.gen(42, N, C, sp[1], dtype == torch.float16)
    S = H.spatial_size(sp)
    shape = (N, C) + tuple(sp)
    h, x = H.point_data(g, dtype, *shape), H.point_data(g, dtype, *shape)
    bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
    hd, xd, bd = dev(h, dtype), dev(x, dtype), par(bias)
    pc = H.ref_bias_residual_add(dtype, h, bias, x)
    held(f"bias_residual_add {shape}", tag, twice(lambda: ops.bias_residual_add(hd, bd, xd)), pc.ref, pc.bound, pc.quarter)
    pc = H.ref_bias_residual_add(dtype, h, bias, None)
    held(f"bias_residual_add {shape} no x", tag, twice(lambda: ops.bias_residual_add(hd, bd, None)), pc.ref, pc.bound, pc.quarter)
    hg, xg, cg = (H.grid_data(g, dtype, *shape) for _ in range(3))
    exact(f"bias_residual_add {shape} no bias", tag, twice(lambda: ops.bias_residual_add(dev(hg, dtype), None, dev(xg, dtype))), (hg + xg).to(dtype))
    al = alphas(N)
    pc = H.ref_blend(dtype, x, h, H.chan(bias, h.dim()), al, lambda v: H.samp(v, h.dim()))
    held(f"bias_residual_blend {shape}", tag, twice(lambda: ops.bias_residual_blend(hd, bd, xd, par(al))), pc.ref, pc.bound, pc.quarter)
    pc = H.ref_bias_silu(dtype, h, bias)
    held(f"bias_silu {shape}", tag, twice(lambda: ops.bias_silu(hd.clone(), bd)), pc.ref, pc.bound, pc.quarter)
    C2 = C // 2 + 4
    sg, cg2 = H.grid_data(g, dtype, N, C2, *sp), H.grid_data(g, dtype, N, C2, *sp)
    want = torch.cat([hg, sg + cg2], 1).to(dtype)
    exact(f"concat_add {shape} + {C2}", tag, twice(lambda: ops.concat_add(dev(hg, dtype), dev(sg, dtype), dev(cg2, dtype))), want)
    exact(f"concat_add {shape} + {C2} no ctrl", tag, twice(lambda: ops.concat_add(dev(hg, dtype), dev(sg, dtype), None)), torch.cat([hg, sg], 1).to(dtype))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N,S,C", ROWS)
def test_add_lerp_and_rows_fused(ops, N, S, C, tag):
    dtype = H.DTYPES[tag]
    g = H.gen(43, N, S, C, dtype == torch.float16)
    x, h, base = (H.point_data(g, dtype, N, S, C) for _ in range(3))
    al = alphas(N)
    for hh in (h, None):
        pc = H.ref_add_lerp(dtype, x, hh, base, H.samp(al, 3))
        held(f"add_lerp {(N, S, C)} h={hh is not None}", tag, twice(lambda: ops.add_lerp(dev(x, dtype), dev(hh, dtype), dev(base, dtype), par(al))),
             pc.ref, pc.bound, pc.quarter)
    bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
    pc = H.point_case(dtype, x + bias + h, H.pointwise_cap(2, x.abs() + bias.abs() + h.abs()))
    held(f"rows_fused add + bias {(N, S, C)}", tag, twice(lambda: ops.rows_fused(dev(x, dtype), dev(h, dtype), bias=par(bias)))[0], pc.ref, pc.bound, pc.quarter)
    ag, bg, cg = (H.grid_data(g, dtype, N, S, C) for _ in range(3))
    exact(f"rows_fused add {(N, S, C)}", tag, twice(lambda: ops.rows_fused(dev(ag, dtype), dev(bg, dtype)))[0], (ag + bg).to(dtype))
    pc = H.ref_blend(dtype, base, x, bias, al, lambda v: H.samp(v, 3))
    held(f"rows_fused blend {(N, S, C)}", tag, twice(lambda: ops.rows_fused(dev(x, dtype), bias=par(bias), base=dev(base, dtype), alpha=par(al)))[0],
         pc.ref, pc.bound, pc.quarter)
    C1 = 24
    a1 = H.grid_data(g, dtype, N, S, C1)
    exact(f"rows_fused concat {(N, S, C1)} | {(N, S, C)}", tag,
          twice(lambda: ops.rows_fused(dev(a1, dtype), dev(bg, dtype), base=dev(cg, dtype), concat=True))[0], torch.cat([a1, bg + cg], 2).to(dtype))
    if tag == "f32":
        a, b = x.reshape(N * S, C), h.reshape(N * S, C)
        for alpha in (0.3, 1.0):
            al32 = float(torch.tensor(alpha, dtype=torch.float32))
            pc = H.point_case(dtype, a + al32 * (b + bias), H.pointwise_cap(3, a.abs() + abs(al32) * (b.abs() + bias.abs())))
            held(f"rows_axpb {(N * S, C)} alpha={alpha}", tag, twice(lambda: ops.rows_axpb(dev(a, dtype), dev(b, dtype).clone(), par(bias), alpha)),
                 pc.ref, pc.bound, pc.quarter)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N,C,S", TOKENS)
def test_token_plane_tails(ops, N, C, S, tag):
    dtype = H.DTYPES[tag]
    g = H.gen(44, N, C, S, dtype == torch.float16)
    tok, base = H.point_data(g, dtype, N, S, C), H.point_data(g, dtype, N, S, C)
    x = H.point_data(g, dtype, N, C, S)
    bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
    sp = (S // 8, 8)
    tp = tok.transpose(1, 2)                                                         # tokens seen as planes [N, C, S]
    pc = H.point_case(dtype, tp + bias[None, :, None] + x, H.pointwise_cap(2, tp.abs() + bias.abs()[None, :, None] + x.abs()))
    y = twice(lambda: ops.tokens_to_planes_add(dev(tok, dtype), dev(x, dtype).reshape(N, C, *sp), bias=par(bias)))
    held(f"tokens_to_planes_add + bias {(N, S, C)}", tag, y.reshape(N, C, S), pc.ref, pc.bound, pc.quarter)
    tg, xg = H.grid_data(g, dtype, N, S, C), H.grid_data(g, dtype, N, C, S)
    y = twice(lambda: ops.tokens_to_planes_add(dev(tg, dtype), dev(xg, dtype).reshape(N, C, *sp)))
    exact(f"tokens_to_planes_add {(N, S, C)}", tag, y.reshape(N, C, S), (tg.transpose(1, 2) + xg).to(dtype))
    pc = H.point_case(dtype, (x + tp + bias[None, :, None]).transpose(1, 2), H.pointwise_cap(2, (x.abs() + tp.abs() + bias.abs()[None, :, None]).transpose(1, 2)))
    y = twice(lambda: ops.planes_add_to_tokens(dev(x, dtype).reshape(N, C, *sp), dev(tok, dtype), bias=par(bias)))
    held(f"planes_add_to_tokens + bias {(N, C, S)}", tag, y, pc.ref, pc.bound, pc.quarter)
    y = twice(lambda: ops.planes_add_to_tokens(dev(xg, dtype).reshape(N, C, *sp), dev(tg, dtype)))
    exact(f"planes_add_to_tokens {(N, C, S)}", tag, y, (xg.transpose(1, 2) + tg).to(dtype))
    al = alphas(N)
    pc = H.ref_blend(dtype, base.transpose(1, 2), tp, bias[None, :, None], al, lambda v: H.samp(v, 3))
    y = twice(lambda: ops.tokens_blend_to_planes(dev(tok, dtype), dev(base, dtype), par(bias), par(al), sp))
    held(f"tokens_blend_to_planes {(N, S, C)}", tag, y.reshape(N, C, S), pc.ref, pc.bound, pc.quarter)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("rows,inner", [(5, 64), (3, 8), (37, 200)])
def test_geglu(ops, rows, inner, tag):
    c = H.geglu_case(tag, rows, inner)
    y = twice(lambda: ops.geglu(dev(c.h, c.dtype)))
    held(f"geglu [{rows}, 2 x {inner}]", tag, y, c.ref, c.bound, c.quarter)

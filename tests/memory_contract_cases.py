"""The case table of tests/test_memory_contract_gpu.py: one entry per (wrapper of multiview_inpaint_amd/svd/hip_ops.py, shape, form), with
the C entries it launches (tests/test_memory_contract_cpu.py holds the table to every launching entry of hip_ops.py). Importing this
module needs no GPU: a case's `build(ops, tag)` runs on the device and returns a Built — the call, its inputs, the check of the unpatched
result against the op's fp64 or exact reference (data, reference and bar are those of the op's own suite: the *_helpers modules and the
tables of the tests named per family), the inputs an in-place op declares as outputs, whether a GroupNorm ran, and the outputs that a
library call made from a guarded intermediate.

Shapes: the smallest each path can go wrong at, from the tables those suites curate — the smallest supported one, one ragged in every
tiled dimension, and for workspace users one on each side of the split policy (asserted through the *_workspace_bytes functions)."""
import collections
import types

import torch
import torch.nn.functional as F

import attention_bwd_helpers as AB
import block_tails_bwd_helpers as BT
import exact_attention_helpers as EA
import exact_gemm_helpers as E
import geglu_bwd_helpers as GG
import norm_bwd_exact_helpers as NB
import norm_exact_helpers as H
import split3_exact_helpers as S3
import stem_bwd_helpers as SB

DEV = "cuda"
ALL = ("f32", "bf16", "f16")
HALF = ("bf16", "f16")
DTYPES = H.DTYPES

Case = collections.namedtuple("Case", "id entries tags build")
Built = collections.namedtuple("Built", "call inputs ref inplace gn foreign", defaults=((), False, ()))
CASES = []


def case(cid, entries, tags=HALF):
    entries = (entries,) if isinstance(entries, str) else tuple(entries)

    def reg(build):
        assert cid not in {c.id for c in CASES}, cid
        CASES.append(Case(cid, entries, tags, build))
        return build
    return reg


def _id(s):
    return "x".join(str(v) for v in s).replace("(", "").replace(")", "").replace(", ", "x")


def D(t, dtype):
    return None if t is None else t.to(dtype).to(DEV)


def P(t):
    """An fp32 parameter (weight, bias, chan_bias, alpha) on the device."""
    return None if t is None else t.float().to(DEV)


def exact_dev(t, dtype):
    """fp64 holding numbers of `dtype` -> the device tensor (exact)."""
    if t is None:
        return None
    d = t.to(dtype)
    assert torch.equal(d.double(), t)
    return d.to(DEV)


def held(what, got, ref, bnd):
    g = got.detach().double().cpu()
    assert g.shape == ref.shape and torch.isfinite(g).all(), (what, g.shape, ref.shape)
    ratio = float(((g - ref).abs() / bnd).max())
    assert ratio <= 1.0, (what, ratio)


def equal(what, got, want):
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (got.double() != want.double()) | torch.isnan(got.double())
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel())


def capped(what, got, ref, cap):
    d = (got.detach().double().cpu() - ref).abs()
    assert d.shape == cap.shape and bool((d <= cap).all()), (what, float((d / cap.clamp_min(1e-300)).max()))


def _lib():
    from multiview_inpaint_amd import _lib
    return _lib.lib()


# ---- GroupNorm forward on planes, frames, stack3, token output, with statistics (tests/test_norm_elementwise_gpu.py) ---------------------

def _gn_forward(form, N, C, sp, G, T):
    def build(ops, tag):
        S = H.spatial_size(sp)
        c = H.gn_case(tag, N, C, S, G, T, True, True)
        ins = [D(c.x, c.dtype).reshape(N, C, *sp), P(c.w), P(c.b), P(c.cb)]
        lay = {"planes_stats": ops.GN_PLANES, "stack3_stats": ops.GN_STACK3, "tokens_stats": ops.GN_TOKENS}.get(form)
        call = {
            "planes": lambda x, w, b, cb: ops.group_norm_silu(x, G, w, b, c.eps, True, chan_bias=cb),
            "frames": lambda x, w, b, cb: ops.group_norm_silu_frames(x, T, G, w, b, c.eps, True, chan_bias=cb),
            "stack3": lambda x, w, b, cb: ops.group_norm_silu_frames(x, T, G, w, b, c.eps, True, chan_bias=cb, stack3=True),
            "tokens": lambda x, w, b, cb: ops.group_norm_silu_tokens(x, G, w, b, c.eps, True, chan_bias=cb),
        }.get(form, lambda x, w, b, cb: ops.group_norm_forward_stats(x, T, G, w, b, c.eps, True, chan_bias=cb, layout=lay))

        def ref(outs):
            y = outs[0]
            if form.startswith("stack3"):
                y3 = y.reshape(N, 3, C, S)
                assert torch.equal(y3.reshape(N, 3 * C, S), H.stack3(y3[:, 1].contiguous(), T))
                y = y3[:, 1]
            elif form.startswith("tokens"):
                y = y.transpose(1, 2)
            held(form, y.reshape(N, C, S), c.ref, c.bound)
            if len(outs) == 2:
                assert outs[1].shape == (N // T * G, 2) and outs[1].dtype == torch.float32
        return Built(call, ins, ref, gn=True)
    return build


TOKENS_SHAPES = [(2, 64, (2, 4)), (2, 96, (8, 8)), (3, 320, (3, 8))]                # tests/test_norm_elementwise_gpu.py
for _form, _shapes in (("planes", [H.GN_PLANES[2], H.MULTI_CHUNK, H.CLUSTER]), ("frames", [H.GN_PLANES[3], H.GN_PLANES[4]]),
                       ("stack3", [H.GN_PLANES[3], H.GN_PLANES[4]]), ("tokens", [(n, c, sp, 32, 1) for n, c, sp in (TOKENS_SHAPES[0], TOKENS_SHAPES[2])]),
                       ("planes_stats", [H.GN_PLANES[0]]), ("stack3_stats", [H.GN_PLANES[3]]), ("tokens_stats", [TOKENS_SHAPES[1] + (32, 1)])):
    for _s in _shapes:
        case(f"group_norm_{_form}_{_id(_s)}", "mvi_groupnorm_forward", ALL)(_gn_forward(_form, *_s))


# ---- token-major GroupNorm, plain and with statistics -------------------------------------------------------------------------------------

def _tok2tok(N, C, S, G, frames, stats):
    def build(ops, tag):
        c = H.gn_case(tag, N, C, S, G, frames, True, True)
        assert ops.group_norm_tok2tok_supported(N, C, S, G, c.dtype)
        ins = [D(c.x.transpose(1, 2).contiguous(), c.dtype), P(c.w), P(c.b), P(c.cb)]
        if stats:
            call = lambda t, w, b, cb: ops.group_norm_tok2tok_forward_stats(t, G, w, b, c.eps, True, chan_bias=cb, frames=frames)
        else:
            call = lambda t, w, b, cb: ops.group_norm_silu_tok2tok(t, G, w, b, c.eps, True, chan_bias=cb, frames=frames)
        return Built(call, ins, lambda outs: held("tok2tok", outs[0].transpose(1, 2), c.ref, c.bound), gn=True)
    return build


for _s in NB.TOK2TOK_SHAPES[:3]:
    case(f"group_norm_tok2tok_{_id(_s)}", "mvi_groupnorm_tok2tok_forward", ALL)(_tok2tok(*_s, False))
case(f"group_norm_tok2tok_stats_{_id(NB.TOK2TOK_SHAPES[1])}", "mvi_groupnorm_tok2tok_forward", ALL)(_tok2tok(*NB.TOK2TOK_SHAPES[1], True))


# ---- both GroupNorm backwards, every combination of outputs (tests/test_norm_bwd_elementwise_gpu.py) -------------------------------------

NEED = [(dx, dp, dcb) for dx in (True, False) for dp in (True, False) for dcb in (True, False)][:-1]


def _gn_check(c, outs, tokens):
    dx, dw, db, dcb = outs
    for k, t in (("dx", dx), ("dweight", dw), ("dbias", db), ("dchan_bias", dcb)):
        if t is not None:
            held(k, t.transpose(1, 2) if (k == "dx" and tokens) else t, c.ref[k], c.bound[k])
    if dw is not None:
        assert int((dw.detach().cpu()[c.const_c] != 0).sum()) == 0


def _gn_backward(N, C, S, G, T, layout, need):
    def build(ops, tag):
        c = NB.gn_bwd_case(tag, N, C, S, G, T, True, True, layout, NB.CONST_VALUES[1])
        lay = {NB.PLANES: ops.GN_PLANES, NB.STACK3: ops.GN_STACK3, NB.TOKENS: ops.GN_TOKENS}[layout]
        assert ops.group_norm_backward_supported(N, C, S, G, T, c.dtype, lay)
        x, w, b, cb = D(c.x, c.dtype), P(c.w), P(c.b), P(c.cb)
        dy = D(c.dy.transpose(1, 2).contiguous() if layout == NB.TOKENS else c.dy, c.dtype)
        stats = ops.group_norm_forward_stats(x, T, G, w, b, c.eps, True, chan_bias=cb, layout=lay)[1]
        call = lambda dy, x, stats, w, b, cb: ops.group_norm_backward(dy, x, stats, T, G, w, b, True, chan_bias=cb, layout=lay, need_dx=need[0],
                                                                      need_dparams=need[1], need_dchan_bias=need[2])
        return Built(call, [dy, x, stats, w, b, cb], lambda outs: _gn_check(c, outs, False), gn=True)
    return build


def _tok2tok_backward(N, C, S, G, frames, need):
    def build(ops, tag):
        c = NB.gn_bwd_case(tag, N, C, S, G, frames, True, True, NB.TOKENS, NB.CONST_VALUES[1])
        t, dy = D(c.x.transpose(1, 2).contiguous(), c.dtype), D(c.dy.transpose(1, 2).contiguous(), c.dtype)
        w, b, cb = P(c.w), P(c.b), P(c.cb)
        stats = ops.group_norm_tok2tok_forward_stats(t, G, w, b, c.eps, True, chan_bias=cb, frames=frames)[1]
        call = lambda dy, t, stats, w, b, cb: ops.group_norm_tok2tok_backward(dy, t, stats, G, w, b, True, chan_bias=cb, frames=frames, need_dx=need[0],
                                                                              need_dparams=need[1], need_dchan_bias=need[2])
        return Built(call, [dy, t, stats, w, b, cb], lambda outs: _gn_check(c, outs, True), gn=True)
    return build


_need_id = lambda n: "".join("xpc"[i] for i in range(3) if n[i])
for _n in NEED:
    case(f"group_norm_backward_{_id(NB.GN_BWD_SHAPES[1][:5])}_{_need_id(_n)}", "mvi_groupnorm_backward", ALL)(_gn_backward(*NB.GN_BWD_SHAPES[1], _n))
    case(f"group_norm_tok2tok_backward_{_id(NB.TOK2TOK_SHAPES[1])}_{_need_id(_n)}", "mvi_groupnorm_tok2tok_backward", ALL)(
        _tok2tok_backward(*NB.TOK2TOK_SHAPES[1], _n))
for _s in (NB.GN_BWD_SHAPES[6], NB.GN_BWD_SHAPES[10]):
    case(f"group_norm_backward_{_s[5]}_{_id(_s[:5])}", "mvi_groupnorm_backward", ALL)(_gn_backward(*_s, NEED[0]))
for _s in (NB.TOK2TOK_SHAPES[0], NB.TOK2TOK_SHAPES[2]):
    case(f"group_norm_tok2tok_backward_{_id(_s)}", "mvi_groupnorm_tok2tok_backward", ALL)(_tok2tok_backward(*_s, NEED[0]))


# ---- add + LayerNorm, forward (four modes) and backward (every gradient-presence mode) ---------------------------------------------------

def _add_layer_norm(R, C, mode):
    def build(ops, tag):
        c = H.ln_case(tag, R, C, mode)
        dt = c.dtype if hasattr(c, "dtype") else DTYPES[tag]
        assert ops.layernorm_supported(C, dt)
        ins = [D(c.x, dt), D(c.h, dt), D(c.row, dt), P(c.w), P(c.b)]
        call = lambda x, h, row, w, b: ops.add_layer_norm(x, w, b, c.eps, h=h, row=row, ret_pre=mode == "h_row_pre")

        def ref(outs):
            y, s, s_pre = outs
            if mode == "plain":
                assert s is None
            else:
                equal("s", s, c.s.to(dt))
            if mode == "h_row_pre":
                equal("s_pre", s_pre, c.s_pre.to(dt))
            held("y", y, c.ref, c.bound)
        return Built(call, ins, ref)
    return build


for _mode in H.LN_MODES:
    for _R, _C in ((H.LN_ROWS[0], H.LN_WIDTHS[0]), (H.LN_ROWS[1], H.LN_WIDTHS[2]), (H.LN_ROWS[1], H.LN_WIDTHS[4])):
        case(f"add_layer_norm_{_mode}_{_R}x{_C}", "mvi_add_layernorm", ALL)(_add_layer_norm(_R, _C, _mode))


def _add_layer_norm_backward(R, C, runs, mode):
    def build(ops, tag):
        c = NB.ln_bwd_case(tag, R, C, runs, mode)
        assert ops.add_layer_norm_backward_supported(C, c.dtype)
        ins = [D(c.s, c.dtype), P(c.w), D(c.gy, c.dtype), D(c.gs, c.dtype), D(c.gsp, c.dtype)]
        call = lambda s, w, gy, gs, gsp: ops.add_layer_norm_backward(s, w, c.eps, gy=gy, gs=gs, gs_pre=gsp, row_groups=runs or None)

        def ref(outs):
            got = dict(dx=outs[0], dweight=outs[1], dbias=outs[2])
            if runs:
                got["drow"] = outs[3]
            for k in c.ref:
                held(k, got[k], c.ref[k], c.bound[k])
        return Built(call, ins, ref)
    return build


for _m in NB.LN_BWD_MODES:
    case(f"add_layer_norm_backward_{_id(NB.LN_BWD_MODE_SHAPE)}_{''.join(str(int(v)) for v in _m)}", "mvi_add_layernorm_backward", ALL)(
        _add_layer_norm_backward(*NB.LN_BWD_MODE_SHAPE, _m))
for _s in NB.LN_BWD_SHAPES[1:3]:
    case(f"add_layer_norm_backward_{_id(_s)}", "mvi_add_layernorm_backward", ALL)(_add_layer_norm_backward(*_s, NB.LN_BWD_MODES[0]))


# ---- row GEMMs on integers (tests/test_gemm_exact_gpu.py) -----------------------------------------------------------------------------------

def _linear(which, rows, K, N, with_bias, ident=0):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        c = E.linear_case("parity", tag, rows, K, N, with_bias, ident)
        fn = {"k320": ops.linear_k320, "n320": ops.linear_n320, "dgrad": ops.linear_dgrad}[which]
        if which == "dgrad":
            return Built(lambda x, w: fn(x, w), [exact_dev(c.x, dt), exact_dev(c.w, dt)], lambda outs: equal(which, outs[0], c.want))
        return Built(lambda x, w, b: fn(x, w, b), [exact_dev(c.x, dt), exact_dev(c.w, dt), P(c.b)], lambda outs: equal(which, outs[0], c.want))
    return build


for _r, _N, _b in ((1, 128, True), (255, 192, False), (257, 960, True)):
    case(f"linear_k320_{_r}x320x{_N}", "mvi_linear_k320")(_linear("k320", _r, 320, _N, _b))
for _r, _K, _N, _b in ((1, 128, 320, True), (255, 192, 640, False), (257, 704, 320, True)):
    case(f"linear_n320_{_r}x{_K}x{_N}", "mvi_linear_n320")(_linear("n320", _r, _K, _N, _b))
for (_r, _K, _N), _e in zip(E.LINEAR_DGRAD, ("mvi_linear_k320", "mvi_linear_n320")):
    case(f"linear_dgrad_{_r}x{_K}x{_N}", _e)(_linear("dgrad", _r, _N, _K, False, 1))


def _ff_geglu(which, rows, K, inner):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        c = E.geglu_case(tag, rows, K, inner)
        fn = ops.ff_geglu if which == "k320" else ops.ff_geglu_n320

        def ref(outs):
            y = outs[0].detach().cpu()
            neg = y[c.neg].double().abs()
            assert neg.numel() and neg.max().item() <= 1e-20
            equal(which, torch.where(c.neg, torch.zeros_like(y), y), c.want)
        return Built(lambda x, w, b: fn(x, w, b), [exact_dev(c.x, dt), exact_dev(c.w, dt), P(c.b)], ref)
    return build


for _r, _i in ((33, 64), (255, 96), (257, 64)):
    case(f"ff_geglu_{_r}x320x{_i}", "mvi_ff_geglu")(_ff_geglu("k320", _r, 320, _i))
for _r, _K, _i in ((33, 128, 160), (255, 128, 480), (257, 640, 160)):
    case(f"ff_geglu_n320_{_r}x{_K}x{_i}", "mvi_ff_geglu_n320")(_ff_geglu("n320", _r, _K, _i))


def _linear_ln(rows, K, G, with_resid, ret_pre):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        c = E.linear_ln_case(tag, rows, K, G, with_resid, ret_pre)
        ins = [exact_dev(c.x, dt), exact_dev(c.w, dt), P(c.b), P(c.lw), P(c.lb), exact_dev(c.resid, dt), exact_dev(c.row, dt)]
        call = lambda x, w, b, lw, lb, resid, row: ops.linear_n320_add_layer_norm(x, w, b, lw, lb, 1e-5, resid=resid, row=row, ret_pre=ret_pre)

        def ref(outs):
            y, s, s_pre = outs
            equal("s", s, c.want_s)
            if ret_pre:
                equal("s_pre", s_pre, c.want_s_pre)
            else:
                assert s_pre is None
            err = (y.double().cpu() - c.y_ref).abs().max().item()
            assert err <= {"bf16": 1.0 / 128, "f16": 1.0 / 1024}[tag] * max(1.0, c.y_ref.abs().max().item()), err
        return Built(call, ins, ref)
    return build


for _s in (E.LINEAR_LN[0], E.LINEAR_LN[1], E.LINEAR_LN[3]):
    case(f"linear_n320_add_layer_norm_{_id(_s)}", "mvi_linear_n320_add_layernorm")(_linear_ln(*_s))


# ---- implicit-GEMM convolutions on integers ---------------------------------------------------------------------------------------------------

def _conv3x3(shape, stride, up2, split, splits):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        N, Hh, W, C, Co = shape
        c = E.conv3x3_case("parity", tag, *shape, stride, up2)
        if split and not up2:
            assert (int(_lib().mvi_conv3x3_n320_workspace_bytes(N, Hh, W, C, Co, stride)) > 0) == splits, shape
        wt = ops.conv3x3_n320_weight(exact_dev(c.w, dt))
        call = lambda tok, wt, b: ops.conv3x3_n320(tok, wt, b, Hh, W, stride=stride, split=split, up2=up2)
        Ho, Wo = c.ref.shape[2], c.ref.shape[3]
        return Built(call, [exact_dev(E.tokens(c.x), dt), wt, P(c.b)], lambda outs: equal("conv3x3", E.planes(outs[0], Ho, Wo), c.want))
    return build


for _s, _sp, _splits in ((E.CONV3X3[0], True, False), (E.CONV3X3[3], True, False), (E.CONV3X3[4], True, True), (E.CONV3X3[4], False, False)):
    case(f"conv3x3_n320_{_id(_s)}_split{int(_sp)}", "mvi_conv3x3_n320")(_conv3x3(_s, 1, False, _sp, _splits))
for _s, _sp, _splits in ((E.CONV3X3_S2[0], True, False), (E.CONV3X3_S2[1], True, True), (E.CONV3X3_S2[1], False, False)):
    case(f"conv3x3_n320_s2_{_id(_s)}_split{int(_sp)}", "mvi_conv3x3_n320")(_conv3x3(_s, 2, False, _sp, _splits))
for _s in E.CONV3X3_UP2:
    case(f"conv3x3_up2_n320_{_id(_s)}", "mvi_conv3x3_up2_n320")(_conv3x3(_s, 1, True, True, False))


def _conv3t(shape, split):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        B, T, S, C, Co = shape
        c = E.conv3t_case("parity", tag, *shape)
        assert (int(_lib().mvi_conv3t_n320_workspace_bytes(B, T, S, C, Co)) > 0) == (C >= 384), shape
        wt = ops.conv3t_n320_weight(exact_dev(c.w, dt))
        call = lambda tok, wt, b: ops.conv3t_n320(tok, wt, b, T, split=split)
        return Built(call, [exact_dev(c.tok, dt), wt, P(c.b)], lambda outs: equal("conv3t", outs[0], c.want))
    return build


for _s, _sp in ((E.CONV3T[0], True), (E.CONV3T[1], True), (E.CONV3T[2], True), (E.CONV3T[2], False)):
    case(f"conv3t_n320_{_id(_s)}_split{int(_sp)}", "mvi_conv3t_n320")(_conv3t(_s, _sp))


def _conv3x3_s2_dgrad(shape):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        N, h, w, Ci, Co = shape
        c = E.conv3x3_s2_dgrad_case("parity", tag, *shape)
        assert ops.conv3x3_s2_dgrad_supported(Ci, Co, dt)
        wt = ops.conv3x3_n320_weight(ops.conv3x3_transposed_weight(exact_dev(c.w, dt)))
        call = lambda dy, wt: ops.conv3x3_s2_dgrad(dy, wt, 2 * h, 2 * w)
        return Built(call, [exact_dev(E.tokens(c.dy), dt), wt], lambda outs: equal("s2_dgrad", E.planes(outs[0], 2 * h, 2 * w), c.want))
    return build


for _s in E.CONV3X3_S2_DGRAD[:2]:
    case(f"conv3x3_s2_dgrad_{_id(_s)}", "mvi_conv3x3_s2_dgrad")(_conv3x3_s2_dgrad(_s))


def _conv_gnstats(taps, N, Hh, W, C, Co, frames):
    """The convolution with the GroupNorm partials in its epilogue, and the norm that consumes them (the partials are opaque: they are
    tested through group_norm_silu_tok2tok(partials=...)): the data and the bars of
    tests/test_unet_ops_gpu.py::test_groupnorm_statistics_from_the_convolution_epilogue at the smallest shape the epilogue takes."""
    def build(ops, tag):
        dt = E.DTYPES[tag]
        g = torch.Generator().manual_seed(C + taps)
        samples, S = (N, Hh * W) if taps == 9 else (N * Hh, W)
        tok = (torch.randn(samples, S, C, generator=g) * 0.7).to(dt).to(DEV)
        if taps == 9:
            wt = ops.conv3x3_n320_weight((torch.randn(Co, C, 3, 3, generator=g) / (3.0 * C ** 0.5)).to(dt).to(DEV))
            conv = lambda tok, wt, gn: ops.conv3x3_n320(tok, wt, None, Hh, W, gn=gn)
        else:
            wt = ops.conv3t_n320_weight((torch.randn(Co, C, 3, 1, 1, generator=g) / (1.7 * C ** 0.5)).to(dt).to(DEV))
            conv = lambda tok, wt, gn: ops.conv3t_n320(tok, wt, None, Hh, gn=gn)
        assert ops.conv_n320_gnstats_supported(samples * S, taps, C, Co, S, 32)
        w, bb = (1.0 + 0.1 * torch.randn(Co, generator=g)).to(DEV), (0.1 * torch.randn(Co, generator=g)).to(DEV)
        cb = (0.5 * torch.randn(samples, Co, generator=g)).to(DEV)

        def call(tok, wt, w, bb, cb):
            out, part = conv(tok, wt, (32, cb))
            assert part.chunks == S // 256 and part.part.numel() == samples * (S // 256) * 32 * 3
            return out, ops.group_norm_silu_tok2tok(out, 32, w, bb, 1e-5, True, chan_bias=cb, frames=frames, partials=part)

        def ref(outs):
            out, y = outs
            assert torch.equal(out, conv(tok, wt, None))
            xf = out.double().cpu() + cb.double().cpu()[:, None, :]
            x5 = xf.reshape(samples // frames, frames * S, Co).transpose(1, 2)
            want = F.silu(F.group_norm(x5, 32, w.double().cpu(), bb.double().cpu(), 1e-5)).transpose(1, 2).reshape(samples, S, Co)
            y3 = ops.group_norm_silu_tok2tok(out, 32, w, bb, 1e-5, True, chan_bias=cb, frames=frames)
            scale = max(1.0, want.abs().max().item())
            e_pre, e_3 = (y.double().cpu() - want).abs().max().item() / scale, (y3.double().cpu() - want).abs().max().item() / scale
            assert e_pre <= {"bf16": 1.0 / 64, "f16": 1.0 / 512}[tag] and e_pre <= 1.5 * e_3 + 1e-6, (e_pre, e_3)
        return Built(call, [tok, wt, w, bb, cb], ref, gn=True)
    return build


case("conv3x3_n320_gnstats_1x16x16x64x320", ("mvi_conv3x3_n320_gnstats", "mvi_groupnorm_silu_tok2tok_pre"))(_conv_gnstats(9, 1, 16, 16, 64, 320, 1))
case("conv3t_n320_gnstats_1x2x256x64x320", ("mvi_conv3t_n320_gnstats", "mvi_groupnorm_silu_tok2tok_pre"))(_conv_gnstats(3, 1, 2, 256, 64, 320, 2))


# ---- weight gradients on integers, split and unsplit (tests/test_wgrad_exact_gpu.py) ------------------------------------------------------

def _wgrad_tables():
    import test_wgrad_exact_gpu as W
    return W


def _conv_wgrad(which, idx, split):
    def build(ops, tag):
        W = _wgrad_tables()
        dt = E.DTYPES[tag]
        if which == "t3":
            shape = W.CONV3T[idx]
            x, dy, want = W._conv3t_case(shape)
            ws = ops.conv3t_wgrad_workspace_bytes(*shape)
            xd, dyd = x.to(dt).to(DEV), dy.to(dt).to(DEV)
            call = lambda x, dy: ops.conv3t_wgrad(x, dy, shape[1], split=split)
        else:
            shape = (W.CONV3X3 if which == "s1" else W.CONV3X3_S2)[idx]
            x, dy, want = W._conv3x3_case(shape, 1 if which == "s1" else 2)
            fn, wsf = (ops.conv3x3_wgrad, ops.conv3x3_wgrad_workspace_bytes) if which == "s1" else (ops.conv3x3_s2_wgrad, ops.conv3x3_s2_wgrad_workspace_bytes)
            ws = wsf(*shape)
            xd, dyd = W.B.tokens(x).to(dt).to(DEV), W.B.tokens(dy).to(dt).to(DEV)
            call = lambda x, dy: fn(x, dy, shape[1], shape[2], split=split)
        assert (ws > 0) == (idx > 0), (which, shape, ws)           # the first shape of each list is the unsplit one
        return Built(call, [xd, dyd], lambda outs: equal(which, outs[0], want))
    return build


for _which, _entry, _n in (("s1", "mvi_conv3x3_wgrad", 3), ("s2", "mvi_conv3x3_s2_wgrad", 3), ("t3", "mvi_conv3t_wgrad", 4)):
    for _i, _sp in ((0, True), (1, True), (_n - 1, True), (_n - 1, False)):
        case(f"conv_wgrad_{_which}_{_i}_split{int(_sp)}", _entry)(_conv_wgrad(_which, _i, _sp))


def _linear_wgrad(idx, split, strided, need_dbias):
    def build(ops, tag):
        W = _wgrad_tables()
        dt = E.DTYPES[tag]
        shape = W.LINEAR[idx]
        rows, K, N = shape
        x, dy, want_w, want_b = W._linear_case(shape, strided)
        assert (ops.linear_wgrad_workspace_bytes(*shape) > 0) == (idx > 0)
        if strided:                                               # the views are cut inside the call: the wide matrices are the inputs
            xw, dyw = x._base.to(dt).to(DEV), dy._base.to(dt).to(DEV)
            call = lambda xw, dyw: ops.linear_wgrad(xw[:, :K], dyw[:, N:2 * N], need_dbias, split=split)
            ins = [xw, dyw]
        else:
            call = lambda x, dy: ops.linear_wgrad(x, dy, need_dbias, split=split)
            ins = [x.to(dt).to(DEV), dy.to(dt).to(DEV)]

        def ref(outs):
            equal("dweight", outs[0], want_w)
            if need_dbias:
                equal("dbias", outs[1], want_b)
            else:
                assert outs[1] is None
        return Built(call, ins, ref)
    return build


for _i, _sp, _st, _db in ((0, True, False, True), (1, True, False, True), (3, True, False, False), (3, False, False, True), (1, True, True, True),
                          (3, True, True, True)):
    case(f"linear_wgrad_{_i}_split{int(_sp)}{'_strided' if _st else ''}{'' if _db else '_nodbias'}", "mvi_linear_wgrad")(_linear_wgrad(_i, _sp, _st, _db))


# ---- stem convolution: forward, dz, wgrad, dgrad ---------------------------------------------------------------------------------------------

STEM = [(1, 16, 16, 9, 72, 1), (1, 16, 32, 9, 80, 2)]                 # two of exact_gemm_helpers.STEM, one per stride
assert all(s in E.STEM for s in STEM)
STEM_TOL = {"bf16": 1.0 / 128, "f16": 1.0 / 1024}                     # tests/test_stem_conv_bwd_gpu.py TOL


def _stem_forward(shape):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        c = E.stem_case("parity", tag, *shape)
        call = lambda x, w, b: ops.stem_conv3x3_silu(x, w, b, silu=False, stride=shape[5])
        return Built(call, [exact_dev(c.x, dt), exact_dev(c.w, dt), P(c.b)], lambda outs: equal("stem", outs[0], c.want))
    return build


def _stem_dz(shape):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        stride = shape[5]
        x, w, b, dy = SB.make_case(shape[:5], stride, dt, seed=31 + sum(shape[:5]) + stride)
        assert ops.stem_conv3x3_bwd_supported(shape[1], shape[2], shape[4], stride, dt)
        want = SB.dz_formula(x, w, b, dy, stride, True)
        call = lambda x, w, b, dy: ops.stem_conv3x3_dz(x, w, b, dy, silu=True, stride=stride, with_y=True)

        def ref(outs):
            e = SB.errors(outs[0].cpu(), want)[0]
            assert e < STEM_TOL[tag], e
            assert torch.equal(outs[1], ops.stem_conv3x3_silu(x.to(DEV), w.to(DEV), b.to(DEV), silu=True, stride=stride))
        return Built(call, [x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)], ref)
    return build


def _stem_wgrad(shape, need_dbias):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        stride = shape[5]
        N, Ci, Co, Hh, W = shape[:5]
        x, _, _, dz = SB.make_case(shape[:5], stride, dt, seed=31 + sum(shape[:5]) + stride)
        K = dz.numel() // Co
        assert ops.stem_conv3x3_wgrad_workspace_bytes(N, Ci, Co, Hh, W, stride) > 0
        call = lambda x, dz: ops.stem_conv3x3_wgrad(x, dz, stride=stride, need_dbias=need_dbias)

        def ref(outs):
            capped("dweight", outs[0], SB.wgrad_formula(x, dz, stride), 2.0 * K * 2.0 ** -24 * SB.wgrad_formula(x.abs(), dz.abs(), stride))
            if need_dbias:
                capped("dbias", outs[1], SB.dbias_formula(dz), 2.0 * K * 2.0 ** -24 * SB.dbias_formula(dz.abs()))
        return Built(call, [x.to(DEV), dz.to(DEV)], ref)
    return build


def _stem_dgrad(shape):
    def build(ops, tag):
        dt = E.DTYPES[tag]
        c = E.stem_dgrad_case(tag, *shape)
        return Built(lambda dz, w: ops.stem_conv3x3_dgrad(dz, w), [exact_dev(c.dz, dt), exact_dev(c.w, dt)], lambda outs: equal("stem_dgrad", outs[0], c.want))
    return build


for _s in STEM:
    case(f"stem_conv3x3_{_id(_s)}", ("mvi_stem_conv3x3_silu", "mvi_stem_conv3x3_pack"))(_stem_forward(_s))
    case(f"stem_conv3x3_dz_{_id(_s)}", ("mvi_stem_conv3x3_dz", "mvi_stem_conv3x3_pack"))(_stem_dz(_s))
    case(f"stem_conv3x3_wgrad_{_id(_s)}", "mvi_stem_conv3x3_wgrad")(_stem_wgrad(_s, True))
case(f"stem_conv3x3_wgrad_{_id(STEM[0])}_nodbias", "mvi_stem_conv3x3_wgrad")(_stem_wgrad(STEM[0], False))
case(f"stem_conv3x3_dgrad_{_id(E.STEM_DGRAD[0])}", ("mvi_stem_conv3x3_silu", "mvi_stem_conv3x3_pack"))(_stem_dgrad(E.STEM_DGRAD[0]))


# ---- attention, forward (tests/test_attention_exact_gpu.py, the selector set: a key of the wrong row, tile or head selects a wrong value) -

def _check_selector(c, got, tag):
    got = got.detach().cpu()
    assert got.shape == c.want.shape and got.dtype == c.want.dtype
    g, w = got.double(), c.want.double()
    bad = ~((g - w).abs() <= 2.0 ** -13 * w.abs()) if tag == "f32" else ((g != w) | torch.isnan(g))
    assert not bool(bad.any()), int(bad.sum())


def _attention(shape, variant):
    def build(ops, tag):
        dt = EA.DTYPES[tag]
        B, Hh, Sq, Sk = shape[:4]
        Dh = shape[4] if len(shape) > 4 else 64
        assert ops.attention_kernel_variant(Sq, Sk, Dh, dt) == variant
        c = EA.selector_case(tag, B, Hh, Sq, Sk, Dh)
        return Built(lambda q, k, v: ops.attention(q, k, v, Hh), [exact_dev(t, dt) for t in (c.q, c.k, c.v)], lambda outs: _check_selector(c, outs[0], tag))
    return build


case(f"attention_rowtile_{_id(EA.ROWTILE[1])}", "mvi_attention_forward", ("bf16", "f16", "f32"))(_attention(EA.ROWTILE[1], 0))
case(f"attention_flash4_{_id(EA.FLASH4[1])}", "mvi_attention_forward")(_attention(EA.FLASH4[1], 4))
case(f"attention_flash8_{_id(EA.FLASH8[1])}", "mvi_attention_forward")(_attention(EA.FLASH8[1], 16))


def _attention_packed(shape, mode):
    def build(ops, tag):
        dt = EA.DTYPES[tag]
        B, Hh, Sq, Sk = shape
        c = EA.selector_case(tag, B, Hh, Sq, Sk, 64, mode)
        qkv = torch.cat([exact_dev(t, dt) for t in (c.q, c.k, c.v)], -1).contiguous()
        return Built(lambda qkv: ops.attention_packed(qkv, Hh, q_log2=mode == "q_log2"), [qkv], lambda outs: _check_selector(c, outs[0], tag))
    return build


case(f"attention_packed_{_id(EA.PACKED[0])}", "mvi_attention_forward_strided")(_attention_packed(EA.PACKED[0], "scale"))
case(f"attention_packed_qlog2_{_id(EA.PACKED[0])}", "mvi_attention_forward_strided_qlog2")(_attention_packed(EA.PACKED[0], "q_log2"))


def _attention_wide(B, S, Dw):
    """tests/test_vae_gpu.py::test_attention_wide_fp32: library GEMMs around the HIP softmax, 1e-4 relative to fp64."""
    def build(ops, tag):
        g = torch.Generator().manual_seed(B * S + Dw)
        q, k, v = (torch.randn(B, S, Dw, generator=g) for _ in range(3))
        want = F.scaled_dot_product_attention(q.double()[:, None], k.double()[:, None], v.double()[:, None])[:, 0]

        def ref(outs):
            assert float((outs[0].double().cpu() - want).abs().max() / want.abs().max()) < 1e-4
        return Built(lambda q, k, v: ops.attention_wide(q, k, v), [q.to(DEV), k.to(DEV), v.to(DEV)], ref)
    return build


case("attention_wide_2x77x96", "mvi_softmax_rows", ("f32",))(_attention_wide(2, 77, 96))


def _attention_temporal(shape, form):
    def build(ops, tag):
        dt = EA.DTYPES[tag]
        Bo, T, S, Hh, Dh = shape
        c = EA.selector_case(tag, Bo * S, Hh, T, T, Dh, "q_log2" if form == "packed_qlog2" else "scale")
        q, k, v = (exact_dev(EA.to_temporal(t, Bo, S), dt) for t in (c.q, c.k, c.v))
        ct = EA.Case(kind=c.kind, want=EA.to_temporal(c.want, Bo, S))
        ref = lambda outs: _check_selector(ct, outs[0], tag)
        if form == "separate":
            return Built(lambda q, k, v: ops.attention_temporal(q, k, v, Hh, T), [q, k, v], ref)
        qkv = torch.cat([q, k, v], -1).contiguous()
        return Built(lambda qkv: ops.attention_temporal_packed(qkv, Hh, T, q_log2=form == "packed_qlog2"), [qkv], ref)
    return build


T7, T7_ROWTILE, T17 = (2, 7, 5, 2, 64), EA.TEMPORAL_ROWTILE[0], (2, 17, 5, 2, 64)
assert T7 in EA.TEMPORAL
for _s, _tags in ((T7, HALF), (T7_ROWTILE, ALL), (T17, HALF)):
    case(f"attention_temporal_{_id(_s)}", "mvi_attention_temporal", _tags)(_attention_temporal(_s, "separate"))
    case(f"attention_temporal_packed_{_id(_s)}", "mvi_attention_temporal_strided", _tags)(_attention_temporal(_s, "packed"))
for _s in (T7, T17):
    case(f"attention_temporal_packed_qlog2_{_id(_s)}", "mvi_attention_temporal_strided_qlog2")(_attention_temporal(_s, "packed_qlog2"))


# ---- attention under autograd: forward with lse, both backwards ----------------------------------------------------------------------------

LSE_BAR = 4 * 2.0 ** -23                                               # tests/test_attention_exact_gpu.py


def _attention_forward_lse(shape):
    def build(ops, tag):
        dt = EA.DTYPES[tag]
        c = EA.selector_bwd_case(tag, *shape)

        def ref(outs):
            _check_selector(c.fwd, outs[0], tag)
            err = ((outs[1].detach().double().cpu() - c.fwd.lse).abs() / c.fwd.lse.abs().clamp(min=1.0)).max().item()
            assert err <= LSE_BAR, err
        return Built(lambda q, k, v: ops.attention_forward_lse(q, k, v, c.H), [exact_dev(t, dt) for t in (c.fwd.q, c.fwd.k, c.fwd.v)], ref)
    return build


for _s in (EA.FLASH4[1], EA.FLASH8[1]):
    case(f"attention_forward_lse_{_id(_s)}", "mvi_attention_forward_lse")(_attention_forward_lse(_s))


def _check_selector_bwd(c, dq, dk, dv, tag):
    if dv is not None:
        assert EA.dv_mismatches(c, dv.cpu(), tag) == 0
    if dq is not None:
        assert dq.double().abs().max().item() <= (0.0 if tag == "f16" else c.tiny)
    if dk is not None:
        assert ((dk.detach().double().cpu()).abs() / c.dk_bound).max().item() <= 1.0


def _attention_backward(shape, need_dq, need_dkv):
    def build(ops, tag):
        dt = EA.DTYPES[tag]
        assert ops.attention_backward_supported(shape[2], shape[3], 64, dt)
        c = EA.selector_bwd_case(tag, *shape)
        q, k, v = (exact_dev(t, dt) for t in (c.fwd.q, c.fwd.k, c.fwd.v))
        out, lse = ops.attention_forward_lse(q, k, v, c.H)
        call = lambda q, k, v, out, dout, lse: ops.attention_backward(q, k, v, out, dout, lse, c.H, need_dq=need_dq, need_dkv=need_dkv)
        return Built(call, [q, k, v, out, exact_dev(c.dout, dt), lse], lambda outs: _check_selector_bwd(c, *outs, tag))
    return build


for _s in AB.TENSOR_CASES[2:] + [AB.RAGGED_CASES[4]]:
    case(f"attention_backward_{_id(_s)}", "mvi_attention_backward")(_attention_backward(_s, True, True))
case(f"attention_backward_{_id(AB.RAGGED_CASES[4])}_dq_only", "mvi_attention_backward")(_attention_backward(AB.RAGGED_CASES[4], True, False))
case(f"attention_backward_{_id(AB.RAGGED_CASES[4])}_dkv_only", "mvi_attention_backward")(_attention_backward(AB.RAGGED_CASES[4], False, True))


def _attention_temporal_backward(shape):
    def build(ops, tag):
        dt = EA.DTYPES[tag]
        Bo, T, S, Hh, Dh = shape
        c = EA.selector_bwd_case(tag, Bo * S, Hh, T, T, Dh)
        tt = lambda t: exact_dev(EA.to_temporal(t, Bo, S), dt)

        def ref(outs):
            dq, dk, dv = (EA.from_temporal(t.cpu(), Bo, T) for t in outs)
            assert EA.dv_mismatches(c, dv, tag) == 0
            assert max(dq.double().abs().max().item(), dk.double().abs().max().item()) <= (0.0 if tag == "f16" else c.tiny)
        return Built(lambda q, k, v, d: ops.attention_temporal_backward(q, k, v, d, Hh, T), [tt(c.fwd.q), tt(c.fwd.k), tt(c.fwd.v), tt(c.dout)], ref)
    return build


for _s, _tags in ((T7, HALF), (T7_ROWTILE, ALL), (T17, HALF)):
    case(f"attention_temporal_backward_{_id(_s)}", "mvi_attention_temporal_backward", _tags)(_attention_temporal_backward(_s))


# ---- pointwise and layout ops (tests/test_norm_elementwise_gpu.py) ---------------------------------------------------------------------------

PLANES = [(4, 64, (6, 8)), (4, 24, (5, 9))]                           # tests/test_norm_elementwise_gpu.py PLANES, TOKENS, ROWS
TOKENS = [(4, 64, 64), (4, 72, 72)]
ROWS = [(4, 48, 64), (4, 37, 72)]


def _alphas(n=4):
    return H.f32(torch.tensor([H.ALPHAS[i % 4] for i in range(n)], dtype=torch.float64))


def _point(pc):
    return lambda outs: held("pointwise", outs[0], pc.ref, pc.bound)


def _planes_ops(which, N, C, sp):
    def build(ops, tag):
        dt = DTYPES[tag]
        g = H.gen(42, N, C, sp[1], dt == torch.float16)
        shape = (N, C) + tuple(sp)
        h, x = H.point_data(g, dt, *shape), H.point_data(g, dt, *shape)
        bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
        hd, xd, bd = D(h, dt), D(x, dt), P(bias)
        if which == "add":
            return Built(lambda h, b, x: ops.bias_residual_add(h, b, x), [hd, bd, xd], _point(H.ref_bias_residual_add(dt, h, bias, x)))
        if which == "add_nox":
            return Built(lambda h, b: ops.bias_residual_add(h, b, None), [hd, bd], _point(H.ref_bias_residual_add(dt, h, bias, None)))
        if which == "blend":
            al = _alphas(N)
            pc = H.ref_blend(dt, x, h, H.chan(bias, h.dim()), al, lambda v: H.samp(v, h.dim()))
            return Built(lambda h, b, x, a: ops.bias_residual_blend(h, b, x, a), [hd, bd, xd, P(al)], _point(pc))
        if which == "silu":
            return Built(lambda h, b: ops.bias_silu(h, b), [hd, bd], _point(H.ref_bias_silu(dt, h, bias)), inplace=(0,))
        hg = H.grid_data(g, dt, *shape)
        C2 = C // 2 + 4
        sg, cg = H.grid_data(g, dt, N, C2, *sp), H.grid_data(g, dt, N, C2, *sp)
        if which == "concat":
            return Built(lambda h, s, c: ops.concat_add(h, s, c), [D(hg, dt), D(sg, dt), D(cg, dt)],
                         lambda outs: equal("concat_add", outs[0], torch.cat([hg, sg + cg], 1).to(dt)))
        return Built(lambda h, s: ops.concat_add(h, s, None), [D(hg, dt), D(sg, dt)], lambda outs: equal("concat_add", outs[0], torch.cat([hg, sg], 1).to(dt)))
    return build


for _w, _e in (("add", "mvi_bias_residual_add"), ("add_nox", "mvi_bias_residual_add"), ("blend", "mvi_bias_residual_blend"), ("silu", "mvi_bias_silu"),
               ("concat", "mvi_concat_add"), ("concat_noctrl", "mvi_concat_add")):
    for _s in PLANES:
        case(f"planes_{_w}_{_id(_s)}", _e, ALL)(_planes_ops(_w, *_s))


def _rows_ops(which, N, S, C):
    def build(ops, tag):
        dt = DTYPES[tag]
        g = H.gen(43, N, S, C, dt == torch.float16)
        x, h, base = (H.point_data(g, dt, N, S, C) for _ in range(3))
        al = _alphas(N)
        bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
        xd, hd, based, ad, bd = D(x, dt), D(h, dt), D(base, dt), P(al), P(bias)
        if which == "add_lerp":
            return Built(lambda x, h, base, a: ops.add_lerp(x, h, base, a), [xd, hd, based, ad], _point(H.ref_add_lerp(dt, x, h, base, H.samp(al, 3))))
        if which == "add_lerp_noh":
            return Built(lambda x, base, a: ops.add_lerp(x, None, base, a), [xd, based, ad], _point(H.ref_add_lerp(dt, x, None, base, H.samp(al, 3))))
        if which == "fused_add":
            pc = H.point_case(dt, x + bias + h, H.pointwise_cap(2, x.abs() + bias.abs() + h.abs()))
            return Built(lambda x, h, b: ops.rows_fused(x, h, bias=b)[0], [xd, hd, bd], _point(pc))
        if which == "fused_blend":
            pc = H.ref_blend(dt, base, x, bias, al, lambda v: H.samp(v, 3))
            return Built(lambda x, b, base, a: ops.rows_fused(x, bias=b, base=base, alpha=a)[0], [xd, bd, based, ad], _point(pc))
        if which == "fused_concat":
            ag, bg, cg = (H.grid_data(g, dt, N, S, C) for _ in range(3))
            a1 = H.grid_data(g, dt, N, S, 24)
            return Built(lambda a, b, base: ops.rows_fused(a, b, base=base, concat=True)[0], [D(a1, dt), D(bg, dt), D(cg, dt)],
                         lambda outs: equal("rows_fused concat", outs[0], torch.cat([a1, bg + cg], 2).to(dt)))
        a, b = x.reshape(N * S, C), h.reshape(N * S, C)                # rows_axpb: fp32 only; the result lands in b
        al32 = float(torch.tensor(0.3, dtype=torch.float32))
        pc = H.point_case(dt, a + al32 * (b + bias), H.pointwise_cap(3, a.abs() + abs(al32) * (b.abs() + bias.abs())))
        return Built(lambda a, b, bias: ops.rows_axpb(a, b, bias, 0.3), [D(a, dt), D(b, dt), bd], _point(pc), inplace=(1,))
    return build


for _w, _e, _tags in (("add_lerp", "mvi_add_lerp", ALL), ("add_lerp_noh", "mvi_add_lerp", ALL), ("fused_add", "mvi_rows_fused_gnstats", ALL),
                      ("fused_blend", "mvi_rows_fused_gnstats", ALL), ("fused_concat", "mvi_rows_fused_gnstats", ALL), ("axpb", "mvi_rows_axpb_f32", ("f32",))):
    for _s in ROWS:
        case(f"rows_{_w}_{_id(_s)}", _e, _tags)(_rows_ops(_w, *_s))


def _rows_fused_partials(mode, C):
    """rows_fused(groups=32) and the norm that consumes its partials, as
    tests/test_norm_elementwise_gpu.py::test_group_norm_silu_tok2tok_on_rows_fused_partials (no outlier): one full block of the statistics
    pass and a ragged one per sample."""
    def build(ops, tag):
        dt = DTYPES[tag]
        N, frames = 4, (2 if mode == "blend" else 1)
        one = _lib().mvi_groupnorm_tok2tok_workspace_bytes(1, C, 1, 32, ops._DT[dt])
        rows = next(s for s in range(1, 4096) if _lib().mvi_groupnorm_tok2tok_workspace_bytes(1, C, s + 1, 32, ops._DT[dt]) != one)
        S = rows + 37
        assert ops.rows_gnstats_supported(N, C, S, 32, dt)
        c = H.gn_case(tag, N, C, S, 32, frames, False, True, 0, rows, ident=1)
        g = H.gen(41, C, 0, ("add", "blend", "concat").index(mode), dt == torch.float16)
        x = c.x.transpose(1, 2).contiguous()
        w, b_ = P(c.w), P(c.b)
        norm = lambda out, part, w, b_: ops.group_norm_silu_tok2tok(out, 32, w, b_, c.eps, True, frames=frames, partials=part)
        pc = None
        if mode == "add":
            b = H.q(0.25 * torch.randn(N, S, C, generator=g, dtype=torch.float64), dt)
            bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
            pc = H.point_case(dt, x + bias + b, H.pointwise_cap(2, x.abs() + bias.abs() + b.abs()))
            ins = [D(x, dt), D(b, dt), P(bias), w, b_]
            fused = lambda x, b, bias: ops.rows_fused(x, b, bias=bias, groups=32)
        elif mode == "blend":
            a = H.q(0.25 * torch.randn(N, S, C, generator=g, dtype=torch.float64), dt)
            bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
            alpha = H.f32(torch.tensor(H.ALPHAS, dtype=torch.float64))
            pc = H.ref_blend(dt, x, a, bias, alpha, lambda v: H.samp(v, 3))
            ins = [D(a, dt), P(bias), D(x, dt), P(alpha), w, b_]
            fused = lambda a, bias, x, alpha: ops.rows_fused(a, bias=bias, base=x, alpha=alpha, groups=32)
        else:
            C1 = C // 2
            ins = [D(x[..., :C1].contiguous(), dt), D(x[..., C1:].contiguous(), dt), w, b_]
            fused = lambda x1, x2: ops.rows_fused(x1, x2, groups=32, concat=True)

        def call(*a):
            out, part = fused(*a[:-2])
            assert part is not None
            return out, norm(out, part, *a[-2:])

        def ref(outs):
            out, y = outs
            if pc is None:
                equal("rows_fused concat", out, x.to(dt))
            else:
                held("rows_fused", out, pc.ref, pc.bound)
            stored = out.double().cpu()
            x5 = stored.transpose(1, 2).reshape(N // frames, frames, 32, C // 32, S)
            want, cap = H.norm_cap(x5, (1, 3, 4), c.w.reshape(1, 1, 32, -1, 1), c.b.reshape(1, 1, 32, -1, 1), c.eps, True, 1.0)
            want, cap = want.reshape(N, C, S).transpose(1, 2), cap.reshape(N, C, S).transpose(1, 2)
            held("tok2tok on partials", y, want, H.bound(want, cap, dt))
        return Built(call, ins, ref, gn=True)
    return build


for _mode in ("add", "blend", "concat"):
    for _C in (64, 96):
        case(f"rows_fused_partials_{_mode}_C{_C}", ("mvi_rows_fused_gnstats", "mvi_groupnorm_silu_tok2tok_pre"))(_rows_fused_partials(_mode, _C))


def _token_plane_ops(which, N, C, S):
    def build(ops, tag):
        dt = DTYPES[tag]
        g = H.gen(44, N, C, S, dt == torch.float16)
        tok, base = H.point_data(g, dt, N, S, C), H.point_data(g, dt, N, S, C)
        x = H.point_data(g, dt, N, C, S)
        bias = H.f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
        sp = (S // 8, 8)
        tp = tok.transpose(1, 2)
        bc = bias[None, :, None]
        tg, xg = H.grid_data(g, dt, N, S, C), H.grid_data(g, dt, N, C, S)
        if which == "t2p_bias":
            pc = H.point_case(dt, tp + bc + x, H.pointwise_cap(2, tp.abs() + bc.abs() + x.abs()))
            return Built(lambda t, x, b: ops.tokens_to_planes_add(t, x, bias=b).reshape(N, C, S), [D(tok, dt), D(x, dt).reshape(N, C, *sp), P(bias)], _point(pc))
        if which == "t2p":
            return Built(lambda t, x: ops.tokens_to_planes_add(t, x).reshape(N, C, S), [D(tg, dt), D(xg, dt).reshape(N, C, *sp)],
                         lambda outs: equal(which, outs[0], (tg.transpose(1, 2) + xg).to(dt)))
        if which == "t2p_layout":
            return Built(lambda t: ops.tokens_to_planes_add(t, None, spatial=sp).reshape(N, C, S), [D(tg, dt)],
                         lambda outs: equal(which, outs[0], tg.transpose(1, 2).contiguous().to(dt)))
        if which == "p2t_bias":
            pc = H.point_case(dt, (x + tp + bc).transpose(1, 2), H.pointwise_cap(2, (x.abs() + tp.abs() + bc.abs()).transpose(1, 2)))
            return Built(lambda x, t, b: ops.planes_add_to_tokens(x, t, bias=b), [D(x, dt).reshape(N, C, *sp), D(tok, dt), P(bias)], _point(pc))
        if which == "p2t":
            return Built(lambda x, t: ops.planes_add_to_tokens(x, t), [D(xg, dt).reshape(N, C, *sp), D(tg, dt)],
                         lambda outs: equal(which, outs[0], (xg.transpose(1, 2) + tg).to(dt)))
        if which == "blend":
            al = _alphas(N)
            pc = H.ref_blend(dt, base.transpose(1, 2), tp, bc, al, lambda v: H.samp(v, 3))
            return Built(lambda t, base, b, a: ops.tokens_blend_to_planes(t, base, b, a, sp).reshape(N, C, S), [D(tok, dt), D(base, dt), P(bias), P(al)], _point(pc))
        up = 2 if which == "planes_to_tokens_up2" else 1                # the layout change alone: exact
        x4 = xg.reshape(N, C, *sp)
        want = (F.interpolate(x4, scale_factor=2, mode="nearest") if up == 2 else x4).permute(0, 2, 3, 1).reshape(N, S * up * up, C).contiguous().to(dt)
        return Built(lambda x: ops.planes_to_tokens(x, upsample=up), [D(xg, dt).reshape(N, C, *sp)], lambda outs: equal(which, outs[0], want))
    return build


for _w, _e in (("t2p_bias", "mvi_tokens_to_planes_add_bias"), ("t2p", "mvi_tokens_to_planes_add"), ("t2p_layout", "mvi_tokens_to_planes_add"),
               ("p2t_bias", "mvi_planes_add_to_tokens"), ("p2t", "mvi_planes_add_to_tokens"), ("blend", "mvi_tokens_blend_to_planes"),
               ("planes_to_tokens", "mvi_planes_to_tokens"), ("planes_to_tokens_up2", "mvi_planes_to_tokens")):
    for _s in TOKENS:
        case(f"tokens_{_w}_{_id(_s)}", _e, ALL)(_token_plane_ops(_w, *_s))


def _geglu(rows, inner):
    def build(ops, tag):
        c = H.geglu_case(tag, rows, inner)
        return Built(lambda h: ops.geglu(h), [D(c.h, c.dtype)], lambda outs: held("geglu", outs[0], c.ref, c.bound))
    return build


def _geglu_backward(rows, inner):
    def build(ops, tag):
        c = NB.geglu_bwd_case(tag, rows, inner)

        def ref(outs):
            assert NB.tail_ok(outs[0].detach().cpu(), c) == 0
            held("geglu_backward", outs[0], c.ref, c.bound)
        return Built(lambda h, dy: ops.geglu_backward(h, dy), [D(c.h, c.dtype), D(c.dy, c.dtype)], ref)
    return build


for _s in ((3, 8), (5, 64), (37, 200)):                               # tests/test_norm_elementwise_gpu.py::test_geglu
    case(f"geglu_{_id(_s)}", "mvi_geglu", ALL)(_geglu(*_s))
for _s in (NB.GEGLU_BWD_SHAPES[0], NB.GEGLU_BWD_SHAPES[3]):
    case(f"geglu_backward_{_id(_s)}", "mvi_geglu_backward", ALL)(_geglu_backward(*_s))


def _ff_geglu_backward(shape, need):
    """tests/test_geglu_bwd_gpu.py: the fp64 formula, 2.0 x / 1.6 x the reference's own error of the shape. dweight goes through the
    library GEMM (no fixed summation order): it is held to its bar, not to bit identity — the kernel's own outputs dx, dbias, dh are."""
    def build(ops, tag):
        dt = GG.DTYPES[tag]
        rows, K, inner = shape
        assert ops.ff_geglu_backward_supported(K, inner, dt)
        x, w, b, dy = GG.make_inputs(shape, dt)
        _, fdx, fdw, fdb = GG.formula(x, w, b, dy)
        r = GG.ref_error_for(shape, tag)
        last = {}

        def call(x, w, b, dy):
            dx, dw, db, dh = ops._ff_geglu_backward(x, w, b, dy, *need)
            last["dw"] = dw
            return dx, db, dh

        def ref(outs):
            for name, got, want in (("dx", outs[0], fdx), ("dweight", last["dw"], fdw), ("dbias", outs[1], fdb)):
                if got is None:
                    continue
                e_max, e_rms = GG.errors(got.cpu().to(dt), want)
                assert e_max <= 2.0 * r[name + "_max"] and e_rms <= 1.6 * r[name + "_rms"], (name, e_max, e_rms, r)
            assert (outs[0] is None) == (not need[0]) and (outs[2] is None) == (not (need[1] or need[2]))
        return Built(call, [x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)], ref, foreign=(1,))      # dbias: torch's column sum of the guarded dh
    return build


# geglu_bwd_helpers.TAIL_CASES[0] has K = 96: the elementwise pair takes it (geglu / geglu_backward above cover that kernel); the fused
# kernel is K = 320 only (mvi_ff_geglu_backward_supported), so every combination of outputs runs on TAIL_CASES[1], the smallest it takes
for _n in [n for n in ((dx, dw, db) for dx in (True, False) for dw in (True, False) for db in (True, False)) if any(n)]:
    case(f"ff_geglu_backward_{_id(GG.TAIL_CASES[1])}_{''.join('xwb'[i] for i in range(3) if _n[i])}", "mvi_ff_geglu_backward")(
        _ff_geglu_backward(GG.TAIL_CASES[1], _n))


def _softmax(cols):
    def build(ops, tag):
        c = H.softmax_case(tag, cols)
        return Built(lambda x: ops.softmax_rows_(x, H.SOFTMAX_SCALE), [D(c.x, c.dtype)], lambda outs: held("softmax", outs[0], c.ref, c.bound), inplace=(0,))
    return build


for _c in (1, 65, 300):
    case(f"softmax_rows_{_c}", "mvi_softmax_rows", ALL)(_softmax(_c))


def _pool2x2(N, h, w, C):
    """tests/test_resample_conv_bwd_gpu.py::test_pool2x2_sum: an fp32 sum of four rounded once."""
    def build(ops, tag):
        dt = DTYPES[tag]
        g = torch.randn(N, 4 * h * w, C, generator=torch.Generator().manual_seed(N + h + w + C)).to(dt)
        cells = g.double().reshape(N, h, 2, w, 2, C)
        s, sa = cells.sum(dim=(2, 4)).reshape(N, h * w, C), cells.abs().sum(dim=(2, 4)).reshape(N, h * w, C)
        bnd = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}[tag] * s.abs() + 4 * 2.0 ** -24 * sa
        return Built(lambda g: ops.pool2x2_sum(g, h, w), [g.to(DEV)], lambda outs: capped("pool2x2_sum", outs[0], s, bnd))
    return build


for _s in ((1, 1, 1, 8), (2, 3, 5, 320)):
    case(f"pool2x2_sum_{_id(_s)}", "mvi_rows_pool2x2_sum")(_pool2x2(*_s))


# ---- block-tail backwards and their reduces (tests/test_block_tails_bwd_gpu.py) ------------------------------------------------------------

PLANES_TAIL_SHAPES = [(3, 64, 72), (2, 72, 64)]                       # tests/test_block_tails_bwd_gpu.py PLANES_SHAPES[1:3]
ROWS_TAIL_SHAPES = [(3, 37, 64), (6, 144, 1280)]                      # ROWS_SHAPES[1], ROWS_SHAPES[3]


def _same_bits(a, b):
    it = torch.int16 if a.element_size() == 2 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it).cpu(), b.contiguous().view(it).cpu())


def _frac(got, ref, cap):
    d = (got.double().cpu() - ref).abs()
    assert bool((d[cap == 0] == 0).all())
    return (d[cap > 0] / cap[cap > 0]).max().item() if bool((cap > 0).any()) else 0.0


def _planes_tail(shape, blend):
    def build(ops, tag):
        dt = BT.DTYPES[tag]
        N, C, S = shape
        dy, tok, base, bias, alpha = BT.make_planes(N, C, S, dt, seed=7)
        assert ops.block_tails_backward_supported(C, S, dt)
        dyt = dy.transpose(1, 2).contiguous()
        if not blend:
            assert ops.planes_tail_backward_workspace_bytes(N, C, S, ops.TAILS_DBIAS) > 0
            want = BT.planes_formulas(dy)

            def ref(outs):
                assert outs[1] is None and outs[3] is None and _same_bits(outs[0], dyt)
                assert _frac(outs[2], want["dbias"], BT.dbias_cap(dy)) <= 1.0
            return Built(lambda dy: ops.planes_tail_backward(dy, need_dtok=True, need_dbias=True), [dy.to(DEV)], ref)
        want = BT.planes_formulas(dy, alpha=alpha, tok=tok, bias=bias)
        want_tok = ((1.0 - alpha).reshape(N, 1, 1) * dyt.float()).to(dt)

        def ref(outs):
            d_tok, d_base, dbias, dalpha = outs
            assert _same_bits(d_tok, want_tok) and _same_bits(d_base, dyt)
            assert _frac(dbias, want["dbias"], BT.dbias_cap(dy, alpha)) <= 1.0
            assert _frac(dalpha, want["dalpha"], BT.planes_dalpha_cap(dy, tok, bias)) <= 1.0
        call = lambda dy, a, tok, bias: ops.planes_tail_backward(dy, alpha=a, tok=tok, bias=bias, need_dtok=True, need_dbase=True, need_dbias=True)
        return Built(call, [dy.to(DEV), alpha.to(DEV), tok.to(DEV), bias.to(DEV)], ref)
    return build


def _rows_tail(shape):
    def build(ops, tag):
        dt = BT.DTYPES[tag]
        G, row_div, C = shape
        dy, x, h, base, alpha = BT.make_rows(G, row_div, C, dt, seed=9)
        assert ops.rows_tail_backward_workspace_bytes(G * row_div, C, row_div) > 0
        a = alpha.repeat_interleave(row_div).reshape(-1, 1)
        want_t, want_base = ((1.0 - a) * dy.float()).to(dt), (a * dy.float()).to(dt)
        t = (x.float() + h.float()).to(dt)
        want = BT.rows_formulas(dy, alpha, base=base, t=t)

        def ref(outs):
            assert _same_bits(outs[0], want_t) and _same_bits(outs[1], want_base)
            assert _frac(outs[2], want["dalpha"], BT.rows_dalpha_cap(dy, base, t, G)) <= 1.0
        call = lambda dy, a, x, h, base: ops.rows_tail_backward(dy, a, x=x, h=h, base=base)
        return Built(call, [dy.to(DEV), alpha.to(DEV), x.to(DEV), h.to(DEV), base.to(DEV)], ref)
    return build


for _s in PLANES_TAIL_SHAPES:
    case(f"planes_tail_backward_add_{_id(_s)}", ("mvi_planes_tail_backward", "mvi_planes_tail_reduce"))(_planes_tail(_s, False))
    case(f"planes_tail_backward_blend_{_id(_s)}", ("mvi_planes_tail_backward", "mvi_planes_tail_reduce"))(_planes_tail(_s, True))
for _s in ROWS_TAIL_SHAPES:
    case(f"rows_tail_backward_{_id(_s)}", ("mvi_rows_tail_backward", "mvi_rows_tail_reduce"))(_rows_tail(_s))


# ---- first stage: split-operand convolutions, the fp32 stem, the operand producer (tests/test_split3_exact_gpu.py) ------------------------

def _conv_split3(geom, shape):
    def build(ops, tag):
        c = S3.conv_case(geom, "unit", shape)
        n, a, b = c.dims
        x2 = exact_dev(torch.cat([c.xh.reshape(-1, c.C), c.xl.reshape(-1, c.C)], dim=1), torch.bfloat16)
        w3 = ops.split3_weight(c.w32.to(DEV))
        if geom == "s2":
            call = lambda x2, w3: ops.conv_split3_s2(x2, w3, n, a, b, c.Co)
        else:
            call = lambda x2, w3: ops.conv_split3(x2, w3, n, a, b, c.Co, taps=c.taps)
        return Built(call, [x2, w3], lambda outs: equal(geom, outs[0], c.want))
    return build


for _geom, _e, _shapes in (("conv9", "mvi_conv3x3_split3_f32", (S3.CONV9[0], S3.CONV9[1])), ("conv3t", "mvi_conv3t_split3_f32", (S3.CONV3T[0], S3.CONV3T[1])),
                           ("s2", "mvi_conv3x3_s2_split3_f32", (S3.S2[0], S3.S2[2]))):
    for _s in _shapes:
        case(f"conv_split3_{_geom}_{_id(_s)}", _e, ("bf16",))(_conv_split3(_geom, _s))


def _conv_in_f32(N, Ci, Hh, W, Co):
    """tests/test_vae_encode_split_gpu.py::test_stem_writes_fp32_tokens: |got - want| <= 28 2^-24 (conv(|x|, |w|) + |b|)."""
    def build(ops, tag):
        g = torch.Generator().manual_seed(N * 100 + Ci * 10 + Hh + Co)
        x = torch.randn(N, Ci, Hh, W, generator=g) * 1.5
        wt = torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5
        bs = torch.randn(Co, generator=g) * 0.3
        wd, bd = wt.double(), bs.double()
        want = F.conv2d(x.double(), wd, bd, padding=1).permute(0, 2, 3, 1).reshape(N, Hh * W, Co)
        mag = F.conv2d(x.double().abs(), wd.abs(), bd.abs(), padding=1).permute(0, 2, 3, 1).reshape(N, Hh * W, Co)

        def call(x, wt, bs):
            conv = types.SimpleNamespace(weight=wt, bias=bs, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1,
                                         padding_mode="zeros", in_channels=Ci, out_channels=Co)
            return ops.conv_in_f32_tokens(x, conv)
        return Built(call, [x.to(DEV), wt.to(DEV), bs.to(DEV)], lambda outs: capped("conv_in", outs[0], want, 28 * 2.0 ** -24 * mag))
    return build


for _s in ((1, 1, 2, 2, 128), (2, 3, 9, 15, 128)):
    case(f"conv_in_f32_tokens_{_id(_s)}", "mvi_conv3x3_small_cin_f32_tokens", ("f32",))(_conv_in_f32(*_s))


def _group_norm_split_plain(S_, Cc, mode):
    def build(ops, tag):
        v = S3.probe_values(S3.gen(45, S_, Cc), S_, Cc)
        hi, lo, _ = S3.bit_split(v.double())
        want = {"split3": torch.cat([hi, lo], dim=2).to(torch.bfloat16), "bf16": hi.to(torch.bfloat16), "f16": v.to(torch.float16)}[mode]

        def ref(outs):
            got = outs[0].cpu()
            assert got.dtype == want.dtype and got.shape == want.shape
            assert not bool(((got != want) & ~(torch.isnan(got.float()) & torch.isnan(want.float()))).any())
        return Built(lambda v: ops.group_norm_split(v, 0, None, None, 0.0, False, mode=mode), [v.to(DEV)], ref)
    return build


def _group_norm_split(N, Cc, S_, frames, mode):
    def build(ops, tag):
        Nt = N * frames
        c = H.gn_case("f32", Nt, Cc, S_, 32, frames, True, True)
        x = c.x.transpose(1, 2).contiguous().float().to(DEV)
        want, cap = c.ref.transpose(1, 2), c.cap.transpose(1, 2)
        dt = {"split3": torch.bfloat16, "bf16": torch.bfloat16, "f16": torch.float16}[mode]

        def ref(outs):
            y = outs[0].cpu()
            assert y.dtype == dt and torch.isfinite(y.float()).all()
            if mode == "split3":
                hi, lo = y[..., :Cc].double(), y[..., Cc:].double()
                s = hi + lo
                assert ((s - want).abs() / (cap + 2.0 ** -17 * (want.abs() + cap))).max().item() <= 1.0
                assert (lo.abs() / (0.5 * E.ulp_of(s, torch.bfloat16))).max().item() <= 1.0
            else:
                assert ((y.double() - want).abs() / H.bound(want, cap, dt)).max().item() <= 1.0
        call = lambda x, w, b, cb: ops.group_norm_split(x, 32, w, b, c.eps, True, chan_bias=cb, frames=frames, mode=mode)
        return Built(call, [x, P(c.w), P(c.b), P(c.cb)], ref, gn=True)
    return build


for _mode in ("split3", "bf16", "f16"):
    case(f"group_norm_split_plain_{_mode}", "mvi_groupnorm_silu_tok2tok_split", ("f32",))(_group_norm_split_plain(65, 64, _mode))
    case(f"group_norm_split_{_mode}_{_id(H.GN_ISSUE_SHAPES[0])}", "mvi_groupnorm_silu_tok2tok_split", ("f32",))(
        _group_norm_split(*H.GN_ISSUE_SHAPES[0], 1, _mode))
case(f"group_norm_split_split3_frames3_{_id(H.GN_ISSUE_SHAPES[3])}", "mvi_groupnorm_silu_tok2tok_split", ("f32",))(
    _group_norm_split(*H.GN_ISSUE_SHAPES[3], 3, "split3"))


PARAMS = [(c, tag) for c in CASES for tag in c.tags]
COVERED = frozenset(e for c in CASES for e in c.entries)

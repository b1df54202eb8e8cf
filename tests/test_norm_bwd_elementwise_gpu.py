"""The backward normalisation and gate kernels (csrc/groupnorm_bwd.hip, csrc/layernorm_bwd.hip, csrc/geglu.hip's geglu_bwd_kernel) against
an fp64 reference of the same operation, ELEMENT BY ELEMENT: |got - ref| <= cap + ulp(|ref| + cap) / 2 on every element of every output,
the caps derived in tests/norm_bwd_exact_helpers.py (tests/test_norm_bwd_elementwise_cpu.py shows what the comparison rejects), torch.equal
where fp32 leaves one answer — dweight == 0 on the channels of the constant group —, and the same bits from a second call. All calls go
through multiview_inpaint_amd.svd.hip_ops. The statistics are the forward's own (group_norm_forward_stats,
group_norm_tok2tok_forward_stats); on the constant group the table must hold the value itself and eps^-1/2 within 4 u, which is what the
caps take for granted there.

Every launch writes one line through svd_helpers.report: entry point, shape, type, the worst ratio to the bound per output, the share of
dx elements whose cap is below a quarter ulp (profiles/norm_bwd_elementwise_gpu.txt is that output of a run on an MI355X).

Out of scope: stem_conv3x3_dz, the fused ff_geglu_backward contraction and every wgrad (tests/test_gemm_exact_gpu.py), the block tails
(tests/test_block_tails_bwd_gpu.py)."""
import pytest
import torch

import norm_bwd_exact_helpers as B
import svd_helpers as SH

pytestmark = pytest.mark.gpu

TAGS = ("f32", "bf16", "f16")


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
    return None if v is None else v.float().cuda()


def twice(fn):
    """fn() twice: the same bits both times."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert torch.equal(u, v), "a second call gave other bits"
    return a


def held(what, tag, got, ref, bnd, quarter, note=""):
    """One report line for the launch, then the bound on every element of every output. got / ref / bnd: dicts over the outputs."""
    ratios, bad = {}, {}
    for k in ref:
        g = got[k].detach().double().cpu()
        assert g.shape == ref[k].shape, (what, k, g.shape, ref[k].shape)
        assert torch.isfinite(g).all(), (what, k)
        ratios[k] = float(((g - ref[k]).abs() / bnd[k]).max())
        bad[k] = int(((g - ref[k]).abs() > bnd[k]).sum())
    SH.report(f"{what} {tag}: worst |got - ref| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items())
              + f"; cap <= ulp / 4 on {quarter:.3f} of dx{note}")
    assert all(v <= 1.0 for v in ratios.values()), (what, tag, ratios, bad)


# ---- group_norm_backward ----------------------------------------------------------------------------------------------------------------------

def const_stats(what, c, stats):
    """The forward's table on the constant group: the value itself and eps^-1/2 within 4 u."""
    st = stats.detach().double().cpu().reshape(c.N // c.T, c.G, 2)[:, B.CONST_GROUP]
    assert (st[:, 0] == c.cv).all(), (what, "the constant group's mean", st[:, 0].tolist())
    assert ((st[:, 1] * c.eps ** 0.5 - 1.0).abs() <= 4.0 * B.U).all(), (what, "the constant group's rstd", st[:, 1].tolist())


def gn_check(what, c, dx_ncs, dw, db, dcb):
    got = dict(dx=dx_ncs, dweight=dw, dbias=db)
    if c.cb is not None:
        got["dchan_bias"] = dcb
    assert dx_ncs.dtype == c.dtype and dw.dtype == db.dtype == torch.float32
    zeros = int((dw.detach().cpu()[c.const_c] != 0).sum())
    held(what, c.tag, got, c.ref, c.bound, c.quarter, f"; dweight == 0 on the constant group ({c.cv}): {zeros} of {int(c.const_c.sum())} channels differ")
    assert zeros == 0, (what, c.tag, "dweight of the constant group", dw.detach().cpu()[c.const_c].tolist())


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("with_cb,silu,cv", B.GN_BWD_VARIANTS)
@pytest.mark.parametrize("N,C,S,G,T,layout", B.GN_BWD_SHAPES)
def test_group_norm_backward(ops, N, C, S, G, T, layout, with_cb, silu, cv, tag):
    c = B.gn_bwd_case(tag, N, C, S, G, T, with_cb, silu, layout, cv)
    lay = {B.PLANES: ops.GN_PLANES, B.STACK3: ops.GN_STACK3, B.TOKENS: ops.GN_TOKENS}[layout]
    assert ops.group_norm_backward_supported(N, C, S, G, T, c.dtype, lay)
    x, w, b, cb = dev(c.x, c.dtype), par(c.w), par(c.b), par(c.cb)
    dy = dev(c.dy.transpose(1, 2).contiguous() if layout == B.TOKENS else c.dy, c.dtype)
    _, stats = ops.group_norm_forward_stats(x, T, G, w, b, c.eps, silu, chan_bias=cb, layout=lay)
    what = f"group_norm_backward {layout} {(N, C, S)} G={G} T={T} cb={with_cb} silu={silu}"
    const_stats(what, c, stats)
    dx, dw, db, dcb = twice(lambda: ops.group_norm_backward(dy, x, stats, T, G, w, b, silu, chan_bias=cb, layout=lay, need_dx=True, need_dparams=True,
                                                            need_dchan_bias=with_cb))
    assert dx.shape == x.shape
    gn_check(what, c, dx, dw, db, dcb)


# ---- group_norm_tok2tok_backward --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("with_cb,silu,cv", B.GN_BWD_VARIANTS)
@pytest.mark.parametrize("N,C,S,G,frames", B.TOK2TOK_SHAPES)
def test_group_norm_tok2tok_backward(ops, N, C, S, G, frames, with_cb, silu, cv, tag):
    """Token-major x, dy and dx; the outputs asked for all together, and one at a time with the same bits."""
    c = B.gn_bwd_case(tag, N, C, S, G, frames, with_cb, silu, B.TOKENS, cv)
    t, dy = dev(c.x.transpose(1, 2).contiguous(), c.dtype), dev(c.dy.transpose(1, 2).contiguous(), c.dtype)
    w, b, cb = par(c.w), par(c.b), par(c.cb)
    _, stats = ops.group_norm_tok2tok_forward_stats(t, G, w, b, c.eps, silu, chan_bias=cb, frames=frames)
    what = f"group_norm_tok2tok_backward {(N, S, C)} G={G} frames={frames} cb={with_cb} silu={silu}"
    const_stats(what, c, stats)
    call = lambda **kw: ops.group_norm_tok2tok_backward(dy, t, stats, G, w, b, silu, chan_bias=cb, frames=frames, **kw)
    dx, dw, db, dcb = twice(lambda: call(need_dx=True, need_dparams=True, need_dchan_bias=with_cb))
    assert dx.shape == t.shape
    gn_check(what, c, dx.transpose(1, 2), dw, db, dcb)
    only_dx = call(need_dx=True)
    only_par = call(need_dx=False, need_dparams=True)
    assert only_dx[1:] == (None, None, None) and only_par[0] is None and only_par[3] is None
    assert torch.equal(only_dx[0], dx) and torch.equal(only_par[1], dw) and torch.equal(only_par[2], db), "an output asked for alone has other bits"
    if with_cb:
        only_cb = call(need_dx=False, need_dchan_bias=True)
        assert only_cb[:3] == (None, None, None) and torch.equal(only_cb[3], dcb), "dchan_bias asked for alone has other bits"


# ---- add_layer_norm_backward ------------------------------------------------------------------------------------------------------------------

def run_ln(ops, c):
    s, w = dev(c.s, c.dtype), par(c.w)
    assert ops.add_layer_norm_backward_supported(c.C, c.dtype)
    g, dw, db, drow = twice(lambda: ops.add_layer_norm_backward(s, w, c.eps, gy=dev(c.gy, c.dtype), gs=dev(c.gs, c.dtype), gs_pre=dev(c.gsp, c.dtype),
                                                                row_groups=c.runs or None))
    assert g.dtype == c.dtype and dw.dtype == db.dtype == torch.float32 and (drow is None) == (c.runs == 0)
    got = dict(dx=g, dweight=dw, dbias=db)
    if c.runs:
        got["drow"] = drow
    held(f"add_layer_norm_backward {(c.R, c.C)} runs={c.runs} gy,gs,gs_pre={tuple(int(m) for m in c.mode)}", c.tag, got, c.ref, c.bound, c.quarter)


LN_CASES = [(R, C, runs, tag) for tag in TAGS for R, C, runs in B.ln_bwd_shapes(tag)]


@pytest.mark.parametrize("R,C,runs,tag", LN_CASES)
def test_add_layer_norm_backward(ops, R, C, runs, tag):
    run_ln(ops, B.ln_bwd_case(tag, R, C, runs))


def test_the_widest_fp32_row_is_2048(ops):
    """Why the fp32 list has no C = 4096: 64 lanes x 8 vectors of 4 fp32 elements end at 2048, and the wrapper says so."""
    assert ops.add_layer_norm_backward_supported(2048, torch.float32) and not ops.add_layer_norm_backward_supported(4096, torch.float32)
    assert ops.add_layer_norm_backward_supported(4096, torch.bfloat16)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("mode", B.LN_BWD_MODES[1:], ids=lambda m: "".join(str(int(v)) for v in m))
def test_add_layer_norm_backward_gradient_presence(ops, mode, tag):
    """Every set of upstream gradients (gy, gs, gs_pre) but the empty one; all three present runs above."""
    run_ln(ops, B.ln_bwd_case(tag, *B.LN_BWD_MODE_SHAPE, mode))


# ---- geglu_backward ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("rows,inner", B.GEGLU_BWD_SHAPES)
def test_geglu_backward_against_the_true_gate(ops, rows, inner, tag):
    """The gate sweep of geglu_bwd_case; on the deep negative tail the result is a product: the reference's sign, within a factor of two."""
    c = B.geglu_bwd_case(tag, rows, inner)
    (dh,) = twice(lambda: (ops.geglu_backward(dev(c.h, c.dtype), dev(c.dy, c.dtype)),))
    assert dh.dtype == c.dtype and dh.shape == (rows, 2 * inner)
    wrong = B.tail_ok(dh.detach().cpu(), c)
    held(f"geglu_backward {(rows, inner)}", tag, dict(dh=dh), dict(dh=c.ref), dict(dh=c.bound), c.quarter,
         f" (of dh); cap above half an ulp on {c.wide:.3f}; deep tail (g <= {B.TAIL_FROM}): {wrong} of {int(c.tail.sum())} outside a factor of two")
    assert wrong == 0

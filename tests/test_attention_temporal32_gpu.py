"""Temporal attention for 17 .. 32 frames on the GPU: the MFMA forward of csrc/attn_temporal32.hip (bf16 / f16, D = 64) and the
frame-cap-32 instantiation of the temporal backward in csrc/attn_bwd.hip, through hip_ops, svd/ops.py's autograd Function and
CrossAttention.forward_temporal. The 25-frame checkpoint of the reference's stock sampler (svd_xt) is the shape this serves.

Oracles and bars are those of the tests of the 16-frame kernels, imported, not copied: the exact-answer sets of
tests/exact_attention_helpers.py judged by tests/test_attention_exact_gpu.py's checker, the fp64 formula of
tests/attention_bwd_helpers.py with the bars of tests/test_attention_bwd_gpu.py, and the fp64 softmax on the rounded inputs with the
bars of tests/test_unet_ops_gpu.py::test_attention_temporal_mfma_kernel (1/128 in bf16, 1/1024 in f16 of max(1, |ref|max)).
Every test runs with ops.STRICT = True: a GPU tensor that left the HIP path would raise."""
import pytest
import torch

import attention_bwd_helpers as A
import exact_attention_helpers as E
import svd_helpers as H
from test_attention_bwd_gpu import SMALL_LATENT_BAR, SMALL_LATENT_MAX_BAR, _assert_all, _check
from test_attention_exact_gpu import _check_forward, _describe, _dev, _ratio

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF = ("bf16", "f16")
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
# (Bo, T, S, H, D). T = 17: one row into the second key / query tile; 32: no padding; S = 5: fewer problems than waves;
# the last: 20 500 problems, more than the grid holds waves — the grid-stride walk and its prefetch
SMALL = [(2, T, S, 2, 64) for T in (17, 24, 25, 31, 32) for S in (5, 33)]
BIG = (1, 25, 4100, 5, 64)
FORWARD = SMALL + [BIG]
BACKWARD = [((2, T, 5, 2, 64), tag) for T in (17, 25, 32) for tag in HALF] + [((2, 25, 5, 2, 32), "f32")]
_ids = lambda v: v if isinstance(v, str) else "x".join(map(str, v))


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "ATTENTION_BACKWARD", True)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


def _kind(T, Hh, D, dtype, packed, qkv_ts=None, o_ts=None):
    from multiview_inpaint_amd import _lib
    if qkv_ts is None:
        qkv_ts, o_ts = (3 * Hh * D, Hh * D) if packed else (0, 0)
    return _lib.lib().mvi_attention_temporal_kernel_kind(T, Hh, D, CODE[dtype], qkv_ts, o_ts)


def _variant(T, Hh, D, dtype):
    from multiview_inpaint_amd import _lib
    return _lib.lib().mvi_attention_temporal_kernel_variant(T, Hh, D, CODE[dtype], 0, 0)


def test_kernel_selection():
    """mvi_attention_temporal_kernel_kind, the function the C dispatch itself asks: 32 for 17 .. 32 frames in bf16 / f16 at D = 64,
    packed and separate; 16 up to 16 frames; 0 (rowtile) at 33 frames, D = 32, fp32 and a token stride that breaks the 16-byte
    alignment of the rows. mvi_attention_temporal_kernel_variant keeps its meaning: 1 only for the 16-frame kernel."""
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    for dtype in (bf, f16):
        for packed in (False, True):
            for T in (17, 25, 32):
                assert _kind(T, 5, 64, dtype, packed) == 32, (T, dtype, packed)
            assert _kind(14, 5, 64, dtype, packed) == 16 and _kind(16, 5, 64, dtype, packed) == 16
            assert _kind(33, 5, 64, dtype, packed) == 0
            assert _kind(25, 10, 32, dtype, packed) == 0
        assert _kind(25, 5, 64, dtype, False, 3 * 320 + 4, 320) == 0          # q / k / v rows 8 bytes off
        assert _kind(25, 5, 64, dtype, False, 3 * 320, 320 + 2) == 0          # out rows 4 bytes off
        assert _variant(25, 5, 64, dtype) == 0 and _variant(14, 5, 64, dtype) == 1
    assert _kind(25, 5, 64, f32, False) == 0 and _kind(25, 5, 64, f32, True) == 0


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 1.0 / 128), (torch.float16, 1.0 / 1024)], ids=HALF)
@pytest.mark.parametrize("shape", FORWARD, ids=_ids)
def test_forward_against_fp64_on_the_rounded_inputs(ops, dtype, tol, shape):
    """attention_temporal and attention_temporal_packed against fp64 softmax attention on the same rounded inputs, at gains 1 and 6
    (large logits: one dominant key per row); the packed entry is bit-equal to the separate one."""
    bo, T, S, Hh, D = shape
    assert _kind(T, Hh, D, dtype, True) == 32 and _kind(T, Hh, D, dtype, False) == 32
    g = torch.Generator().manual_seed(T * 100 + S)
    for gain in (1.0, 6.0):
        qkv = (torch.randn(bo * T, S, 3 * Hh * D, generator=g) * gain ** 0.5).to(dtype)
        q, k, v = (t.contiguous() for t in qkv.chunk(3, dim=-1))
        out_p = ops.attention_temporal_packed(qkv.to(DEV), Hh, T)
        out_s = ops.attention_temporal(q.to(DEV), k.to(DEV), v.to(DEV), Hh, T)
        torch.cuda.synchronize()
        assert torch.equal(out_p, out_s)
        rg = lambda t: t.double().reshape(bo, T, S, Hh, D).permute(0, 2, 3, 1, 4)                  # bo s h t d
        att = torch.softmax(rg(q) @ rg(k).transpose(-1, -2) * D ** -0.5, -1) @ rg(v)
        ref = att.permute(0, 3, 1, 2, 4).reshape(bo * T, S, Hh * D)
        err, bar = (out_p.double().cpu() - ref).abs().max().item(), tol * max(1.0, ref.abs().max().item())
        H.report(f"temporal32 forward {_ids(shape)} {dtype} gain {gain}: max |err| {err:.3e}, bar {bar:.3e}")
        assert out_p.dtype == dtype and err <= bar, (shape, gain, err, bar)


@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("shape", FORWARD, ids=_ids)
def test_forward_exact_answer_sets(ops, tag, shape):
    """The selector, uniform and pairs sets per (video, spatial token, head), judged by test_temporal_forward's checker. selector: a
    random mask per problem, so a key from the wrong tile, token or video selects a wrong value; uniform: a dropped or doubled key of
    the second tile leaves a non-zero integer; pairs: the two selected keys lie in different key tiles from T = 17 on."""
    dtype = E.DTYPES[tag]
    Bo, T, S, Hh, D = shape
    for kind in E.sets_for(T):
        c = E.SETS[kind](tag, Bo * S, Hh, T, T, D)
        q, k, v = (_dev(E.to_temporal(t, Bo, S), dtype) for t in (c.q, c.k, c.v))
        out = ops.attention_temporal(q, k, v, Hh, T)
        extra = dict(tie=E.to_temporal(c.tie, Bo, S), ref=E.to_temporal(c.ref, Bo, S)) if kind == "pairs" else {}
        c_t = E.Case(kind=c.kind, want=E.to_temporal(c.want, Bo, S), **extra)
        _check_forward(c_t, out, f"attention_temporal {tag} {kind} {shape}", tag)
        out_p = ops.attention_temporal_packed(torch.cat([q, k, v], -1).contiguous(), Hh, T)
        assert torch.equal(out_p, out), (kind, shape)


@pytest.mark.parametrize("shape,tag", BACKWARD, ids=_ids)
def test_backward_exact_answer_sets(ops, shape, tag):
    """attention_temporal_backward above 16 frames with the assertions of test_temporal_backward. selector: dv the exact sums, dq
    and dk dust below `tiny` (+-0 in f16). uniform (16-bit types): dq, dk under the elementwise bound, dv under the fp32 summation
    cap, == 0 at T = 32 where P = 1 / T is a power of two. Two runs are bit-identical."""
    dtype = E.DTYPES[tag]
    Bo, T, S, Hh, D = shape
    tt = lambda t: _dev(E.to_temporal(t, Bo, S), dtype)
    cases = [E.selector_bwd_case(tag, Bo * S, Hh, T, T, D)]
    if tag != "f32":
        cases.append(E.uniform_bwd_case(tag, Bo * S, Hh, T, T, D))
    for c in cases:
        what = f"temporal backward {c.kind} {tag} {shape}"
        q, k, v, d = tt(c.fwd.q), tt(c.fwd.k), tt(c.fwd.v), tt(c.dout)
        g1 = ops.attention_temporal_backward(q, k, v, d, Hh, T)
        g2 = ops.attention_temporal_backward(q, k, v, d, Hh, T)
        assert all(torch.equal(a, b) for a, b in zip(g1, g2)), what
        dq, dk, dv = (E.from_temporal(t.cpu(), Bo, T) for t in g1)
        if c.kind == "selector":
            assert E.dv_mismatches(c, dv, tag) == 0, f"{what} dv: {_describe(dv.double() != c.dv, dv, c.dv_want)}"
            worst = max(dq.double().abs().max().item(), dk.double().abs().max().item())
            assert worst <= (0.0 if tag == "f16" else c.tiny), (what, worst, c.tiny)
        else:
            rq, rk = _ratio(dq, c.dq, c.dq_bound), _ratio(dk, c.dk, c.dk_bound)
            if T & (T - 1) == 0:                                           # P = 1 / T is a power of two: the sums are exact
                assert bool((dv == 0).all()) and not bool(c.dv_bound.any()), what
                rv = 0.0
            else:
                rv = _ratio(dv, torch.zeros_like(c.dv_bound), c.dv_bound)
            H.report(f"{what}: worst |got - ref| / bound: dq {rq:.3f}, dk {rk:.3f}, dv {rv:.3f}")
            assert rq <= 1.0 and rk <= 1.0 and rv <= 1.0, (what, rq, rk, rv)


@pytest.mark.parametrize("shape,tag", BACKWARD, ids=_ids)
def test_backward_against_the_regrouped_fp64_formula(shape, tag):
    """ops.attention_temporal under autograd above 16 frames, with the bars of test_temporal_backward_against_the_regrouped_fp64_formula:
    fp32 I/O 1e-4 relative; bf16 / f16 1.6 x (rms) / 2.0 x (max) the largest reference error of the type in ref_errors.json. The
    forward under autograd is the inference forward, and the profile shows the two HIP kinds and nothing else."""
    from multiview_inpaint_amd.svd import hip_ops, ops
    dtype = E.DTYPES[tag]
    bo, T, S, Hh, D = shape
    g = torch.Generator().manual_seed(7 + S + T)
    q, k, v, dy = (torch.randn(bo * T, S, Hh * D, generator=g).to(dtype) for _ in range(4))
    ref_out, rdq, rdk, rdv = A.temporal_formula(q, k, v, dy, Hh, T)
    qa, ka, va = (t.to(DEV).requires_grad_() for t in (q, k, v))
    hip_ops.PROFILE = []
    try:
        out = ops.attention_temporal(qa, ka, va, Hh, T)
        out.backward(dy.to(DEV))
        kinds = [p[0] for p in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = None
    assert kinds == ["attention_temporal", "attention_temporal_bwd"], kinds
    with torch.no_grad():
        assert torch.equal(out.detach(), ops.attention_temporal(qa, ka, va, Hh, T))
    again = hip_ops.attention_temporal_backward(qa.detach(), ka.detach(), va.detach(), dy.to(DEV), Hh, T)
    assert all(torch.equal(a, b) for a, b in zip(again, (qa.grad, ka.grad, va.grad)))
    name = "temporal32 " + _ids(shape)
    if dtype == torch.float32:
        for n, got, ref in (("dq", qa.grad, rdq), ("dk", ka.grad, rdk), ("dv", va.grad, rdv)):
            e_max, e_rms = A.errors(got.cpu(), ref)
            H.report(f"{name} fp32 {n}: max {e_max:.2e}, rms {e_rms:.2e}")
            assert e_max <= 1e-4 and e_rms <= 1e-4, (n, e_max, e_rms)
        return
    r = A.ref_error_for((0, 0, 0, 0), tag)                      # no entry of this shape: the largest of the type
    _assert_all([_check(f"{name} {tag} dq", qa.grad, rdq, r["dx_max"], r["dx_rms"]),
                 _check(f"{name} {tag} dk", ka.grad, rdk, r["dcontext_max"], r["dcontext_rms"]),
                 _check(f"{name} {tag} dv", va.grad, rdv, r["dcontext_max"], r["dcontext_rms"])])


def test_cross_attention_module_at_25_frames_stays_on_the_hip_path():
    """CrossAttention(128, heads 2, dim_head 64).forward_temporal at T = 25, S = 9 in bf16 with parameters requiring grad: no
    attention_temporal fallback is recorded, the profile shows the HIP forward and backward, and the gradients of x and of the four
    weights are held against the same module in fp32 on the regrouping PyTorch route. Yardstick, as in
    test_cross_attention_module_under_checkpoint_against_the_parent_route: the bf16 module on that same regrouping route (the route
    before this feature, ATTENTION_BACKWARD off and strict mode lifted for that one run) against the fp32 result; the HIP route's
    error may be at most 1.6 x (rms) / 2.0 x (max) of it per gradient tensor."""
    from multiview_inpaint_amd.svd import hip_ops, ops
    from multiview_inpaint_amd.svd.transformer import CrossAttention
    assert (SMALL_LATENT_BAR, SMALL_LATENT_MAX_BAR) == (1.6, 2.0)
    T, S, dt = 25, 9, torch.bfloat16
    torch.manual_seed(25)
    m32 = CrossAttention(query_dim=128, heads=2, dim_head=64)
    with torch.no_grad():                                        # weights and inputs representable in bf16 on both sides
        for p in m32.parameters():
            p.copy_(p.to(dt).float())
    x = torch.randn(2 * T, S, 128).to(dt)
    dy = torch.randn(2 * T, S, 128).to(dt)

    def run(dtype, hip):
        m = CrossAttention(query_dim=128, heads=2, dim_head=64)
        m.load_state_dict(m32.state_dict())
        m = m.to(DEV, dtype)
        xg = x.to(DEV, dtype).requires_grad_()
        ops.STRICT, ops.ATTENTION_BACKWARD = hip, hip           # (both restored by the module's fixture)
        del ops.FALLBACKS[:]
        hip_ops.PROFILE = []
        try:
            m.forward_temporal(xg, T).backward(dy.to(DEV, dtype))
            kinds = [p[0] for p in hip_ops.PROFILE]
        finally:
            hip_ops.PROFILE = None
            ops.STRICT, ops.ATTENTION_BACKWARD = True, True
        return {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters()}}, kinds, list(ops.FALLBACKS)

    new, kinds, fallbacks = run(dt, True)
    assert not [f for f in fallbacks if f[0].startswith("attention")], fallbacks
    assert kinds.count("attention_temporal") == 1 and kinds.count("attention_temporal_bwd") == 1, kinds
    ref, _, ref_fallbacks = run(torch.float32, False)
    old, old_kinds, old_fallbacks = run(dt, False)
    for fb in (ref_fallbacks, old_fallbacks):
        assert ("attention_temporal", "requires grad") in fb, fb
    assert "attention_temporal_bwd" not in old_kinds
    results = []
    for name, r in ref.items():
        r = r.double().cpu()
        o_max, o_rms = A.errors(old[name].cpu(), r)
        results.append(_check(f"CrossAttention 128/2 T=25 S=9 bf16 d{name} (against the PyTorch route's own error {o_max:.2e} / {o_rms:.2e})",
                              new[name], r, o_max, o_rms))
    _assert_all(results)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=HALF)
@pytest.mark.parametrize("T", [14, 16])
def test_small_path_is_unchanged(ops, dtype, T):
    """Up to 16 frames the 16-frame kernel still serves the call (kind 16, variant 1), and two calls agree bit for bit."""
    bo, S, Hh, D = 2, 33, 5, 64
    assert _kind(T, Hh, D, dtype, False) == 16 and _kind(T, Hh, D, dtype, True) == 16 and _variant(T, Hh, D, dtype) == 1
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(bo * T, S, 3 * Hh * D, generator=g).to(dtype).to(DEV)
    q, k, v = (t.contiguous() for t in qkv.chunk(3, dim=-1))
    first = ops.attention_temporal(q, k, v, Hh, T)
    assert torch.equal(first, ops.attention_temporal(q, k, v, Hh, T))
    assert torch.equal(first, ops.attention_temporal_packed(qkv, Hh, T))

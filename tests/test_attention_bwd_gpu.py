"""GPU parity of the differentiable attention (csrc/attn_bwd.hip through svd/ops.py's autograd Functions).

Parity chain: the reference's CrossAttention under fp64 autograd -> the fp64 formula of tests/attention_bwd_helpers.py
(tests/test_attention_bwd_cpu.py, 1e-12) -> the kernels (here). Bars: the project's small-tensor bars applied to the reference's OWN
error in the same 16-bit type (the same module run in bf16 / f16 on the CPU against its fp64 self, recorded by
tools/gen_golden_attention_bwd.py in the fixtures and in tests/golden/attention_bwd/ref_errors.json): rms <= 1.6 x, max norm <= 2.0 x.
dk and dv are each held to the reference's dcontext figure, relative to their own fp64 norm.
Every test runs with ops.STRICT = True: an attention that left the HIP path under autograd would raise."""
import os
import sys

import numpy as np
import pytest
import torch

import attention_bwd_helpers as A
import svd_helpers as H

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multiview_inpaint_amd", "dropin")
if DROPIN not in sys.path:
    sys.path.insert(0, DROPIN)

# The small-tensor bars of tests/test_unet_ops_gpu.py (SMALL_LATENT_BAR / SMALL_LATENT_MAX_BAR there; copied, not imported): the build's
# error as a multiple of the reference's own error in the same type, rms and max norm.
SMALL_LATENT_BAR = 1.6
SMALL_LATENT_MAX_BAR = 2.0
DEV = "cuda"


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    """MVI_STRICT for every test of this module (svd/ops.py), the HIP backward on whatever the environment says."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "ATTENTION_BACKWARD", True)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """ops.attention_backward_pays is a speed decision (small problems are left to PyTorch); the parity of the autograd route on the
    small fixtures is checked with the decision lifted, so that what is tested is what the kernels compute."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "ATTENTION_BACKWARD_MIN_SCORES", 0)


def _ops():
    from multiview_inpaint_amd.svd import hip_ops, ops
    return ops, hip_ops


def _check(name, got, ref, r_max, r_rms):
    e_max, e_rms = A.errors(got.detach().cpu(), ref)
    H.report(f"{name}: max {e_max:.2e} = {e_max / r_max:.2f} x, rms {e_rms:.2e} = {e_rms / r_rms:.2f} x the reference's own error")
    return e_max <= SMALL_LATENT_MAX_BAR * r_max and e_rms <= SMALL_LATENT_BAR * r_rms, (name, e_max, r_max, e_rms, r_rms)


def _assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


def _autograd(x, ctx, dy, heads):
    """ops.attention under autograd with q = x, k = v = context as separate leaves: (out, dq, dk, dv)."""
    ops, _ = _ops()
    q = x.to(DEV).requires_grad_()
    k = ctx.to(DEV).requires_grad_()
    v = ctx.to(DEV).clone().requires_grad_()
    out = ops.attention(q, k, v, heads)
    out.backward(dy.to(DEV))
    return out.detach(), q.grad, k.grad, v.grad


FIXTURES = [(case, tag) for case in A.TENSOR_CASES for tag in A.DTYPES]


@pytest.mark.parametrize("case,tag", FIXTURES, ids=[A.case_name(c, t) for c, t in FIXTURES])
def test_fixture_gradients_within_the_reference_own_error(case, tag, route_every_supported_shape):
    """ops.attention on the fixture's inputs under autograd: dq against the reference's dx, dk + dv against its dcontext, at 1.6 x
    (rms) / 2.0 x (max norm) of the reference's own error in that type stored in the fixture."""
    G = np.load(os.path.join(A.GOLDEN, A.case_name(case, tag) + ".npz"))
    dtype = A.DTYPES[tag]
    x, ctx, dy = (A.from_bits(G[n], dtype) for n in ("x", "context", "dy"))
    dx_max, dx_rms, dc_max, dc_rms = (float(e) for e in G["ref_err"])
    out, dq, dk, dv = _autograd(x, ctx, dy, case[1])
    _assert_all([_check(f"{A.case_name(case, tag)} dx", dq.float(), torch.from_numpy(G["dx"]), dx_max, dx_rms),
                 _check(f"{A.case_name(case, tag)} dcontext", dk.float() + dv.float(), torch.from_numpy(G["dcontext"]), dc_max, dc_rms)])


SHAPES = [(case, tag) for case in A.TRAINING_CASES + A.RAGGED_CASES for tag in A.DTYPES]


@pytest.mark.parametrize("case,tag", SHAPES, ids=[A.case_name(c, t) for c, t in SHAPES])
def test_training_and_ragged_shapes_against_the_fp64_formula(case, tag):
    """hip_ops.attention_forward_lse / attention_backward called directly (so a routing decision of ops.attention_backward_pays never
    removes a shape), dq, dk, dv separately against the fp64 formula evaluated on this machine's CPU. Bar: 1.6 x / 2.0 x the
    reference's own error of ref_errors.json — the entry of the same shape where there is one, else the largest of the type.
    Also for every shape: the forward that returns the row statistics is bit-identical to the inference forward, and two backward
    runs are bit-identical.
    Observed on the MI355X (rms / max multiples): training shapes 0.34 - 1.00 / 0.13 - 1.00, ragged shapes with their peaked row
    0.33 - 1.41 / 0.10 - 1.50; the largest are f16 (1, 2, 1300, 1300), dk rms 1.41 x and dq max 1.50 x — the 8-wave f16 forward rounds
    scale * log2 e into q a second time (attn_flash8m16.hip `kExact`), and the backward recomputes P from the same rounded q.
    """
    _, hip_ops = _ops()
    B, Hh, Sq, Sk = case
    dtype = A.DTYPES[tag]
    x, ctx, dy = A.make_inputs(case, dtype)
    _, fdq, fdk, fdv = A.formula(x, ctx, ctx, dy, Hh)
    q, k, v, d = x.to(DEV), ctx.to(DEV), ctx.to(DEV).clone(), dy.to(DEV)
    assert hip_ops.attention_backward_supported(Sq, Sk, A.D, dtype)
    out0 = hip_ops.attention(q, k, v, Hh)
    out, lse = hip_ops.attention_forward_lse(q, k, v, Hh)
    assert torch.equal(out0, out), "the forward under autograd must be the inference forward, bit for bit"
    dq, dk, dv = hip_ops.attention_backward(q, k, v, out, d, lse, Hh)
    dq2, dk2, dv2 = hip_ops.attention_backward(q, k, v, out, d, lse, Hh)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2), "two backward runs must match bit for bit"
    r = A.ref_error_for(case, tag)
    name = A.case_name(case, tag)
    _assert_all([_check(f"{name} dq", dq, fdq, r["dx_max"], r["dx_rms"]),
                 _check(f"{name} dk", dk, fdk, r["dcontext_max"], r["dcontext_rms"]),
                 _check(f"{name} dv", dv, fdv, r["dcontext_max"], r["dcontext_rms"])])


@pytest.mark.parametrize("tag", list(A.DTYPES))
def test_autograd_route_matches_the_direct_calls_and_skips_unneeded_kernels(tag, route_every_supported_shape):
    """ops.attention under autograd returns exactly what the direct calls return; inputs that need no gradient get None; with only
    k / v requiring grad dk and dv are the same bits as in the full run, and with only q requiring grad the dK/dV kernel is skipped."""
    ops, hip_ops = _ops()
    case = (2, 3, 1024, 300)
    dtype = A.DTYPES[tag]
    x, ctx, dy = A.make_inputs(case, dtype)
    out, dq, dk, dv = _autograd(x, ctx, dy, case[1])
    q, k, v, d = x.to(DEV), ctx.to(DEV), ctx.to(DEV).clone(), dy.to(DEV)
    o2, lse = hip_ops.attention_forward_lse(q, k, v, case[1])
    g = hip_ops.attention_backward(q, k, v, o2, d, lse, case[1])
    assert torch.equal(out, o2) and torch.equal(out, hip_ops.attention(q, k, v, case[1]))
    assert all(torch.equal(a, b) for a, b in zip((dq, dk, dv), g))
    # a non-contiguous upstream gradient
    qa = q.clone().requires_grad_()
    o = ops.attention(qa, k, v, case[1])
    (o.transpose(1, 2) * d.transpose(1, 2)).sum().backward()
    assert torch.equal(qa.grad, dq)
    # only k and v need grad
    ka, va = k.clone().requires_grad_(), v.clone().requires_grad_()
    ops.attention(q, ka, va, case[1]).backward(d)
    assert torch.equal(ka.grad, dk) and torch.equal(va.grad, dv)
    only_dq = hip_ops.attention_backward(q, k, v, o2, d, lse, case[1], need_dkv=False)
    assert only_dq[1] is None and only_dq[2] is None and torch.equal(only_dq[0], dq)


TEMPORAL = [(2, 14, 192, 5, 64), (1, 14, 3072, 5, 64), (3, 9, 50, 2, 32), (2, 16, 64, 4, 16)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("shape", TEMPORAL, ids=["x".join(map(str, s)) for s in TEMPORAL])
def test_temporal_backward_against_the_regrouped_fp64_formula(shape, dtype):
    """ops.attention_temporal under autograd, [(bo T), S, H D] as the spatial layers leave it. fp32 I/O: 1e-4 relative (the project's
    fp32 contract); bf16 / f16: 1.6 x / 2.0 x the largest reference error of the type in ref_errors.json (dq to the dx figure, dk and
    dv to the dcontext figure). Two runs are bit-identical."""
    ops, hip_ops = _ops()
    bo, T, S, Hh, D = shape
    g = torch.Generator().manual_seed(7 + S)
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
    name = "temporal " + "x".join(map(str, shape))
    if dtype == torch.float32:
        for n, got, ref in (("dq", qa.grad, rdq), ("dk", ka.grad, rdk), ("dv", va.grad, rdv)):
            e_max, e_rms = A.errors(got.cpu(), ref)
            H.report(f"{name} fp32 {n}: max {e_max:.2e}, rms {e_rms:.2e}")
            assert e_max <= 1e-4 and e_rms <= 1e-4, (n, e_max, e_rms)
        return
    tag = "bf16" if dtype == torch.bfloat16 else "f16"
    r = A.ref_error_for((0, 0, 0, 0), tag)                      # no entry of this shape: the largest of the type
    _assert_all([_check(f"{name} {tag} dq", qa.grad, rdq, r["dx_max"], r["dx_rms"]),
                 _check(f"{name} {tag} dk", ka.grad, rdk, r["dcontext_max"], r["dcontext_rms"]),
                 _check(f"{name} {tag} dv", va.grad, rdv, r["dcontext_max"], r["dcontext_rms"])])


def test_gate_edges():
    """hip_ops.attention_backward_supported is mvi_attention_backward_supported, a host-only C function: D = 64 yes, 32 no; Sk = 33
    yes, 32 no; fp32 no. Unsupported arguments to the C entry return the invalid-argument status (a Python Exception)."""
    _, hip_ops = _ops()
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    assert hip_ops.attention_backward_supported(192, 192, 64, bf) and hip_ops.attention_backward_supported(192, 192, 64, f16)
    assert not hip_ops.attention_backward_supported(192, 192, 32, bf)
    assert hip_ops.attention_backward_supported(192, 33, 64, bf) and not hip_ops.attention_backward_supported(192, 32, 64, bf)
    assert not hip_ops.attention_backward_supported(192, 192, 64, f32)
    q = torch.randn(1, 64, 2 * 32, device=DEV, dtype=bf)
    with pytest.raises(Exception, match="attention"):
        hip_ops.attention_forward_lse(q, q, q, 2)


def test_routing_and_strict_mode():
    """With STRICT on: a supported call under grad records the new kinds and does not raise; D = 32 under grad raises HipPathError;
    ATTENTION_BACKWARD = False raises as before this feature; under no_grad PROFILE shows the kinds it always showed."""
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    q = torch.randn(14, 768, 5 * 64, device=DEV, dtype=dt)      # 14 x 5 x 768 x 768 scores: above ops.ATTENTION_BACKWARD_MIN_SCORES
    assert ops.attention_backward_pays(14, 768, 768, 5, dt)
    hip_ops.PROFILE = []
    try:
        qa = q.clone().requires_grad_()
        ops.attention(qa, q, q, 5).sum().backward()
        assert [p[0] for p in hip_ops.PROFILE] == ["attention_mfma_lse", "attention_mfma_bwd"], hip_ops.PROFILE
        assert qa.grad is not None and qa.grad.shape == q.shape
        del hip_ops.PROFILE[:]
        with torch.no_grad():
            ops.attention(qa, q, q, 5)
            ops.attention_temporal(qa, q, q, 5, 14)
        ops.attention(q, q, q, 5)                               # grad mode on, nothing requires grad
        assert [p[0] for p in hip_ops.PROFILE] == ["attention_mfma", "attention_temporal", "attention_mfma"], hip_ops.PROFILE
    finally:
        hip_ops.PROFILE = None
    q32 = torch.randn(14, 768, 10 * 32, device=DEV, dtype=dt, requires_grad=True)
    with pytest.raises(ops.HipPathError):
        ops.attention(q32, q32, q32, 10)                         # D = 32: no HIP backward
    qf = torch.randn(14, 768, 5 * 64, device=DEV, requires_grad=True)
    with pytest.raises(ops.HipPathError):
        ops.attention(qf, qf, qf, 5)                             # fp32 I/O
    few = torch.randn(14, 32, 5 * 64, device=DEV, dtype=dt)
    with pytest.raises(ops.HipPathError):
        ops.attention(q.clone().requires_grad_(), few, few, 5)   # Sk = 32
    small = torch.randn(2, 192, 5 * 64, device=DEV, dtype=dt)    # supported, but below the speed line: PyTorch's path, so strict mode raises
    assert hip_ops.attention_backward_supported(192, 192, 64, dt) and not ops.attention_backward_pays(2, 192, 192, 5, dt)
    with pytest.raises(ops.HipPathError):
        ops.attention(small.clone().requires_grad_(), small, small, 5)
    ops.ATTENTION_BACKWARD = False                               # (restored by the module's fixture)
    with pytest.raises(ops.HipPathError):
        ops.attention(q.clone().requires_grad_(), q, q, 5)
    with pytest.raises(ops.HipPathError):
        ops.attention_temporal(q.clone().requires_grad_(), q, q, 5, 14)


def test_cross_attention_module_under_checkpoint_against_the_parent_route():
    """The package's CrossAttention (self-attention, 320 channels, 5 heads, S = 768, bf16) with x.requires_grad_() inside
    torch.utils.checkpoint.checkpoint(use_reentrant=False): input and weight gradients against the same module and weights on the CPU
    in fp64. Yardstick: the route before this feature — the same GPU call with ATTENTION_BACKWARD = False (strict mode lifted for that
    one run) — against the same fp64 result; the new route's error may be at most 1.6 x (rms) / 2.0 x (max) of it per gradient tensor,
    and FALLBACKS holds no attention entry for the new route's run."""
    from torch.utils.checkpoint import checkpoint
    from sgm.modules.attention import CrossAttention
    ops, hip_ops = _ops()
    torch.manual_seed(11)
    m64 = CrossAttention(query_dim=320, heads=5, dim_head=64).double()
    dt = torch.bfloat16
    with torch.no_grad():                                        # weights and inputs representable in bf16 on both sides
        for p in m64.parameters():
            p.copy_(p.to(dt).double())
    x = torch.randn(14, 768, 320).to(dt)                         # the reference's training batch: 14 frames (and a routed shape)
    dy = torch.randn(14, 768, 320).to(dt)
    x64 = x.double().requires_grad_()
    m64(x64).backward(dy.double())
    ref = {"x": x64.grad, **{n: p.grad for n, p in m64.named_parameters()}}

    def gpu_run():
        m = CrossAttention(query_dim=320, heads=5, dim_head=64)
        m.load_state_dict({k: v.float() for k, v in m64.state_dict().items()})
        m = m.to(DEV, dt)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        hip_ops.PROFILE = []
        try:
            checkpoint(m, xg, use_reentrant=False).backward(dy.to(DEV))
            kinds = [p[0] for p in hip_ops.PROFILE]
        finally:
            hip_ops.PROFILE = None
        return {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters()}}, kinds, list(ops.FALLBACKS)

    new, kinds, fallbacks = gpu_run()
    assert not [f for f in fallbacks if f[0].startswith("attention")], fallbacks
    # checkpoint runs the forward under grad, drops what it saved, and recomputes it inside the backward: the Function runs twice
    # (nothing outside ctx is cached), the backward kernels once, and the inference entry never
    assert kinds.count("attention_mfma_bwd") == 1 and kinds.count("attention_mfma_lse") in (1, 2) and "attention_mfma" not in kinds, kinds
    ops.STRICT, ops.ATTENTION_BACKWARD = False, False            # the parent's route (both restored by the module's fixture)
    old, old_kinds, old_fallbacks = gpu_run()
    ops.STRICT, ops.ATTENTION_BACKWARD = True, True
    assert ("attention", "requires grad") in old_fallbacks and "attention_mfma_bwd" not in old_kinds
    results = []
    for name, r in ref.items():
        o_max, o_rms = A.errors(old[name].cpu(), r)
        results.append(_check(f"CrossAttention 320/5 S=768 bf16 d{name} (against the PyTorch route's own error {o_max:.2e} / {o_rms:.2e})",
                              new[name], r, o_max, o_rms))
    _assert_all(results)

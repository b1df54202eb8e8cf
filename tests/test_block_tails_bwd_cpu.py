"""What the HIP backward of the block tails rests on, on the CPU: tests/block_tails_bwd_helpers.py's written-out gradients — the GPU
tests' oracle — are fp64 autograd's of the reference expressions; on CPU tensors the ops are the compositions they were, whatever the
switch says; and the speed decision routes nothing it has not been told."""
import pytest
import torch

import block_tails_bwd_helpers as B

TOL = 1e-12


def _alpha(n, g):
    a = torch.rand(n, generator=g, dtype=torch.float64)
    a[0] = 1.0
    if n > 1:
        a[1] = 0.0
    return a


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 5, 7), (4, 24, 16)], ids=lambda s: "x".join(map(str, s)))
def test_planes_formulas_against_fp64_autograd(shape, with_bias):
    N, C, S = shape
    g = torch.Generator().manual_seed(11)
    tok, base = (torch.randn(N, S, C, generator=g, dtype=torch.float64).requires_grad_() for _ in range(2))
    x_in = torch.randn(N, C, S, generator=g, dtype=torch.float64).requires_grad_()
    bias = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_() if with_bias else None
    alpha = _alpha(N, g).requires_grad_()
    dy = torch.randn(N, C, S, generator=g, dtype=torch.float64)
    # A
    B.planes_add_reference(tok, x_in, bias).backward(dy)
    f = B.planes_formulas(dy)
    assert (f["d_tok"] - tok.grad).abs().max().item() <= TOL
    assert (dy - x_in.grad).abs().max().item() <= TOL                    # d_x_in is dy itself
    if with_bias:
        assert (f["dbias"] - bias.grad).abs().max().item() <= TOL
        bias.grad = None
    tok.grad = None
    # B
    B.planes_blend_reference(tok, base, bias, alpha).backward(dy)
    f = B.planes_formulas(dy, alpha=alpha.detach(), tok=tok.detach(), bias=None if bias is None else bias.detach())
    assert (f["d_tok"] - tok.grad).abs().max().item() <= TOL
    assert (f["d_base"] - base.grad).abs().max().item() <= TOL
    assert (f["dalpha"] - alpha.grad).abs().max().item() <= TOL
    if with_bias:
        assert (f["dbias"] - bias.grad).abs().max().item() <= TOL
    # the kernel's one-sided form has the reference's value
    a = alpha.detach().reshape(N, 1, 1)
    t = tok.detach() if bias is None else tok.detach() + bias.detach()
    assert ((base.detach() + (1 - a) * t).transpose(1, 2) - B.planes_blend_reference(tok, base, bias, alpha).detach()).abs().max().item() <= TOL


@pytest.mark.parametrize("with_h", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 8), (3, 5, 4), (2, 7, 24)], ids=lambda s: "x".join(map(str, s)))
def test_rows_formulas_against_fp64_autograd(shape, with_h):
    G, row_div, C = shape
    g = torch.Generator().manual_seed(13)
    R = G * row_div
    x, base = (torch.randn(R, C, generator=g, dtype=torch.float64).requires_grad_() for _ in range(2))
    h = torch.randn(R, C, generator=g, dtype=torch.float64).requires_grad_() if with_h else None
    alpha = _alpha(G, g).requires_grad_()
    dy = torch.randn(R, C, generator=g, dtype=torch.float64)
    B.add_lerp_reference(x, h, base, alpha).backward(dy)
    f = B.rows_formulas(dy, alpha.detach(), x=x.detach(), h=None if h is None else h.detach(), base=base.detach())
    assert (f["d_t"] - x.grad).abs().max().item() <= TOL
    if with_h:
        assert (f["d_t"] - h.grad).abs().max().item() <= TOL             # one tensor for both
    assert (f["d_base"] - base.grad).abs().max().item() <= TOL
    assert (f["dalpha"] - alpha.grad).abs().max().item() <= TOL


def _run(fn, tensors, dy):
    leaves = [None if t is None else t.clone().requires_grad_() for t in tensors]
    y = fn(*leaves)
    y.backward(dy)
    return [y.detach()] + [l.grad for l in leaves if l is not None]


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_on_cpu_tensors_are_the_compositions(on, dtype, monkeypatch):
    """Switch off (and on: a CPU tensor never leaves PyTorch): output and gradients of tokens_to_planes_add, add_lerp,
    tokens_blend_to_planes and planes_to_tokens under autograd are bit-equal to the compositions written out here — for the first two
    the code ops ran before the switch existed."""
    from multiview_inpaint_amd.svd import ops
    monkeypatch.setattr(ops, "BLOCK_TAILS_BACKWARD", on)
    monkeypatch.setattr(ops, "block_tails_backward_pays", lambda *a: True)
    g = torch.Generator().manual_seed(3)
    N, C, H, W = 3, 16, 4, 6
    S = H * W
    tok, base = (torch.randn(N, S, C, generator=g).to(dtype) for _ in range(2))
    x_in = torch.randn(N, C, H, W, generator=g).to(dtype)
    bias = torch.randn(C, generator=g).to(dtype)
    alpha = torch.rand(N, generator=g)
    dy = torch.randn(N, C, H, W, generator=g).to(dtype)

    def add_today(tok, x_in, bias):
        t = tok if bias is None else tok + bias.to(tok.dtype)
        return t.transpose(1, 2).reshape(x_in.shape) + x_in
    for b in (bias, None):
        for got, ref in zip(_run(ops.tokens_to_planes_add, (tok, x_in, b), dy), _run(add_today, (tok, x_in, b), dy)):
            assert torch.equal(got, ref)

    def blend_composition(tok, base, bias, alpha):
        t = tok if bias is None else tok + bias.to(tok.dtype)
        return torch.lerp(base + t, base, alpha.reshape(N, 1, 1).to(tok.dtype)).transpose(1, 2).reshape(N, C, H, W)
    for b in (bias, None):
        got = _run(lambda t, ba, bi, a: ops.tokens_blend_to_planes(t, ba, bi, a, (H, W)), (tok, base, b, alpha), dy)
        for g_, r_ in zip(got, _run(blend_composition, (tok, base, b, alpha), dy)):
            assert torch.equal(g_, r_)

    def lerp_today(x, h, base, alpha):
        t = x if h is None else x + h
        C_ = x.shape[-1]
        G = alpha.numel()
        return torch.lerp(t.reshape(G, -1, C_), base.reshape(G, -1, C_), alpha.reshape(G, 1, 1).to(x.dtype)).reshape(x.shape)
    a_rows = torch.rand(N, generator=g).to(dtype)
    dyr = torch.randn(N, S, C, generator=g).to(dtype)
    for h in (base, None):
        for got, ref in zip(_run(ops.add_lerp, (tok, h, x_in.reshape(N, S, C), a_rows), dyr), _run(lerp_today, (tok, h, x_in.reshape(N, S, C), a_rows), dyr)):
            assert torch.equal(got, ref)

    for got, ref in zip(_run(ops.planes_to_tokens, (x_in,), dyr), _run(lambda x: x.flatten(2).transpose(1, 2).contiguous(), (x_in,), dyr)):
        assert torch.equal(got, ref)


def test_speed_decision_routes_only_what_the_table_lists(monkeypatch):
    from multiview_inpaint_amd.svd import ops
    bf = torch.bfloat16
    assert ops.block_tails_backward_pays("planes_add", 28, 328, 9216, bf, True) is False          # a class nobody measured
    assert ops.block_tails_backward_pays("no_such_tail", 28, 320, 9216, bf, True) is False
    for key, lo in ops.BLOCK_TAILS_BACKWARD_ROUTED.items():
        kind, C, S, need = key
        assert kind in ("planes_add", "planes_blend", "add_lerp", "to_tokens") and type(need) is bool
        assert ops.block_tails_backward_pays(kind, lo, C, S, bf, need) is True
        assert ops.block_tails_backward_pays(kind, lo - 1, C, S, bf, need) is False
    monkeypatch.setattr(ops, "BLOCK_TAILS_BACKWARD_ROUTED", {("add_lerp", 320, 9216, True): 14 * 9216})
    assert ops.block_tails_backward_pays("add_lerp", 14 * 9216, 320, 9216, bf, True) is True
    assert ops.block_tails_backward_pays("add_lerp", 14 * 9216, 320, 9216, bf, False) is False
    assert ops.block_tails_backward_pays("add_lerp", 7 * 9216, 320, 9216, bf, True) is False


def test_the_switch_is_off_by_default():
    import os
    from multiview_inpaint_amd.svd import ops
    if os.environ.get("MVI_BLOCK_TAILS_BWD") is None:
        assert ops.BLOCK_TAILS_BACKWARD is False
    x = torch.randn(2, 8, 2, 4).requires_grad_()
    assert not ops.planes_to_tokens_routed(x) and not ops.tokens_to_planes_add_routed(x.flatten(2).transpose(1, 2), x, None)

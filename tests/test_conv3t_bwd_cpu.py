"""What the HIP backward of the (3, 1, 1) frame convolution rests on, in fp64 on the CPU (no GPU, no library): the input gradient is
the same convolution of dy with hip_ops.conv3t_transposed_weight(w), tests/conv3t_bwd_helpers.py's written-out weight gradient — the
GPU tests' oracle — is autograd's, and ops.conv3t_tokens on CPU tensors is F.conv3d with autograd's gradients."""
import pytest
import torch
import torch.nn.functional as F

import conv3t_bwd_helpers as B

SHAPES = [(2, 3, 5, 4, 6), (1, 1, 7, 3, 2), (2, 2, 1, 2, 2)]          # (B, T, S, C_in, C_out)
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _case(shape):
    Bv, T, S, Ci, Co = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(Bv * T, S, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 1, 1, generator=g, dtype=torch.float64)
    dy = torch.randn(Bv * T, S, Co, generator=g, dtype=torch.float64)
    return x, w, dy


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dgrad_identity_and_wgrad_formula_against_fp64_autograd(shape):
    from multiview_inpaint_amd.svd import hip_ops                 # pure torch up to here: importing the module loads no library
    Bv, T, S, Ci, Co = shape
    x, w, dy = _case(shape)
    dx, dw = B.autograd_grads(x, w, dy, T)
    wt = hip_ops.conv3t_transposed_weight(w)
    assert tuple(wt.shape) == (Ci, Co, 3, 1, 1)
    for kt in range(3):
        assert torch.equal(wt[:, :, kt, 0, 0], w[:, :, 2 - kt, 0, 0].t())
    assert (B.dgrad_formula(dy, w, T) - dx).abs().max().item() <= 1e-12
    assert (B.wgrad_formula(x, dy, T) - dw).abs().max().item() <= 1e-12
    # the layout helpers are inverses
    assert torch.equal(B.tokens(B.video(x, T)), x)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conv3t_tokens_on_the_cpu_is_conv3d_with_autograd_gradients(shape):
    from multiview_inpaint_amd.svd import hip_ops, ops
    Bv, T, S, Ci, Co = shape
    x, w, dy = _case(shape)
    ref = B.tokens(F.conv3d(B.video(x, T), w, padding=(1, 0, 0)))
    y = ops.conv3t_tokens(x, w, T)
    assert tuple(y.shape) == (Bv * T, S, Co) and y.dtype == torch.float64
    assert (y - ref).abs().max().item() <= 1e-12
    dx, dw = B.autograd_grads(x, w, dy, T)
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    ops.conv3t_tokens(xa, wa, T).backward(dy)
    assert (xa.grad - dx).abs().max().item() <= 1e-12
    assert (wa.grad - dw).abs().max().item() <= 1e-12
    # the packed transposed weight of the input gradient, index by index: row ci, column kt C_out + co holds W[co, ci, 2 - kt]
    packed = hip_ops.conv3t_n320_weight(hip_ops.conv3t_transposed_weight(w))
    hand = torch.empty(Ci, 3 * Co, dtype=w.dtype)
    for ci in range(Ci):
        for kt in range(3):
            for co in range(Co):
                hand[ci, kt * Co + co] = w[co, ci, 2 - kt, 0, 0]
    assert packed.is_contiguous() and torch.equal(packed, hand)

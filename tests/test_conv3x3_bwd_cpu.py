"""The two identities the HIP backward of the 3x3 convolution rests on, in fp64 on the CPU (no GPU, no library): the input gradient is
the same convolution of dy with hip_ops.conv3x3_transposed_weight(w), and tests/conv_bwd_helpers.py's written-out weight gradient —
the GPU tests' oracle — is autograd's."""
import pytest
import torch
import torch.nn.functional as F

import conv_bwd_helpers as B

SHAPES = [(2, 5, 7, 6, 4), (1, 1, 1, 3, 5), (3, 1, 9, 4, 4), (1, 33, 5, 2, 3)]          # (N, H, W, C_in, C_out)


def _transposed_weight():
    """hip_ops.conv3x3_transposed_weight: pure torch; importing the module loads no library."""
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops.conv3x3_transposed_weight


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_dgrad_identity_and_wgrad_formula_against_fp64_autograd(shape):
    N, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(N, Co, H, W, generator=g, dtype=torch.float64)
    dx, dw = B.autograd_grads(x, w, dy)
    wt = _transposed_weight()(w)
    assert tuple(wt.shape) == (Ci, Co, 3, 3)
    assert (F.conv2d(dy, wt, padding=1) - dx).abs().max().item() <= 1e-12
    assert (B.dgrad_formula(dy, w) - dx).abs().max().item() <= 1e-12
    assert (B.wgrad_formula(x, dy) - dw).abs().max().item() <= 1e-12
    # the token-major helpers are inverses
    assert torch.equal(B.planes(B.tokens(x), H, W), x)

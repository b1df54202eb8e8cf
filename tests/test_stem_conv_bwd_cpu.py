"""The fp64 formulas of tests/stem_bwd_helpers.py (the oracle of the GPU tests of the hint stem's backward) against fp64 autograd, and
hip_ops.stem_conv3x3_transposed_weight. No GPU, no library."""
import pytest
import torch
import torch.nn.functional as F

import stem_bwd_helpers as B

TOL = 1e-12
# (N, C_in, H, W) into C_out output channels
CASES = [((2, 5, 5, 8), 4, 1), ((1, 3, 1, 1), 5, 1), ((3, 4, 9, 6), 4, 1),
         ((2, 5, 7, 10), 5, 2), ((1, 3, 1, 2), 4, 2), ((1, 4, 8, 8), 5, 2)]


def _case(shape, Co, stride, seed):
    N, Ci, H, W = shape
    x, w, b, dy = B.make_case((N, Ci, Co, H, W), stride, torch.float64, seed)
    return x, w, b, dy


def _close(a, b):
    return (a - b).abs().max().item() <= TOL * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("shape,Co,stride", CASES)
def test_formulas_against_fp64_autograd(shape, Co, stride, silu):
    x, w, b, dy = _case(shape, Co, stride, seed=11 + sum(shape) + stride)
    dx, dw, db = B.autograd_grads(x, w, b, dy, stride, silu)
    dz = B.dz_formula(x, w, b, dy, stride, silu)
    assert _close(B.wgrad_formula(x, dz, stride), dw)
    assert _close(B.dbias_formula(dz), db)
    if stride == 1:
        assert _close(B.dgrad_formula(dz, w), dx)
    else:
        assert _close(torch.nn.grad.conv2d_input(x.shape, w, dz, stride=2, padding=1), dx)
    # without a bias: the same dz rule on z = conv(x)
    dx0, dw0, db0 = B.autograd_grads(x, w, None, dy, stride, silu)
    assert db0 is None and _close(B.wgrad_formula(x, B.dz_formula(x, w, None, dy, stride, silu), stride), dw0)


@pytest.mark.parametrize("shape,Co,stride", [c for c in CASES if c[2] == 1])
def test_transposed_weight_gives_the_input_gradient(shape, Co, stride):
    from multiview_inpaint_amd.svd import hip_ops
    x, w, b, dy = _case(shape, Co, 1, seed=5 + sum(shape))
    dx, _, _ = B.autograd_grads(x, w, b, dy, 1, True)
    dz = B.dz_formula(x, w, b, dy, 1, True)
    wt = hip_ops.stem_conv3x3_transposed_weight(w)
    assert tuple(wt.shape) == (w.shape[1], w.shape[0], 3, 3)
    assert _close(F.conv2d(dz, wt, padding=1), dx)

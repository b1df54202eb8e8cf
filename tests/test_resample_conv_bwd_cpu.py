"""The identities the HIP backward of the two resampling 3x3 convolutions rests on, in fp64 on the CPU (no GPU, no library):
tests/resample_bwd_helpers.py's written-out gradients — the GPU tests' oracle — are autograd's, and ops.conv3x3_down_tokens /
ops.conv3x3_up_tokens on CPU tensors are F.conv2d (F.interpolate + F.conv2d) with the same gradients."""
import pytest
import torch
import torch.nn.functional as F

import resample_bwd_helpers as R

SHAPES = [(1, 2, 2, 3, 4), (2, 6, 10, 5, 7), (3, 4, 8, 6, 2)]          # (N, H, W, C_in, C_out): H x W the stride-2 input / the upsampled image
TOL = 1e-12


def _id(s):
    return "x".join(map(str, s))


def _rand(shape, seed, *sizes):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return [torch.randn(*s, generator=g, dtype=torch.float64) for s in sizes]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_s2_formulas_against_fp64_autograd(shape):
    N, H, W, Ci, Co = shape
    x, w, b, dy = _rand(shape, 5, (N, Ci, H, W), (Co, Ci, 3, 3), (Co,), (N, Co, H // 2, W // 2))
    dx, dw, db = R.autograd_grads_s2(x, w, b, dy)
    assert (R.s2_dgrad_formula(dy, w, H, W) - dx).abs().max().item() <= TOL
    assert (R.s2_wgrad_formula(x, dy) - dw).abs().max().item() <= TOL
    assert (dy.sum(dim=(0, 2, 3)) - db).abs().max().item() <= TOL
    if H == 2 and W == 2:                                        # one output pixel at (0, 0): taps ky = 0 and kx = 0 read the padding only
        assert not R.s2_wgrad_formula(x, dy)[:, :, 0, :].any() and not R.s2_wgrad_formula(x, dy)[:, :, :, 0].any()


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_up_dgrad_formula_against_fp64_autograd(shape):
    N, H, W, Ci, Co = shape                                      # the source is (H / 2) x (W / 2)
    x, w, dy = _rand(shape, 9, (N, Ci, H // 2, W // 2), (Co, Ci, 3, 3), (N, Co, H, W))
    dx = R.autograd_grads_up(x, w, dy)
    got = R.up_dgrad_formula(dy, w)
    assert got.shape == x.shape and (got - dx).abs().max().item() <= TOL


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_ops_on_cpu_tensors_are_the_pytorch_path(shape):
    from multiview_inpaint_amd.svd import ops
    N, H, W, Ci, Co = shape
    x, w, b, dy = _rand(shape, 13, (N, Ci, H, W), (Co, Ci, 3, 3), (Co,), (N, Co, H // 2, W // 2))
    before = list(ops.FALLBACKS)
    tok, wa, ba = R.tokens(x).requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = ops.conv3x3_down_tokens(tok, wa, ba, H, W)
    assert tuple(y.shape) == (N, (H // 2) * (W // 2), Co)
    assert (R.planes(y, H // 2, W // 2) - F.conv2d(x, w, b, stride=2, padding=1)).abs().max().item() <= TOL
    y.backward(R.tokens(dy))
    dx, dw, db = R.autograd_grads_s2(x, w, b, dy)
    assert (R.planes(tok.grad, H, W) - dx).abs().max().item() <= TOL
    assert (wa.grad - dw).abs().max().item() <= TOL and (ba.grad - db).abs().max().item() <= TOL
    assert (ops.conv3x3_down_tokens(R.tokens(x), w, None, H, W) - R.tokens(F.conv2d(x, w, None, stride=2, padding=1))).abs().max().item() <= TOL

    h, w_ = H // 2, W // 2
    xs, dyu = _rand(shape, 17, (N, Ci, h, w_), (N, Co, H, W))
    tok = R.tokens(xs).requires_grad_()
    y = ops.conv3x3_up_tokens(tok, w, b, h, w_)
    assert tuple(y.shape) == (N, H * W, Co)
    ref = F.conv2d(F.interpolate(xs, scale_factor=2, mode="nearest"), w, b, padding=1)
    assert (R.planes(y, H, W) - ref).abs().max().item() <= TOL
    y.backward(R.tokens(dyu))
    assert (R.planes(tok.grad, h, w_) - R.autograd_grads_up(xs, w, dyu)).abs().max().item() <= TOL
    assert ops.FALLBACKS == before, "a CPU tensor's PyTorch path is not a recorded fallback"
    with pytest.raises(ValueError):
        ops.conv3x3_down_tokens(R.tokens(x), w, None, H, W + 2)
    with pytest.raises(ValueError):
        ops.conv3x3_up_tokens(R.tokens(xs), w, None, h + 1, w_)

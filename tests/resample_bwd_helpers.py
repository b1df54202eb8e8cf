"""The written-out fp64 backward of the two resampling 3x3 convolutions — stride 2 / padding 1 (Downsample.op) and the convolution of the
nearest-neighbour 2x upsampled image (Upsample.conv): the oracle of tests/test_resample_conv_bwd_gpu.py, itself held to fp64 autograd in
tests/test_resample_conv_bwd_cpu.py. Pure torch on the CPU; nothing outside the repository is read."""
import torch
import torch.nn.functional as F

from conv_bwd_helpers import DTYPES, dgrad_formula, errors, planes, tokens, wgrad_formula  # noqa: F401  (re-exported for the tests)


def zero_stuffed(dy, H, W):
    """dy [N, C, H / 2, W / 2] -> z [N, C, H, W] with z[2 r, 2 c] = dy[r, c] and 0 elsewhere (H, W even)."""
    z = dy.new_zeros(dy.shape[0], dy.shape[1], H, W)
    z[:, :, ::2, ::2] = dy
    return z


def s2_dgrad_formula(dy, w, H, W):
    """dx [N, C_in, H, W] of conv2d(x, w, stride=2, padding=1) from dy [N, C_out, H / 2, W / 2]: the stride-1 convolution of the zero-stuffed
    dy with W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx], in fp64."""
    return dgrad_formula(zero_stuffed(dy.double(), H, W), w)


def s2_wgrad_formula(x, dy):
    """dweight[co, ci, ky, kx] = sum over (n, u, v) of z[n, co, u, v] * x[n, ci, u + ky - 1, v + kx - 1] with z the zero-stuffed dy: the
    stride-1 formula with z in place of dy. x [N, C_in, H, W], dy [N, C_out, H / 2, W / 2] -> [C_out, C_in, 3, 3], in fp64."""
    return wgrad_formula(x, zero_stuffed(dy.double(), x.shape[2], x.shape[3]))


def up_dgrad_formula(dy, w):
    """dx [N, C_in, h, w] of conv2d(interpolate(x, 2, nearest), w, padding=1) from dy [N, C_out, 2 h, 2 w]: the stride-1 input gradient at
    2 h x 2 w summed over every 2x2 cell, in fp64."""
    g = dgrad_formula(dy, w)
    N, C, H2, W2 = g.shape
    return g.reshape(N, C, H2 // 2, 2, W2 // 2, 2).sum(dim=(3, 5))


def autograd_grads_s2(x, w, b, dy):
    """(dx, dweight, dbias) of F.conv2d(x, w, b, stride=2, padding=1) under fp64 autograd."""
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    F.conv2d(x64, w64, b64, stride=2, padding=1).backward(dy.double())
    return x64.grad, w64.grad, b64.grad


def autograd_grads_up(x, w, dy):
    """dx of F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) under fp64 autograd."""
    x64 = x.double().requires_grad_()
    F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), w.double(), padding=1).backward(dy.double())
    return x64.grad


def make_s2(shape, dtype, seed, w_std=None):
    """shape (N, H, W, C_in, C_out) of the module: x [N, H W, C_in], dy [N, (H / 2)(W / 2), C_out] ~ N(0, 1), w [C_out, C_in, 3, 3] ~
    N(0, w_std^2) (default 1 / (9 C_out)) and b [C_out] ~ N(0, 0.01), rounded to dtype."""
    N, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H * W, Ci, generator=g).to(dtype)
    dy = torch.randn(N, (H // 2) * (W // 2), Co, generator=g).to(dtype)
    std = (1.0 / (9 * Co)) ** 0.5 if w_std is None else w_std
    w = (std * torch.randn(Co, Ci, 3, 3, generator=g)).to(dtype)
    b = (0.1 * torch.randn(Co, generator=g)).to(dtype)
    return x, dy, w, b


def make_up(shape, dtype, seed):
    """shape (N, h, w, C_in, C_out) of the module (h x w: the source): x [N, h w, C_in], dy [N, (2 h)(2 w), C_out], w, b as make_s2."""
    N, h, w_, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, h * w_, Ci, generator=g).to(dtype)
    dy = torch.randn(N, 4 * h * w_, Co, generator=g).to(dtype)
    w = ((1.0 / (9 * Co)) ** 0.5 * torch.randn(Co, Ci, 3, 3, generator=g)).to(dtype)
    b = (0.1 * torch.randn(Co, generator=g)).to(dtype)
    return x, dy, w, b

"""The written-out fp64 backward of the 3x3 / padding 1 / stride 1 convolution: the oracle of tests/test_conv3x3_bwd_gpu.py, itself held
to fp64 autograd in tests/test_conv3x3_bwd_cpu.py. Pure torch on the CPU; nothing outside the repository is read."""
import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def wgrad_formula(x, dy):
    """dweight[co, ci, ky, kx] = sum over (n, y, x) of dy[n, co, y, x] * x[n, ci, y + ky - 1, x + kx - 1], pixels outside the image 0.
    x [N, C_in, H, W], dy [N, C_out, H, W] -> [C_out, C_in, 3, 3], in fp64."""
    x, dy = x.double(), dy.double()
    H, W = x.shape[2], x.shape[3]
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.empty(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", dy, xp[:, :, ky:ky + H, kx:kx + W])
    return dw


def dgrad_formula(dy, w):
    """dx of conv2d(x, w, padding=1) from dy: the same convolution of dy with W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx], in fp64."""
    return F.conv2d(dy.double(), w.double().flip(2, 3).transpose(0, 1), padding=1)


def autograd_grads(x, w, dy):
    """(dx, dweight) of F.conv2d(x, w, padding=1) under fp64 autograd."""
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    F.conv2d(x64, w64, padding=1).backward(dy.double())
    return x64.grad, w64.grad


def planes(tok, H, W):
    """token-major [N, H W, C] -> [N, C, H, W]"""
    N, S, C = tok.shape
    return tok.reshape(N, H, W, C).permute(0, 3, 1, 2)


def tokens(x):
    """[N, C, H, W] -> token-major [N, H W, C], contiguous"""
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N, H * W, C).contiguous()


def make_tokens(shape, dtype, seed, w_std=None):
    """x [N, H W, C_in], dy [N, H W, C_out] ~ N(0, 1) and w [C_out, C_in, 3, 3] ~ N(0, w_std^2) (default 1 / (9 C_out)), rounded to dtype."""
    N, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H * W, Ci, generator=g).to(dtype)
    dy = torch.randn(N, H * W, Co, generator=g).to(dtype)
    std = (1.0 / (9 * Co)) ** 0.5 if w_std is None else w_std
    w = (std * torch.randn(Co, Ci, 3, 3, generator=g)).to(dtype)
    return x, dy, w


def errors(got, ref):
    """(max-norm, rms) error of got against ref, relative to ref's own max / rms."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()

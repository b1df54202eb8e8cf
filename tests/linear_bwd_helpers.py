"""The written-out fp64 backward of a projection y = x W^T + b: the oracle of tests/test_linear_bwd_gpu.py, itself held to fp64
autograd in tests/test_linear_bwd_cpu.py. Pure torch on the CPU; nothing outside the repository is read."""
import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def dx_formula(dy, w):
    """dx[r, k] = sum over n of dy[r, n] * w[n, k]: dy [rows, N], w [N, K] -> [rows, K], in fp64."""
    return dy.double() @ w.double()


def dweight_formula(x, dy):
    """dweight[n, k] = sum over r of dy[r, n] * x[r, k]: x [rows, K], dy [rows, N] -> [N, K], in fp64."""
    return dy.double().t() @ x.double()


def dbias_formula(dy):
    """dbias[n] = sum over r of dy[r, n], in fp64."""
    return dy.double().sum(0)


def autograd_grads(x, w, b, dy):
    """(dx, dweight, dbias) of F.linear(x, w, b) under fp64 autograd."""
    x64, w64, b64 = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    F.linear(x64, w64, b64).backward(dy.double())
    return x64.grad, w64.grad, b64.grad


def make_rows(rows, K, N, dtype, seed, strided=False):
    """x [rows, K], dy [rows, N] ~ N(0, 1), w [N, K] ~ N(0, 1 / K), b [N] ~ N(0, 0.09), rounded to dtype. strided: x is the first K
    columns of a [rows, K + 64] matrix and dy the middle third of a [rows, 3 N] one (the packed q | k | v layout) — views, same values
    as the contiguous case of the same seed would not be; the caller compares against the views' own values."""
    g = torch.Generator().manual_seed(seed)
    if strided:
        x = torch.randn(rows, K + 64, generator=g).to(dtype)[:, :K]
        dy = torch.randn(rows, 3 * N, generator=g).to(dtype)[:, N:2 * N]
    else:
        x = torch.randn(rows, K, generator=g).to(dtype)
        dy = torch.randn(rows, N, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    b = (torch.randn(N, generator=g) * 0.3).to(dtype)
    return x, dy, w, b


def wgrad_caps(x, dy):
    """The elementwise caps of an fp32-accumulated weight / bias gradient of exactly representable products: any summation order of
    `rows` terms errs by at most rows 2^-24 sum|terms|; doubled for the matrix pipe's internal accumulation (the bound of
    tests/test_conv3x3_bwd_gpu.py). (cap of dweight [N, K], cap of dbias [N])"""
    rows = x.shape[0]
    u = 2.0 * rows * 2.0 ** -24
    return u * dweight_formula(x.abs(), dy.abs()), u * dy.double().abs().sum(0)


def errors(got, ref):
    """(max-norm, rms) error of got against ref, relative to ref's own max / rms."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()

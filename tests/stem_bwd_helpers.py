"""The written-out fp64 backward of the hint-stem layers act(conv2d(x, w, b, stride, padding=1)), act = SiLU or nothing, stride 1 or 2:
the oracle of tests/test_stem_conv_bwd_gpu.py, itself held to fp64 autograd in tests/test_stem_conv_bwd_cpu.py. Pure torch on the CPU;
nothing outside the repository is read."""
import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def dz_formula(x, w, b, dy, stride=1, silu=True):
    """dz = dy * silu'(z), z = conv2d(x, w, b, stride, padding=1), silu'(z) = s (1 + z (1 - s)), s = sigmoid(z); without SiLU dz = dy. fp64."""
    dy = dy.double()
    if not silu:
        return dy.clone()
    z = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride, 1)
    s = torch.sigmoid(z)
    return dy * s * (1 + z * (1 - s))


def wgrad_formula(x, dz, stride=1):
    """dweight[co, ci, ky, kx] = sum over (n, oy, ox) of dz[n, co, oy, ox] * x[n, ci, s oy + ky - 1, s ox + kx - 1], pixels outside the
    image 0. x [N, C_in, H, W], dz [N, C_out, H_o, W_o] -> [C_out, C_in, 3, 3], in fp64."""
    x, dz = x.double(), dz.double()
    Ho, Wo = dz.shape[2], dz.shape[3]
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.empty(dz.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            dw[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", dz, win)
    return dw


def dbias_formula(dz):
    return dz.double().sum(dim=(0, 2, 3))


def dgrad_formula(dz, w):
    """dx of the stride-1 conv2d(x, w, padding=1) from dz: the same convolution of dz with W'[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx]."""
    return F.conv2d(dz.double(), w.double().flip(2, 3).transpose(0, 1), padding=1)


def autograd_grads(x, w, b, dy, stride=1, silu=True):
    """(dx, dweight, dbias) of act(conv2d(x, w, b, stride, padding=1)) under fp64 autograd (dbias None without a bias)."""
    x64, w64 = x.detach().double().clone().requires_grad_(), w.detach().double().clone().requires_grad_()
    b64 = None if b is None else b.detach().double().clone().requires_grad_()
    z = F.conv2d(x64, w64, b64, stride, 1)
    (F.silu(z) if silu else z).backward(dy.double())
    return x64.grad, w64.grad, None if b64 is None else b64.grad


def make_case(shape, stride, dtype, seed, bias=True):
    """shape (N, C_in, C_out, H, W): x, dy ~ N(0, 1), w ~ N(0, 1 / (9 C_in)), b ~ 0.3 N(0, 1) (the forward test's scales), rounded to dtype."""
    N, Ci, Co, H, W = shape
    Ho, Wo = out_size(H, W, stride)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, H, W, generator=g).to(dtype)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5).to(dtype)
    b = (torch.randn(Co, generator=g) * 0.3).to(dtype) if bias else None
    dy = torch.randn(N, Co, Ho, Wo, generator=g).to(dtype)
    return x, w, b, dy


def errors(got, ref):
    """(max-norm, rms) error of got against ref, relative to ref's own max / rms."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()

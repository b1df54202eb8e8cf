"""The written-out fp64 backward of the (3, 1, 1) / padding (1, 0, 0) frame convolution on token-major activations: the oracle of
tests/test_conv3t_bwd_gpu.py, itself held to fp64 autograd of F.conv3d in tests/test_conv3t_bwd_cpu.py. Pure torch on the CPU; nothing
outside the repository is read. Activations are [(b T), S, C] with the T frames of a video consecutive, weights [C_out, C_in, 3, 1, 1]."""
import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def video(tok, T):
    """token-major [(b T), S, C] -> b c t s 1, the layout F.conv3d takes (a view)"""
    BT, S, C = tok.shape
    return tok.reshape(BT // T, T, S, C).permute(0, 3, 1, 2).unsqueeze(-1)


def tokens(x5):
    """b c t s 1 -> token-major [(b T), S, C], contiguous"""
    B, C, T, S, _ = x5.shape
    return x5.squeeze(-1).permute(0, 2, 3, 1).reshape(B * T, S, C).contiguous()


def wgrad_formula(x, dy, T):
    """dweight[co, ci, kt] = sum over (b, t, p) of dy[b, t, p, co] * x[b, t + kt - 1, p, ci], frames outside [0, T) 0.
    x [(b T), S, C_in], dy [(b T), S, C_out] -> [C_out, C_in, 3, 1, 1], in fp64."""
    x, dy = x.double(), dy.double()
    BT, S, Ci = x.shape
    xv = F.pad(x.reshape(BT // T, T, S, Ci), (0, 0, 0, 0, 1, 1))                # one zero frame in front of and behind every video
    dv = dy.reshape(BT // T, T, S, dy.shape[2])
    dw = torch.empty(dy.shape[2], Ci, 3, 1, 1, dtype=torch.float64)
    for kt in range(3):
        dw[:, :, kt, 0, 0] = torch.einsum("btpo,btpi->oi", dv, xv[:, kt:kt + T])
    return dw


def dgrad_formula(dy, w, T):
    """dx [(b T), S, C_in] of the frame convolution from dy [(b T), S, C_out]: the same convolution of dy with
    hip_ops.conv3t_transposed_weight(w) (W'[ci, co, kt] = W[co, ci, 2 - kt]), in fp64."""
    from multiview_inpaint_amd.svd import hip_ops
    return tokens(F.conv3d(video(dy.double(), T), hip_ops.conv3t_transposed_weight(w.double()), padding=(1, 0, 0)))


def autograd_grads(x, w, dy, T):
    """(dx, dweight) of F.conv3d(video(x), w, padding=(1, 0, 0)) under fp64 autograd, dx token-major."""
    x64, w64 = x.detach().double().clone().requires_grad_(), w.detach().double().clone().requires_grad_()     # (never the caller's own tensors)
    F.conv3d(video(x64, T), w64, padding=(1, 0, 0)).backward(video(dy.double(), T))
    return x64.grad, w64.grad


def make_tokens(shape, dtype, seed):
    """x [(B T), S, C_in], dy [(B T), S, C_out] ~ N(0, 1) and w [C_out, C_in, 3, 1, 1] ~ N(0, 1 / (3 C_out)), rounded to dtype."""
    B, T, S, Ci, Co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, S, Ci, generator=g).to(dtype)
    dy = torch.randn(B * T, S, Co, generator=g).to(dtype)
    w = ((3 * Co) ** -0.5 * torch.randn(Co, Ci, 3, 1, 1, generator=g)).to(dtype)
    return x, dy, w


def errors(got, ref):
    """(max-norm, rms) error of got against ref, relative to ref's own max / rms."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()

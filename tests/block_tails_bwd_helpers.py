"""The written-out fp64 backward of the block tails (tokens_to_planes_add, tokens_blend_to_planes, add_lerp): the oracle of
tests/test_block_tails_bwd_gpu.py, itself held to fp64 autograd of the reference expressions in tests/test_block_tails_bwd_cpu.py.
Pure torch on the CPU; nothing outside the repository is read. dy is the incoming gradient.

  A  out[n, c, p] = tok[n, p, c] + bias[c] + x_in[n, c, p]
  B  out[n, c, p] = base[n, p, c] + (1 - a_n)(tok[n, p, c] + bias[c])   (= a x_spatial + (1 - a)(x_spatial + h + b) of the reference)
  C  t = x + h (rounded to the storage type by the kernels), out = lerp(t, base, a_g), g = r / row_div
"""
import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


# ---- the reference expressions (what fp64 autograd differentiates) ---------------------------------------------------------------
def planes_add_reference(tok, x_in, bias):
    t = tok if bias is None else tok + bias
    out = t.transpose(1, 2)
    return out if x_in is None else out + x_in.reshape(out.shape)


def planes_blend_reference(tok, base, bias, alpha):
    a = alpha.reshape(-1, 1, 1)
    t = tok if bias is None else tok + bias
    return (a * base + (1 - a) * (base + t)).transpose(1, 2)


def add_lerp_reference(x, h, base, alpha):
    """x, h, base [R, C]; alpha [G]."""
    G = alpha.numel()
    t = x if h is None else x + h
    C = x.shape[-1]
    return torch.lerp(t.reshape(G, -1, C), base.reshape(G, -1, C), alpha.reshape(G, 1, 1)).reshape(x.shape)


# ---- the formulas, fp64 --------------------------------------------------------------------------------------------------------------
def planes_formulas(dy, alpha=None, tok=None, bias=None):
    """dy [N, C, S] -> dict(d_tok [N, S, C], d_base [N, S, C] (= d_x_in transposed), dbias [C], dalpha [N] when tok is given)."""
    dy = dy.double()
    N = dy.shape[0]
    w = torch.ones(N, dtype=torch.float64) if alpha is None else 1.0 - alpha.double().reshape(N)
    dyt = dy.transpose(1, 2)
    out = {"d_tok": w.reshape(N, 1, 1) * dyt, "d_base": dyt.clone(), "dbias": (w.reshape(N, 1) * dy.sum(2)).sum(0)}
    if tok is not None:
        t = tok.double() if bias is None else tok.double() + bias.double()
        out["dalpha"] = -(dyt * t).sum((1, 2))
    return out


def rows_formulas(dy, alpha, x=None, h=None, base=None, t=None):
    """dy [R, C], alpha [G] -> dict(d_t, d_base, dalpha [G] when x (or t, the rounded x + h) and base are given)."""
    dy = dy.double()
    G = alpha.numel()
    C = dy.shape[-1]
    a = alpha.double().reshape(G, 1, 1)
    d3 = dy.reshape(G, -1, C)
    out = {"d_t": ((1.0 - a) * d3).reshape(dy.shape), "d_base": (a * d3).reshape(dy.shape)}
    if base is not None and (x is not None or t is not None):
        if t is None:
            t = x.double() if h is None else x.double() + h.double()
        out["dalpha"] = (d3 * (base.double() - t.double()).reshape(G, -1, C)).sum((1, 2))
    return out


# ---- the caps of the sums: any fp32 summation order of n terms errs by at most n 2^-24 sum|terms|, doubled (tests/linear_bwd_helpers.py)
def dbias_cap(dy, alpha=None):
    N, C, S = dy.shape
    w = torch.ones(N, dtype=torch.float64) if alpha is None else (1.0 - alpha.double().reshape(N)).abs()
    return 2.0 * (N * S) * 2.0 ** -24 * (w.reshape(N, 1) * dy.double().abs().sum(2)).sum(0)


def planes_dalpha_cap(dy, tok, bias):
    """terms: dy tok, and bias[c] colsum[n, c] (C S + C of them per sample)."""
    N, C, S = dy.shape
    d = dy.double()
    terms = (d.abs().transpose(1, 2) * tok.double().abs()).sum((1, 2))
    n = C * S
    if bias is not None:
        terms = terms + (bias.double().abs().reshape(1, C) * d.abs().sum(2)).sum(1)
        n += C
    return 2.0 * n * 2.0 ** -24 * terms


def rows_dalpha_cap(dy, base, t, G):
    C = dy.shape[-1]
    terms = (dy.double().abs() * (base.double() - t.double()).abs()).reshape(G, -1, C)
    return 2.0 * (terms.shape[1] * C) * 2.0 ** -24 * terms.sum((1, 2))


def make_planes(N, C, S, dtype, seed):
    """dy [N, C, S], tok, base [N, S, C] ~ N(0, 1), bias [C] ~ N(0, 0.09) rounded to dtype; alpha fp32 [N] in [0, 1] with different
    values per sample, exactly 1 (the image-only frame) first and exactly 0 second where N allows."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(N, C, S, generator=g).to(dtype)
    tok = torch.randn(N, S, C, generator=g).to(dtype)
    base = torch.randn(N, S, C, generator=g).to(dtype)
    bias = (torch.randn(C, generator=g) * 0.3).to(dtype)
    alpha = torch.rand(N, generator=g)
    alpha[0] = 1.0
    if N > 1:
        alpha[1] = 0.0
    return dy, tok, base, bias, alpha


def make_rows(G, row_div, C, dtype, seed):
    """dy, x, h, base [G row_div, C] rounded to dtype; alpha [G] fp32 holding values of the storage type (what the transformer
    passes), exactly 1 first and exactly 0 second where G allows."""
    g = torch.Generator().manual_seed(seed)
    R = G * row_div
    dy, x, h, base = (torch.randn(R, C, generator=g).to(dtype) for _ in range(4))
    alpha = torch.rand(G, generator=g).to(dtype).float()
    alpha[0] = 1.0
    if G > 1:
        alpha[1] = 0.0
    return dy, x, h, base, alpha


def errors(got, ref):
    """(max-norm, rms) error of got against ref, relative to ref's own max / rms."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()

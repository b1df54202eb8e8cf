"""Shared by tools/gen_golden_attention_bwd.py (reference side, build container only) and the attention-backward tests: the fp64
formula of softmax(q k^T D^-1/2) v and its gradients, the seeded inputs, and the error measures. The generator pins the formula to
the reference's CrossAttention (sgm/modules/attention.py:250-344 with identity projections); the GPU tests use the formula as their
oracle, so nothing of the reference has to exist where they run."""
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bwd")
D = 64                                                   # head dim of every spatial attention of the SVD UNet

# (B, H, Sq, Sk) of the fixtures that carry tensors, and of the shapes whose reference error only is recorded
TENSOR_CASES = [(1, 2, 192, 192), (2, 2, 48, 48), (1, 2, 200, 77), (1, 2, 130, 33)]
ERROR_CASES = [(1, 5, 768, 768), (1, 5, 3072, 3072), (1, 2, 1300, 1300), (1, 5, 200, 77), (2, 20, 48, 48)]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
# What the GPU tests run against the fp64 formula. Training shapes of the reference's configuration (latent 64 x 48, 14 frames; the batch
# cut to 2) and the sampling size (5, 9216) with one head (the fp64 oracle holds an S x S matrix per head on the CPU) ...
TRAINING_CASES = [(2, 5, 3072, 3072), (2, 10, 768, 768), (2, 20, 192, 192), (2, 20, 48, 48), (1, 1, 9216, 9216)]
# ... and ragged ones. Each ragged case carries ONE PEAKED ROW (q[0, 0] *= 6: scores six times larger, a softmax dominated by few
# keys) wherever its inputs are drawn — make_inputs applies it by membership in this list, so the generator (which records the
# reference's own error for (1, 2, 1300, 1300)) and the GPU test draw the same inputs for the same case.
RAGGED_CASES = [(1, 2, 1300, 1300), (2, 3, 1024, 300), (1, 1, 1500, 257), (1, 2, 1025, 4100), (3, 2, 33, 65), (1, 2, 130, 200)]


def case_name(case, tag):
    return "b%d_h%d_q%d_k%d_%s" % (*case, tag)


def case_seed(case):
    B, H, Sq, Sk = case
    return 1000003 * B + 10007 * H + 101 * Sq + Sk


def make_inputs(case, dtype):
    """Seeded x [B, Sq, H*D], context [B, Sk, H*D] and dy [B, Sq, H*D], rounded to dtype (always the cross form: q = x, k = v = context).
    The cases of RAGGED_CASES get their peaked row (x[0, 0] *= 6)."""
    B, H, Sq, Sk = case = tuple(case)
    peaked = case in RAGGED_CASES
    g = torch.Generator().manual_seed(case_seed(case))
    x = torch.randn(B, Sq, H * D, generator=g)
    ctx = torch.randn(B, Sk, H * D, generator=g)
    dy = torch.randn(B, Sq, H * D, generator=g)
    if peaked:
        x[0, 0] *= 6.0
    return x.to(dtype), ctx.to(dtype), dy.to(dtype)


def formula(q, k, v, dy, heads):
    """fp64: out and (dq, dk, dv) of out = softmax(q k^T D^-1/2) v for token-major q [B, Sq, H*D], k/v [B, Sk, H*D], written out as
    the six lines of the backward (no autograd)."""
    B, Sq, HD = q.shape
    Sk = k.shape[1]
    d = HD // heads
    scale = d ** -0.5
    qh, kh, vh, doh = (t.double().reshape(B, -1, heads, d).transpose(1, 2) for t in (q, k, v, dy))
    s = scale * qh @ kh.transpose(-1, -2)
    p = torch.softmax(s, dim=-1)
    out = p @ vh
    delta = (doh * out).sum(-1, keepdim=True)
    dv = p.transpose(-1, -2) @ doh
    dp = doh @ vh.transpose(-1, -2)
    ds = p * (dp - delta)
    dq = scale * ds @ kh
    dk = scale * ds.transpose(-1, -2) @ qh

    def back(t, S):
        return t.transpose(1, 2).reshape(B, S, HD)
    return back(out, Sq), back(dq, Sq), back(dk, Sk), back(dv, Sk)


def temporal_formula(q, k, v, dy, heads, T):
    """fp64 oracle of attention_temporal and its gradients: regroup [(bo T), S, C] -> [(bo S), T, C], formula, regroup back."""
    BT, S, HD = q.shape
    bo = BT // T

    def regroup(t):
        return t.reshape(bo, T, S, HD).transpose(1, 2).reshape(bo * S, T, HD)

    def back(t):
        return t.reshape(bo, S, T, HD).transpose(1, 2).reshape(BT, S, HD)
    return tuple(back(t) for t in formula(regroup(q), regroup(k), regroup(v), regroup(dy), heads))


def errors(got, ref):
    """(max-norm, rms) error of got against ref, relative to ref's own max / rms."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def bits(t):
    """16-bit patterns of a bf16 / f16 tensor as an int16 numpy array, and back."""
    return t.contiguous().view(torch.int16).numpy()


def from_bits(a, dtype):
    return torch.from_numpy(a.copy()).view(dtype)


def ref_errors():
    with open(os.path.join(GOLDEN, "ref_errors.json")) as fh:
        return json.load(fh)


def ref_error_for(case, tag, table=None):
    """{dx_max, dx_rms, dcontext_max, dcontext_rms}: the reference's own error in that type for this shape where it was recorded,
    else the largest recorded entry of the type (the error barely moves with the shape)."""
    table = table or ref_errors()
    key = case_name(case, tag)
    if key in table:
        return table[key]
    rows = [v for k, v in table.items() if k.endswith("_" + tag)]
    return {f: max(r[f] for r in rows) for f in ("dx_max", "dx_rms", "dcontext_max", "dcontext_rms")}

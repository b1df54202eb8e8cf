"""Shared by tools/gen_golden_geglu_bwd.py (reference side, build container only) and the GEGLU-backward tests: the fp64 formula of
GEGLU (sgm/modules/attention.py:87-95: `x, gate = proj(x).chunk(2, -1); x * F.gelu(gate)`) and its gradients, the seeded inputs, and
the error measures. The generator pins the formula to the reference's GEGLU under fp64 autograd; the GPU tests use the formula as
their oracle, so nothing of the reference has to exist where they run."""
import json
import math
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geglu_bwd")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
OUTPUTS = ("dx", "dweight", "dbias")

# (rows, K, inner) of the fixtures that carry tensors (the formula does not depend on K; odd row counts, inner 40 and 64) ...
TENSOR_CASES = [(129, 64, 40), (77, 96, 64), (33, 64, 64), (161, 96, 40)]
# ... and of the K = 320 shapes whose reference error only is recorded
ERROR_CASES = [(rows, 320, inner) for rows in (300, 515, 2125, 4096) for inner in (64, 160, 1280)]
# Cases whose gate bias is set to +6 on the first quarter of the gate columns and to -6 on the second: gates deep in both GELU tails
# (Phi(-6) = 1e-9, the gradient of the upper tail is dy a to 1e-8). make_inputs applies it by membership in this list, so the
# generator and the tests draw the same inputs for the same case.
TAIL_CASES = [(161, 96, 40), (515, 320, 160), (2125, 320, 1280)]
TRAINING_ROWS = 14 * 3072                                # 14 frames of the 64 x 48 training latent


def case_name(case, tag):
    return "r%d_k%d_n%d_%s" % (*case, tag)


def case_seed(case):
    rows, K, inner = case
    return 1000003 * K + 10007 * inner + rows


def make_inputs(case, dtype):
    """Seeded x [rows, K], weight [2 inner, K] (unit-variance projection), bias [2 inner] and dy [rows, inner], rounded to dtype."""
    rows, K, inner = case = tuple(case)
    g = torch.Generator().manual_seed(case_seed(case))
    x = torch.randn(rows, K, generator=g)
    w = torch.randn(2 * inner, K, generator=g) / math.sqrt(K)
    b = 0.5 * torch.randn(2 * inner, generator=g)
    dy = torch.randn(rows, inner, generator=g)
    if case in TAIL_CASES:
        q = inner // 4
        b[inner:inner + q] = 6.0
        b[inner + q:inner + 2 * q] = -6.0
    return x.to(dtype), w.to(dtype), b.to(dtype), dy.to(dtype)


def gate_formula(h, dy):
    """fp64: y and dh = [da | dg] of y = a gelu(g) for h = [a | g] [..., 2 inner] and the upstream gradient dy, written out."""
    h, dy = h.double(), dy.double()
    a, g = h.chunk(2, dim=-1)
    Phi = 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))
    phi = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    y = a * g * Phi
    da = dy * g * Phi
    dg = dy * a * (Phi + g * phi)
    return y, torch.cat([da, dg], dim=-1)


def formula(x, w, b, dy):
    """fp64: (y, dx, dweight, dbias) of y = GEGLU(x) with projection weight w [2 inner, K] and bias b [2 inner] or None, for 2-D x,
    written out (no autograd). dbias is returned for b None too (it is the column sum of dh)."""
    x64, w64 = x.double(), w.double()
    h = x64 @ w64.t()
    if b is not None:
        h = h + b.double()
    y, dh = gate_formula(h, dy)
    return y, dh @ w64, dh.t() @ x64, dh.sum(0)


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


ERROR_FIELDS = tuple(f"{o}_{m}" for o in OUTPUTS for m in ("max", "rms"))


def ref_errors():
    with open(os.path.join(GOLDEN, "ref_errors.json")) as fh:
        return json.load(fh)


def ref_error_for(case, tag, table=None):
    """{dx_max, dx_rms, dweight_max, dweight_rms, dbias_max, dbias_rms}: the reference's own error in that type for this shape
    where it was recorded, else the largest recorded entry of the type."""
    table = table or ref_errors()
    key = case_name(case, tag)
    if key in table:
        return table[key]
    rows = [v for k, v in table.items() if k.endswith("_" + tag)]
    return {f: max(r[f] for r in rows) for f in ERROR_FIELDS}

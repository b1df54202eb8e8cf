"""Pins the oracle of the attention-backward GPU tests to the reference (no GPU, no HIP library): the fp64 formula of
tests/attention_bwd_helpers.py reproduces what the reference's CrossAttention (sgm/modules/attention.py:250-344, identity
projections, run under autograd in fp64 by tools/gen_golden_attention_bwd.py) produced for every fixture under
tests/golden/attention_bwd/."""
import os

import numpy as np
import pytest
import torch

import attention_bwd_helpers as A

CASES = [(case, tag) for case in A.TENSOR_CASES for tag in A.DTYPES]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("case,tag", CASES, ids=[A.case_name(c, t) for c, t in CASES])
def test_fp64_formula_reproduces_the_reference_fixture(case, tag):
    """y, dx and dcontext (= dk + dv: with identity projections the context feeds k and v) to 1e-12 relative. The fixture stores the
    fp64 results as fp32, so the comparison is made on the fp32 rounding of the formula's result; the 1e-12 is what is left of
    fp64 against fp64 where the two roundings agree, and a one-ulp fp32 disagreement (6e-8) would fail it."""
    G = np.load(os.path.join(A.GOLDEN, A.case_name(case, tag) + ".npz"))
    dtype = A.DTYPES[tag]
    x, ctx, dy = (A.from_bits(G[n], dtype) for n in ("x", "context", "dy"))
    # the stored inputs are the seeded ones
    sx, sc, sdy = A.make_inputs(case, dtype)
    assert torch.equal(x, sx) and torch.equal(ctx, sc) and torch.equal(dy, sdy)
    y, dq, dk, dv = A.formula(x, ctx, ctx, dy, case[1])
    for name, got in (("y", y), ("dx", dq), ("dcontext", dk + dv)):
        ref = torch.from_numpy(G[name])
        assert ref.dtype == torch.float32 and ref.shape == got.shape
        # fp64 -> fp32 is a rounding to nearest on both sides: equal unless the two fp64 values straddle a rounding boundary
        err = _rel(got.float(), ref)
        print(f"{A.case_name(case, tag)} {name}: {err:.2e}")
        assert err <= 1e-12, (name, err)


def test_reference_error_table_covers_the_gpu_shapes():
    """ref_errors.json: four positive numbers per shape and type, in the range the issue's own runs of the recipe indicate
    (bf16 ~2e-3 .. 2e-2, f16 eight times smaller); every fixture carries the same four numbers."""
    table = A.ref_errors()
    for case in A.ERROR_CASES:
        for tag in A.DTYPES:
            row = table[A.case_name(case, tag)]
            lo, hi = (1e-3, 3e-2) if tag == "bf16" else (1e-4, 4e-3)
            for f in ("dx_max", "dx_rms", "dcontext_max", "dcontext_rms"):
                assert lo < row[f] < hi, (case, tag, f, row[f])
    for case, tag in CASES:
        e = np.load(os.path.join(A.GOLDEN, A.case_name(case, tag) + ".npz"))["ref_err"]
        assert e.shape == (4,) and (e > 0).all()
    # a shape without an entry takes the largest entry of its type
    worst = A.ref_error_for((9, 9, 99, 99), "bf16", table)
    assert worst["dx_rms"] == max(v["dx_rms"] for k, v in table.items() if k.endswith("_bf16"))


def test_temporal_formula_is_the_regrouped_formula():
    """The temporal oracle against autograd through the regrouping the reference does (video_attention.py:115, :136-140)."""
    g = torch.Generator().manual_seed(3)
    bo, T, S, H, D = 2, 5, 7, 2, 16
    q, k, v, dy = (torch.randn(bo * T, S, H * D, generator=g, dtype=torch.float64) for _ in range(4))
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))

    def regroup(t):
        return t.reshape(bo, T, S, H * D).transpose(1, 2).reshape(bo * S, T, H, D).transpose(1, 2)
    o = torch.nn.functional.scaled_dot_product_attention(regroup(qa), regroup(ka), regroup(va))
    o = o.transpose(1, 2).reshape(bo, S, T, H * D).transpose(1, 2).reshape(bo * T, S, H * D)
    o.backward(dy)
    out, dq, dk, dv = A.temporal_formula(q, k, v, dy, H, T)
    for got, ref in ((out, o.detach()), (dq, qa.grad), (dk, ka.grad), (dv, va.grad)):
        assert _rel(got, ref) < 1e-12

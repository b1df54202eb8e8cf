"""Fixtures of the attention backward (tests/golden/attention_bwd/), generated in the BUILD container from the imported reference:

    python tools/gen_golden_attention_bwd.py

The reference's CrossAttention (sgm/modules/attention.py:250-344) with its four projections set to the identity (zero bias) IS its
attention core: y = softmax(x context^T D^-1/2) context. For every case it is run under autograd in fp64 on inputs rounded to bf16 /
f16 — y, dx, dcontext — and again in that 16-bit type on the CPU: the reference's OWN error in the type, per gradient, as max-norm and
rms relative error. Small cases store tensors (<case>.npz); the shapes the GPU tests draw themselves (same seeded inputs,
tests/attention_bwd_helpers.py) store the four error numbers only (ref_errors.json). Arrays and numbers, no program text.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import attention_bwd_helpers as A  # noqa: E402
import ref_import  # noqa: E402


def identity_module(CrossAttention, heads, dtype):
    m = CrossAttention(query_dim=heads * A.D, heads=heads, dim_head=A.D)
    with torch.no_grad():
        for lin in (m.to_q, m.to_k, m.to_v, m.to_out[0]):
            lin.weight.copy_(torch.eye(heads * A.D))
            if lin.bias is not None:
                lin.bias.zero_()
    return m.to(dtype).eval()


def run(CrossAttention, heads, dtype, x, ctx, dy):
    m = identity_module(CrossAttention, heads, dtype)
    x = x.to(dtype).requires_grad_()
    ctx = ctx.to(dtype).requires_grad_()
    y = m(x, context=ctx)
    y.backward(dy.to(dtype))
    return y.detach(), x.grad, ctx.grad


def one_case(CrossAttention, case, tag):
    B, H, Sq, Sk = case
    dtype = A.DTYPES[tag]
    x, ctx, dy = A.make_inputs(case, dtype)
    y64, dx64, dc64 = run(CrossAttention, H, torch.float64, x, ctx, dy)
    _, dx16, dc16 = run(CrossAttention, H, dtype, x, ctx, dy)
    # the six-line formula against the reference's own fp64 autograd (what tests/test_attention_bwd_cpu.py re-checks from the files)
    fy, fdq, fdk, fdv = A.formula(x, ctx, ctx, dy, H)
    agree = max(A.errors(fy, y64)[0], A.errors(fdq, dx64)[0], A.errors(fdk + fdv, dc64)[0])
    dx_max, dx_rms = A.errors(dx16, dx64)
    dc_max, dc_rms = A.errors(dc16, dc64)
    err = dict(dx_max=dx_max, dx_rms=dx_rms, dcontext_max=dc_max, dcontext_rms=dc_rms)
    print(f"{A.case_name(case, tag)}: formula vs reference fp64 {agree:.1e}; reference's own error dx {dx_max:.2e} / {dx_rms:.2e}, "
          f"dcontext {dc_max:.2e} / {dc_rms:.2e} (max / rms)", flush=True)
    return x, ctx, dy, y64, dx64, dc64, err


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref_import.import_reference()
    from sgm.modules.attention import CrossAttention
    os.makedirs(A.GOLDEN, exist_ok=True)
    for case in A.TENSOR_CASES:
        for tag in A.DTYPES:
            x, ctx, dy, y, dx, dc, err = one_case(CrossAttention, case, tag)
            np.savez_compressed(os.path.join(A.GOLDEN, A.case_name(case, tag) + ".npz"), x=A.bits(x), context=A.bits(ctx), dy=A.bits(dy),
                                y=y.float().numpy(), dx=dx.float().numpy(), dcontext=dc.float().numpy(),
                                ref_err=np.array([err["dx_max"], err["dx_rms"], err["dcontext_max"], err["dcontext_rms"]], dtype=np.float64))
    table = {}
    for case in A.ERROR_CASES:
        for tag in A.DTYPES:
            table[A.case_name(case, tag)] = one_case(CrossAttention, case, tag)[-1]
    with open(os.path.join(A.GOLDEN, "ref_errors.json"), "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

"""The token-major GroupNorm(+SiLU) under autograd, the parts that need no GPU: what ops.group_norm_tok2tok computes (its CPU path in fp64
against the fp64 formula of tests/groupnorm_bwd_helpers.py on the transposed input — the formula the fallback and the kernels of
csrc/groupnorm_bwd.hip must both reproduce, the `frames` form included), and the host-only gate of the backward through the built
library."""
import pytest
import torch

import groupnorm_bwd_helpers as G
from test_groupnorm_bwd_cpu import load_fixture

CASES = [(case, tag) for case in G.TENSOR_CASES for tag in G.DTYPES]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _tokens(t):
    """[N, C, H, W] -> token-major [N, H W, C]"""
    return t.flatten(2).transpose(1, 2).contiguous()


@pytest.mark.parametrize("case,tag", CASES, ids=[G.case_name(c, t) for c, t in CASES])
def test_cpu_path_against_the_fp64_formula(case, tag):
    """ops.group_norm_tok2tok on CPU tensors under fp64 autograd, frames = case.T, against G.formula on the planes input: y and every
    gradient to 1e-12 relative max norm."""
    from multiview_inpaint_amd.svd import ops
    _, x, emb, dy, weight, bias = load_fixture(case, tag)
    f = G.formula(x, emb, dy, weight, bias, case.T, case.silu, case.eps)
    ta = _tokens(x.double()).requires_grad_()
    wa, ba = weight.double().requires_grad_(), bias.double().requires_grad_()
    ea = None if emb is None else emb.double().requires_grad_()
    y = ops.group_norm_tok2tok(ta, G.GROUPS, wa, ba, case.eps, silu=case.silu, chan_bias=ea, frames=case.T)
    assert y.dtype == torch.float64 and y.shape == ta.shape and y.is_contiguous()
    y.backward(_tokens(dy.double()))
    got = dict(y=y.detach(), dx=ta.grad, dweight=wa.grad, dbias=ba.grad, demb=None if ea is None else ea.grad)
    for n in G.OUTPUTS:
        if f[n] is None:
            assert n == "demb" and got[n] is None
            continue
        ref = _tokens(f[n]) if n in ("y", "dx") else f[n]
        err = _rel(got[n], ref)
        print(f"{G.case_name(case, tag)} {n}: {err:.2e}")
        assert err <= 1e-12, (n, err)


def test_host_gate_of_the_backward():
    """hip_ops.group_norm_tok2tok_backward_supported (mvi_groupnorm_tok2tok_backward_supported, a pure host function of the built
    library): yes for odd token counts, groups that cross a vector, whole videos and the widest row; no where C is not a multiple of the
    16-byte vector, N is not a whole number of videos, there are more than 64 groups, or N exceeds the forward's grid."""
    from multiview_inpaint_amd.svd import hip_ops
    ok = hip_ops.group_norm_tok2tok_backward_supported
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert ok(2, 64, 45, 32, 1, dt)
        assert ok(2, 96, 64, 32, 1, dt)
        assert ok(4, 64, 48, 32, 2, dt)
        assert ok(28, 2560, 48, 32, 1, dt)
        assert not ok(3, 64, 48, 32, 2, dt)                        # N = 3 is not a whole number of 2-frame videos
        assert not ok(2, 65 * 8, 48, 65, 1, dt)                    # 65 groups
        assert not ok(65536, 64, 48, 32, 1, dt)
    assert not ok(2, 36, 48, 4, 1, torch.bfloat16) and not ok(2, 36, 48, 4, 1, torch.float16)     # 36 is no multiple of 8
    assert not ok(2, 64, 48, 32, 1, torch.float64)

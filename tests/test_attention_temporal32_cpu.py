"""The routing edit of temporal attention for 17 .. 32 frames (svd/ops.py), checked without a GPU: the CPU path of
ops.attention_temporal is still the regrouped reference at 25 frames, under autograd too, and the gate of the HIP backward ends
at 32 frames."""
import pytest
import torch

import attention_bwd_helpers as A


def _ops():
    from multiview_inpaint_amd.svd import ops
    return ops


def test_cpu_path_at_25_frames_equals_the_regrouped_reference():
    """ops.attention_temporal on fp64 CPU tensors at T = 25 (and its autograd gradients) against the fp64 formula of
    tests/attention_bwd_helpers.py on `(b t) s c -> (b s) t c`: 1e-12 relative, fp64 against fp64."""
    ops = _ops()
    bo, T, S, Hh, D = 2, 25, 3, 2, 16
    g = torch.Generator().manual_seed(25)
    q, k, v, dy = (torch.randn(bo * T, S, Hh * D, generator=g, dtype=torch.float64) for _ in range(4))
    ref = A.temporal_formula(q, k, v, dy, Hh, T)
    with torch.no_grad():
        out = ops.attention_temporal(q, k, v, Hh, T)
    assert out.shape == q.shape and A.errors(out, ref[0])[0] <= 1e-12
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    ops.attention_temporal(qa, ka, va, Hh, T).backward(dy)
    for name, got, want in (("dq", qa.grad, ref[1]), ("dk", ka.grad, ref[2]), ("dv", va.grad, ref[3])):
        assert A.errors(got, want)[0] <= 1e-12, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_backward_gate_ends_at_32_frames(dtype):
    ops = _ops()
    for T, want in ((1, True), (16, True), (17, True), (25, True), (32, True), (33, False), (0, False)):
        q = torch.zeros(2 * max(T, 1), 3, 2 * 64, dtype=dtype)
        assert ops._temporal_backward_supported(q, q, q, 2, T) is want, (T, want)
    q = torch.zeros(2 * 25, 3, 2 * 64, dtype=dtype)
    assert not ops._temporal_backward_supported(q, q, q, 3, 25)              # 128 channels are not 3 heads
    assert not ops._temporal_backward_supported(q, q, q[:, :2], 2, 25)
    assert not ops._temporal_backward_supported(q[:49], q[:49], q[:49], 2, 25)   # 49 rows are not a multiple of 25

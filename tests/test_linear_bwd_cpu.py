"""What the HIP backward of the projections rests on, on the CPU: tests/linear_bwd_helpers.py's written-out gradients — the GPU tests'
oracle — are fp64 autograd's; the routing questions of ops.linear are pure functions of the shape; and on CPU tensors ops.linear is
F.linear whatever the switch says."""
import pytest
import torch
import torch.nn.functional as F

import linear_bwd_helpers as B

SHAPES = [(5, 3, 4), (1, 1, 1), (33, 7, 2), (64, 64, 128)]          # (rows, K, N)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_formulas_against_fp64_autograd(shape):
    rows, K, N = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, N, generator=g, dtype=torch.float64)
    dx, dw, db = B.autograd_grads(x, w, b, dy)
    assert (B.dx_formula(dy, w) - dx).abs().max().item() <= 1e-12
    assert (B.dweight_formula(x, dy) - dw).abs().max().item() <= 1e-12
    assert (B.dbias_formula(dy) - db).abs().max().item() <= 1e-12
    # dx is a projection with the transposed weight: what ops._linear_transposed hands the forward kernels
    assert (F.linear(dy, w.t().contiguous()) - dx).abs().max().item() <= 1e-12


def test_make_rows_strided_views():
    x, dy, w, b = B.make_rows(9, 64, 128, torch.bfloat16, seed=1, strided=True)
    assert tuple(x.shape) == (9, 64) and x.stride() == (128, 1)
    assert tuple(dy.shape) == (9, 128) and dy.stride() == (384, 1) and dy.storage_offset() == 128
    assert tuple(w.shape) == (128, 64) and tuple(b.shape) == (128,)


def test_gates_and_speed_decision_are_pure_functions():
    """Same arguments, same answer, a bool each time, no state in between; linear_gates declines K or N that are not multiples of 64,
    fp32, and empty inputs."""
    from multiview_inpaint_amd.svd import ops
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    shapes = [(rows, K, N) for rows in (14 * 576, 28 * 2304, 28 * 9216)
              for N, K in ((320, 320), (960, 320), (320, 1280), (640, 640), (1920, 640), (640, 2560), (1280, 1280), (3840, 1280), (1280, 5120))]
    first = [(ops.linear_gates(r, K, N, dt), ops.linear_backward_pays(r, K, N, dt, nd)) for r, K, N in shapes for dt in (bf, f16) for nd in (False, True)]
    again = [(ops.linear_gates(r, K, N, dt), ops.linear_backward_pays(r, K, N, dt, nd)) for r, K, N in shapes for dt in (bf, f16) for nd in (False, True)]
    assert first == again
    assert all(type(a) is bool and type(b) is bool for a, b in first)
    for K, N in ((96, 320), (320, 32), (320, 96), (100, 320), (330, 960)):
        assert ops.linear_gates(28 * 9216, K, N, bf) is False, (K, N)
    assert ops.linear_gates(28 * 9216, 320, 960, f32) is False
    assert ops.linear_gates(0, 320, 960, bf) is False
    # the level-0 projections pass the gates at the full step's row count (the speed decision is a separate question)
    assert ops.linear_gates(28 * 9216, 320, 960, bf) and ops.linear_gates(28 * 9216, 1280, 320, f16) and ops.linear_gates(28 * 9216, 320, 320, bf)
    # what the table does not list is not routed
    assert ops.linear_backward_pays(28 * 9216, 384, 448, bf, True) is False


def test_the_switch_is_off_by_default():
    import os
    from multiview_inpaint_amd.svd import ops
    if os.environ.get("MVI_LINEAR_BWD") is None:
        assert ops.LINEAR_BACKWARD is False


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_linear_on_cpu_tensors_is_f_linear(on, dtype, monkeypatch):
    """Switch off and on: output and gradients of ops.linear on CPU tensors under grad are bit-equal to F.linear's."""
    from multiview_inpaint_amd.svd import ops
    monkeypatch.setattr(ops, "LINEAR_BACKWARD", on)
    monkeypatch.setattr(ops, "linear_backward_pays", lambda *a: True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 70, 320, generator=g).to(dtype)
    w = (torch.randn(960, 320, generator=g) / 18).to(dtype)
    b = torch.randn(960, generator=g).to(dtype)
    dy = torch.randn(2, 70, 960, generator=g).to(dtype)

    def run(fn):
        xa, wa, ba = (t.clone().requires_grad_() for t in (x, w, b))
        y = fn(xa, wa, ba)
        y.backward(dy)
        return y.detach(), xa.grad, wa.grad, ba.grad
    for got, ref in zip(run(ops.linear), run(F.linear)):
        assert torch.equal(got, ref)
    lin = torch.nn.Linear(320, 960).to(dtype)
    xa = x.clone().requires_grad_()
    assert torch.equal(ops.linear_module(lin, xa), lin(xa))

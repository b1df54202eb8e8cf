"""The references of tests/train_ops_helpers.py against independent plain-Python formulations on small inputs (no GPU): what the
GPU edge tests of the training-loop ops (tests/test_train_ops_edges_gpu.py) compare the HIP kernels with is itself checked here."""
import numpy as np
import pytest
import torch

import train_ops_helpers as TH


def _loop_rows(mask):
    return [i for i, m in enumerate(mask.tolist()) if m != 0]


@pytest.mark.parametrize("first,cap", [(0, 40), (0, 5), (3, 4), (7, 1), (0, None), (-1, 6), (None, 6), (None, 0)])
@pytest.mark.parametrize("offset,pad", [(0, 0), (2, 3)])
def test_window_references_against_python_loops(first, cap, offset, pad):
    P, w = 40, 3
    g = torch.Generator().manual_seed(11)
    mask = (torch.rand(P, generator=g) < 0.4).to(torch.uint8) * 0x80
    rows = _loop_rows(mask)
    nk = len(rows)
    first = {None: nk, -1: nk - 1}.get(first, first)             # None: at the count; -1: the last kept row
    cap = nk if cap is None else cap
    stride = w + offset + pad if (offset or pad) else 0
    s = stride or w
    full, comp = TH.rand_words((P, w), g), TH.rand_words((max(cap, 1) * s + offset,), g)
    n = max(0, min(cap, nk - first))
    # gather
    want = comp.clone()
    for j in range(n):
        for k in range(w):
            want[offset + j * s + k] = full[rows[first + j], k]
    assert torch.equal(TH.gather_window_ref(full, comp, mask, first, cap, offset, stride), want)
    # scatter, and the zero fill of a missing input
    want, want0 = full.clone(), full.clone()
    for j in range(n):
        for k in range(w):
            want[rows[first + j], k] = comp[offset + j * s + k]
            want0[rows[first + j], k] = 0
    assert torch.equal(TH.scatter_window_ref(full, comp, mask, first, cap, offset, stride), want)
    assert torch.equal(TH.scatter_window_ref(full, None, mask, first, cap), want0)
    assert TH.window_rows(mask, first, cap).tolist() == rows[first:first + n]
    if first >= nk:
        assert n == 0 and torch.equal(want, full)


@pytest.mark.parametrize("P", [1, 31, 32, 33, 64, 65, 100])
def test_bit_pack_and_union_references_against_python_loops(P):
    rng = np.random.default_rng(P)
    flags = rng.choice(np.array([0, 0, 1, 2, 0x80, 255], np.uint8), size=(3, P))
    words = (P + 31) // 32
    packed = []
    for r in range(3):
        want = [0] * words
        for i in range(P):
            if flags[r, i] != 0:
                want[i // 32] |= 1 << (i % 32)
        got = TH.pack_bits_ref(flags[r])
        assert got.dtype == np.uint32 and got.tolist() == want
        packed.append(got)
    # union: garbage past P in the inputs must not matter
    dirty = np.stack(packed).copy()
    if P % 32:
        dirty[:, -1] |= np.uint32((0xFFFFFFFF << (P % 32)) & 0xFFFFFFFF)
    want = [int(any(flags[r, i] != 0 for r in range(3))) for i in range(P)]
    got = TH.union_bits_ref(dirty, P)
    assert got.dtype == np.uint8 and got.shape == (P,) and got.tolist() == want
    assert TH.union_bits_ref(dirty[:1], P).tolist() == [int(f != 0) for f in flags[0]]


def test_adam_float64_reference_against_torch_adam_in_float64():
    rng = np.random.default_rng(3)
    n, steps, lr = 257, 5, 1e-2
    p0 = rng.standard_normal(n)
    grads = [g.astype(np.float64) for g in TH.sweep_grads(n, steps, 5)]
    p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, eps=1e-15, foreach=False)
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    rp, rm, rv = TH.adam_ref64(p0, grads, lr)
    st = opt.state[p]
    assert np.abs(rp - p.detach().numpy()).max() <= 1e-13 * lr * steps
    assert np.abs(rm - st["exp_avg"].numpy()).max() <= 1e-13 * np.abs(rm).max()
    assert (np.abs(rv - st["exp_avg_sq"].numpy()) <= 1e-13 * np.abs(rv)).all()
    # continuing from given moments equals running straight through
    qp, qm, qv = TH.adam_ref64(p0, grads[:2], lr)
    qp, qm, qv = TH.adam_ref64(qp, grads[2:], lr, exp_avg=qm, exp_avg_sq=qv, first_step=3)
    assert np.array_equal(qp, rp) and np.array_equal(qm, rm) and np.array_equal(qv, rv)
    # the sweep covers the decades either side of eps, where sqrt(v) / sqrt(bc2) and eps trade places
    mags = np.abs(np.concatenate(TH.sweep_grads(4096, 1, 0)))
    assert mags.min() >= 1e-30 and mags.max() <= 1e3 and (mags < 1e-17).any() and (mags > 1e-13).any()


@pytest.mark.parametrize("N", [3, 4, 40, 300])
def test_lattice_knn_reference_against_the_oracle(N):
    import loss_oracle as lo
    pts = TH.lattice_points(N, N, copies=5 if N >= 40 else 0)
    got = TH.knn3_lattice_ref(pts)
    assert got.dtype == np.float32 and got.shape == (N,)
    if N == 3:                                                   # two other points only: one FLT_MAX term, in fp32
        d = ((pts[:, None] - pts[None]) ** 2).sum(-1)
        for i in range(3):
            a, b = sorted(int(d[i, j]) for j in range(3) if j != i)
            assert got[i] == (np.float32(a) + np.float32(b) + TH.FLT_MAX) / np.float32(3)
        return
    want = lo.knn3_mean_dist2(pts.astype(np.float32))
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * want.max()      # one fp32 rounding of sum / 3
    if N >= 40:                                                  # five copies of one point: three nearest distances are 0
        assert (got == 0).sum() == 5


def test_loss_gradient_tolerance_is_measured_and_capped():
    ratios = TH.loss_fp32_ratios()
    assert set(ratios) == set(TH.LOSS_CASES) and all(0.0 < r < 1e-3 for r in ratios.values())
    tol = TH.loss_grad_tolerance()
    print("fp32 restatement against the fp64 oracle, worst |d| / max(|ref|, 1e-2 max|ref|):")
    for case, r in ratios.items():
        print(f"  {case}: {r:.3e}")
    print(f"gradient tolerance: {tol:.3e}")
    assert tol == min(4.0 * max(ratios.values()), 1e-4) and tol <= 1e-4
    # masked pixels: the oracle's gradient is exactly zero there
    for case in TH.LOSS_CASES:
        w = TH.loss_inputs(*case)[2]
        if w is not None:
            assert (w == 0).any() and not TH.loss_oracle(*case)["grad"][:, w == 0].any()

"""Pins the oracle of the GEGLU-backward GPU tests to the reference (no GPU, no HIP library): the fp64 formula of
tests/geglu_bwd_helpers.py reproduces what the reference's GEGLU (sgm/modules/attention.py:87-95, run under autograd in fp64 by
tools/gen_golden_geglu_bwd.py) produced for every fixture under tests/golden/geglu_bwd/."""
import os

import numpy as np
import pytest
import torch

import geglu_bwd_helpers as G

CASES = [(case, tag) for case in G.TENSOR_CASES for tag in G.DTYPES]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("case,tag", CASES, ids=[G.case_name(c, t) for c, t in CASES])
def test_fp64_formula_reproduces_the_reference_fixture(case, tag):
    """y, dx, dweight and dbias to 1e-12 relative (max norm), fp64 against the fp64 the fixture stores; the stored inputs are the
    seeded ones."""
    F = np.load(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz"))
    dtype = G.DTYPES[tag]
    x, w, b, dy = (G.from_bits(F[n], dtype) for n in ("x", "weight", "bias", "dy"))
    for got, seeded in zip((x, w, b, dy), G.make_inputs(case, dtype)):
        assert torch.equal(got, seeded)
    for name, got in zip(("y",) + G.OUTPUTS, G.formula(x, w, b, dy)):
        ref = torch.from_numpy(F[name])
        assert ref.dtype == torch.float64 and ref.shape == got.shape
        err = _rel(got, ref)
        print(f"{G.case_name(case, tag)} {name}: {err:.2e}")
        assert err <= 1e-12, (name, err)


def test_fixtures_stay_small():
    """No fixture larger than the largest of tests/golden/attention_bwd/ (about 410 KB)."""
    for case, tag in CASES:
        assert os.path.getsize(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz")) <= 410 * 1024


def test_tail_case_reaches_both_tails():
    """The tail cases put gate columns near +6 and -6."""
    for case in G.TAIL_CASES:
        x, w, b, dy = G.make_inputs(case, torch.bfloat16)
        inner = case[2]
        gate = (x.double() @ w.double().t() + b.double())[:, inner:]
        q = inner // 4
        assert gate[:, :q].mean() > 5.5 and gate[:, q:2 * q].mean() < -5.5
    assert any(c in G.TENSOR_CASES for c in G.TAIL_CASES) and any(c in G.ERROR_CASES for c in G.TAIL_CASES)


def test_gate_formula_against_autograd():
    """The written-out gate (used as the oracle of the elementwise kernel) against fp64 autograd through chunk, gelu and mul."""
    g = torch.Generator().manual_seed(5)
    h = (3.0 * torch.randn(37, 2 * 24, generator=g, dtype=torch.float64)).requires_grad_()
    dy = torch.randn(37, 24, generator=g, dtype=torch.float64)
    a, gate = h.chunk(2, dim=-1)
    y = a * torch.nn.functional.gelu(gate)
    y.backward(dy)
    fy, fdh = G.gate_formula(h.detach(), dy)
    assert _rel(fy, y.detach()) < 1e-12 and _rel(fdh, h.grad) < 1e-12


def test_reference_error_table_covers_the_gpu_shapes():
    """ref_errors.json: six positive numbers per K = 320 shape and type, in the range the reference's rounding of the projection to
    the 16-bit type indicates (bf16: 2^-9 = 2e-3 per rounding, f16 eight times smaller); every fixture carries the same six numbers."""
    table = G.ref_errors()
    assert len(table) == len(G.ERROR_CASES) * len(G.DTYPES)
    for case in G.ERROR_CASES:
        for tag in G.DTYPES:
            row = table[G.case_name(case, tag)]
            assert sorted(row) == sorted(G.ERROR_FIELDS)
            lo, hi = (5e-4, 5e-2) if tag == "bf16" else (5e-5, 6e-3)
            for f in G.ERROR_FIELDS:
                assert lo < row[f] < hi, (case, tag, f, row[f])
    for case, tag in CASES:
        e = np.load(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz"))["ref_err"]
        assert e.shape == (len(G.ERROR_FIELDS),) and (e > 0).all()
    # a shape without an entry takes the largest entry of its type
    worst = G.ref_error_for((9, 9, 9), "bf16", table)
    assert worst["dx_rms"] == max(v["dx_rms"] for k, v in table.items() if k.endswith("_bf16"))

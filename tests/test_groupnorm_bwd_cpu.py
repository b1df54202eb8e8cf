"""Pins the oracle of the GroupNorm-backward GPU tests to the reference (no GPU, no HIP library): the fp64 formula of
tests/groupnorm_bwd_helpers.py reproduces what the reference's modules (normalization + SiLU behind `h + emb_out`, the b c t h w form,
Normalize; run under autograd in fp64 by tools/gen_golden_groupnorm_bwd.py) produced for every fixture under
tests/golden/groupnorm_bwd/, and the helper's stack3 / token-major gradient folds are what autograd gives for ops._stack3 / a transpose."""
import os

import numpy as np
import pytest
import torch

import groupnorm_bwd_helpers as G

CASES = [(case, tag) for case in G.TENSOR_CASES for tag in G.DTYPES]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def load_fixture(case, tag):
    Z = np.load(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz"))
    dtype = G.DTYPES[tag]
    x, dy = G.from_bits(Z["x"], dtype), G.from_bits(Z["dy"], dtype)
    emb = torch.from_numpy(Z["emb"]) if "emb" in Z.files else None
    return Z, x, emb, dy, torch.from_numpy(Z["weight"]), torch.from_numpy(Z["bias"])


@pytest.mark.parametrize("case,tag", CASES, ids=[G.case_name(c, t) for c, t in CASES])
def test_fp64_formula_reproduces_the_reference_fixture(case, tag):
    """y, dx, dweight, dbias, demb to 1e-12 relative max-norm against the fp64 tensors of the fixture; the stored inputs are the seeded ones."""
    Z, x, emb, dy, weight, bias = load_fixture(case, tag)
    sx, semb, sdy, sw, sb = G.make_inputs(case, G.DTYPES[tag])
    assert torch.equal(x, sx) and torch.equal(dy, sdy) and torch.equal(weight, sw) and torch.equal(bias, sb)
    assert (emb is None) == (semb is None) == (not case.cb) and (emb is None or torch.equal(emb, semb))
    f = G.formula(x, emb, dy, weight, bias, case.T, case.silu, case.eps)
    for n in G.OUTPUTS:
        if f[n] is None:
            assert n == "demb" and n not in Z.files
            continue
        ref = torch.from_numpy(Z[n])
        assert ref.dtype == torch.float64 and ref.shape == f[n].shape
        err = _rel(f[n], ref)
        print(f"{G.case_name(case, tag)} {n}: {err:.2e}")
        assert err <= 1e-12, (n, err)


def test_fixture_set_and_error_table():
    """The cases the issue names are there; every file is at most 500 KB and the set at most 3 MB; ref_errors.json holds positive
    numbers for every training shape and type (bf16 roughly eight times f16)."""
    names = {c.name: c for c in G.TENSOR_CASES}
    odd = names["odd_s45"]
    assert (odd.H * odd.W) % 2 == 1 and (odd.C // G.GROUPS * odd.H * odd.W) % 8 != 0
    assert names["cg3"].C == 96 and (names["temporal_t2"].T, names["temporal_t2"].N) == (2, 4)
    nz = names["normalize"]
    assert not nz.silu and not nz.cb and nz.eps == 1e-6 and nz.C == 96 and nz.H * nz.W == 64
    assert names["offset"].offset
    total = 0
    for case, tag in CASES:
        size = os.path.getsize(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz"))
        assert size <= 500 * 1024
        total += size
    assert total <= 3 * 1024 * 1024
    table = G.ref_errors()
    for case in G.ERROR_CASES:
        for tag in G.DTYPES:
            row = table[G.case_name(case, tag)]
            lo, hi = (1e-3, 3e-2) if tag == "bf16" else (1e-4, 4e-3)
            for n in G.OUTPUTS:
                for s in ("_max", "_rms"):
                    assert lo < row[n + s] < hi, (case.name, tag, n + s, row[n + s])
    worst = G.ref_error_for(G.Case("absent", 1, 32, 1, 1, 1, True, True, 1e-5, False), "bf16", table)
    assert worst["dx_rms"] == max(v["dx_rms"] for k, v in table.items() if k.endswith("_bf16"))


def test_gradient_folds_are_what_autograd_gives():
    """fold_stack3 against autograd of ops._stack3, fold_tokens against autograd of the b c h w -> b (h w) c transpose, in fp64."""
    from multiview_inpaint_amd.svd import ops
    g = torch.Generator().manual_seed(5)
    for T, N in ((3, 6), (1, 2), (2, 2)):
        y = torch.randn(N, 4, 3, 5, generator=g, dtype=torch.float64, requires_grad=True)
        d3 = torch.randn(N, 12, 3, 5, generator=g, dtype=torch.float64)
        ops._stack3(y, T).backward(d3)
        assert _rel(G.fold_stack3(d3, T), y.grad) < 1e-12
    y = torch.randn(2, 4, 3, 5, generator=g, dtype=torch.float64, requires_grad=True)
    dt = torch.randn(2, 15, 4, generator=g, dtype=torch.float64)
    y.flatten(2).transpose(1, 2).contiguous().backward(dt)
    assert _rel(G.fold_tokens(dt, (3, 5)), y.grad) < 1e-12


def test_formula_against_autograd_of_the_package_cpu_ops():
    """The formula against fp64 autograd through the package's own CPU ops (ops.group_norm_frames with chan_bias), temporal form."""
    from multiview_inpaint_amd.svd import ops
    case = G.Case("cpu_t3", 6, 64, 3, 5, 3, True, True, 1e-5, True)
    x, emb, dy, w, b = (t.double() for t in G.make_inputs(case, torch.bfloat16))
    xa, ea, wa, ba = (t.clone().requires_grad_() for t in (x, emb, w, b))
    y = ops.group_norm_frames(xa, 3, G.GROUPS, wa, ba, 1e-5, silu=True, chan_bias=ea)
    y.backward(dy)
    f = G.formula(x, emb, dy, w, b, 3, True, 1e-5)
    # (ops.group_norm_frames upcasts through .float(): fp32 statistics, so the agreement is at fp32 level)
    for n, got in (("y", y.detach()), ("dx", xa.grad), ("dweight", wa.grad), ("dbias", ba.grad), ("demb", ea.grad)):
        assert _rel(got, f[n]) < 1e-5, n

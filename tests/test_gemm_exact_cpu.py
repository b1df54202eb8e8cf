"""The data of tests/test_gemm_exact_gpu.py on the CPU: the preconditions of every construction at every shape the GPU tests run
(tests/exact_gemm_helpers.py asserts them while it builds a case), and a mutation check of the comparison itself — the fp64 reference
recomputed six times with one planted fault each; torch.equal against the clean expected output has to be False every time. No GPU
code runs here."""
import pytest
import torch
import torch.nn.functional as F

import exact_gemm_helpers as E

TAGS = list(E.DTYPES)


@pytest.mark.parametrize("tag", TAGS)
def test_every_case_of_the_gpu_tests_meets_its_preconditions(tag):
    """parity: every reference element an (even) integer the type holds exactly, no exclusions. rounding: finite, below 2^24, at least one
    exact tie, more than half of the elements need rounding. gates: the three gate classes occur, v g finite. The rounding set is absent
    (None) only where the helpers say so: f16 launches WITHOUT a bias whose K_total < 1280 cannot reach 4096, and the bias-free
    stride-2 dgrad in f16 and at a 64-channel contraction."""
    absent = []
    for name, build in E.every_case(tag):
        case = build()
        if case is None:
            absent.append(name)
            continue
        for t in (getattr(case, "want", None), getattr(case, "want_s", None)):
            assert t is None or (t.dtype == E.DTYPES[tag] and torch.isfinite(t).all()), name
    for name in absent:
        assert " rounding " in name, name
        assert name.startswith("conv3x3_s2_dgrad") or (tag == "f16" and name.split()[0] in ("linear_n320", "linear_k320")), name
    if tag == "bf16":
        assert absent == [n for n, _ in E.every_case(tag) if n.startswith("conv3x3_s2_dgrad rounding") and n.endswith("64)")], absent
    many = E.geglu_case(tag, *E.FF_GEGLU_N320_MANY_TILES)
    rows, K, inner = E.FF_GEGLU_N320_MANY_TILES
    assert -(-rows // 256) * (inner // 160) > 256 and (K // 64) >= 4 and (K // 64) % 2 == 0 and torch.isfinite(many.want).all()


def test_the_rounding_examples_of_the_types():
    """257 -> 256 and 259 -> 260 in bf16, 2049 -> 2048 and 2051 -> 2052 in f16: torch's fp64 -> half conversion rounds ties to even; the
    helpers' tie / spacing / truncation arithmetic agrees with it."""
    v = torch.tensor([257.0, 259.0, 2049.0, 2051.0], dtype=torch.float64)
    assert v[:2].to(torch.bfloat16).tolist() == [256.0, 260.0] and v[2:].to(torch.float16).tolist() == [2048.0, 2052.0]
    assert E.is_tie(v[:2], torch.bfloat16).all() and E.is_tie(v[2:], torch.float16).all()
    assert not E.is_tie(torch.tensor([258.0, 513.0], dtype=torch.float64), torch.bfloat16).any()
    assert E.ulp_of(v, torch.bfloat16).tolist() == [2.0, 2.0, 16.0, 16.0] and E.ulp_of(v, torch.float16).tolist() == [0.25, 0.25, 2.0, 2.0]
    assert E.truncate_to(torch.tensor([259.0, -259.0, 255.0]).double(), torch.bfloat16).tolist() == [258.0, -258.0, 255.0]
    x = torch.randn(4096, dtype=torch.float64) * 100
    for dtype in E.DTYPES.values():
        r, t = x.to(dtype).double(), E.truncate_to(x, dtype)
        assert torch.equal(t.to(dtype).double(), t) and (t.abs() <= x.abs()).all() and ((t == r) | ((t - r).abs() == E.ulp_of(x, dtype))).all()


# ---- the mutation check ----------------------------------------------------------------------------------------------------------------

MUT_LINEAR = (257, 1280, 640, True)            # (rows, K, N, with_bias): the longest plain projection of the GPU list. (At K = 704 the first
#                                                half of K sums to 4 * 352 < 2048: f16 holds it exactly and fault 6 would be invisible in f16)
MUT_CONV = (3, 3, 5, 64, 640)                  # rows that straddle image rows: where a missing border test reads the neighbouring row


def _detected(mutant, case, dtype):
    """What the GPU test would see: the faulty kernel's output, stored in the type, against the clean expected output."""
    return not torch.equal(mutant.to(dtype), case.want)


@pytest.mark.parametrize("tag", TAGS)
def test_the_comparison_notices_each_of_six_planted_faults(tag):
    dtype = E.DTYPES[tag]
    rows, K, N, wb = MUT_LINEAR
    par, rnd = E.linear_case("parity", tag, rows, K, N, wb), E.linear_case("rounding", tag, rows, K, N, wb)
    assert not _detected(par.ref.clone(), par, dtype) and not _detected(rnd.ref.clone(), rnd, dtype)     # (the clean recomputation passes)
    found = {}
    r, c, k = 200, 417, 129
    # 1. one (row, k) product dropped from one output
    m = par.ref.clone()
    m[r, c] -= par.x[r, k] * par.w[c, k]
    found["one product dropped"] = _detected(m, par, dtype)
    # 2. one product doubled
    m = par.ref.clone()
    m[r, c] += par.x[r, k] * par.w[c, k]
    found["one product doubled"] = _detected(m, par, dtype)
    # 3. two K-chunks of 64 swapped between two output columns (columns 5 and 325: the same column of two 320-column groups)
    ca, cb, ch = 5, 325, slice(3 * 64, 4 * 64)
    w = par.w.clone()
    w[ca, ch], w[cb, ch] = par.w[cb, ch], par.w[ca, ch]
    found["two K chunks swapped between two columns"] = _detected(F.linear(par.x, w, par.b), par, dtype)
    # 4. one border tap taken from the neighbouring image row instead of zero: pixel (y, 0)'s left tap (ky 1, kx 0) reads token
    #    y W + 0 - 1 = (y - 1, W - 1)
    cv = E.conv3x3_case("parity", tag, *MUT_CONV)
    m, y, Wd = cv.ref.clone(), 1, MUT_CONV[2]
    m[0, :, y, 0] += cv.w[:, :, 1, 0] @ cv.x[0, :, y - 1, Wd - 1]
    found["a border tap from the neighbouring image row"] = _detected(m, cv, dtype)
    # 5. truncation instead of round-to-nearest-even on the store
    found["truncation on the store"] = _detected(E.truncate_to(rnd.ref, dtype), rnd, dtype)
    # 6. the partial sum of the first half of K rounded to the storage type before the second half is added
    h = K // 2
    first = F.linear(rnd.x[:, :h], rnd.w[:, :h]).to(dtype).double()
    found["a partial sum kept in the storage type"] = _detected(first + F.linear(rnd.x[:, h:], rnd.w[:, h:], rnd.b), rnd, dtype)
    for what, hit in found.items():
        print(f"mutation [{tag}] {what}: {'detected' if hit else 'MISSED'}")
    assert len(found) == 6 and all(found.values()), found
    # round-half-away is caught too (the ties exist: asserted by the helper)
    tie = E.is_tie(rnd.ref, dtype)
    away = torch.where(tie, rnd.ref + torch.sign(rnd.ref) * 0.5 * E.ulp_of(rnd.ref, dtype), rnd.ref)
    assert _detected(away, rnd, dtype)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("which", ["linear", "conv3x3", "conv3t"])
def test_share_of_single_dropped_terms_the_parity_comparison_catches(tag, which):
    """1000 random (output, k) positions at the largest K_total of each family: a dropped +-1 term makes the even output odd, and every
    odd integer up to 256 is a number of bf16 (2048 in f16) — every drop that lands on an output with |ref| <= 256 is caught, and that is
    more than 99.9 % of the positions."""
    dtype = E.DTYPES[tag]
    if which == "linear":
        case = E.linear_case("parity", tag, *MUT_LINEAR)
        terms = lambda i, k: case.x[i // 640, k] * case.w[i % 640, k]
    elif which == "conv3x3":
        case = E.conv3x3_case("parity", tag, *E.CONV3X3[-1])                 # K_total = 9 * 192
        terms = None
    else:
        case = E.conv3t_case("parity", tag, *E.CONV3T[-1])                   # K_total = 3 * 640
        terms = None
    ref = case.ref.reshape(-1)
    g = torch.Generator().manual_seed(5)
    pos = torch.randint(0, ref.numel(), (1000,), generator=g)
    ks = torch.randint(0, case.K_total if which == "linear" else 1, (1000,), generator=g)
    # (a term of +-1 data is +-1 whichever (tap, channel) it is: for the convolutions the sign alone is drawn)
    t = torch.stack([terms(int(i), int(k)) for i, k in zip(pos, ks)]) if terms else E.signs(g, 1000)
    clean = ref[pos]
    caught = (clean - t).to(dtype) != clean.to(dtype)
    small = clean.abs() <= 256
    share = caught.double().mean().item()
    print(f"dropped terms [{tag}, {which}, K_total {case.K_total}]: {share:.4f} caught, max |ref| = {ref.abs().max().item():.0f}")
    assert caught[small].all() and share > 0.999

"""Exact-answer tests of every attention kernel, forward and backward: attn_flash.hip (4 waves), attn_flash8m16.hip (8 waves),
attn_rowtile.hip, attn_temporal.hip and attn_bwd.hip under multiview_inpaint_amd/csrc/, through hip_ops.
The data, its preconditions, the expectations and the case lists are tests/exact_attention_helpers.py's;
tests/test_attention_exact_cpu.py checks the preconditions on the CPU and shows
that the comparisons used here notice eight planted faults.

Held BIT FOR BIT (torch.equal, or == 0 for the zero-sum set): the output of every forward kernel and entry in bf16 and f16 on the
selector, uniform, pairs and comb sets (comb: the data that keeps the 8-wave kernel in its fast form) — on the 8-wave and the rowtile
kernel the exact ties of pairs and comb included; dv of the backward on the selector set (where the exact sum is not zero) and on
the uniform set.
Held to a bound that a reading of the kernels put in place of equality (each derived in the helpers):
  * pairs and comb, exact ties, 4-wave kernel only: it normalises by the sum of the UNROUNDED probabilities, 2 (1 + e) with e the
    fp32 rounding of its reference exponent: a result that lies exactly between two numbers of the type may fall to either. There —
    and only there — both neighbours pass. The 8-wave kernel sums the rounded P on the matrix pipe: every block of the pairs set
    repeats with the online form (asserted in fp64 by the helper), P = 1, l = 2 and inv = 0.5 exactly.
  * backward, selector set, what should vanish: bf16 (and fp32) can hold the other keys' probabilities 2^-gap, so dq, and dv where no
    row chose the key, carry dust below the case's `tiny` (< 2^-30); where the chosen rows' dout cancel, the matrix pipe's fp32 sums
    (not rounded to nearest) turn that dust into single fp32 ulps of the partial sums: the fp32 summation cap. In f16 all of these are
    +-0. dk is NOT zero: see selector_bwd_case.
  * backward, uniform set, dq and dk: the elementwise bound of uniform_bwd_case; the worst ratio is printed and recorded in DESIGN.md.
  * fp32 I/O (rowtile): |got - want| <= 2^-13 |want| on the selector and pairs sets, as fp32 storage does not absorb the score rounding.
  * lse: |err| <= 4 x 2^-23 max(|lse|, 1); on the signed uniform case, where scale s and ln(Sk) may cancel, relative to the larger term."""
import pytest
import torch

import exact_attention_helpers as E
import svd_helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF = ("bf16", "f16")
KINDS = ("selector", "uniform", "pairs", "comb")
LSE_BAR = 4 * 2.0 ** -23


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    """MVI_STRICT for every test of this module: a GPU tensor that would leave the HIP path raises (svd/ops.py)."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


def _dev(t, dtype):
    """fp64 holding numbers of `dtype` -> the device tensor (exact)."""
    d = t.to(dtype)
    assert torch.equal(d.double(), t)
    return d.to(DEV)


def _describe(bad, got, want):
    idx = bad.nonzero()
    diff = (got.double() - want.double())[bad]
    dims = [sorted(set(idx[:, d].tolist()))[:12] for d in range(idx.shape[1])]
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; indices per axis (first 12) {dims}; got - want in "
            f"[{diff.min().item()}, {diff.max().item()}], first {diff[:6].tolist()} at {idx[:6].tolist()}")


def _check_forward(case, got, what, tag, strict_ties=False):
    """selector: one right bit pattern. uniform: == 0. pairs, comb: one right bit pattern; at an exact tie either neighbour unless
    strict_ties. fp32 I/O: uniform == 0, the others within 2^-13 |want| elementwise."""
    got = got.detach().cpu()
    assert got.shape == case.want.shape and got.dtype == case.want.dtype, (what, got.shape, got.dtype)
    g, w = got.double(), case.want.double()
    if case.kind == "uniform":
        bad = (g != 0) | torch.isnan(g)
    elif tag == "f32":
        bad = ~((g - w).abs() <= 2.0 ** -13 * w.abs())
    elif case.kind == "selector":
        bad = (g != w) | torch.isnan(g)                                        # (no +-0 in v: equal values are equal bits)
    else:
        bad = (g != w) | torch.isnan(g)
        if not strict_ties:
            bad = bad & ~(case.tie & ((g - case.ref).abs() == 0.5 * E.ulp_of(case.ref, case.want.dtype)))
    assert not bool(bad.any()), f"{what}: {_describe(bad, got, case.want)}"


def _check_lse(case, lse, what):
    err = ((lse.detach().double().cpu() - case.lse).abs() / case.lse.abs().clamp(min=1.0)).max().item()
    H.report(f"{what}: worst |lse - fp64| = {err / 2.0 ** -23:.2f} x 2^-23 max(|lse|, 1)")
    assert err <= LSE_BAR, (what, err)


def _qkv(case, dtype):
    return tuple(_dev(t, dtype) for t in (case.q, case.k, case.v))


# ---- forward ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("shape", E.FLASH4 + E.FLASH8, ids=lambda s: "x".join(map(str, s)))
def test_flash_forward(ops, tag, shape):
    """hip_ops.attention on the four sets. 4-wave kernel: the smallest shape it serves, one row past a 128-query block and one key past
    a tile, nine query blocks. 8-wave kernel: no tails, a last block of one row with a last tile of one key, the ring wrapped eight
    times with a tail of 12 keys; bf16 runs its exact-scale form, f16 the folded one. The kernel that ran is asserted."""
    dtype = E.DTYPES[tag]
    B, Hh, Sq, Sk = shape
    want_variant = 4 if shape in E.FLASH4 else 16
    assert ops.attention_kernel_variant(Sq, Sk, 64, dtype) == want_variant == E.kernel_variant(Sq, Sk, 64, tag)
    assert ops.attention_kernel_kind(Sq, Sk, 64, dtype) == 1
    for kind in KINDS:
        c = E.SETS[kind](tag, *shape, 64)
        out = ops.attention(*_qkv(c, dtype), Hh)
        # the 8-wave kernel takes the row sum of the ROUNDED P from the matrix pipe — 2 (pairs: every block repeats with the online
        # form, asserted by the helper, and P = 1) or n (comb) — so inv is a power of two and ties are held bit for bit
        _check_forward(c, out, f"attention {tag} {kind} {shape} variant {want_variant}", tag, strict_ties=want_variant == 16)


@pytest.mark.parametrize("tag", list(E.DTYPES))
@pytest.mark.parametrize("shape", E.ROWTILE, ids=lambda s: "x".join(map(str, s)))
def test_rowtile_forward(ops, tag, shape):
    """The fp32-math kernel: D = 16 and 32, D = 64 at Sk = 1, 25 and 32 — the last key count before the flash kernel takes over (33 is
    the first after, FLASH4[0]); bf16, f16 and fp32 I/O. Its two selected keys of the pairs set see identical arithmetic, P = 1 and
    l = 2 exactly: ties are held bit for bit."""
    dtype = E.DTYPES[tag]
    B, Hh, Sq, Sk, D = shape
    assert ops.attention_kernel_kind(Sq, Sk, D, dtype) == 0 and ops.attention_kernel_variant(Sq, Sk, D, dtype) == 0
    if D == 64 and tag != "f32":
        assert ops.attention_kernel_kind(Sq, 32, 64, dtype) == 0 and ops.attention_kernel_kind(Sq, 33, 64, dtype) == 1
    for kind in E.sets_for(Sk):
        c = E.SETS[kind](tag, *shape)
        out = ops.attention(*_qkv(c, dtype), Hh)
        _check_forward(c, out, f"attention rowtile {tag} {kind} {shape}", tag, strict_ties=True)


@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("mode", ["scale", "q_log2"])
@pytest.mark.parametrize("shape", E.PACKED, ids=lambda s: "x".join(map(str, s)))
def test_packed_forward(ops, tag, mode, shape):
    """attention_packed on a [B, S, 3 H D] projection output, one shape per flash kernel: the exact answer itself, and (plain scale)
    torch.equal to the separate-tensor call. q_log2: Q carries D^-1/2 log2(e) already — for the selector codes another magnitude."""
    dtype = E.DTYPES[tag]
    B, Hh, S, _ = shape
    for kind in KINDS:
        c = E.SETS[kind](tag, *shape, 64, mode)
        q, k, v = _qkv(c, dtype)
        qkv = torch.cat([q, k, v], -1).contiguous()
        out = ops.attention_packed(qkv, Hh, q_log2=mode == "q_log2")
        strict = E.kernel_variant(S, S, 64, tag) == 16
        _check_forward(c, out, f"attention_packed {tag} {kind} {shape} {mode}", tag, strict_ties=strict)
        if mode == "scale":
            assert torch.equal(out, ops.attention(q, k, v, Hh)), (kind, shape)


def _temporal_variant(T, Hh, D, dtype, packed):
    from multiview_inpaint_amd import _lib
    code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]
    return _lib.lib().mvi_attention_temporal_kernel_variant(T, Hh, D, code, 3 * Hh * D if packed else 0, Hh * D if packed else 0)


@pytest.mark.parametrize("tag", list(E.DTYPES))
@pytest.mark.parametrize("shape", E.TEMPORAL + E.TEMPORAL_ROWTILE, ids=lambda s: "x".join(map(str, s)))
def test_temporal_forward(ops, tag, shape):
    """attention_temporal and attention_temporal_packed on [(Bo T), S, H D]: the sequence is the frame axis, keys and codes are per
    (video, spatial token, head) — the selector codes carry a random mask per problem, so the frames of a neighbouring token or video
    would select a wrong key, and the zero sums are per problem. T = 1 (selector only: one key admits no zero sum), 2, 7, 14, 16 at
    S = 5 and 33 on the MFMA kernel (D = 64, 16 bit); the rowtile form at D = 32 and in fp32."""
    dtype = E.DTYPES[tag]
    Bo, T, S, Hh, D = shape
    mfma = D == 64 and tag != "f32"                                        # (fp32 I/O and D = 32: the rowtile kernel)
    for packed in (False, True):
        assert _temporal_variant(T, Hh, D, dtype, packed) == (1 if mfma else 0)
    for kind in E.sets_for(T)[:2]:
        c = E.SETS[kind](tag, Bo * S, Hh, T, T, D)
        q, k, v = (_dev(E.to_temporal(t, Bo, S), dtype) for t in (c.q, c.k, c.v))
        out = ops.attention_temporal(q, k, v, Hh, T)
        c_t = E.Case(kind=c.kind, want=E.to_temporal(c.want, Bo, S))
        _check_forward(c_t, out, f"attention_temporal {tag} {kind} {shape}", tag)
        out_p = ops.attention_temporal_packed(torch.cat([q, k, v], -1).contiguous(), Hh, T)
        assert torch.equal(out_p, out), (kind, shape)


# ---- backward -----------------------------------------------------------------------------------------------------------------------------

def _ratio(got, ref, bound):
    return ((got.detach().double().cpu() - ref).abs() / bound).max().item()


def _forward_backward(ops, c, dtype, what):
    """attention, attention_forward_lse (bit-identical out), attention_backward twice (bit-identical). -> (out, lse, dq, dk, dv)."""
    q, k, v = _qkv(c.fwd, dtype)
    d = _dev(c.dout, dtype)
    out, lse = ops.attention_forward_lse(q, k, v, c.H)
    assert torch.equal(out, ops.attention(q, k, v, c.H)), f"{what}: the forward under autograd is not the inference forward"
    g1 = ops.attention_backward(q, k, v, out, d, lse, c.H)
    g2 = ops.attention_backward(q, k, v, out, d, lse, c.H)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)), f"{what}: two backward runs differ"
    return (out, lse) + tuple(g1)


@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("shape", E.FLASH4 + E.FLASH8, ids=lambda s: "x".join(map(str, s)))
def test_backward_selector(ops, tag, shape):
    """P is one-hot after rounding to the type: dv[j] is the exact integer sum of dout over the rows that chose j; dq vanishes (delta from
    the rounded out equals dP of the selected key, both exact integer sums); dk is bounded by what the unrounded P of the selected
    key leaves of dP - delta in the dK/dV kernel. lse = scale * s_match."""
    dtype = E.DTYPES[tag]
    assert ops.attention_backward_supported(shape[2], shape[3], 64, dtype)
    c = E.selector_bwd_case(tag, *shape)
    what = f"backward selector {tag} {shape}"
    out, lse, dq, dk, dv = _forward_backward(ops, c, dtype, what)
    _check_forward(c.fwd, out, what + " out", tag)
    _check_lse(c.fwd, lse, what)
    assert E.dv_mismatches(c, dv.cpu(), tag) == 0, f"{what} dv: {_describe(dv.cpu().double() != c.dv, dv.cpu(), c.dv_want)}"
    worst_dq = dq.double().abs().max().item()
    assert worst_dq <= (0.0 if tag == "f16" else c.tiny), (what, "dq", worst_dq, c.tiny)
    r = _ratio(dk, torch.zeros_like(c.dk_bound), c.dk_bound)
    H.report(f"{what}: worst |dk| / bound = {r:.3f}, max |dq| = {worst_dq:.2e}")
    assert r <= 1.0, (what, "dk", r)


@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("shape", E.FLASH4 + E.FLASH8, ids=lambda s: "x".join(map(str, s)))
def test_backward_uniform(ops, tag, shape):
    """The recomputed P is one constant and dout's columns sum to zero over the queries: dv == 0 exactly. dq and dk against the fp64
    formula under the elementwise bound of uniform_bwd_case. lse = scale * s + ln(Sk)."""
    dtype = E.DTYPES[tag]
    c = E.uniform_bwd_case(tag, *shape)
    what = f"backward uniform {tag} {shape}"
    out, lse, dq, dk, dv = _forward_backward(ops, c, dtype, what)
    _check_forward(c.fwd, out, what + " out", tag)
    _check_lse(c.fwd, lse, what)
    assert bool((dv == 0).all()), f"{what} dv: {_describe((dv != 0).cpu(), dv.cpu(), torch.zeros_like(dv.cpu()))}"
    rq, rk = _ratio(dq, c.dq, c.dq_bound), _ratio(dk, c.dk, c.dk_bound)
    H.report(f"{what}: worst |got - ref| / bound: dq {rq:.3f}, dk {rk:.3f}")
    assert rq <= 1.0 and rk <= 1.0, (what, rq, rk)


SIGNED = [(1, 2, 130, 200), (1, 2, 1025, 257)]


@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("shape", SIGNED, ids=lambda s: "x".join(map(str, s)))
def test_lse_of_signed_uniform_scores(ops, tag, shape):
    """The uniform set with scores of either sign, one shape per flash kernel: out == 0, and lse = scale s + ln(Sk) — where the two
    terms may cancel — within 4 x 2^-23 of the LARGER of |scale s|, ln(Sk) and 1: each term carries its own fp32 rounding."""
    dtype = E.DTYPES[tag]
    c = E.uniform_case(tag, *shape, 64, "scale", True)
    out, lse = ops.attention_forward_lse(*_qkv(c, dtype), c.H)
    _check_forward(c, out, f"signed uniform {tag} {shape}", tag)
    err = ((lse.double().cpu() - c.lse).abs() / c.lse_scale).max().item()
    H.report(f"signed uniform {tag} {shape}: worst |lse - fp64| = {err / 2.0 ** -23:.2f} x 2^-23 max(|scale s|, ln Sk, 1)")
    assert err <= LSE_BAR, (shape, err)


TEMPORAL_BWD = [(s, t) for s in E.TEMPORAL + E.TEMPORAL_ROWTILE for t in HALF] + [(s, "f32") for s in E.TEMPORAL_ROWTILE]


@pytest.mark.parametrize("shape,tag", TEMPORAL_BWD, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_temporal_backward(ops, shape, tag):
    """attention_temporal_backward (fp32 math on an LDS copy; P of the selected key is exactly 1 = e^0 / 1). selector: dv the exact
    sums, dq and dk dust below `tiny` (+-0 in f16). uniform (16-bit types, T >= 2): dq, dk under the elementwise bound, dv under the
    fp32 summation cap — P = 1 / T is a 24-bit number and T multiples of it do not sum exactly unless T is a power of two.
    Two runs are bit-identical."""
    dtype = E.DTYPES[tag]
    Bo, T, S, Hh, D = shape
    tt = lambda t: _dev(E.to_temporal(t, Bo, S), dtype)
    cases = [E.selector_bwd_case(tag, Bo * S, Hh, T, T, D)]
    if T >= 2 and tag != "f32":
        cases.append(E.uniform_bwd_case(tag, Bo * S, Hh, T, T, D))
    for c in cases:
        what = f"temporal backward {c.kind} {tag} {shape}"
        q, k, v, d = tt(c.fwd.q), tt(c.fwd.k), tt(c.fwd.v), tt(c.dout)
        g1 = ops.attention_temporal_backward(q, k, v, d, Hh, T)
        g2 = ops.attention_temporal_backward(q, k, v, d, Hh, T)
        assert all(torch.equal(a, b) for a, b in zip(g1, g2)), what
        dq, dk, dv = (E.from_temporal(t.cpu(), Bo, T) for t in g1)
        if c.kind == "selector":
            assert E.dv_mismatches(c, dv, tag) == 0, f"{what} dv: {_describe(dv.double() != c.dv, dv, c.dv_want)}"
            worst = max(dq.double().abs().max().item(), dk.double().abs().max().item())
            assert worst <= (0.0 if tag == "f16" else c.tiny), (what, worst, c.tiny)
        else:
            rq, rk = _ratio(dq, c.dq, c.dq_bound), _ratio(dk, c.dk, c.dk_bound)
            if T & (T - 1) == 0:                                           # P = 1 / T is a power of two: the sums are exact
                assert bool((dv == 0).all()) and not bool(c.dv_bound.any()), what
                rv = 0.0
            else:
                rv = _ratio(dv, torch.zeros_like(c.dv_bound), c.dv_bound)
            H.report(f"{what}: worst |got - ref| / bound: dq {rq:.3f}, dk {rk:.3f}, dv {rv:.3f}")
            assert rq <= 1.0 and rk <= 1.0 and rv <= 1.0, (what, rq, rk, rv)

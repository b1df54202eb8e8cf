"""CPU side of tests/test_norm_bwd_elementwise_gpu.py: the preconditions of tests/norm_bwd_exact_helpers.py on every case (asserted where
a case is built: numbers of the storage type, n * 1.703125 exact in fp32, an exact A on the constant group, the caps' own values equal to
the written-out formulas), the GroupNorm formula pinned to fp64 autograd, a plain CENTRED fp32 restatement of every operation inside its
own bound on every element of every case the GPU module runs (the reference alone leaves the kernels room), and the comparison's reaction
to planted faults — each on its smallest case, the share of elements outside the bound held to a FLOOR of half what the
correct-against-faulty run shows on the CPU. Measured shares (fault: case, output, type -> share):
    a store that truncates              gn (2, 64, 45) dx bf16 0.366, f16 0.201; ln (77, 64) dx bf16 0.473, f16 0.410; geglu (5, 1288) bf16 0.408, f16 0.364
    g rounded to the type before sums   gn (2, 64, 45) dx bf16 0.310, f16 0.186; dbias bf16 0.813, f16 0.391
    the neighbouring group's coef       gn (2, 64, 45) dx bf16 0.999, f16 1.000, fp32 1.000
    A, B per frame                      gn (4, 64, 40) T = 2 dx bf16 0.997, f16 0.999, fp32 0.999
    an unmasked tail in sum xh          gn (2, 64, 136) dchan_bias 0.961 in every type (dx does not read that sum: 0)
    stack3 across a video boundary      gn (4, 64, 40) T = 2 dx bf16 0.978, f16 0.995, fp32 0.993
    drow from the rounded gS            ln (77, 64, 7 runs) bf16 0.900, f16 0.534; (21, 40, one row per run) bf16 0.979, f16 0.780
    Phi(-|g|) as 1 - Phi(|g|)           geglu: EVERY deep-tail element outside the factor of two; none outside the absolute cap
    the folded xh, 1.703125 group       gn (2, 64, 45): dweight != 0 on every channel of the constant group, in every type (the centred
                                        form gives exactly 0); its dx stays under the cap in this emulation (the shift's 4e-6 relative
                                        is what a sum of 90 terms may lose): the exact check is what sees it
and the truncating store and the folded xh PASS the bars the backward tests had (tests/test_groupnorm_bwd_gpu.py: 1.6 x rms / 2.0 x max norm
of the reference's own 16-bit error) on the same data: the reason for this module."""
import collections

import pytest
import torch

import groupnorm_bwd_helpers as GB
import norm_bwd_exact_helpers as B

TAGS = ("f32", "bf16", "f16")
HALF = ("bf16", "f16")


def test_the_groupnorm_formula_is_fp64_autograd():
    assert B.pin_gn_formula_to_autograd() <= 1e-12


def _gn_cases(tag):
    for N, C, S, G, T, layout in B.GN_BWD_SHAPES:
        for cb, silu, cv in B.GN_BWD_VARIANTS:
            yield B.gn_bwd_case(tag, N, C, S, G, T, cb, silu, layout, cv)
    for N, C, S, G, T in B.TOK2TOK_SHAPES:
        for cb, silu, cv in B.GN_BWD_VARIANTS:
            yield B.gn_bwd_case(tag, N, C, S, G, T, cb, silu, B.TOKENS, cv)


def _ln_cases(tag):
    for R, C, runs in B.ln_bwd_shapes(tag):
        for mode in (B.LN_BWD_MODES if (R, C, runs) == B.LN_BWD_MODE_SHAPE else B.LN_BWD_MODES[:1]):
            yield B.ln_bwd_case(tag, R, C, runs, mode)


@pytest.mark.parametrize("tag", TAGS)
def test_fp32_restatements_stay_inside_their_own_bounds(tag):
    """Every case of the GPU module: the centred fp32 restatement is inside the bound on every element of every output, gives dweight
    == 0 on the constant group, and both constant values are in use."""
    values = set()
    for c in _gn_cases(tag):
        got = B.gn_bwd_f32(c)
        values.add(c.cv)
        for k in c.ref:
            assert B.worst_ratio(got[k], c.ref[k], c.bound[k]) <= 1.0, (c.N, c.C, c.S, c.T, c.layout, c.silu, k)
        assert torch.equal(got["dweight"][c.const_c], torch.zeros(int(c.const_c.sum()), dtype=torch.float64))
        if c.exact_dx:                               # no SiLU: 8 u |t1| + 10 u |t2| with t1 = eps^-1/2 w dy, |t2| <= |t1| + |dx| — nothing of the data
            cc = c.const_c
            t1 = (c.w[cc, None] * c.dyf[:, cc]).abs() * c.eps ** -0.5
            assert (c.cap["dx"][:, cc] <= (18.0 * t1 + 10.0 * c.ref["dx"][:, cc].abs()) * B.U * (1.0 + 1e-9)).all()
    assert values == set(B.CONST_VALUES)
    for c in _ln_cases(tag):
        got = B.ln_bwd_f32(c)
        for k in c.ref:
            assert B.worst_ratio(got[k], c.ref[k], c.bound[k]) <= 1.0, (c.R, c.C, c.runs, c.mode, k)
    for rows, inner in B.GEGLU_BWD_SHAPES:
        c = B.geglu_bwd_case(tag, rows, inner)
        got = B.geglu_bwd_f32(c)
        assert B.worst_ratio(got, c.ref, c.bound) <= 1.0 and B.tail_ok(got, c) == 0, (rows, inner)
        print(f"geglu_backward {(rows, inner)} {tag}: cap above half an ulp on {c.wide:.3f} of the elements, {int(c.tail.sum())} deep-tail elements")
        if inner > 8:
            assert int(c.tail.sum()) > 0


# (fault, (N, C, S, G, T, layout), output, {type: floor})
GN_FAULTS = [("truncate", (2, 64, 45, 32, 1, B.PLANES), "dx", dict(bf16=0.18, f16=0.10)),
             ("round_g", (2, 64, 45, 32, 1, B.PLANES), "dx", dict(bf16=0.15, f16=0.09)),
             ("round_g", (2, 64, 45, 32, 1, B.PLANES), "dbias", dict(bf16=0.40, f16=0.19)),
             ("neighbour", (2, 64, 45, 32, 1, B.PLANES), "dx", dict(bf16=0.49, f16=0.49, f32=0.49)),
             ("per_frame", (4, 64, 40, 32, 2, B.PLANES), "dx", dict(bf16=0.49, f16=0.49, f32=0.49)),
             ("tail", (2, 64, 136, 32, 1, B.PLANES), "dchan_bias", dict(bf16=0.48, f16=0.48, f32=0.48)),
             ("stack3_cross", (4, 64, 40, 32, 2, B.STACK3), "dx", dict(bf16=0.48, f16=0.49, f32=0.49))]


@pytest.mark.parametrize("fault,shape,out,floors", GN_FAULTS, ids=[f"{f}-{o}" for f, _, o, _ in GN_FAULTS])
def test_the_bound_flags_a_planted_groupnorm_fault(fault, shape, out, floors):
    for tag, floor in floors.items():
        c = B.gn_bwd_case(tag, *shape[:5], True, True, shape[5])
        assert B.outside_share(B.gn_bwd_f32(c)[out], c.ref[out], c.bound[out]) == 0.0
        share = B.outside_share(B.gn_bwd_f32(c, fault)[out], c.ref[out], c.bound[out])
        print(f"{fault} {shape} {out} {tag}: {share:.3f} of the elements outside the bound")
        assert share >= floor, (tag, share)


def test_every_planted_groupnorm_fault_is_exercised():
    assert {f for f, _, _, _ in GN_FAULTS} | {"fold"} == set(B.GN_FAULTS)


@pytest.mark.parametrize("tag", TAGS)
def test_the_folded_xh_is_seen_on_the_constant_group(tag):
    """xh = x r + (chan_bias - m) r on the group that is constant at 1.703125: dweight, exactly 0 in the centred form, is not 0 on any of
    the group's channels. At 2.0 both products are exact and nothing shows: the reason for the second value."""
    c = B.gn_bwd_case(tag, 2, 64, 45, 32, 1, True, True)
    bad = B.gn_bwd_f32(c, "fold")["dweight"][c.const_c]
    assert (bad != 0).all() and bad.abs().max().item() < 1e-2
    c2 = B.gn_bwd_case(tag, 2, 64, 45, 32, 1, True, True, B.PLANES, B.CONST_VALUES[0])
    assert (B.gn_bwd_f32(c2, "fold")["dweight"][c2.const_c] == 0).all()


LN_FAULTS = [("truncate", (77, 64, 7), "dx", dict(bf16=0.23, f16=0.20)), ("drow_rounded", (77, 64, 7), "drow", dict(bf16=0.44, f16=0.26)),
             ("drow_rounded", (21, 40, 21), "drow", dict(bf16=0.48, f16=0.38))]


@pytest.mark.parametrize("fault,shape,out,floors", LN_FAULTS, ids=[f"{f}-{s[0]}" for f, s, _, _ in LN_FAULTS])
def test_the_bound_flags_a_planted_layernorm_fault(fault, shape, out, floors):
    """drow's cap excludes a sum of rounded values: the sum of gS rounded to the storage type falls outside it, summed (11 rows per run)
    and stored directly (one row per run)."""
    for tag, floor in floors.items():
        c = B.ln_bwd_case(tag, *shape)
        assert B.outside_share(B.ln_bwd_f32(c)[out], c.ref[out], c.bound[out]) == 0.0
        share = B.outside_share(B.ln_bwd_f32(c, fault)[out], c.ref[out], c.bound[out])
        print(f"{fault} {shape} {out} {tag}: {share:.3f} of the elements outside the bound")
        assert share >= floor, (tag, share)


@pytest.mark.parametrize("tag", HALF)
def test_the_gate_checks_flag_their_faults(tag):
    c = B.geglu_bwd_case(tag, 5, 1288)
    share = B.outside_share(B.geglu_bwd_f32(c, "truncate"), c.ref, c.bound)
    assert share >= (0.20 if tag == "bf16" else 0.18), share
    bad = B.geglu_bwd_f32(c, "one_minus")
    assert int(c.tail.sum()) > 0 and B.tail_ok(bad, c) == int(c.tail.sum())
    assert B.outside_share(bad, c.ref, c.bound) == 0.0                             # the absolute cap alone does not see it


@pytest.mark.parametrize("tag", HALF)
def test_truncation_and_the_fold_pass_the_global_norm_bars(tag):
    """Against 1.6 x (rms) / 2.0 x (max norm) of the reference's own error in the type (tests/golden/groupnorm_bwd/ref_errors.json, the
    largest recorded entry: what tests/test_groupnorm_bwd_gpu.py applies to a shape that was not recorded) a truncating store of dx and
    the folded xh both pass on every output — on the data whose elementwise checks reject them. (The truncating store in bf16, where the
    reference's own error holds several roundings; in f16 its max norm passes, 1.4 x, and its rms, 1.63 x, sits on the bar: not asserted.)"""
    c = B.gn_bwd_case(tag, 2, 64, 45, 32, 1, True, True)
    r = GB.ref_error_for(collections.namedtuple("C", "name")("not recorded"), tag)
    names = dict(dx="dx", dweight="dweight", dbias="dbias", dchan_bias="demb")
    for fault in ("truncate", "fold") if tag == "bf16" else ("fold",):
        got = B.gn_bwd_f32(c, fault)
        for k, n in names.items():
            e_max, e_rms = GB.errors(got[k], c.ref[k])
            assert e_max <= 2.0 * r[n + "_max"] and e_rms <= 1.6 * r[n + "_rms"], (fault, k, e_max, e_rms)
    assert B.outside_share(B.gn_bwd_f32(c, "truncate")["dx"], c.ref["dx"], c.bound["dx"]) > 0.1
    assert (B.gn_bwd_f32(c, "fold")["dweight"][c.const_c] != 0).all()

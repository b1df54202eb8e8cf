"""CPU side of tests/test_norm_elementwise_gpu.py: every precondition of tests/norm_exact_helpers.py on every case, a plain fp32
restatement of each operation inside its own bound (the reference alone leaves the kernels room), and the comparison's reaction to nine
planted faults — each on the smallest case where it applies, the share of elements outside the bound held to a FLOOR of half what the
correct-against-faulty run shows on the CPU. Measured shares (fault: case, type -> share; floor):
    a store that truncates            (2, 64, 3) bf16 0.503; (2, 64, 45) bf16 0.465, f16 0.385      -> 0.25 / 0.23 / 0.19
    z rounded to the type before SiLU (2, 64, 45) bf16 0.224, f16 0.142                             -> 0.11 / 0.07
    the neighbouring group's moments  (2, 64, 3) bf16 1.000, f16 1.000, fp32 1.000                  -> 0.50
    per-frame statistics              (4, 64, 48) T = 2 bf16 0.962, f16 0.967, fp32 0.969           -> 0.48
    unbiased variance                 (2, 64, 3) n = 6 bf16 0.951; (2, 64, 45) n = 90 bf16 0.616; (2, 96, 64) n = 192 bf16 0.391
                                                                                                     -> 0.47 / 0.30 / 0.19
    eps outside the square root       (2, 64, 3) fp32 0.477 (bf16 0.008: eps = 1e-5 against a variance of 2^-6 and more is a relative
                                      1e-4, below bf16's half ulp — the fp32 cases are the ones that see it)  -> 0.23
    chan_bias after the statistics    (2, 64, 3) bf16 0.956, f16 0.966                               -> 0.47
    a row's vector tail on the neighbouring channel's weight / bias   (2, 64, 3): 8 of 64 channels in bf16, 0.125 -> 0.06
    alpha of the neighbouring sample  (4, 64, 45) blend bf16 0.995                                   -> 0.49
and the truncating store PASSES the bar the forward tests had before (tests/test_unet_ops_gpu.py: max|got - ref| / max|ref| < 1 / 128)
on the same data: the reason for this module."""
import pytest
import torch

import norm_exact_helpers as H

TAGS = ("f32", "bf16", "f16")


def _is_of(v, dtype):
    return torch.equal(v.to(dtype).double(), v)


@pytest.mark.parametrize("tag", TAGS)
def test_groupnorm_cases_meet_their_preconditions(tag):
    """Numbers of the storage type, fp32 parameters, distinct statistics per unit, the constant group with its one right output, and — on
    every case with units of at most 192 elements — a bound that is the rounding: cap <= ulp / 4 on 90 % of the elements in bf16, 60 %
    in f16 (fp32 output has no rounding to test: its cap is 2^4 ... 2^10 ulps by construction). Larger units are printed."""
    dtype = H.DTYPES[tag]
    for name, build in H.every_gn_case(tag):
        c = build()
        assert _is_of(c.x, dtype), name
        for p in (c.w, c.b) + (() if c.cb is None else (c.cb,)):
            assert _is_of(p, torch.float32), name
        G, Cg, V = c.G, c.C // c.G, c.N // c.T
        xe = c.x if c.cb is None else c.x + c.cb[:, :, None]
        x5 = xe.reshape(V, c.T, G, Cg, c.S)
        m = x5.mean((1, 3, 4))
        sd = x5.var((1, 3, 4), unbiased=False).sqrt()
        assert (sd[:, H.CONST_GROUP] == 0).all() and torch.equal(c.x.reshape(V, c.T, G, Cg, c.S)[:, :, H.CONST_GROUP],
                                                                 torch.full((V, c.T, Cg, c.S), H.CONST_VALUE, dtype=torch.float64)), name
        others = [g for g in range(G) if g != H.CONST_GROUP]
        # neighbouring units differ grossly: by more than a tenth of their spread in the mean or by a factor in the spread, for most pairs
        dm = (m[:, others][:, 1:] - m[:, others][:, :-1]).abs() / sd[:, others][:, 1:]
        assert (dm > 0.1).double().mean().item() > 0.8, name
        if c.T > 1:                                                                 # frames of a video differ by about a scale
            fm = x5.mean((3, 4))
            spread = (fm.max(1).values - fm.min(1).values)[:, others] / sd[:, others]
            assert spread.median().item() > 0.3, name
        assert int(c.const.sum()) == c.want_const.numel() == V * c.T * Cg * c.S
        line = f"{tag} {name}: n = {c.n}, cap <= ulp / 4 on {c.quarter:.3f} of the elements"
        if c.n <= H.SMALL_UNIT and tag != "f32":
            assert c.quarter >= (0.9 if tag == "bf16" else 0.6), line
        else:
            print(line)
        if c.outlier:
            assert (c.cap_out >= c.cap).all() and c.D > 3.0, (name, c.D)


@pytest.mark.parametrize("tag", TAGS)
def test_fp32_restatements_stay_inside_their_own_bounds(tag):
    """A plain fp32 evaluation of every operation, stored once in the case's type, is inside the bound on every element of every case —
    and reproduces the constant group's one right output (fp32 output with SiLU excepted: an fp32 evaluation of the sigmoid has no
    single right bit pattern; there the constant group stays under the bound)."""
    dtype = H.DTYPES[tag]
    for name, build in H.every_gn_case(tag):
        c = build()
        got = H.gn_f32(c)
        assert H.worst_ratio(got, c.ref, c.bound) <= 1.0, name
        if tag != "f32" or not c.silu:
            assert torch.equal(got[c.const].to(dtype), c.want_const), name
    for C in H.LN_WIDTHS:
        for R in H.LN_ROWS:
            for mode in H.LN_MODES:
                c = H.ln_case(tag, R, C, mode)
                assert _is_of(c.s, dtype) and _is_of(c.s_pre, dtype)
                assert H.worst_ratio(H.ln_f32(c), c.ref, c.bound) <= 1.0, (R, C, mode)
                if C <= H.SMALL_UNIT and tag != "f32":
                    assert c.quarter >= (0.9 if tag == "bf16" else 0.6), (R, C, mode, c.quarter)
    for cols in H.SOFTMAX_COLS:
        c = H.softmax_case(tag, cols)
        assert H.worst_ratio(H.softmax_f32(c), c.ref, c.bound) <= 1.0, cols
        assert torch.allclose(c.ref[6], torch.full((cols,), 1.0 / cols, dtype=torch.float64), rtol=1e-14) and c.ref[5].max().item() > 1.0 - 1e-6 * cols
    for rows, inner in ((5, 64), (3, 8)):
        c = H.geglu_case(tag, rows, inner)
        assert H.worst_ratio(H.geglu_f32(c), c.ref, c.bound) <= 1.0, (rows, inner)
    base, t, bias, alpha, c = H.blend_case(tag, 4, 64, 45)
    assert H.worst_ratio(H.blend_f32(dtype, base, t, H.chan(bias, 3), alpha, lambda v: H.samp(v, 3)), c.ref, c.bound) <= 1.0
    assert torch.equal(c.ref[1], base[1])                                           # alpha = 1 returns base


# (fault, (N, C, S, G, T), type, floor): see the module docstring for the measured shares
FAULTS = [("truncate", (2, 64, 3, 32, 1), "bf16", 0.25), ("truncate", (2, 64, 45, 32, 1), "bf16", 0.23), ("truncate", (2, 64, 45, 32, 1), "f16", 0.19),
          ("round_z", (2, 64, 45, 32, 1), "bf16", 0.11), ("round_z", (2, 64, 45, 32, 1), "f16", 0.07),
          ("neighbour", (2, 64, 3, 32, 1), "bf16", 0.5), ("neighbour", (2, 64, 3, 32, 1), "f16", 0.5), ("neighbour", (2, 64, 3, 32, 1), "f32", 0.5),
          ("per_frame", (4, 64, 48, 32, 2), "bf16", 0.48), ("per_frame", (4, 64, 48, 32, 2), "f16", 0.48), ("per_frame", (4, 64, 48, 32, 2), "f32", 0.48),
          ("unbiased", (2, 64, 3, 32, 1), "bf16", 0.47), ("unbiased", (2, 64, 45, 32, 1), "bf16", 0.30), ("unbiased", (2, 96, 64, 32, 1), "bf16", 0.19),
          ("eps_outside", (2, 64, 3, 32, 1), "f32", 0.23),
          ("cb_after", (2, 64, 3, 32, 1), "bf16", 0.47), ("cb_after", (2, 64, 3, 32, 1), "f16", 0.47),
          ("tail", (2, 64, 3, 32, 1), "bf16", 0.06)]


@pytest.mark.parametrize("fault,shape,tag,floor", FAULTS)
def test_the_bound_flags_a_planted_fault(fault, shape, tag, floor):
    c = H.gn_case(tag, *shape, True, True)
    assert H.outside_share(H.gn_f32(c), c.ref, c.bound) == 0.0
    share = H.outside_share(H.gn_f32(c, fault), c.ref, c.bound)
    print(f"{fault} {shape} {tag}: {share:.3f} of the elements outside the bound")
    assert share >= floor


def test_the_bound_flags_the_neighbouring_samples_alpha():
    base, t, bias, alpha, c = H.blend_case("bf16", 4, 64, 45)
    bad = H.blend_f32(c.dtype, base, t, H.chan(bias, 3), alpha, lambda v: H.samp(v, 3), neighbour=True)
    share = H.outside_share(bad, c.ref, c.bound)
    print(f"alpha of the neighbouring sample: {share:.3f} of the elements outside the bound")
    assert share >= 0.49


@pytest.mark.parametrize("tag", ("bf16", "f16"))
def test_a_truncating_store_passes_the_global_norm_bar(tag):
    """max|got - ref| / max|ref| of a store that rounds toward zero is below the 1 / 128 (bf16) and 1 / 1024 (f16) the forward tests of
    tests/test_unet_ops_gpu.py hold the kernels to, on the very data whose elementwise bound rejects a third of its elements."""
    c = H.gn_case(tag, 2, 64, 45, 32, 1, True, True)
    bad = H.gn_f32(c, "truncate")
    rel = float((bad - c.ref).abs().max() / c.ref.abs().max())
    assert rel < (1.0 / 128 if tag == "bf16" else 1.0 / 1024), rel
    assert H.outside_share(bad, c.ref, c.bound) > 0.19

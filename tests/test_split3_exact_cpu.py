"""The data of tests/test_split3_exact_gpu.py on the CPU: every precondition of tests/split3_exact_helpers.py at every shape the GPU tests
run, a plain fp32 restatement of the three-term contraction in a shuffled chunk order that has to give the expected bits, and a mutation
check of the comparison itself — the contraction recomputed with one planted fault each; torch.equal against the clean expected output
has to be False every time. No GPU code runs here.

What the Gaussian comparisons see is measured too (test_what_the_max_norm_bar_and_the_gauss_bound_see). Errors of independent terms add
in quadrature, so a fault in one 64-channel chunk of x_lo . w_hi is 2^-9.4 sqrt(64 / (9 C)) of the output — 6e-4 at C = 64, 5e-4 at
C = 128 — and the 3e-5 max-norm bar of tests/test_vae_gpu.py DOES see it, as it sees a border tap that leaks a whole pixel (0.2 to 0.4).
What it cannot see are the faults below the omitted x_lo . w_lo term (3e-6 of the output scale on this data): a single wrong lo
element from C = 128 on, a truncating split, lo taken from the truncated hi, the fourth term added. The derived elementwise bound on
Gaussian data (2 K_total 2^-24 sum|terms|) is wider than the max-norm bar on a typical element: it rejects the gross faults only. The
exact sets reject every one of them."""
import pytest
import torch
import torch.nn.functional as F

import exact_gemm_helpers as E
import split3_exact_helpers as S

MAX_NORM_BAR = 3e-5                                               # tests/test_vae_gpu.py, tests/test_vae_encode_split_gpu.py


def test_every_case_of_the_gpu_tests_meets_its_preconditions():
    """conv_case / int_case assert on every element: both halves bf16 numbers, hi + lo an fp32 number whose split on the bit pattern is
    (hi, lo) with no tie, sum|terms| below 2^24 units, the reference a multiple of the unit and an fp32 number. The mags set is absent
    exactly where the helper names it. The fp32 restatement in a shuffled chunk order gives the expected bits (exact sets), and stays
    inside the elementwise bound (gauss)."""
    absent = set()
    for name, build in S.every_case():
        c = build()
        geom, kind = name.split()[0], name.split()[1]
        if c is None:
            assert kind == "mags", name
            absent.add((geom, next(s for s in S.CASES[geom] if name.endswith(str(s)))))
            continue
        if kind == "int":
            assert c.want.dtype == torch.float32 and torch.isfinite(c.want).all(), name
            continue
        got = S.restate_f32(c, S.gen(43, c.rows, c.Co))
        if kind in S.EXACT:
            assert c.want.dtype == torch.float32 and torch.equal(got, c.want), name
            assert c.abs_ref.max().item() / S.U < 2 ** 24, name
        else:
            ratio = ((got.double() - c.ref).abs() / c.bound).max().item()
            assert ratio <= 1.0, (name, ratio)
    assert absent == S.MAGS_ABSENT, absent


def test_the_three_term_sum_is_not_the_rounded_product():
    """On the unit set the omitted x_lo . w_lo terms are +-2^-20 each: the expected output differs from fp32(x . w) on most elements, so
    the comparison also holds the kernel to the deliberate omission."""
    for geom, shape in (("conv9", (1, 16, 17, 128, 256)), ("conv3t", (2, 5, 300, 128, 320)), ("s2", (3, 6, 10, 64, 320))):
        c = S.conv_case(geom, "unit", shape)
        full = S.ref_conv(geom, c.xh + c.xl, c.wh + c.wl, c.dims)
        share = (full.float() != c.want).double().mean().item()
        print(f"{geom} {shape}: the three-term sum differs from fp32(x . w) on {share:.3f} of the elements")
        assert share > 0.9, (geom, shape, share)


# ---- the split itself --------------------------------------------------------------------------------------------------------------------

def test_bit_split_agrees_with_the_conversions_and_rejects_the_planted_splits():
    """bit_split against torch's own round-to-nearest-even conversions on the planted patterns and on random ones (two independent
    statements of the same rounding), its truncation against exact_gemm_helpers.truncate_to — and the comparison used on the GPU
    (torch.equal on both halves) rejects hi truncated, lo taken from the truncated hi, and lo zeroed."""
    v = S.probe_values(S.gen(44), 65, 64).double().reshape(-1)
    pat = S._from_bits(torch.tensor(S.PROBE_BITS, dtype=torch.int64)).double()
    assert all(bool((v == p).any()) for p in pat)                              # every planted pattern is in the tensor
    hi, lo, ties = S.bit_split(v)
    t_hi = v.float().to(torch.bfloat16)
    t_lo = (v.float() - t_hi.float()).to(torch.bfloat16)
    assert torch.equal(hi, t_hi.double()) and torch.equal(lo, t_lo.double())
    assert int(ties.sum()) >= 4 and torch.isfinite(hi).all()
    sub = (lo != 0) & (lo.abs() < 2.0 ** -126)
    assert bool(sub.any()), "no lo is a bf16 subnormal"
    assert bool((hi[v == 0] == 0).all()) and bool((lo[v == 0] == 0).all())
    cut, _ = S.bf16_of_bits(v, truncate=True)
    assert torch.equal(cut, E.truncate_to(v, torch.bfloat16))
    want_hi, want_lo = hi.to(torch.bfloat16), lo.to(torch.bfloat16)
    for fault in ("hi_truncated", "lo_from_truncated_hi", "lo_zero"):
        h, l, _ = S.bit_split(v, fault)
        ok = torch.equal(h.to(torch.bfloat16), want_hi) and torch.equal(l.to(torch.bfloat16), want_lo)
        print(f"planted split {fault}: {'MISSED' if ok else 'rejected'}")
        assert not ok, fault
    # the exact sets see them through the convolution too: 1 + 2^-10 has nothing to truncate (hi is exact), so the split faults are
    # the producer tests' business; lo zeroed changes every output
    c = S.conv_case("conv9", "unit", (3, 5, 7, 64, 128))
    assert not torch.equal(S.ref3("conv9", c.xh, torch.zeros_like(c.xl), c.wh, c.wl, c.dims).float(), c.want)


# ---- the mutation check --------------------------------------------------------------------------------------------------------------------

# (geom, shape, (output row, tap, flat source token) of one border tap that is zero and reads `source` when its test is missing)
#   conv9: image 1, pixel (0, 2), tap (ky 0, kx 1) -> token r - W, the last row of image 0;
#          image 0, pixel (1, W - 1), tap (1, 2) -> token r + 1, the first pixel of the next row
#   conv3t: video 1, frame 0, pixel 3, tap kt 0 -> the last frame of video 0
#   s2:    image 0, output (2, 1) (centre (5, 3) of 6 x 10), tap (2, 1) -> the pad's zero row, token 63 = image 1, pixel (0, 3)
BORDERS = [("conv9", (3, 5, 7, 64, 128), [(35 + 2, 1, 35 + 2 - 7), (7 + 6, 5, 7 + 7)]),
           ("conv3t", (3, 3, 40, 64, 128), [(3 * 40 + 3, 0, 2 * 40 + 3)]),
           ("s2", (3, 6, 10, 64, 320), [(2 * 5 + 1, 7, 60 + 3)])]
RAGGED = [("conv9", (1, 4, 6, 64, 272), 256), ("conv9", (1, 4, 6, 64, 48), 128)]          # (.., column group)


def _parts(c):
    return S.im2col(c.geom, c.xh, c.dims), S.im2col(c.geom, c.xl, c.dims), S.weight_taps(c.wh), S.weight_taps(c.wl)


def _term_faults(c):
    """(name, the faulty contraction in fp64) for the faults every geometry has."""
    Ah, Al, Wh, Wl = _parts(c)
    clean = S.contract([Ah, Ah, Al], [Wh, Wl, Wh])
    # im2col and F.conv* agree: exactly on the exact sets, to fp64 summation order on gauss
    assert torch.equal(clean, c.ref) if c.kind in S.EXACT else (clean - c.ref).abs().max().item() <= 1e-12 * c.abs_ref.max().item()
    r, o, t, ch = c.rows // 2, c.Co - 3, c.taps // 2, 17                        # (the centre tap: valid at every pixel)
    one = torch.zeros_like(clean)
    one[r, o] = Al[r, t, ch] * Wh[o, t, ch]
    assert one[r, o] != 0
    yield "one x_lo . w_hi product dropped", clean - one
    yield "one x_lo . w_hi product doubled", clean + one
    yield "x_lo . w_lo in place of x_lo . w_hi", S.contract([Ah, Ah, Al], [Wh, Wl, Wl])
    yield "the weight thirds as (w_hi | w_hi | w_lo)", S.contract([Ah, Ah, Al], [Wh, Wh, Wl])
    yield "the fourth term added", S.contract([Ah, Ah, Al, Al], [Wh, Wl, Wh, Wl])
    z = Al.clone()
    z[r, t, ch] = 0
    yield "one x_lo element zeroed", S.contract([Ah, Ah, z], [Wh, Wl, Wh])
    z = Al.clone()
    z[:, t, :64] = Ah[:, t, :64]
    yield "one x_lo chunk read from the hi half", S.contract([Ah, Ah, z], [Wh, Wl, Wh])
    z = Al.clone()
    z[:, t, :64] = 0
    yield "one x_lo chunk zeroed", S.contract([Ah, Ah, z], [Wh, Wl, Wh])


def _border_faults(c, taps_list):
    Ah, Al, Wh, Wl = _parts(c)
    th, tl = c.xh.reshape(-1, c.C), c.xl.reshape(-1, c.C)
    for r, tap, src in taps_list:
        assert not Ah[r, tap].any() and not Al[r, tap].any(), "not a border tap"
        a, b = Ah.clone(), Al.clone()
        a[r, tap], b[r, tap] = th[src], tl[src]
        yield f"border tap {tap} of output row {r} reads token {src}", S.contract([a, a, b], [Wh, Wl, Wh])
        b = Al.clone()
        b[r, tap, 5] = tl[src, 5]
        yield f"border tap {tap} of output row {r} reads ONE lo element of token {src}", S.contract([Ah, Ah, b], [Wh, Wl, Wh])


def _rejected(c, mutant):
    """What the GPU test would see: the faulty kernel's fp32 output against the clean expected one."""
    return not torch.equal(mutant.float(), c.want)


@pytest.mark.parametrize("kind", S.EXACT)
def test_the_comparison_rejects_every_planted_fault(kind):
    found = {}
    for geom, shape, taps_list in BORDERS:
        c = S.conv_case(geom, kind, shape)
        assert not _rejected(c, c.ref.clone())                                  # (the clean recomputation passes)
        for name, m in list(_term_faults(c)) + list(_border_faults(c, taps_list)):
            found[f"{geom} {shape}: {name}"] = _rejected(c, m)
    # stride 2 with origin 0: the centre at (2 yo, 2 xo) — F.conv2d(padding 1, stride 2), cut to the Ho x Wo outputs
    shape = (2, 5, 7, 64, 128)
    c = S.conv_case("s2", kind, shape)
    N, H, W = c.dims
    Ho, Wo = S.out_hw("s2", H, W)
    o0 = lambda a, b: S._rows(F.conv2d(S._planes(a, N, H, W), b, stride=2, padding=1)[:, :, :Ho, :Wo])
    found[f"s2 {shape}: origin 0 instead of 1"] = _rejected(c, o0(c.xh, c.wh) + o0(c.xh, c.wl) + o0(c.xl, c.wh))
    # the stride-2 output IS the stride-1 one at [1::2, 1::2] (the GPU test asserts it on the kernel)
    full = S.conv_case("conv9", kind, shape)
    assert torch.equal(full.want.reshape(N, H, W, -1)[:, 1::2, 1::2].reshape(-1, c.Co), c.want)
    for geom, shape, group in RAGGED:
        c = S.conv_case(geom, kind, shape)
        Ah = S.im2col(geom, c.xh, c.dims)
        live = c.Co - (c.Co - 1) // group * group                               # live columns of the last group
        assert 0 < live < group and live % 16 == 0
        m = c.ref.clone()
        m[:, c.Co - 1] += Ah[:, 4, 0]                                           # a padding row holding 1.0 at (tap 4, channel 0) added to the last live column
        found[f"{geom} {shape}: a non-zero padded weight row reaches a live column"] = _rejected(c, m)
        m = c.ref.clone()
        m[:, c.Co - 16:] = 7.5                                                  # the output buffer's fill
        found[f"{geom} {shape}: the last live 16-column tile left unwritten"] = _rejected(c, m)
    for what, hit in found.items():
        print(f"mutation [{kind}] {what}: {'rejected' if hit else 'MISSED'}")
    assert all(found.values()), [k for k, v in found.items() if not v]


@pytest.mark.parametrize("kind", S.EXACT)
def test_the_weight_order_that_commutes_is_caught_on_the_packed_weight(kind):
    """The activations' logical channel axis is (x_hi | x_hi | x_lo): the weight thirds (w_lo | w_hi | w_hi) give x_hi . w_lo +
    x_hi . w_hi + x_lo . w_hi, the SAME sum — that order is no fault of the output and no output comparison can reject it (the order
    that is one, (w_hi | w_hi | w_lo), is among the planted faults above). What the GPU module asserts on the way rejects it: the
    packed weight has to equal pack_w3((w_hi, w_lo, w_hi)) element for element, in both contraction orders."""
    c = S.conv_case("conv9", kind, (1, 4, 6, 64, 272))
    Ah, Al, Wh, Wl = _parts(c)
    assert torch.equal(S.contract([Ah, Ah, Al], [Wl, Wh, Wh]), c.ref)
    for k_order in (0, 1):
        good = S.pack_w3((c.wh, c.wl, c.wh), 9, k_order, 256)
        assert good.shape == (512, 27 * 64) and not good[272:].any()
        assert not torch.equal(S.pack_w3((c.wl, c.wh, c.wh), 9, k_order, 256), good)
        assert not torch.equal(S.pack_w3((c.wh, c.wh, c.wl), 9, k_order, 256), good)
    assert not torch.equal(S.pack_w3((c.wh, c.wl, c.wh), 9, 0, 256), S.pack_w3((c.wh, c.wl, c.wh), 9, 1, 256))


# ---- what the Gaussian comparisons see ------------------------------------------------------------------------------------------------------

def test_what_the_max_norm_bar_and_the_gauss_bound_see():
    """Every planted fault on the gauss set, under the two Gaussian comparisons: the old bar — max|got - x . w| / max|x . w| < 3e-5
    against the fp64 convolution of the fp32 operands — and the derived elementwise bound against the three-term sum. Measured, see
    the module docstring; asserted: the clean three-term sum passes both; the old bar misses a single wrong lo element (in x_lo, or
    leaking through a border tap) from C = 128 on, and the fourth term; the elementwise bound rejects a leaking border pixel and (at
    C = 64) x_lo . w_lo in place of x_lo . w_hi; the exact sets reject all of them (the test above)."""
    seen = {}
    for geom, shape, taps_list in BORDERS + [("conv9", (1, 16, 17, 128, 256), [(0, 0, 18)]), ("conv3t", (2, 5, 300, 128, 320), [(7, 0, 1500 + 7)])]:
        c = S.conv_case(geom, "gauss", shape)
        full = S.ref_conv(geom, c.xh + c.xl, c.wh + c.wl, c.dims)
        scale = full.abs().max().item()
        rel = lambda m: (m - full).abs().max().item() / scale
        ratio = lambda m: ((m - c.ref).abs() / c.bound).max().item()
        assert rel(c.ref) < MAX_NORM_BAR and ratio(c.ref) <= 1.0
        print(f"gauss {geom} {shape}: clean three-term sum {rel(c.ref):.2e} of the output scale")
        for name, m in list(_term_faults(c)) + list(_border_faults(c, taps_list)):
            print(f"    {name}: max norm {rel(m):.2e} ({'seen' if rel(m) >= MAX_NORM_BAR else 'MISSED'}), worst ratio to the elementwise bound "
                  f"{ratio(m):.3g} ({'rejected' if ratio(m) > 1.0 else 'MISSED'})")
            seen[(geom, shape, name.split(" of output")[0] + (" ONE lo" if "ONE lo" in name else ""))] = (rel(m) >= MAX_NORM_BAR, ratio(m) > 1.0, c.C)
    for (geom, shape, name), (by_norm, by_bound, C) in seen.items():
        if name in ("one x_lo element zeroed", "the fourth term added") or "ONE lo" in name:
            assert not by_norm or C < 128, (geom, shape, name)                  # the gap: the old bar cannot see these
        if name.startswith("border tap") and "ONE lo" not in name:
            assert by_norm and by_bound, (geom, shape, name)
        if name == "x_lo . w_lo in place of x_lo . w_hi" and C == 64 and geom != "conv3t":
            assert by_bound, (geom, shape, name)
    # a truncating split of the activations (hi cut toward zero, lo its residue rounded): below the old bar as well
    c = S.conv_case("conv9", "gauss", (1, 16, 17, 128, 256))
    v = c.xh + c.xl
    cut, _ = S.bf16_of_bits(v, truncate=True)
    _, lo, _ = S.bit_split(v, "lo_from_truncated_hi")
    full = S.ref_conv("conv9", v, c.wh + c.wl, c.dims)
    e = (S.ref3("conv9", cut, lo, c.wh, c.wl, c.dims) - full).abs().max().item() / full.abs().max().item()
    print(f"gauss conv9 {c.shape}: truncating split {e:.2e} of the output scale")
    assert e < MAX_NORM_BAR

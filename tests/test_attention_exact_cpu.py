"""The data of tests/test_attention_exact_gpu.py on the CPU: the preconditions of the four constructions at every shape the GPU tests
run (tests/exact_attention_helpers.py asserts them while it builds a case), the coverage of the selector map j(i), a plain fp32
emulation of tiled flash attention that reproduces the expected outputs bit for bit, and a mutation check: eight faults planted in the
emulation, one at a time, each of which at least one data set has to notice at every ragged shape. No GPU code runs here."""
import math

import pytest
import torch

import exact_attention_helpers as E

HALF = ("bf16", "f16")
FLASH = E.FLASH4 + E.FLASH8
ALL_SETS = ("selector", "uniform", "pairs", "comb")
RAGGED = [s for s in FLASH if s[3] % E.KT or s[2] % 128]                   # every flash shape but (2, 1, 1024, 256)


@pytest.mark.parametrize("tag", list(E.DTYPES))
def test_every_case_of_the_gpu_tests_meets_its_preconditions(tag):
    """Building a case asserts: selector / pairs — the non-selected mass (against the range of |v|) and |s|max 2^-23 both at most 2^-14
    in log2 units, with the scale the f16 8-wave kernel rounds into Q included; uniform — no zero in v, zero column sums, sums below
    2^24, one score per (batch, head); pairs — at least one exact tie, more than half of the results need rounding (16-bit types).
    Here on top: the expected outputs are finite numbers of the type, the pairs sit in different tiles wherever there are two tiles
    and in different ring passes from 512 keys on, and the minimum code distance is what the construction promises."""
    dtype = E.DTYPES[tag]
    n = 0
    for name, build in E.every_forward_case(tag):
        c = build()
        n += 1
        assert c.want.dtype == dtype and torch.isfinite(c.want).all(), name
        Sk = c.k.shape[1]
        if c.kind == "selector":
            assert c.dist == c.D // E.code_bits(Sk) and (Sk == 1 or c.gap >= 40.0), (name, c.dist, c.gap)
        if c.kind == "pairs":
            assert c.cross_tile >= 1 or Sk <= E.KT, name
            assert c.cross_ring >= 1 or Sk < 512, name
            assert bool(c.tie.any()) or tag == "f32", name
    assert n >= (19 if tag == "f32" else 70)
    if tag != "f32":
        for name, build in E.every_backward_case(tag):
            c = build()
            assert torch.isfinite(c.dk_bound).all() and (c.dk_bound >= 0).all(), name
            if c.kind == "selector":               # what must vanish: dust, and for dk less than 1e-3 of what a wrong unit of P moves it by
                assert c.tiny < 2.0 ** -30 and c.eps < 1e-3, (name, c.tiny, c.eps)
                assert (bool((~c.chosen).any()) or "temporal" in name) and torch.equal(c.dv_want.double(), c.dv), name


@pytest.mark.parametrize("tag", HALF)
def test_the_selector_map_reaches_every_key_class(tag):
    """j(i) of every (batch, head) of every flash shape: the first and the last valid key, a key of the first 32-key block and of the
    first tile, rows whose key lies only in a later block / tile (the 8-wave kernel's fast path overflows for those and the block
    repeats with the online path), the ragged last tile, every ring slot the shape has, a key nobody chose and one chosen twice."""
    for B, H, Sq, Sk in FLASH + E.PACKED:
        c = E.selector_case(tag, B, H, Sq, Sk, 64)
        tiles = (Sk + E.KT - 1) // E.KT
        for row in c.cov:
            for cov in row:
                assert cov["first"] and cov["last"] and cov["first_tile"] and cov["ragged"], (Sq, Sk, cov)
                assert cov["unchosen"] and cov["multi"], (Sq, Sk, cov)
                assert cov["later_block"] and (cov["later"] or Sk <= E.KT), (Sq, Sk, cov)
                assert cov["slots"] == list(range(min(E.RING, tiles))), (Sq, Sk, cov)


def _row_sum_of(shape):
    return "mfma" if E.kernel_variant(shape[2], shape[3], 64, "bf16") == 16 else "valu"


@pytest.mark.parametrize("tag", HALF)
def test_the_emulation_reproduces_the_expected_outputs_bit_for_bit(tag):
    """Every flash shape, all four sets, the row sum taken both ways. selector: torch.equal; uniform: == 0; pairs and comb: torch.equal
    away from exact ties everywhere, and AT the ties too where the row sum is that of the rounded probabilities (l = 2 P exactly). With the
    row sum of the unrounded ones l = 2 (1 + e), e the rounding of the reference exponent, and a tie falls to either side: there the
    comparison admits both neighbours (and only there). lse within 4 x 2^-23 max(|lse|, 1) in the form the shape's kernel uses."""
    for shape in FLASH:
        for kind in ALL_SETS:
            c = E.SETS[kind](tag, *shape, 64)
            for row_sum in ("valu", "mfma"):
                out, lse = E.emulate_forward(c.q, c.k, c.v, c.H, tag, row_sum=row_sum)
                assert E.matches(c, out), (shape, kind, row_sum)
                if kind in ("pairs", "comb") and row_sum == "mfma":
                    assert E.pairs_mismatches(c, out, strict=True) == 0, shape
                if row_sum == _row_sum_of(shape):
                    err = ((lse - c.lse).abs() / c.lse.abs().clamp(min=1.0)).max().item()
                    assert err <= 4 * 2.0 ** -23, (shape, kind, err)
    for shape in E.PACKED:                                                 # a q that carries D^-1/2 log2 e already
        for kind in ALL_SETS:
            c = E.SETS[kind](tag, *shape, 64, "q_log2")
            out, _ = E.emulate_forward(c.q, c.k, c.v, c.H, tag, mode="q_log2", row_sum=_row_sum_of(shape))
            assert E.matches(c, out), (shape, kind)


@pytest.mark.parametrize("tag", HALF)
@pytest.mark.parametrize("fault", E.FAULTS)
def test_a_planted_fault_is_noticed_at_every_ragged_shape(tag, fault):
    """The last valid key dropped; the clamped copy of key Sk - 1 counted; one whole tile skipped; two keys swapped inside a 32-key block
    of P V only; the keys and values of the neighbouring head (of the neighbouring batch entry where there is one head); the rescale
    omitted when the maximum moves; P truncated instead of rounded. Each has to change the verdict of at least one set, at every ragged
    shape, in both row-sum forms — truncation in that of the 4-wave kernel only (P = 2^(rounding of the exponent), the one place where
    P is not a number of the type: where the exponent is subtracted exactly P is 1 and truncation has nothing to cut).
    A shape with one head and one batch entry has no neighbour to swap with, and with one key tile the maximum never moves: those
    two faults cannot be planted there."""
    for shape in RAGGED:
        if fault == "swap_heads" and shape[0] * shape[1] == 1 or fault == "no_rescale" and shape[3] <= E.KT:
            continue
        for row_sum in ("valu",) if fault == "truncate_p" else ("valu", "mfma"):
            seen = []
            for kind in ALL_SETS:
                c = E.SETS[kind](tag, *shape, 64)
                out, _ = E.emulate_forward(c.q, c.k, c.v, c.H, tag, row_sum=row_sum, fault=fault)
                if not E.matches(c, out):
                    seen.append(kind)
            assert seen, (fault, shape, row_sum)


@pytest.mark.parametrize("tag", HALF)
def test_a_query_row_past_the_end_in_the_dv_sums_is_noticed(tag):
    """The backward's key-major sums dv = P^T dout on the selector set: the emulation equals the exact integer sums (where the sum
    is zero bf16 keeps the 2^-gap dust of the other
    rows' probabilities, bounded by the case's `tiny`; f16 rounds it to 0), and the clamped copy
    of query row Sq - 1 added once more moves dv[j(Sq - 1)] by dout[Sq - 1], never 0."""
    for shape in RAGGED:
        c = E.selector_bwd_case(tag, *shape)
        f = c.fwd
        assert E.dv_mismatches(c, E.emulate_dv(f.q, f.k, c.dout, f.lse, c.H, tag), tag) == 0, shape
        assert E.dv_mismatches(c, E.emulate_dv(f.q, f.k, c.dout, f.lse, c.H, tag, leak_row=True), tag) > 0, shape


def test_the_helpers_arithmetic():
    """Code distance, magnitudes, the zero-sum columns and the tie / spacing arithmetic."""
    assert [E.code_magnitudes(D) for D in (64, 32, 16)] == [(5.0, 8.0), (7.0, 7.0), (9.0, 9.0)]
    for n, D in ((2060, 64), (300, 64), (37, 32), (64, 16), (16, 64), (1, 64)):
        cd, r = E.codes(n, D)
        assert r == D // E.code_bits(n) and cd.abs().eq(1).all()
        if n > 1:
            ham = (D - cd @ cd.T) / 2 + torch.eye(n) * D
            assert ham.min().item() >= r, (n, D, ham.min().item())
    g = E.gen(9)
    for n in (2, 3, 33, 64, 257):
        v = E.zero_sum_columns(g, (2, 3), n, 16)
        assert v.shape == (2, 3, n, 16) and (v != 0).all() and v.abs().max() <= 3 and (v.sum(2) == 0).all()
    x = torch.tensor([257.0, 259.0, 2049.0, 2051.0], dtype=torch.float64)
    assert E.is_tie(x[:2], torch.bfloat16).all() and E.is_tie(x[2:], torch.float16).all()
    assert E.truncate_to(torch.tensor([259.0, -259.0, 0.998]).double(), torch.bfloat16).tolist() == [258.0, -258.0, 0.99609375]
    assert E.kernel_variant(1024, 256, 64, "bf16") == 16 and E.kernel_variant(1023, 256, 64, "bf16") == 4
    assert E.kernel_variant(40, 32, 64, "bf16") == 0 and E.kernel_variant(40, 33, 64, "bf16") == 4
    assert E.kernel_variant(40, 33, 64, "f32") == 0
    assert math.isclose(E.selector_case("bf16", 1, 1, 1279, 2060, 64).s_match.max().item(), 40 * 64 * 0.125 * E.LOG2E)

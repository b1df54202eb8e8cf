"""Data with exactly one right answer for the split-operand first-stage convolutions (csrc/linear_n320.hip: mvi_conv3x3_split3_f32,
mvi_conv3t_split3_f32, mvi_conv3x3_s2_split3_f32) and their operand producer (csrc/groupnorm_tokens.hip, gt_apply_split_kernel), the
fp64 references of tests/test_split3_exact_gpu.py and the case lists it shares with tests/test_split3_exact_cpu.py (which checks every
precondition stated here on the CPU and shows what the comparison rejects). Pure torch on the CPU; nothing outside the repository is
read. gen, signs, mags, ulp_of and truncate_to are those of tests/exact_gemm_helpers.py.

The kernels compute x_hi . w_hi + x_hi . w_lo + x_lo . w_hi in fp32 on the bf16 matrix pipe, v = hi + lo the split of an fp32 operand
into two bf16 numbers. Three data sets (split_data), every one as (x_hi, x_lo, w_hi, w_lo) in fp64:
  * unit   hi in {-1, +1}, lo in {-2^-10, +2^-10}: lo lies strictly inside half a bf16 ulp of +-1 on both sides (2^-9 above, 2^-10
           below), so the split of hi + lo is (hi, lo) with no tie. Every product of the three kept terms is a multiple of
           u = 2^-10 and one contraction element adds at most (1024 + 2) u: below 2^24 u in all (asserted per case on the absolute
           values) every partial sum in every order is an fp32 number, and the fp32 output has ONE right bit pattern. The omitted
           x_lo . w_lo term is +-2^-20: the three-term sum differs from fp32(x . w) on most elements.
  * mags   hi in +-{2, 3}, lo in +-{1, 2, 3} 2^-10 (the bf16 spacing from 2 to 4 is 2^-6, half of it 8 u): unequal weights. One
           element adds up to (9 * 1024 + 18) u, so the set exists only up to 1816 contraction elements; conv_case returns None past
           its bound and the case runs the unit set alone.
  * gauss  the Gaussian operands of the existing tests (activations randn with per-channel scales in [0.2, 3.2], weights
           randn K^-1/2), for a derived ELEMENTWISE bound. An fp32 value v is replaced by hi + lo of its own split — 16 significant
           bits, always an fp32 number — and split again: that second split is a fixed point (hi + lo == v exactly), so one fp32
           tensor stands for both halves in every set, and split3_weight is handed (w_hi + w_lo).float() everywhere.

bit_split is the split on the fp32 BIT PATTERN (round to nearest even by integer arithmetic), independent of hip_ops.split_hi_lo and of
torch's conversions: what the preconditions and the expected outputs of the producer tests are taken from."""
import functools

import torch
import torch.nn.functional as F

import exact_gemm_helpers as E
from exact_gemm_helpers import gen, mags, signs, truncate_to, ulp_of  # noqa: F401 (re-exported to the two test modules)

U = 2.0 ** -10                                                   # the unit of the exact sets
EXACT = ("unit", "mags")
KINDS = EXACT + ("gauss",)
TAPS = {"conv9": 9, "conv3t": 3, "s2": 9}
BF16 = torch.bfloat16


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---- the split on the bit pattern -------------------------------------------------------------------------------------------------------

def _bits(v32):
    """fp32 tensor -> its bit patterns as int64 in [0, 2^32)."""
    return v32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(b):
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(torch.float32)


def bf16_of_bits(v, truncate=False):
    """v (fp64 holding fp32 numbers) -> (the nearest bf16 number, ties to even — or v cut toward zero —, as fp64; the mask of exact
    ties). Sign-magnitude patterns: adding to the low bits moves the magnitude, whatever the sign; subnormals are ordinary patterns."""
    v32 = v.float()
    assert torch.equal(v32.double(), v), "not an fp32 number"
    b = _bits(v32)
    low = b & 0xFFFF
    r = b if truncate else b + 0x7FFF + ((b >> 16) & 1)
    return _from_bits(r - (r & 0xFFFF)).double(), low == 0x8000


def bit_split(v, fault=None):
    """(hi, lo, ties) of fp64 v holding fp32 numbers: hi = bf16(v), lo = bf16(v - hi), both to nearest even on the bit pattern (the
    residue of two fp32 numbers this close is an fp32 number: the subtraction is exact). `fault` plants what the CPU module must see
    rejected: 'hi_truncated' (hi cut toward zero, lo as it should be), 'lo_from_truncated_hi' (hi right, lo the residue of the cut
    hi), 'lo_zero'."""
    hi, tie_hi = bf16_of_bits(v)
    cut, _ = bf16_of_bits(v, truncate=True)
    lo, tie_lo = bf16_of_bits(v - (cut if fault == "lo_from_truncated_hi" else hi))
    if fault == "hi_truncated":
        hi = cut
    if fault == "lo_zero":
        lo = torch.zeros_like(lo)
    return hi, lo, tie_hi | tie_lo


def check_split(hi, lo, tie_free):
    """The preconditions on one operand, every element: hi and lo are bf16 numbers, hi + lo is an fp32 number, and the split of that
    number on its bit pattern is exactly (hi, lo) — with no tie on the way for the exact sets. -> hi + lo."""
    assert torch.equal(hi.to(BF16).double(), hi) and torch.equal(lo.to(BF16).double(), lo), "a half is no bf16 number"
    v = hi + lo
    assert torch.equal(v.float().double(), v), "hi + lo is no fp32 number"
    h2, l2, ties = bit_split(v)
    assert torch.equal(h2, hi) and torch.equal(l2, lo), "the split of hi + lo on the bit pattern is not (hi, lo)"
    assert not (tie_free and bool(ties.any())), "a tie in an exact set"
    return v


def _fixed_point(v32):
    """fp32 -> (hi, lo) with hi + lo an fp32 number whose split is (hi, lo) again (see the module docstring)."""
    hi, lo, _ = bit_split(v32.double())
    hi, lo, _ = bit_split((hi + lo).float().double())
    return hi, lo


def split_data(kind, g, x_shape, w_shape):
    """(x_hi, x_lo, w_hi, w_lo) in fp64. x token-major [..., C]; w [C_out, C, 3, 3] or [C_out, C, 3, 1, 1]."""
    if kind == "unit":
        return signs(g, *x_shape), signs(g, *x_shape) * U, signs(g, *w_shape), signs(g, *w_shape) * U
    if kind == "mags":
        two3 = lambda s: signs(g, *s) * torch.randint(2, 4, s, generator=g).double()
        lo = lambda s: signs(g, *s) * mags(g, *s) * U
        return two3(tuple(x_shape)), lo(tuple(x_shape)), two3(tuple(w_shape)), lo(tuple(w_shape))
    if kind == "gauss":
        C = x_shape[-1]
        K = 1
        for d in w_shape[1:]:
            K *= d
        x = torch.randn(*x_shape, generator=g) * torch.rand(*([1] * (len(x_shape) - 1)), C, generator=g).mul(3).add(0.2)
        w = torch.randn(*w_shape, generator=g) * K ** -0.5
        return _fixed_point(x) + _fixed_point(w)
    raise ValueError(kind)


# ---- the three geometries on token-major data ------------------------------------------------------------------------------------------

def _planes(tok, N, H, W):
    return tok.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _rows(y):
    """[N, C_out, Ho, Wo] -> [N Ho Wo, C_out], the kernels' output."""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def ref_conv(geom, tok, w, dims):
    """fp64. conv9: 3x3 / padding 1 of tok [N, H W, C], dims (N, H, W). s2: 3x3 / stride 2 over F.pad(x, (0, 1, 0, 1)), same dims.
    conv3t: (3,1,1) / padding (1,0,0) of tok [(B T), S, C], dims (B, T, S). -> [rows, C_out]."""
    if geom == "conv9":
        return _rows(F.conv2d(_planes(tok, *dims), w, padding=1))
    if geom == "s2":
        return _rows(F.conv2d(F.pad(_planes(tok, *dims), (0, 1, 0, 1)), w, stride=2))
    B, T, S = dims
    return E.ref_conv3t(tok.reshape(B * T, S, -1), w, None, B, T).reshape(B * T * S, -1)


def ref3(geom, xh, xl, wh, wl, dims):
    """The three kept terms, each an fp64 convolution of its own."""
    return ref_conv(geom, xh, wh, dims) + ref_conv(geom, xh, wl, dims) + ref_conv(geom, xl, wh, dims)


def abs3(geom, xh, xl, wh, wl, dims):
    """sum |terms|: the same operation on absolute values."""
    return ref3(geom, xh.abs(), xl.abs(), wh.abs(), wl.abs(), dims)


def out_hw(geom, H, W):
    return ((H - 2) // 2 + 1, (W - 2) // 2 + 1) if geom == "s2" else (H, W)


def gauss_bound(abs_ref, K_total):
    """|got - ref3| <= 2 K_total 2^-24 sum|terms|: n u sum|terms| for any fp32 order of n exactly representable products, doubled for
    the matrix pipe (exact_gemm_helpers.elementwise_bound without the store's rounding: the output IS the fp32 accumulator)."""
    return 2.0 * K_total * 2.0 ** -24 * abs_ref


# ---- the case lists ------------------------------------------------------------------------------------------------------------------------

# (N, H, W, C, C_out): centre tap only, one live row of a 256-row block, group 128 padded from 64; three images in one row block; the
# block boundary inside an image row; the 320-column form with a ragged second block; the 256-column group; two 256-column groups at
# the longest contraction (unit only, by the bound); two groups, the second with 16 live columns; group 128 with three live tiles
CONV9 = [(1, 1, 1, 64, 64), (3, 5, 7, 64, 128), (1, 2, 200, 64, 64), (2, 9, 15, 64, 320), (1, 16, 17, 128, 256), (1, 3, 3, 512, 512),
         (1, 4, 6, 64, 272), (1, 4, 6, 64, 48)]
# (B, T, pixels, C, C_out): one frame; two frames; three videos in one block; either side of the W % 256 == 0 frame-major walk; the
# 320-column form; the longest contraction (the mags set fits: 2 x 512 elements)
CONV3T = [(1, 1, 5, 64, 64), (2, 2, 7, 64, 64), (3, 3, 40, 64, 128), (1, 3, 256, 64, 64), (1, 3, 257, 64, 64), (2, 5, 300, 128, 320),
          (1, 2, 3, 512, 256)]
# (N, H, W, C, C_out): one output pixel each; odd sizes (the pad's zero row and column are live taps, the last input row and column are
# reached only as taps); the 320-column form; 289 output rows, two blocks
S2 = [(1, 2, 2, 64, 64), (1, 3, 3, 64, 64), (2, 5, 7, 64, 128), (3, 6, 10, 64, 320), (1, 34, 34, 64, 64)]
CASES = {"conv9": CONV9, "conv3t": CONV3T, "s2": S2}
MAGS_ABSENT = {("conv9", (1, 3, 3, 512, 512))}                    # where conv_case("mags") is None: asserted by the CPU module


def _data(geom, kind, shape):
    """The operands of a case. conv9 and s2 share them at the same shape (the stride-2 result is the stride-1 one at [1::2, 1::2])."""
    n, a, b, C, Co = shape
    taps = TAPS[geom]
    g = gen(41, taps, n, a, b, C, Co, KINDS.index(kind))
    x_shape = (n, a * b, C) if taps == 9 else (n * a, b, C)
    w_shape = (Co, C, 3, 3) if taps == 9 else (Co, C, 3, 1, 1)
    return split_data(kind, g, x_shape, w_shape)


@functools.lru_cache(maxsize=None)
def conv_case(geom, kind, shape):
    """One launch in mode "split3". Fields: xh, xl [.., C] token-major and wh, wl in fp64, w32 = (wh + wl).float() (what split3_weight
    is handed), dims, rows, K_total = 3 taps C, ref [rows, C_out] (fp64, the three-term sum), abs_ref, and `want` (fp32, the one right
    output) for the exact sets or `bound` for gauss. The preconditions are asserted on the way; None where the mags set does not fit."""
    n, a, b, C, Co = shape
    xh, xl, wh, wl = _data(geom, kind, shape)
    exact = kind in EXACT
    x = check_split(xh, xl, exact)
    w = check_split(wh, wl, exact)
    dims = (n, a, b)
    ref = ref3(geom, xh, xl, wh, wl, dims)
    abs_ref = abs3(geom, xh, xl, wh, wl, dims)
    Ho, Wo = out_hw(geom, a, b)
    rows = n * Ho * Wo
    assert ref.shape == (rows, Co)
    c = Case(geom=geom, kind=kind, shape=shape, dims=dims, rows=rows, C=C, Co=Co, taps=TAPS[geom], K_total=3 * TAPS[geom] * C,
             xh=xh, xl=xl, wh=wh, wl=wl, x32=x.float(), w32=w.float(), ref=ref, abs_ref=abs_ref)
    if exact:
        if abs_ref.max().item() / U >= 2 ** 24:
            assert kind == "mags", "the unit set must fit every shape"
            return None
        assert torch.equal(ref, torch.round(ref / U) * U), "a reference element is no multiple of the unit"
        c.want = ref.float()
        assert torch.equal(c.want.double(), ref)
    else:
        c.bound = gauss_bound(abs_ref, c.K_total)
        assert c.bound.min().item() > 0
    return c


@functools.lru_cache(maxsize=None)
def int_case(geom, tag, shape):
    """One launch in mode "bf16" / "f16" (terms = 1): x, w in +-{1, 2, 3} with i.i.d. signs, both numbers of either type. The output is
    fp32 and every sum stays below 9 * 9 * 512 < 2^24: nothing rounds, one right bit pattern."""
    n, a, b, C, Co = shape
    taps = TAPS[geom]
    g = gen(42, taps, n, a, b, C, Co, tag == "f16")
    x = signs(g, *((n, a * b, C) if taps == 9 else (n * a, b, C))) * mags(g, *((n, a * b, C) if taps == 9 else (n * a, b, C)))
    w = signs(g, *((Co, C, 3, 3) if taps == 9 else (Co, C, 3, 1, 1)))
    w = w * mags(g, *w.shape)
    dims = (n, a, b)
    ref = ref_conv(geom, x, w, dims)
    assert ref_conv(geom, x.abs(), w.abs(), dims).max().item() < 2 ** 24 and torch.equal(ref, ref.round())
    want = ref.float()
    assert torch.equal(want.double(), ref)
    Ho, Wo = out_hw(geom, a, b)
    return Case(geom=geom, kind="int", shape=shape, dims=dims, rows=n * Ho * Wo, C=C, Co=Co, taps=taps, x=x, w=w, ref=ref, want=want)


def every_case():
    """(name, builder) of every split3 case of the GPU module; a builder returns the Case or None (mags past its bound)."""
    out = []
    for geom, shapes in CASES.items():
        for shape in shapes:
            for kind in KINDS:
                out.append((f"{geom} {kind} {shape}", functools.partial(conv_case, geom, kind, shape)))
            for tag in E.DTYPES:
                out.append((f"{geom} int {tag} {shape}", functools.partial(int_case, geom, tag, shape)))
    return out


# ---- the contraction written out: the fp32 restatement and the planted faults -----------------------------------------------------------

def im2col(geom, tok, dims):
    """tok -> [rows, taps, C] in fp64: tap (ky, kx) (or kt) of every output row, zeros where the tap leaves the image / video."""
    if geom in ("conv9", "s2"):
        x = _planes(tok, *dims)
        C = x.shape[1]
        cols = F.unfold(x, 3, padding=1) if geom == "conv9" else F.unfold(F.pad(x, (0, 1, 0, 1)), 3, stride=2)
        return cols.reshape(dims[0], C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9, C)
    B, T, S = dims
    v = F.pad(tok.reshape(B, T, S, -1), (0, 0, 0, 0, 1, 1))
    return torch.stack([v[:, t:t + T] for t in range(3)], dim=3).reshape(B * T * S, 3, -1)


def weight_taps(w):
    """[C_out, C, 3, 3] or [C_out, C, 3, 1, 1] -> [C_out, taps, C]."""
    return w.reshape(w.shape[0], w.shape[1], -1).permute(0, 2, 1)


def contract(parts_x, parts_w):
    """sum over the logical channel axis: x parts [rows, taps, C] and w parts [C_out, taps, C], pairwise, in fp64."""
    A = torch.cat(parts_x, dim=2).reshape(parts_x[0].shape[0], -1)
    Bm = torch.cat(parts_w, dim=2).reshape(parts_w[0].shape[0], -1)
    return A @ Bm.t()


def restate_f32(c, g, chunk=64):
    """The kernel's contraction restated in plain fp32: logical channel axis (x_hi | x_hi | x_lo) against (w_hi | w_lo | w_hi), cut
    into chunks of 64 taken in a SHUFFLED order, every chunk an fp32 matrix product added to an fp32 accumulator."""
    Ah, Al = im2col(c.geom, c.xh, c.dims), im2col(c.geom, c.xl, c.dims)
    Wh, Wl = weight_taps(c.wh), weight_taps(c.wl)
    A = torch.cat([Ah, Ah, Al], dim=2).reshape(c.rows, -1).float()
    Bm = torch.cat([Wh, Wl, Wh], dim=2).reshape(c.Co, -1).float()
    acc = torch.zeros(c.rows, c.Co, dtype=torch.float32)
    for i in torch.randperm(A.shape[1] // chunk, generator=g).tolist():
        acc += A[:, i * chunk:(i + 1) * chunk] @ Bm[:, i * chunk:(i + 1) * chunk].t()
    return acc


def pack_w3(parts, taps, k_order, group):
    """The layout split3_weight must produce, written out independently of it: parts = (w_hi, w_lo, w_hi) (or (w,) for terms = 1) joined
    on the channel axis, [C_out][taps][channels] tap-major — or, 3x3 with k_order 1, [C_out][channels / 64][9][64] — and zero rows up
    to a whole number of column groups. fp64 in, fp64 out."""
    t = torch.cat([weight_taps(p) for p in parts], dim=2)         # [Co, taps, Cl]
    Co, _, Cl = t.shape
    if taps == 9 and k_order == 1:
        t = t.reshape(Co, 9, Cl // 64, 64).permute(0, 2, 1, 3)
    t = t.reshape(Co, -1)
    pad = -Co % group
    return torch.cat([t, t.new_zeros(pad, t.shape[1])]) if pad else t


# ---- planted fp32 values for the plain split ----------------------------------------------------------------------------------------------

PROBE_BITS = [
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,              # exact bf16 ties, even and odd hi (down, up), both signs
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF807FFF, 0xBF818001,     # one fp32 ulp on either side of a tie
    0x3FFFFFFF, 0x3FFFFF80, 0x3FFF8000, 0xBFFFFFFF, 0x477FFFFF,  # just below a power of two: hi rounds up into the next binade
    0x4049FFFF, 0xC049FFFF, 0x3E2AFFFF, 0x0080FFFF,              # low 16 bits all ones
    0x00000000, 0x80000000,                                      # +-0
    0x03804800, 0x03804200, 0x03804080, 0x83804800, 0x01004000,  # lo is a bf16 subnormal: exact, a tie of its own, rounded; hi 2^-125
    0x7F7F0000, 0x7F7F7FFF, 0xFF7F7FFF,                          # the largest values whose hi stays finite
]


def probe_values(g, S, C):
    """[1, S, C] fp32: the planted patterns cycled from a different offset in every row, every third element a random pattern with an
    exponent field in [96, 159] (|v| from 2^-31 to 2^33): a row or column read from the wrong place changes the output."""
    n = S * C
    pat = torch.tensor(PROBE_BITS, dtype=torch.int64)
    idx = (torch.arange(n) + 7 * (torch.arange(n) // C)) % len(pat)
    b = pat[idx]
    rnd = (torch.randint(0, 2, (n,), generator=g) << 31) | (torch.randint(96, 160, (n,), generator=g) << 23) | torch.randint(0, 1 << 23, (n,), generator=g)
    b = torch.where(torch.arange(n) % 3 == 2, rnd, b)
    v = _from_bits(b).reshape(1, S, C)
    assert torch.isfinite(v).all()
    return v

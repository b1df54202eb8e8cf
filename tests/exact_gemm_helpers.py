"""Data with exactly one right answer for the half-precision MFMA GEMM and convolution kernels (csrc/linear_n320.hip, csrc/ff_geglu.hip,
csrc/stem_conv.hip), the fp64 references of tests/test_gemm_exact_gpu.py and the case lists it shares with tests/test_gemm_exact_cpu.py
(which checks every precondition stated here on the CPU and shows that the comparison notices six planted faults). Pure torch on the CPU;
nothing outside the repository is read.

Three data sets:
  * parity    x, w in {-1, +1}, even integer bias, even K_total: every exact output is an EVEN integer, and small enough to be a bf16 /
              f16 number. fp32 accumulation of integers below 2^24 is exact in any order and any K split, so the kernel's output has
              one right bit pattern: ref.to(dtype). A dropped term makes an output odd; a doubled or misplaced one moves it by 2.
  * rounding  x, w in {+-1, +-2, +-3}, integer bias in [-8, 8] (plus a large multiple of the type's ulp where K_total is too short to
              carry the sums past the type's integer range, see rounding_bias_scale): sums stay below 2^24, so the fp32 accumulator is
              still exact, but most results are NOT numbers of the storage type and some are exact ties: the store has to round to
              nearest even, once. All elements of one row of x (one image, one pixel column of a video) share a sign, and so do all
              elements of one output channel of w: i.i.d. signs would leave |sum| ~ 4.7 sqrt(K), inside the integers bf16 holds exactly
              (|v| <= 256) for every K of these tests, and nothing would round. Dropped terms are the parity set's business.
  * gauss     the Gaussian inputs of the existing tests, for a derived ELEMENTWISE bound (elementwise_bound): integers do not reach
              the fractional bits.
GEGLU gates: see geglu_case."""
import functools

import torch
import torch.nn.functional as F

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}                # significand bits, the hidden one included
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}             # exponent of the smallest normal number


def gen(*key):
    """A generator seeded by the case: a test never depends on which other tests ran."""
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def signs(g, *shape):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def mags(g, *shape):
    return torch.randint(1, 4, shape, generator=g).double()


def ulp_of(v, dtype):
    """The spacing of `dtype` at |v| (fp64 tensor in, fp64 out): 2^(e - p + 1) for 2^e <= |v| < 2^(e + 1), the subnormal spacing below."""
    _, ex = torch.frexp(v.abs().double())                        # |v| = m 2^ex, m in [0.5, 1)
    ex = torch.clamp(ex, min=MIN_EXP[dtype] + 1)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - SIG_BITS[dtype])


def truncate_to(v, dtype):
    """v rounded TOWARD ZERO to `dtype` (the planted fault of the mutation check), as fp64."""
    u = ulp_of(v, dtype)
    return torch.sign(v) * torch.floor(v.abs() / u) * u


def needs_rounding(ref, dtype):
    return ref.to(dtype).double() != ref


def is_tie(ref, dtype):
    """Exactly halfway between two neighbouring numbers of `dtype`."""
    return (ref - ref.to(dtype).double()).abs() == 0.5 * ulp_of(ref, dtype)


def expect_parity(ref, dtype, even=True):
    """The preconditions of the parity set, on EVERY element: an integer (even where K_total is), exactly a number of `dtype`.
    -> the one right output."""
    assert torch.equal(ref, ref.round()), "parity data: a reference element is no integer"
    if even:
        assert torch.equal(ref % 2, torch.zeros_like(ref)), "parity data: a reference element is odd"
    want = ref.to(dtype)
    assert torch.equal(want.double(), ref), f"parity data: max |ref| = {ref.abs().max().item()} is not representable in {dtype}"
    return want


def expect_rounding(ref, dtype):
    """The preconditions of the rounding set: finite in `dtype`, below 2^24, at least one exact tie, more than half of the elements
    need rounding. -> the one right output."""
    want = ref.to(dtype)
    assert torch.isfinite(want).all(), f"rounding data: the reference overflows {dtype}"
    assert ref.abs().max().item() < 2 ** 24
    frac = needs_rounding(ref, dtype).double().mean().item()
    ties = int(is_tie(ref, dtype).sum())
    assert ties >= 1 and frac > 0.5, f"rounding data: {ties} ties, {frac:.3f} of the elements need rounding in {dtype}"
    return want


def rounding_bias_scale(K_total, dtype):
    """0 where the sums of the rounding set (|sum| ~ 4 K_total) pass the integers `dtype` holds exactly far enough that more than half
    of them need rounding; otherwise the multiple of the type's spacing the bias carries them there with (the issue's `scaled bias`):
    bf16 rounds from 256 on, three values in four from 512 (K_total >= 128); f16 from 2048, three in four from 4096 (K_total >= 1280)."""
    if dtype == torch.bfloat16:
        return 0 if K_total >= 128 else 2048
    return 0 if K_total >= 1280 else 16384


def gemm_data(kind, g, x_shape, x_sign_shape, w_shape, K_total, dtype, with_bias=True, odd_bias=False):
    """(x, w, b) in fp64, every value a number of `dtype`; None where the rounding set cannot be built (no bias to carry a short K_total
    past the type's exact integers: that case runs the other sets only). w_shape[0] is the output-channel axis."""
    n_out = w_shape[0]
    w_sign_shape = (n_out,) + (1,) * (len(w_shape) - 1)
    if kind == "parity":
        x, w = signs(g, *x_shape), signs(g, *w_shape)
        b = torch.randint(-4, 5, (n_out,), generator=g).double() * 2 + (1.0 if odd_bias else 0.0)
    elif kind == "rounding":
        scale = rounding_bias_scale(K_total, dtype)
        if scale and not with_bias:
            return None
        x = signs(g, *x_sign_shape) * mags(g, *x_shape)
        ws = signs(g, *w_sign_shape)
        w = ws * mags(g, *w_shape)
        b = torch.randint(-8, 9, (n_out,), generator=g).double() + scale * ws.reshape(-1)
    elif kind == "gauss":
        x = (torch.randn(*x_shape, generator=g) * 1.2).to(dtype).double()
        w = (torch.randn(*w_shape, generator=g) * K_total ** -0.5).to(dtype).double()
        b = (torch.randn(n_out, generator=g) * 0.3).to(dtype).double()
    else:
        raise ValueError(kind)
    return x, w, (b if with_bias else None)


def elementwise_bound(ref, abs_ref, K_total, dtype):
    """The derived per-element bound of an fp32-accumulated, once-rounded output: |got - ref| <= cap + ulp(|ref| + cap) / 2 with
    cap = 2 K_total 2^-24 (|x| (*) |w| + |b|) — any fp32 summation order of K_total exactly representable products errs by at most
    K_total 2^-24 sum|terms|, doubled for the matrix pipe's internal accumulation (the cap of the wgrad tests); abs_ref is the same
    operation on absolute values, bias included."""
    cap = 2.0 * K_total * 2.0 ** -24 * abs_ref
    return cap + 0.5 * ulp_of(ref.abs() + cap, dtype)


class Case:
    """One launch: inputs (fp64 holding numbers of the dtype), the fp64 reference `ref`, and either the one right output `want`
    (parity / rounding / gates) or the per-element `bound` (gauss). Everything in the layout of the F.* reference."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _finish(kind, dtype, ref, abs_ref_fn, K_total, even=True, **kw):
    kw["K_total"] = K_total
    if kind == "parity":
        return Case(kind=kind, ref=ref, want=expect_parity(ref, dtype, even), **kw)
    if kind == "rounding":
        return Case(kind=kind, ref=ref, want=expect_rounding(ref, dtype), **kw)
    return Case(kind=kind, ref=ref, bound=elementwise_bound(ref, abs_ref_fn(), K_total, dtype), **kw)


def _abs(t):
    return None if t is None else t.abs()


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------

def tokens(x):
    """[N, C, H, W] -> token-major [N, H W, C]."""
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N, H * W, C).contiguous()


def planes(tok, H, W):
    """[N, H W, C] -> [N, C, H, W]."""
    N, _, C = tok.shape
    return tok.reshape(N, H, W, C).permute(0, 3, 1, 2)


def ref_conv3t(tok, w, b, B, T):
    """The (3, 1, 1) / padding (1, 0, 0) frame convolution of tok [(B T), S, C] with w [Co, C, 3, 1, 1] through F.conv3d on b c t h w."""
    _, S, C = tok.shape
    x5 = tok.reshape(B, T, S, 1, C).permute(0, 4, 1, 2, 3)
    return F.conv3d(x5, w, b, 1, (1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(B * T, S, w.shape[0])


# ---- the case lists (tests/test_gemm_exact_gpu.py runs them, tests/test_gemm_exact_cpu.py checks their preconditions) -----------------

ROWS = (1, 255, 256, 257, 513)                 # one row; a block less one; one block; a block and a row; two blocks and a row
# (rows, K, N, with_bias, strided): K = 128 two chunks (the minimum), 192 one full ring of three, 256 wraps the ring by one, 704 an odd
# count that wraps; N = 320 / 640 one and two column groups; bias and the strided view alternate over the cross product
LINEAR_N320 = [(r, K, N, (i + j + n) % 2 == 0, (i + 2 * j + n) % 3 == 0)
               for i, r in enumerate(ROWS) for j, K in enumerate((128, 192, 256, 704)) for n, N in enumerate((320, 640))]
# K = 1280 (20 chunks, the production contraction): f16 sums pass 2048 inside the K loop, so a partial sum kept in f16 between chunks
# is visible to the rounding set there too (at K <= 704 only bf16 sees it), and f16 has a bias-free rounding case
LINEAR_N320 += [(257, 1280, 640, True, False), (257, 1280, 320, False, False)]
LINEAR_N320_GAUSS = [(513, 704, 640, True, True), (257, 1280, 640, True, False)]
# (rows, N, with_bias, strided), K = 320: N = 128 the minimum, 192 an odd number of 64-wide pairs, 960 the packed q | k | v width
LINEAR_K320 = [(r, N, (i + n) % 2 == 0, (i + n) % 3 == 1) for i, r in enumerate(ROWS) for n, N in enumerate((128, 192, 960))]
LINEAR_K320_GAUSS = [(513, 960, True, False)]
# (rows, inner), K = 320: 2 steps, 3 steps (the two accumulator sets end on the other one), the production width
FF_GEGLU = [(r, inner) for r in (33, 256, 257) for inner in (64, 96, 1280)]
# (rows, K, inner)
FF_GEGLU_N320 = [(r, K, inner) for r in (33, 257) for K in (128, 640) for inner in (160, 480)]
# more than 256 tiles of (256 rows, 160 + 160 columns), and K = 256: the persistent grid wants an even number >= 4 of chunks (persist_ok
# in csrc/linear_n320.hip) — at K = 128 both settings of MVI_N320_PERSIST would run the plain grid
FF_GEGLU_N320_MANY_TILES = (257 * 256, 256, 160)
# (rows, K, G row runs or 0, with_resid, ret_pre)
LINEAR_LN = [(257, 128, 0, True, False), (512, 192, 2, True, True), (513, 704, 0, False, False), (255, 256, 3, False, True),
             (256, 320, 4, True, True)]
# (N, H, W, C, Co): one pixel; rows that straddle image rows and images inside one wave; a ragged last block
CONV3X3 = [s + (Co,) for s in ((1, 1, 1, 64), (3, 3, 5, 64), (2, 9, 16, 128), (1, 16, 17, 192)) for Co in (320, 640)]
CONV3X3_GAUSS = [(1, 16, 17, 192, 640)]
CONV3X3_S2 = [(1, 1, 1, 64, 320), (2, 7, 9, 128, 320), (1, 8, 6, 128, 640)]
CONV3X3_S2_GAUSS = [(2, 7, 9, 128, 320)]
CONV3X3_UP2 = [(1, 1, 1, 64, 320), (2, 3, 5, 128, 320)]
CONV3X3_UP2_GAUSS = [(2, 3, 5, 128, 320)]
# (N, h, w, C_in, C_out) of the FORWARD stride-2 convolution whose input gradient is taken, (h, w) the size of dy: the kernel contracts
# over C_out (a multiple of 64) into C_in outputs (a multiple of 320, mvi_conv3x3_s2_dgrad_supported) — the 64- and 128-channel
# contractions into 320 columns
CONV3X3_S2_DGRAD = [(1, 2, 2, 320, 64), (2, 6, 10, 320, 128), (1, 2, 2, 320, 128), (2, 6, 10, 320, 64)]
CONV3X3_S2_DGRAD_GAUSS = [(2, 6, 10, 320, 128)]
# (B, T, S, C, Co): the last two split K (3 C / 64 >= 16 chunks)
CONV3T = [(2, 1, 5, 64, 320), (1, 3, 33, 128, 640), (2, 4, 40, 384, 320), (1, 14, 8, 640, 320)]
CONV3T_GAUSS = [(1, 14, 8, 640, 320)]
# (N, C_in, C_out, H, W, stride): 4 x 64 one tile; 9 x 72 and 5 x 136 ragged tiles and borders. Stride 2 takes W % 16 == 0 only
# (mvi_stem_conv3x3_supported): its ragged images are 9 x 80 and 5 x 144
STEM = ([(1, ci, co, H, W, 1) for ci, co in ((7, 16), (16, 16), (20, 32), (32, 32), (8, 320)) for H, W in ((4, 64), (9, 72), (5, 136))] +
        [(1, ci, 32, H, W, 2) for ci in (5, 16) for H, W in ((4, 64), (9, 80), (5, 144))])
STEM_GAUSS = [(1, 32, 32, 9, 72, 1), (1, 16, 32, 9, 80, 2), (1, 8, 320, 5, 136, 1)]
# the dgrad entry points, one parity case each
# (rows, K, N) of the forward: dx = dy W contracts over N into K outputs — 320 into 192 on linear_k320, 1280 into 640 on linear_n320
LINEAR_DGRAD = [(257, 192, 320), (257, 640, 1280)]
CONV3X3_DGRAD = (2, 5, 7, 320, 128)                              # (N, H, W, C_in, C_out) of the forward
CONV3T_DGRAD = (2, 3, 9, 320, 128)                               # (B, T, S, C_in, C_out) of the forward
STEM_DGRAD = [(1, 16, 9, 72), (1, 32, 5, 136)]                   # (N, C, H, W)


def _tag_dtype(tag):
    return DTYPES[tag]


@functools.lru_cache(maxsize=None)
def linear_case(kind, tag, rows, K, N, with_bias, ident=0):
    """x [rows, K], w [N, K], b [N] -> F.linear in fp64."""
    dtype = _tag_dtype(tag)
    d = gemm_data(kind, gen(1, rows, K, N, with_bias, ident, len(kind)), (rows, K), (rows, 1), (N, K), K, dtype, with_bias)
    if d is None:
        return None
    x, w, b = d
    return _finish(kind, dtype, F.linear(x, w, b), lambda: F.linear(x.abs(), w.abs(), _abs(b)), K, x=x, w=w, b=b)


@functools.lru_cache(maxsize=None)
def conv3x3_case(kind, tag, N, H, W, C, Co, stride=1, up2=False):
    """x [N, C, H, W], w [Co, C, 3, 3], b [Co] -> F.conv2d(padding 1) in fp64, of the nearest-neighbour 2x upsampled image with up2."""
    dtype = _tag_dtype(tag)
    Hs, Ws = (2 * H, 2 * W) if up2 else (H, W)
    K_valid = min(3, Hs) * min(3, Ws) * C                        # the taps an inner pixel has (one for a one-pixel image): the bias scale
    x, w, b = gemm_data(kind, gen(2, N, H, W, C, Co, stride, up2, len(kind)), (N, C, H, W), (N, 1, 1, 1), (Co, C, 3, 3), K_valid, dtype)
    src = (lambda t: F.interpolate(t, scale_factor=2, mode="nearest")) if up2 else (lambda t: t)
    cv = lambda a, ww, bb: F.conv2d(src(a), ww, bb, stride=stride, padding=1)
    return _finish(kind, dtype, cv(x, w, b), lambda: cv(x.abs(), w.abs(), b.abs()), 9 * C, x=x, w=w, b=b)


@functools.lru_cache(maxsize=None)
def conv3x3_s2_dgrad_case(kind, tag, N, h, w_, Ci, Co):
    """dy [N, Co, h, w], the forward weight w [Co, Ci, 3, 3] -> dx [N, Ci, 2 h, 2 w] = F.conv_transpose2d(dy, w, stride 2, padding 1,
    output_padding 1) in fp64. The valid taps of an output depend on the parity of its pixel (1, 2 or 4 of them, fewer at the last
    row / column) — K_total is a multiple of Co, so it is even. The kernel has no bias: the rounding set exists only where Co (the one
    tap of a quarter of the pixels) carries the sums far enough — bf16 at Co = 128 (at Co = 64 a quarter of the outputs sits at 256, and
    0.497 of all would round); in f16 (4 * 4 Co <= 2048) nothing would round: None."""
    dtype = _tag_dtype(tag)
    # the kernel's weight is the transposed one: its output channels are the forward's INPUT channels (axis 1 of the forward weight)
    d = gemm_data(kind, gen(3, N, h, w_, Ci, Co, len(kind)), (N, Co, h, w_), (N, 1, 1, 1), (Ci, Co, 3, 3), Co, dtype, with_bias=False)
    if d is None:
        return None
    dy, wt, _ = d
    w = wt.transpose(0, 1).contiguous()                          # [Co, Ci, 3, 3], the forward's layout (signs per Ci: per output column)
    ct = lambda a, b: F.conv_transpose2d(a, b, stride=2, padding=1, output_padding=1)
    return _finish(kind, dtype, ct(dy, w), lambda: ct(dy.abs(), w.abs()), 4 * Co, dy=dy, w=w)


@functools.lru_cache(maxsize=None)
def conv3t_case(kind, tag, B, T, S, C, Co):
    """tok [(B T), S, C], w [Co, C, 3, 1, 1], b [Co] -> ref_conv3t in fp64 [(B T), S, Co]. The first and last frame of every video
    have two valid taps: with +-1 data a frame leaking in from the neighbouring video moves every output of that frame."""
    dtype = _tag_dtype(tag)
    d = gemm_data(kind, gen(4, B, T, S, C, Co, len(kind)), (B, T, S, C), (B, 1, S, 1), (Co, C, 3, 1, 1), (3 if T > 2 else T) * C, dtype)
    x, w, b = d
    tok = x.reshape(B * T, S, C)
    return _finish(kind, dtype, ref_conv3t(tok, w, b, B, T), lambda: ref_conv3t(tok.abs(), w.abs(), b.abs(), B, T), 3 * C,
                   tok=tok, w=w, b=b)


@functools.lru_cache(maxsize=None)
def stem_case(kind, tag, N, Ci, Co, H, W, stride):
    """x [N, Ci, H, W], w [Co, Ci, 3, 3], b [Co] -> F.conv2d(stride, padding 1) in fp64. Odd C_in: K_total = 9 C_in is odd at interior
    pixels and even at the borders with 6 or 4 taps, so no bias makes every output even; the parity set takes an ODD bias (interior
    outputs even) and keeps the precondition that matters — every output is an integer the type holds exactly, |ref| <= 9 * 32 + 9 is
    below 2^8 for every odd C_in of the list — without the evenness assertion. A dropped term still moves an output by 1."""
    dtype = _tag_dtype(tag)
    odd = Ci % 2 == 1
    d = gemm_data(kind, gen(5, N, Ci, Co, H, W, stride, len(kind)), (N, Ci, H, W), (N, 1, 1, 1), (Co, Ci, 3, 3), 9 * Ci, dtype, odd_bias=odd)
    x, w, b = d
    cv = lambda a, ww, bb: F.conv2d(a, ww, bb, stride=stride, padding=1)
    return _finish(kind, dtype, cv(x, w, b), lambda: cv(x.abs(), w.abs(), b.abs()), 9 * Ci, even=not odd, x=x, w=w, b=b)


def gate_weight(K, dtype):
    """|gate weight| of geglu_case: 16 (gates are multiples of 32) unless v g could pass f16's 65504: |v| <= K + 8 and |g| <= gw (K + 8)
    cannot both be reached, but 5 sigma of each is sqrt(K) 5 * gw sqrt(K) 5 = 25 gw K: 8 at K = 128, 4 (multiples of 8, still
    exp(-g^2 / 2) <= e^-32 < 2^-26) from K = 320 on."""
    if dtype == torch.bfloat16:
        return 16
    return 8 if K <= 128 else 4


@functools.lru_cache(maxsize=None)
def geglu_case(tag, rows, K, inner):
    """x [rows, K] of +-1; weight [2 inner, K]: the value half +-1 (parity data, even bias), the gate half +-gw with a bias that is an
    even multiple of gw — every gate is a multiple of 2 gw >= 8. geglu1 / geglu2 (csrc/geglu_math.h) return EXACTLY v g once
    exp(-g^2 / 2) < 2^-26 (fma(-p, e, 1) is 1 whatever v_rcp_f32 and v_exp_f32 return, and g/2 + |g/2| 1 = g), exactly +-0 at g = 0, and
    +-0 for g <= -8 where the true value is below 1e-14 |v| |g| (1e-22 |v| at -10). v g < 2^24 is exact in fp32, so the store's
    rounding is the only one. -> Case with want = (v g).to(dtype) where g > 0 and 0 where g = 0, `neg` the mask of g < 0 (there the
    test asks |got| <= 1e-20). The three gate classes all occur (asserted)."""
    dtype = _tag_dtype(tag)
    g = gen(6, rows, K, inner, dtype == torch.float16)
    gw = gate_weight(K, dtype)
    x = signs(g, rows, K)
    w = torch.cat([signs(g, inner, K), gw * signs(g, inner, K)])
    b = torch.cat([torch.randint(-4, 5, (inner,), generator=g).double() * 2, torch.randint(-2, 3, (inner,), generator=g).double() * 2 * gw])
    h = F.linear(x, w, b)
    v, gate = h[:, :inner], h[:, inner:]
    expect_parity(v, dtype)
    assert torch.equal(gate % (2 * gw), torch.zeros_like(gate)) and 2 * gw >= 8
    pos, zero, neg = gate > 0, gate == 0, gate < 0
    assert pos.any() and zero.any() and neg.any(), "GEGLU gates: a gate class does not occur"
    prod = v * gate
    assert prod.abs().max().item() < 2 ** 24
    want = torch.where(pos, prod, torch.zeros_like(prod)).to(dtype)
    assert torch.isfinite(want).all(), f"GEGLU gates: v g overflows {dtype}"
    return Case(kind="gates", x=x, w=w, b=b, ref=torch.where(pos, prod, torch.zeros_like(prod)), want=want, neg=neg)


@functools.lru_cache(maxsize=None)
def linear_ln_case(tag, rows, K, G, with_resid, ret_pre):
    """The add + LayerNorm epilogue on integers: h = x W^T + b on parity data (even, a number of the type), resid [rows, 320] and
    row [G, 1, 320] even integers in [-16, 16] — h, resid + h and resid + h + row are even integers below 2^8, numbers of bf16 and f16:
    the kernel's roundings of h, s_pre and s all leave them unchanged, and s / s_pre must equal the fp64 sums bit for bit.
    LayerNorm itself is not exact: y keeps the bar of the existing test against F.layer_norm of the exact s."""
    dtype = _tag_dtype(tag)
    N = 320
    g = gen(7, rows, K, G, with_resid, ret_pre)
    x, w, b = gemm_data("parity", g, (rows, K), (rows, 1), (N, K), K, dtype)
    even16 = lambda *shape: torch.randint(-8, 9, shape, generator=g).double() * 2
    resid = even16(rows, N) if with_resid else None
    row = even16(G, 1, N) if G else None
    lw, lb = torch.randn(N, generator=g).double() * 0.5 + 1.0, torch.randn(N, generator=g).double() * 0.2
    h = F.linear(x, w, b)
    s_pre = h if resid is None else resid + h
    s = s_pre if row is None else (s_pre.reshape(G, rows // G, N) + row).reshape(rows, N)
    for t in (h, s_pre, s):
        expect_parity(t, dtype)
    return Case(kind="parity", x=x, w=w, b=b, resid=resid, row=row, lw=lw, lb=lb, s=s, s_pre=s_pre, want_s=s.to(dtype),
                want_s_pre=s_pre.to(dtype), y_ref=F.layer_norm(s, (N,), lw, lb, 1e-5))


# ---- the dgrad entry points: the forward kernels on transposed weights, against the fp64 ADJOINT of the forward ------------------------

@functools.lru_cache(maxsize=None)
def conv3x3_dgrad_case(tag, N, H, W, Ci, Co):
    """dy [N, Co, H, W], the forward weight w [Co, Ci, 3, 3], both +-1 -> dx = F.conv_transpose2d(dy, w, padding 1) [N, Ci, H, W]."""
    g = gen(8, N, H, W, Ci, Co)
    dy, w = signs(g, N, Co, H, W), signs(g, Co, Ci, 3, 3)
    ref = F.conv_transpose2d(dy, w, padding=1)
    return Case(kind="parity", dy=dy, w=w, ref=ref, want=expect_parity(ref, _tag_dtype(tag)), K_total=9 * Co)


@functools.lru_cache(maxsize=None)
def conv3t_dgrad_case(tag, B, T, S, Ci, Co):
    """dy [(B T), S, Co], the forward weight w [Co, Ci, 3, 1, 1], both +-1 -> dx [(B T), S, Ci] = the conv_transpose3d adjoint."""
    g = gen(9, B, T, S, Ci, Co)
    dy, w = signs(g, B * T, S, Co), signs(g, Co, Ci, 3, 1, 1)
    dy5 = dy.reshape(B, T, S, 1, Co).permute(0, 4, 1, 2, 3)
    ref = F.conv_transpose3d(dy5, w, padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(B * T, S, Ci)
    return Case(kind="parity", dy=dy, w=w, ref=ref, want=expect_parity(ref, _tag_dtype(tag)), K_total=3 * Co)


@functools.lru_cache(maxsize=None)
def stem_dgrad_case(tag, N, C, H, W):
    """dz [N, C, H, W], the forward weight w [C, C, 3, 3], both +-1 -> dx = F.conv_transpose2d(dz, w, padding 1)."""
    g = gen(10, N, C, H, W)
    dz, w = signs(g, N, C, H, W), signs(g, C, C, 3, 3)
    ref = F.conv_transpose2d(dz, w, padding=1)
    return Case(kind="parity", dz=dz, w=w, ref=ref, want=expect_parity(ref, _tag_dtype(tag)))


def every_case(tag):
    """(name, builder) of every exact case of the GPU tests in `tag`: what tests/test_gemm_exact_cpu.py walks. A builder returns the
    Case (its preconditions asserted on the way) or None where the rounding set does not exist for the shape and type."""
    out = []
    for kind in ("parity", "rounding"):
        for c in LINEAR_N320:
            out.append((f"linear_n320 {kind} {c}", functools.partial(linear_case, kind, tag, *c[:4])))
        for r, N, wb, _ in LINEAR_K320:
            out.append((f"linear_k320 {kind} {(r, N, wb)}", functools.partial(linear_case, kind, tag, r, 320, N, wb)))
        for c in CONV3X3:
            out.append((f"conv3x3 {kind} {c}", functools.partial(conv3x3_case, kind, tag, *c)))
        for c in CONV3X3_S2:
            out.append((f"conv3x3 s2 {kind} {c}", functools.partial(conv3x3_case, kind, tag, *c, 2)))
        for c in CONV3X3_UP2:
            out.append((f"conv3x3 up2 {kind} {c}", functools.partial(conv3x3_case, kind, tag, *c, 1, True)))
        for c in CONV3X3_S2_DGRAD:
            out.append((f"conv3x3_s2_dgrad {kind} {c}", functools.partial(conv3x3_s2_dgrad_case, kind, tag, *c)))
        for c in CONV3T:
            out.append((f"conv3t {kind} {c}", functools.partial(conv3t_case, kind, tag, *c)))
        for c in STEM:
            out.append((f"stem {kind} {c}", functools.partial(stem_case, kind, tag, *c)))
    for c in FF_GEGLU:
        out.append((f"ff_geglu {c}", functools.partial(geglu_case, tag, c[0], 320, c[1])))
    for c in FF_GEGLU_N320:
        out.append((f"ff_geglu_n320 {c}", functools.partial(geglu_case, tag, *c)))
    for c in LINEAR_LN:
        out.append((f"linear_ln {c}", functools.partial(linear_ln_case, tag, *c)))
    for rows, K, N in LINEAR_DGRAD:
        out.append((f"linear_dgrad {(rows, K, N)}", functools.partial(linear_case, "parity", tag, rows, N, K, False, 1)))
    out.append((f"conv3x3_dgrad {CONV3X3_DGRAD}", functools.partial(conv3x3_dgrad_case, tag, *CONV3X3_DGRAD)))
    out.append((f"conv3t_dgrad {CONV3T_DGRAD}", functools.partial(conv3t_dgrad_case, tag, *CONV3T_DGRAD)))
    for c in STEM_DGRAD:
        out.append((f"stem_dgrad {c}", functools.partial(stem_dgrad_case, tag, *c)))
    return out

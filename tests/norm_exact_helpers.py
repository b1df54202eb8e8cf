"""Data, fp64 references and derived ELEMENTWISE bounds for the forward normalisation and pointwise kernels (csrc/groupnorm_silu.hip,
csrc/groupnorm_tokens.hip, csrc/token_rows.hip, csrc/softmax_rows.hip, csrc/bias_residual.hip, csrc/geglu.hip): what
tests/test_norm_elementwise_gpu.py holds the kernels to and tests/test_norm_elementwise_cpu.py checks on the CPU (every precondition, a plain
fp32 restatement of each operation inside its own bound, nine planted faults outside it). Pure torch on the CPU; nothing outside the
repository is read. ulp_of, truncate_to, gen and SIG_BITS are those of tests/exact_gemm_helpers.py (fp32 is entered into its tables here).

Data (norm_data). Every value is a number of the storage type; weights, biases, chan_bias and alpha are fp32, as the wrappers pass them.
A statistics UNIT — one (sample, group); one (video, group) over all T frames in the temporal forms; one row for LayerNorm and softmax —
has its own mean, uniform in [-8, 8], and its own scale 2^k, k in -3 .. 2; every channel of a group a further offset of up to one
scale, every frame of a video an offset of about one scale: a kernel that reads a neighbour's moments, normalises per frame, or merges
a stale partner is wrong by a multiple of the output, not by 1 / sqrt(n). weight = 1 + 0.5 randn, bias = 0.5 randn, chan_bias [N, C] =
0.5 randn. One group (CONST_GROUP) is constant at 2.0 in every sample, with no chan_bias on it: its sums are exact in any order, its
variance is exactly 0, so its output has ONE right bit pattern, act(bias[c]) rounded once (Case.want_const on Case.const).
outlier = D > 0: the first token of the tensor — and of every later block of `block_rows` tokens, the length the token-major kernels take
their shifted sums over — is moved by D scales (the constant group stays).

Bound. |got - ref| <= cap + ulp_dtype(|ref| + cap) / 2 on every element (bound): `cap` is what fp32 arithmetic may lose before the
ONE rounding to the storage type. Convention (exact_gemm_helpers.elementwise_bound): any fp32 summation order of n terms errs by at
most n u sum|terms|, u = 2^-24; one fp32 operation by u |result|. norm_cap, softmax_case, pointwise_cap and geglu_case derive theirs.
Where fp32 is exact (sums of two or three numbers on a 2^-8 grid below 2^7: grid_data) cap = 0 and the test is torch.equal."""
import functools

import torch
import torch.nn.functional as F

import exact_gemm_helpers as E
from exact_gemm_helpers import SIG_BITS, gen, truncate_to, ulp_of

E.SIG_BITS.setdefault(torch.float32, 24)
E.MIN_EXP.setdefault(torch.float32, -126)

U = 2.0 ** -24
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CONST_GROUP = 1                                                   # the group that is constant at CONST_VALUE in every sample
CONST_VALUE = 2.0
ALPHAS = (0.0, 1.0, 0.5, 0.3)                                     # blends: both ends, a tie of the two forms, and no number of bf16 / f16


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def q(v, dtype):
    """v (fp64) rounded to `dtype`, as fp64."""
    return v.to(dtype).double()


def f32(v):
    """v (fp64) as the fp32 number the wrapper passes, as fp64."""
    return v.float().double()


def bound(ref, cap, dtype):
    """cap + half an ulp of `dtype` at the farthest value the capped fp32 result can have: one rounding, to nearest."""
    return cap + 0.5 * ulp_of(ref.abs() + cap, dtype)


def quarter_share(ref, cap, dtype):
    """Share of elements whose cap is at most a quarter ulp: there the bound is the rounding, and a second rounding or a truncating
    store falls outside it."""
    return float((cap <= 0.25 * ulp_of(ref, dtype)).double().mean())


def worst_ratio(got, ref, bnd):
    return float(((got.double() - ref).abs() / bnd).max())


def outside_share(got, ref, bnd):
    return float(((got.double() - ref).abs() > bnd).double().mean())


# ---- GroupNorm (+ SiLU) ------------------------------------------------------------------------------------------------------------------

def norm_data(g, dtype, N, C, S, G, T=1, with_cb=True, outlier=0, block_rows=0):
    """(x [N, C, S], weight [C], bias [C], chan_bias [N, C] or None) in fp64 as described in the module docstring."""
    V, Cg = N // T, C // G
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    mean = 8.0 * uni(V, 1, G, 1, 1)
    scale = torch.ldexp(torch.ones(V, 1, G, 1, 1, dtype=torch.float64), torch.randint(-3, 3, (V, 1, G, 1, 1), generator=g))
    x = mean + scale * (uni(V, 1, G, Cg, 1) + (rnd(V, T, G, 1, 1) if T > 1 else 0.0) + rnd(V, T, G, Cg, S))
    if outlier:
        starts = list(range(0, S, block_rows)) if block_rows else [0]
        x[..., starts] += outlier * scale
    x[:, :, CONST_GROUP] = CONST_VALUE
    x = q(x.reshape(N, C, S), dtype)
    w, b = f32(1.0 + 0.5 * rnd(C)), f32(0.5 * rnd(C))
    cb = None
    if with_cb:
        cb = f32(0.5 * rnd(N, C))
        cb[:, CONST_GROUP * Cg:(CONST_GROUP + 1) * Cg] = 0.0
    return x, w, b, cb


def silu_and_slope(z):
    s = torch.sigmoid(z)
    return z * s, s * (1.0 + z * (1.0 - s))


def norm_cap(x5, dims, w5, b5, eps, silu, allowance=1.0):
    """(ref, cap) of act((x - m) rstd w + b) with the moments over `dims` of x5 (n elements per unit), r = rstd, u = 2^-24:
      * m is an fp32 sum of n terms over n: |dm| <= n u mean|x|, and moves xhat = (x - m) r by |dm| r;
      * the variance is an fp32 sum of n non-negative terms over n, relative error n u, so r = (var + eps)^-1/2 is off by n/2 u
        relative; the subtraction, the division by n, + eps, the reciprocal square root and the product (x - m) r are 8 more roundings
        (a form that folds m and r into a per-channel scale / shift, x (w r) + (b - m w r), would round |x| r |w| u instead: the first
        term once more, so this bound lets it pass — the constant group does not: its shift is rounded at m eps^-1/2):
            d_xhat = n u mean|x| r + |x - m| r (n/2 A + 8) u
        A = `allowance` = 1 for sums of squares taken around the mean (nothing cancels); outlier_allowance for the shifted sums.
      * z = xhat w + b: two roundings, four with the folded forms:  d_z = |w| d_xhat + 4 u (|z| + |b|)
      * y = z / (1 + exp(-z)): d_z through the slope of SiLU, and the evaluation itself — the argument of exp2 is z log2(e)
        rounded, |z| u there is |z| u relative in exp, the two hardware approximations (exp2, rcp) are within an ulp and a half each,
        1 + e, the product: cap = |silu'(z)| d_z + |y| (1.5 |z| + 8) u;  without SiLU cap = d_z."""
    n = 1
    for d in dims:
        n *= x5.shape[d]
    m = x5.mean(dims, keepdim=True)
    var = ((x5 - m) ** 2).mean(dims, keepdim=True)
    r = (var + eps).rsqrt()
    d_xhat = n * U * x5.abs().mean(dims, keepdim=True) * r + (x5 - m).abs() * r * (0.5 * n * allowance + 8.0) * U
    z = (x5 - m) * r * w5 + b5
    d_z = w5.abs() * d_xhat + 4.0 * U * (z.abs() + b5.abs())
    if not silu:
        return z, d_z
    y, slope = silu_and_slope(z)
    return y, slope.abs() * d_z + y.abs() * (1.5 * z.abs() + 8.0) * U


def outlier_allowance(x5, dims, starts):
    """The factor on the variance term for kernels that take SHIFTED sums around a block's first token x0 (gt_stats_kernel, gt_fused_kernel
    in csrc/groupnorm_tokens.hip): per channel S1 = sum(x - x0), S2 = sum((x - x0)^2) over the block's rows, and the group's
    M2 = sum_c S2_c - 2 d_c S1_c + rows d_c^2 with d_c = m - x0_c (chan_bias included). Write mu_c for the channel's mean, W_c for its
    sum of squares around mu_c, a_c = mu_c - x0_c and e_c = x0_c - m. Then S2_c = W_c + rows a_c^2, S1_c = rows a_c, and the exact M2 is
    n sigma^2 = sum_c W_c + rows (mu_c - m)^2, while the absolute values of what is summed add up to
        sum_c W_c + rows (|a_c| + |e_c|)^2.
    A typical x0 has |a_c|, |e_c| of the size of the spread: a small multiple of n sigma^2, the convention's n u covers it ("nothing
    cancels"). With x0 far from the group a_c ~ -e_c, and the three terms are rows e_c^2, 2 rows e_c^2 and rows e_c^2: 1 + 4 D^2 in units of
    n sigma^2, D^2 the unit's mean over block starts and channels of e_c^2 / sigma^2. The allowance is the issue's 1 + 3 D^2 — each of
    the three assembled terms charged one rows e_c^2 —, the tighter of the two, on top of a convention (n u for a sum whose reduction
    in the kernel is 16 + C / G deep) that is generous already: it holds the kernel to its algebra and excuses nothing more."""
    m = x5.mean(dims, keepdim=True)
    var = ((x5 - m) ** 2).mean(dims, keepdim=True)
    e2 = ((x5[..., starts] - m) ** 2).mean(dims, keepdim=True)
    return 1.0 + 3.0 * e2 / var.clamp_min(1e-300)


@functools.lru_cache(maxsize=None)
def gn_case(tag, N, C, S, G, T=1, with_cb=True, silu=True, outlier=0, block_rows=0, ident=0):
    """GroupNorm(G) (+ SiLU) of x [N, C, S] + chan_bias[:, :, None], the moments per (video, group) over the T frames of a video:
    F.group_norm in fp64 on the "b c t s" view, rounded nowhere before the store. Everything in the planes layout [N, C, S]; the
    token-major forms transpose. Fields: x, w, b, cb, eps, ref, cap, bound (A = 1), and for outlier cases cap_out / bound_out with the
    shifted sums' allowance; const (mask of the constant group), want_const (its one right output)."""
    dtype = DTYPES[tag]
    x, w, b, cb = norm_data(gen(31, N, C, S, G, T, with_cb, outlier, block_rows, ident, dtype == torch.float16), dtype, N, C, S, G, T, with_cb,
                            outlier, block_rows)
    eps = 1e-5 if silu else 1e-6
    V, Cg = N // T, C // G
    xe = x if cb is None else x + cb[:, :, None]
    x5 = xe.reshape(V, T, G, Cg, S)
    w5, b5 = w.reshape(1, 1, G, Cg, 1), b.reshape(1, 1, G, Cg, 1)
    dims = (1, 3, 4)
    ref, cap = norm_cap(x5, dims, w5, b5, eps, silu)
    # the same through the library's own GroupNorm: the written-out formula is the operation the network means
    lib = F.group_norm(x5.permute(0, 2, 3, 1, 4).reshape(V, C, T, S), G, w, b, eps).reshape(V, G, Cg, T, S).permute(0, 3, 1, 2, 4)
    lib = F.silu(lib) if silu else lib
    assert (lib - ref).abs().max().item() <= 1e-12 * (1.0 + ref.abs().max().item())
    const = torch.zeros(V, T, G, Cg, S, dtype=torch.bool)
    const[:, :, CONST_GROUP] = True
    act = (lambda t: t * torch.sigmoid(t)) if silu else (lambda t: t)
    want_const = act(b5.expand(V, T, G, Cg, S))[const].to(dtype)
    assert torch.equal(ref[const].to(dtype), want_const), "the constant group's reference is not act(bias) rounded once"
    c = Case(tag=tag, dtype=dtype, N=N, C=C, S=S, G=G, T=T, silu=silu, eps=eps, x=x, w=w, b=b, cb=cb, n=T * Cg * S,
             ref=ref.reshape(N, C, S), cap=cap.reshape(N, C, S), const=const.reshape(N, C, S), want_const=want_const, outlier=outlier)
    c.bound = bound(c.ref, c.cap, dtype)
    c.quarter = quarter_share(c.ref, c.cap, dtype)
    if outlier:
        starts = list(range(0, S, block_rows)) if block_rows else [0]
        A = outlier_allowance(x5, dims, starts)
        _, cap_out = norm_cap(x5, dims, w5, b5, eps, silu, A)
        c.cap_out = cap_out.reshape(N, C, S)
        c.bound_out = bound(c.ref, c.cap_out, dtype)
        c.D = float(((A - 1.0) / 3.0).sqrt().median())
    return c


def gn_on(t_nsc, tag, G, T, w, b, cb, silu, eps):
    """(ref, cap, bound) of the token-major GroupNorm of a GIVEN tensor t [N, S, C] (fp64 holding numbers of the type): the norm behind
    rows_fused's partials reads the ROUNDED output of the fused pass, so its reference is taken on what that pass stored."""
    dtype = DTYPES[tag]
    N, S, C = t_nsc.shape
    x = t_nsc.transpose(1, 2)
    xe = x if cb is None else x + cb[:, :, None]
    x5 = xe.reshape(N // T, T, G, C // G, S)
    ref, cap = norm_cap(x5, (1, 3, 4), w.reshape(1, 1, G, -1, 1), b.reshape(1, 1, G, -1, 1), eps, silu)
    ref, cap = ref.reshape(N, C, S).transpose(1, 2), cap.reshape(N, C, S).transpose(1, 2)
    return ref, cap, bound(ref, cap, dtype)


def stack3(y, T):
    """[(b T), C, S] -> [(b T), 3 C, S]: (frame t - 1 | frame t | frame t + 1) on the channel axis, zeros at the ends of a video."""
    N, C, S = y.shape
    v = y.reshape(N // T, T, C, S)
    z = torch.zeros_like(v[:, :1])
    return torch.cat([torch.cat([z, v[:, :-1]], 1), v, torch.cat([v[:, 1:], z], 1)], 2).reshape(N, 3 * C, S)


def gn_f32(c, fault=None):
    """The plain fp32 restatement of gn_case (what the bound must leave room for), stored in the case's type — and the planted faults
    of tests/test_norm_elementwise_cpu.py: 'truncate' (the store rounds toward zero), 'round_z' (z rounded to the storage type before
    SiLU), 'neighbour' (the next group's moments), 'per_frame' (moments per frame), 'unbiased' (variance over n - 1), 'eps_outside'
    (1 / (sqrt(var) + eps)), 'cb_after' (chan_bias added after the statistics), 'tail' (a token row's last 16-byte vector takes the
    next channel's weight and bias)."""
    N, C, S, G, T = c.N, c.C, c.S, c.G, c.T
    V, Cg = N // T, C // G
    x = c.x.float()
    cb = None if c.cb is None else c.cb.float()[:, :, None]
    xs = x if (cb is None or fault == "cb_after") else x + cb                     # what the statistics see
    xa = x if cb is None else x + cb                                               # what is normalised
    r5 = lambda t: t.reshape(V, T, G, Cg, S)
    dims = (3, 4) if fault == "per_frame" else (1, 3, 4)
    n = T * Cg * S if fault != "per_frame" else Cg * S
    m = r5(xs).mean(dims, keepdim=True)
    var = ((r5(xs) - m) ** 2).sum(dims, keepdim=True) / (n - 1 if fault == "unbiased" else n)
    r = 1.0 / (var.sqrt() + c.eps) if fault == "eps_outside" else (var + c.eps).rsqrt()
    if fault == "neighbour":
        m, r = m.roll(1, 2), r.roll(1, 2)
    w, b = c.w.float(), c.b.float()
    if fault == "tail":
        vec = 4 if c.dtype == torch.float32 else 8
        w, b = w.clone(), b.clone()
        w[-vec:], b[-vec:] = w[-vec:].roll(-1), b[-vec:].roll(-1)
    z = (r5(xa) - m) * r * w.reshape(1, 1, G, Cg, 1) + b.reshape(1, 1, G, Cg, 1)
    if fault == "round_z":
        z = z.to(c.dtype).float()
    y = (z * torch.sigmoid(z) if c.silu else z).reshape(N, C, S)
    return store(y, c.dtype, fault == "truncate")


def store(y32, dtype, truncate=False):
    """An fp32 result stored in `dtype` (round to nearest even, once) — or truncated, the planted fault — as fp64."""
    if truncate and dtype != torch.float32:
        return truncate_to(y32.double(), dtype)
    return y32.to(dtype).double()


# (N, C, spatial, G, T): the plane / frame forms. C / G = 2 with an odd S (the scalar path); C / G = 3; three pixels; T = 2; T = 3 at
# C / G = 10; MULTI_CHUNK: the smallest 64-channel image on 64-wide rows whose group (C / G = 2) passes one chunk of the two-launch
# kernels — 8192 fp32 elements (the GPU test looks it up from mvi_groupnorm_workspace_bytes and asserts it is this one); CLUSTER: 4 groups
# of 149 760 elements, the one-launch cluster form (7 blocks per group in fp32, 4 in bf16 / f16).
GN_PLANES = [(2, 64, (5, 9), 32, 1), (2, 96, (8, 8), 32, 1), (2, 64, (1, 3), 32, 1), (4, 64, (6, 8), 32, 2), (3, 320, (3, 8), 32, 3)]
MULTI_CHUNK = (1, 64, (65, 64), 32, 1)
CLUSTER = (3, 64, (90, 104), 4, 1)
# (with chan_bias, SiLU)
GN_VARIANTS = [(False, True), (True, True), (True, False)]
# the shapes the issue ran the bound on with a plain fp32 GroupNorm (N, C, S): part of the CPU module's list
GN_ISSUE_SHAPES = [(2, 64, 45), (2, 96, 64), (3, 320, 144), (2, 64, 3)]
SMALL_UNIT = 192                                                  # units up to here must leave the bound to the rounding


def spatial_size(sp):
    n = 1
    for v in sp:
        n *= v
    return n


# ---- LayerNorm rows -----------------------------------------------------------------------------------------------------------------------

LN_WIDTHS = (32, 64, 320, 640, 1280)
LN_ROWS = (3, 37)
LN_MODES = ("plain", "h", "row", "h_row_pre")                     # add_layer_norm's four entries


@functools.lru_cache(maxsize=None)
def ln_case(tag, R, C, mode):
    """add_layer_norm (csrc/token_rows.hip): s_pre = x + h, s = s_pre + row[r / row_div], y = LayerNorm(s) w + b. The kernel's header:
    `intermediates that the unfused graph would materialise (s_pre, s) are rounded to the storage type exactly there` — the reference
    rounds s_pre and s where the op-by-op graph does (an fp32 add of two numbers of the type, stored), takes F.layer_norm in fp64 of the
    rounded s, and s / s_pre have one right answer (want_s, want_s_pre). Rows are the units of the data; row: one broadcast row per run
    of rows (G = 1 for 3 and 37 rows: both are prime). The cap is norm_cap's without SiLU, n = C."""
    dtype = DTYPES[tag]
    g = gen(32, R, C, LN_MODES.index(mode), dtype == torch.float16)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    mean = 8.0 * (torch.rand(R, 1, generator=g, dtype=torch.float64) * 2 - 1)
    scale = torch.ldexp(torch.ones(R, 1, dtype=torch.float64), torch.randint(-3, 3, (R, 1), generator=g))
    x = q(mean + scale * rnd(R, C), dtype)
    h = q(scale * rnd(R, C), dtype) if "h" in mode else None
    row = q(rnd(1, C), dtype) if "row" in mode else None
    w, b = f32(1.0 + 0.5 * rnd(C)), f32(0.5 * rnd(C))
    add = lambda a, t: (a.float() + t.float()).to(dtype).double()                 # the op-by-op graph: fp32 add, stored
    s_pre = x if h is None else add(x, h)
    s = s_pre if row is None else add(s_pre, row)
    eps = 1e-5
    ref, cap = norm_cap(s, (1,), w[None], b[None], eps, False)
    lib = F.layer_norm(s, (C,), w, b, eps)
    assert (lib - ref).abs().max().item() <= 1e-12 * (1.0 + ref.abs().max().item())
    return Case(tag=tag, dtype=dtype, x=x, h=h, row=row, w=w, b=b, eps=eps, s=s, s_pre=s_pre, ref=ref, cap=cap, bound=bound(ref, cap, dtype),
                quarter=quarter_share(ref, cap, dtype), n=C, mode=mode)


def ln_f32(c):
    s = c.s.float()
    m = s.mean(1, keepdim=True)
    r = (((s - m) ** 2).mean(1, keepdim=True) + c.eps).rsqrt()
    return store((s - m) * r * c.w.float() + c.b.float(), c.dtype)


# ---- softmax rows -------------------------------------------------------------------------------------------------------------------------

SOFTMAX_COLS = (1, 7, 64, 65, 300)
SOFTMAX_SCALE = 0.7


@functools.lru_cache(maxsize=None)
def softmax_case(tag, cols):
    """softmax(scale x) over rows (csrc/softmax_rows.hip: fp32 statistics, exp2 with the scale folded into one fma). Five rows with the
    data's own mean and scale each, one row with a single dominant entry (+ 40: every other probability is below e^-20), one row with
    all entries equal (1 / cols each). Relative cap (n + 2 |s (x - max)| + 8) u: the exponent's argument a = s log2(e) (x - max) is
    one fma of a rounded constant — 2 |a| u, which is 2 |a| ln 2 u < 2 |s (x - max)| u relative in exp2 (the rounding of max * s log2(e) is
    common to the whole row and cancels in the quotient) —, exp2 itself, the sum of n positive terms (n u), the reciprocal and the
    product: 8 u for the single operations."""
    dtype = DTYPES[tag]
    g = gen(33, cols, dtype == torch.float16)
    R = 7
    mean = 8.0 * (torch.rand(R, 1, generator=g, dtype=torch.float64) * 2 - 1)
    scale = torch.ldexp(torch.ones(R, 1, dtype=torch.float64), torch.randint(-3, 3, (R, 1), generator=g))
    x = mean + scale * torch.randn(R, cols, generator=g, dtype=torch.float64)
    x[5, cols // 2] += 40.0
    x[6] = x[6, 0]
    x = q(x, dtype)
    a = SOFTMAX_SCALE * (x - x.max(1, keepdim=True).values)
    ref = torch.softmax(SOFTMAX_SCALE * x, 1)
    cap = ref * (cols + 2.0 * a.abs() + 8.0) * U
    assert a.min().item() > -80.0                                                  # nothing near fp32's denormals
    return Case(tag=tag, dtype=dtype, x=x, ref=ref, cap=cap, bound=bound(ref, cap, dtype), quarter=quarter_share(ref, cap, dtype), n=cols)


def softmax_f32(c):
    x = c.x.float() * SOFTMAX_SCALE
    e = torch.exp(x - x.max(1, keepdim=True).values)
    return store(e / e.sum(1, keepdim=True), c.dtype)


# ---- pointwise tails ----------------------------------------------------------------------------------------------------------------------

def grid_data(g, dtype, *shape):
    """Numbers of `dtype` on a 2^-8 grid, |v| < 32: a sum of three is a multiple of 2^-8 below 2^7 — 15 bits, exact in fp32 in any order."""
    v = 8.0 * (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) + 4.0 * torch.randn(*shape, generator=g, dtype=torch.float64).clamp(-5, 5)
    v = torch.round(q(v, dtype) * 256.0) / 256.0
    assert torch.equal(q(v, dtype), v) and v.abs().max().item() < 32.0
    return v


def point_data(g, dtype, *shape):
    """Pointwise operands: a mean in [-8, 8] and a scale 2^k per leading index (sample / row), numbers of the type."""
    lead = (shape[0],) + (1,) * (len(shape) - 1)
    mean = 8.0 * (torch.rand(*lead, generator=g, dtype=torch.float64) * 2 - 1)
    scale = torch.ldexp(torch.ones(*lead, dtype=torch.float64), torch.randint(-3, 3, lead, generator=g))
    return q(mean + scale * torch.randn(*shape, generator=g, dtype=torch.float64), dtype)


def pointwise_cap(k, abs_form):
    """k fp32 operations: every one rounds a partial result no larger than the formula evaluated on absolute values."""
    return k * U * abs_form


def point_case(dtype, ref, cap):
    return Case(dtype=dtype, ref=ref, cap=cap, bound=bound(ref, cap, dtype), quarter=quarter_share(ref, cap, dtype) if torch.is_tensor(cap) else 1.0)


def chan(v, ndim):
    """A per-channel vector against [N, C, *spatial]."""
    return v.reshape(1, -1, *([1] * (ndim - 2)))


def samp(v, ndim):
    """A per-sample vector against [N, ...]."""
    return v.reshape(-1, *([1] * (ndim - 1)))


def ref_bias_residual_add(dtype, h, bias, x):
    """out = h + bias[c] (+ x) (csrc/bias_residual.hip): one fp32 add per operand; without bias one add of two grid numbers — exact, cap 0."""
    b = 0.0 if bias is None else chan(bias, h.dim())
    xx = 0.0 if x is None else x
    ab = (0.0 if bias is None else chan(bias, h.dim()).abs())
    k = 0 if bias is None else 1 + (x is not None)
    return point_case(dtype, h + b + xx, pointwise_cap(k, h.abs() + ab + (0.0 if x is None else x.abs())))


def ref_blend(dtype, base, t, bias, alpha, nd_alpha):
    """out = base + (1 - alpha[n]) (t + bias[c]) — bias_residual_blend, tokens_blend_to_planes, rows_fused's blend: 1 - alpha, the add
    of the bias, the product, the last add: four operations. alpha = 1 returns base, alpha = 0 base + (t + bias)."""
    om = 1.0 - alpha
    b = 0.0 if bias is None else bias
    ref = base + nd_alpha(om) * (t + b)
    return point_case(dtype, ref, pointwise_cap(4, base.abs() + nd_alpha(1.0 + alpha.abs()) * (t.abs() + (0.0 if bias is None else bias.abs()))))


def blend_f32(dtype, base, t, bias, alpha, nd_alpha, neighbour=False):
    """The fp32 restatement of ref_blend; neighbour: the planted fault, every sample blends with the next sample's alpha."""
    a = alpha.float().roll(1) if neighbour else alpha.float()
    return store(base.float() + nd_alpha(1.0 - a) * (t.float() + bias.float()), dtype)


@functools.lru_cache(maxsize=None)
def blend_case(tag, N, C, S):
    """bias_residual_blend's operands [N, C, S] with alpha = ALPHAS cycled over the samples -> (base, t, bias, alpha, Case)."""
    dtype = DTYPES[tag]
    g = gen(35, N, C, S, dtype == torch.float16)
    base, t = point_data(g, dtype, N, C, S), point_data(g, dtype, N, C, S)
    bias = f32(0.5 * torch.randn(C, generator=g, dtype=torch.float64))
    alpha = f32(torch.tensor([ALPHAS[i % len(ALPHAS)] for i in range(N)], dtype=torch.float64))
    return base, t, bias, alpha, ref_blend(dtype, base, t, chan(bias, 3), alpha, lambda v: samp(v, 3))


def ref_bias_silu(dtype, h, bias):
    """silu(h + bias[c]): one add, then SiLU as in norm_cap."""
    b = chan(bias, h.dim())
    z = h + b
    y, slope = silu_and_slope(z)
    return point_case(dtype, y, slope.abs() * U * (h.abs() + b.abs()) + y.abs() * (1.5 * z.abs() + 8.0) * U)


def ref_add_lerp(dtype, x, h, base, alpha_rows):
    """lerp(t, base, alpha) with t = x + h ROUNDED to the storage type (round_to<T> in add_lerp_kernel: the unfused graph materialises
    it), in PyTorch's two-sided form — w < 0.5: t + w (base - t), else base - (base - t)(1 - w): the difference, 1 - w, the product, the
    last add, each on values no larger than (|t| + |base|)(1 + |w| + |1 - w|)."""
    t = x if h is None else (x.float() + h.float()).to(dtype).double()
    w = alpha_rows
    ref = t + w * (base - t)
    return point_case(dtype, ref, pointwise_cap(4, (t.abs() + base.abs()) * (1.0 + w.abs() + (1.0 - w).abs())))


@functools.lru_cache(maxsize=None)
def geglu_case(tag, rows, inner):
    """out = v gelu(g), the erf form (csrc/geglu.hip on geglu_math.h's gelu_erf), held to PyTorch's F.gelu in fp64. The cap is ABSOLUTE
    in Phi, as geglu_math.h documents its forms: |v| |g| / 2 (1.5e-7 + 3 u) — an error of erf of 1.5e-7 plus the roundings of the
    argument g / sqrt 2 (|erf'(z) z| u <= u / 2), of 1 + erf and of erf itself — plus 4 u |ref| for the products. No relative bound on
    the negative tail: 1 + erf cancels there in fp32, and the fp32 reference itself cannot meet one. Gates reach +-10 in four columns."""
    dtype = DTYPES[tag]
    g = gen(34, rows, inner, dtype == torch.float16)
    h = 2.0 * torch.randn(rows, 2 * inner, generator=g, dtype=torch.float64)
    h[:, inner:inner + 4] *= 3.0
    h = q(h, dtype)
    v, gate = h[:, :inner], h[:, inner:]
    ref = v * F.gelu(gate)
    cap = v.abs() * gate.abs() * 0.5 * (1.5e-7 + 3.0 * U) + 4.0 * U * ref.abs()
    return Case(tag=tag, dtype=dtype, h=h, ref=ref, cap=cap, bound=bound(ref, cap, dtype), quarter=quarter_share(ref, cap, dtype))


def geglu_f32(c):
    h = c.h.float()
    inner = h.shape[1] // 2
    return store(h[:, :inner] * F.gelu(h[:, inner:]), c.dtype)


def every_gn_case(tag):
    """(name, builder) of every GroupNorm case of the GPU module that does not depend on a geometry read from the library, plus the
    shapes the issue ran: what the CPU module walks."""
    out = []
    for N, C, sp, G, T in GN_PLANES + [MULTI_CHUNK, CLUSTER]:
        for cb, silu in GN_VARIANTS:
            out.append((f"gn {(N, C, sp, G, T)} cb={cb} silu={silu}", functools.partial(gn_case, tag, N, C, spatial_size(sp), G, T, cb, silu)))
    for N, C, S in GN_ISSUE_SHAPES:
        for silu in (False, True):
            out.append((f"gn issue {(N, C, S)} silu={silu}", functools.partial(gn_case, tag, N, C, S, 32, 1, True, silu)))
    for C in (64, 96, 320):                                                        # token-major stand-ins (block of 64 rows) with outliers
        for D in (8, 64):
            out.append((f"gn outlier C={C} D={D}", functools.partial(gn_case, tag, 2, C, 101, 32, 1, True, True, D, 64)))
    return out

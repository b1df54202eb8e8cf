"""Data, fp64 references and derived ELEMENTWISE bounds for the backward normalisation and gate kernels (csrc/groupnorm_bwd.hip,
csrc/layernorm_bwd.hip, csrc/geglu.hip's geglu_bwd_kernel): what tests/test_norm_bwd_elementwise_gpu.py holds the kernels to and
tests/test_norm_bwd_elementwise_cpu.py checks on the CPU. The forward half is tests/norm_exact_helpers.py; its data (norm_data: every
statistics unit with its own mean and scale, one constant group), its bound (cap + ulp(|ref| + cap) / 2: `cap` is what fp32 arithmetic may
lose before the ONE rounding of the store) and its convention (an fp32 sum of n terms in any order errs by at most n u sum|terms|,
u = 2^-24; one fp32 operation by u |result|) are reused. Pure torch on the CPU; nothing outside the repository is read.

Data. x, weight, bias, chan_bias are norm_data's. The constant group holds CONST_VALUES[1] = 1.703125 (a 7-bit significand: n * value is
exact in fp32 in every order for n < 2^17, asserted; a shift folded into (chan_bias - mean) rstd is rounded there, where 2.0 hides it) or
2.0; its weights are +-2^k and its dy lies on a 2^-4 grid below 8, so that without SiLU A = sum w dy is exact in fp32 (asserted). dy is on
the storage type's grid, with a mean of up to 2 scales and a scale 2^k, k in -2 .. 2, per (video, group), a further offset per frame and
per channel: a neighbour's A, B or coef, or a frame's own A, B, is wrong by a multiple. The stack3 layout has a dy of its own,
[N, 3 C, S], three such blocks.

References. GroupNorm(+SiLU): groupnorm_bwd_helpers.formula (written out, fp64; pinned to fp64 autograd of F.group_norm / F.silu by
pin_gn_formula_to_autograd). Add+LayerNorm: layernorm_bwd_helpers.formula on s, the forward's rounded stream (the wrapper takes s itself).
GEGLU: dh = [dy g Phi(g) | dy a (Phi(g) + g phi(g))] with Phi from erfc in fp64. The references take their moments in fp64; the kernels
take the forward's fp32 statistics — the caps carry that difference (d_xh, d_r below).

Caps: gn_bwd_caps, ln_bwd_caps, geglu_bwd_case derive theirs in their docstrings."""
import functools
import math

import torch
import torch.nn.functional as F

import groupnorm_bwd_helpers as GB
import layernorm_bwd_helpers as LB
from norm_exact_helpers import (CONST_GROUP, DTYPES, Case, U, bound, f32, gen, norm_data, outside_share, q, quarter_share,  # noqa: F401
                                store, ulp_of, worst_ratio)
from exact_gemm_helpers import MIN_EXP                            # (after norm_exact_helpers, which enters fp32 into the tables)

CONST_VALUES = (2.0, 1.703125)
DY_GRID = 16.0                                                    # the constant group's dy: multiples of 2^-4, |dy| <= 8
PLANES, STACK3, TOKENS = "planes", "stack3", "tokens"


# ---- GroupNorm (+ SiLU) backward -------------------------------------------------------------------------------------------------------------

def gn_bwd_caps(x, cb, dyf, dyabs, w, b, N, C, S, G, T, eps, silu, summed_dy):
    """(values, caps) of dx [N, C, S], dweight, dbias [C], dchan_bias [N, C] for x, dyf (the gradient of y, fp64 [N, C, S]; for stack3 the
    folded sum of three blocks, dyabs the sum of their absolute values). Per unit of n = T Cg S elements, r = rstd, u = 2^-24:
      * xh = (x + chan_bias - m) r with the forward's fp32 (m, r): d_xh = n u mean|x| r + |x - m| r (n/2 + 8) u — norm_cap's line: the
        mean is an fp32 sum of n terms, the variance one of n non-negative terms (r off by n/2 u relative), 8 single roundings; r alone
        is off by d_r = (n/2 + 4) u relative. On the CONSTANT group every sum is exact (precondition), the centred differences are
        exact zeros, the variance is 0: d_xh = 0 and d_r = 4 u (eps as an fp32 number, + 0, the reciprocal square root's ulp).
      * g = dy silu'(z), z = w xh + b, silu'(z) = s q, s = sigmoid(z), q = 1 + z (1 - s). d_z = |w| d_xh + 4 u (|z| + |b|) moves
        silu' by at most d_z / 2 (|silu''| = s (1 - s) |2 + z (1 - 2 s)| <= 1/2, z (1 - 2 s) <= 0). The evaluation: the argument of exp2 is z
        log2(e) — the rounded constant and the rounded product are 2 |z| u relative in exp —, exp2 and the reciprocal are within an
        ulp and a half each, 1 + e: d_s = s (2 |z| + 4) u; 1 - s, z (1 - s), 1 + ..: d_q = |z| d_s + 2 u |z| (1 - s) + u |q|; the product
        s q: d_silu' = d_z / 2 + |q| d_s + s d_q + u |s q|. d_g = |dy| d_silu' + u |g| (+ |silu'| d_dy). Without SiLU g = dy, d_g = d_dy.
        d_dy = 0, or 2 u (|block 0| + |block 1| + |block 2|) for stack3's two fp32 additions (0 on the constant group: grid sums are exact).
      * A / n = sum w g / n: the terms' errors |w| d_g, the sum of n terms and the product w (sum g) per channel ((n + 2) u sum|w g|), then
        1 / n, the product with it and with r later: d_An = (sum |w| d_g + (n + 2) u sum|w g|) / n + 3 u |A / n|. Without SiLU the
        constant group's A is exact (precondition): the sum's share is 0 there.
      * B / n = sum w g xh / n: a term errs by |w| (d_g |xh| + |g| d_xh) + u |w g xh|; d_Bn likewise.
      * dx = t1 - t2 - t3, t1 = r w g, t2 = r A / n, t3 = r xh B / n:
            cap = r |w| d_g + |t1| (d_r + 2 u) + r d_An + |t2| (d_r + u) + r (d_xh |B / n| + |xh| d_Bn) + |t3| (d_r + 2 u)
                  + 2 u (|t1| + |t2| + |t3|)                                                   (the two subtractions)
        On the constant group without SiLU that is |t1| 8 u + |t2| 10 u: the assembly's two roundings, those of the constants r and 1 / n
        and of the products with them — nothing of the data.
      * dweight_c = sum over rows and positions of g xh (N S terms): sum (d_g |xh| + |g| d_xh + u |g xh|) + N S u sum|g xh|; it is
        EXACTLY 0 on the constant group (xh = 0). dbias_c = sum g: sum d_g + N S u sum|g|. The summation cap — and what the terms
        themselves carry in from the fp32 statistics, which no order of summation removes (the error of a unit's mean moves all its xh
        the same way).
      * dchan_bias[row, c] = r (w sg - S A / n - sxh B / n) with sg = sum_s g, sxh = sum_s xh (S terms each; the kernel's finalize
        launch forms it from the sums, not from dx): d_sg = sum d_g + S u sum|g|, d_sxh = sum d_xh + S u sum|xh|,
            cap = r (|w| d_sg + S d_An + d_sxh |B / n| + |sxh| d_Bn) + (d_r + 6 u) r (|w sg| + S |A / n| + |sxh B / n|)
        (three products, two subtractions, the product with r)."""
    V, Cg, n = N // T, C // G, T * (C // G) * S
    r5 = lambda t: t.reshape(V, T, G, Cg, S)
    dims = (1, 3, 4)
    xe = x if cb is None else x + cb[:, :, None]
    x5 = r5(xe)
    m = x5.mean(dims, keepdim=True)
    r = (((x5 - m) ** 2).mean(dims, keepdim=True) + eps).rsqrt()
    xh = (x5 - m) * r
    d_xh = n * U * x5.abs().mean(dims, keepdim=True) * r + (x5 - m).abs() * r * (0.5 * n + 8.0) * U
    d_r = torch.full((1, 1, G, 1, 1), (0.5 * n + 4.0) * U, dtype=torch.float64)
    d_xh[:, :, CONST_GROUP] = 0.0
    d_r[:, :, CONST_GROUP] = 4.0 * U
    assert (xh[:, :, CONST_GROUP] == 0).all()
    w5, b5 = w.reshape(1, 1, G, Cg, 1), b.reshape(1, 1, G, Cg, 1)
    dy5 = r5(dyf)
    d_dy = torch.zeros_like(dy5)
    if summed_dy:
        d_dy = 2.0 * U * r5(dyabs)
        d_dy[:, :, CONST_GROUP] = 0.0
    if silu:
        z = w5 * xh + b5
        s = torch.sigmoid(z)
        qv = 1.0 + z * (1.0 - s)
        sp = s * qv
        d_z = w5.abs() * d_xh + 4.0 * U * (z.abs() + b5.abs())
        d_s = s * (2.0 * z.abs() + 4.0) * U
        d_q = z.abs() * d_s + 2.0 * U * z.abs() * (1.0 - s) + U * qv.abs()
        d_sp = 0.5 * d_z + qv.abs() * d_s + s * d_q + U * sp.abs()
        g = dy5 * sp
        d_g = dy5.abs() * d_sp + sp.abs() * d_dy + U * g.abs()
    else:
        g, d_g = dy5, d_dy
    wg = w5 * g
    sum_share = torch.ones(1, 1, G, 1, 1, dtype=torch.float64)
    if not silu:
        sum_share[:, :, CONST_GROUP] = 0.0
    ksum = lambda t: t.sum(dims, keepdim=True)
    An, Bn = ksum(wg) / n, ksum(wg * xh) / n
    d_An = (ksum(w5.abs() * d_g) + sum_share * (n + 2.0) * U * ksum(wg.abs())) / n + 3.0 * U * An.abs()
    d_Bn = (ksum(w5.abs() * (d_g * xh.abs() + g.abs() * d_xh) + U * (wg * xh).abs()) + (n + 2.0) * U * ksum((wg * xh).abs())) / n + 3.0 * U * Bn.abs()
    t1, t2, t3 = r * wg, r * An, r * xh * Bn
    dx = t1 - t2 - t3
    cap_dx = (r * w5.abs() * d_g + t1.abs() * (d_r + 2.0 * U) + r * d_An + t2.abs() * (d_r + U) + r * (d_xh * Bn.abs() + xh.abs() * d_Bn)
              + t3.abs() * (d_r + 2.0 * U) + 2.0 * U * (t1.abs() + t2.abs() + t3.abs()))
    csum = lambda t: t.sum((0, 1, 4)).reshape(C)
    gx = g * xh
    dw, cap_dw = csum(gx), csum(d_g * xh.abs() + g.abs() * d_xh + U * gx.abs()) + N * S * U * csum(gx.abs())
    db, cap_db = csum(g), csum(d_g) + N * S * U * csum(g.abs())
    ssum = lambda t: t.sum(4, keepdim=True)
    sg, sxh = ssum(g), ssum(xh)
    d_sg, d_sxh = ssum(d_g) + S * U * ssum(g.abs()), ssum(d_xh) + S * U * ssum(xh.abs())
    dcb = r * (w5 * sg - S * An - sxh * Bn)
    cap_dcb = (r * (w5.abs() * d_sg + S * d_An + d_sxh * Bn.abs() + sxh.abs() * d_Bn)
               + (d_r + 6.0 * U) * r * ((w5 * sg).abs() + S * An.abs() + (sxh * Bn).abs()))
    assert (dcb - ssum(dx)).abs().max().item() <= 1e-11 * (1.0 + dcb.abs().max().item())
    vals = dict(dx=dx.reshape(N, C, S), dweight=dw, dbias=db, dchan_bias=dcb.expand(V, T, G, Cg, 1).reshape(N, C))
    caps = dict(dx=cap_dx.reshape(N, C, S), dweight=cap_dw, dbias=cap_db, dchan_bias=cap_dcb.expand(V, T, G, Cg, 1).reshape(N, C))
    return vals, caps


def gn_bwd_data(g, dtype, N, C, S, G, T, with_cb, layout, cv):
    """(x, w, b, cb, dy) as the module docstring has them; dy [N, C, S], or [N, 3 C, S] for stack3."""
    V, Cg = N // T, C // G
    x, w, b, cb = norm_data(g, dtype, N, C, S, G, T, with_cb)
    lo, hi = CONST_GROUP * Cg, (CONST_GROUP + 1) * Cg
    x[:, lo:hi] = cv
    w[lo:hi] = torch.ldexp((torch.randint(0, 2, (Cg,), generator=g) * 2 - 1).double(), torch.randint(-1, 2, (Cg,), generator=g))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    dmean = 2.0 * uni(V, 1, G, 1, 1)
    dscale = torch.ldexp(torch.ones(V, 1, G, 1, 1, dtype=torch.float64), torch.randint(-2, 3, (V, 1, G, 1, 1), generator=g))

    def block():
        d = dscale * (dmean + 0.5 * uni(V, 1, G, Cg, 1) + (rnd(V, T, G, 1, 1) if T > 1 else 0.0) + rnd(V, T, G, Cg, S))
        d = q(d, dtype)
        d[:, :, CONST_GROUP] = (torch.round(d[:, :, CONST_GROUP] * DY_GRID) / DY_GRID).clamp(-8.0, 8.0)
        return d.reshape(N, 1, C, S)
    dy = torch.cat([block() for _ in range(3 if layout == STACK3 else 1)], 1).reshape(N, -1, S)
    return x, w, b, cb, dy


@functools.lru_cache(maxsize=None)
def gn_bwd_case(tag, N, C, S, G, T=1, with_cb=True, silu=True, layout=PLANES, cv=CONST_VALUES[1]):
    """One GroupNorm(+SiLU) backward case, everything in the planes layout [N, C, S] (the token-major callers transpose). Fields: x, w, b,
    cb, dy (the layout's own), dyf (the gradient of y it folds to), eps, ref / cap / bound (dicts over dx, dweight, dbias, dchan_bias;
    dchan_bias only with chan_bias), const_c (the constant group's channels), exact_dx (without SiLU: its dx has the cap of the
    roundings of the assembly alone)."""
    dtype = DTYPES[tag]
    x, w, b, cb, dy = gn_bwd_data(gen(41, N, C, S, G, T, with_cb, silu, [PLANES, STACK3, TOKENS].index(layout), int(cv * 64), dtype == torch.float16),
                                  dtype, N, C, S, G, T, with_cb, layout, cv)
    eps = 1e-5 if silu else 1e-6
    Cg, n = C // G, T * (C // G) * S
    if layout == STACK3:
        dyf = GB.fold_stack3(dy, T)
        dyabs = GB.fold_stack3(dy.abs(), T)
    else:
        dyf, dyabs = dy, dy.abs()
    const_c = torch.zeros(C, dtype=torch.bool)
    const_c[CONST_GROUP * Cg:(CONST_GROUP + 1) * Cg] = True
    # preconditions: numbers of the type; n * value exact in fp32; A exact on the constant group (terms on a 2^-5 grid, sum below 2^19)
    assert torch.equal(q(x, dtype), x) and torch.equal(q(dy, dtype), dy) and torch.equal(f32(w), w)
    assert float(torch.tensor(n * cv).float()) == n * cv and (cv * 64) == int(cv * 64) and n * cv * 64 < 2 ** 24
    wd = (w[None, :, None] * dyabs)[:, const_c]
    assert torch.equal(torch.round(wd * 32.0), wd * 32.0) and wd.reshape(N // T, -1).sum(1).max().item() * 32.0 < 2 ** 24
    vals, caps = gn_bwd_caps(x, cb, dyf, dyabs, w, b, N, C, S, G, T, eps, silu, layout == STACK3)
    f = GB.formula(x, cb, dyf, w, b, T, silu, eps, G)
    ref = dict(dx=f["dx"], dweight=f["dweight"], dbias=f["dbias"])
    if cb is not None:
        ref["dchan_bias"] = f["demb"]
    for k, v in ref.items():                                                       # the caps' own values are the formula's
        assert (vals[k] - v).abs().max().item() <= 1e-11 * (1.0 + v.abs().max().item()), k
    assert (ref["dweight"][const_c] == 0).all()
    c = Case(tag=tag, dtype=dtype, N=N, C=C, S=S, G=G, T=T, silu=silu, eps=eps, layout=layout, cv=cv, n=n, x=x, w=w, b=b, cb=cb, dy=dy, dyf=dyf,
             ref=ref, cap={k: caps[k] for k in ref}, const_c=const_c, exact_dx=not silu)
    out_t = lambda k: dtype if k == "dx" else torch.float32
    c.bound = {k: bound(ref[k], c.cap[k], out_t(k)) for k in ref}
    c.quarter = quarter_share(ref["dx"], c.cap["dx"], dtype)
    return c


def pin_gn_formula_to_autograd(N=4, C=64, S=10, G=32, T=2):
    """groupnorm_bwd_helpers.formula against fp64 autograd of F.group_norm / F.silu on the "b c t s" view: largest relative difference."""
    c = gn_bwd_case("f32", N, C, S, G, T, True, True)
    V = N // T
    x = c.x.clone().requires_grad_()
    cb = c.cb.clone().requires_grad_()
    w, b = c.w.clone().requires_grad_(), c.b.clone().requires_grad_()
    v = (x + cb[:, :, None]).reshape(V, T, C, S).transpose(1, 2)
    y = F.silu(F.group_norm(v, G, w, b, c.eps)).transpose(1, 2).reshape(N, C, S)
    y.backward(c.dyf)
    got = dict(dx=x.grad, dweight=w.grad, dbias=b.grad, dchan_bias=cb.grad)
    return max(float((got[k] - c.ref[k]).abs().max() / (1.0 + c.ref[k].abs().max())) for k in got)


GN_FAULTS = ("truncate", "round_g", "neighbour", "per_frame", "tail", "stack3_cross", "fold")


def gn_bwd_f32(c, fault=None):
    """The plain CENTRED fp32 restatement of the backward (dict as c.ref, dx stored in the case's type) — and the planted faults of
    tests/test_norm_bwd_elementwise_cpu.py: 'truncate' (the store rounds toward zero), 'round_g' (g rounded to the storage type before
    the sums), 'neighbour' (the next group's coef), 'per_frame' (A, B per frame), 'tail' (the positions that pad the last 128-wide tile
    read the last position again and are summed into sum xh), 'stack3_cross' (the fold adds the neighbouring frame across a video
    boundary), 'fold' (xh = x r + (chan_bias - m) r, the shift rounded on its own)."""
    N, C, S, G, T = c.N, c.C, c.S, c.G, c.T
    V, Cg, n = N // T, C // G, c.n
    r5 = lambda t: t.reshape(V, T, G, Cg, S)
    dims = (1, 3, 4)
    x = r5(c.x.float())
    cb = torch.zeros(V, T, G, Cg, 1) if c.cb is None else c.cb.float().reshape(V, T, G, Cg, 1)
    xa = x + cb
    m = xa.mean(dims, keepdim=True)
    r = (((xa - m) ** 2).mean(dims, keepdim=True) + c.eps).rsqrt()
    if fault == "fold":                                                            # one fma on the rounded shift (exact in fp64, rounded once)
        xh = (x.double() * r.double() + ((cb - m) * r).double()).float()
    else:
        xh = (x + (cb - m)) * r
    if c.layout == STACK3:
        Tf = N if fault == "stack3_cross" else T
        d = c.dy.float().reshape(N // Tf, Tf, 3, C, S)
        z = torch.zeros_like(d[:, :1, 0])
        dy = d[:, :, 1] + (torch.cat([d[:, 1:, 0], z], 1) + torch.cat([z, d[:, :-1, 2]], 1))
        dy = r5(dy.reshape(N, C, S))
    else:
        dy = r5(c.dy.float())
    w5, b5 = c.w.float().reshape(1, 1, G, Cg, 1), c.b.float().reshape(1, 1, G, Cg, 1)
    if c.silu:
        z = w5 * xh + b5
        s = torch.sigmoid(z)
        g = dy * (s * (1.0 + z * (1.0 - s)))
    else:
        g = dy
    if fault == "round_g":
        g = g.to(c.dtype).float()
    wg = w5 * g
    if fault == "per_frame":
        An, Bn = wg.sum((3, 4), keepdim=True) / (Cg * S), (wg * xh).sum((3, 4), keepdim=True) / (Cg * S)
    else:
        An, Bn = wg.sum(dims, keepdim=True) / n, (wg * xh).sum(dims, keepdim=True) / n
    kA, kB = r * An, r * Bn
    if fault == "neighbour":
        kA, kB = kA.roll(-1, 2), kB.roll(-1, 2)
    dx = (r * w5) * g - kA - xh * kB
    sxh = xh.sum(4, keepdim=True)
    if fault == "tail":
        sxh = sxh + ((-S) % 128) * xh[..., -1:]
    dcb = r * (w5 * g.sum(4, keepdim=True) - S * An - sxh * Bn)
    out = dict(dx=store(dx.reshape(N, C, S), c.dtype, fault == "truncate"), dweight=(g * xh).sum((0, 1, 4)).reshape(C).double(),
               dbias=g.sum((0, 1, 4)).reshape(C).double())
    if c.cb is not None:
        out["dchan_bias"] = dcb.expand(V, T, G, Cg, 1).reshape(N, C).double()
    return out


# (N, C, S, G, T, layout). planes: the vector path with a partial last tile; the scalar path; a group that straddles the 64-channel tile
# (C / G = 3); six position tiles (the finalize kernel's waves stride over them); T Cg = 96 > 64 entries (the finalize entry loop's second
# pass), two videos; T = 2. stack3: T = 2, T = 3 on the scalar path, T = 1 (every frame is both ends), two videos each. tokens: S no
# multiple of 128, C = 64 and 128.
GN_BWD_SHAPES = [(2, 64, 136, 32, 1, PLANES), (2, 64, 45, 32, 1, PLANES), (2, 96, 40, 32, 1, PLANES), (1, 64, 648, 32, 1, PLANES),
                 (6, 64, 24, 2, 3, PLANES), (4, 64, 40, 32, 2, PLANES),
                 (4, 64, 40, 32, 2, STACK3), (6, 64, 45, 32, 3, STACK3), (2, 64, 40, 32, 1, STACK3),
                 (2, 64, 136, 32, 1, TOKENS), (2, 128, 200, 32, 1, TOKENS)]
# (with chan_bias, SiLU, the constant group's value)
GN_BWD_VARIANTS = [(True, True, CONST_VALUES[1]), (False, True, CONST_VALUES[1]), (True, False, CONST_VALUES[1]), (False, False, CONST_VALUES[0])]
# group_norm_tok2tok_backward (N, C, S, G, frames): a 16-byte vector spans four groups (C / G = 2) and S is no multiple of the 64-token
# tile; S below one tile; C = 320 over two videos of two frames (a 48-token tile in fp32); three frames, two videos
TOK2TOK_SHAPES = [(2, 64, 100, 32, 1), (2, 64, 37, 32, 1), (4, 320, 70, 32, 2), (6, 64, 100, 32, 3)]


# ---- Add + LayerNorm backward -----------------------------------------------------------------------------------------------------------------

CONST_ROW = 1
LN_BWD_MODES = [(True, True, True), (True, True, False), (True, False, True), (True, False, False), (False, True, True), (False, True, False),
                (False, False, True)]                             # presence of (gy, gs, gs_pre)


def ln_bwd_caps(s, w, gy, gs, gsp, runs, eps):
    """(values, caps) of dx, dweight, dbias, drow (runs > 0) of csrc/layernorm_bwd.hip's formulas on s [R, C], absent gradients = None.
    Per row, n = C, r = rstd recomputed in fp32 as the forward does:
      * d_xh = C u mean|s| r + |s - m| r (C/2 + 8) u and d_r = (C/2 + 4) u as in gn_bwd_caps; on the constant row (C * value exact)
        d_xh = 0, d_r = 4 u.
      * t = gy w: d_t = u |t|. c1 = mean(t xh): d_c1 = mean(d_t |xh| + |t| d_xh + u |t xh|) + C u mean|t xh| + 2 u |c1| (the terms, the sum of C
        terms, 1 / C and the product with it); c2 = mean(t): d_c2 = mean(d_t) + C u mean|t| + 2 u |c2|.
      * inner = t - c2 - xh c1: d_inner = d_t + d_c2 + d_xh |c1| + |xh| d_c1 + u |xh c1| + 2 u (|t| + |c2| + |xh c1|).
      * gS = r inner (+ gs): d_gS = r d_inner + |r inner| (d_r + u) (+ u (|r inner| + |gs|) for the addition, when gs is there: x + 0 is x).
      * dx = gP = gS (+ gs_pre): d_gP = d_gS (+ u (|gS| + |gs_pre|)). ONE rounding to the storage type follows.
      * drow[g] = sum over the run's L rows of the UNROUNDED gS: sum d_gS + L u sum|gS| (L = 1: gS itself, no sum). A sum of gS rounded
        to the storage type is off by about sqrt(L) 2^-9 |gS| in bf16 — a thousand times this cap.
      * dweight_c = sum_r gy xh: sum (|gy| d_xh + u |gy xh|) + R u sum|gy xh|; dbias_c = sum_r gy: R u sum|gy|."""
    R, C = s.shape
    zero = torch.zeros_like(s)
    gy_ = zero if gy is None else gy
    m = s.mean(1, keepdim=True)
    r = (((s - m) ** 2).mean(1, keepdim=True) + eps).rsqrt()
    xh = (s - m) * r
    d_xh = C * U * s.abs().mean(1, keepdim=True) * r + (s - m).abs() * r * (0.5 * C + 8.0) * U
    d_r = torch.full((R, 1), (0.5 * C + 4.0) * U, dtype=torch.float64)
    d_xh[CONST_ROW] = 0.0
    d_r[CONST_ROW] = 4.0 * U
    assert (xh[CONST_ROW] == 0).all()
    t = gy_ * w
    d_t = U * t.abs()
    mean = lambda v: v.mean(1, keepdim=True)
    c1, c2 = mean(t * xh), mean(t)
    d_c1 = mean(d_t * xh.abs() + t.abs() * d_xh + U * (t * xh).abs()) + C * U * mean((t * xh).abs()) + 2.0 * U * c1.abs()
    d_c2 = mean(d_t) + C * U * mean(t.abs()) + 2.0 * U * c2.abs()
    inner = t - c2 - xh * c1
    d_inner = d_t + d_c2 + d_xh * c1.abs() + xh.abs() * d_c1 + U * (xh * c1).abs() + 2.0 * U * (t.abs() + c2.abs() + (xh * c1).abs())
    gS = r * inner
    d_gS = r * d_inner + gS.abs() * (d_r + U)
    if gs is not None:
        d_gS = d_gS + U * (gS.abs() + gs.abs())
        gS = gS + gs
    gP, d_gP = gS, d_gS
    if gsp is not None:
        d_gP = d_gS + U * (gS.abs() + gsp.abs())
        gP = gS + gsp
    vals = dict(dx=gP, dweight=(gy_ * xh).sum(0), dbias=gy_.sum(0))
    caps = dict(dx=d_gP, dweight=(gy_.abs() * d_xh + U * (gy_ * xh).abs()).sum(0) + R * U * (gy_ * xh).abs().sum(0), dbias=R * U * gy_.abs().sum(0))
    if runs:
        L = R // runs
        vals["drow"] = gS.reshape(runs, L, C).sum(1)
        caps["drow"] = d_gS.reshape(runs, L, C).sum(1) + (L * U * gS.abs().reshape(runs, L, C).sum(1) if L > 1 else 0.0)
    return vals, caps, gS


@functools.lru_cache(maxsize=None)
def ln_bwd_case(tag, R, C, runs, mode=(True, True, True)):
    """One add_layer_norm_backward case: s [R, C] of the storage type, every row with its own mean and scale, row CONST_ROW constant at
    1.703125; gy, gs, gs_pre (those of `mode`) with a mean and a scale 2^k per row; runs = the row groups of drow (0: none; R: one row
    per run, drow is gS itself)."""
    dtype = DTYPES[tag]
    g = gen(42, R, C, runs, LN_BWD_MODES.index(mode), dtype == torch.float16)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    scale = torch.ldexp(torch.ones(R, 1, dtype=torch.float64), torch.randint(-3, 3, (R, 1), generator=g))
    s = q(8.0 * uni(R, 1) + scale * rnd(R, C), dtype)
    s[CONST_ROW] = CONST_VALUES[1]
    assert C * CONST_VALUES[1] * 64 < 2 ** 24 and torch.equal(q(s, dtype), s)
    w = f32(1.0 + 0.5 * rnd(C))

    def grad(present):
        gsc = torch.ldexp(torch.ones(R, 1, dtype=torch.float64), torch.randint(-2, 3, (R, 1), generator=g))
        v = q(gsc * (2.0 * uni(R, 1) + rnd(R, C)), dtype)
        return v if present else None
    gy, gs, gsp = grad(mode[0]), grad(mode[1]), grad(mode[2])
    eps = LB.EPS
    vals, caps, gS = ln_bwd_caps(s, w, gy, gs, gsp, runs, eps)
    f = LB.formula(s, w, gy, gs, gsp, runs, eps)
    ref = {k: f[k] for k in vals}
    for k, v in ref.items():
        assert (vals[k] - v).abs().max().item() <= 1e-11 * (1.0 + v.abs().max().item()), k
    c = Case(tag=tag, dtype=dtype, R=R, C=C, runs=runs, mode=mode, s=s, w=w, gy=gy, gs=gs, gsp=gsp, eps=eps, ref=ref, cap=caps, gS=gS)
    c.bound = {k: bound(ref[k], caps[k], dtype if k == "dx" else torch.float32) for k in ref}
    c.quarter = quarter_share(ref["dx"], caps["dx"], dtype)
    return c


def ln_bwd_f32(c, fault=None):
    """The plain fp32 restatement (dict as c.ref); faults: 'truncate' (dx stored toward zero), 'drow_rounded' (drow sums gS rounded to the
    storage type)."""
    s, w = c.s.float(), c.w.float()
    R, C = s.shape
    zero = torch.zeros_like(s)
    gy = zero if c.gy is None else c.gy.float()
    m = s.mean(1, keepdim=True)
    r = (((s - m) ** 2).mean(1, keepdim=True) + c.eps).rsqrt()
    xh = (s - m) * r
    t = gy * w
    c1, c2 = (t * xh).mean(1, keepdim=True), t.mean(1, keepdim=True)
    gS = r * (t - c2 - xh * c1) + (zero if c.gs is None else c.gs.float())
    gP = gS + (zero if c.gsp is None else c.gsp.float())
    out = dict(dx=store(gP, c.dtype, fault == "truncate"), dweight=(gy * xh).sum(0).double(), dbias=gy.sum(0).double())
    if c.runs:
        src = gS.to(c.dtype).float() if fault == "drow_rounded" else gS
        out["drow"] = src.reshape(c.runs, R // c.runs, C).sum(1).double()
    return out


# (R, C, runs): 7 runs of 11 rows inside one block pass, the slab's tail masked; one row per run at the narrowest width; run boundaries
# inside a pass at C = 320; the widths 1280 and 4096 (no row at 4096)
LN_BWD_SHAPES = [(77, 64, 7), (21, 40, 21), (300, 320, 3), (18, 1280, 2), (12, 4096, 0)]
LN_BWD_F32_SHAPES = [(77, 96, 7)]                                 # L = 4, K = 6 in fp32
LN_BWD_MODE_SHAPE = (77, 64, 7)                                   # every mode of gradient presence runs on this one


def ln_bwd_shapes(tag):
    """The shapes of a type: fp32 rows end at 2048 elements (64 lanes x 8 vectors of 4), so 4096 is a 16-bit width; fp32 adds C = 96."""
    if tag == "f32":
        return [s for s in LN_BWD_SHAPES if s[1] <= 2048] + LN_BWD_F32_SHAPES
    return list(LN_BWD_SHAPES)


# ---- GEGLU backward ---------------------------------------------------------------------------------------------------------------------------

ERF_P, ERF_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)     # Abramowitz-Stegun 7.1.26
ERF_ERR = 1.5e-7                                                  # its stated absolute error on erf (csrc/geglu_math.h)
GATE_SWEEP = (0.0, 2.0 ** -20, 0.5, 1.0, 3.0, 6.0, 9.0, 12.0)
TAIL_FROM = -6.0                                                  # gates at and below: the product form is held to a factor of two
GEGLU_BWD_SHAPES = [(5, 8), (5, 1288), (33, 8), (33, 1288)]


def as_erfc_parts(gate):
    """t, the Horner intermediates h4 .. h1 (poly(t) = h1 t), poly'(t) and e = exp(-g^2 / 2) of the documented polynomial, in fp64."""
    t = 1.0 / (1.0 + ERF_P * gate.abs() / math.sqrt(2.0))
    a1, a2, a3, a4, a5 = ERF_A
    h4 = a5 * t + a4
    h3 = h4 * t + a3
    h2 = h3 * t + a2
    h1 = h2 * t + a1
    dp = a1 + 2 * a2 * t + 3 * a3 * t ** 2 + 4 * a4 * t ** 3 + 5 * a5 * t ** 4
    return t, (h4, h3, h2, h1), dp, torch.exp(-0.5 * gate * gate)


@functools.lru_cache(maxsize=None)
def geglu_bwd_case(tag, rows, inner):
    """geglu_backward against the TRUE gate: dh = [dy g Phi(g) | dy a (Phi(g) + g phi(g))], Phi(g) = erfc(-g / sqrt 2) / 2 and
    phi(g) = exp(-g^2 / 2) / sqrt(2 pi) in fp64. Every second gate is one of +-GATE_SWEEP in turn, the others 2 randn (a tenth of them
    three times that); a and dy are +-2^e (1 + fraction) with e over the type's range — f16: -20 .. 10, down into the subnormals, products
    that underflow included; bf16 / fp32: -40 .. 40 — and e_a <= 11 - e_dy (f16) so that no true result overflows the type.

    Cap. The kernel takes Phi(-|g|) = poly(t) e / 2 from Abramowitz-Stegun 7.1.26, whose stated error on erf, 1.5e-7 absolute, is
    0.75e-7 on Phi; the fp32 evaluation adds: t = 1 / (1 + p |g| / sqrt 2) is 3 u relative (an fma, a reciprocal of an ulp), which moves
    poly by |poly'(t)| t 3 u; the four fmas of Horner's rule round h4 .. h1, each error carried on by powers of t <= 1: u sum|h_k| t^k;
    the product h1 t: u |poly|; e = exp2(g g c): the square, the constant and the product are 1.5 g^2 u relative in e, exp2 itself
    3 u; the two products of poly e / 2: 2 u:
        d_tail = e / 2 (|poly'| t 3 u + u sum|h_k| t^k + u |poly|) + tail (1.5 g^2 + 5) u,      d_Phi = 0.75e-7 + d_tail + u Phi
    (the last for 1 - tail on the positive side). g phi(g) = g e / sqrt(2 pi) is no approximation: d_gphi = |g phi| (1.5 g^2 + 6) u.
        da = dy (g Phi):           cap = |dy g| d_Phi + 2 u |da|
        dg = dy a (Phi + g phi):   cap = |dy a| (d_Phi + d_gphi + u |Phi + g phi|) + 2 u |dg|
    The cap is ABSOLUTE in Phi, as the stated figure is: on the deep negative tail it does not tell a product from 1 - something, whose
    error would be u. `tail` marks the elements with g <= TAIL_FROM and a result above 16 smallest normal numbers of the type (f16, whose
    range ends before the tail does: above 16 of its subnormal steps, where the rounding is still below a thirtieth): there the result must have the reference's sign and lie within a factor of two of it (tail_ok) — the documented polynomial in fp64 is
    within 4 % of the true tail for |g| <= 12 (asserted here), 1 - something is 0 or a multiple of 6e-8."""
    dtype = DTYPES[tag]
    g = gen(43, rows, inner, dtype == torch.float16)
    total = rows * inner
    uni = lambda n: torch.rand(n, generator=g, dtype=torch.float64)
    gate = 2.0 * torch.randn(total, generator=g, dtype=torch.float64)
    gate = torch.where(uni(total) < 0.1, 3.0 * gate, gate).clamp(-12.0, 12.0)
    idx = torch.arange(0, total, 2)
    sweep = torch.tensor([s * v for v in GATE_SWEEP for s in (1.0, -1.0)], dtype=torch.float64)
    gate[idx] = sweep[(idx // 2) % len(sweep)]
    lo, hi, budget = (-20, 10, 11) if dtype == torch.float16 else (-40, 40, 80)
    e_dy = torch.floor(lo + uni(total) * (hi - lo + 1))
    e_a = torch.floor(lo + uni(total) * (torch.minimum(torch.full_like(e_dy, hi), budget - e_dy) - lo + 1))
    sign = lambda: torch.where(uni(total) < 0.5, -1.0, 1.0).double()
    dy = q(sign() * torch.ldexp(1.0 + uni(total), e_dy.int()), dtype).reshape(rows, inner)
    a = q(sign() * torch.ldexp(1.0 + uni(total), e_a.int()), dtype).reshape(rows, inner)
    gate = q(gate, dtype).reshape(rows, inner)
    rt2 = math.sqrt(2.0)
    Phi = 0.5 * torch.special.erfc(-gate / rt2)
    gphi = gate * torch.exp(-0.5 * gate * gate) / math.sqrt(2.0 * math.pi)
    da, dg = dy * gate * Phi, dy * a * (Phi + gphi)
    t, hs, dp, e = as_erfc_parts(gate)
    poly = hs[3] * t
    tail = 0.5 * poly * e
    true_tail = 0.5 * torch.special.erfc(gate.abs() / rt2)
    assert (tail - true_tail).abs().max().item() <= 0.5 * ERF_ERR                  # the documented polynomial keeps its stated error
    assert ((tail - true_tail).abs() / true_tail).max().item() < 0.04
    horner = sum(h.abs() * t ** k for k, h in enumerate(reversed(hs)))
    d_tail = 0.5 * e * (dp.abs() * t * 3.0 * U + U * horner + U * poly.abs()) + tail * (1.5 * gate * gate + 5.0) * U
    d_Phi = 0.5 * ERF_ERR + d_tail + U * Phi
    d_gphi = gphi.abs() * (1.5 * gate * gate + 6.0) * U
    cap = torch.cat([(dy * gate).abs() * d_Phi + 2.0 * U * da.abs(), (dy * a).abs() * (d_Phi + d_gphi + U * (Phi + gphi).abs()) + 2.0 * U * dg.abs()], 1)
    ref = torch.cat([da, dg], 1)
    floor = 16.0 * 2.0 ** (MIN_EXP[dtype] - (10 if dtype == torch.float16 else 0))
    deep = torch.cat([gate <= TAIL_FROM, torch.zeros_like(gate, dtype=torch.bool)], 1) & (ref.abs() >= floor)
    c = Case(tag=tag, dtype=dtype, rows=rows, inner=inner, h=torch.cat([a, gate], 1), dy=dy, ref=ref, cap=cap, bound=bound(ref, cap, dtype),
             quarter=quarter_share(ref, cap, dtype), tail=deep)
    c.wide = float((cap > 0.5 * ulp_of(ref, dtype)).double().mean())              # share of elements whose cap exceeds half an ulp
    return c


def tail_ok(got, c):
    """Number of deep-tail elements (c.tail) whose result has the wrong sign or is not within a factor of two of the reference."""
    g, r = got.double()[c.tail], c.ref[c.tail]
    return int(((g * r <= 0) | (g.abs() < 0.5 * r.abs()) | (g.abs() > 2.0 * r.abs())).sum())


def geglu_bwd_f32(c, fault=None):
    """The plain fp32 restatement (Phi from the library's fp32 erfc on the side of the tail), stored in the case's type; faults:
    'truncate', 'one_minus' (Phi(-|g|) formed as 1 - Phi(|g|))."""
    h, dy = c.h.float(), c.dy.float()
    a, g = h[:, :c.inner], h[:, c.inner:]
    tail = 0.5 * torch.special.erfc(g.abs() * (1.0 / math.sqrt(2.0)))
    if fault == "one_minus":
        tail = 1.0 - (1.0 - tail)
    Phi = torch.where(g < 0, tail, 1.0 - tail)
    gphi = g * torch.exp(-0.5 * g * g) * (1.0 / math.sqrt(2.0 * math.pi))
    return store(torch.cat([dy * (g * Phi), dy * a * (Phi + gphi)], 1), c.dtype, fault == "truncate")

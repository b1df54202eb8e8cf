"""Data with exactly one right answer for the attention kernels (attn_flash.hip, attn_flash8m16.hip, attn_rowtile.hip,
attn_temporal.hip and attn_bwd.hip under multiview_inpaint_amd/csrc/, as every kernel file named below), the fp64 expectations
of tests/test_attention_exact_gpu.py and the case lists it shares with tests/test_attention_exact_cpu.py (which checks every
precondition stated here on the CPU and shows that the comparisons notice
eight planted faults). Pure torch on the CPU; nothing outside the repository is read.

Token-major layout as in hip_ops.attention: q [B, Sq, H D], k and v [B, Sk, H D]. The data sets:
  * selector  every key j carries a +-c code, query i the code of its chosen key j(i): softmax is one-hot to far below the storage
              type's half ulp and out[i] = v[j(i)] BIT FOR BIT. The codes are the binary index of j repeated over the D channels
              (minimum Hamming distance D // bits, not left to chance), flipped by a random mask per (batch, head). v holds random
              bit patterns of the type (random sign and significand, exponent in a window of 2^8: the other keys enter with weight
              2^-gap times THEIR v, so the budget below is taken against max |v| / min |v|). j(i) covers the first and the last valid
              key, every ring slot, the first tile, later tiles only, the ragged tile, a key nobody chose and one chosen twice.
  * uniform   all keys of a (batch, head) are one vector: every valid probability is exactly 1 (identical arithmetic per key), v in
              {+-1, +-2, +-3} with every column summing to zero over the valid keys: out is +-0 everywhere. A dropped, doubled or
              leaked key leaves a non-zero integer in the accumulator, and zero is where storage rounding hides nothing.
  * comb      (comb_case) 32 codes, each carried by n = 2^k keys spread over every tile, every row's maximum inside the first 32 keys:
              the set that keeps the 8-wave kernel in its FAST form. out = (sum of the group's v) / n.
  * pairs     selector codes carried by exactly two keys a = g, b = g + Sk / 2 (different 64-key tiles for every pair from 128 keys on
              and for the pairs that reach the second tile below that; different passes of the 4-slot ring from 512 keys on):
              out = (v_a + v_b) / 2 rounded once. v_a in [2^(p+1), 2^(p+2)) and |v_b| in 1..4 of the
              same sign: a quarter of the results are exact ties, half need rounding, a quarter are exact.
All scores below are in log2 units (what the kernels exponentiate with exp2)."""
import functools
import math

import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}
LOG2E = 1.4426950408889634
BUDGET = 2.0 ** -14                      # a quarter of f16's half ulp: what the non-selected mass and the score rounding may each reach
V_EXP_WINDOW = 8                         # selector v: exponents in [-4, 4)
KT = 64                                  # keys per tile of both flash kernels
RING = 4                                 # K / V ring slots of the 8-wave kernel
FIRST_BLOCK = 32                         # the 8-wave kernel's fast path takes its exponent from the first 32 keys


def gen(*key):
    """A generator seeded by the case: a test never depends on which other tests ran."""
    seed = 23
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rnd(x, dtype):
    """fp64 -> the nearest number of `dtype`, as fp64."""
    return x.to(dtype).double()


def ulp_of(v, dtype):
    _, ex = torch.frexp(v.abs().double())
    ex = torch.clamp(ex, min=MIN_EXP[dtype] + 1)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - SIG_BITS[dtype])


def is_tie(ref, dtype):
    return (ref - rnd(ref, dtype)).abs() == 0.5 * ulp_of(ref, dtype)


def needs_rounding(ref, dtype):
    return rnd(ref, dtype) != ref


def truncate_to(v, dtype):
    """v rounded TOWARD ZERO to `dtype` (a planted fault), as fp64."""
    u = ulp_of(v, dtype)
    return torch.sign(v) * torch.floor(v.abs() / u) * u


def tok(x):
    """[B, H, S, D] -> token-major [B, S, H D]."""
    B, H, S, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, S, H * D).contiguous()


def heads(x, H):
    """[B, S, H D] -> [B, H, S, D]."""
    B, S, HD = x.shape
    return x.reshape(B, S, H, HD // H).permute(0, 2, 1, 3)


def to_temporal(x, Bo, S):
    """[(Bo S), T, C] (one softmax problem per video and spatial token) -> [(Bo T), S, C] as the temporal entries take it."""
    _, T, C = x.shape
    return x.reshape(Bo, S, T, C).transpose(1, 2).reshape(Bo * T, S, C).contiguous()


def from_temporal(x, Bo, T):
    _, S, C = x.shape
    return x.reshape(Bo, T, S, C).transpose(1, 2).reshape(Bo * S, T, C).contiguous()


def kernel_variant(Sq, Sk, D, tag):
    """What mvi_attention_kernel_variant answers (the GPU tests assert that it does): 0 rowtile, 4 / 16 the 4- / 8-wave MFMA kernel."""
    if tag == "f32" or D != 64 or Sk <= 32:
        return 0
    return 16 if Sq >= 1024 and Sk >= 256 else 4


def folds_scale(Sq, Sk, D, tag):
    """The 8-wave kernel rounds scale log2(e) into Q for f16 (attention_folds_scale in attn_api.hip)."""
    return kernel_variant(Sq, Sk, D, tag) == 16 and tag == "f16"


def code_magnitude(D):
    """The largest integer c with a match score c^2 sqrt(D) log2(e) <= 500 log2 units (the score-rounding budget ends at 512):
    7 at D = 32 (400, 25 per differing channel), 9 at D = 16 (467, 58); D = 64: code_magnitudes."""
    return int(math.floor(math.sqrt(500.0 / (math.sqrt(D) * LOG2E))))


def code_magnitudes(D):
    """(|q|, |k|) of the codes. D = 16, 32: (c, c). D = 64: (5, 8) — a match score of 2560, 461.7 log2 units, 14.4 per differing channel
    — instead of (6, 6): the 4-wave kernel takes its reference exponent as the ROUNDED product max * scale log2 e and P of the selected
    key is 2^(what that rounding lost). fp32(2560 * fp32(log2 e / 8)) lies ABOVE the exact product, so that P is 1 - 8e-6: a kernel
    that truncated P to the type instead of rounding it would store 1 - ulp, and the selector set sees it (at 2304 the product rounds
    down, P is 1 + 1e-5, and truncation would go unnoticed; tests/test_attention_exact_cpu.py plants that fault)."""
    return (5.0, 8.0) if D == 64 else (float(code_magnitude(D)),) * 2


def code_bits(n):
    return max(1, (max(n, 2) - 1).bit_length())


def codes(n, D):
    """[n, D] of +-1: the binary index repeated D // bits times, the rest +1. Two different indices differ in >= D // bits channels."""
    nb = code_bits(n)
    r = D // nb
    assert r >= 1, (n, D)
    idx = torch.arange(n)
    bits = torch.stack([(idx >> b) & 1 for b in range(nb)], 1)              # [n, nb]
    out = torch.ones(n, D, dtype=torch.float64)
    out[:, :nb * r] = (1.0 - 2.0 * bits.double()).repeat(1, r)
    return out, r


def q_operand(code_q, D, tag, mode, fold):
    """-> (q, the q the scores are taken with, the factor that takes q . k to log2 units, |k|) for +-1 codes.
    mode "scale": q = +-c, the kernel applies D^-1/2 (and log2 e). Where it folds (f16, 8-wave) the scores it sees come from
    q' = f16(fp32(q) * fp32(scale log2 e)) — returned as the second tensor, the one the fp64 check scores with.
    mode "q_log2": q = +-(c D^-1/2 log2 e rounded to the type), the kernel applies nothing (ln 2 where it exponentiates with e)."""
    dtype = DTYPES[tag]
    cq, ck = code_magnitudes(D)
    scale = float(D) ** -0.5
    if mode == "q_log2":
        q = code_q * rnd(torch.tensor(cq * scale * LOG2E, dtype=torch.float64), dtype).item()
        return q, q, 1.0, ck
    q = code_q * cq
    if fold:
        return q, folded_q(q, D, dtype), 1.0, ck
    return q, q, scale * LOG2E, ck


def folded_q(q, D, dtype):
    """q as the 8-wave f16 kernel scores with it: fp32(q) * fp32(D^-1/2 log2 e), rounded to the type."""
    sl2 = torch.tensor(float(D) ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    return (q.float() * sl2).to(dtype).double()


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


BLOCK8 = 256                             # query rows per block of the 8-wave kernel


def block_last_rows(Sq):
    """The last row of every 256-row block of the 8-wave kernel."""
    return sorted({min(r + BLOCK8, Sq) - 1 for r in range(0, Sq, BLOCK8)})


def free_rows(g, Sq, n, taken):
    """n seeded rows outside `taken`."""
    rows = [r for r in torch.randperm(Sq, generator=g).tolist() if r not in set(taken)]
    return torch.tensor(rows[:n], dtype=torch.long)


def assert_blocks_repeat(s, tag, what):
    """The 8-wave kernel first runs every 256-row block in its fast form (reference exponent = row maximum of the first 32 keys) and
    repeats the block with the online form if a row sum leaves [0, 2^100] ([0, 2^15] in f16). Asserted here, in fp64 with a factor
    of sqrt(2) to either side of the limit (the gaps are multiples of 14.4: seven of them are 2^100.99; bf16's P errs by 2^-8):
    EVERY block of this case has a row beyond it, so every block repeats — the selected keys then
    carry P = 1 exactly (the online form puts the exponent on the selected score) and l is the exact count."""
    limit = 15.0 if tag == "f16" else 100.0
    m = s[..., :FIRST_BLOCK].amax(-1, keepdim=True)
    log2_l = torch.log2(torch.exp2(s - s.amax(-1, keepdim=True)).sum(-1)) + (s.amax(-1) - m.squeeze(-1))
    assert ((log2_l - limit).abs() >= 0.5).all(), f"{what}: a row sum within sqrt(2) of the fast form's limit"
    Sq = s.shape[2]
    for r0 in range(0, Sq, BLOCK8):
        over = (log2_l[:, :, r0:r0 + BLOCK8] > limit).any(-1)
        assert over.all(), f"{what}: the block at row {r0} stays in the fast form"


def far_code(base, exclude=()):
    """The code index >= 32 farthest (in Hamming distance) from all of the first 32: what a forced row asks for."""
    D = base.shape[1]
    near = ((D - base @ base[:FIRST_BLOCK].T) / 2).amin(-1)
    near[:FIRST_BLOCK] = -1
    for j in exclude:
        near[j] = -1
    return int(near.argmax())


def selector_map(g, Sq, Sk, forced=(), far=None):
    """j(i) for one (batch, head), and the key nobody chooses (None below 3 keys). forced: rows that choose the key `far`."""
    tiles = (Sk + KT - 1) // KT
    unchosen = Sk // 2 if Sk >= 3 else None
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    must = [0, Sk - 1, 0]                                                  # first, last, and the first a second time
    for slot in range(min(RING, tiles)):
        t = max(t for t in range(tiles) if t % RING == slot)
        must.append(ri(t * KT, min(Sk, (t + 1) * KT)))
    must.append(ri(0, min(FIRST_BLOCK, Sk)))
    if Sk > FIRST_BLOCK:
        must.append(ri(FIRST_BLOCK, Sk))
    if Sk > KT:
        must.append(ri(KT, Sk))
    if Sk % KT:
        must.append(ri(KT * (tiles - 1), Sk))
    must = [j for j in must if j != unchosen][:Sq]
    jmap = torch.randint(0, Sk, (Sq,), generator=g)
    if unchosen is not None:
        jmap[jmap == unchosen] = 0
    pos = free_rows(g, Sq, len(must), forced)
    jmap[pos] = torch.tensor(must[:len(pos)], dtype=jmap.dtype)
    for r in forced:
        jmap[r] = far
    return jmap, unchosen


def coverage(jmap, unchosen, Sq, Sk):
    """Which of the issue's j(i) requirements a map meets (those its shape can meet are asserted by the CPU test)."""
    tiles = (Sk + KT - 1) // KT
    counts = torch.bincount(jmap, minlength=Sk)
    return dict(first=bool((jmap == 0).any()), last=bool((jmap == Sk - 1).any()), first_tile=bool((jmap < FIRST_BLOCK).any()),
                later=bool((jmap >= KT).any()), later_block=bool((jmap >= FIRST_BLOCK).any()),
                ragged=bool((jmap >= KT * (tiles - 1)).any()), slots=sorted(set(((jmap // KT) % RING).tolist())),
                unchosen=unchosen is not None and int(counts[unchosen]) == 0, multi=bool((counts >= 2).any()))


def random_bits(g, shape, dtype):
    """Random bit patterns of `dtype` with the exponent in [-4, 4): random sign and significand, no zero, fp64 out."""
    p = SIG_BITS[dtype] if dtype != torch.float32 else 12                  # fp32 I/O: at most 12 significant bits
    mant = torch.randint(0, 2 ** (p - 1), shape, generator=g).double() / 2 ** (p - 1)
    ex = torch.randint(-V_EXP_WINDOW // 2, V_EXP_WINDOW // 2, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return sign * torch.ldexp(1.0 + mant, ex)


def small_ints(g, shape, hi=3):
    return (torch.randint(0, 2, shape, generator=g).double() * 2 - 1) * torch.randint(1, hi + 1, shape, generator=g).double()


def zero_sum_columns(g, lead, n, D):
    """[*lead, n, D] in {+-1, +-2, +-3}, never 0, every column summing to zero over n (n >= 2): pairs (a, -a) — and one triple
    +-(1, 1, -2) where n is odd — in a random order per column."""
    assert n >= 2
    shape = tuple(lead)
    parts = []
    m = n
    if n % 2:
        s = torch.randint(0, 2, shape + (1, D), generator=g).double() * 2 - 1
        parts.append(torch.cat([s, s, -2 * s], -2))
        m -= 3
    if m:
        a = small_ints(g, shape + (m // 2, D))
        parts += [a, -a]
    v = torch.cat(parts, -2)
    order = torch.rand(shape + (n, D), generator=g).argsort(-2)
    return torch.gather(v, -2, order)


def _log2_scores(qs, k, mult):
    return mult * (qs @ k.transpose(-1, -2))


def assert_budgets(s, sel, vratio, what):
    """The two disturbance budgets of the selector / pairs sets, in fp64 on every row: the non-selected mass (times max |v| / min |v|)
    and the score rounding |s|max 2^-23, each at most 2^-14. sel: bool [.., Sq, Sk] of the selected keys, all at the row's maximum.
    -> (mass max, smallest gap between a selected and a non-selected score)."""
    top = s.masked_fill(~sel, -math.inf).amax(-1, keepdim=True)
    low = s.masked_fill(sel, -math.inf)
    assert torch.equal(s.masked_fill(~sel, 0.0), (top * sel).masked_fill(~sel, 0.0)), f"{what}: selected keys do not share one score"
    mass = torch.exp2(low - top).sum(-1)
    gap = (top.squeeze(-1) - low.amax(-1)).min().item()                   # (inf where every key is selected)
    smax = s.abs().max().item()
    assert mass.max().item() * vratio <= BUDGET, f"{what}: non-selected mass {mass.max().item():.3e} x v range {vratio}"
    assert smax * 2.0 ** -23 <= BUDGET, f"{what}: |s|max = {smax} log2 units"
    return mass.max().item(), gap


@functools.lru_cache(maxsize=None)
def selector_case(tag, B, H, Sq, Sk, D, mode="scale", int_v=False):
    """Set 1. int_v: v in {+-1 .. +-7} (the backward's precondition: dout . v is then an exact small integer)."""
    dtype = DTYPES[tag]
    g = gen(1, B, H, Sq, Sk, D, len(tag), len(mode), int_v)
    base, dist = codes(Sk, D)
    mask = torch.randint(0, 2, (B, H, 1, D), generator=g).double() * 2 - 1
    eight = kernel_variant(Sq, Sk, D, tag) == 16
    forced = block_last_rows(Sq) if eight else ()      # the last row of every 8-wave block asks for a far key: the block repeats
    far = far_code(base, (Sk // 2,)) if eight else None
    maps = [[selector_map(g, Sq, Sk, forced, far) for _ in range(H)] for _ in range(B)]
    jmap = torch.stack([torch.stack([m[0] for m in row]) for row in maps])               # [B, H, Sq]
    fold = folds_scale(Sq, Sk, D, tag)
    kcode = base[None, None] * mask                                                       # [B, H, Sk, D]
    qcode = torch.gather(kcode, 2, jmap[..., None].expand(B, H, Sq, D))
    q, qs, mult, ck = q_operand(qcode, D, tag, mode, fold)
    k = kcode * ck
    v = small_ints(g, (B, H, Sk, D), 7) if int_v else random_bits(g, (B, H, Sk, D), dtype)
    for t in (q, k, v):
        assert torch.equal(rnd(t, dtype), t)
    s = _log2_scores(qs, k, mult)
    sel = torch.zeros(B, H, Sq, Sk, dtype=torch.bool).scatter_(3, jmap[..., None], True)
    vratio = (v.abs().max() / v.abs().min()).item()
    mass, gap = assert_budgets(s, sel, vratio, f"selector {tag} {(B, H, Sq, Sk, D)} {mode}")
    if eight:
        assert_blocks_repeat(s, tag, f"selector {tag} {(B, H, Sq, Sk, D)} {mode}")
    want = torch.gather(v, 2, jmap[..., None].expand(B, H, Sq, D))
    s_match = torch.gather(s, 3, jmap[..., None]).squeeze(-1)                             # [B, H, Sq], log2 units
    cov = [[coverage(m[0], m[1], Sq, Sk) for m in row] for row in maps]
    return Case(kind="selector", q=tok(q), k=tok(k), v=tok(v), want=tok(want).to(dtype), jmap=jmap, mass=mass, gap=gap, dist=dist,
                c=max(code_magnitudes(D)),
                lse=s_match / LOG2E, s_match=s_match, cov=cov, H=H, D=D, mode=mode, vmax=v.abs().max().item())


@functools.lru_cache(maxsize=None)
def uniform_case(tag, B, H, Sq, Sk, D, mode="scale", signed=False):
    """Set 2 (Sk >= 2). -> out == +-0. The first D / 2 channels of q are one fixed vector w per (batch, head) and kappa is non-zero
    only there: every
    row of a (batch, head) has the SAME score w . kappa (so the backward's recomputed P is one constant), while the rows of q differ
    in the other half."""
    dtype = DTYPES[tag]
    g = gen(2, B, H, Sq, Sk, D, len(tag), len(mode), signed)
    half = D // 2
    kappa = torch.zeros(B, H, 1, D, dtype=torch.float64)
    kappa[..., :half] = small_ints(g, (B, H, 1, half))
    # w takes kappa's signs: the score w . kappa is positive and lse = scale s + ln(Sk) adds two positive terms. The bar on lse,
    # 4 x 2^-23 max(|lse|, 1), is the fp32 log and the multiply of the LARGER term: it cannot hold where the two cancel (seen on the
    # MI355X with random signs: f16 (1, 2, 1025, 257), lse = -6.12 + 5.55, 4.4 x 2^-23 — m alone is rounded to 2^-24 of 8.8).
    # signed: random signs instead, at least one head with a negative score (asserted). Its lse is held relative to `lse_scale` =
    # max(|scale s|, ln Sk, 1), the larger of the two terms that are added.
    w = small_ints(g, (B, H, 1, half))
    if signed:
        w[0, 0] = -w[0, 0].abs() * torch.sign(kappa[0, 0, :, :half])
    else:
        w = w.abs() * torch.sign(kappa[..., :half])
    q = torch.cat([w.expand(B, H, Sq, half), torch.randint(-3, 4, (B, H, Sq, D - half), generator=g).double()], -1).contiguous()
    if mode == "q_log2":                                                   # small multiples of 1/8 stand in for the folded scale
        q = q / 8.0
    k = kappa.expand(B, H, Sk, D).contiguous()
    v = zero_sum_columns(g, (B, H), Sk, D)
    assert q.abs().sum() > 0 and (v != 0).all(), "uniform data: a zero in v"
    assert torch.equal(v.sum(2), torch.zeros(B, H, D, dtype=torch.float64)), "uniform data: a column does not sum to zero"
    assert 3 * Sk < 2 ** 24
    for t in (q, k, v):
        assert torch.equal(rnd(t, dtype), t)
    mult = 1.0 if mode == "q_log2" else float(D) ** -0.5 * LOG2E
    qs = q
    if mode == "scale" and folds_scale(Sq, Sk, D, tag):
        qs, mult = folded_q(q, D, dtype), 1.0
    s = mult * (qs[:, :, :1] @ kappa.transpose(-1, -2)).reshape(B, H, 1)                  # one score per (batch, head)
    assert torch.equal(_log2_scores(qs, k, mult), s[..., None].expand(B, H, Sq, Sk)), "uniform data: the scores of a row differ"
    assert s.abs().max().item() * 2.0 ** -23 <= BUDGET and (s.min().item() < 0 if signed else s.min().item() > 0)
    lse = (s / LOG2E + math.log(Sk)).expand(B, H, Sq)
    lse_scale = torch.clamp((s / LOG2E).abs(), min=max(math.log(Sk), 1.0)).expand(B, H, Sq)
    return Case(kind="uniform", q=tok(q), k=tok(k), v=tok(v), want=torch.zeros(B, Sq, H * D, dtype=dtype), lse=lse, lse_scale=lse_scale,
                s=s, H=H, D=D, mode=mode)


def pair_layout(Sk):
    """Keys of group g: a = g and b = g + G (+ 1 behind the spare key G where Sk is odd), G = Sk // 2 groups: the last valid key is a b."""
    G = Sk // 2
    a = torch.arange(G)
    b = a + G + (Sk % 2)
    return G, a, b


@functools.lru_cache(maxsize=None)
def pairs_case(tag, B, H, Sq, Sk, D, mode="scale"):
    """Set 3 (Sk >= 2). -> want = the fp64 (v_a + v_b) / 2 rounded once; `tie` marks the exact ties."""
    dtype = DTYPES[tag]
    p = SIG_BITS[dtype] if dtype != torch.float32 else 10
    g = gen(3, B, H, Sq, Sk, D, len(tag), len(mode))
    G, a, b = pair_layout(Sk)
    base, dist = codes(G + 1, D)                                           # code G: the spare key of an odd Sk, chosen by nobody
    group_of = torch.full((Sk,), G, dtype=torch.long)
    group_of[a] = torch.arange(G)
    group_of[b] = torch.arange(G)
    mask = torch.randint(0, 2, (B, H, 1, D), generator=g).double() * 2 - 1
    gmap = torch.randint(0, G, (B, H, Sq), generator=g)
    must = torch.tensor([0, G - 1, G // 2][:Sq])
    eight = kernel_variant(Sq, Sk, D, tag) == 16
    forced = block_last_rows(Sq) if eight else []      # the last row of every 8-wave block asks for a far pair: the block repeats
    far = far_code(base[:G]) if eight else 0
    for bi in range(B):
        for hi in range(H):
            gmap[bi, hi, free_rows(g, Sq, len(must), forced)] = must
            gmap[bi, hi, forced] = far
    kcode = base[group_of][None, None] * mask
    qcode = torch.gather(base[None, None] * mask, 2, gmap[..., None].expand(B, H, Sq, D))
    fold = folds_scale(Sq, Sk, D, tag)
    q, qs, mult, ck = q_operand(qcode, D, tag, mode, fold)
    k = kcode * ck
    sign = torch.randint(0, 2, (B, H, G, D), generator=g).double() * 2 - 1
    big = sign * (2.0 ** (p + 1) + 4.0 * torch.randint(0, 2 ** (p - 1), (B, H, G, D), generator=g).double())
    small = sign * torch.randint(1, 5, (B, H, G, D), generator=g).double()
    v = torch.ones(B, H, Sk, D, dtype=torch.float64)
    v[:, :, a] = big
    v[:, :, b] = small
    for t in (q, k, v):
        assert torch.equal(rnd(t, dtype), t)
    s = _log2_scores(qs, k, mult)
    sel = (group_of[None, None, None, :] == gmap[..., None])
    assert (sel.sum(-1) == 2).all()
    mass, gap = assert_budgets(s, sel, 1.0, f"pairs {tag} {(B, H, Sq, Sk, D)} {mode}")
    if eight:                                          # -> P = 1 for both keys, l = 2 and inv = 0.5 exactly: ties are held bit for bit
        assert_blocks_repeat(s, tag, f"pairs {tag} {(B, H, Sq, Sk, D)} {mode}")
    # the other keys enter with 2^-gap |v_j| against |v_a + v_b| >= 2^(p+1): the budget against the largest |v|
    assert mass * v.abs().max().item() / 2.0 ** (p + 1) <= BUDGET
    pick = lambda t: torch.gather(t, 2, gmap[..., None].expand(B, H, Sq, D))
    ref = (pick(big) + pick(small)) / 2
    # P (at most p bits) times v_a + v_b (p + 2 bits) is exact in fp32, and so is either product alone
    assert 2 * p + 2 <= 24 and (pick(big) + pick(small)).abs().max().item() <= 2.0 ** (p + 2)
    tie = is_tie(ref, dtype)
    frac = needs_rounding(ref, dtype).double().mean().item()
    ties = int(tie.sum())
    assert dtype == torch.float32 or (ties >= 1 and frac > 0.5), f"pairs data: {ties} ties, {frac:.3f} need rounding in {dtype}"
    s_match = torch.gather(s, 3, a[gmap][..., None]).squeeze(-1)
    ta, tb = a // KT, b // KT
    return Case(kind="pairs", q=tok(q), k=tok(k), v=tok(v), ref=tok(ref), want=tok(ref).to(dtype), tie=tok(tie), gmap=gmap, mass=mass,
                gap=gap, lse=(s_match + 1.0) / LOG2E, cross_tile=int((ta != tb).sum()), cross_ring=int(((tb - ta) >= RING).sum()), H=H, D=D,
                mode=mode, a=a, b=b)


COMB_GROUPS = 32


@functools.lru_cache(maxsize=None)
def comb_case(tag, B, H, Sq, Sk, D, mode="scale"):
    """A fourth set, for the FAST form of the 8-wave kernel (the one production runs): its reference exponent is the row maximum of the
    first 32 keys and never moves, and a block repeats with the online form as soon as one of its 256 rows sees a score ~69 above
    that — which every block of the selector and pairs sets does (assert_blocks_repeat), so those two hold the online form
    and only the uniform set, whose rows are all alike, would hold the fast one. Here key j carries code j mod 32 for j < 32 n, n the
    largest power of two with 32 n <= Sk (the keys behind carry a 33rd code nobody asks for): every row's maximum is reached inside the
    first 32 keys (asserted: the fast form's row sum is n <= 64, far inside its range in both types), P = 1 for the n keys of the
    chosen group, spread over every tile and ring slot, and out = (sum of their v) / n — a power of two, so the normalisation is exact
    where the row sum is that of the rounded P (8-wave: bit for bit); the 4-wave kernel divides by n (1 + e) and may break an exact
    tie, as in the pairs set. v: integers of up to p bits, one sign per (group, channel): |sum| >= n, no result is 0."""
    dtype = DTYPES[tag]
    p = SIG_BITS[dtype] if dtype != torch.float32 else 10
    g = gen(6, B, H, Sq, Sk, D, len(tag), len(mode))
    NG = COMB_GROUPS
    n = 1 << ((Sk // NG).bit_length() - 1)
    group_of = torch.where(torch.arange(Sk) < NG * n, torch.arange(Sk) % NG, torch.tensor(NG))
    base, dist = codes(NG + 1, D)
    mask = torch.randint(0, 2, (B, H, 1, D), generator=g).double() * 2 - 1
    gmap = torch.randint(0, NG, (B, H, Sq), generator=g)
    must = torch.tensor([0, NG - 1])
    for bi in range(B):
        for hi in range(H):
            gmap[bi, hi, torch.randperm(Sq, generator=g)[:2]] = must
    kcode = base[group_of][None, None] * mask
    qcode = torch.gather(base[None, None] * mask, 2, gmap[..., None].expand(B, H, Sq, D))
    q, qs, mult, ck = q_operand(qcode, D, tag, mode, folds_scale(Sq, Sk, D, tag))
    k = kcode * ck
    sign = (torch.randint(0, 2, (B, H, NG + 1, D), generator=g).double() * 2 - 1)[:, :, group_of]
    v = sign * torch.randint(1, 2 ** p, (B, H, Sk, D), generator=g).double()
    for t in (q, k, v):
        assert torch.equal(rnd(t, dtype), t)
    s = _log2_scores(qs, k, mult)
    sel = group_of[None, None, None, :] == gmap[..., None]
    assert (sel.sum(-1) == n).all() and n * 2 ** p < 2 ** 24
    mass, gap = assert_budgets(s, sel, 2.0 ** p / n, f"comb {tag} {(B, H, Sq, Sk, D)} {mode}")
    assert torch.equal(s[..., :FIRST_BLOCK].amax(-1), s.amax(-1)), "comb data: a row's maximum lies behind the first 32 keys"
    onehot = torch.zeros(NG + 1, Sk, dtype=torch.float64)
    onehot[group_of, torch.arange(Sk)] = 1.0
    sums = onehot[None, None] @ v                                                         # [B, H, NG + 1, D]
    ref = torch.gather(sums, 2, gmap[..., None].expand(B, H, Sq, D)) / n
    assert ref.abs().min().item() >= 1.0
    frac = needs_rounding(ref, dtype).double().mean().item()
    assert dtype == torch.float32 or n < 4 or frac > 0.5, f"comb data: {frac:.3f} need rounding"
    s_match = s.amax(-1)
    return Case(kind="comb", q=tok(q), k=tok(k), v=tok(v), ref=tok(ref), want=tok(ref).to(dtype), tie=tok(is_tie(ref, dtype)), gmap=gmap,
                mass=mass, gap=gap, n=n, lse=(s_match + math.log2(n)) / LOG2E, H=H, D=D, mode=mode)


# ---- the backward's data: dout in {+-1, +-2, +-3} -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def selector_bwd_case(tag, B, H, Sq, Sk, D=64):
    """Set 1 under the backward: v in {+-1 .. +-7} (every dout . v is an exact integer below 2^24), P one-hot after rounding to the type.
    -> dv = the fp64 sum of dout over the rows that chose the key, cast (an exact integer); the bounds on what must vanish:
       dq, dv where nobody chose: `tiny` — the other keys' P is 2^-gap, a bf16 number, so bf16 leaves 2^-gap-sized dust (exactly 0 in
           f16, where P below 2^-25 rounds to 0);
       dv where the chosen rows' dout cancel: `tiny + dv_cap` in bf16. The matrix pipe does not round its fp32 sums to nearest: 2 plus
           dust of the other sign comes out as the fp32 number below 2, and the -2 that follows leaves -2^-23 (seen on the MI355X, bf16
           (1, 2, 130, 200); a non-zero sum hides it under the store's rounding). dv_cap = 2 Sq 2^-24 sum_{i: j(i) = j} |dout_i|, the
           summation cap of tests/exact_gemm_helpers.py; f16 has no dust and stays at +-0;
       dk: the dK/dV kernel takes delta = sum_j P dP in fp32 with the UNROUNDED recomputed P of the selected key, 2^x with
           |x| <= X = 8 2^-23 max(|s| log2, 1) (four units of the lse bar, one each for lse log2 e, the fma and v_exp_f32, one spare):
           dS at the selected key is P (1 - P) dP, not 0. |dk[j, d]| <= scale |q| 1.02 ln2 X sum_{i: j(i) = j} |dP_i| + tiny,
           a few 1e-4 of what ONE wrong unit of P would move dk by."""
    c = selector_case(tag, B, H, Sq, Sk, D, "scale", True)
    dtype = DTYPES[tag]
    g = gen(4, B, H, Sq, Sk, len(tag))
    dout = small_ints(g, (B, H, Sq, D))
    v = heads(c.v, H)
    idx = c.jmap[..., None].expand(B, H, Sq, D)
    dv = torch.zeros(B, H, Sk, D, dtype=torch.float64).scatter_add_(2, idx, dout)
    dp_match = (dout * torch.gather(v, 2, idx)).sum(-1)                                   # [B, H, Sq] = delta
    assert (dout.abs() @ v.abs().transpose(-1, -2)).max().item() < 2 ** 24 and dv.abs().max().item() < 2 ** SIG_BITS[dtype]
    scale = float(D) ** -0.5
    tiny = 4.0 * max(Sq, Sk) * 2.0 ** -c.gap * (2 * D * 3 * 7) * c.c
    X = 8.0 * 2.0 ** -23 * max(c.s_match.abs().max().item(), 1.0)
    eps = 1.02 * math.log(2.0) * X                                         # |1 - P| of the selected key
    dk_bound = scale * code_magnitudes(D)[0] * eps * torch.zeros(B, H, Sk, dtype=torch.float64).scatter_add_(2, c.jmap, dp_match.abs())
    chosen = torch.zeros(B, H, Sk, dtype=torch.bool).scatter_(2, c.jmap, True)
    dv_cap = 2.0 * Sq * 2.0 ** -24 * torch.zeros(B, H, Sk, D, dtype=torch.float64).scatter_add_(2, idx, dout.abs())
    return Case(kind="selector", fwd=c, dout=tok(dout), dv=tok(dv), dv_want=tok(dv).to(dtype), chosen=chosen, tiny=tiny, eps=eps,
                dv_cap=tok(dv_cap),
                dk_bound=tok(dk_bound[..., None].expand(B, H, Sk, D)) + tiny, H=H, D=D)


@functools.lru_cache(maxsize=None)
def uniform_bwd_case(tag, B, H, Sq, Sk, D=64):
    """Set 2 under the backward: dout's columns sum to zero over the queries of each (batch, head) and P is one constant, so dv == 0
    exactly (3 Sq multiples of one p-bit number stay below 2^24). dq and dk against the fp64 formula under
        |got - ref| <= scale (2^-(p-1) + 2 n 2^-24) (|dS| (*) |k or q|) + ulp(|ref| + that) / 2
    — dS is rounded to the type as an MFMA operand (2^-p relative; the second 2^-p covers the recomputed P, 2^x with |x| <= 1e-5 here,
    and the fp32 delta), n terms are summed in fp32 (any order, doubled for the matrix pipe), the store rounds once."""
    c = uniform_case(tag, B, H, Sq, Sk, D)
    dtype = DTYPES[tag]
    p = SIG_BITS[dtype]
    g = gen(5, B, H, Sq, Sk, len(tag))
    dout = zero_sum_columns(g, (B, H), Sq, D)
    assert 3 * Sq * 2 ** p < 2 ** 24
    q, k, v = (heads(t, H) for t in (c.q, c.k, c.v))
    scale = float(D) ** -0.5
    P = torch.full((B, H, Sq, Sk), 1.0 / Sk, dtype=torch.float64)
    dP = dout @ v.transpose(-1, -2)
    assert dP.sum(-1).abs().max().item() == 0.0                            # delta = sum_j P dP = 0: v's columns sum to zero
    dS = P * dP
    dq, dk = scale * dS @ k, scale * dS.transpose(-1, -2) @ q
    bound = lambda ref, a, n: (lambda cap: cap + 0.5 * ulp_of(ref.abs() + cap, dtype))(scale * (2.0 ** -(p - 1) + 2.0 * n * 2.0 ** -24) * a)
    # the temporal backward (fp32 math, P = e / l an fp32 number with 24 bits) sums Sq multiples of P in fp32: not exactly zero unless
    # Sk is a power of two. Its dv is held to the summation cap alone (the reference is 0) — and to == 0 where Sk is a power of two.
    dv_cap = 2.0 * Sq * 2.0 ** -24 * (P.transpose(-1, -2) @ dout.abs())
    if Sk & (Sk - 1) == 0:
        dv_cap = torch.zeros_like(dv_cap)
    return Case(kind="uniform", fwd=c, dout=tok(dout), dq=tok(dq), dk=tok(dk), dq_bound=tok(bound(dq, dS.abs() @ k.abs(), Sk)),
                dk_bound=tok(bound(dk, dS.abs().transpose(-1, -2) @ q.abs(), Sq)), 
                dv_bound=tok(torch.where(dv_cap > 0, dv_cap + 0.5 * ulp_of(dv_cap, dtype), dv_cap)),
                H=H, D=D)


# ---- the case lists: (B, H, Sq, Sk) -------------------------------------------------------------------------------------------------------

FLASH4 = [(2, 2, 33, 33), (1, 3, 129, 65), (1, 2, 130, 200), (2, 1, 257, 63), (1, 1, 1030, 100)]
FLASH8 = [(2, 1, 1024, 256), (1, 2, 1025, 257), (1, 1, 1300, 300), (1, 1, 1279, 2060)]
# (B, H, Sq, Sk, D): the rowtile kernel; D = 64 up to Sk = 32, the last shape before the flash kernel takes over
ROWTILE = [(2, 4, 64, 64, 16), (1, 3, 100, 37, 32), (1, 2, 40, 1, 64), (1, 2, 40, 25, 64), (2, 1, 17, 32, 64)]
PACKED = [(2, 2, 130, 130), (1, 1, 1025, 1025)]                            # self-attention on (q | k | v): Sq = Sk, one per flash kernel
TEMPORAL_T = (1, 2, 7, 14, 16)
TEMPORAL_S = (5, 33)
TEMPORAL = [(2, T, S, 2, 64) for T in TEMPORAL_T for S in TEMPORAL_S]      # (Bo, T, S, H, D): the MFMA kernel in 16 bit
TEMPORAL_ROWTILE = [(2, 7, 5, 2, 32), (2, 14, 33, 2, 32), (2, 16, 5, 2, 32)]
SETS = {"selector": selector_case, "uniform": uniform_case, "pairs": pairs_case, "comb": comb_case}


def sets_for(Sk):
    """One key admits no zero sum of non-zero numbers and no pair."""
    return ("selector",) if Sk < 2 else ("selector", "uniform", "pairs")


def every_forward_case(tag):
    """(name, builder) of every forward case of the GPU tests in `tag`."""
    out = []
    half = tag != "f32"
    if half:
        for shape in FLASH4 + FLASH8 + PACKED:
            for mode in ("scale", "q_log2") if shape in PACKED else ("scale",):  # (q_log2 exists on the packed entry only)
                for kind in sets_for(shape[3]) + ("comb",):
                    out.append((f"{kind} {shape} {mode}", functools.partial(SETS[kind], tag, *shape, 64, mode)))
    for shape in ROWTILE:
        for kind in sets_for(shape[3]):
            out.append((f"{kind} rowtile {shape}", functools.partial(SETS[kind], tag, *shape)))
    for Bo, T, S, Hh, D in TEMPORAL + TEMPORAL_ROWTILE:                    # (fp32 I/O at D = 64 too: the rowtile kernel)
        for kind in sets_for(T)[:2]:
            out.append((f"{kind} temporal {(Bo, T, S, Hh, D)}", functools.partial(SETS[kind], tag, Bo * S, Hh, T, T, D)))
    return out


def every_backward_case(tag):
    out = []
    for shape in FLASH4 + FLASH8:
        out.append((f"selector bwd {shape}", functools.partial(selector_bwd_case, tag, *shape)))
        out.append((f"uniform bwd {shape}", functools.partial(uniform_bwd_case, tag, *shape)))
    for Bo, T, S, Hh, D in TEMPORAL + TEMPORAL_ROWTILE:
        out.append((f"selector temporal bwd {(Bo, T, S, Hh, D)}", functools.partial(selector_bwd_case, tag, Bo * S, Hh, T, T, D)))
        if T >= 2:
            out.append((f"uniform temporal bwd {(Bo, T, S, Hh, D)}", functools.partial(uniform_bwd_case, tag, Bo * S, Hh, T, T, D)))
    return out


# ---- a plain fp32 emulation of tiled flash attention, written from the kernels' comments, and the faults planted in it ---------------------

FAULTS = ("drop_last_key", "clamped_key_twice", "skip_tile", "swap_pv_keys", "swap_heads", "no_rescale", "truncate_p")


def emulate_forward(q, k, v, H, tag, mode="scale", row_sum="valu", fault=None):
    """softmax(q k^T D^-1/2) v the way the flash kernels compute it, in fp32: key tiles of 64, online maximum (the accumulators are
    rescaled whenever it moves), P rounded to the I/O type before P V, the row sum taken from the unrounded P ("valu", attn_flash.hip:
    the reference exponent is the ROUNDED product max * scale log2 e and enters through an fma) or from the rounded ones ("mfma",
    attn_flash8m16.hip: the maximum is subtracted from the unscaled scores, exactly). Inputs fp64 token-major, output in the type.
    fault: one of FAULTS."""
    dtype = DTYPES[tag]
    qh, kh, vh = (heads(t, H) for t in (q, k, v))
    B, _, Sq, D = qh.shape
    Sk = kh.shape[2]
    if fault == "swap_heads":                                              # keys and values of the neighbouring head (batch entry)
        if H > 1:
            kh, vh = kh.roll(1, 1), vh.roll(1, 1)
        else:
            kh, vh = kh.roll(1, 0), vh.roll(1, 0)
    if fault == "clamped_key_twice":                                       # the clamped copy of key Sk - 1 passes the mask
        kh, vh = torch.cat([kh, kh[:, :, -1:]], 2), torch.cat([vh, vh[:, :, -1:]], 2)
    n_keys = kh.shape[2] - (1 if fault == "drop_last_key" else 0)
    sl2 = torch.tensor(1.0 if mode == "q_log2" else float(D) ** -0.5, dtype=torch.float32) * (
        torch.tensor(1.0 if mode == "q_log2" else LOG2E, dtype=torch.float32))
    if row_sum == "mfma" and tag == "f16" and mode == "scale":             # the fold: scale log2 e rounded into Q
        qh, sl2 = (qh.float() * sl2).to(dtype).double(), torch.tensor(1.0, dtype=torch.float32)
    sl2 = sl2.double()
    m = torch.full((B, H, Sq, 1), -math.inf, dtype=torch.float64)          # log2 units ("valu") / score units ("mfma"); an fp32 number
    l = torch.zeros(B, H, Sq, 1, dtype=torch.float32)
    o = torch.zeros(B, H, Sq, D, dtype=torch.float32)
    tiles = (n_keys + KT - 1) // KT
    for t in range(tiles):
        if fault == "skip_tile" and t == (1 if tiles > 1 else 0):
            continue
        lo, hi = t * KT, min(n_keys, (t + 1) * KT)
        s = qh @ kh[:, :, lo:hi].transpose(-1, -2)                         # exact: integers (multiples of one product) below 2^24
        assert torch.equal(s.float().double(), s)
        smax = s.amax(-1, keepdim=True)
        if row_sum == "valu":
            m_new = torch.maximum(m, (smax * sl2).float().double())
            x = (s * sl2 - m_new).float()                                  # one rounding: the fma
            alpha = torch.exp2((m - m_new).float())
        else:
            m_new = torch.maximum(m, smax)
            x = ((s - m_new).float() * sl2.float()).float()
            alpha = torch.exp2(((m - m_new).float() * sl2.float()).float())
        alpha = torch.where(torch.isinf(m), torch.zeros_like(alpha), alpha)
        if fault == "no_rescale":
            alpha = torch.ones_like(alpha)
        p = torch.exp2(x)
        pr = (truncate_to(p.double(), dtype) if fault == "truncate_p" else rnd(p.double(), dtype)).float()
        pv = pr.clone()
        if fault == "swap_pv_keys" and hi - lo >= 2:                       # two keys of one 32-key block change places in P V only
            pv[..., [0, 1]] = pr[..., [1, 0]]                              # (key 0 is always somebody's choice)
        o = o * alpha + (pv.double() @ vh[:, :, lo:hi]).float()
        l = l * alpha + (p if row_sum == "valu" else pr).sum(-1, keepdim=True)
        m = m_new
    out = (o * (1.0 / l)).to(dtype)
    m_log2 = m if row_sum == "valu" else m * sl2
    lse = ((m_log2 + torch.log2(l.double())) / LOG2E).squeeze(-1)
    return tok(out), lse


def emulate_dv(q, k, dout, lse, H, tag, leak_row=False):
    """dv = P^T dout of the backward in fp32: P = exp2(s log2 e - lse log2 e) recomputed, rounded to the type as an MFMA operand.
    leak_row (the planted fault): the clamped copy of query row Sq - 1 is added to the key-major sums once more."""
    dtype = DTYPES[tag]
    qh, kh, dh = (heads(t, H) for t in (q, k, dout))
    D = qh.shape[-1]
    sl2 = (torch.tensor(float(D) ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).double()
    if folds_scale(qh.shape[2], kh.shape[2], D, tag):                      # the recomputation takes the forward's form (kFold)
        qh, sl2 = folded_q(qh, D, dtype), torch.tensor(1.0, dtype=torch.float64)
    x = ((qh @ kh.transpose(-1, -2)) * sl2 - (lse.float() * torch.tensor(LOG2E, dtype=torch.float32)).double()[..., None]).float()
    pr = rnd(torch.exp2(x).double(), dtype)
    if leak_row:
        pr, dh = torch.cat([pr, pr[:, :, -1:]], 2), torch.cat([dh, dh[:, :, -1:]], 2)
    return tok((pr.transpose(-1, -2) @ dh).float()).to(dtype)


def dv_mismatches(case, got, tag):
    """dv of the selector set under the backward: the exact integer sums bit for bit; where the sum is zero, +-0 in f16 and at most the
    case's `tiny` + `dv_cap` in bf16 and fp32 (see selector_bwd_case). -> the number of elements that miss."""
    g = got.double()
    zero = case.dv == 0
    bad = torch.where(zero, g.abs() > (0.0 if tag == "f16" else case.tiny + case.dv_cap), g != case.dv)
    return int((bad | torch.isnan(g)).sum())


def matches(case, got):
    """The comparison of the GPU tests: selector bit for bit, uniform == 0, pairs bit for bit away from exact ties and one of the two
    neighbours at a tie (strict: bit for bit there too)."""
    if case.kind == "uniform":
        return bool((got.double() == 0).all())
    if case.kind == "selector":
        return torch.equal(got, case.want)
    return pairs_mismatches(case, got, strict=False) == 0


def pairs_mismatches(case, got, strict):
    """(pairs and comb sets) elements that are not the one right number — at an exact tie either neighbour unless `strict`."""
    g = got.double()
    bad = g != case.want.double()
    if not strict:
        dtype = case.want.dtype
        near = (g - case.ref).abs() == 0.5 * ulp_of(case.ref, dtype)
        bad = bad & ~(case.tie & near)
    return int((bad | torch.isnan(g)).sum())

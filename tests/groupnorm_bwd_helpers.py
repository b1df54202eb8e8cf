"""Shared by tools/gen_golden_groupnorm_bwd.py (reference side, build container only) and the GroupNorm-backward tests: the fp64
formula of GroupNorm(+SiLU) with the embedding bias in front and its gradients (written out, no autograd), the seeded inputs, the
error measures and the case lists. The generator pins the formula to the reference's modules (normalization + SiLU as
ResBlock.out_layers[:2] uses them, the dims = 3 form on b c t h w, Normalize); the GPU tests use the formula as their oracle, so nothing
of the reference has to exist where they run."""
import collections
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groupnorm_bwd")
GROUPS = 32
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
OUTPUTS = ("y", "dx", "dweight", "dbias", "demb")

# N rows = videos * T of [C, H, W]; silu / cb (the embedding bias h + emb_out) / eps as the reference module has them; offset: per-channel
# mean of up to 3 standard deviations (cancellation in the variance and in w g - A / m - xh B / m)
Case = collections.namedtuple("Case", "name N C H W T silu cb eps offset")

# fixtures that carry tensors
TENSOR_CASES = [
    Case("odd_s45", 2, 64, 5, 9, 1, True, True, 1e-5, False),             # S odd, C/G * S = 90: the scalar path
    Case("cg3", 2, 96, 8, 8, 1, True, True, 1e-5, False),                 # C/G = 3
    Case("temporal_t2", 4, 64, 6, 8, 2, True, True, 1e-5, False),         # T = 2, N = 4
    Case("normalize", 2, 96, 8, 8, 1, False, False, 1e-6, False),         # Normalize: no SiLU, no bias, eps 1e-6; token-major on the GPU
    Case("offset", 2, 64, 8, 8, 1, True, True, 1e-5, True),
]
# training shapes of the reference's configuration (latent 64 x 48, 14 frames, 32 groups): the reference's own error only
ERROR_CASES = [Case("n2_c%d_%dx%d" % (c, h, w), 2, c, h, w, 1, True, True, 1e-5, True)
               for c, h, w in ((320, 48, 64), (640, 24, 32), (1280, 12, 16), (1280, 6, 8), (2560, 6, 8), (1920, 24, 32), (960, 48, 64))]
ERROR_CASES += [Case("t14_c%d_%dx%d" % (c, h, w), 14, c, h, w, 14, True, True, 1e-5, True) for c, h, w in ((320, 48, 64), (1280, 12, 16))]


def case_name(case, tag):
    return "%s_%s" % (case.name, tag)


def make_inputs(case, dtype):
    """Seeded x [N, C, H, W], emb [N, C] (None without cb), dy [N, C, H, W], weight, bias [C]; every value representable in dtype
    (weight, bias and emb are returned in fp32). Not white noise: per-channel scale in [1, 2], and for offset cases a per-channel mean of
    up to 3 standard deviations."""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)))
    N, C, H, W = case.N, case.C, case.H, case.W
    scale = 1.0 + torch.rand(C, generator=g)
    x = torch.randn(N, C, H, W, generator=g) * scale[None, :, None, None]
    if case.offset:
        x = x + ((torch.rand(C, generator=g) * 6.0 - 3.0) * scale)[None, :, None, None]
    emb = 0.5 * torch.randn(N, C, generator=g) if case.cb else None
    dy = torch.randn(N, C, H, W, generator=g)
    weight = 1.0 + 0.3 * torch.randn(C, generator=g)
    bias = 0.3 * torch.randn(C, generator=g)
    r = lambda t: None if t is None else t.to(dtype)
    f = lambda t: None if t is None else t.to(dtype).float()
    return r(x), f(emb), r(dy), f(weight), f(bias)


def formula(x, emb, dy, weight, bias, T, silu, eps, groups=GROUPS):
    """fp64: dict y, dx, dweight, dbias, demb of y = act(GroupNorm(x + emb)) with statistics per (video of T rows, group), written out as
    the lines of the backward (no autograd). x, dy [N, C, ...]; emb [N, C] or None."""
    N, C = x.shape[:2]
    xd = x.double().reshape(N, C, -1)
    S = xd.shape[2]
    g = dy.double().reshape(N, C, S)
    u = xd if emb is None else xd + emb.double()[:, :, None]
    V, Cg = N // T, C // groups

    def grp(t):                                            # [N, C, S] -> [V, G, T, Cg, S]
        return t.reshape(V, T, groups, Cg, S).transpose(1, 2)

    def back(t):
        return t.transpose(1, 2).reshape(N, C, S)
    ug = grp(u)
    mean = ug.mean(dim=(2, 3, 4), keepdim=True)
    rstd = (ug.var(dim=(2, 3, 4), unbiased=False, keepdim=True) + eps).rsqrt()
    xh = back((ug - mean) * rstd)
    w = weight.double()[None, :, None]
    z = w * xh + bias.double()[None, :, None]
    if silu:
        s = torch.sigmoid(z)
        y = z * s
        g = g * s * (1 + z * (1 - s))
    else:
        y = z
    m = T * Cg * S
    wg = grp(w * g)
    A = wg.sum(dim=(2, 3, 4), keepdim=True)
    B = (wg * grp(xh)).sum(dim=(2, 3, 4), keepdim=True)
    du = back(rstd * (wg - A / m - grp(xh) * B / m))
    return dict(y=y.reshape(x.shape), dx=du.reshape(x.shape), dweight=(g * xh).sum(dim=(0, 2)), dbias=g.sum(dim=(0, 2)),
                demb=None if emb is None else du.sum(dim=2))


def fold_stack3(dy3, T):
    """Gradient of y [N, C, ...] from the gradient of ops._stack3(y, T) [N, 3 C, ...]: block 1 of row t + block 0 of row t + 1 + block 2
    of row t - 1, the missing neighbours at the ends of a video being zero."""
    N, C3 = dy3.shape[:2]
    C = C3 // 3
    d = dy3.reshape(N // T, T, 3, C, *dy3.shape[2:])
    out = d[:, :, 1].clone()
    out[:, :-1] += d[:, 1:, 0]
    out[:, 1:] += d[:, :-1, 2]
    return out.reshape(N, C, *dy3.shape[2:])


def fold_tokens(dy_tok, spatial):
    """Gradient of y [N, C, *spatial] from the gradient of its token-major form [N, S, C]."""
    return dy_tok.transpose(1, 2).reshape(dy_tok.shape[0], dy_tok.shape[2], *spatial)


def errors(got, ref):
    """(max-norm, rms) error of got against ref, relative to ref's own max / rms."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return (d.abs().max() / ref.abs().max()).item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def bits(t):
    return t.contiguous().view(torch.int16).numpy()


def from_bits(a, dtype):
    return torch.from_numpy(a.copy()).view(dtype)


def ref_errors():
    with open(os.path.join(GOLDEN, "ref_errors.json")) as fh:
        return json.load(fh)


def ref_error_for(case, tag, table=None):
    """{<output>_max, <output>_rms}: the reference's own error in that type for this case where it was recorded, else the largest recorded
    entry of the type per field."""
    table = table or ref_errors()
    key = case_name(case, tag)
    if key in table:
        return table[key]
    rows = [v for k, v in table.items() if k.endswith("_" + tag)]
    fields = sorted({f for r in rows for f in r})
    return {f: max(r[f] for r in rows if f in r) for f in fields}

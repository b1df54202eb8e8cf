"""Shared by tools/gen_golden_layernorm_bwd.py (reference side, build container only) and the Add+LayerNorm-backward tests: the fp64
formula of the backward of  s_pre = x + h, s = s_pre + row, y = LayerNorm(s)  written out with no autograd, the unfused expression
itself, the seeded inputs, the error measures and the case lists. The generator pins the formula to the reference's nn.LayerNorm and
`+` (sgm/modules/attention.py:544-572); the GPU tests use the formula as their oracle, so nothing of the reference has to exist
where they run.

The formula's input is s as the forward hands it on: the residual stream ROUNDED to the storage type where the unfused graph rounds it
(x + h, then + row). `stream` computes it; in fp64 nothing is rounded and the formula is the gradient of the unfused expression."""
import collections
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layernorm_bwd")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
OUTPUTS = ("dx", "dweight", "dbias", "drow")
EPS = 1e-5

# R rows of C channels; G runs of the broadcast row (0: no row); h / gs / gsp: whether the residual branch and the gradients of s and
# s_pre exist (gsp means ret_pre); offset: per-channel mean of up to 3 standard deviations (cancellation in t - c2 - xh c1)
Case = collections.namedtuple("Case", "name R C G h gs gsp offset")

# fixtures that carry tensors
TENSOR_CASES = [
    Case("r77_c64_g7", 77, 64, 7, True, True, True, False),          # L = 1, K = 8; a run shorter than a block pass
    Case("r21_c40_g21", 21, 40, 21, True, True, True, False),        # K = 5 at L = 1; one row per run
]
# every other case the GPU module runs: the reference's own error only
BASE_999 = Case("r999_c320_g3", 999, 320, 3, True, True, True, True)
ERROR_CASES = [
    BASE_999,                                                         # L = 8, K = 5; run boundaries inside a block pass
    Case("r96_c1280_g1", 96, 1280, 1, True, True, True, False),       # L = 32
    Case("r50_c4096_norow", 50, 4096, 0, True, True, False, False),   # L = 64, K = 8: the widest row
    Case("r2688_c1280_g14", 2688, 1280, 14, True, True, True, False),     # level 2 of the training latent
    Case("r10752_c640_g14", 10752, 640, 14, True, True, True, False),     # level 1
    Case("r43008_c320_g14", 43008, 320, 14, True, True, True, True),      # level 0: many slabs per run, the long column sums
    Case("r999_c320_plain", 999, 320, 0, False, False, False, True),      # plain LayerNorm: s is x
    Case("r999_c320_h", 999, 320, 0, True, True, False, True),
    Case("r999_c320_row", 999, 320, 3, False, True, True, True),
    Case("r999_c320_nogs", 999, 320, 3, True, False, True, True),
    Case("r999_c320_nogsp", 999, 320, 3, True, True, False, True),
]
GPU_CASES = TENSOR_CASES + ERROR_CASES
FP32_CASES = [Case("r77_c96_g7", 77, 96, 7, True, True, True, False), BASE_999]      # L = 4, K = 6 in fp32


def case_name(case, tag):
    return "%s_%s" % (case.name, tag)


def make_inputs(case, dtype):
    """Seeded dict x, h, row, gy, gs, gsp [R, C] / [G, C] (None where the case has none), w, b [C]; every value representable in dtype.
    Not white noise: per-channel scale in [1, 2], for offset cases a per-channel mean of up to 3 standard deviations, row ~ 0.5 randn,
    w ~ 1 + 0.3 randn."""
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)))
    R, C = case.R, case.C
    scale = 1.0 + torch.rand(C, generator=g)
    x = torch.randn(R, C, generator=g) * scale
    if case.offset:
        x = x + (torch.rand(C, generator=g) * 6.0 - 3.0) * scale
    h = torch.randn(R, C, generator=g) * scale
    row = 0.5 * torch.randn(max(case.G, 1), C, generator=g)
    w = 1.0 + 0.3 * torch.randn(C, generator=g)
    b = 0.3 * torch.randn(C, generator=g)
    gy, gs, gsp = (torch.randn(R, C, generator=g) for _ in range(3))
    r = lambda t, keep: t.to(dtype) if keep else None
    return dict(x=r(x, True), h=r(h, case.h), row=r(row, case.G > 0), w=r(w, True), b=r(b, True), gy=r(gy, True), gs=r(gs, case.gs),
                gsp=r(gsp, case.gsp))


def unfused(x, h, row, w, b, eps=EPS):
    """(y, s, s_pre) of the unfused expression in the dtype of its arguments (differentiable): the PyTorch branch of ops.add_layer_norm."""
    R, C = x.shape
    s_pre = x if h is None else x + h
    s = s_pre
    if row is not None:
        G = row.shape[0]
        s = (s_pre.reshape(G, R // G, C) + row.reshape(G, 1, C)).reshape(R, C)
    return torch.nn.functional.layer_norm(s, (C,), w, b, eps), s, s_pre


def stream(x, h, row):
    """s as the forward hands it on, in x's dtype: rounded after each add."""
    with torch.no_grad():
        return unfused(x, h, row, torch.ones(x.shape[1], dtype=x.dtype), torch.zeros(x.shape[1], dtype=x.dtype))[1]


def formula(s, w, gy=None, gs=None, gsp=None, G=0, eps=EPS):
    """fp64, no autograd: dict dx (= dh), dweight, dbias, drow (None when G == 0) from s [R, C], the norm's weight and the gradients of
    y, s and s_pre (None = absent)."""
    s, w = s.double(), w.double()
    R, C = s.shape
    z = torch.zeros_like(s)
    gy = z if gy is None else gy.double()
    mean = s.mean(dim=1, keepdim=True)
    rstd = ((s - mean).pow(2).mean(dim=1, keepdim=True) + eps).rsqrt()
    xh = (s - mean) * rstd
    t = gy * w
    c1 = (t * xh).mean(dim=1, keepdim=True)
    c2 = t.mean(dim=1, keepdim=True)
    gS = rstd * (t - c2 - xh * c1) + (z if gs is None else gs.double())
    gP = gS + (z if gsp is None else gsp.double())
    return dict(dx=gP, dweight=(gy * xh).sum(dim=0), dbias=gy.sum(dim=0), drow=gS.reshape(G, R // G, C).sum(dim=1) if G else None)


def autograd_unfused(inp, dtype):
    """The unfused expression under autograd in `dtype` on the CPU: dict dx, dh, dweight, dbias, drow (None where there is no such input)."""
    leaf = {k: (None if v is None else v.detach().to(dtype).requires_grad_()) for k, v in inp.items() if k in ("x", "h", "row", "w", "b")}
    y, s, s_pre = unfused(leaf["x"], leaf["h"], leaf["row"], leaf["w"], leaf["b"])
    outs, grads = [y], [inp["gy"].to(dtype)]
    if inp["gs"] is not None:
        outs.append(s); grads.append(inp["gs"].to(dtype))
    if inp["gsp"] is not None:
        outs.append(s_pre); grads.append(inp["gsp"].to(dtype))
    torch.autograd.backward(outs, grads)
    gr = lambda k: None if leaf[k] is None else leaf[k].grad
    return dict(dx=gr("x"), dh=gr("h"), dweight=gr("w"), dbias=gr("b"), drow=gr("row"))


def truth(inp, case):
    """The fp64 formula on the forward's rounded stream of these inputs."""
    return formula(stream(inp["x"], inp["h"], inp["row"]), inp["w"], inp["gy"], inp["gs"], inp["gsp"], case.G)


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


def load_fixture(case, tag):
    """(inputs as make_inputs returns them, fp64 outputs) of a stored tensor fixture."""
    import numpy as np
    dtype = DTYPES[tag]
    with np.load(os.path.join(GOLDEN, case_name(case, tag) + ".npz")) as z:
        inp = {k: (from_bits(z[k], dtype) if k in z.files else None) for k in ("x", "h", "row", "w", "b", "gy", "gs", "gsp")}
        out = {k: (torch.from_numpy(z["out_" + k].copy()) if "out_" + k in z.files else None) for k in OUTPUTS}
    return inp, out

"""GPU parity of the differentiable GroupNorm(+SiLU) (csrc/groupnorm_bwd.hip through svd/ops.py's _GroupNormFn).

Parity chain: the reference's modules under fp64 autograd -> the fp64 formula of tests/groupnorm_bwd_helpers.py
(tests/test_groupnorm_bwd_cpu.py, 1e-12) -> the kernels (here). Bars, 16-bit: the error against fp64 as a multiple of the reference's OWN
error in that type for the same output (fixture, or tests/golden/groupnorm_bwd/ref_errors.json; the largest entry of the type where the
shape was not recorded): rms <= 1.6 x, max norm <= 2.0 x, the project's bars for 16-bit gradient kernels. fp32 I/O: 1e-4 relative max norm
per output. Every test runs with ops.STRICT = True (the module test lifts it, see there)."""
import functools

import pytest
import torch

import groupnorm_bwd_helpers as G
import svd_helpers as H
from test_groupnorm_bwd_cpu import load_fixture

pytestmark = pytest.mark.gpu

SMALL_LATENT_BAR = 1.6          # rms, as tests/test_attention_bwd_gpu.py
SMALL_LATENT_MAX_BAR = 2.0      # max norm
FP32_BAR = 1e-4
DEV = "cuda"
ALL_DTYPES = dict(G.DTYPES, fp32=torch.float32)


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "GROUPNORM_BACKWARD", True)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """ops.group_norm_backward_pays is a speed decision; parity is checked with the decision lifted, so that what is tested is what the
    kernels compute."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "GROUPNORM_BACKWARD_MIN_ELEMENTS", (0, 0, 0))


def _ops():
    from multiview_inpaint_amd.svd import hip_ops, ops
    return ops, hip_ops


def _check(name, n, got, ref, tag, r):
    e_max, e_rms = G.errors(got.detach().cpu(), ref)
    if tag == "fp32":
        H.report(f"{name} {n}: max {e_max:.2e}, rms {e_rms:.2e} (fp32 I/O)")
        return e_max <= FP32_BAR, (name, n, e_max, e_rms)
    r_max, r_rms = r[n + "_max"], r[n + "_rms"]
    H.report(f"{name} {n}: max {e_max:.2e} = {e_max / r_max:.2f} x, rms {e_rms:.2e} = {e_rms / r_rms:.2f} x the reference's own error")
    return e_max <= SMALL_LATENT_MAX_BAR * r_max and e_rms <= SMALL_LATENT_BAR * r_rms, (name, n, e_max, r_max, e_rms, r_rms)


def _assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


def _call(case, xa, ea, wa, ba, layout):
    ops, _ = _ops()
    kw = dict(silu=case.silu, chan_bias=ea)
    if layout == "tokens":
        return ops.group_norm_tokens(xa, G.GROUPS, wa, ba, case.eps, **kw)
    if layout == "stack3" or case.T > 1:
        return ops.group_norm_frames(xa, case.T, G.GROUPS, wa, ba, case.eps, stack3=layout == "stack3", **kw)
    return ops.group_norm(xa, G.GROUPS, wa, ba, case.eps, **kw)


def _run(case, x, emb, dy, weight, bias, layout="planes", emb_grad=True):
    """The case through ops.group_norm / group_norm_frames / group_norm_tokens under autograd, dy in the layout's own shape:
    (y, dict of gradients)."""
    xa = x.to(DEV).requires_grad_()
    wa, ba = weight.to(DEV).requires_grad_(), bias.to(DEV).requires_grad_()
    ea = None if emb is None else emb.to(DEV).requires_grad_(emb_grad)
    y = _call(case, xa, ea, wa, ba, layout)
    y.backward(dy.to(DEV))
    return y.detach(), dict(dx=xa.grad, dweight=wa.grad, dbias=ba.grad, demb=None if ea is None else ea.grad)


def _no_grad_y(case, x, emb, weight, bias, layout):
    with torch.no_grad():
        return _call(case, x.to(DEV), None if emb is None else emb.to(DEV), weight.to(DEV), bias.to(DEV), layout)


def _planes(y, layout, spatial):
    if layout == "tokens":
        return y.transpose(1, 2).reshape(y.shape[0], y.shape[2], *spatial)
    if layout == "stack3":
        C = y.shape[1] // 3
        return y[:, C:2 * C]
    return y


FIXTURES = [(case, tag) for case in G.TENSOR_CASES for tag in G.DTYPES]


@pytest.mark.parametrize("case,tag", FIXTURES, ids=[G.case_name(c, t) for c, t in FIXTURES])
def test_fixture_within_the_reference_own_error(case, tag, route_every_supported_shape):
    """Every fixture through the public op under autograd (the Normalize fixture through ops.group_norm_tokens, the temporal one through
    ops.group_norm_frames): y and every gradient at 1.6 x (rms) / 2.0 x (max) of the reference's own error in the fixture; y of the grad
    route bit-identical to the no-grad route; two runs bit-identical."""
    Z, x, emb, dy, weight, bias = load_fixture(case, tag)
    layout = "tokens" if case.name == "normalize" else "planes"
    r = {n + s: float(Z["ref_err"][i][j]) for i, n in enumerate(G.OUTPUTS) for j, s in enumerate(("_max", "_rms"))}
    d = dy.flatten(2).transpose(1, 2).contiguous() if layout == "tokens" else dy
    y, grads = _run(case, x, emb, d, weight, bias, layout)
    assert torch.equal(y, _no_grad_y(case, x, emb, weight, bias, layout)), "y under autograd must be the inference y, bit for bit"
    _, grads2 = _run(case, x, emb, d, weight, bias, layout)
    assert all(torch.equal(grads[n], grads2[n]) for n in grads if grads[n] is not None), "two backward runs must match bit for bit"
    name = G.case_name(case, tag)
    results = [_check(name, "y", _planes(y, layout, x.shape[2:]).float(), torch.from_numpy(Z["y"]), tag, r)]
    for n in ("dx", "dweight", "dbias", "demb"):
        if n in Z.files:
            results.append(_check(name, n, grads[n].float(), torch.from_numpy(Z[n]), tag, r))
    _assert_all(results)


@functools.lru_cache(maxsize=2)
def _oracle(case, tag):
    x, emb, dy, weight, bias = G.make_inputs(case, ALL_DTYPES[tag])
    return (x, emb, dy, weight, bias), G.formula(x, emb, dy, weight, bias, case.T, case.silu, case.eps)


SHAPES = [(case, tag) for case in G.ERROR_CASES for tag in ALL_DTYPES]


@pytest.mark.parametrize("case,tag", SHAPES, ids=[G.case_name(c, t) for c, t in SHAPES])
def test_training_shapes_against_the_fp64_formula(case, tag, route_every_supported_shape):
    """The training shapes against the fp64 formula evaluated on this machine's CPU, in all three dy layouts (token-major for the plain
    form; stack3, with a gradient of its own, for every shape), with and without chan_bias requiring grad. For every run: y bit-identical
    to the no-grad route and a second backward bit-identical."""
    (x, emb, dy, weight, bias), f = _oracle(case, tag)
    r = None if tag == "fp32" else G.ref_error_for(case, tag)
    name = G.case_name(case, tag)
    results = []
    for layout in ["planes", "stack3"] + (["tokens"] if case.T == 1 else []):
        ref = f
        if layout == "tokens":
            d = dy.flatten(2).transpose(1, 2).contiguous()
        elif layout == "stack3":
            g = torch.Generator().manual_seed(17)
            d = torch.randn(case.N, 3 * case.C, case.H, case.W, generator=g).to(ALL_DTYPES[tag])
            ref = G.formula(x, emb, G.fold_stack3(d.double(), case.T), weight, bias, case.T, case.silu, case.eps)
        else:
            d = dy
        y, grads = _run(case, x, emb, d, weight, bias, layout)
        y0 = _no_grad_y(case, x, emb, weight, bias, layout)
        assert torch.equal(y, y0), f"{layout}: y under autograd must be the inference y, bit for bit"
        _, grads2 = _run(case, x, emb, d, weight, bias, layout)
        assert all(torch.equal(grads[n], grads2[n]) for n in grads), f"{layout}: two backward runs must match bit for bit"
        results.append(_check(f"{name} {layout}", "y", _planes(y, layout, x.shape[2:]).float(), ref["y"], tag, r))
        for n in ("dx", "dweight", "dbias", "demb"):
            results.append(_check(f"{name} {layout}", n, grads[n].float(), ref[n], tag, r))
        # chan_bias not requiring grad: no demb, the other gradients the same bits
        _, g3 = _run(case, x, emb, d, weight, bias, layout, emb_grad=False)
        assert g3["demb"] is None and all(torch.equal(g3[n], grads[n]) for n in ("dx", "dweight", "dbias"))
    _assert_all(results)


def test_routing_and_strict_mode():
    """Under grad PROFILE shows the new kinds and FALLBACKS holds no group_norm* entry; under no_grad, or with nothing requiring grad,
    PROFILE shows exactly the kinds it always showed; only dx requested -> the kind without the parameter launch; GROUPNORM_BACKWARD =
    False raises HipPathError under strict mode as before this feature."""
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    x = torch.randn(28, 320, 48, 64, device=DEV).to(dt)         # 27.5 M elements: above every line of ops.group_norm_backward_pays
    w, b = torch.randn(320, device=DEV), torch.randn(320, device=DEV)
    e = torch.randn(28, 320, device=DEV)
    assert all(ops.group_norm_backward_pays(28, 320, 48 * 64, T, dt, lay) for T, lay in ((1, 0), (14, 1), (1, 2)))
    small = torch.randn(2, 320, 12, 16, device=DEV).to(dt)      # supported, but below the speed line: PyTorch's path, so strict mode raises
    assert hip_ops.group_norm_backward_supported(2, 320, 192, 32, 1, dt, 0) and not ops.group_norm_backward_pays(2, 320, 192, 1, dt, 0)
    with pytest.raises(ops.HipPathError):
        ops.group_norm(small.requires_grad_(), 32, w, b, 1e-5)
    del ops.FALLBACKS[:]
    hip_ops.PROFILE = []
    try:
        xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
        ops.group_norm(xa, 32, wa, b, 1e-5, silu=True, chan_bias=e).sum().backward()
        ops.group_norm_frames(xa, 14, 32, wa, b, 1e-5, silu=True, chan_bias=e, stack3=True).sum().backward()
        ops.group_norm_tokens(xa, 32, wa, b, 1e-6).sum().backward()
        assert [p[0] for p in hip_ops.PROFILE] == ["groupnorm_stats_fwd", "groupnorm_bwd_params"] * 3, hip_ops.PROFILE
        assert xa.grad.shape == x.shape and wa.grad.shape == w.shape
        del hip_ops.PROFILE[:]
        xb = x.clone().requires_grad_()                              # the frozen UNet: dx only
        ops.group_norm(xb, 32, w, b, 1e-5, silu=True, chan_bias=e).sum().backward()
        assert [p[0] for p in hip_ops.PROFILE] == ["groupnorm_stats_fwd", "groupnorm_bwd"], hip_ops.PROFILE
        del hip_ops.PROFILE[:]
        with torch.no_grad():
            ops.group_norm(xa, 32, wa, b, 1e-5, silu=True, chan_bias=e)
            ops.group_norm_frames(xa, 14, 32, wa, b, 1e-5, silu=True, stack3=True)
            ops.group_norm_tokens(xa, 32, wa, b, 1e-6)
        ops.group_norm(x, 32, w, b, 1e-5)                            # grad mode on, nothing requires grad
        assert [p[0] for p in hip_ops.PROFILE] == ["groupnorm", "groupnorm", "groupnorm_tokens", "groupnorm"], hip_ops.PROFILE
    finally:
        hip_ops.PROFILE = None
    assert not [f for f in ops.FALLBACKS if f[0].startswith("group_norm")], ops.FALLBACKS
    ops.GROUPNORM_BACKWARD = False                                   # (restored by the module's fixture)
    for call in (lambda t: ops.group_norm(t, 32, w, b, 1e-5), lambda t: ops.group_norm_frames(t, 14, 32, w, b, 1e-5, stack3=True),
                 lambda t: ops.group_norm_tokens(t, 32, w, b, 1e-6)):
        with pytest.raises(ops.HipPathError):
            call(x.clone().requires_grad_())


def _seed_params(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.copy_((1.0 if n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
            p.copy_(p.to(torch.bfloat16).to(p.dtype))


@pytest.mark.parametrize("kind", ["ResBlock", "VideoResBlock"])
def test_resblock_under_checkpoint_against_the_parent_route(kind, route_every_supported_shape):
    """The package's ResBlock / VideoResBlock (320 -> 320, 14 x 48x64, bf16, T = 14) with parameters requiring grad inside
    checkpoint(use_reentrant=False): input and every parameter gradient against the same module in fp64 on the CPU (whose norms keep the
    package's fp32 statistics: 1e-7, far below what is compared). Yardstick: the route before this feature in the same process
    (GROUPNORM_BACKWARD = False) against the same result; the new route's error may be at most 1.6 x (rms) / 2.0 x (max) of it per
    gradient tensor. ops.STRICT = False for BOTH routes: the blocks' skip adds (ops.bias_residual_add / bias_residual_blend) still record
    "requires grad" and would raise under strict mode — they are pass-through in the backward and not part of this feature. The new
    route's FALLBACKS holds no group_norm* entry, the parent's does. The speed decision is lifted: the plain norms of this shape
    (13.8 M elements) sit below the line of ops.group_norm_backward_pays, and what is tested is what the kernels compute."""
    from torch.utils.checkpoint import checkpoint
    from multiview_inpaint_amd.svd import layers
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    video = kind == "VideoResBlock"

    def make():
        m = getattr(layers, kind)(320, 1280, 0.0, out_channels=320)
        _seed_params(m, 23)
        return m
    g = torch.Generator().manual_seed(29)
    x = torch.randn(14, 320, 48, 64, generator=g).to(dt)
    emb = torch.randn(14, 1280, generator=g).to(dt)
    dy = torch.randn(14, 320, 48, 64, generator=g).to(dt)
    args = (14,) if video else ()
    m64 = make().double()
    x64 = x.double().requires_grad_()
    m64(x64, emb.double(), *args).backward(dy.double())
    ref = {"x": x64.grad, **{n: p.grad for n, p in m64.named_parameters() if p.grad is not None}}

    def gpu_run():
        m = make().to(DEV, dt)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        hip_ops.PROFILE = []
        try:
            checkpoint(m, xg, emb.to(DEV), *args, use_reentrant=False).backward(dy.to(DEV))
            kinds = [p[0] for p in hip_ops.PROFILE]
        finally:
            hip_ops.PROFILE = None
        return {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters() if p.grad is not None}}, kinds, list(ops.FALLBACKS)

    ops.STRICT = False                                               # (restored by the module's fixture)
    new, kinds, fallbacks = gpu_run()
    assert not [f for f in fallbacks if f[0].startswith("group_norm")], fallbacks
    assert kinds.count("groupnorm_bwd_params") == (4 if video else 2) and "groupnorm" not in kinds, kinds
    ops.GROUPNORM_BACKWARD = False
    old, old_kinds, old_fallbacks = gpu_run()
    ops.GROUPNORM_BACKWARD = True
    assert [f for f in old_fallbacks if f[0].startswith("group_norm")] and not [k for k in old_kinds if k.startswith("groupnorm_bwd")]
    # (on the GPU, in both routes alike, layers._emb_chan_bias adds a cached detached fp32 copy of conv1's bias: that one parameter gets
    # no gradient there, before and after this feature; every other gradient of the fp64 module is compared)
    assert set(new) == set(old) and set(new) <= set(ref) and len(ref) - len(new) <= (2 if video else 1), (set(ref) - set(new))
    results = []
    for name, r in ref.items():
        if name not in new:
            continue
        o_max, o_rms = G.errors(old[name].cpu(), r)
        results.append(_check(f"{kind} 320 14x48x64 bf16", "d" + name, new[name], r, "bf16",
                              {"d" + name + "_max": o_max, "d" + name + "_rms": o_rms}))
    _assert_all(results)

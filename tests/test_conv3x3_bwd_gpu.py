"""GPU parity of the 3x3 convolution under autograd: the weight-gradient kernel (csrc/conv3x3_wgrad.hip), the input gradient on the
forward's implicit-GEMM kernel with the transposed weight, ops._ConvTokensFn / ops.conv3x3_tokens and the ResBlock route behind
layers.RESBLOCK_CONV_BWD.

Oracle: the fp64 formulas of tests/conv_bwd_helpers.py (held to fp64 autograd in tests/test_conv3x3_bwd_cpu.py, 1e-12), evaluated on
this machine's CPU on the rounded inputs. Every test runs with ops.STRICT = True unless it says otherwise, and with the speed decision
ops.conv3x3_backward_pays lifted where it routes through ops: what is tested is what the kernels compute."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import conv_bwd_helpers as B
import svd_helpers as H_

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multiview_inpaint_amd", "dropin")
if DROPIN not in sys.path:
    sys.path.insert(0, DROPIN)

DEV = "cuda"
RMS_BAR = 1.6                     # the bars of every *_bwd module test here: the new route's error as a multiple of the parent route's
MAX_BAR = 2.0
FP32_BAR = 1e-4                   # the project's fp32 contract (max norm, relative)
ROUND = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
DGRAD_TOL = {"bf16": 1.0 / 128, "f16": 1.0 / 1024}         # tests/test_unet_ops_gpu.py::test_conv3x3_n320_equals_conv2d

# (N, H, W, C_in, C_out); "split": the smallest shape csrc/conv3x3_wgrad.hip splits, taken from its host function at run time
WGRAD_SHAPES = [(2, 24, 32, 320, 320), (3, 9, 16, 64, 128), (1, 7, 5, 128, 64), (5, 1, 1, 64, 64), (1, 40, 33, 192, 320),
                (2, 3, 96, 640, 320), "split"]
DGRAD_SHAPES = [(2, 24, 32, 320, 320), (1, 9, 16, 640, 64), (3, 5, 7, 320, 192), (1, 1, 1, 320, 64), (2, 12, 16, 960, 640)]


def _id(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import layers, ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "CONV3X3_BACKWARD", True)
    monkeypatch.setattr(layers, "RESBLOCK_CONV_BWD", layers.RESBLOCK_CONV_BWD)           # (tests set it; restored here)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """ops.conv3x3_backward_pays is a speed decision; parity is checked with it lifted (so are the GroupNorm's, whose token-major
    backward the ResBlock route runs on)."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "conv3x3_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "group_norm_backward_pays", lambda *a, **k: True)


def _ops():
    from multiview_inpaint_amd.svd import hip_ops, ops
    return ops, hip_ops


def _profiled(fn):
    _, hip_ops = _ops()
    hip_ops.PROFILE = []
    try:
        out = fn()
        kinds = [p[0] for p in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = None
    return out, kinds


def _smallest_split_shape():
    """The smallest (by N H W C_in C_out) shape with C = 64 for which mvi_conv3x3_wgrad_workspace_bytes > 0."""
    _, hip_ops = _ops()
    cands = sorted(((n, h, w, 64, 64) for n in range(1, 4) for h in range(1, 4) for w in range(1, 4)), key=lambda s: (s[0] * s[1] * s[2], s))
    for s in cands:
        if hip_ops.conv3x3_wgrad_workspace_bytes(*s) > 0:
            return s
    raise AssertionError("no small shape is split")


def _resolve(shape):
    return _smallest_split_shape() if shape == "split" else shape


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape, tag):
    """Inputs and the fp64 reference with its error cap, computed once per (shape, dtype) and left unchanged."""
    N, H, W, Ci, Co = shape
    x, dy, _ = B.make_tokens(shape, B.DTYPES[tag], seed=sum(shape))
    xp, dyp = B.planes(x, H, W), B.planes(dy, H, W)
    ref = B.wgrad_formula(xp, dyp)
    cap = 2.0 * (N * H * W) * 2.0 ** -24 * B.wgrad_formula(xp.abs(), dyp.abs())
    return x, dy, ref, cap


def test_the_shape_list_holds_a_split_and_an_unsplit_shape():
    _, hip_ops = _ops()
    ws = [hip_ops.conv3x3_wgrad_workspace_bytes(*_resolve(s)) for s in WGRAD_SHAPES]
    H_.report(f"conv3x3_wgrad workspace bytes per shape: {dict(zip(map(_id, WGRAD_SHAPES), ws))}; smallest split shape {_smallest_split_shape()}")
    assert any(b > 0 for b in ws) and any(b == 0 for b in ws), ws
    assert ws[-1] > 0
    # a pure function of the shape
    assert ws == [hip_ops.conv3x3_wgrad_workspace_bytes(*_resolve(s)) for s in WGRAD_SHAPES]


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_id)
def test_wgrad_kernel_against_the_fp64_formula(shape, tag):
    """hip_ops.conv3x3_wgrad against the fp64 formula. Elementwise |got - ref| <= 2 n 2^-24 wgrad(|dy|, |x|), n = N H W: the worst case
    of any fp32 summation order of exactly representable products, doubled for the matrix pipe's internal accumulation (where the cap
    is 0 — the eight outer taps of one-pixel images — the result is exactly 0); max norm <= 1e-4 of max|ref|; two calls bit-identical;
    the unsplit launch (workspace withheld) inside the same cap."""
    _, hip_ops = _ops()
    shape = _resolve(shape)
    N, H, W, Ci, Co = shape
    x, dy, ref, cap = _wgrad_case(shape, tag)
    assert hip_ops.conv3x3_wgrad_supported(Ci, Co, B.DTYPES[tag])
    xd, dyd = x.to(DEV), dy.to(DEV)
    got, kinds = _profiled(lambda: hip_ops.conv3x3_wgrad(xd, dyd, H, W))
    assert kinds == ["conv3x3_wgrad"], kinds
    assert got.dtype == torch.float32 and tuple(got.shape) == (Co, Ci, 3, 3)
    again = hip_ops.conv3x3_wgrad(xd, dyd, H, W)
    unsplit = hip_ops.conv3x3_wgrad(xd, dyd, H, W, split=False)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two runs must give the same bits"
    name = f"conv3x3_wgrad {_id(shape)} {tag}"
    for what, g in (("", got), (" unsplit", unsplit)):
        d = (g.double().cpu() - ref).abs()
        live = cap > 0
        r_cap = (d[live] / cap[live]).max().item() if live.any() else 0.0
        r_max = d.max().item() / ref.abs().max().item()
        H_.report(f"{name}{what}: {r_cap:.4f} of the elementwise cap, max norm {r_max:.2e} (bar {FP32_BAR:.0e})")
        assert (d <= cap).all(), (name + what, r_cap)
        assert r_max <= FP32_BAR, (name + what, r_max)
    if N * H * W == N:                                           # one-pixel images: only the centre tap sees a pixel
        outer = got.clone()
        outer[:, :, 1, 1] = 0
        assert not outer.any()


def test_wgrad_gate_edges():
    """C_in = 72, C_out = 96 and fp32 are declined: ..._supported says 0 and the entry returns the invalid-argument status."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    L = _lib.lib()
    bf, f32 = torch.bfloat16, torch.float32
    assert hip_ops.conv3x3_wgrad_supported(64, 64, bf) and hip_ops.conv3x3_wgrad_supported(2560, 1280, torch.float16)
    for Ci, Co, dt in ((72, 64, bf), (64, 96, bf), (64, 64, f32)):
        assert not hip_ops.conv3x3_wgrad_supported(Ci, Co, dt)
        assert L.mvi_conv3x3_wgrad_supported(Ci, Co, hip_ops._DT[dt]) == 0
        x = torch.randn(1, 16, Ci, device=DEV).to(dt)
        dy = torch.randn(1, 16, Co, device=DEV).to(dt)
        dw = torch.zeros(Co, Ci, 3, 3, device=DEV)
        rc = L.mvi_conv3x3_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 1, 4, 4, Ci, Co, hip_ops._DT[dt], None, 0, None)
        assert rc == -1, rc                                      # MVI_EINVAL
        with pytest.raises(Exception, match="conv3x3 wgrad"):
            hip_ops.conv3x3_wgrad(x, dy, 4, 4)
        torch.cuda.synchronize()
        assert not dw.any()


@functools.lru_cache(maxsize=None)
def _dgrad_case(shape, tag):
    N, H, W, Ci, Co = shape
    x, dy, w = B.make_tokens(shape, B.DTYPES[tag], seed=7 + sum(shape))
    return x, dy, w, B.dgrad_formula(B.planes(dy, H, W), w)


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=_id)
def test_dgrad_on_the_forward_kernel_against_fp64(shape, tag):
    """dx = conv3x3_n320(dy, packed transposed weight) against fp64 dx at the forward kernel's own bar
    (max|got - ref| <= tol max(1, max|ref|), tol 1/128 bf16, 1/1024 f16), with and without the K split; PROFILE kind conv3x3_dgrad."""
    _, hip_ops = _ops()
    N, H, W, Ci, Co = shape
    _, dy, w, ref = _dgrad_case(shape, tag)
    assert hip_ops.conv3x3_n320_supported(Co, Ci, B.DTYPES[tag])
    wt = hip_ops.conv3x3_n320_weight(hip_ops.conv3x3_transposed_weight(w.to(DEV)))
    for split in (False, True):
        out, kinds = _profiled(lambda: hip_ops.conv3x3_dgrad(dy.to(DEV), wt, H, W, split=split))
        assert kinds == ["conv3x3_dgrad"], kinds
        assert tuple(out.shape) == (N, H * W, Ci)
        err = (B.planes(out.double().cpu(), H, W) - ref).abs().max().item()
        bar = DGRAD_TOL[tag] * max(1.0, ref.abs().max().item())
        H_.report(f"conv3x3_dgrad {_id(shape)} {tag} split={split}: max error {err:.2e} = {err / bar:.3f} of the bar")
        assert err <= bar, (shape, tag, split, err, bar)


@pytest.mark.parametrize("tag", list(B.DTYPES))
def test_conv3x3_tokens_under_autograd(tag, route_every_supported_shape):
    """ops.conv3x3_tokens under autograd on the dgrad shapes where the gates hold: y bit-identical to the no-grad y; dx the same bits
    whether or not the weight requires grad; only the kinds that are needed run; weight.grad = conv3x3_wgrad(...).to(dtype) bit for bit
    and within one rounding of fp64 (relative max norm 2^-8 bf16 / 2^-11 f16, plus the 1e-4 of the kernel's contract); under
    checkpoint(use_reentrant=False) the forward runs once or twice and each backward kind once."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    shapes = [s for s in DGRAD_SHAPES if ops.conv3x3_tokens_gates(*s, dt)]
    assert (2, 24, 32, 320, 320) in shapes and (2, 12, 16, 960, 640) in shapes, shapes
    for shape in shapes:
        N, H, W, Ci, Co = shape
        x, dy, w, ref_dx = _dgrad_case(shape, tag)
        xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
        with torch.no_grad():
            y0, kinds = _profiled(lambda: ops.conv3x3_tokens(xd, wd, H, W))
        assert kinds == ["conv3x3_n320"], kinds
        _, kinds = _profiled(lambda: ops.conv3x3_tokens(xd, wd, H, W))              # grad mode on, nothing requires grad
        assert kinds == ["conv3x3_n320"], kinds

        xa, wa = xd.clone().requires_grad_(), wd.clone().requires_grad_()
        y, kinds = _profiled(lambda: ops.conv3x3_tokens(xa, wa, H, W))
        assert kinds == ["conv3x3_n320"] and torch.equal(y.detach(), y0)
        _, kinds = _profiled(lambda: y.backward(dyd))
        assert sorted(kinds) == ["conv3x3_dgrad", "conv3x3_wgrad"], kinds

        xo = xd.clone().requires_grad_()
        _, kinds = _profiled(lambda: ops.conv3x3_tokens(xo, wd, H, W).backward(dyd))
        assert kinds == ["conv3x3_n320", "conv3x3_dgrad"], kinds
        assert torch.equal(xo.grad, xa.grad), "dx must not depend on whether the weight requires grad"
        wo = wd.clone().requires_grad_()
        _, kinds = _profiled(lambda: ops.conv3x3_tokens(xd, wo, H, W).backward(dyd))
        assert kinds == ["conv3x3_n320", "conv3x3_wgrad"], kinds
        assert torch.equal(wo.grad, wa.grad)

        direct = hip_ops.conv3x3_wgrad(xd, dyd, H, W)
        assert wa.grad.dtype == dt and torch.equal(wa.grad, direct.to(dt))
        ref_dw = B.wgrad_formula(B.planes(x, H, W), B.planes(dy, H, W))
        e_w = B.errors(wa.grad.cpu(), ref_dw)[0]
        e_x = (B.planes(xa.grad.double().cpu(), H, W) - ref_dx).abs().max().item()
        bar_x = DGRAD_TOL[tag] * max(1.0, ref_dx.abs().max().item())
        H_.report(f"conv3x3_tokens {_id(shape)} {tag}: dweight max norm {e_w:.2e} (bar {ROUND[tag] + FP32_BAR:.2e}), dx {e_x / bar_x:.3f} of its bar")
        assert e_w <= ROUND[tag] + FP32_BAR, (shape, tag, e_w)
        assert e_x <= bar_x, (shape, tag, e_x, bar_x)

        xc, wc = xd.clone().requires_grad_(), wd.clone().requires_grad_()
        _, kinds = _profiled(lambda: checkpoint(ops.conv3x3_tokens, xc, wc, H, W, use_reentrant=False).backward(dyd))
        assert kinds.count("conv3x3_n320") in (1, 2) and kinds.count("conv3x3_dgrad") == 1 and kinds.count("conv3x3_wgrad") == 1, kinds
        assert torch.equal(xc.grad, xa.grad) and torch.equal(wc.grad, wa.grad)


def test_routing_and_strict_mode(route_every_supported_shape):
    """CONV3X3_BACKWARD off: strict mode raises, non-strict mode records ("conv3x3_tokens", "requires grad") and runs no conv3x3_* kind;
    C_in = 72 under grad falls through the same way; under no_grad, or with nothing requiring grad, only conv3x3_n320 runs. The speed
    decision is lifted by the fixture: 2 x 24x32 rows sit between the two measured lines of ops.conv3x3_backward_pays."""
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    N, H, W, Ci, Co = 2, 24, 32, 320, 320
    x, dy, w = (t.to(DEV) for t in B.make_tokens((N, H, W, Ci, Co), dt, seed=3))

    def grad_run(xx, ww):
        xa = xx.clone().requires_grad_()
        y = ops.conv3x3_tokens(xa, ww, H, W)
        y.backward(torch.ones_like(y))
        return xa.grad

    _, kinds = _profiled(lambda: grad_run(x, w))
    assert kinds == ["conv3x3_n320", "conv3x3_dgrad"], kinds
    with torch.no_grad():
        _, kinds = _profiled(lambda: ops.conv3x3_tokens(x.clone().requires_grad_(), w, H, W))
    assert kinds == ["conv3x3_n320"], kinds
    _, kinds = _profiled(lambda: ops.conv3x3_tokens(x, w, H, W))
    assert kinds == ["conv3x3_n320"], kinds

    x72 = torch.randn(N, H * W, 72, device=DEV).to(dt)
    w72 = (torch.randn(Co, 72, 3, 3, device=DEV) / 25).to(dt)
    for off, xx, ww in ((True, x, w), (False, x72, w72)):
        ops.CONV3X3_BACKWARD = not off                           # (restored by the module's fixture)
        ops.STRICT = True
        with pytest.raises(ops.HipPathError):
            grad_run(xx, ww)
        ops.STRICT = False
        del ops.FALLBACKS[:]
        g, kinds = _profiled(lambda: grad_run(xx, ww))
        assert ("conv3x3_tokens", "requires grad") in ops.FALLBACKS and not [k for k in kinds if k.startswith("conv3x3_")], (ops.FALLBACKS, kinds)
        assert g is not None and g.shape == xx.shape
    ops.CONV3X3_BACKWARD, ops.STRICT = True, True
    # the substitute computes the same convolution
    ops.STRICT = False
    ops.CONV3X3_BACKWARD = False
    g_lib = grad_run(x, w)
    ops.CONV3X3_BACKWARD = True
    g_hip = grad_run(x, w)
    ops.STRICT = True
    assert B.errors(g_hip.cpu(), g_lib.double().cpu())[0] <= 4 * ROUND["bf16"]


def test_speed_decision_answers_for_every_training_shape():
    """ops.conv3x3_backward_pays and layers.RESBLOCK_CONV_BWD follow tools/bench_conv_bwd.py; a class the bench has not shown to win
    stays on PyTorch. Whatever the table says, the answer is a bool for every training shape and strict mode raises where it is no."""
    from multiview_inpaint_amd.svd import layers
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    for N in (14, 28):
        for H, W, Ci, Co in ((48, 64, 320, 320), (48, 64, 640, 320), (24, 32, 640, 640), (24, 32, 1280, 640), (12, 16, 1280, 1280),
                             (12, 16, 2560, 1280), (6, 8, 1280, 1280)):
            assert ops.conv3x3_backward_pays(N, H, W, Ci, Co, dt, True) in (True, False)
    assert isinstance(layers.RESBLOCK_CONV_BWD, bool)
    if not ops.conv3x3_backward_pays(2, 24, 32, 320, 320, dt, False):
        x, _, w = (t.to(DEV) for t in B.make_tokens((2, 24, 32, 320, 320), dt, seed=3))
        with pytest.raises(ops.HipPathError):
            ops.conv3x3_tokens(x.requires_grad_(), w, 24, 32)


def _seed_params(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.copy_((1.0 if n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
            p.copy_(p.to(torch.bfloat16).to(p.dtype))


def test_resblock_under_checkpoint_against_the_parent_route(route_every_supported_shape):
    """layers.ResBlock(320, 1280, 0.0, out_channels=320), bf16, 14 x 48x64, under checkpoint(use_reentrant=False), with
    RESBLOCK_CONV_BWD forced on whatever its default: input and parameter gradients against the fp64 CPU module. Yardstick: the parent
    route in the same process (RESBLOCK_CONV_BWD and CONV3X3_BACKWARD off) against the same fp64 result; the new route's error per
    tensor is at most 1.6 x (rms) / 2.0 x (max) of it. ops.STRICT = False for both (the skip adds still record fallbacks). The new
    route's FALLBACKS holds no conv3x3_tokens entry and PROFILE holds 2 x conv3x3_wgrad; frozen with only x requiring grad: no
    conv3x3_wgrad and 2 x conv3x3_dgrad."""
    from torch.utils.checkpoint import checkpoint
    from multiview_inpaint_amd.svd import layers
    ops, hip_ops = _ops()
    dt = torch.bfloat16

    def make():
        m = layers.ResBlock(320, 1280, 0.0, out_channels=320)
        _seed_params(m, 23)
        return m
    g = torch.Generator().manual_seed(29)
    x = torch.randn(14, 320, 48, 64, generator=g).to(dt)
    emb = torch.randn(14, 1280, generator=g).to(dt)
    dy = torch.randn(14, 320, 48, 64, generator=g).to(dt)
    m64 = make().double()
    x64 = x.double().requires_grad_()
    m64(x64, emb.double()).backward(dy.double())
    ref = {"x": x64.grad, **{n: p.grad for n, p in m64.named_parameters() if p.grad is not None}}

    def gpu_run(trainable=True):
        m = make().to(DEV, dt).requires_grad_(trainable)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        _, kinds = _profiled(lambda: checkpoint(m, xg, emb.to(DEV), use_reentrant=False).backward(dy.to(DEV)))
        return {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters() if p.grad is not None}}, kinds, list(ops.FALLBACKS)

    ops.STRICT = False                                               # (restored by the module's fixture)
    layers.RESBLOCK_CONV_BWD = True
    new, kinds, fallbacks = gpu_run()
    assert not [f for f in fallbacks if f[0] == "conv3x3_tokens"], fallbacks
    assert kinds.count("conv3x3_wgrad") == 2 and kinds.count("conv3x3_dgrad") == 2, kinds
    frozen, kinds_f, fallbacks_f = gpu_run(trainable=False)
    assert not [f for f in fallbacks_f if f[0] == "conv3x3_tokens"], fallbacks_f
    assert kinds_f.count("conv3x3_wgrad") == 0 and kinds_f.count("conv3x3_dgrad") == 2, kinds_f
    layers.RESBLOCK_CONV_BWD, ops.CONV3X3_BACKWARD = False, False
    old, old_kinds, _ = gpu_run()
    layers.RESBLOCK_CONV_BWD, ops.CONV3X3_BACKWARD = True, True
    assert not [k for k in old_kinds if k.startswith("conv3x3_")], old_kinds
    assert set(new) == set(old) and set(new) <= set(ref), (set(new) ^ set(old), set(new) - set(ref))
    bad = []
    for name in list(new) + ["frozen x"]:
        got, key = (frozen["x"], "x") if name == "frozen x" else (new[name], name)
        o_max, o_rms = B.errors(old[key].cpu(), ref[key])
        e_max, e_rms = B.errors(got.cpu(), ref[key])
        H_.report(f"ResBlock 320 14x48x64 bf16 d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the parent route's own error")
        if not (e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms):
            bad.append((name, e_max, o_max, e_rms, o_rms))
    assert not bad, bad

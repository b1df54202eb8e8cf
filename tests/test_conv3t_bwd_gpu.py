"""GPU parity of the (3, 1, 1) frame convolution under autograd: the weight-gradient kernel (csrc/conv3t_wgrad.hip), the input gradient
on the forward's three-tap implicit-GEMM kernel with the transposed weight, ops._ConvTokensFn / ops.conv3t_tokens and the temporal
ResBlock route behind layers.TIME_STACK_CONV_BWD.

Oracle: the fp64 formulas of tests/conv3t_bwd_helpers.py (held to fp64 autograd in tests/test_conv3t_bwd_cpu.py, 1e-12), evaluated on
this machine's CPU on the rounded inputs. Every test runs with ops.STRICT = True unless it says otherwise, and with the speed decisions
lifted where it routes through ops — ops.conv3t_backward_pays and the fill-the-chip line ops.CONV3T_MIN_BLOCKS (the test shapes are a
few blocks; the kernels compute them all the same): what is tested is what the kernels compute."""
import functools

import pytest
import torch

import conv3t_bwd_helpers as B
import svd_helpers as H_

pytestmark = pytest.mark.gpu

DEV = "cuda"
RMS_BAR = 1.6                     # the bars of every *_bwd module test here: the new route's error as a multiple of the parent route's
MAX_BAR = 2.0
FP32_BAR = 1e-4                   # the project's fp32 contract (max norm, relative)
ROUND = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
DGRAD_TOL = {"bf16": 1.0 / 128, "f16": 1.0 / 1024}         # tests/test_unet_ops_gpu.py::test_conv3t_n320_equals_conv3d


def _chunk():
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops.CONV3T_WGRAD_CHUNK


# (B, T, S, C_in, C_out); "chunk+1": one pixel past a chunk of csrc/conv3t_wgrad.hip (hip_ops.CONV3T_WGRAD_CHUNK); "split": the
# smallest 64 x 64-channel shape the kernel splits, taken from its host function at run time
WGRAD_SHAPES = [(1, 1, 5, 64, 64), (2, 2, 1, 64, 128), (2, 3, 45, 128, 64), "chunk+1", (1, 14, 161, 64, 64), (2, 14, 333, 320, 320),
                (1, 4, 96, 640, 320), "split"]
DGRAD_SHAPES = [(2, 3, 45, 320, 320), (1, 1, 7, 320, 64), (2, 14, 40, 640, 320), (1, 2, 1, 320, 128)]
OP_SHAPES = [(2, 3, 45, 320, 320), (1, 14, 64, 640, 320)]


def _id(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import layers, ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "CONV3T_BACKWARD", True)
    monkeypatch.setattr(layers, "TIME_STACK_CONV_BWD", layers.TIME_STACK_CONV_BWD)       # (tests set it; restored here)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """ops.conv3t_backward_pays and ops.CONV3T_MIN_BLOCKS are speed decisions; parity is checked with them lifted (so are the
    GroupNorms', whose token-major backward the block route runs on)."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "conv3t_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "CONV3T_MIN_BLOCKS", 0)
    monkeypatch.setattr(dev_ops, "group_norm_backward_pays", lambda *a, **k: True)
    monkeypatch.setattr(dev_ops, "group_norm_tok2tok_backward_pays", lambda *a, **k: True)


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


def _conv3t_kinds(kinds):
    return [k for k in kinds if k.startswith("conv3t_")]


def _smallest_split_shape():
    """The smallest (by B T S) shape with C_in = C_out = 64 for which mvi_conv3t_wgrad_workspace_bytes > 0."""
    _, hip_ops = _ops()
    c = _chunk()
    cands = sorted(((b, t, s, 64, 64) for b in range(1, 4) for t in range(1, 3) for s in (1, c, c + 1, 2 * c, 2 * c + 1)),
                   key=lambda s: (s[0] * s[1] * s[2], s))
    for s in cands:
        if hip_ops.conv3t_wgrad_workspace_bytes(*s) > 0:
            return s
    raise AssertionError("no small shape is split")


def _resolve(shape):
    if shape == "split":
        return _smallest_split_shape()
    if shape == "chunk+1":
        return (1, 14, _chunk() + 1, 64, 64)
    return shape


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape, tag):
    """Inputs and the fp64 reference with its error cap, computed once per (shape, dtype) and left unchanged."""
    Bv, T, S, Ci, Co = shape
    x, dy, _ = B.make_tokens(shape, B.DTYPES[tag], seed=sum(shape))
    ref = B.wgrad_formula(x, dy, T)
    cap = 2.0 * (Bv * T * S) * 2.0 ** -24 * B.wgrad_formula(x.abs(), dy.abs(), T)
    return x, dy, ref, cap


def test_the_shape_list_holds_a_split_and_an_unsplit_shape():
    _, hip_ops = _ops()
    ws = [hip_ops.conv3t_wgrad_workspace_bytes(*_resolve(s)) for s in WGRAD_SHAPES]
    H_.report(f"conv3t_wgrad workspace bytes per shape: {dict(zip(map(_id, WGRAD_SHAPES), ws))}; smallest split shape {_smallest_split_shape()}; "
              f"chunk {_chunk()}")
    assert any(b > 0 for b in ws) and any(b == 0 for b in ws), ws
    assert ws[-1] > 0
    # a pure function of the shape
    assert ws == [hip_ops.conv3t_wgrad_workspace_bytes(*_resolve(s)) for s in WGRAD_SHAPES]
    assert hip_ops.conv3t_wgrad_workspace_bytes(0, 14, 64, 64, 64) == 0


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_id)
def test_wgrad_kernel_against_the_fp64_formula(shape, tag):
    """hip_ops.conv3t_wgrad against the fp64 formula. Elementwise |got - ref| <= 2 n 2^-24 wgrad(|x|, |dy|), n = B T S: the worst case
    of any fp32 summation order of exactly representable products, doubled for the matrix pipe's internal accumulation (where the cap
    is 0 — the outer taps of one-frame videos — the result is exactly 0); max norm <= 1e-4 of max|ref|; two calls bit-identical;
    the unsplit launch (workspace withheld) inside the same cap."""
    _, hip_ops = _ops()
    shape = _resolve(shape)
    Bv, T, S, Ci, Co = shape
    x, dy, ref, cap = _wgrad_case(shape, tag)
    assert hip_ops.conv3t_wgrad_supported(Ci, Co, B.DTYPES[tag])
    xd, dyd = x.to(DEV), dy.to(DEV)
    got, kinds = _profiled(lambda: hip_ops.conv3t_wgrad(xd, dyd, T))
    assert kinds == ["conv3t_wgrad"], kinds
    assert got.dtype == torch.float32 and tuple(got.shape) == (Co, Ci, 3, 1, 1)
    again = hip_ops.conv3t_wgrad(xd, dyd, T)
    unsplit = hip_ops.conv3t_wgrad(xd, dyd, T, split=False)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two runs must give the same bits"
    name = f"conv3t_wgrad {_id(shape)} {tag}"
    for what, g in (("", got), (" unsplit", unsplit)):
        d = (g.double().cpu() - ref).abs()
        live = cap > 0
        r_cap = (d[live] / cap[live]).max().item() if live.any() else 0.0
        r_max = d.max().item() / ref.abs().max().item()
        H_.report(f"{name}{what}: {r_cap:.4f} of the elementwise cap, max norm {r_max:.2e} (bar {FP32_BAR:.0e})")
        assert (d <= cap).all(), (name + what, r_cap)
        assert r_max <= FP32_BAR, (name + what, r_max)
    if T == 1:                                                   # one-frame videos: only the centre tap sees a frame
        assert not got[:, :, 0].any() and not got[:, :, 2].any()


def test_wgrad_empty_batch_and_gate_edges():
    """B = 0 gives zeros. C_in = 72, C_out = 96 and fp32 are declined: ..._supported says 0 and the entry returns the invalid-argument
    status without touching dweight."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    L = _lib.lib()
    bf, f32 = torch.bfloat16, torch.float32
    dw = hip_ops.conv3t_wgrad(torch.empty(0, 5, 64, device=DEV, dtype=bf), torch.empty(0, 5, 128, device=DEV, dtype=bf), 3)
    assert tuple(dw.shape) == (128, 64, 3, 1, 1) and dw.dtype == f32 and not dw.any()
    assert hip_ops.conv3t_wgrad_supported(64, 64, bf) and hip_ops.conv3t_wgrad_supported(1280, 1280, torch.float16)
    for Ci, Co, dt in ((72, 64, bf), (64, 96, bf), (64, 64, f32)):
        assert not hip_ops.conv3t_wgrad_supported(Ci, Co, dt)
        assert L.mvi_conv3t_wgrad_supported(Ci, Co, hip_ops._DT[dt]) == 0
        x = torch.randn(2, 16, Ci, device=DEV).to(dt)
        dy = torch.randn(2, 16, Co, device=DEV).to(dt)
        dw = torch.zeros(Co, Ci, 3, device=DEV)
        rc = L.mvi_conv3t_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 1, 2, 16, Ci, Co, hip_ops._DT[dt], None, 0, None)
        assert rc == -1, rc                                      # MVI_EINVAL
        with pytest.raises(Exception, match="conv3t wgrad"):
            hip_ops.conv3t_wgrad(x, dy, 2)
        torch.cuda.synchronize()
        assert not dw.any()


@functools.lru_cache(maxsize=None)
def _dgrad_case(shape, tag):
    Bv, T, S, Ci, Co = shape
    x, dy, w = B.make_tokens(shape, B.DTYPES[tag], seed=7 + sum(shape))
    return x, dy, w, B.dgrad_formula(dy, w, T)


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=_id)
def test_dgrad_on_the_forward_kernel_against_fp64(shape, tag):
    """dx = conv3t_n320(dy, packed transposed weight) against fp64 dx at the forward kernel's own bar
    (max|got - ref| <= tol max(1, max|ref|), tol 1/128 bf16, 1/1024 f16), with and without the K split; PROFILE kind conv3t_dgrad."""
    _, hip_ops = _ops()
    Bv, T, S, Ci, Co = shape
    _, dy, w, ref = _dgrad_case(shape, tag)
    assert hip_ops.conv3x3_n320_supported(Co, Ci, B.DTYPES[tag])
    wt = hip_ops.conv3t_n320_weight(hip_ops.conv3t_transposed_weight(w.to(DEV)))
    for split in (False, True):
        out, kinds = _profiled(lambda: hip_ops.conv3t_dgrad(dy.to(DEV), wt, T, split=split))
        assert kinds == ["conv3t_dgrad"], kinds
        assert tuple(out.shape) == (Bv * T, S, Ci)
        err = (out.double().cpu() - ref).abs().max().item()
        bar = DGRAD_TOL[tag] * max(1.0, ref.abs().max().item())
        H_.report(f"conv3t_dgrad {_id(shape)} {tag} split={split}: max error {err:.2e} = {err / bar:.3f} of the bar")
        assert err <= bar, (shape, tag, split, err, bar)


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", OP_SHAPES, ids=_id)
def test_conv3t_tokens_under_autograd(shape, tag, route_every_supported_shape):
    """ops.conv3t_tokens under autograd: y bit-identical to the no-grad y; the PROFILE kinds are exactly conv3t_n320, conv3t_dgrad and
    conv3t_wgrad, each only where its gradient is needed; dx the same bits whether or not the weight requires grad and inside the dgrad
    bar; weight.grad = conv3t_wgrad(...).to(dtype) bit for bit and within one rounding of fp64 (relative max norm 2^-8 bf16 / 2^-11 f16,
    plus the 1e-4 of the kernel's contract); under checkpoint(use_reentrant=False) the forward runs once or twice and each backward kind
    once."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    Bv, T, S, Ci, Co = shape
    assert ops.conv3t_tokens_gates(*shape, dt)
    x, dy, w, ref_dx = _dgrad_case(shape, tag)
    xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
    with torch.no_grad():
        y0, kinds = _profiled(lambda: ops.conv3t_tokens(xd, wd, T))
    assert kinds == ["conv3t_n320"], kinds
    _, kinds = _profiled(lambda: ops.conv3t_tokens(xd, wd, T))                 # grad mode on, nothing requires grad
    assert kinds == ["conv3t_n320"], kinds

    xa, wa = xd.clone().requires_grad_(), wd.clone().requires_grad_()
    y, kinds = _profiled(lambda: ops.conv3t_tokens(xa, wa, T))
    assert kinds == ["conv3t_n320"] and torch.equal(y.detach(), y0)
    _, kinds = _profiled(lambda: y.backward(dyd))
    assert sorted(kinds) == ["conv3t_dgrad", "conv3t_wgrad"], kinds

    xo = xd.clone().requires_grad_()
    _, kinds = _profiled(lambda: ops.conv3t_tokens(xo, wd, T).backward(dyd))
    assert kinds == ["conv3t_n320", "conv3t_dgrad"], kinds
    assert torch.equal(xo.grad, xa.grad), "dx must not depend on whether the weight requires grad"
    wo = wd.clone().requires_grad_()
    _, kinds = _profiled(lambda: ops.conv3t_tokens(xd, wo, T).backward(dyd))
    assert kinds == ["conv3t_n320", "conv3t_wgrad"], kinds
    assert torch.equal(wo.grad, wa.grad)

    direct = hip_ops.conv3t_wgrad(xd, dyd, T)
    assert wa.grad.dtype == dt and wa.grad.shape == wd.shape and torch.equal(wa.grad, direct.to(dt))
    e_w = B.errors(wa.grad.cpu(), B.wgrad_formula(x, dy, T))[0]
    e_x = (xa.grad.double().cpu() - ref_dx).abs().max().item()
    bar_x = DGRAD_TOL[tag] * max(1.0, ref_dx.abs().max().item())
    H_.report(f"conv3t_tokens {_id(shape)} {tag}: dweight max norm {e_w:.2e} (bar {ROUND[tag] + FP32_BAR:.2e}), dx {e_x / bar_x:.3f} of its bar")
    assert e_w <= ROUND[tag] + FP32_BAR, (shape, tag, e_w)
    assert e_x <= bar_x, (shape, tag, e_x, bar_x)

    xc, wc = xd.clone().requires_grad_(), wd.clone().requires_grad_()
    _, kinds = _profiled(lambda: checkpoint(ops.conv3t_tokens, xc, wc, T, use_reentrant=False).backward(dyd))
    assert kinds.count("conv3t_n320") in (1, 2) and kinds.count("conv3t_dgrad") == 1 and kinds.count("conv3t_wgrad") == 1, kinds
    assert torch.equal(xc.grad, xa.grad) and torch.equal(wc.grad, wa.grad)


def test_routing_and_strict_mode(route_every_supported_shape):
    """A shape outside the gates (C_out = 192) and the switch off: strict mode raises HipPathError; out of strict mode the call records
    ("conv3t_tokens", "requires grad"), runs no conv3t_* kind and its gradients equal the fp64 ones inside the dtype's rounding
    (F.conv3d in bf16: relative max norm 4 x 2^-8 for dx, whose sums are rounded once, and for dweight)."""
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    Bv, T, S = 2, 3, 45

    def grad_run(xx, ww, dyy):
        xa, wa = xx.clone().requires_grad_(), ww.clone().requires_grad_()
        ops.conv3t_tokens(xa, wa, T).backward(dyy)
        return xa.grad, wa.grad

    for off, (Ci, Co) in ((False, (320, 192)), (True, (320, 320))):
        shape = (Bv, T, S, Ci, Co)
        x, dy, w = B.make_tokens(shape, dt, seed=3)
        xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
        assert ops.conv3t_tokens_gates(*shape, dt) == off
        ops.CONV3T_BACKWARD = not off                            # (restored by the module's fixture)
        ops.STRICT = True
        with pytest.raises(ops.HipPathError):
            grad_run(xd, wd, dyd)
        ops.STRICT = False
        del ops.FALLBACKS[:]
        (gx, gw), kinds = _profiled(lambda: grad_run(xd, wd, dyd))
        ops.STRICT = True
        assert ("conv3t_tokens", "requires grad") in ops.FALLBACKS and not _conv3t_kinds(kinds), (ops.FALLBACKS, kinds)
        e_x = B.errors(gx.cpu(), B.dgrad_formula(dy, w, T))[0]
        e_w = B.errors(gw.cpu(), B.wgrad_formula(x, dy, T))[0]
        H_.report(f"conv3t_tokens fallback {_id(shape)} bf16: dx max norm {e_x:.2e}, dweight {e_w:.2e} (bar {4 * ROUND['bf16']:.2e})")
        assert gx.shape == xd.shape and gw.shape == wd.shape
        assert e_x <= 4 * ROUND["bf16"] and e_w <= 4 * ROUND["bf16"], (e_x, e_w)
    ops.CONV3T_BACKWARD = True


def test_speed_decision_answers_for_every_training_shape():
    """ops.conv3t_backward_pays and layers.TIME_STACK_CONV_BWD follow tools/bench_conv3t_bwd.py; a class the bench has not shown to win
    stays on PyTorch. Whatever the table says, the answer is a bool for every training shape (all of which pass the gates) and strict
    mode raises where it is no."""
    from multiview_inpaint_amd.svd import layers
    ops, hip_ops = _ops()
    for dt in (torch.bfloat16, torch.float16):
        for S, C in ((3072, 320), (768, 640), (192, 1280), (48, 1280)):
            assert ops.conv3t_tokens_gates(1, 14, S, C, C, dt), (S, C)
            for need_dw in (False, True):
                assert ops.conv3t_backward_pays(1, 14, S, C, C, dt, need_dw) in (True, False)
    assert isinstance(layers.TIME_STACK_CONV_BWD, bool)
    if not ops.conv3t_backward_pays(1, 14, 48, 1280, 1280, torch.bfloat16, False):
        x, _, w = (t.to(DEV) for t in B.make_tokens((1, 14, 48, 1280, 1280), torch.bfloat16, seed=3))
        with pytest.raises(ops.HipPathError):
            ops.conv3t_tokens(x.requires_grad_(), w, 14)


def _seed_params(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.copy_((1.0 if n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
            p.copy_(p.to(torch.bfloat16).to(torch.float16).to(p.dtype))          # exact in bf16 and in f16


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("blend", ["fixed", "learned_with_images"])
def test_video_resblock_under_checkpoint_against_the_parent_route(blend, tag, route_every_supported_shape):
    """layers.VideoResBlock(320, 1280, 0.0, video_kernel_size (3, 1, 1), out_channels=320), 2 videos x 3 frames of 8x8, every parameter
    trainable, under checkpoint(use_reentrant=False), with TIME_STACK_CONV_BWD on and off: gradients of x and of every parameter against
    the fp64 CPU module (whose temporal norms ops.group_norm_frames evaluates in fp32: 1e-7, far below either route's error).
    Yardstick: the parent route (switch off) in the same process against the same fp64 result; the new route's error per tensor is at
    most 1.6 x (rms) / 2.0 x (max) of it. ops.STRICT = False for both (the skip adds still record fallbacks). Switch on: no
    conv3t_tokens fallback, 2 x conv3t_wgrad and 2 x conv3t_dgrad; switch off: no conv3t_dgrad / conv3t_wgrad kind.
    blend = "fixed": the blend factor is a buffer, the time stack returns before the blend (VideoResBlock's own default); every gradient
    tensor is held to the bars. blend = "learned_with_images" (the networks' configuration, the blend folded into the skip add): the
    same, except that the gradient of the one-element time_mixer.mix_factor is reported and not held to a RATIO: it is a sum with heavy
    cancellation formed by the tail both routes share, and the ratio of two single rounding errors is Cauchy-distributed — above 2.0
    in 30 % of draws whatever the code (three runs of the same code: identical in bf16 every time; in f16 2.58 x in two and 1.11 x in
    one, at errors of 1.4e-2 against 5.5e-3 and 1.3e-2 — the parent route's own value moves from run to run)."""
    from torch.utils.checkpoint import checkpoint
    from multiview_inpaint_amd.svd import layers
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    T, N = 3, 6

    def make():
        m = layers.VideoResBlock(320, 1280, 0.0, video_kernel_size=[3, 1, 1], out_channels=320, merge_strategy=blend, merge_factor=0.5)
        _seed_params(m, 23)
        return m
    g = torch.Generator().manual_seed(29)
    x = torch.randn(N, 320, 8, 8, generator=g).to(dt)
    emb = torch.randn(N, 1280, generator=g).to(dt)
    dy = torch.randn(N, 320, 8, 8, generator=g).to(dt)
    m64 = make().double()
    x64 = x.double().requires_grad_()
    ind = torch.zeros(N // T, T) if blend == "learned_with_images" else None
    m64(x64, emb.double(), T, ind).backward(dy.double())
    ref = {"x": x64.grad, **{n: p.grad for n, p in m64.named_parameters() if p.grad is not None}}

    def gpu_run():
        m = make().to(DEV, dt)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        _, kinds = _profiled(lambda: checkpoint(m, xg, emb.to(DEV), T, None if ind is None else ind.to(DEV), use_reentrant=False).backward(dy.to(DEV)))
        return {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters() if p.grad is not None}}, kinds, list(ops.FALLBACKS)

    ops.STRICT = False                                               # (restored by the module's fixture)
    layers.TIME_STACK_CONV_BWD = True
    new, kinds, fallbacks = gpu_run()
    assert not [f for f in fallbacks if f[0] == "conv3t_tokens"], fallbacks
    assert kinds.count("conv3t_wgrad") == 2 and kinds.count("conv3t_dgrad") == 2, kinds
    layers.TIME_STACK_CONV_BWD = False
    old, old_kinds, _ = gpu_run()
    assert not [k for k in old_kinds if k in ("conv3t_dgrad", "conv3t_wgrad")], old_kinds
    assert set(new) == set(old) and set(new) <= set(ref), (set(new) ^ set(old), set(new) - set(ref))
    assert {"time_stack.in_layers.2.weight", "time_stack.out_layers.3.weight"} <= set(new)
    bad = []
    for name in new:
        o_max, o_rms = B.errors(old[name].cpu(), ref[name])
        e_max, e_rms = B.errors(new[name].cpu(), ref[name])
        H_.report(f"VideoResBlock 320 2x3x8x8 {blend} {tag} d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the parent route's own error")
        if new[name].numel() > 1 and not (e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms):
            bad.append((name, e_max, o_max, e_rms, o_rms))
    assert not bad, bad
    assert [n for n in new if new[n].numel() == 1] == (["time_mixer.mix_factor"] if blend == "learned_with_images" else [])

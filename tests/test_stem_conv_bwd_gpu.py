"""GPU parity of the hint-stem convolutions under autograd: the dz epilogue of csrc/stem_conv.hip, the weight / bias gradient kernel
(csrc/stem_conv_bwd.hip), the stride-1 input gradient on the forward kernel with the transposed weight, ops._StemConvSiluFn /
ops.stem_conv3x3_silu and the ControlNet route behind unet.HINT_STEM_BWD.

Oracle: the fp64 formulas of tests/stem_bwd_helpers.py (held to fp64 autograd in tests/test_stem_conv_bwd_cpu.py, 1e-12), evaluated on
this machine's CPU on the rounded inputs. Every test runs with ops.STRICT = True unless it says otherwise, and with the speed decision
ops.stem_conv_backward_pays lifted where it routes through ops: what is tested is what the kernels compute."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import stem_bwd_helpers as B
import svd_helpers as H_

pytestmark = pytest.mark.gpu

DEV = "cuda"
RMS_BAR = 1.6                     # the bars of every *_bwd module test here: the new route's error as a multiple of the PyTorch route's
MAX_BAR = 2.0
TOL = {"bf16": 1.0 / 128, "f16": 1.0 / 1024}               # tests/test_unet_ops_gpu.py::test_stem_conv3x3_silu_kernel

# stride 1, (N, C_in, C_out, H, W)
S1 = [(2, 7, 16, 20, 128),        # the 8-channel padded form, ragged row tile
      (1, 16, 16, 37, 72),        # width not a multiple of the 64-pixel tile
      (3, 3, 16, 4, 64),          # fewer rows than a tile
      (1, 9, 16, 1, 8),           # one row, one 8-pixel piece
      (2, 32, 32, 19, 136),       # 32 -> 32
      (1, 20, 32, 8, 64),         # channels padded to 32
      (3, 16, 16, 64, 192)]       # 72 blocks: the partials reduce (several tiles per block: WALK below)
# stride 2 into 32 channels, (N, C_in, H, W)
S2 = [(2, 16, 20, 128), (1, 5, 37, 80), (1, 16, 7, 16)]
CASES = [(s, 1) for s in S1] + [((n, c, 32, h, w), 2) for n, c, h, w in S2]
SQUARE = [s for s in S1 if s[1] == s[2]]
# more tiles than the grid's bound in each form (1024 / 512 / 768 blocks): a block walks two tiles with its accumulators in registers
WALK = [((2, 16, 16, 520, 512), 1), ((3, 32, 32, 176, 256), 1), ((4, 8, 32, 400, 512), 2)]


def _id(c):
    return "x".join(map(str, c[0])) + f"s{c[1]}" if isinstance(c[0], tuple) else "x".join(map(str, c))


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import ops as dev_ops, unet
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "STEM_CONV_BACKWARD", True)
    monkeypatch.setattr(unet, "HINT_STEM_BWD", unet.HINT_STEM_BWD)               # (tests set it; restored here)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """ops.stem_conv_backward_pays is a speed decision; parity is checked with it lifted."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "stem_conv_backward_pays", lambda *a, **k: True)


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


NEW_KINDS = ("stem_conv_dz", "stem_conv_wgrad", "stem_conv_dgrad")


@functools.lru_cache(maxsize=None)
def _case(shape, stride, tag, bias=True):
    """Inputs computed once per (shape, stride, dtype) and left unchanged."""
    return B.make_case(shape, stride, B.DTYPES[tag], seed=31 + sum(shape) + stride, bias=bias)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dz_pass_against_the_fp64_formula(case, tag):
    """dz = dy silu'(z) with z recomputed by the forward kernel, with and without bias: relative max norm below the forward kernel's
    own bar; the y of the same launch has the forward's bits."""
    _, hip_ops = _ops()
    shape, stride = case
    for bias in (True, False):
        x, w, b, dy = _case(shape, stride, tag, bias)
        assert hip_ops.stem_conv3x3_bwd_supported(shape[1], shape[2], shape[4], stride, B.DTYPES[tag])
        ref = B.dz_formula(x, w, b, dy, stride, True)
        xd, wd, bd, dyd = _dev(x, w, b, dy)
        (dz, y), kinds = _profiled(lambda: hip_ops.stem_conv3x3_dz(xd, wd, bd, dyd, silu=True, stride=stride, with_y=True))
        assert kinds == ["stem_conv_dz"], kinds
        only = hip_ops.stem_conv3x3_dz(xd, wd, bd, dyd, silu=True, stride=stride)
        y0 = hip_ops.stem_conv3x3_silu(xd, wd, bd, silu=True, stride=stride)
        torch.cuda.synchronize()
        assert dz.dtype == dy.dtype and dz.shape == dy.shape
        e = B.errors(dz.cpu(), ref)[0]
        H_.report(f"stem_conv_dz {_id(case)} {tag} bias={bias}: max norm {e:.2e} (bar {TOL[tag]:.2e})")
        assert e < TOL[tag], (case, tag, bias, e)
        assert torch.equal(y, y0), "the forward output of the dz launch must have the forward's bits"
        assert torch.equal(only, dz)


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("case", CASES + WALK, ids=_id)
def test_wgrad_kernel_against_the_fp64_formula(case, tag):
    """hip_ops.stem_conv3x3_wgrad given rounded x and a rounded dz. Elementwise |got - ref| <= 2 K 2^-24 wgrad(|x|, |dz|), K = N H_o W_o:
    the worst case of any fp32 summation order of exactly representable products, doubled for the matrix pipe's internal accumulation;
    the same for dbias with sum |dz|. Two calls bit-identical; the workspace size is a pure function of the shape and a workspace one
    byte short is refused with the invalid-argument status."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    shape, stride = case
    N, Ci, Co, H, W = shape
    x, _, _, dz = _case(shape, stride, tag)
    K = dz.numel() // Co
    ref_w, ref_b = B.wgrad_formula(x, dz, stride), B.dbias_formula(dz)
    cap_w = 2.0 * K * 2.0 ** -24 * B.wgrad_formula(x.abs(), dz.abs(), stride)
    cap_b = 2.0 * K * 2.0 ** -24 * B.dbias_formula(dz.abs())
    xd, dzd = _dev(x, dz)
    (dw, db), kinds = _profiled(lambda: hip_ops.stem_conv3x3_wgrad(xd, dzd, stride=stride))
    assert kinds == ["stem_conv_wgrad"], kinds
    dw2, db2 = hip_ops.stem_conv3x3_wgrad(xd, dzd, stride=stride)
    dw3, none = hip_ops.stem_conv3x3_wgrad(xd, dzd, stride=stride, need_dbias=False)
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (Co, Ci, 3, 3) and tuple(db.shape) == (Co,) and none is None
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dw, dw3), "two runs must give the same bits"
    for what, got, ref, cap in (("dweight", dw, ref_w, cap_w), ("dbias", db, ref_b, cap_b)):
        d = (got.double().cpu() - ref).abs()
        live = cap > 0
        r_cap = (d[live] / cap[live]).max().item() if live.any() else 0.0
        H_.report(f"stem_conv_wgrad {_id(case)} {tag} {what}: {r_cap:.4f} of the elementwise cap, max norm {d.max().item() / ref.abs().max().item():.2e}")
        assert (d <= cap).all(), (case, tag, what, r_cap)

    ws = hip_ops.stem_conv3x3_wgrad_workspace_bytes(N, Ci, Co, H, W, stride)
    assert ws > 0 and ws == hip_ops.stem_conv3x3_wgrad_workspace_bytes(N, Ci, Co, H, W, stride)
    L = _lib.lib()
    buf = torch.empty(ws, dtype=torch.uint8, device=DEV)
    out = torch.zeros(Co, Ci, 3, 3, device=DEV)
    rc = L.mvi_stem_conv3x3_wgrad(xd.data_ptr(), dzd.data_ptr(), out.data_ptr(), None, N, Ci, Co, H, W, stride, hip_ops._DT[B.DTYPES[tag]],
                                  buf.data_ptr(), ws - 1, None)
    torch.cuda.synchronize()
    assert rc == -1 and not out.any(), rc                            # MVI_EINVAL, nothing launched


def test_the_partials_are_bounded_by_the_grid_not_the_image():
    """The workspace of the workload's largest layer (14 x 16 x 576 x 1024) is a few MB: a bounded grid of blocks, one partial each."""
    _, hip_ops = _ops()
    small = hip_ops.stem_conv3x3_wgrad_workspace_bytes(3, 16, 16, 64, 192, 1)
    full = hip_ops.stem_conv3x3_wgrad_workspace_bytes(14, 16, 16, 576, 1024, 1)
    twice = hip_ops.stem_conv3x3_wgrad_workspace_bytes(28, 16, 16, 576, 1024, 1)
    H_.report(f"stem_conv_wgrad workspace bytes: 3x64x192 {small}, 14x576x1024 {full}, 28x576x1024 {twice}")
    assert 0 < small < full <= 16 << 20 and twice <= 16 << 20
    per_block = 10 * 256 * 4                                         # the 16 -> 16 form: 9 tap tiles + the bias tile of 16 x 16 fp32
    assert small == 3 * 8 * 3 * per_block                            # one tile per block, 72 blocks: the partials reduce
    assert hip_ops.stem_conv3x3_wgrad_workspace_bytes(2, 16, 16, 520, 512, 1) == 520 * per_block          # 1040 tiles, two per block
    assert hip_ops.stem_conv3x3_wgrad_workspace_bytes(3, 32, 32, 176, 256, 1) == 264 * 2 * 19 * 256 * 4   # 528 tiles, two per block
    assert hip_ops.stem_conv3x3_wgrad_workspace_bytes(4, 8, 32, 400, 512, 2) == 400 * 2 * 10 * 256 * 4    # 800 tiles, two per block


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", SQUARE, ids=_id)
def test_stride1_input_gradient_against_fp64(shape, tag):
    """dx = the forward kernel on dz with the packed transposed weight, 16 -> 16 and 32 -> 32, against dgrad_formula."""
    _, hip_ops = _ops()
    _, w, _, dz = _case(shape, 1, tag)
    ref = B.dgrad_formula(dz, w)
    dzd, wd = _dev(dz, w)
    for train in (False, True):
        dx, kinds = _profiled(lambda: hip_ops.stem_conv3x3_dgrad(dzd, wd.clone().requires_grad_(train)))
        assert kinds == ["stem_conv_dgrad"], kinds
        e = B.errors(dx.cpu(), ref)[0]
        H_.report(f"stem_conv_dgrad {_id(shape)} {tag} live weight={train}: max norm {e:.2e} (bar {TOL[tag]:.2e})")
        assert dx.shape == dz.shape and e < TOL[tag], (shape, tag, e)


# (shape, stride, x requires grad): the three classes; a stride-1 layer with C_in != C_out is routed only where its input needs no gradient
AUTOGRAD_CASES = [((2, 7, 16, 20, 128), 1, False), ((1, 16, 16, 37, 72), 1, True), ((2, 32, 32, 19, 136), 1, True), ((1, 20, 32, 8, 64), 1, False),
                  ((1, 5, 32, 37, 80), 2, True), ((2, 16, 32, 20, 128), 2, False)]


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape,stride,need_dx", AUTOGRAD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_stem_conv3x3_silu_under_autograd(shape, stride, need_dx, tag, route_every_supported_shape):
    """ops.stem_conv3x3_silu under autograd against fp64 autograd on the rounded inputs: per gradient the new route's max-norm error is at
    most 2.0 x and its rms error at most 1.6 x the error of F.silu(F.conv2d(...)) under autograd in the same dtype on the same GPU and
    inputs. The profile holds exactly the expected kinds; with the switch off none of the new kinds."""
    ops, hip_ops = _ops()
    x, w, b, dy = _case(shape, stride, tag)
    ref = dict(zip(("x", "weight", "bias"), B.autograd_grads(x, w, b, dy, stride, True)))

    def run(fn):
        xa, wa, ba = (t.clone().requires_grad_(r) for t, r in zip(_dev(x, w, b), (need_dx, True, True)))
        (y, _), kinds = _profiled(lambda: (lambda y: (y, y.backward(_dev(dy)[0])))(fn(xa, wa, ba)))
        return y.detach(), {"x": xa.grad, "weight": wa.grad, "bias": ba.grad}, kinds

    y_new, new, kinds = run(lambda xa, wa, ba: ops.stem_conv3x3_silu(xa, wa, ba, silu=True, stride=stride))
    want = ["stem_conv", "stem_conv_dz", "stem_conv_wgrad"] + (["stem_conv_dgrad"] if need_dx and stride == 1 else [])
    assert kinds == want, kinds
    y_old, old, _ = run(lambda xa, wa, ba: F.silu(F.conv2d(xa, wa, ba, stride, 1)))
    with torch.no_grad():
        assert torch.equal(y_new, ops.stem_conv3x3_silu(*_dev(x, w, b), silu=True, stride=stride))
    assert new["weight"].dtype == w.dtype and new["bias"].dtype == b.dtype
    assert (new["x"] is None) == (not need_dx)
    bad = []
    for name in ("x", "weight", "bias") if need_dx else ("weight", "bias"):
        e_max, e_rms = B.errors(new[name].cpu(), ref[name])
        o_max, o_rms = B.errors(old[name].cpu(), ref[name])
        H_.report(f"stem_conv3x3_silu {'x'.join(map(str, shape))} s{stride} {tag} d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, "
                  f"rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the PyTorch route's own error ({o_max:.2e}, {o_rms:.2e})")
        if not (e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms):
            bad.append((name, e_max, o_max, e_rms, o_rms))
    assert not bad, bad

    # without SiLU: dy is dz, no dz pass
    xa, wa = (t.clone().requires_grad_(r) for t, r in zip(_dev(x, w), (need_dx, True)))
    _, kinds = _profiled(lambda: ops.stem_conv3x3_silu(xa, wa, None, silu=False, stride=stride).backward(_dev(dy)[0]))
    assert kinds == [k for k in want if k != "stem_conv_dz"], kinds
    e = B.errors(wa.grad.cpu(), B.wgrad_formula(x, dy, stride))[0]
    assert e <= 2 * TOL[tag], e

    # the switch off: strict mode raises; otherwise a recorded fallback and none of the new kinds
    ops.STEM_CONV_BACKWARD = False                                   # (restored by the module's fixture)
    with pytest.raises(ops.HipPathError):
        run(lambda xa, wa, ba: ops.stem_conv3x3_silu(xa, wa, ba, silu=True, stride=stride))
    ops.STRICT = False
    del ops.FALLBACKS[:]
    _, off, kinds = run(lambda xa, wa, ba: ops.stem_conv3x3_silu(xa, wa, ba, silu=True, stride=stride))
    assert ("stem_conv3x3_silu", "requires grad") in ops.FALLBACKS and not [k for k in kinds if k in NEW_KINDS + ("stem_conv",)], (ops.FALLBACKS, kinds)
    assert off["weight"].shape == w.shape and bool(torch.isfinite(off["weight"]).all())


def test_unrouted_shapes_and_the_default_decision():
    """A stride-1 layer with C_in != C_out whose input needs a gradient is not routed (strict mode raises); the speed decision as
    committed routes the measured classes from their smallest measured size up and nothing else, and strict mode raises where it is no."""
    ops, _ = _ops()
    x, w, b, _ = _dev(*_case((2, 7, 16, 20, 128), 1, "bf16"))
    assert not ops.stem_conv_gates(2, 7, 16, 20, 128, 1, torch.bfloat16, True)
    assert ops.stem_conv_gates(2, 7, 16, 20, 128, 1, torch.bfloat16, False)
    # the committed decision (profiles/stem_bwd_bench.json: every class won): the workload's four layers and their half-size forms
    # are routed in both types, a size below a class's smallest measured one is not
    for dt in (torch.bfloat16, torch.float16):
        for scale in (1, 2):
            for Ci, Co, H, W, s in ((7, 16, 576, 1024, 1), (16, 16, 576, 1024, 1), (16, 32, 576, 1024, 2), (32, 32, 288, 512, 1)):
                assert ops.stem_conv_backward_pays(14, Ci, Co, H // scale, W // scale, s, dt, Ci != 7) is True
        for Ci, Co, H, W, s in ((7, 16, 288, 504, 1), (16, 16, 144, 256, 1), (16, 32, 288, 496, 2), (32, 32, 144, 248, 1)):
            assert ops.stem_conv_backward_pays(14, Ci, Co, H, W, s, dt, Ci != 7) is False
        assert ops.stem_conv_backward_pays(14, 16, 48, 576, 1024, 1, dt, False) is False          # no such class
    if not ops.stem_conv_backward_pays(2, 7, 16, 20, 128, 1, torch.bfloat16, False):
        with pytest.raises(ops.HipPathError):
            ops.stem_conv3x3_silu(x, w.requires_grad_(), b, silu=True, stride=1)


def test_the_hint_stem_route(route_every_supported_shape):
    """ControlNet._hint_stem of the small configuration under autograd on a (2, 7, 36, 80) hint (ragged against both tile heights and the
    tile width at every level, 36 -> 18 -> 9 -> 5 rows), the last convolution unzeroed. With unet.HINT_STEM_BWD on the four leading
    layers run on the HIP kernels (4 stem_conv, 4 stem_conv_dz, 4 stem_conv_wgrad; stem_conv_dgrad for the two stride-1 C -> C layers,
    16 -> 16 and 32 -> 32, the stride-2 layer's input gradient being the library's) and the 16 parameter gradients meet the 2.0 x / 1.6 x
    bars against the fp64 CPU stem, relative to the default route's errors. By default the same call launches none of the new kinds."""
    from multiview_inpaint_amd.svd import unet
    from multiview_inpaint_amd.svd.unet import ControlNet
    ops, hip_ops = _ops()
    assert unet.HINT_STEM_BWD is False                               # the committed default: nothing that runs today changes
    dt = torch.bfloat16
    torch.manual_seed(7)
    cnet = ControlNet(**H_.SMALL_CTRL)
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():
        for p in cnet.input_hint_block.parameters():
            if p.ndim == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (p[0].numel()) ** -0.5)
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            p.copy_(p.to(dt).to(p.dtype))
    hint = torch.randn(2, 7, 36, 80, generator=g).to(dt)
    stem64 = copy.deepcopy(cnet.input_hint_block).double()
    out64 = hint.double()
    for m in stem64:
        out64 = m(out64)
    dy = torch.randn(out64.shape, generator=g).to(dt)
    out64.backward(dy.double())
    ref = {n: p.grad for n, p in stem64.named_parameters()}
    assert len(ref) == 16 and tuple(out64.shape[2:]) == (5, 10)

    cnet = cnet.to(DEV, dt)

    def gpu_run():
        cnet.zero_grad(set_to_none=True)
        _, kinds = _profiled(lambda: cnet._hint_stem(hint.to(DEV), None, None).backward(dy.to(DEV)))
        return {n: p.grad.clone() for n, p in cnet.input_hint_block.named_parameters()}, kinds

    ops.STRICT = False                                               # (restored by the module's fixture)
    old, kinds = gpu_run()
    assert not [k for k in kinds if k in NEW_KINDS + ("stem_conv",)], kinds
    unet.HINT_STEM_BWD = True
    ops.STRICT = True
    new, kinds = gpu_run()
    count = {k: kinds.count(k) for k in NEW_KINDS + ("stem_conv",)}
    assert count == {"stem_conv": 4, "stem_conv_dz": 4, "stem_conv_wgrad": 4, "stem_conv_dgrad": 2}, kinds
    bad = []
    for name in ref:
        e_max, e_rms = B.errors(new[name].cpu(), ref[name])
        o_max, o_rms = B.errors(old[name].cpu(), ref[name])
        H_.report(f"hint stem 2x7x36x80 bf16 d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the default route's own error")
        if not (e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms):
            bad.append((name, e_max, o_max, e_rms, o_rms))
    assert not bad, bad

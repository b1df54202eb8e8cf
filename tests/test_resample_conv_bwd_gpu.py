"""GPU parity of the two resampling 3x3 convolutions under autograd: the stride-2 weight gradient (csrc/conv3x3_wgrad.hip, stride-2 form),
the stride-2 input gradient on the forward kernel's zero-stuffed-source form (csrc/linear_n320.hip), the 2x2 pooling pass of the upsampling
form's input gradient (csrc/token_rows.hip), ops.conv3x3_down_tokens / ops.conv3x3_up_tokens and the Downsample / Upsample route behind
layers.RESAMPLE_CONV_BWD.

Oracle: the fp64 formulas of tests/resample_bwd_helpers.py (held to fp64 autograd in tests/test_resample_conv_bwd_cpu.py, 1e-12),
evaluated on this machine's CPU on the rounded inputs. Every test runs with ops.STRICT = True unless it says otherwise; where a test routes
through ops, the fill-the-chip line and the speed decisions are lifted: what is tested is what the kernels compute."""
import functools

import pytest
import torch
import torch.nn.functional as F

import resample_bwd_helpers as R
import svd_helpers as H_

pytestmark = pytest.mark.gpu

DEV = "cuda"
RMS_BAR = 1.6                     # the bars of every *_bwd module test here: the new route's error as a multiple of the parent route's
MAX_BAR = 2.0
ROUND = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
DGRAD_TOL = {"bf16": 1.0 / 128, "f16": 1.0 / 1024}         # the forward kernel's own bar (tests/test_conv3x3_bwd_gpu.py)
MAX_W = 256                                                 # csrc/conv3x3_wgrad.hip's LDS limit (hip_ops.CONV3X3_WGRAD_MAX_W)

# (N, H, W, C_in, C_out) of the module; H x W is the stride-2 convolution's input
S2_WGRAD_SHAPES = [(1, 2, 2, 64, 64), (5, 2, 2, 64, 64), (2, 6, 10, 128, 64), (1, 2, MAX_W, 64, 64), (3, 18, 32, 320, 320), (1, 40, 34, 192, 320)]
S2_DGRAD_SHAPES = [(1, 2, 2, 320, 64), (2, 6, 10, 320, 128), (3, 10, 14, 320, 192), (1, 18, 32, 640, 640), (2, 4, 6, 960, 320)]
POOL_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 320), (3, 9, 16, 1280)]                         # (N, h, w, C)
# (N, h, w, C_in, C_out) of the module, h x w the source: dy has C_out channels, dx C_in
UP_DGRAD_SHAPES = [(1, 1, 1, 320, 64), (2, 3, 5, 320, 128), (3, 5, 7, 320, 192), (1, 9, 16, 1280, 1280)]
DOWN_OP_SHAPES = [(3, 10, 14, 320, 320), (1, 18, 32, 640, 320)]
UP_OP_SHAPES = [(2, 3, 5, 320, 320), (1, 9, 16, 1280, 640)]
TRAINING_SHAPES = [(72, 128, 320), (36, 64, 640), (18, 32, 1280)]                      # Downsample inputs / Upsample outputs, C -> C, N = 14


def _id(s):
    return "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import layers, ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "RESAMPLE_CONV_BACKWARD", True)
    monkeypatch.setattr(layers, "RESAMPLE_CONV_BWD", layers.RESAMPLE_CONV_BWD)          # (tests set it; restored here)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """The fill-the-chip line and the two *_backward_pays are speed decisions; parity is checked with them lifted."""
    from multiview_inpaint_amd.svd import layers, ops as dev_ops
    monkeypatch.setattr(layers, "resample_conv_module_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "RESAMPLE_CONV_MIN_BLOCKS", 1)
    monkeypatch.setattr(dev_ops, "conv3x3_down_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "conv3x3_up_backward_pays", lambda *a: True)


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


# ---- the stride-2 weight gradient -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _s2_case(shape, tag):
    """Inputs and the fp64 references with the wgrad's error cap, computed once per (shape, dtype) and left unchanged."""
    N, H, W, Ci, Co = shape
    x, dy, w, b = R.make_s2(shape, R.DTYPES[tag], seed=sum(shape))
    xp, dyp = R.planes(x, H, W), R.planes(dy, H // 2, W // 2)
    n = N * (H // 2) * (W // 2)
    return {"x": x, "dy": dy, "w": w, "b": b, "dw": R.s2_wgrad_formula(xp, dyp),
            "cap": 2.0 * n * 2.0 ** -24 * R.s2_wgrad_formula(xp.abs(), dyp.abs())}


def test_the_wgrad_shape_list_holds_a_split_and_an_unsplit_shape():
    _, hip_ops = _ops()
    assert MAX_W == hip_ops.CONV3X3_WGRAD_MAX_W
    ws = [hip_ops.conv3x3_s2_wgrad_workspace_bytes(*s) for s in S2_WGRAD_SHAPES]
    H_.report(f"conv3x3_s2_wgrad workspace bytes per shape: {dict(zip(map(_id, S2_WGRAD_SHAPES), ws))}")
    assert any(b > 0 for b in ws) and any(b == 0 for b in ws), ws
    assert ws == [hip_ops.conv3x3_s2_wgrad_workspace_bytes(*s) for s in S2_WGRAD_SHAPES]      # a pure function of the shape


@pytest.mark.parametrize("tag", list(R.DTYPES))
@pytest.mark.parametrize("shape", S2_WGRAD_SHAPES, ids=_id)
def test_s2_wgrad_kernel_against_the_fp64_formula(shape, tag):
    """hip_ops.conv3x3_s2_wgrad against the fp64 formula, with the workspace and with it withheld. Elementwise
    |got - ref| <= 2 n 2^-24 s2_wgrad(|x|, |dy|), n = N (H / 2)(W / 2): the worst case of any fp32 summation order of exactly representable
    products, doubled for the matrix pipe's internal accumulation (the stride-1 test's cap; where it is 0 the result is exactly 0). Two
    calls bit-identical. One output pixel: the taps ky = 0 and kx = 0 see the padding only."""
    _, hip_ops = _ops()
    N, H, W, Ci, Co = shape
    c = _s2_case(shape, tag)
    assert hip_ops.conv3x3_s2_wgrad_supported(Ci, Co, R.DTYPES[tag])
    xd, dyd = c["x"].to(DEV), c["dy"].to(DEV)
    got, kinds = _profiled(lambda: hip_ops.conv3x3_s2_wgrad(xd, dyd, H, W))
    assert kinds == ["conv3x3_s2_wgrad"], kinds
    assert got.dtype == torch.float32 and tuple(got.shape) == (Co, Ci, 3, 3)
    again = hip_ops.conv3x3_s2_wgrad(xd, dyd, H, W)
    unsplit = hip_ops.conv3x3_s2_wgrad(xd, dyd, H, W, split=False)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two runs must give the same bits"
    ref, cap = c["dw"], c["cap"]
    for what, g in (("", got), (" unsplit", unsplit)):
        d = (g.double().cpu() - ref).abs()
        live = cap > 0
        r_cap = (d[live] / cap[live]).max().item() if live.any() else 0.0
        H_.report(f"conv3x3_s2_wgrad {_id(shape)} {tag}{what}: {r_cap:.4f} of the elementwise cap, max norm {d.max().item() / ref.abs().max().item():.2e}")
        assert (d <= cap).all(), (shape, tag, what, r_cap)
    if (H, W) == (2, 2):
        assert not got[:, :, 0, :].any() and not got[:, :, :, 0].any()


def test_s2_wgrad_gate_edges():
    """Odd H, odd W, a channel count that is no multiple of 64, fp32 and W over the limit are declined with the invalid-argument status
    and launch nothing; N = 0 writes zeros."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    L = _lib.lib()
    bf, f32 = torch.bfloat16, torch.float32
    assert hip_ops.conv3x3_s2_wgrad_supported(64, 64, bf) and hip_ops.conv3x3_s2_wgrad_supported(1280, 1280, torch.float16)
    assert not hip_ops.conv3x3_s2_wgrad_supported(72, 64, bf) and not hip_ops.conv3x3_s2_wgrad_supported(64, 96, bf)
    assert not hip_ops.conv3x3_s2_wgrad_supported(64, 64, f32)
    for H, W, Ci, Co, dt in ((3, 4, 64, 64, bf), (4, 5, 64, 64, bf), (4, 4, 72, 64, bf), (4, 4, 64, 96, bf), (4, 4, 64, 64, f32),
                             (2, MAX_W + 2, 64, 64, bf)):
        x = torch.randn(1, H * W, Ci, device=DEV).to(dt)
        dy = torch.randn(1, ((H + 1) // 2) * ((W + 1) // 2), Co, device=DEV).to(dt)
        dw = torch.zeros(Co, Ci, 3, 3, device=DEV)
        rc = L.mvi_conv3x3_s2_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 1, H, W, Ci, Co, hip_ops._DT[dt], None, 0, None)
        assert rc == -1, (H, W, Ci, Co, dt, rc)                  # MVI_EINVAL
        with pytest.raises(Exception, match="conv3x3.s2.wgrad"):
            hip_ops.conv3x3_s2_wgrad(x, dy, H, W)
        torch.cuda.synchronize()
        assert not dw.any()
    x = torch.randn(1, 16, 64, device=DEV).to(bf)
    dw = torch.ones(64, 64, 3, 3, device=DEV)
    rc = L.mvi_conv3x3_s2_wgrad(x.data_ptr(), x.data_ptr(), dw.data_ptr(), 0, 4, 4, 64, 64, hip_ops._DT[bf], None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and not dw.any()


# ---- the stride-2 input gradient --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _s2_dx(shape, tag):
    N, H, W, Ci, Co = shape
    c = _s2_case(shape, tag)
    return R.s2_dgrad_formula(R.planes(c["dy"], H // 2, W // 2), c["w"], H, W)


@pytest.mark.parametrize("tag", list(R.DTYPES))
@pytest.mark.parametrize("shape", S2_DGRAD_SHAPES, ids=_id)
def test_s2_dgrad_on_the_forward_kernel_against_fp64(shape, tag):
    """dx = conv3x3_s2_dgrad(dy, packed transposed weight) against fp64 dx at the forward kernel's own bar
    (max|got - ref| <= tol max(1, max|ref|), tol 1/128 bf16, 1/1024 f16); with a zero weight dx is exactly 0."""
    _, hip_ops = _ops()
    N, H, W, Ci, Co = shape
    c, ref = _s2_case(shape, tag), _s2_dx(shape, tag)
    assert hip_ops.conv3x3_s2_dgrad_supported(Ci, Co, R.DTYPES[tag])
    wt = hip_ops.conv3x3_n320_weight(hip_ops.conv3x3_transposed_weight(c["w"].to(DEV)))
    dyd = c["dy"].to(DEV)
    out, kinds = _profiled(lambda: hip_ops.conv3x3_s2_dgrad(dyd, wt, H, W))
    assert kinds == ["conv3x3_s2_dgrad"], kinds
    assert tuple(out.shape) == (N, H * W, Ci)
    err = (R.planes(out.double().cpu(), H, W) - ref).abs().max().item()
    bar = DGRAD_TOL[tag] * max(1.0, ref.abs().max().item())
    H_.report(f"conv3x3_s2_dgrad {_id(shape)} {tag}: max error {err:.2e} = {err / bar:.3f} of the bar")
    assert err <= bar, (shape, tag, err, bar)
    zero = hip_ops.conv3x3_s2_dgrad(dyd, torch.zeros_like(wt), H, W)
    assert not zero.any()


def test_s2_dgrad_gate_edges():
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    L = _lib.lib()
    bf = torch.bfloat16
    assert hip_ops.conv3x3_s2_dgrad_supported(320, 64, bf) and not hip_ops.conv3x3_s2_dgrad_supported(64, 320, bf)
    assert not hip_ops.conv3x3_s2_dgrad_supported(320, 64, torch.float32)
    dy = torch.randn(1, 6, 64, device=DEV).to(bf)
    wt = torch.zeros(320, 9 * 64, device=DEV, dtype=bf)
    dx = torch.zeros(256, 320, device=DEV, dtype=bf)
    for H, W in ((3, 4), (4, 3)):
        rc = L.mvi_conv3x3_s2_dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1, H, W, 320, 64, 256, 320, hip_ops._DT[bf], None)
        assert rc == -1, rc
    rc = L.mvi_conv3x3_s2_dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1, 4, 6, 320, 64, 0, 320, hip_ops._DT[bf], None)   # no room for a block
    assert rc == -1, rc


# ---- the 2x2 pooling pass and the upsampling form's input gradient -----------------------------------------------------------------------

@pytest.mark.parametrize("tag", list(R.DTYPES))
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_id)
def test_pool2x2_sum(shape, tag):
    """|out - s| <= ROUND |s| + 4 2^-24 sum|g_i| against the fp64 sum s of the four values: an fp32 sum rounded once."""
    _, hip_ops = _ops()
    N, h, w, C = shape
    g = torch.randn(N, 4 * h * w, C, generator=torch.Generator().manual_seed(sum(shape))).to(R.DTYPES[tag])
    out, kinds = _profiled(lambda: hip_ops.pool2x2_sum(g.to(DEV), h, w))
    assert kinds == ["pool2x2_sum"] and tuple(out.shape) == (N, h * w, C) and out.dtype == g.dtype
    cells = g.double().reshape(N, h, 2, w, 2, C)
    s, sa = cells.sum(dim=(2, 4)).reshape(N, h * w, C), cells.abs().sum(dim=(2, 4)).reshape(N, h * w, C)
    d = (out.double().cpu() - s).abs()
    bound = ROUND[tag] * s.abs() + 4 * 2.0 ** -24 * sa
    H_.report(f"pool2x2_sum {_id(shape)} {tag}: {(d / bound.clamp_min(1e-300)).max().item():.3f} of the bound")
    assert (d <= bound).all()
    with pytest.raises(Exception, match="pool2x2_sum"):
        hip_ops.pool2x2_sum(torch.zeros(1, 4, 12, device=DEV, dtype=g.dtype), 1, 1)


@functools.lru_cache(maxsize=None)
def _up_case(shape, tag):
    N, h, w, Ci, Co = shape
    x, dy, wt, b = R.make_up(shape, R.DTYPES[tag], seed=11 + sum(shape))
    return {"x": x, "dy": dy, "w": wt, "b": b, "dx": R.up_dgrad_formula(R.planes(dy, 2 * h, 2 * w), wt)}


def _pytorch_up_dx(c, shape):
    """dx of the PyTorch route, F.conv2d(F.interpolate(x), ...) under autograd on the GPU in the same dtype, as planes."""
    N, h, w, Ci, Co = shape
    xg = R.planes(c["x"], h, w).to(DEV).contiguous().requires_grad_()
    y = F.conv2d(F.interpolate(xg, scale_factor=2, mode="nearest"), c["w"].to(DEV), c["b"].to(DEV), padding=1)
    y.backward(R.planes(c["dy"], 2 * h, 2 * w).to(DEV).contiguous())
    return xg.grad.cpu()


def _assert_inside_module_bar(name, got, old, ref):
    o_max, o_rms = R.errors(old, ref)
    e_max, e_rms = R.errors(got, ref)
    H_.report(f"{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the PyTorch route's own error "
              f"(max {o_max:.2e}, rms {o_rms:.2e})")
    assert e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms, (name, e_max, o_max, e_rms, o_rms)


@pytest.mark.parametrize("tag", list(R.DTYPES))
@pytest.mark.parametrize("shape", UP_DGRAD_SHAPES, ids=_id)
def test_up_dgrad_against_fp64_and_the_pytorch_route(shape, tag, route_every_supported_shape):
    """dx of the upsampling form — ops.conv3x3_up_dgrad, the backward of ops._ConvTokensFn's "up2" form: conv3x3_dgrad at 2 h x 2 w + pool2x2_sum —
    against fp64. It carries one more rounding than a bare dgrad, so its bar is the module bar: error <= 2.0 x (max) / 1.6 x (rms) of the
    error of F.conv2d(F.interpolate(x)) under autograd on the GPU in the same dtype. Where the forward kernel takes the shape too (C_out a
    multiple of 320) the same bits come out of ops.conv3x3_up_tokens(...).backward."""
    ops, hip_ops = _ops()
    N, h, w, Ci, Co = shape
    c = _up_case(shape, tag)
    dyd, wd = c["dy"].to(DEV), c["w"].to(DEV)
    dx, kinds = _profiled(lambda: ops.conv3x3_up_dgrad(dyd, wd, h, w))
    assert kinds == ["conv3x3_dgrad", "pool2x2_sum"], kinds
    assert tuple(dx.shape) == (N, h * w, Ci)
    _assert_inside_module_bar(f"conv3x3_up dgrad {_id(shape)} {tag}", R.planes(dx.cpu(), h, w), _pytorch_up_dx(c, shape), c["dx"])
    if ops.conv3x3_up_tokens_gates(N, h, w, Ci, Co, R.DTYPES[tag]):
        xa = c["x"].to(DEV).requires_grad_()
        ops.conv3x3_up_tokens(xa, wd, c["b"].to(DEV), h, w).backward(dyd)
        assert torch.equal(xa.grad, dx)
    else:
        assert Co % 320, "only the forward kernel's C_out gate may keep a shape of this list off the op"


def test_up_dgrad_list_reaches_the_op(route_every_supported_shape):
    ops, _ = _ops()
    assert any(ops.conv3x3_up_tokens_gates(*s, torch.bfloat16) for s in UP_DGRAD_SHAPES)


# ---- the ops under autograd --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", list(R.DTYPES))
@pytest.mark.parametrize("shape", DOWN_OP_SHAPES, ids=_id)
def test_conv3x3_down_tokens_under_autograd(shape, tag, route_every_supported_shape):
    """y bit-identical to the no-grad launch; weight.grad = conv3x3_s2_wgrad(...).to(dtype) bit for bit; dx inside the dgrad bar; dbias
    inside ROUND |ref| + n 2^-24 sum|dy|; two backward runs bit-identical; with the weight frozen only the dgrad kind runs; the same
    numbers under checkpoint(use_reentrant=False)."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = R.DTYPES[tag]
    N, H, W, Ci, Co = shape
    assert ops.conv3x3_down_tokens_gates(*shape, dt)
    c = _s2_case(shape, tag)
    xd, dyd, wd, bd = (c[k].to(DEV) for k in ("x", "dy", "w", "b"))
    with torch.no_grad():
        y0, kinds = _profiled(lambda: ops.conv3x3_down_tokens(xd, wd, bd, H, W))
    assert kinds == ["conv3x3_n320"], kinds

    def run(train=True, ckpt=False):
        xa, wa, ba = xd.clone().requires_grad_(), wd.clone().requires_grad_(train), bd.clone().requires_grad_(train)
        fn = (lambda: checkpoint(ops.conv3x3_down_tokens, xa, wa, ba, H, W, use_reentrant=False)) if ckpt else \
            (lambda: ops.conv3x3_down_tokens(xa, wa, ba, H, W))
        y, k_f = _profiled(fn)
        _, k_b = _profiled(lambda: y.backward(dyd))
        return y.detach(), xa.grad, wa.grad, ba.grad, k_f, k_b

    y, dx, dw, db, k_f, k_b = run()
    assert k_f == ["conv3x3_n320"] and torch.equal(y, y0)
    assert sorted(k_b) == ["conv3x3_s2_dgrad", "conv3x3_s2_wgrad"], k_b
    _, dx2, dw2, db2, _, _ = run()
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2), "two backward runs must give the same bits"
    assert dw.dtype == dt and torch.equal(dw, hip_ops.conv3x3_s2_wgrad(xd, dyd, H, W).to(dt))
    ref_dx = _s2_dx(shape, tag)
    e_x = (R.planes(dx.double().cpu(), H, W) - ref_dx).abs().max().item()
    bar_x = DGRAD_TOL[tag] * max(1.0, ref_dx.abs().max().item())
    ref_db = c["dy"].double().sum(dim=(0, 1))
    n = c["dy"].shape[0] * c["dy"].shape[1]
    bar_b = ROUND[tag] * ref_db.abs() + n * 2.0 ** -24 * c["dy"].double().abs().sum(dim=(0, 1))
    d_b = (db.double().cpu() - ref_db).abs()
    H_.report(f"conv3x3_down_tokens {_id(shape)} {tag}: dx {e_x / bar_x:.3f} of its bar, dbias {(d_b / bar_b).max().item():.3f} of its bound")
    assert e_x <= bar_x, (shape, tag, e_x, bar_x)
    assert (d_b <= bar_b).all()

    _, dx_f, dw_f, db_f, k_f, k_b = run(train=False)
    assert k_f == ["conv3x3_n320"] and k_b == ["conv3x3_s2_dgrad"], (k_f, k_b)
    assert dw_f is None and db_f is None and torch.equal(dx_f, dx), "dx must not depend on whether the weight requires grad"
    wo = wd.clone().requires_grad_()
    _, k = _profiled(lambda: ops.conv3x3_down_tokens(xd, wo, None, H, W).backward(dyd))
    assert k == ["conv3x3_n320", "conv3x3_s2_wgrad"], k
    assert torch.equal(wo.grad, dw)

    _, dx_c, dw_c, db_c, k_f, k_b = run(ckpt=True)
    kinds = k_f + k_b
    assert kinds.count("conv3x3_n320") in (1, 2) and kinds.count("conv3x3_s2_dgrad") == 1 and kinds.count("conv3x3_s2_wgrad") == 1, kinds
    assert torch.equal(dx_c, dx) and torch.equal(dw_c, dw) and torch.equal(db_c, db)


@pytest.mark.parametrize("tag", list(R.DTYPES))
@pytest.mark.parametrize("shape", UP_OP_SHAPES, ids=_id)
def test_conv3x3_up_tokens_under_autograd(shape, tag, route_every_supported_shape):
    """y bit-identical to the no-grad launch; dx inside the module bar; two backward runs bit-identical; only the forward, the dgrad and the
    pooling kinds run; nothing but the weight is saved for the backward; the same numbers under checkpoint(use_reentrant=False)."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = R.DTYPES[tag]
    N, h, w, Ci, Co = shape
    assert ops.conv3x3_up_tokens_gates(*shape, dt)
    c = _up_case(shape, tag)
    xd, dyd, wd, bd = (c[k].to(DEV) for k in ("x", "dy", "w", "b"))
    with torch.no_grad():
        y0, kinds = _profiled(lambda: ops.conv3x3_up_tokens(xd, wd, bd, h, w))
    assert kinds == ["conv3x3_n320"], kinds

    def run(ckpt=False):
        xa = xd.clone().requires_grad_()
        fn = (lambda: checkpoint(ops.conv3x3_up_tokens, xa, wd, bd, h, w, use_reentrant=False)) if ckpt else \
            (lambda: ops.conv3x3_up_tokens(xa, wd, bd, h, w))
        y, k_f = _profiled(fn)
        saved = [t for t in getattr(y.grad_fn, "saved_tensors", ())]
        _, k_b = _profiled(lambda: y.backward(dyd))
        return y.detach(), xa.grad, k_f + k_b, saved

    y, dx, kinds, saved = run()
    assert torch.equal(y, y0) and kinds == ["conv3x3_n320", "conv3x3_dgrad", "pool2x2_sum"], kinds
    assert [tuple(t.shape) for t in saved] == [tuple(wd.shape)], "the op keeps the weight only: neither x nor the 4x tensor"
    _, dx2, _, _ = run()
    assert torch.equal(dx, dx2)
    _assert_inside_module_bar(f"conv3x3_up_tokens {_id(shape)} {tag} dx", R.planes(dx.cpu(), h, w), _pytorch_up_dx(c, shape), c["dx"])
    _, dx_c, kinds, _ = run(ckpt=True)
    assert kinds.count("conv3x3_dgrad") == 1 and kinds.count("pool2x2_sum") == 1 and kinds.count("conv3x3_n320") in (1, 2), kinds
    assert torch.equal(dx_c, dx)


# ---- routing -----------------------------------------------------------------------------------------------------------------------------

def test_routing_and_strict_mode(route_every_supported_shape):
    """Switch off, odd H, fp32: strict mode raises, non-strict mode records the op's name with "requires grad" and runs no resample kind;
    conv3x3_up_tokens with a trainable weight is a recorded fallback; the substitutes compute the same convolution."""
    ops, hip_ops = _ops()
    bf = torch.bfloat16
    new_kinds = ("conv3x3_s2_dgrad", "conv3x3_s2_wgrad", "pool2x2_sum", "conv3x3_dgrad")
    g = torch.Generator().manual_seed(3)

    def down(N, H, W, C, dt, train=False):
        x = torch.randn(N, H * W, C, generator=g).to(dt).to(DEV).requires_grad_()
        wt = (torch.randn(320, C, 3, 3, generator=g) / 50).to(dt).to(DEV).requires_grad_(train)
        return lambda: ops.conv3x3_down_tokens(x, wt, None, H, W).sum().backward() or x.grad

    def up(N, h, w, C, dt, train=False):
        x = torch.randn(N, h * w, C, generator=g).to(dt).to(DEV).requires_grad_()
        wt = (torch.randn(320, C, 3, 3, generator=g) / 50).to(dt).to(DEV).requires_grad_(train)
        return lambda: ops.conv3x3_up_tokens(x, wt, None, h, w).sum().backward() or x.grad

    _, kinds = _profiled(down(2, 6, 10, 320, bf))
    assert kinds == ["conv3x3_n320", "conv3x3_s2_dgrad"], kinds
    _, kinds = _profiled(up(2, 3, 5, 320, bf))
    assert kinds == ["conv3x3_n320", "conv3x3_dgrad", "pool2x2_sum"], kinds

    cases = [("conv3x3_down_tokens", down(2, 6, 10, 320, bf), True), ("conv3x3_up_tokens", up(2, 3, 5, 320, bf), True),
             ("conv3x3_down_tokens", down(2, 5, 10, 320, bf), False), ("conv3x3_down_tokens", down(2, 6, 9, 320, bf), False),
             ("conv3x3_down_tokens", down(2, 6, 10, 320, torch.float32), False), ("conv3x3_up_tokens", up(2, 3, 5, 320, torch.float32), False),
             ("conv3x3_up_tokens", up(2, 3, 5, 320, bf, train=True), False)]
    for name, fn, switch_off in cases:
        ops.RESAMPLE_CONV_BACKWARD = not switch_off              # (restored by the module's fixture)
        ops.STRICT = True
        with pytest.raises(ops.HipPathError, match=name):
            fn()
        ops.STRICT = False
        del ops.FALLBACKS[:]
        gx, kinds = _profiled(fn)
        assert (name, "requires grad") in ops.FALLBACKS and not [k for k in kinds if k in new_kinds], (name, ops.FALLBACKS, kinds)
        assert gx is not None
        ops.RESAMPLE_CONV_BACKWARD, ops.STRICT = True, True


def test_speed_decisions_answer_for_every_training_shape():
    """ops.conv3x3_down_backward_pays / conv3x3_up_backward_pays follow tools/bench_resample_conv_bwd.py; whatever the table says the answer is
    a bool for every training shape, the gates take every one of them, and strict mode raises where the answer is no."""
    from multiview_inpaint_amd.svd import layers
    ops, _ = _ops()
    for dt in (torch.bfloat16, torch.float16):
        for H, W, C in TRAINING_SHAPES:
            assert ops.conv3x3_down_tokens_gates(14, H, W, C, C, dt) and ops.conv3x3_up_tokens_gates(14, H // 2, W // 2, C, C, dt)
            for need_dw in (False, True):
                assert ops.conv3x3_down_backward_pays(14, H, W, C, C, dt, need_dw) in (True, False)
            assert ops.conv3x3_up_backward_pays(14, H // 2, W // 2, C, C, dt) in (True, False)
            for which, trains in (("down", True), ("down", False), ("up", False)):
                assert layers.resample_conv_module_pays(which, 14, H, W, C, dt, trains) in (True, False)
    assert isinstance(layers.RESAMPLE_CONV_BWD, bool) and layers.RESAMPLE_CONV_BWD is False
    if not ops.conv3x3_down_backward_pays(2, 6, 10, 320, 320, torch.bfloat16, False):
        x = torch.zeros(2, 60, 320, device=DEV, dtype=torch.bfloat16).requires_grad_()
        with pytest.raises(ops.HipPathError):
            ops.conv3x3_down_tokens(x, torch.zeros(320, 320, 3, 3, device=DEV, dtype=torch.bfloat16), None, 6, 10)


# ---- the modules -------------------------------------------------------------------------------------------------------------------------

def _seed_params(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
            p.copy_(p.to(torch.bfloat16).to(p.dtype))


@pytest.mark.parametrize("which", ["Downsample", "Upsample"])
def test_module_under_checkpoint_against_the_parent_route(which, route_every_supported_shape):
    """layers.Downsample(320, True) on [3, 320, 10, 14] (trainable) and layers.Upsample(320, True) on [3, 320, 5, 7] (frozen: its HIP route
    is the frozen UNet's), bf16, under checkpoint(use_reentrant=False) with RESAMPLE_CONV_BWD on: every gradient against the fp64 CPU
    module, at most 2.0 x (max) / 1.6 x (rms) of the parent route's own error. With the switch off the module IS the parent route: output
    and gradients equal the plain library calls bit for bit and no resample kind runs."""
    from torch.utils.checkpoint import checkpoint
    from multiview_inpaint_amd.svd import layers
    ops, _ = _ops()
    dt = torch.bfloat16
    down = which == "Downsample"
    h, w = (10, 14) if down else (5, 7)

    def make():
        m = (layers.Downsample if down else layers.Upsample)(320, True)
        _seed_params(m, 23)
        return m
    g = torch.Generator().manual_seed(29)
    x = torch.randn(3, 320, h, w, generator=g).to(dt)
    dy = torch.randn(3, 320, *((h // 2, w // 2) if down else (2 * h, 2 * w)), generator=g).to(dt)
    m64 = make().double()
    x64 = x.double().requires_grad_()
    m64(x64).backward(dy.double())
    ref = {"x": x64.grad, **({n: p.grad for n, p in m64.named_parameters()} if down else {})}

    def gpu_run():
        m = make().to(DEV, dt).requires_grad_(down)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        y, k_f = _profiled(lambda: checkpoint(m, xg, use_reentrant=False))
        _, k_b = _profiled(lambda: y.backward(dy.to(DEV)))
        return m, y.detach(), {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters() if p.grad is not None}}, k_f + k_b, list(ops.FALLBACKS)

    layers.RESAMPLE_CONV_BWD = True
    _, y_new, new, kinds, fallbacks = gpu_run()
    assert not fallbacks, fallbacks
    if down:
        assert kinds.count("conv3x3_s2_dgrad") == 1 and kinds.count("conv3x3_s2_wgrad") == 1, kinds
    else:
        assert kinds.count("conv3x3_dgrad") == 1 and kinds.count("pool2x2_sum") == 1, kinds
    layers.RESAMPLE_CONV_BWD = False
    m, y_old, old, old_kinds, _ = gpu_run()
    assert not old_kinds, old_kinds
    assert set(new) == set(old) == set(ref), (set(new), set(old), set(ref))
    for name in new:
        _assert_inside_module_bar(f"{which} 320 3x{h}x{w} bf16 d{name}", new[name].cpu(), old[name].cpu(), ref[name])

    # the switch off: the parent route, bit for bit
    conv = m.op if down else m.conv
    xg = x.to(DEV).requires_grad_()
    wl, bl = conv.weight.detach().clone().requires_grad_(down), conv.bias.detach().clone().requires_grad_(down)
    yl = F.conv2d(xg, wl, bl, 2, 1) if down else F.conv2d(F.interpolate(xg, scale_factor=2, mode="nearest"), wl, bl, 1, 1)
    yl.backward(dy.to(DEV))
    assert torch.equal(yl.detach(), y_old) and torch.equal(xg.grad, old["x"])
    if down:
        assert torch.equal(wl.grad, old["op.weight"]) and torch.equal(bl.grad, old["op.bias"])

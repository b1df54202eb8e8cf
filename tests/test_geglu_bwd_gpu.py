"""GPU parity of the differentiable GEGLU (csrc/ff_geglu_bwd.hip and csrc/geglu.hip through svd/ops.py's autograd Functions).

Parity chain: the reference's GEGLU under fp64 autograd -> the fp64 formula of tests/geglu_bwd_helpers.py
(tests/test_geglu_bwd_cpu.py, 1e-12) -> the kernels (here). Bars: the project's 16-bit gradient bars applied to the reference's OWN
error in the same 16-bit type (the same module run in bf16 / f16 on the CPU against its fp64 self, recorded by
tools/gen_golden_geglu_bwd.py in the fixtures and in tests/golden/geglu_bwd/ref_errors.json): rms <= 1.6 x, max norm <= 2.0 x.
Every test runs with ops.STRICT = True unless it says otherwise: a GEGLU that left the HIP path under autograd would raise."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import geglu_bwd_helpers as G
import svd_helpers as H

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multiview_inpaint_amd", "dropin")
if DROPIN not in sys.path:
    sys.path.insert(0, DROPIN)

# The bars of tests/test_attention_bwd_gpu.py / test_groupnorm_bwd_gpu.py (copied, not imported): the build's error as a multiple of
# the reference's own error in the same type, rms and max norm.
RMS_BAR = 1.6
MAX_BAR = 2.0
DEV = "cuda"
MIB = 1 << 20


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    """MVI_STRICT for every test of this module (svd/ops.py), and the HIP backward switched on even where the environment says
    MVI_FF_GEGLU_BWD=0."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "FF_GEGLU_BACKWARD", True)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """ops.linear_geglu_backward_pays / geglu_backward_pays are speed decisions (small problems are left to PyTorch); parity on small
    shapes is checked with the decisions lifted, so that what is tested is what the kernels compute."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "linear_geglu_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "geglu_backward_pays", lambda *a: True)


def _ops():
    from multiview_inpaint_amd.svd import hip_ops, ops
    return ops, hip_ops


def _check(name, got, ref, r_max, r_rms):
    e_max, e_rms = G.errors(got.detach().cpu(), ref)
    H.report(f"{name}: max {e_max:.2e} = {e_max / r_max:.2f} x, rms {e_rms:.2e} = {e_rms / r_rms:.2f} x the reference's own error")
    return e_max <= MAX_BAR * r_max and e_rms <= RMS_BAR * r_rms, (name, e_max, r_max, e_rms, r_rms)


def _assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


def _profiled(fn):
    _, hip_ops = _ops()
    hip_ops.PROFILE = []
    try:
        out = fn()
        kinds = [p[0] for p in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = None
    return out, kinds


FIXTURES = [(case, tag) for case in G.TENSOR_CASES for tag in G.DTYPES]


@pytest.mark.parametrize("case,tag", FIXTURES, ids=[G.case_name(c, t) for c, t in FIXTURES])
def test_fixture_gradients_within_the_reference_own_error(case, tag, route_every_supported_shape):
    """ops.geglu(F.linear(x, w, b)) on the fixture's inputs under autograd (K = 64 / 96: the elementwise pair geglu / geglu_backward
    behind the library GEMM): dx, dweight, dbias against the reference's fp64 results at 1.6 x (rms) / 2.0 x (max norm) of the
    reference's own error in that type by G.ref_error_for: these shapes are not in ref_errors.json, so the largest recorded entry
    of the type. The fixture's own six numbers are printed beside it, not asserted; DESIGN.md 'GEGLU under autograd' records what
    they came to on an MI355X (one f16 dbias max norm at 2.04 x its fixture's own figure, 0.79 x the asserted bar) and why the bar
    is ref_error_for's."""
    ops, _ = _ops()
    Fx = np.load(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz"))
    dtype = G.DTYPES[tag]
    x, w, b, dy = (G.from_bits(Fx[n], dtype).to(DEV).requires_grad_() for n in ("x", "weight", "bias", "dy"))
    err = dict(zip(G.ERROR_FIELDS, (float(e) for e in Fx["ref_err"])))

    def run():
        y = ops.geglu(F.linear(x, w, b))
        y.backward(dy.detach())
        return y
    y, kinds = _profiled(run)
    assert kinds == ["geglu", "geglu_bwd"], kinds
    name = G.case_name(case, tag)
    r = G.ref_error_for(case, tag)
    for n, t in (("dx", x), ("dweight", w), ("dbias", b)):
        e_max, e_rms = G.errors(t.grad.float().cpu(), torch.from_numpy(Fx[n]))
        H.report(f"{name} {n}: {e_max / err[n + '_max']:.2f} x max, {e_rms / err[n + '_rms']:.2f} x rms of the fixture's own figures")
    _assert_all([_check(f"{name} {n}", t.grad.float(), torch.from_numpy(Fx[n]), r[n + "_max"], r[n + "_rms"])
                 for n, t in (("dx", x), ("dweight", w), ("dbias", b))])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "f16"])
def test_elementwise_backward_against_the_fp64_gate(dtype, route_every_supported_shape):
    """hip_ops.geglu_backward on h = 2.5 randn with gates out to +-8 against the written-out fp64 gate. fp32 I/O: 1e-4 relative max
    norm (the project's fp32 contract); bf16 / f16: one rounding of the result, 2^-8 / 2^-11 relative max norm. Two runs are
    bit-identical; through ops.geglu under autograd the same bits arrive."""
    ops, hip_ops = _ops()
    g = torch.Generator().manual_seed(17)
    rows, inner = 1037, 160
    h = (2.5 * torch.randn(rows, 2 * inner, generator=g)).to(dtype)
    h[:, inner:inner + 8] = torch.linspace(-8.0, 8.0, rows)[:, None].to(dtype)
    dy = torch.randn(rows, inner, generator=g).to(dtype)
    _, dh_ref = G.gate_formula(h, dy)
    hd, dyd = h.to(DEV), dy.to(DEV)
    dh = hip_ops.geglu_backward(hd, dyd)
    assert torch.equal(dh, hip_ops.geglu_backward(hd, dyd))
    ha = hd.clone().requires_grad_()
    ya = ops.geglu(ha)
    ya.backward(dyd)
    assert torch.equal(ha.grad, dh) and torch.equal(ya.detach(), hip_ops.geglu(hd))
    e_max, e_rms = G.errors(dh.cpu(), dh_ref)
    H.report(f"geglu_backward {dtype}: max {e_max:.2e}, rms {e_rms:.2e}")
    bar = {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    assert e_max <= bar, (e_max, bar)


# (case, variant): K = 320 through ops.linear_geglu. rows a multiple of 256, ragged rows, inner 64 and 1280, gates in both tails
# (G.TAIL_CASES), a strided x view, bias None, and the training shape 14 x 3072 rows.
SHAPE_CASES = [((4096, 320, 1280), "plain"), ((2125, 320, 1280), "plain"), ((4096, 320, 64), "plain"), ((2125, 320, 64), "plain"),
               ((515, 320, 160), "plain"), ((2125, 320, 160), "strided"), ((300, 320, 1280), "nobias"),
               ((G.TRAINING_ROWS, 320, 1280), "plain")]
SHAPES = [(case, variant, tag) for case, variant in SHAPE_CASES for tag in G.DTYPES]


@pytest.mark.parametrize("case,variant,tag", SHAPES, ids=[f"{G.case_name(c, t)}_{v}" for c, v, t in SHAPES])
def test_k320_shapes_against_the_fp64_formula(case, variant, tag, route_every_supported_shape):
    """ops.linear_geglu under autograd against the fp64 formula evaluated on this machine's CPU, once with every leaf requiring grad
    (need_dparams on: dx, dweight, dbias) and once with only x requiring grad (need_dparams off: the kStoreDh = false form). Bar:
    1.6 x / 2.0 x the reference's own error of ref_errors.json — the entry of the same shape where there is one, else the largest of
    the type. Also for every shape: y under autograd is bit-identical to the no-grad y; dx is the same bits in both forms; two
    backward runs are bit-identical in dx, dh and dbias. dweight = dh^T x goes through the library GEMM, which does not sum in a fixed
    order ('What's weak', item 2): it is held to the bars only, not to bit identity."""
    ops, hip_ops = _ops()
    rows, K, inner = case
    dtype = G.DTYPES[tag]
    x, w, b, dy = G.make_inputs(case, dtype)
    if variant == "nobias":
        b = None
    _, fdx, fdw, fdb = G.formula(x, w, b, dy)
    if variant == "strided":                                     # rows of 320 inside rows of 384
        wide = torch.zeros(rows, 384, dtype=dtype, device=DEV)
        wide[:, 32:352] = x.to(DEV)
        xd = wide[:, 32:352]
        assert not xd.is_contiguous()
    else:
        xd = x.to(DEV)
    wd, dyd = w.to(DEV), dy.to(DEV)
    bd = None if b is None else b.to(DEV)
    assert hip_ops.ff_geglu_backward_supported(K, inner, dtype)
    with torch.no_grad():
        y0 = ops.linear_geglu(xd, wd, bd) if rows >= ops.FF_GEGLU_MIN_ROWS else hip_ops.ff_geglu(xd, wd, bd)

    xa, wa = xd.detach().requires_grad_(), wd.clone().requires_grad_()
    ba = None if bd is None else bd.clone().requires_grad_()

    def run_all():
        y = ops.linear_geglu(xa, wa, ba)
        y.backward(dyd)
        return y
    y, kinds = _profiled(run_all)
    assert kinds == ["ff_geglu", "ff_geglu_bwd", "ff_geglu_dparams"], kinds
    assert torch.equal(y.detach(), y0), "the forward under autograd must be the inference forward, bit for bit"
    xo = xd.detach().requires_grad_()
    _, kinds = _profiled(lambda: ops.linear_geglu(xo, wd, bd).backward(dyd))
    assert kinds == ["ff_geglu", "ff_geglu_bwd"], kinds
    assert torch.equal(xo.grad, xa.grad), "dx must not depend on whether dh is stored"

    one = hip_ops._ff_geglu_backward(xd, wd, bd, dyd, True, True, True)
    two = hip_ops._ff_geglu_backward(xd, wd, bd, dyd, True, True, True)
    assert torch.equal(one[0], two[0]) and torch.equal(one[3], two[3]) and torch.equal(one[0], xa.grad.reshape(one[0].shape))
    if bd is not None:
        assert torch.equal(one[2], two[2]) and torch.equal(one[2].to(dtype), ba.grad)
        # only the bias trainable, x frozen: the kernel's dh-only form (no contraction, no GEMM) stores the same dh
        only_b = hip_ops._ff_geglu_backward(xd, wd, bd, dyd, False, False, True)
        assert only_b[0] is None and only_b[1] is None and torch.equal(only_b[2], one[2]) and torch.equal(only_b[3], one[3])

    r = G.ref_error_for(case, tag)
    name = f"{G.case_name(case, tag)} {variant}"
    results = [_check(f"{name} dx", xa.grad, fdx, r["dx_max"], r["dx_rms"]),
               _check(f"{name} dweight", wa.grad, fdw, r["dweight_max"], r["dweight_rms"])]
    if ba is not None:
        results.append(_check(f"{name} dbias", ba.grad, fdb, r["dbias_max"], r["dbias_rms"]))
    _assert_all(results)


@pytest.mark.parametrize("tag", list(G.DTYPES))
def test_memory_held_between_forward_and_backward(tag, route_every_supported_shape):
    """A condition, not a measurement, at rows = 14 x 3072, inner = 1280, x and w resident: after the forward the HIP route holds its
    output (whole 256-row blocks) and nothing else tensor-sized — at most out_rows x inner x itemsize + 1 MiB — where the PyTorch
    route (FF_GEGLU_BACKWARD off) holds more than 3 x that (the projection, gelu(gate) and the product). With frozen weights the
    backward's peak above that level is at most dx + 1 MiB: no dh."""
    ops, hip_ops = _ops()
    from multiview_inpaint_amd import _lib
    dtype = G.DTYPES[tag]
    rows, K, inner = G.TRAINING_ROWS, 320, 1280
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(rows, K, device=DEV, generator=g).to(dtype).requires_grad_()
    w = (torch.randn(2 * inner, K, device=DEV, generator=g) / K ** 0.5).to(dtype)
    b = torch.randn(2 * inner, device=DEV, generator=g).to(dtype)
    dy = torch.randn(rows, inner, device=DEV, generator=g).to(dtype)
    hip_ops.ff_geglu(x.detach(), w, b)                           # the fp32 copy of the bias is cached before anything is measured
    out_bytes = int(_lib.lib().mvi_ff_geglu_out_rows(rows)) * inner * x.element_size()
    dx_bytes = rows * K * x.element_size()

    def held(on):
        ops.FF_GEGLU_BACKWARD, ops.STRICT = on, on               # (restored by the module's fixture)
        x.grad = None
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        y = ops.linear_geglu(x, w, b)
        torch.cuda.synchronize()
        m1 = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y.backward(dy)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - m1
        del y
        return m1 - m0, peak
    hip_fwd, hip_peak = held(True)
    lib_fwd, lib_peak = held(False)
    ops.FF_GEGLU_BACKWARD, ops.STRICT = True, True
    H.report(f"GEGLU {tag} rows {rows}: held after forward HIP {hip_fwd / MIB:.1f} MiB, PyTorch {lib_fwd / MIB:.1f} MiB (output "
             f"{out_bytes / MIB:.1f}); backward peak above it HIP {hip_peak / MIB:.1f} MiB, PyTorch {lib_peak / MIB:.1f} MiB (dx {dx_bytes / MIB:.1f})")
    assert hip_fwd <= out_bytes + MIB, (hip_fwd, out_bytes)
    assert lib_fwd > 3 * (out_bytes + MIB), (lib_fwd, out_bytes)
    assert hip_peak <= dx_bytes + MIB, (hip_peak, dx_bytes)


def test_routing_and_strict_mode(monkeypatch):
    """With STRICT on: supported, paying shapes under grad record the new kinds and do not raise; with FF_GEGLU_BACKWARD off strict
    mode raises as before this feature, and without strict mode FALLBACKS holds ("geglu", "requires grad"); with nothing requiring
    grad, or under no_grad, PROFILE shows the inference kinds; an unsupported dtype or K, or a shape below the speed line, falls
    through as before."""
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    rows = 2 * G.TRAINING_ROWS                                   # bf16: the smallest size routed by default (28 x 3072 rows)
    x = torch.randn(28, 3072, 320, device=DEV, dtype=dt)
    w = torch.randn(2560, 320, device=DEV, dtype=dt) / 18
    b = torch.randn(2560, device=DEV, dtype=dt)
    h = torch.randn(14, 768, 2 * 2560, device=DEV, dtype=dt)     # level 1 of the training latent
    assert ops.linear_geglu_backward_pays(rows, 320, 1280, dt, True) and ops.geglu_backward_pays(14 * 768, 2560, dt)
    del ops.FALLBACKS[:]

    def under_grad():
        xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
        ops.linear_geglu(xa, wa, b).sum().backward()
        ha = h.clone().requires_grad_()
        ops.geglu(ha).sum().backward()
        return xa, wa, ha
    (xa, wa, ha), kinds = _profiled(under_grad)
    assert kinds == ["ff_geglu", "ff_geglu_bwd", "ff_geglu_dparams", "geglu", "geglu_bwd"], kinds
    assert xa.grad.shape == x.shape and wa.grad.shape == w.shape and ha.grad.shape == h.shape
    assert not [f for f in ops.FALLBACKS if f[0] == "geglu"], ops.FALLBACKS

    def inference():
        with torch.no_grad():
            ops.linear_geglu(xa, wa, b)
            ops.geglu(ha)
        ops.linear_geglu(x, w, b)                                # grad mode on, nothing requires grad
        ops.geglu(h)
    _, kinds = _profiled(inference)
    assert kinds == ["ff_geglu", "geglu", "ff_geglu", "geglu"], kinds

    # fp32 I/O at K = 320: no fused kernel; library GEMM, then ops.geglu, whose fp32 class was not measured and is not routed by
    # default (strict mode raises); with the speed decision lifted it is the elementwise pair, which takes fp32
    xf = x[:14].float().requires_grad_()
    assert not ops.geglu_backward_pays(rows // 2, 1280, torch.float32)
    with pytest.raises(ops.HipPathError):
        ops.linear_geglu(xf, w.float(), b.float())
    with monkeypatch.context() as m:
        m.setattr(ops, "geglu_backward_pays", lambda *a: True)
        _, kinds = _profiled(lambda: ops.linear_geglu(xf, w.float(), b.float()).sum().backward())
    assert kinds == ["geglu", "geglu_bwd"] and xf.grad is not None, kinds
    # bf16 at the training latent's 14 x 3072 rows tied in the bench: not routed by default
    assert not ops.linear_geglu_backward_pays(rows // 2, 320, 1280, dt, False)
    # K = 640 under grad: library GEMM, then the elementwise pair (no fused backward for the long contractions)
    x640 = torch.randn(14 * 768, 640, device=DEV, dtype=dt, requires_grad=True)
    w640 = torch.randn(2 * 2560, 640, device=DEV, dtype=dt) / 25
    _, kinds = _profiled(lambda: ops.linear_geglu(x640, w640, None).sum().backward())
    assert kinds == ["geglu", "geglu_bwd"], kinds
    # supported, but below the speed lines: PyTorch's path, so strict mode raises
    few = torch.randn(300, 320, device=DEV, dtype=dt, requires_grad=True)
    assert hip_ops.ff_geglu_backward_supported(320, 1280, dt) and not ops.linear_geglu_backward_pays(300, 320, 1280, dt, False)
    assert not ops.geglu_backward_pays(300, 1280, dt)
    with pytest.raises(ops.HipPathError):
        ops.linear_geglu(few, w, b)
    # the switch off: the parent's routing
    ops.FF_GEGLU_BACKWARD = False                                # (restored by the module's fixture)
    with pytest.raises(ops.HipPathError):
        ops.linear_geglu(x.clone().requires_grad_(), w, b)
    with pytest.raises(ops.HipPathError):
        ops.geglu(h.clone().requires_grad_())
    ops.STRICT = False
    del ops.FALLBACKS[:]
    _, kinds = _profiled(lambda: ops.linear_geglu(x.clone().requires_grad_(), w, b).sum().backward())
    assert ("geglu", "requires grad") in ops.FALLBACKS and not kinds, (ops.FALLBACKS, kinds)


def _module_gradients(make, ref_run, tag_name, strict):
    """Shared by the two module tests: `make()` builds the fp64 CPU module; gradients of the GPU bf16 copy under
    checkpoint(use_reentrant=False) against fp64, the new route held to 1.6 x / 2.0 x the parent route's own error per tensor, once
    with every parameter trainable and once frozen with only x requiring grad (then the GEGLU backward must not allocate dh: the peak
    above the level at its entry is at most dx + 1 MiB)."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    torch.manual_seed(23)
    m64 = make().double()
    with torch.no_grad():                                        # weights and inputs representable in bf16 on both sides
        for p in m64.parameters():
            p.copy_(p.to(dt).double())
    x = torch.randn(14, 3072, 320).to(dt)
    dy = torch.randn(14, 3072, 320).to(dt)
    ref = ref_run(m64, x, dy)

    peaks = []
    real_bwd = hip_ops.ff_geglu_backward

    def watched(xx, ww, bb, dd, need_dx=True, need_dparams=True, **kw):               # **kw: need_dweight / need_dbias
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = real_bwd(xx, ww, bb, dd, need_dx=need_dx, need_dparams=need_dparams, **kw)
        torch.cuda.synchronize()
        peaks.append((need_dparams, torch.cuda.max_memory_allocated() - m0, xx.numel() * xx.element_size()))
        return out

    def gpu_run(trainable):
        m = make()
        m.load_state_dict({k: v.float() for k, v in m64.state_dict().items()})
        m = m.to(DEV, dt).requires_grad_(trainable)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        del peaks[:]
        hip_ops.ff_geglu_backward = watched
        try:
            _, kinds = _profiled(lambda: checkpoint(m, xg, use_reentrant=False).backward(dy.to(DEV)))
        finally:
            hip_ops.ff_geglu_backward = real_bwd
        grads = {"x": xg.grad}
        if trainable:
            grads.update({n: p.grad for n, p in m.named_parameters()})
        return grads, kinds, list(ops.FALLBACKS), list(peaks)

    ops.STRICT = strict
    new, kinds, fallbacks, _ = gpu_run(True)
    assert not [f for f in fallbacks if f[0] == "geglu"], fallbacks
    # checkpoint re-runs the forward inside the backward: the Function's forward up to twice (nothing outside ctx is cached),
    # the backward once
    assert kinds.count("ff_geglu_bwd") == 1 and kinds.count("ff_geglu") in (1, 2), kinds
    frozen, kinds_f, fallbacks_f, peaks_f = gpu_run(False)
    assert not [f for f in fallbacks_f if f[0] == "geglu"] and kinds_f.count("ff_geglu_bwd") == 1, (fallbacks_f, kinds_f)
    assert len(peaks_f) == 1 and peaks_f[0][0] is False, peaks_f
    H.report(f"{tag_name} frozen: GEGLU backward peak {peaks_f[0][1] / MIB:.1f} MiB above its entry (dx {peaks_f[0][2] / MIB:.1f} MiB)")
    assert peaks_f[0][1] <= peaks_f[0][2] + MIB, peaks_f
    ops.STRICT, ops.FF_GEGLU_BACKWARD = False, False             # the parent's route (both restored by the module's fixture)
    old, old_kinds, old_fallbacks, _ = gpu_run(True)
    ops.STRICT, ops.FF_GEGLU_BACKWARD = True, True
    assert ("geglu", "requires grad") in old_fallbacks and "ff_geglu_bwd" not in old_kinds
    results = []
    for name, r in ref.items():
        o_max, o_rms = G.errors(old[name].cpu(), r)
        results.append(_check(f"{tag_name} bf16 d{name} (against the PyTorch route's own error {o_max:.2e} / {o_rms:.2e})",
                              new[name], r, o_max, o_rms))
    o_max, o_rms = G.errors(old["x"].cpu(), ref["x"])
    results.append(_check(f"{tag_name} bf16 frozen dx (against the PyTorch route's own error {o_max:.2e} / {o_rms:.2e})",
                          frozen["x"], ref["x"], o_max, o_rms))
    _assert_all(results)


def test_feedforward_module_under_checkpoint_against_the_parent_route(route_every_supported_shape):
    """The package's FeedForward(320, glu=True), bf16, 14 x 3072 tokens, in strict mode: see _module_gradients. (bf16 at 14 x 3072
    rows tied in the bench and is not routed by default: the speed decision is lifted, as for every parity test here.)"""
    from sgm.modules.attention import FeedForward

    def ref_run(m64, x, dy):
        x64 = x.double().requires_grad_()
        m64(x64).backward(dy.double())
        return {"x": x64.grad, **{n: p.grad for n, p in m64.named_parameters()}}
    _module_gradients(lambda: FeedForward(320, glu=True), ref_run, "FeedForward 320", strict=True)


def test_transformer_block_under_checkpoint_against_the_parent_route(route_every_supported_shape):
    """One BasicTransformerBlock(320, 5, 64), bf16, 14 x 3072 tokens: see _module_gradients. The block's residual adds + LayerNorms
    (ops.add_layer_norm) have no HIP backward and are recorded fallbacks under grad, so this run cannot be strict; what is asserted
    instead is that FALLBACKS holds no geglu entry and PROFILE shows ff_geglu + ff_geglu_bwd. The fp64 run goes frame by frame (the
    frames of a batch are independent in a spatial block): one 3072 x 3072 score matrix per head at a time."""
    from sgm.modules.attention import BasicTransformerBlock

    def ref_run(m64, x, dy):
        gx = []
        for f in range(x.shape[0]):
            xf = x[f:f + 1].double().requires_grad_()
            m64(xf).backward(dy[f:f + 1].double())               # parameter gradients accumulate over the frames
            gx.append(xf.grad)
        return {"x": torch.cat(gx), **{n: p.grad for n, p in m64.named_parameters()}}
    _module_gradients(lambda: BasicTransformerBlock(320, 5, 64, checkpoint=False), ref_run, "BasicTransformerBlock 320/5/64", strict=False)


def test_gate_edges():
    """hip_ops.ff_geglu_backward_supported is mvi_ff_geglu_backward_supported, a host-only C function with the forward's gate: K = 320
    yes, 640 no; inner a multiple of 32 from 64; fp32 no. Unsupported arguments to the C entry return the invalid-argument status."""
    _, hip_ops = _ops()
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    assert hip_ops.ff_geglu_backward_supported(320, 1280, bf) and hip_ops.ff_geglu_backward_supported(320, 64, f16)
    assert not hip_ops.ff_geglu_backward_supported(640, 1280, bf) and not hip_ops.ff_geglu_backward_supported(320, 32, bf)
    assert not hip_ops.ff_geglu_backward_supported(320, 80, bf) and not hip_ops.ff_geglu_backward_supported(320, 1280, f32)
    for inner in (64, 160, 1280, 4864):
        assert hip_ops.ff_geglu_backward_supported(320, inner, bf) == hip_ops.ff_geglu_supported(320, inner, bf)
    x = torch.randn(64, 640, device=DEV, dtype=bf)
    w = torch.randn(128, 640, device=DEV, dtype=bf)
    with pytest.raises(Exception, match="ff_geglu backward"):
        hip_ops.ff_geglu_backward(x, w, None, torch.randn(64, 64, device=DEV, dtype=bf))

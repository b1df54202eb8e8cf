"""GPU parity of the differentiable add_layer_norm (csrc/layernorm_bwd.hip through svd/ops.py's _AddLayerNormFn).

Parity chain: the reference's nn.LayerNorm and `+` under fp64 autograd -> the fp64 formula of tests/layernorm_bwd_helpers.py
(tests/test_layernorm_bwd_cpu.py, 1e-12) -> the kernels (here). The formula's input is the forward's rounded residual stream s, as
the kernel's is. Bars: the project's 16-bit gradient bars applied to the reference's OWN error of the SAME case in the same type
(tools/gen_golden_layernorm_bwd.py -> tests/golden/layernorm_bwd/ref_errors.json): rms <= 1.6 x, max norm <= 2.0 x; for the column sums
(dweight, dbias, drow) also a max-norm relative error <= 2^-8 (bf16) / 2^-10 (f16): twice the unit roundoff of the one final rounding
of an fp32 sum, which the reference's own (row-count dependent) error cannot hide. fp32 I/O: 1e-4 of each output's scale.
Every test runs with ops.STRICT = True unless it says otherwise."""
import functools
import os
import sys

import pytest
import torch

import layernorm_bwd_helpers as L
import svd_helpers as H

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multiview_inpaint_amd", "dropin")
if DROPIN not in sys.path:
    sys.path.insert(0, DROPIN)

# The bars of the attention / GroupNorm / GEGLU backward modules (copied, not imported)
RMS_BAR = 1.6
MAX_BAR = 2.0
SUM_CAP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10}
FP32_BAR = 1e-4
DEV = "cuda"
MIB = 1 << 20


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "LAYERNORM_BACKWARD", True)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """ops.add_layer_norm_backward_pays is a speed decision (small problems are left to PyTorch); parity on small shapes is checked
    with the decision lifted, so that what is tested is what the kernels compute."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "add_layer_norm_backward_pays", lambda *a: True)


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


def _assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _case_data(case, tag):
    """(inputs, fp64 truth) of a case, computed once and shared (never modified)."""
    dtype = L.DTYPES.get(tag, torch.float32)
    if case in L.TENSOR_CASES and tag in L.DTYPES:
        return L.load_fixture(case, tag)
    inp = L.make_inputs(case, dtype)
    return inp, L.truth(inp, case)


def _norm(inp, dtype, trainable=True):
    C = inp["w"].numel()
    norm = torch.nn.LayerNorm(C, eps=L.EPS)
    with torch.no_grad():
        norm.weight.copy_(inp["w"].float())
        norm.bias.copy_(inp["b"].float())
    return norm.to(DEV, dtype).requires_grad_(trainable)


def _run(case, inp, dtype, grad=("x", "h", "row", "norm"), shape3=True):
    """ops.add_layer_norm forward + backward on the GPU: dict of outputs (y, s, s_pre) and gradients (dx, dh, drow, dweight, dbias)."""
    ops, _ = _ops()
    R, C = case.R, case.C
    G = case.G if inp["row"] is not None else 0
    B = G if G else 1                                           # x as [B, R / B, C]: the blocks' token layout
    leaf = {}
    for k in ("x", "h"):
        leaf[k] = None if inp[k] is None else inp[k].to(DEV).reshape(B, R // B, C).requires_grad_(k in grad)
    leaf["row"] = None if inp["row"] is None else inp["row"].to(DEV).reshape(G, 1, C).requires_grad_("row" in grad)
    norm = _norm(inp, dtype, "norm" in grad)
    ret_pre = inp["gsp"] is not None
    y, s, s_pre = ops.add_layer_norm(leaf["x"], norm, h=leaf["h"], row=leaf["row"], ret_pre=ret_pre)
    outs, grads = [y], [inp["gy"].to(DEV).reshape(y.shape)]
    if inp["gs"] is not None:
        outs.append(s); grads.append(inp["gs"].to(DEV).reshape(y.shape))
    if ret_pre:
        outs.append(s_pre); grads.append(inp["gsp"].to(DEV).reshape(y.shape))
    torch.autograd.backward(outs, grads)
    g = lambda t: None if t is None or t.grad is None else t.grad
    return dict(y=y.detach(), s=s.detach(), s_pre=None if s_pre is None else s_pre.detach(), dx=g(leaf["x"]), dh=g(leaf["h"]),
                drow=g(leaf["row"]), dweight=norm.weight.grad, dbias=norm.bias.grad), leaf, norm


def _same_bits(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                                            b.view(torch.int16 if b.element_size() == 2 else torch.int32)))


def _check16(name, got, ref, r, key, tag, cap):
    e_max, e_rms = L.errors(got.detach().cpu().reshape(ref.shape), ref)
    r_max, r_rms = r[key + "_max"], r[key + "_rms"]
    H.report(f"{name} {key}: max {e_max:.2e} = {e_max / r_max:.2f} x, rms {e_rms:.2e} = {e_rms / r_rms:.2f} x the reference's own error"
             + (f"; cap {e_max / SUM_CAP[tag]:.2f} x 2^{-8 if tag == 'bf16' else -10}" if cap else ""))
    ok = e_max <= MAX_BAR * r_max and e_rms <= RMS_BAR * r_rms and (not cap or e_max <= SUM_CAP[tag])
    return ok, (name, key, e_max, r_max, e_rms, r_rms)


CASES16 = [(case, tag) for case in L.GPU_CASES for tag in L.DTYPES]


@pytest.mark.parametrize("case,tag", CASES16, ids=[L.case_name(c, t) for c, t in CASES16])
def test_gradients_within_the_reference_own_error(case, tag, route_every_supported_shape):
    """Every op-level case in bf16 and f16, everything requiring grad: each gradient against the fp64 formula (the stored fp64 outputs
    for the tensor fixtures) under the bars of the module docstring; y, s, s_pre bit-identical to the no-grad call; two runs
    bit-identical; x.grad and h.grad equal and not aliased."""
    ops, _ = _ops()
    dtype = L.DTYPES[tag]
    inp, ref = _case_data(case, tag)
    r = L.ref_errors()[L.case_name(case, tag)]
    (out, leaf, norm), kinds = _profiled(lambda: _run(case, inp, dtype))
    assert kinds == ["add_layernorm", "add_layernorm_bwd"], kinds
    with torch.no_grad():
        y0, s0, p0 = ops.add_layer_norm(leaf["x"], norm, h=leaf["h"], row=leaf["row"], ret_pre=inp["gsp"] is not None)
    assert _same_bits(out["y"], y0) and _same_bits(out["s"], s0) and _same_bits(out["s_pre"], p0)
    again, _, _ = _run(case, inp, dtype)
    for k in ("dx", "dh", "drow", "dweight", "dbias"):
        assert _same_bits(out[k], again[k]), k
    name = L.case_name(case, tag)
    results = [_check16(name, out["dx"], ref["dx"], r, "dx", tag, False)]
    if case.h:
        assert _same_bits(out["dx"], out["dh"]) and out["dx"].data_ptr() != out["dh"].data_ptr()
    results.append(_check16(name, out["dweight"], ref["dweight"], r, "dweight", tag, True))
    results.append(_check16(name, out["dbias"], ref["dbias"], r, "dbias", tag, True))
    if case.G:
        results.append(_check16(name, out["drow"], ref["drow"], r, "drow", tag, True))
    _assert_all(results)


@pytest.mark.parametrize("case", L.FP32_CASES, ids=[c.name for c in L.FP32_CASES])
def test_fp32_io_against_the_fp64_formula(case, route_every_supported_shape):
    inp, ref = _case_data(case, "fp32")
    out, _, _ = _run(case, inp, torch.float32)
    bad = []
    for k in ("dx", "dh", "dweight", "dbias", "drow"):
        e_max, e_rms = L.errors(out[k].cpu().reshape(ref["dx" if k == "dh" else k].shape), ref["dx" if k == "dh" else k])
        H.report(f"{case.name} fp32 {k}: max {e_max:.2e}, rms {e_rms:.2e}")
        if e_max > FP32_BAR:
            bad.append((k, e_max))
    assert not bad, bad


@pytest.mark.parametrize("tag", list(L.DTYPES))
def test_requested_outputs_only(tag, route_every_supported_shape, monkeypatch):
    """999 x 320 with h, row and ret_pre. Frozen norm: no parameter sums are asked of the kernel and the workspace is what drow needs;
    only x requiring grad: no workspace at all; only the norm's parameters (and the row) requiring grad: no gP store. gP, a
    row-local result, is the same bits whatever else is asked for; a column sum is the same bits wherever the blocks own the same slabs
    (with and without the gP store). Without drow the slabs no longer follow the runs of `row`, so the fp32 sum of the same terms is
    taken in another fixed order: it differs by reordering error (about 1e-7 of the sum of magnitudes), and after the one rounding to
    the 16-bit type the two results are equal or adjacent values of that type, which lie within 2^-10 (f16) / 2^-7 (bf16) of each
    other relative to the larger."""
    ops, hip_ops = _ops()
    case, dtype = L.BASE_999, L.DTYPES[tag]
    inp, _ = _case_data(case, tag)
    calls = []
    real = hip_ops.add_layer_norm_backward

    def spy(s, weight, eps, **kw):
        out = real(s, weight, eps, **kw)
        calls.append((kw.get("need_dx", True), kw.get("need_dparams", True), kw.get("row_groups"), out))
        return out
    monkeypatch.setattr(hip_ops, "add_layer_norm_backward", spy)
    full, _, _ = _run(case, inp, dtype)
    frozen, _, _ = _run(case, inp, dtype, grad=("x", "h", "row"))
    only_x, _, _ = _run(case, inp, dtype, grad=("x",))
    params, _, _ = _run(case, inp, dtype, grad=("norm",))
    row_params, _, _ = _run(case, inp, dtype, grad=("row", "norm"))
    assert [c[:3] for c in calls] == [(True, True, case.G), (True, False, case.G), (True, False, None), (False, True, None),
                                      (False, True, case.G)], [c[:3] for c in calls]
    assert calls[4][3][0] is None
    assert calls[1][3][1] is None and calls[1][3][2] is None and calls[3][3][0] is None and calls[2][3][3] is None
    row_div = case.R // case.G
    ws = hip_ops.add_layer_norm_backward_workspace_bytes
    assert ws(case.R, case.C, row_div, False, False) == 0
    assert 0 < ws(case.R, case.C, row_div, False, True) < ws(case.R, case.C, row_div, True, True)
    for other in (frozen, only_x):
        assert _same_bits(full["dx"], other["dx"])
    assert _same_bits(full["dh"], frozen["dh"]) and _same_bits(full["drow"], frozen["drow"])
    assert frozen["dweight"] is None and only_x["dh"] is None and only_x["drow"] is None and params["dx"] is None
    assert row_params["dx"] is None and _same_bits(full["drow"], row_params["drow"])
    assert _same_bits(full["dweight"], row_params["dweight"]) and _same_bits(full["dbias"], row_params["dbias"])
    adjacent = 2.0 ** (-10 if tag == "f16" else -7)
    for k in ("dweight", "dbias"):
        a, b = full[k].double(), params[k].double()
        assert bool(((a - b).abs() <= adjacent * torch.maximum(a.abs(), b.abs())).all()), k


def test_memory_held_between_forward_and_backward(route_every_supported_shape):
    """A condition, not a measurement, at 14 x 3072 x 320 bf16 with h, row and ret_pre: after the forward the HIP route holds its three
    outputs and at most 1 MiB more (the PyTorch route holds more: printed); the backward's peak above its entry is at most one
    gradient tensor + the workspace + 1 MiB."""
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    B, S, C = 14, 3072, 320
    g = torch.Generator(device=DEV).manual_seed(5)
    x, h, gy, gs, gp = (torch.randn(B, S, C, device=DEV, generator=g).to(dt) for _ in range(5))
    row = torch.randn(B, 1, C, device=DEV, generator=g).to(dt)
    norm = torch.nn.LayerNorm(C).to(DEV, dt)
    tensor = B * S * C * x.element_size()
    ws = hip_ops.add_layer_norm_backward_workspace_bytes(B * S, C, S, True, True)
    with torch.no_grad():                                        # the fp32 copies of the parameters and the scratch exist before anything is measured
        ops.add_layer_norm(x, norm, h=h, row=row, ret_pre=True)
    hip_ops._workspace(x.device, ws)

    def held(on):
        ops.LAYERNORM_BACKWARD, ops.STRICT = on, on              # (restored by the module's fixture)
        xa, ha, ra = x.clone().requires_grad_(), h.clone().requires_grad_(), row.clone().requires_grad_()
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        outs = ops.add_layer_norm(xa, norm, h=ha, row=ra, ret_pre=True)
        torch.cuda.synchronize()
        m1 = torch.cuda.memory_allocated()
        peaks = []
        if on:
            real = hip_ops.add_layer_norm_backward

            def watched(*a, **kw):
                torch.cuda.synchronize()
                e0 = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                out = real(*a, **kw)
                torch.cuda.synchronize()
                peaks.append(torch.cuda.max_memory_allocated() - e0)
                return out
            hip_ops.add_layer_norm_backward = watched
        try:
            torch.autograd.backward(list(outs), [gy, gs, gp])
        finally:
            if on:
                hip_ops.add_layer_norm_backward = real
        torch.cuda.synchronize()
        return m1 - m0, peaks
    norm.weight.grad = torch.zeros_like(norm.weight)
    norm.bias.grad = torch.zeros_like(norm.bias)
    hip_fwd, peaks = held(True)
    lib_fwd, _ = held(False)
    ops.LAYERNORM_BACKWARD, ops.STRICT = True, True
    H.report(f"add_layer_norm bf16 {B} x {S} x {C}: held after forward HIP {hip_fwd / MIB:.1f} MiB, PyTorch {lib_fwd / MIB:.1f} MiB (one tensor "
             f"{tensor / MIB:.1f}); backward peak above its entry {peaks[0] / MIB:.1f} MiB (workspace {ws / MIB:.2f})")
    assert hip_fwd <= 3 * tensor + MIB, (hip_fwd, tensor)
    assert len(peaks) == 1 and peaks[0] <= tensor + ws + MIB, (peaks, tensor, ws)


def test_routing_and_strict_mode(route_every_supported_shape):
    """Under grad in strict mode the call runs on the HIP kernels (PROFILE: add_layernorm, add_layernorm_bwd; no fallback recorded);
    with LAYERNORM_BACKWARD off strict mode raises as before this feature and non-strict mode records ("add_layer_norm", "requires
    grad"); under no_grad, or with nothing requiring grad, the Function is not entered; an unsupported width takes the PyTorch
    branch as before."""
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    x = torch.randn(2, 512, 320, device=DEV, dtype=dt)
    h = torch.randn(2, 512, 320, device=DEV, dtype=dt)
    row = torch.randn(2, 1, 320, device=DEV, dtype=dt)
    norm = torch.nn.LayerNorm(320).to(DEV, dt)
    del ops.FALLBACKS[:]

    def under_grad():
        xa = x.clone().requires_grad_()
        y, s, p = ops.add_layer_norm(xa, norm, h=h, row=row, ret_pre=True)
        (y.float().sum() + s.float().sum() + p.float().sum()).backward()
        return xa, y
    (xa, y), kinds = _profiled(under_grad)
    assert kinds == ["add_layernorm", "add_layernorm_bwd"], kinds
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_AddLayerNormFn"), y.grad_fn
    assert xa.grad is not None and xa.grad.shape == x.shape and norm.weight.grad is not None
    assert not [f for f in ops.FALLBACKS if f[0] == "add_layer_norm"], ops.FALLBACKS

    def inference():
        with torch.no_grad():
            a = ops.add_layer_norm(xa, norm, h=h, row=row)[0]
        norm.requires_grad_(False)
        b = ops.add_layer_norm(x, norm, h=h, row=row)[0]         # grad mode on, nothing requires grad
        norm.requires_grad_(True)
        return a, b
    (a, b), kinds = _profiled(inference)
    assert kinds == ["add_layernorm", "add_layernorm"] and a.grad_fn is None and b.grad_fn is None, kinds

    # an unsupported width under grad: the PyTorch branch, a recorded "requires grad" fallback (strict mode raises)
    x20 = torch.randn(2, 8, 20, device=DEV, dtype=dt, requires_grad=True)
    n20 = torch.nn.LayerNorm(20).to(DEV, dt)
    assert not hip_ops.add_layer_norm_backward_supported(20, dt)
    with pytest.raises(ops.HipPathError):
        ops.add_layer_norm(x20, n20)
    ops.STRICT = False                                           # (restored by the module's fixture)
    _, kinds = _profiled(lambda: ops.add_layer_norm(x20, n20)[0])
    assert not kinds and ("add_layer_norm", "requires grad") in ops.FALLBACKS
    # the switch off: the parent's routing
    ops.STRICT, ops.LAYERNORM_BACKWARD = True, False
    with pytest.raises(ops.HipPathError):
        ops.add_layer_norm(x.clone().requires_grad_(), norm, h=h, row=row)
    ops.STRICT = False
    del ops.FALLBACKS[:]
    _, kinds = _profiled(lambda: ops.add_layer_norm(x.clone().requires_grad_(), norm, h=h, row=row)[0].float().sum().backward())
    assert ("add_layer_norm", "requires grad") in ops.FALLBACKS and "add_layernorm_bwd" not in kinds and "add_layernorm" not in kinds, (ops.FALLBACKS, kinds)


def test_gate_edges():
    """hip_ops.add_layer_norm_backward_supported is mvi_add_layernorm_backward_supported, a host-only C function with the forward's
    gate."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    lib = _lib.lib()
    for code, dt in ((0, torch.float32), (1, torch.bfloat16), (2, torch.float16)):
        for C in (8, 20, 40, 64, 96, 320, 640, 1280, 4096, 4104):
            assert hip_ops.add_layer_norm_backward_supported(C, dt) == bool(lib.mvi_add_layernorm_backward_supported(C, code)), (C, dt)
            assert hip_ops.add_layer_norm_backward_supported(C, dt) == hip_ops.layernorm_supported(C, dt), (C, dt)
    assert hip_ops.add_layer_norm_backward_supported(4096, torch.bfloat16) and not hip_ops.add_layer_norm_backward_supported(4096, torch.float32)
    assert not hip_ops.add_layer_norm_backward_supported(320, torch.float64)


def _module_gradients(make, run, inputs, tag_name, n_bwd, strict):
    """Shared by the two module tests. `make()` builds the module; run(module, inputs) -> dict of gradients. Truth: the fp64 CPU module;
    the new route is held to 1.6 x / 2.0 x the parent route's own error (LAYERNORM_BACKWARD off) per tensor."""
    ops, _ = _ops()
    dt = torch.bfloat16
    torch.manual_seed(29)
    m64 = make().double()
    with torch.no_grad():                                        # weights representable in bf16 on both sides
        for p in m64.parameters():
            p.copy_(p.to(dt).double())
    ref = run(m64, {k: v.double() for k, v in inputs.items()})

    def gpu_run():
        m = make()
        m.load_state_dict({k: v.float() for k, v in m64.state_dict().items()})
        m = m.to(DEV, dt)
        del ops.FALLBACKS[:]
        grads, kinds = _profiled(lambda: run(m, {k: v.to(DEV) for k, v in inputs.items()}))
        return grads, kinds, list(ops.FALLBACKS)
    ops.STRICT = strict
    new, kinds, fallbacks = gpu_run()
    assert not [f for f in fallbacks if f[0] == "add_layer_norm"], fallbacks
    assert kinds.count("add_layernorm_bwd") == n_bwd, kinds
    H.report(f"{tag_name}: ops that left the HIP path under grad: {sorted(set(f[0] for f in fallbacks))}")
    ops.STRICT, ops.LAYERNORM_BACKWARD = False, False            # the parent's route (both restored by the module's fixture)
    old, old_kinds, old_fallbacks = gpu_run()
    ops.STRICT, ops.LAYERNORM_BACKWARD = True, True
    assert ("add_layer_norm", "requires grad") in old_fallbacks and "add_layernorm_bwd" not in old_kinds
    results = []
    for name, r in ref.items():
        assert new[name] is not None, name
        o_max, o_rms = L.errors(old[name].cpu(), r)
        e_max, e_rms = L.errors(new[name].cpu(), r)
        H.report(f"{tag_name} bf16 d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the PyTorch route's own error")
        results.append((e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms, (name, e_max, o_max, e_rms, o_rms)))
    _assert_all(results)


def test_transformer_block_under_checkpoint_against_the_parent_route(route_every_supported_shape):
    """BasicTransformerBlock(320, 5, 64) with a context of ONE token (the collapsed `row` path: norm1 alone, then both inner adds +
    norm3 in one call), bf16, 2 x 1024 tokens, under torch.utils.checkpoint: x and every parameter that takes part get gradients, no
    add_layer_norm fallback, one add_layernorm_bwd per routed norm (2). Not strict: at this size the GEGLU of the FeedForward is below
    its own speed line and takes PyTorch's path (the ops that left the HIP path are printed)."""
    from sgm.modules.attention import BasicTransformerBlock
    from torch.utils.checkpoint import checkpoint
    dt = torch.bfloat16
    torch.manual_seed(31)
    inputs = dict(x=torch.randn(2, 1024, 320).to(dt), ctx=torch.randn(2, 1, 1024).to(dt), dy=torch.randn(2, 1024, 320).to(dt))

    def run(m, t):
        x = t["x"].clone().requires_grad_()
        checkpoint(m, x, t["ctx"], use_reentrant=False).backward(t["dy"])
        grads = {"x": x.grad}
        grads.update({n: p.grad for n, p in m.named_parameters() if p.grad is not None})
        return grads
    _module_gradients(lambda: BasicTransformerBlock(320, 5, 64, context_dim=1024, checkpoint=False), run, inputs,
                      "BasicTransformerBlock 320/5/64, one context token", n_bwd=2, strict=False)


def test_time_mix_block_against_the_parent_route(route_every_supported_shape):
    """VideoTransformerBlock.forward_in_place_layout (T = 2, 256 tokens, ff_in): the entry add_layer_norm carries the frame-index
    embedding as `row` with ret_pre=True, so all three outputs carry gradient; three routed norms."""
    from sgm.modules.video_attention import VideoTransformerBlock
    dt = torch.bfloat16
    torch.manual_seed(37)
    T, S, C = 2, 256, 320
    inputs = dict(h=torch.randn(T, S, C).to(dt), skip=torch.randn(T, S, C).to(dt), emb=(0.5 * torch.randn(T, 1, C)).to(dt),
                  ctx=torch.randn(1, 1, 1024).to(dt), g0=torch.randn(T, S, C).to(dt), g1=torch.randn(T, S, C).to(dt),
                  g2=torch.randn(T, S, C).to(dt))

    def run(m, t):
        leaf = {k: t[k].clone().requires_grad_() for k in ("h", "skip", "emb")}
        xs, f, x = m.forward_in_place_layout(leaf["h"], leaf["skip"], leaf["emb"], t["ctx"], T)
        torch.autograd.backward([xs, f, x], [t["g0"], t["g1"], t["g2"]])
        grads = {k: v.grad for k, v in leaf.items()}
        grads.update({n: p.grad for n, p in m.named_parameters() if p.grad is not None})
        return grads
    _module_gradients(lambda: VideoTransformerBlock(C, 5, 64, context_dim=1024, checkpoint=False, timesteps=T, ff_in=True, inner_dim=C),
                      run, inputs, "VideoTransformerBlock 320/5/64 in place, T = 2", n_bwd=3, strict=False)

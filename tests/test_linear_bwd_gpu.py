"""GPU parity of the projections under autograd: the weight / bias gradient kernel (csrc/linear_wgrad.hip), the input gradient on the
forward kernels with the transposed weight (hip_ops.linear_dgrad), ops._LinearFn / ops.linear behind ops.LINEAR_BACKWARD, and one
transformer-block chain.

Oracle: the fp64 formulas of tests/linear_bwd_helpers.py (held to fp64 autograd in tests/test_linear_bwd_cpu.py, 1e-12), evaluated on
this machine's CPU on the rounded inputs. Every test runs with ops.STRICT = True unless it says otherwise, with the switch on, with the
speed decision ops.linear_backward_pays lifted and with the forward's fill-the-chip row thresholds lowered (the tests' row counts are
far below them): what is tested is what the kernels compute."""
import functools

import pytest
import torch
import torch.nn.functional as F

import linear_bwd_helpers as B
import svd_helpers as H_

pytestmark = pytest.mark.gpu

DEV = "cuda"
RMS_BAR = 1.6                     # the bars of every *_bwd module test here: the new route's error as a multiple of the parent route's
MAX_BAR = 2.0
DGRAD_TOL = {"bf16": 1.0 / 128, "f16": 1.0 / 1024}         # tests/test_unet_ops_gpu.py::test_linear_n320_kernel / test_linear_k320_kernel:
#                                                             max|got - ref| < tol max|ref|

# (rows, K, N); "split": the smallest shape csrc/linear_wgrad.hip splits, taken from its host function at run time
WGRAD_SHAPES = [(300, 128, 320), (1, 64, 64), (257, 320, 960), (513, 1280, 320), (70001, 64, 128), "split"]
DGRAD_SHAPES = [(300, 320, 960), (257, 320, 320), (513, 1280, 320), (300, 640, 1920), (260, 1280, 3840)]
AUTOGRAD_SHAPES = [(2600, 320, 960, True), (2600, 1280, 320, False)]           # (rows, K, N, with bias)
BWD_KINDS = ("linear_wgrad", "linear_dgrad_n320", "linear_dgrad_k320")


def _id(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "LINEAR_BACKWARD", True)
    monkeypatch.setattr(dev_ops, "linear_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "FF_GEGLU_MIN_ROWS", 1)
    monkeypatch.setattr(dev_ops, "N320_GROUP_MIN_BLOCKS", 1)


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
    """The smallest (by rows) shape with K = N = 64 for which mvi_linear_wgrad_workspace_bytes > 0."""
    _, hip_ops = _ops()
    for rows in range(1, 1025):
        if hip_ops.linear_wgrad_workspace_bytes(rows, 64, 64) > 0:
            return (rows, 64, 64)
    raise AssertionError("no small shape is split")


def _resolve(shape):
    return _smallest_split_shape() if shape == "split" else shape


@functools.lru_cache(maxsize=None)
def _case(shape, tag, strided=False):
    """Inputs, the fp64 references and the error caps, computed once per (shape, dtype, layout) and left unchanged."""
    rows, K, N = shape
    x, dy, w, b = B.make_rows(rows, K, N, B.DTYPES[tag], seed=sum(shape) + 1000 * strided, strided=strided)
    cap_w, cap_b = B.wgrad_caps(x, dy)
    return dict(x=x, dy=dy, w=w, b=b, dw=B.dweight_formula(x, dy), db=B.dbias_formula(dy), cap_w=cap_w, cap_b=cap_b)


def _gpu_view(t):
    """t on the GPU with t's own strides (a column range of a wider matrix stays one)."""
    if t.is_contiguous():
        return t.to(DEV)
    base = torch.empty(t.untyped_storage().nbytes() // t.element_size(), dtype=t.dtype)
    base.set_(t.untyped_storage(), 0, base.shape)
    return base.to(DEV).as_strided(t.shape, t.stride(), t.storage_offset())


def test_the_shape_list_holds_a_split_and_an_unsplit_shape():
    _, hip_ops = _ops()
    ws = [hip_ops.linear_wgrad_workspace_bytes(*_resolve(s)) for s in WGRAD_SHAPES]
    H_.report(f"linear_wgrad workspace bytes per shape: {dict(zip(map(_id, WGRAD_SHAPES), ws))}; smallest split shape {_smallest_split_shape()}")
    assert any(b > 0 for b in ws) and any(b == 0 for b in ws), ws
    assert ws[-1] > 0
    # S N K 4 + S N 4 for a whole number of slices S >= 2
    for s, b in zip(WGRAD_SHAPES, ws):
        rows, K, N = _resolve(s)
        assert b % ((N * K + N) * 4) == 0 and b // ((N * K + N) * 4) != 1, (s, b)
    # a pure function of the shape
    assert ws == [hip_ops.linear_wgrad_workspace_bytes(*_resolve(s)) for s in WGRAD_SHAPES]


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_id)
def test_wgrad_kernel_against_the_fp64_formula(shape, tag, strided):
    """hip_ops.linear_wgrad against the fp64 formulas. Elementwise |dweight - ref| <= 2 rows 2^-24 dweight(|x|, |dy|) and
    |dbias - ref| <= 2 rows 2^-24 sum|dy|: the worst case of any fp32 summation order of exactly representable products, doubled for
    the matrix pipe's internal accumulation; two calls bit-identical; the unsplit launch (workspace withheld) inside the same caps;
    dweight the same bits with and without dbias. strided: x the first K columns of a [rows, K + 64] matrix, dy the middle third of
    a [rows, 3 N] one, read in place."""
    _, hip_ops = _ops()
    shape = _resolve(shape)
    rows, K, N = shape
    c = _case(shape, tag, strided)
    assert hip_ops.linear_wgrad_supported(K, N, B.DTYPES[tag])
    xd, dyd = _gpu_view(c["x"]), _gpu_view(c["dy"])
    assert xd.stride() == c["x"].stride() and dyd.stride() == c["dy"].stride() and torch.equal(dyd.cpu(), c["dy"])
    (dw, db), kinds = _profiled(lambda: hip_ops.linear_wgrad(xd, dyd, True))
    assert kinds == ["linear_wgrad"], kinds
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (N, K) and db.dtype == torch.float32 and tuple(db.shape) == (N,)
    dw2, db2 = hip_ops.linear_wgrad(xd, dyd, True)
    dw_u, db_u = hip_ops.linear_wgrad(xd, dyd, True, split=False)
    dw_nb, none = hip_ops.linear_wgrad(xd, dyd, False)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs must give the same bits"
    assert none is None and torch.equal(dw_nb, dw)
    name = f"linear_wgrad {_id(shape)} {tag}{' strided' if strided else ''}"
    for what, gw, gb in (("", dw, db), (" unsplit", dw_u, db_u)):
        d_w = (gw.double().cpu() - c["dw"]).abs()
        d_b = (gb.double().cpu() - c["db"]).abs()
        r_w = (d_w / c["cap_w"]).max().item()
        r_b = (d_b / c["cap_b"]).max().item()
        H_.report(f"{name}{what}: dweight {r_w:.4f}, dbias {r_b:.4f} of the elementwise cap")
        assert (d_w <= c["cap_w"]).all(), (name + what, r_w)
        assert (d_b <= c["cap_b"]).all(), (name + what, r_b)


def test_wgrad_of_no_rows_is_zero():
    _, hip_ops = _ops()
    for dt in B.DTYPES.values():
        x = torch.empty(0, 128, dtype=dt, device=DEV)
        dy = torch.empty(0, 192, dtype=dt, device=DEV)
        dw, db = hip_ops.linear_wgrad(x, dy, True)
        torch.cuda.synchronize()
        assert tuple(dw.shape) == (192, 128) and not dw.any() and tuple(db.shape) == (192,) and not db.any()


def test_wgrad_gate_edges():
    """K = 96, N = 32, fp32, a misaligned pointer and a short workspace: ..._supported says 0 where it is the shape, and the entry returns
    the invalid-argument status without a launch (the outputs keep their fill)."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    L = _lib.lib()
    bf, f32 = torch.bfloat16, torch.float32
    assert hip_ops.linear_wgrad_supported(64, 64, bf) and hip_ops.linear_wgrad_supported(5120, 1280, torch.float16)
    rows = 200

    def call(x, dy, dw, db, K, N, dt, ws=None, ws_bytes=0, x_off=0):
        return L.mvi_linear_wgrad(x.data_ptr() + x_off, dy.data_ptr(), dw.data_ptr(), db.data_ptr(), rows, K, N, x.stride(0), dy.stride(0),
                                  hip_ops._DT[dt], None if ws is None else ws.data_ptr(), ws_bytes, None)

    for K, N, dt in ((96, 64, bf), (64, 32, bf), (64, 64, f32)):
        assert not hip_ops.linear_wgrad_supported(K, N, dt)
        assert L.mvi_linear_wgrad_supported(K, N, hip_ops._DT[dt]) == 0
        x = torch.randn(rows, K, device=DEV).to(dt)
        dy = torch.randn(rows, N, device=DEV).to(dt)
        dw, db = torch.full((N, K), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)
        assert call(x, dy, dw, db, K, N, dt) == -1               # MVI_EINVAL
        with pytest.raises(Exception, match="linear wgrad"):
            hip_ops.linear_wgrad(x, dy, True)
        torch.cuda.synchronize()
        assert (dw == 7).all() and (db == 7).all()
    K = N = 64
    x = torch.randn(rows + 1, K, device=DEV).to(bf)
    dy = torch.randn(rows, N, device=DEV).to(bf)
    dw, db = torch.full((N, K), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)
    assert call(x, dy, dw, db, K, N, bf, x_off=8) == -1          # x 8 bytes off a 16-byte boundary
    need = hip_ops.linear_wgrad_workspace_bytes(rows, K, N)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    assert call(x, dy, dw, db, K, N, bf, ws=ws, ws_bytes=need - 4) == -1
    assert call(x, dy, dw, db, K, N, bf, ws=None, ws_bytes=need) == -1
    torch.cuda.synchronize()
    assert (dw == 7).all() and (db == 7).all() and not ws.any()
    assert call(x, dy, dw, db, K, N, bf, ws=ws, ws_bytes=need) == 0
    torch.cuda.synchronize()
    ref = B.dweight_formula(x[:rows].cpu(), dy.cpu())
    assert (dw.double().cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=_id)
def test_dgrad_on_the_forward_kernels_against_fp64(shape, tag):
    """dx = linear_dgrad(dy, W^T) against fp64 dx at the forward kernels' own bar (max|got - ref| < tol max|ref|, tol 1/128 bf16,
    1/1024 f16); exactly 0 with a zero weight; the same bits as the forward kernel called by hand on weight.t().contiguous()."""
    _, hip_ops = _ops()
    rows, K, N = shape
    c = _case(shape, tag)
    dt = B.DTYPES[tag]
    ref = B.dx_formula(c["dy"], c["w"])
    wt = c["w"].to(DEV).t().contiguous()
    dyd = c["dy"].to(DEV)
    which = hip_ops.linear_dgrad_kernel(K, N, dt)
    assert which in ("n320", "k320"), (shape, which)
    dx, kinds = _profiled(lambda: hip_ops.linear_dgrad(dyd, wt))
    assert kinds == ["linear_dgrad_" + which], kinds
    assert tuple(dx.shape) == (rows, K) and dx.dtype == dt
    err = (dx.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    H_.report(f"linear_dgrad {_id(shape)} {tag} ({which}): max norm {err:.2e} = {err / DGRAD_TOL[tag]:.3f} of the bar")
    assert err < DGRAD_TOL[tag], (shape, tag, err)
    by_hand = (hip_ops.linear_n320 if which == "n320" else hip_ops.linear_k320)(dyd, wt, None)
    assert torch.equal(dx, by_hand)
    zero = hip_ops.linear_dgrad(dyd, torch.zeros_like(wt))
    torch.cuda.synchronize()
    assert not zero.any()


def test_dgrad_raises_where_no_kernel_takes_the_shape():
    _, hip_ops = _ops()
    dy = torch.randn(100, 128, device=DEV).to(torch.bfloat16)
    assert hip_ops.linear_dgrad_kernel(192, 128, torch.bfloat16) is None
    with pytest.raises(ValueError, match="linear_dgrad"):
        hip_ops.linear_dgrad(dy, torch.zeros(192, 128, device=DEV, dtype=torch.bfloat16))


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("rows,K,N,with_bias", AUTOGRAD_SHAPES, ids=["2600x320x960+b", "2600x1280x320"])
def test_ops_linear_under_autograd(rows, K, N, with_bias, tag):
    """ops.linear under autograd: y bit-identical to the no-grad call; weight.grad = linear_wgrad(...).to(dtype), bias.grad and x.grad =
    linear_dgrad(...) bit for bit; _LinearFn holds x and weight only; only the kinds that are asked for run; two backward runs and the
    run under checkpoint(use_reentrant=False) give the same bits."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    c = _case((rows, K, N), tag)
    x, dy = c["x"].to(DEV).reshape(2, rows // 2, K), c["dy"].to(DEV).reshape(2, rows // 2, N)
    w, b = c["w"].to(DEV), (c["b"].to(DEV) if with_bias else None)
    assert ops.linear_gates(rows, K, N, dt)
    fwd = "linear_" + ops._linear_route(rows, K, N, dt)
    dgrad = "linear_dgrad_" + hip_ops.linear_dgrad_kernel(K, N, dt)
    with torch.no_grad():
        y0, kinds = _profiled(lambda: ops.linear(x, w, b))
    assert kinds == [fwd], kinds
    _, kinds = _profiled(lambda: ops.linear(x, w, b))                                # grad mode on, nothing requires grad
    assert kinds == [fwd], kinds

    def leaves(need_x=True, need_p=True):
        return (x.clone().requires_grad_(need_x), w.clone().requires_grad_(need_p), None if b is None else b.clone().requires_grad_(need_p))

    xa, wa, ba = leaves()
    y, kinds = _profiled(lambda: ops.linear(xa, wa, ba))
    assert kinds == [fwd] and torch.equal(y.detach(), y0)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == xa.data_ptr() and saved[1].data_ptr() == wa.data_ptr()
    _, kinds = _profiled(lambda: y.backward(dy))
    assert sorted(kinds) == sorted([dgrad, "linear_wgrad"]), kinds

    dw, db = hip_ops.linear_wgrad(x, dy, with_bias)
    assert wa.grad.dtype == dt and torch.equal(wa.grad, dw.to(dt))
    if with_bias:
        assert ba.grad.dtype == dt and torch.equal(ba.grad, db.to(dt))
    assert torch.equal(xa.grad, hip_ops.linear_dgrad(dy, w.t().contiguous()))
    # within one rounding of fp64 (plus the kernel's accumulation, far below it)
    e_w = B.errors(wa.grad.cpu(), c["dw"])[0]
    e_x = B.errors(xa.grad.reshape(rows, K).cpu(), B.dx_formula(c["dy"], c["w"]))[0]
    H_.report(f"ops.linear {rows}x{K}x{N} {tag}: dweight max norm {e_w:.2e}, dx max norm {e_x:.2e} (bar {DGRAD_TOL[tag]:.2e})")
    assert e_w < DGRAD_TOL[tag] and e_x < DGRAD_TOL[tag]

    xo, wo, bo = leaves(need_p=False)
    _, kinds = _profiled(lambda: ops.linear(xo, wo, bo).backward(dy))
    assert kinds == [fwd, dgrad], kinds
    assert torch.equal(xo.grad, xa.grad), "dx must not depend on whether the parameters require grad"
    xp, wp, bp = leaves(need_x=False)
    _, kinds = _profiled(lambda: ops.linear(xp, wp, bp).backward(dy))
    assert kinds == [fwd, "linear_wgrad"], kinds
    assert torch.equal(wp.grad, wa.grad) and (b is None or torch.equal(bp.grad, ba.grad))

    x2, w2, b2 = leaves()
    ops.linear(x2, w2, b2).backward(dy)
    assert torch.equal(x2.grad, xa.grad) and torch.equal(w2.grad, wa.grad) and (b is None or torch.equal(b2.grad, ba.grad))
    xc, wc, bc = leaves()
    _, kinds = _profiled(lambda: checkpoint(ops.linear, xc, wc, bc, use_reentrant=False).backward(dy))
    assert kinds.count(fwd) in (1, 2) and kinds.count(dgrad) == 1 and kinds.count("linear_wgrad") == 1, kinds
    assert torch.equal(xc.grad, xa.grad) and torch.equal(wc.grad, wa.grad) and (b is None or torch.equal(bc.grad, ba.grad))


def test_frozen_weight_takes_its_transposed_copy_from_the_derived_table():
    """A frozen weight's W^T is kept in svd/derived.py's table (one build for two backward runs) and rebuilt after an in-place update;
    a weight that trains is transposed from the live tensor and leaves no entry."""
    from multiview_inpaint_amd.svd import derived
    ops, hip_ops = _ops()
    rows, K, N = 2600, 320, 960
    c = _case((rows, K, N), "bf16")
    x, dy, w = c["x"].to(DEV), c["dy"].to(DEV), c["w"].to(DEV).clone()
    key = ("linear_transposed", id(w))
    assert key not in derived._table

    def dx_of():
        xa = x.clone().requires_grad_()
        ops.linear(xa, w).backward(dy)
        return xa.grad
    g1 = dx_of()
    e1 = derived._table[key][2]
    assert torch.equal(e1, w.t()) and e1.is_contiguous()
    g2 = dx_of()
    assert derived._table[key][2] is e1 and torch.equal(g1, g2)
    w.mul_(2)
    g3 = dx_of()
    e3 = derived._table[key][2]
    assert e3 is not e1 and torch.equal(e3, w.t())
    assert torch.equal(g3, hip_ops.linear_dgrad(dy, w.t().contiguous())) and not torch.equal(g3, g1)
    wt = w.clone().requires_grad_()
    ops.linear(x.clone().requires_grad_(), wt).backward(dy)
    assert ("linear_transposed", id(wt)) not in derived._table


def test_switch_off_is_the_f_linear_route():
    """ops.LINEAR_BACKWARD off (the default): output and gradients equal F.linear's bit for bit, and no linear_wgrad / linear_dgrad_* kind
    is launched."""
    ops, hip_ops = _ops()
    ops.LINEAR_BACKWARD = False                                      # (restored by the module's fixture)
    rows, K, N = 2600, 320, 960
    c = _case((rows, K, N), "bf16")
    x, dy, w, b = (c[k].to(DEV) for k in ("x", "dy", "w", "b"))

    def run(fn):
        xa, wa, ba = (t.clone().requires_grad_() for t in (x, w, b))
        y = fn(xa, wa, ba)
        y.backward(dy)
        return y.detach(), xa.grad, wa.grad, ba.grad
    got, kinds = _profiled(lambda: run(ops.linear))
    assert not [k for k in kinds if k in BWD_KINDS or k.startswith("linear_")], kinds
    for g, r in zip(got, run(F.linear)):
        assert torch.equal(g, r)


def _block_chain(ops, x, h, norm, w_qkv, w_out, b_out, heads):
    """add_layer_norm -> linear(qkv) -> attention_packed -> linear(to_out): the self-attention layer of a BasicTransformerBlock."""
    y, _, _ = ops.add_layer_norm(x, norm, h=h)
    qkv = ops.linear(y, w_qkv)
    a = ops.attention_packed(qkv, heads)
    return ops.linear(a, w_out, b_out)


def test_transformer_block_chain_against_the_switch_off_route(monkeypatch):
    """add_layer_norm -> linear(qkv) -> attention_packed -> linear(to_out) at 320 channels, 5 heads, 2 x 1024 tokens,
    bf16, with the existing LayerNorm and attention backward routes on: gradients of the two inputs and the five parameters against the
    fp64 CPU evaluation of the same chain. Yardstick: the same chain with ops.LINEAR_BACKWARD off (F.linear under autograd) against the
    same fp64 result; the new route's error per tensor is at most 1.6 x (rms) / 2.0 x (max) of it. ops.STRICT = False for both
    (attention_packed under grad records its unpacking). The new route launches two linear_wgrad and two linear_dgrad_*; the parent none."""
    ops, hip_ops = _ops()
    monkeypatch.setattr(ops, "attention_backward_pays", lambda *a: True)
    monkeypatch.setattr(ops, "add_layer_norm_backward_pays", lambda *a: True)
    ops.STRICT = False                                               # (restored by the module's fixture)
    dt, C, heads, Bn, S = torch.bfloat16, 320, 5, 2, 1024
    g = torch.Generator().manual_seed(31)
    x = torch.randn(Bn, S, C, generator=g).to(dt)
    h = torch.randn(Bn, S, C, generator=g).to(dt)
    dy = torch.randn(Bn, S, C, generator=g).to(dt)
    par = {"ln_w": (1.0 + 0.1 * torch.randn(C, generator=g)).to(dt), "ln_b": (0.1 * torch.randn(C, generator=g)).to(dt),
           "w_qkv": (torch.randn(3 * C, C, generator=g) * C ** -0.5).to(dt), "w_out": (torch.randn(C, C, generator=g) * C ** -0.5).to(dt),
           "b_out": (0.3 * torch.randn(C, generator=g)).to(dt)}

    def run(device, dtype):
        leaf = {k: v.to(device, dtype).clone().requires_grad_() for k, v in dict(par, x=x, h=h).items()}
        norm = torch.nn.LayerNorm(C).to(device, dtype)
        norm.weight, norm.bias = torch.nn.Parameter(leaf["ln_w"]), torch.nn.Parameter(leaf["ln_b"])
        leaf["ln_w"], leaf["ln_b"] = norm.weight, norm.bias
        out = _block_chain(ops, leaf["x"], leaf["h"], norm, leaf["w_qkv"], leaf["w_out"], leaf["b_out"], heads)
        out.backward(dy.to(device, dtype))
        return {k: v.grad for k, v in leaf.items()}

    ref = run("cpu", torch.float64)
    del ops.FALLBACKS[:]
    new, kinds = _profiled(lambda: run(DEV, dt))
    assert kinds.count("linear_wgrad") == 2 and sum(k.startswith("linear_dgrad_") for k in kinds) == 2, kinds
    assert not [f for f in ops.FALLBACKS if f[0] in ("attention", "add_layer_norm")], ops.FALLBACKS      # their HIP backward routes ran
    ops.LINEAR_BACKWARD = False
    old, old_kinds = _profiled(lambda: run(DEV, dt))
    ops.LINEAR_BACKWARD = True
    assert not [k for k in old_kinds if k in BWD_KINDS], old_kinds
    bad = []
    for name in ref:
        o_max, o_rms = B.errors(old[name].cpu(), ref[name])
        e_max, e_rms = B.errors(new[name].cpu(), ref[name])
        H_.report(f"block chain 320 2x1024 bf16 d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the switch-off route's own error")
        if not (e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms):
            bad.append((name, e_max, o_max, e_rms, o_rms))
    assert not bad, bad

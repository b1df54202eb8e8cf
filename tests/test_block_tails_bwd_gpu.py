"""GPU parity of the block tails under autograd: the kernels of csrc/block_tails_bwd.hip called directly (hip_ops.planes_tail_backward,
hip_ops.rows_tail_backward), the Functions behind ops.tokens_to_planes_add / tokens_blend_to_planes / add_lerp / planes_to_tokens with
ops.BLOCK_TAILS_BACKWARD on, and one VideoResBlock that no longer leaves the HIP path.

Oracle: the fp64 formulas of tests/block_tails_bwd_helpers.py (held to fp64 autograd in tests/test_block_tails_bwd_cpu.py, 1e-12),
evaluated on this machine's CPU on the rounded 16-bit inputs. The scaled copies are held BIT FOR BIT to the fp32 expression rounded
once; the sums elementwise to 2 n 2^-24 sum|terms| (n terms, any fp32 order; the form of tests/test_linear_bwd_gpu.py). Every test
runs with ops.STRICT = True unless it says otherwise, and with the speed decision ops.block_tails_backward_pays lifted where it routes
through ops: what is tested is what the kernels compute. Every test calls a symbol the parent commit lacks."""
import pytest
import torch

import block_tails_bwd_helpers as B
import svd_helpers as H_

pytestmark = pytest.mark.gpu

DEV = "cuda"
RMS_BAR = 1.6                     # the bars of every *_bwd module test here: the new route's error as a multiple of the parent route's
MAX_BAR = 2.0
# (N, C, S); the last: the smallest image class whose blocks walk two pixel tiles (34 tiles, the last ragged; ragged channel tile)
PLANES_SHAPES = [(1, 8, 8), (3, 64, 72), (2, 72, 64), (3, 320, 200), (6, 128, 64), (1, 72, 2120)]
ROWS_SHAPES = [(1, 1, 8), (3, 37, 64), (2, 64, 320), (6, 144, 1280)]                          # (G, row_div, C)
TAIL_KINDS = ("planes_tail_bwd", "rows_tail_bwd", "tails_reduce")


def _id(s):
    return "x".join(map(str, s))


def _ops():
    from multiview_inpaint_amd.svd import hip_ops, ops
    return ops, hip_ops


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import layers, ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "BLOCK_TAILS_BACKWARD", True)
    monkeypatch.setattr(layers, "TIME_STACK_CONV_BWD", layers.TIME_STACK_CONV_BWD)       # (tests set them; restored here)
    monkeypatch.setattr(layers, "RESBLOCK_CONV_BWD", layers.RESBLOCK_CONV_BWD)


@pytest.fixture()
def route_every_supported_shape(monkeypatch):
    """The speed decisions are lifted (the test shapes are a few blocks; the kernels compute them all the same)."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "block_tails_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "conv3t_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "conv3x3_backward_pays", lambda *a: True)
    monkeypatch.setattr(dev_ops, "CONV3T_MIN_BLOCKS", 0)
    monkeypatch.setattr(dev_ops, "CONV3X3_MIN_BLOCKS", 0)
    monkeypatch.setattr(dev_ops, "group_norm_backward_pays", lambda *a, **k: True)
    monkeypatch.setattr(dev_ops, "group_norm_tok2tok_backward_pays", lambda *a, **k: True)


def _profiled(fn):
    _, hip_ops = _ops()
    hip_ops.PROFILE = []
    try:
        out = fn()
        kinds = [p[0] for p in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = None
    return out, kinds


def _bits(a, b):
    """Same bits (signed zeros included) of two 16-bit or fp32 tensors, the second possibly on the CPU."""
    if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(it).cpu(), b.contiguous().view(it).cpu())


def _frac(got, ref, cap):
    """max over elements of |got - ref| / cap (0 where the cap is 0 and the values agree)."""
    d = (got.double().cpu() - ref).abs()
    assert bool((d[cap == 0] == 0).all())
    return (d[cap > 0] / cap[cap > 0]).max().item() if bool((cap > 0).any()) else 0.0


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("shape", PLANES_SHAPES, ids=_id)
def test_planes_kernel_against_fp64(shape, tag):
    """hip_ops.planes_tail_backward, modes A and B, with and without tok, each output switched off in turn. d_tok and d_base: bit for
    bit ((1 - a32) * dy.float()).to(dtype) transposed, resp. the transposition itself; dbias and dalpha inside 2 n 2^-24 sum|terms|.
    Two calls identical; dbias has the same bits whether or not dalpha is asked for; only the asked-for kinds are launched."""
    _, hip_ops = _ops()
    N, C, S = shape
    dt = B.DTYPES[tag]
    dy, tok, base, bias, alpha = B.make_planes(N, C, S, dt, seed=7)
    assert hip_ops.block_tails_backward_supported(C, S, dt)
    dyd, tokd, biasd, ad = dy.to(DEV), tok.to(DEV), bias.to(DEV), alpha.to(DEV)
    dyt = dy.transpose(1, 2).contiguous()
    name = f"planes_tail_backward {_id(shape)} {tag}"
    # mode A
    fa = B.planes_formulas(dy)
    (d_tok, d_base, dbias, dalpha), kinds = _profiled(lambda: hip_ops.planes_tail_backward(dyd, need_dtok=True, need_dbias=True))
    assert kinds == ["planes_tail_bwd", "tails_reduce"], kinds
    assert d_base is None and dalpha is None and dbias.dtype == torch.float32 and tuple(dbias.shape) == (C,)
    assert _bits(d_tok, dyt)
    fr_a = _frac(dbias, fa["dbias"], B.dbias_cap(dy))
    (only_tok, _, none_b, _), kinds = _profiled(lambda: hip_ops.planes_tail_backward(dyd, need_dtok=True, need_dbias=False))
    assert kinds == ["planes_tail_bwd"] and none_b is None and _bits(only_tok, dyt), kinds
    none_t, _, only_b, _ = hip_ops.planes_tail_backward(dyd, need_dtok=False, need_dbias=True)
    assert none_t is None and _bits(only_b, dbias)
    # mode B
    fb = B.planes_formulas(dy, alpha=alpha, tok=tok, bias=bias)
    want_tok = ((1.0 - alpha).reshape(N, 1, 1) * dyt.float()).to(dt)                 # fp32: one subtraction, one multiply, one rounding
    full = lambda **k: hip_ops.planes_tail_backward(dyd, alpha=ad, tok=tokd, bias=biasd, **{**dict(need_dtok=True, need_dbase=True, need_dbias=True), **k})
    (d_tok, d_base, dbias, dalpha), kinds = _profiled(full)
    assert kinds == ["planes_tail_bwd", "tails_reduce"], kinds
    assert _bits(d_tok, want_tok) and _bits(d_base, dyt)
    assert dalpha.dtype == torch.float32 and tuple(dalpha.shape) == (N,)
    fr_b = _frac(dbias, fb["dbias"], B.dbias_cap(dy, alpha))
    fr_al = _frac(dalpha, fb["dalpha"], B.planes_dalpha_cap(dy, tok, bias))
    again = full()
    assert all(_bits(a, b) for a, b in zip(again, (d_tok, d_base, dbias, dalpha)))
    nb = hip_ops.planes_tail_backward(dyd, alpha=ad, tok=tokd, bias=None, need_dtok=False, need_dbias=False)      # dalpha alone, no bias
    assert nb[0] is None and nb[1] is None and nb[2] is None
    fr_al0 = _frac(nb[3], B.planes_formulas(dy, alpha=alpha, tok=tok)["dalpha"], B.planes_dalpha_cap(dy, tok, None))
    no_tok = hip_ops.planes_tail_backward(dyd, alpha=ad, need_dtok=True, need_dbase=True, need_dbias=True)        # dalpha not asked for
    assert no_tok[3] is None and _bits(no_tok[0], want_tok) and _bits(no_tok[1], dyt) and _bits(no_tok[2], dbias)
    for off in ("need_dtok", "need_dbase", "need_dbias"):
        out = full(**{off: False})
        keep = [(o, w) for o, w, k in zip(out, (d_tok, d_base, dbias), ("need_dtok", "need_dbase", "need_dbias")) if k != off]
        assert out[("need_dtok", "need_dbase", "need_dbias").index(off)] is None and all(_bits(o, w) for o, w in keep) and _bits(out[3], dalpha), off
    (plain, base_only, _, _), kinds = _profiled(lambda: hip_ops.planes_tail_backward(dyd, alpha=ad, need_dtok=False, need_dbase=True))
    assert kinds == ["planes_tail_bwd"] and plain is None and _bits(base_only, dyt), kinds
    H_.report(f"{name}: walk {hip_ops._lib.lib().mvi_planes_tail_backward_walk(S)}, fraction of the cap: dbias A {fr_a:.4f}, dbias B {fr_b:.4f}, "
              f"dalpha {fr_al:.4f}, dalpha without bias {fr_al0:.4f}")
    assert max(fr_a, fr_b, fr_al, fr_al0) <= 1.0, (fr_a, fr_b, fr_al, fr_al0)


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("with_h", [False, True], ids=["x", "x+h"])
@pytest.mark.parametrize("shape", ROWS_SHAPES, ids=_id)
def test_rows_kernel_against_fp64(shape, with_h, tag):
    """hip_ops.rows_tail_backward with and without h: d_t = ((1 - a32) * dy.float()).to(dtype) and d_base = (a32 * dy.float()).to(dtype)
    bit for bit; dalpha against fp64 on t = x + h rounded to the storage type (the forward's own t) inside its cap. Two calls
    identical; outputs switched off cost their launch (no reduce without dalpha)."""
    _, hip_ops = _ops()
    G, row_div, C = shape
    dt = B.DTYPES[tag]
    dy, x, h, base, alpha = B.make_rows(G, row_div, C, dt, seed=9)
    if not with_h:
        h = None
    dev = lambda t: None if t is None else t.to(DEV)
    dyd, xd, hd, based, ad = dev(dy), dev(x), dev(h), dev(base), dev(alpha)
    a = alpha.repeat_interleave(row_div).reshape(-1, 1)
    want_t, want_base = ((1.0 - a) * dy.float()).to(dt), (a * dy.float()).to(dt)
    t = x if h is None else (x.float() + h.float()).to(dt)
    ref = B.rows_formulas(dy, alpha, base=base, t=t)
    (d_t, d_base, dalpha), kinds = _profiled(lambda: hip_ops.rows_tail_backward(dyd, ad, x=xd, h=hd, base=based))
    assert kinds == ["rows_tail_bwd", "tails_reduce"], kinds
    assert _bits(d_t, want_t) and _bits(d_base, want_base)
    assert dalpha.dtype == torch.float32 and tuple(dalpha.shape) == (G,)
    fr = _frac(dalpha, ref["dalpha"], B.rows_dalpha_cap(dy, base, t, G))
    again = hip_ops.rows_tail_backward(dyd, ad, x=xd, h=hd, base=based)
    assert all(_bits(p, q) for p, q in zip(again, (d_t, d_base, dalpha)))
    (t_only, none_b, none_a), kinds = _profiled(lambda: hip_ops.rows_tail_backward(dyd, ad, need_dbase=False))
    assert kinds == ["rows_tail_bwd"] and none_b is None and none_a is None and _bits(t_only, want_t), kinds
    none_t, b_only, a_only = hip_ops.rows_tail_backward(dyd, ad, x=xd, h=hd, base=based, need_dt=False)
    assert none_t is None and _bits(b_only, want_base) and _bits(a_only, dalpha)
    none_t, none_b, a_only = hip_ops.rows_tail_backward(dyd, ad, x=xd, h=hd, base=based, need_dt=False, need_dbase=False)
    assert none_t is None and none_b is None and _bits(a_only, dalpha)
    bpg = hip_ops._lib.lib().mvi_rows_tail_backward_blocks_per_group(row_div, C)
    H_.report(f"rows_tail_backward {_id(shape)} {'x+h' if with_h else 'x'} {tag}: {bpg} block(s) per group, dalpha at {fr:.4f} of its cap")
    assert fr <= 1.0, fr


def test_zero_size_inputs():
    """N = 0, S = 0, R = 0: MVI_OK, nothing is launched, empty outputs of the right shape, zeros where a sum is asked for (the
    wrappers, and the library entries called directly on sentinel-filled sums)."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    L = _lib.lib()
    bf = torch.bfloat16
    some = torch.zeros(64, device=DEV)                                   # a valid, aligned address for pointers that are never read
    for N, C, S in ((0, 64, 72), (3, 64, 0)):
        dy = torch.zeros(N, C, S, device=DEV, dtype=bf)
        tok = torch.zeros(N, S, C, device=DEV, dtype=bf)
        al = torch.rand(N, device=DEV)
        (d_tok, d_base, dbias, dalpha), kinds = _profiled(lambda: hip_ops.planes_tail_backward(dy, alpha=al, tok=tok, need_dtok=True, need_dbase=True,
                                                                                             need_dbias=True))
        assert kinds == [] and tuple(d_tok.shape) == (N, S, C) and tuple(d_base.shape) == (N, S, C)
        assert tuple(dbias.shape) == (C,) and not dbias.any() and tuple(dalpha.shape) == (N,) and not dalpha.any()
        db, da = torch.full((C,), 7.0, device=DEV), torch.full((3,), 7.0, device=DEV)
        assert L.mvi_planes_tail_backward(some.data_ptr(), some.data_ptr(), some.data_ptr(), None, None, hip_ops.TAILS_DBIAS | hip_ops.TAILS_DALPHA,
                                          None, 0, N, C, S, 1, None) == 0
        assert L.mvi_planes_tail_reduce(None, 0, some.data_ptr(), None, db.data_ptr(), da.data_ptr(), N, C, S, None) == 0
        torch.cuda.synchronize()
        assert not db.any() and bool((da[N:] == 7).all()) and not da[:N].any()
    dy = torch.zeros(0, 64, device=DEV, dtype=bf)
    assert L.mvi_rows_tail_backward(some.data_ptr(), some.data_ptr(), some.data_ptr(), None, some.data_ptr(), None, None, hip_ops.TAILS_DALPHA,
                                    None, 0, 0, 64, 5, 1, None) == 0
    assert L.mvi_rows_tail_reduce(None, 0, some.data_ptr(), 0, 64, 5, None) == 0
    torch.cuda.synchronize()
    assert not some.any()
    with pytest.raises(ValueError):                                      # (the wrapper: no alpha, so no groups to split the rows into)
        hip_ops.rows_tail_backward(dy, torch.zeros(0, device=DEV))


def test_gates_decline_before_any_launch():
    """Every gate of the two passes returns the invalid-argument status with the outputs untouched (filled with a sentinel first):
    C % 8, S % 8, fp32, a NULL required pointer, a misaligned pointer, a short workspace, row_div <= 0 or not dividing R, too many blocks."""
    from multiview_inpaint_amd import _lib
    _, hip_ops = _ops()
    L = _lib.lib()
    bf = torch.bfloat16
    N, C, S = 2, 64, 72
    DB, DA = hip_ops.TAILS_DBIAS, hip_ops.TAILS_DALPHA
    dy = torch.randn(N, C, S, device=DEV).to(bf)
    tok = torch.randn(N, S, C, device=DEV).to(bf)
    al = torch.rand(N, device=DEV)
    outs = [torch.full((N, S, C), 7.0, device=DEV, dtype=bf) for _ in range(2)]
    need = hip_ops.planes_tail_backward_workspace_bytes(N, C, S, DB | DA)
    assert need > 0 and hip_ops.planes_tail_backward_workspace_bytes(N, C, S, 0) == 0
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: None if t is None else t.data_ptr() + off

    def planes(dy_=dy, al_=al, tok_=tok, o0=outs[0], o1=outs[1], sums=DB | DA, ws_=ws, wsb=need, n=N, c=C, s=S, dt=1, off=0, ws_off=0):
        return L.mvi_planes_tail_backward(p(dy_, off), p(al_), p(tok_), p(o0), p(o1), sums, p(ws_, ws_off), wsb, n, c, s, dt, None)
    assert not hip_ops.block_tails_backward_supported(60, S, bf) and not hip_ops.block_tails_backward_supported(C, 76, bf)
    assert not hip_ops.block_tails_backward_supported(C, S, torch.float32)
    for kw in (dict(c=60), dict(s=76), dict(dt=0), dict(n=-1), dict(dy_=None), dict(al_=None), dict(tok_=None), dict(off=8), dict(ws_off=4),
               dict(wsb=need - 4), dict(ws_=None), dict(n=1 << 40, sums=0, ws_=None, wsb=0)):
        assert planes(**kw) == -1, kw                                    # MVI_EINVAL
    with pytest.raises(Exception, match="planes_tail_backward"):
        hip_ops.planes_tail_backward(torch.randn(N, 60, S, device=DEV).to(bf), need_dbias=True)
    with pytest.raises(TypeError):
        hip_ops.planes_tail_backward(dy.float())
    db, da = torch.full((C,), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)
    for args in ((p(ws), need, p(al), None, p(db), p(da), N, 60, S), (p(ws), need - 4, p(al), None, p(db), p(da), N, C, S),
                 (None, need, p(al), None, p(db), p(da), N, C, S), (p(ws), need, p(al), None, None, None, N, C, S),
                 (p(ws, 4), need, p(al), None, p(db), p(da), N, C, S)):
        assert L.mvi_planes_tail_reduce(*args, None) == -1, args
    # rows
    R, rd = 3 * 37, 37
    ry = torch.randn(R, C, device=DEV).to(bf)
    ra = torch.rand(3, device=DEV)
    routs = [torch.full((R, C), 7.0, device=DEV, dtype=bf) for _ in range(2)]
    rneed = hip_ops.rows_tail_backward_workspace_bytes(R, C, rd)
    assert rneed == 3 * 4 * L.mvi_rows_tail_backward_blocks_per_group(rd, C)

    def rows(dy_=ry, al_=ra, x_=ry, b_=ry, o0=routs[0], o1=routs[1], sums=DA, ws_=ws, wsb=rneed, r=R, c=C, rd_=rd, dt=1, off=0):
        return L.mvi_rows_tail_backward(p(dy_), p(al_), p(x_), None, p(b_, off), p(o0), p(o1), sums, p(ws_), wsb, r, c, rd_, dt, None)
    for kw in (dict(c=60), dict(dt=0), dict(rd_=0), dict(rd_=-37), dict(rd_=36), dict(dy_=None), dict(al_=None), dict(x_=None), dict(b_=None),
               dict(off=8), dict(wsb=rneed - 4), dict(ws_=None), dict(r=1 << 42, c=8, rd_=1, sums=0, ws_=None, wsb=0)):
        assert rows(**kw) == -1, kw
    for args in ((p(ws), rneed, None, R, C, rd), (p(ws), rneed - 4, p(da), R, C, rd), (p(ws), rneed, p(da), R, C, 36), (None, rneed, p(da), R, C, rd)):
        assert L.mvi_rows_tail_reduce(*args, None) == -1, args
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs + routs + [db, da]) and not ws.any()
    # and the same calls with nothing wrong go through
    assert planes() == 0 and L.mvi_planes_tail_reduce(p(ws), need, p(al), None, p(db), p(da), N, C, S, None) == 0
    torch.cuda.synchronize()
    assert _bits(outs[1], dy.transpose(1, 2).contiguous()) and not bool((db == 7).any())


# ---- through ops, switch on, the speed decision lifted ---------------------------------------------------------------------------
def _saved_sizes(fn):
    """numel of every tensor the graph recorded by fn() saved for backward."""
    sizes = []

    def pack(t):
        sizes.append(t.numel())
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = fn()
    return out, sizes


def _grads(fn, leaves, dy):
    for l in leaves:
        if l is not None:
            l.grad = None
    fn().backward(dy)
    return [None if l is None else l.grad for l in leaves]


@pytest.mark.parametrize("tag", list(B.DTYPES))
def test_ops_tokens_to_planes_add_under_autograd(tag, route_every_supported_shape):
    """ops.tokens_to_planes_add at (3, 320, 10 x 20) with a bias: y bit-identical to the no-grad call; tok.grad, x_in.grad (dy itself)
    and bias.grad bit-equal to the direct launches; kinds: the forward, planes_tail_bwd + tails_reduce — with the bias frozen the
    planes_to_tokens kernel and no reduce; nothing is saved; two backward runs and the run under checkpoint(use_reentrant=False) give
    the same bits."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    N, C, Hh, Ww = 3, 320, 10, 20
    dy, tok, _, bias, _ = (t.to(DEV) for t in B.make_planes(N, C, Hh * Ww, dt, seed=17))
    dy = dy.reshape(N, C, Hh, Ww)
    x_in = torch.randn(N, C, Hh, Ww, device=DEV).to(dt)
    with torch.no_grad():
        y0 = ops.tokens_to_planes_add(tok, x_in, bias)
    leaves = [tok.clone().requires_grad_(), x_in.clone().requires_grad_(), bias.clone().requires_grad_()]
    run = lambda: ops.tokens_to_planes_add(*leaves)
    (y, sizes), kinds_f = _profiled(lambda: _saved_sizes(run))
    assert kinds_f == ["tokens_to_planes_add"] and _bits(y, y0) and sizes == [], (kinds_f, sizes)
    _, kinds_b = _profiled(lambda: y.backward(dy))
    assert kinds_b == ["planes_tail_bwd", "tails_reduce"], kinds_b
    d_tok, _, dbias, _ = hip_ops.planes_tail_backward(dy, need_dtok=True, need_dbias=True)
    g = [l.grad for l in leaves]
    assert _bits(g[0], d_tok) and _bits(g[1], dy) and _bits(g[2], dbias.to(dt)) and g[2].shape == bias.shape
    again = _grads(run, leaves, dy)
    ck = _grads(lambda: checkpoint(ops.tokens_to_planes_add, *leaves, use_reentrant=False), leaves, dy)
    assert all(_bits(a, b) and _bits(c, b) for a, b, c in zip(again, g, ck))
    frozen = [leaves[0], leaves[1], bias]                                             # the bias frozen: no reduce, the plain transposition
    _, kinds = _profiled(lambda: _grads(lambda: ops.tokens_to_planes_add(*frozen), leaves[:2], dy))
    assert kinds == ["tokens_to_planes_add", "planes_to_tokens"] and _bits(leaves[0].grad, d_tok), kinds
    only_bias = [tok, x_in, leaves[2]]
    _, kinds = _profiled(lambda: _grads(lambda: ops.tokens_to_planes_add(*only_bias), leaves[2:], dy))
    assert kinds == ["tokens_to_planes_add", "planes_tail_bwd", "tails_reduce"] and _bits(leaves[2].grad, dbias.to(dt)), kinds


@pytest.mark.parametrize("tag", list(B.DTYPES))
def test_ops_tokens_blend_to_planes_under_autograd(tag, route_every_supported_shape):
    """ops.tokens_blend_to_planes at (6, 128, 8 x 8), alpha fp32 [N] as layers.py passes it: y bit-identical to the no-grad call, every
    gradient bit-equal to the direct launch (dalpha in alpha's shape and dtype); alpha and bias frozen: one planes_tail_bwd, no
    reduce, and nothing tensor-sized is saved (alpha alone); with alpha trainable tok and bias are saved; repeatable, also under
    checkpoint(use_reentrant=False)."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    N, C, Hh, Ww = 6, 128, 8, 8
    dy, tok, base, bias, alpha = (t.to(DEV) for t in B.make_planes(N, C, Hh * Ww, dt, seed=19))
    dy4 = dy.reshape(N, C, Hh, Ww)
    with torch.no_grad():
        y0 = ops.tokens_blend_to_planes(tok, base, bias, alpha, (Hh, Ww))
    leaves = [t.clone().requires_grad_() for t in (tok, base, bias, alpha)]
    run = lambda: ops.tokens_blend_to_planes(*leaves, (Hh, Ww))
    (y, sizes), kinds_f = _profiled(lambda: _saved_sizes(run))
    assert kinds_f == ["tokens_blend_to_planes"] and _bits(y, y0) and tuple(y.shape) == (N, C, Hh, Ww), kinds_f
    assert sorted(sizes) == sorted([N, tok.numel(), C]), sizes
    _, kinds_b = _profiled(lambda: y.backward(dy4))
    assert kinds_b == ["planes_tail_bwd", "tails_reduce"], kinds_b
    d_tok, d_base, dbias, dalpha = hip_ops.planes_tail_backward(dy, alpha=alpha, tok=tok, bias=bias, need_dtok=True, need_dbase=True, need_dbias=True)
    g = [l.grad for l in leaves]
    assert _bits(g[0], d_tok) and _bits(g[1], d_base) and _bits(g[2], dbias.to(dt)) and _bits(g[3], dalpha)
    assert g[3].dtype == torch.float32 and g[3].shape == alpha.shape
    again = _grads(run, leaves, dy4)
    ck = _grads(lambda: checkpoint(lambda *a: ops.tokens_blend_to_planes(*a, (Hh, Ww)), *leaves, use_reentrant=False), leaves, dy4)
    assert all(_bits(a, b) and _bits(c, b) for a, b, c in zip(again, g, ck))
    frozen = [leaves[0], leaves[1], bias, alpha]
    (_, sizes), _ = _profiled(lambda: _saved_sizes(lambda: ops.tokens_blend_to_planes(*frozen, (Hh, Ww))))
    assert sizes == [N], sizes                                                        # alpha alone: no activation is held
    _, kinds = _profiled(lambda: _grads(lambda: ops.tokens_blend_to_planes(*frozen, (Hh, Ww)), leaves[:2], dy4))
    assert kinds == ["tokens_blend_to_planes", "planes_tail_bwd"] and _bits(leaves[0].grad, d_tok) and _bits(leaves[1].grad, d_base), kinds
    only_alpha = [tok, base, bias, leaves[3]]
    _, kinds = _profiled(lambda: _grads(lambda: ops.tokens_blend_to_planes(*only_alpha, (Hh, Ww)), leaves[3:], dy4))
    assert kinds == ["tokens_blend_to_planes", "planes_tail_bwd", "tails_reduce"] and _bits(leaves[3].grad, dalpha), kinds


@pytest.mark.parametrize("tag", list(B.DTYPES))
@pytest.mark.parametrize("with_h", [False, True], ids=["x", "x+h"])
def test_ops_add_lerp_under_autograd(with_h, tag, route_every_supported_shape):
    """ops.add_lerp at 3 x 37 rows of 64 with alpha [3] in the storage type (what SpatialVideoTransformer passes under grad): y
    bit-identical to the no-grad call; d_x and d_h the same bits, d_base, and dalpha = the direct fp32 sum rounded once to alpha's
    type; alpha frozen: one rows_tail_bwd, no reduce, alpha alone is saved; repeatable, also under checkpoint."""
    from torch.utils.checkpoint import checkpoint
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    G, rd, C = 3, 37, 64
    dy, x, h, base, alpha = (t.to(DEV) for t in B.make_rows(G, rd, C, dt, seed=21))
    dy, x, h, base = (t.reshape(G, rd, C) for t in (dy, x, h, base))
    alpha = alpha.to(dt)
    if not with_h:
        h = None
    with torch.no_grad():
        y0 = ops.add_lerp(x, h, base, alpha)
    leaves = [None if t is None else t.clone().requires_grad_() for t in (x, h, base, alpha)]
    run = lambda: ops.add_lerp(*leaves)
    (y, sizes), kinds_f = _profiled(lambda: _saved_sizes(run))
    assert kinds_f == ["add_lerp"] and _bits(y, y0), kinds_f
    assert sorted(sizes) == sorted([G] + [x.numel()] * (3 if with_h else 2)), sizes
    _, kinds_b = _profiled(lambda: y.backward(dy))
    assert kinds_b == ["rows_tail_bwd", "tails_reduce"], kinds_b
    d_t, d_base, dalpha = hip_ops.rows_tail_backward(dy, alpha, x=x, h=h, base=base)
    g = [None if l is None else l.grad for l in leaves]
    assert _bits(g[0], d_t) and _bits(g[2], d_base) and _bits(g[3], dalpha.to(dt)) and g[3].shape == alpha.shape
    assert not with_h or _bits(g[1], d_t)
    again = _grads(run, leaves, dy)
    ck = _grads(lambda: checkpoint(ops.add_lerp, *leaves, use_reentrant=False), leaves, dy)
    assert all(a is None and b is None or (_bits(a, b) and _bits(c, b)) for a, b, c in zip(again, g, ck))
    frozen = leaves[:3] + [alpha]
    (_, sizes), _ = _profiled(lambda: _saved_sizes(lambda: ops.add_lerp(*frozen)))
    assert sizes == [G], sizes
    _, kinds = _profiled(lambda: _grads(lambda: ops.add_lerp(*frozen), leaves[:3], dy))
    assert kinds == ["add_lerp", "rows_tail_bwd"] and _bits(leaves[0].grad, d_t) and _bits(leaves[2].grad, d_base), kinds
    only_base = [x, h, leaves[2], alpha]
    _, kinds = _profiled(lambda: _grads(lambda: ops.add_lerp(*only_base), leaves[2:3], dy))
    assert kinds == ["add_lerp", "rows_tail_bwd"] and _bits(leaves[2].grad, d_base), kinds


def test_ops_planes_to_tokens_under_autograd(route_every_supported_shape):
    """ops.planes_to_tokens: the kernel forward, the opposite kernel backward — both exact transpositions."""
    ops, hip_ops = _ops()
    x = torch.randn(3, 72, 5, 8, device=DEV).to(torch.bfloat16)
    g = torch.randn(3, 40, 72, device=DEV).to(torch.bfloat16)
    assert ops.planes_to_tokens_routed(x.clone().requires_grad_()) and not ops.planes_to_tokens_routed(x)
    xa = x.clone().requires_grad_()
    y, kinds_f = _profiled(lambda: ops.planes_to_tokens(xa))
    _, kinds_b = _profiled(lambda: y.backward(g))
    assert kinds_f == ["planes_to_tokens"] and kinds_b == ["tokens_to_planes_add"], (kinds_f, kinds_b)
    assert _bits(y, x.flatten(2).transpose(1, 2).contiguous()) and _bits(xa.grad, g.transpose(1, 2).reshape(x.shape).contiguous())
    with torch.no_grad():
        assert _bits(ops.planes_to_tokens(x), y)


@pytest.mark.parametrize("tag", list(B.DTYPES))
def test_switch_off_is_the_composition_of_today(tag, monkeypatch):
    """ops.BLOCK_TAILS_BACKWARD off (the default): under autograd tokens_to_planes_add and add_lerp run the PyTorch compositions they
    ran before — output and gradients bit for bit — record their fallbacks, launch no *_tail_bwd kind, and strict mode raises."""
    ops, hip_ops = _ops()
    monkeypatch.setattr(ops, "BLOCK_TAILS_BACKWARD", False)
    dt = B.DTYPES[tag]
    N, C, Hh, Ww = 3, 64, 8, 9
    dy, tok, base, bias, alpha = (t.to(DEV) for t in B.make_planes(N, C, Hh * Ww, dt, seed=23))
    x_in, dy4 = base.transpose(1, 2).reshape(N, C, Hh, Ww).contiguous(), dy.reshape(N, C, Hh, Ww)
    a_rows = alpha.to(dt)
    with pytest.raises(ops.HipPathError):
        ops.tokens_to_planes_add(tok.clone().requires_grad_(), x_in, bias)
    monkeypatch.setattr(ops, "STRICT", False)

    def add_today(tok, x_in, bias):
        return (tok + bias.to(tok.dtype)).transpose(1, 2).reshape(x_in.shape) + x_in

    def lerp_today(x, h, base, alpha):
        return torch.lerp((x + h).reshape(N, -1, C), base.reshape(N, -1, C), alpha.reshape(N, 1, 1).to(x.dtype)).reshape(x.shape)

    def both(fn, ref, tensors, g):
        outs = []
        for f in (fn, ref):
            leaves = [t.clone().requires_grad_() for t in tensors]
            y = f(*leaves)
            y.backward(g)
            outs.append([y.detach()] + [l.grad for l in leaves])
        return outs
    del ops.FALLBACKS[:]
    (got, want), kinds = _profiled(lambda: both(ops.tokens_to_planes_add, add_today, (tok, x_in, bias), dy4))
    assert all(_bits(a, b) for a, b in zip(got, want)) and not [k for k in kinds if k in TAIL_KINDS], kinds
    (got, want), kinds = _profiled(lambda: both(ops.add_lerp, lerp_today, (tok, base, base.flip(0), a_rows), dy.transpose(1, 2).contiguous()))
    assert all(_bits(a, b) for a, b in zip(got, want)) and not [k for k in kinds if k in TAIL_KINDS], kinds
    assert {f[0] for f in ops.FALLBACKS} == {"tokens_to_planes_add", "add_lerp"}, ops.FALLBACKS


# ---- one block -----------------------------------------------------------------------------------------------------------------------
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
def test_video_resblock_stays_on_the_hip_path(tag, route_every_supported_shape):
    """The configuration of tests/test_conv3t_bwd_gpu.py::test_video_resblock_under_checkpoint_against_the_parent_route:
    layers.VideoResBlock(320, 1280, 0.0, (3, 1, 1), out_channels=320, learned_with_images), 2 videos x 3 frames of 8x8, every parameter
    trainable, under checkpoint(use_reentrant=False), RESBLOCK_CONV_BWD and TIME_STACK_CONV_BWD on. With BLOCK_TAILS_BACKWARD on,
    ops.STRICT = True holds: no tokens_to_planes_add, bias_residual_blend or bias_residual_add fallback. Every gradient tensor with
    more than one element is within 2.0 x (max) / 1.6 x (rms) of the switch-off route's own error (ops.STRICT = False there) against
    the fp64 CPU module. time_mixer.mix_factor.grad is reported, not held to a ratio (the reason stands in that test's docstring; the
    direct dalpha cap above holds the sum), and two runs of the new route give it bit-identical — which the parent route cannot promise."""
    from torch.utils.checkpoint import checkpoint
    from multiview_inpaint_amd.svd import layers
    ops, hip_ops = _ops()
    dt = B.DTYPES[tag]
    T, N = 3, 6

    def make():
        m = layers.VideoResBlock(320, 1280, 0.0, video_kernel_size=[3, 1, 1], out_channels=320, merge_strategy="learned_with_images", merge_factor=0.5)
        _seed_params(m, 23)
        return m
    g = torch.Generator().manual_seed(29)
    x = torch.randn(N, 320, 8, 8, generator=g).to(dt)
    emb = torch.randn(N, 1280, generator=g).to(dt)
    dy = torch.randn(N, 320, 8, 8, generator=g).to(dt)
    ind = torch.zeros(N // T, T)
    m64 = make().double()
    x64 = x.double().requires_grad_()
    m64(x64, emb.double(), T, ind).backward(dy.double())
    ref = {"x": x64.grad, **{n: p.grad for n, p in m64.named_parameters() if p.grad is not None}}

    def gpu_run():
        m = make().to(DEV, dt)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        _, kinds = _profiled(lambda: checkpoint(m, xg, emb.to(DEV), T, ind.to(DEV), use_reentrant=False).backward(dy.to(DEV)))
        return {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters() if p.grad is not None}}, kinds, list(ops.FALLBACKS)

    layers.TIME_STACK_CONV_BWD = layers.RESBLOCK_CONV_BWD = True     # (restored by the module's fixture)
    new, kinds, fallbacks = gpu_run()                                # ops.STRICT is True here
    assert not [f for f in fallbacks if f[0] in ("tokens_to_planes_add", "bias_residual_blend", "bias_residual_add")], fallbacks
    assert kinds.count("planes_tail_bwd") == 2 and kinds.count("tails_reduce") == 2 and kinds.count("tokens_blend_to_planes") == 2, kinds
    new2, _, _ = gpu_run()
    assert _bits(new2["time_mixer.mix_factor"], new["time_mixer.mix_factor"])
    ops.BLOCK_TAILS_BACKWARD, ops.STRICT = False, False
    old, old_kinds, old_fallbacks = gpu_run()
    ops.BLOCK_TAILS_BACKWARD, ops.STRICT = True, True
    assert not [k for k in old_kinds if k in TAIL_KINDS], old_kinds
    assert {"tokens_to_planes_add", "bias_residual_blend"} <= {f[0] for f in old_fallbacks}, old_fallbacks
    assert set(new) == set(old) and set(new) <= set(ref), (set(new) ^ set(old), set(new) - set(ref))
    bad = []
    for name in new:
        o_max, o_rms = B.errors(old[name].cpu(), ref[name])
        e_max, e_rms = B.errors(new[name].cpu(), ref[name])
        H_.report(f"VideoResBlock 320 2x3x8x8 tails {tag} d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = {e_rms / o_rms:.2f} x the switch-off route's own error")
        if new[name].numel() > 1 and not (e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms):
            bad.append((name, e_max, o_max, e_rms, o_rms))
    assert not bad, bad
    assert [n for n in new if new[n].numel() == 1] == ["time_mixer.mix_factor"]

"""The GroupNorm entry points after they were folded to one forward per family — no GPU.

* The C library: the nine removed entries are gone, and the argument checks of mvi_groupnorm_forward / mvi_groupnorm_tok2tok_forward
  answer, in order, what the entries they replace answered (mvi_groupnorm_forward_stats followed by gn_dispatch; tok2tok_impl) — code and
  mvi_unet_last_error() text written out below, the same with `stats` NULL and non-NULL. Every case returns before any HIP call, so
  host buffers stand in for device pointers: nothing dereferences them.
* svd/ops.py: where a call of the four public norms lands — the no-grad launch, _GroupNormFn.apply with which layout and T, or
  ops.HipPathError before the PyTorch expression — against the conditions the ops spelled out before _GroupNormFn served all four
  and the two predicates shared a body, restated here in plain Python (`parent_*`). The ops are called with stand-ins for CUDA tensors
  and the hip_ops launches replaced, as in tests/test_conv_launch_gate_cpu.py; hip_ops.*_backward_supported are host-only functions
  and run for real."""
import ctypes
import itertools

import pytest
import torch

from multiview_inpaint_amd.svd import hip_ops, ops

EINVAL, ENOMEM = -1, -3
REMOVED = ("mvi_groupnorm_silu", "mvi_groupnorm_silu_temporal", "mvi_groupnorm_silu_ex", "mvi_groupnorm_silu_ex2",
           "mvi_groupnorm_silu_tokens", "mvi_groupnorm_forward_stats", "mvi_groupnorm_silu_tok2tok", "mvi_groupnorm_silu_tok2tok_frames",
           "mvi_groupnorm_tok2tok_forward_stats")


@pytest.fixture(scope="module")
def L():
    from multiview_inpaint_amd import _lib
    return _lib.lib()                                            # raises if a declared symbol is missing


def test_symbol_set(L):
    for name in REMOVED:
        assert not hasattr(L, name), name
    for name in ("mvi_groupnorm_forward", "mvi_groupnorm_tok2tok_forward", "mvi_groupnorm_silu_tok2tok_pre", "mvi_groupnorm_silu_tok2tok_split",
                 "mvi_groupnorm_workspace_bytes", "mvi_groupnorm_sync_bytes", "mvi_groupnorm_tok2tok_workspace_bytes"):
        assert hasattr(L, name), name


# ---- the error tables ---------------------------------------------------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(4096 + 64)
_A = (ctypes.addressof(_BUF) + 63) // 64 * 64                    # a 64-byte aligned host address
X, Y, W, B, WS, SYNC, STATS = _A, _A + 512, _A + 1024, _A + 1536, _A + 2048, _A + 2560, _A + 3072
PLANES, STACK3, TOKENS = 0, 1, 2
BF16 = 1

# a call that every check passes (it would launch: never made) ...
PLANES_OK = dict(x=X, y=Y, weight=W, bias=B, chan_bias=None, videos=2, T=1, C=64, spatial=64, groups=32, eps=1e-5, silu=1, layout=PLANES,
                 dtype=BF16, ws=WS, ws_bytes=1 << 20, sync=None, sync_bytes=0)
# ... and what one or two changed arguments are answered, in the order of the checks
MSG_VEC = "groupnorm (token-major output): C and spatial must be multiples of the 16-byte vector, 16-B aligned"
PLANES_CASES = [
    (dict(layout=3), EINVAL, "groupnorm: unknown output layout"),
    (dict(layout=-1), EINVAL, "groupnorm: unknown output layout"),
    (dict(layout=3, y=X, C=60, x=None), EINVAL, "groupnorm: unknown output layout"),                 # first of several
    (dict(layout=STACK3, y=X), EINVAL, "groupnorm: this output layout cannot alias the input"),
    (dict(layout=TOKENS, y=X), EINVAL, "groupnorm: this output layout cannot alias the input"),
    (dict(layout=TOKENS, y=X, T=2), EINVAL, "groupnorm: this output layout cannot alias the input"),
    (dict(layout=TOKENS, T=2), EINVAL, "groupnorm (token-major output): T must be 1"),
    (dict(layout=TOKENS, T=2, C=60), EINVAL, "groupnorm (token-major output): T must be 1"),
    (dict(sync=SYNC, sync_bytes=8), ENOMEM, "groupnorm: sync buffer too small"),
    (dict(sync=SYNC, sync_bytes=8, layout=STACK3, T=2), ENOMEM, "groupnorm: sync buffer too small"),
    (dict(sync=SYNC, sync_bytes=8, C=60), ENOMEM, "groupnorm: sync buffer too small"),
    (dict(sync=SYNC, sync_bytes=8, layout=TOKENS, C=60), EINVAL, "groupnorm: C must be a positive multiple of groups"),     # token-major: sync not looked at
    (dict(C=60), EINVAL, "groupnorm: C must be a positive multiple of groups"),
    (dict(groups=0), EINVAL, "groupnorm: C must be a positive multiple of groups"),
    (dict(T=0), EINVAL, "groupnorm: C must be a positive multiple of groups"),
    (dict(videos=-1), EINVAL, "groupnorm: C must be a positive multiple of groups"),
    (dict(C=60, x=None), EINVAL, "groupnorm: C must be a positive multiple of groups"),
    (dict(x=None), EINVAL, "groupnorm: NULL pointer"),
    (dict(y=None), EINVAL, "groupnorm: NULL pointer"),
    (dict(weight=None), EINVAL, "groupnorm: NULL pointer"),
    (dict(bias=None), EINVAL, "groupnorm: NULL pointer"),
    (dict(ws=None), EINVAL, "groupnorm: NULL pointer"),
    (dict(ws=None, videos=2048), EINVAL, "groupnorm: NULL pointer"),
    (dict(videos=2048), EINVAL, "groupnorm: N*groups exceeds grid.y (65535)"),
    (dict(videos=2048, ws_bytes=0), EINVAL, "groupnorm: N*groups exceeds grid.y (65535)"),
    (dict(ws_bytes=0), ENOMEM, "groupnorm: workspace too small"),
    (dict(ws_bytes=0, dtype=7), ENOMEM, "groupnorm: workspace too small"),
    (dict(ws_bytes=2 * 32 * 3 * 4 - 1), ENOMEM, "groupnorm: workspace too small"),                  # one byte short of 2 x 32 groups x 1 chunk x 3 floats
    (dict(dtype=7), EINVAL, "groupnorm: unknown dtype"),
    (dict(dtype=-1, layout=TOKENS, C=60, groups=30), EINVAL, "groupnorm: unknown dtype"),
    (dict(layout=TOKENS, C=60, groups=30), EINVAL, MSG_VEC),
    (dict(layout=TOKENS, spatial=45), EINVAL, MSG_VEC),
    (dict(layout=TOKENS, x=X + 8), EINVAL, MSG_VEC),
    (dict(layout=TOKENS, y=Y + 2), EINVAL, MSG_VEC),
    (dict(layout=TOKENS, dtype=0, C=36, groups=9, spatial=64, x=X + 4), EINVAL, MSG_VEC),            # fp32: multiples of 4, still unaligned
]
PLANES_EMPTY = [dict(videos=0), dict(spatial=0), dict(videos=0, T=14, layout=STACK3, y=Y), dict(spatial=0, layout=TOKENS, y=Y)]

TOK_OK = dict(x=X, y=Y, weight=W, bias=B, chan_bias=None, N=4, frames=1, C=64, spatial=64, groups=32, eps=1e-5, silu=1, dtype=BF16, ws=WS,
              ws_bytes=1 << 20)
MSG_GEOM = "groupnorm_tok2tok: C must be a multiple of groups (<= 64) and of the 16-byte vector width"
MSG_VIDEOS = "groupnorm_tok2tok: N must be a whole number of videos of `frames` samples"
TOK_CASES = [
    (dict(C=60, groups=30), EINVAL, MSG_GEOM),                   # no multiple of the bf16 vector
    (dict(C=60, groups=32), EINVAL, MSG_GEOM),
    (dict(C=1280, groups=128), EINVAL, MSG_GEOM),                # more than 64 groups
    (dict(dtype=0, C=36, groups=8), EINVAL, MSG_GEOM),
    (dict(groups=0), EINVAL, MSG_GEOM),
    (dict(N=65536), EINVAL, MSG_GEOM),
    (dict(N=-1), EINVAL, MSG_GEOM),
    (dict(C=16384, groups=32), EINVAL, MSG_GEOM),                # C / 8 vectors per row over 1024
    (dict(C=60, groups=30, frames=3, x=None), EINVAL, MSG_GEOM),
    (dict(frames=3), EINVAL, MSG_VIDEOS),
    (dict(frames=0), EINVAL, MSG_VIDEOS),
    (dict(frames=3, x=None), EINVAL, MSG_VIDEOS),
    (dict(x=None), EINVAL, "groupnorm_tok2tok: NULL pointer"),
    (dict(y=None), EINVAL, "groupnorm_tok2tok: NULL pointer"),
    (dict(weight=None), EINVAL, "groupnorm_tok2tok: NULL pointer"),
    (dict(bias=None), EINVAL, "groupnorm_tok2tok: NULL pointer"),
    (dict(ws=None), EINVAL, "groupnorm_tok2tok: NULL pointer"),
    (dict(ws=None, x=X + 8), EINVAL, "groupnorm_tok2tok: NULL pointer"),
    (dict(x=X + 8), EINVAL, "groupnorm_tok2tok: x / y must be 16-byte aligned"),
    (dict(y=Y + 2), EINVAL, "groupnorm_tok2tok: x / y must be 16-byte aligned"),
    (dict(y=Y + 2, ws_bytes=0), EINVAL, "groupnorm_tok2tok: x / y must be 16-byte aligned"),
    (dict(ws_bytes=0), ENOMEM, "groupnorm_tok2tok: workspace too small"),
    (dict(ws_bytes=0, dtype=7), ENOMEM, "groupnorm_tok2tok: workspace too small"),
    (dict(ws_bytes=(4 * 1 * 32 * 3 + 4 * 64 * 2) * 4 - 1), ENOMEM, "groupnorm_tok2tok: workspace too small"),    # 64 tokens = one chunk per sample
    (dict(dtype=7), EINVAL, "groupnorm_tok2tok: unknown dtype"),
    (dict(dtype=-1, frames=2), EINVAL, "groupnorm_tok2tok: unknown dtype"),
]
TOK_EMPTY = [dict(N=0), dict(spatial=0), dict(N=0, frames=0, C=60, dtype=7)]      # the empty test comes first


def call_planes(L, a, stats, entry="mvi_groupnorm_forward"):
    rc = getattr(L, entry)(a["x"], a["y"], a["weight"], a["bias"], a["chan_bias"], stats, a["videos"], a["T"], a["C"], a["spatial"], a["groups"],
                           a["eps"], a["silu"], a["layout"], a["dtype"], a["ws"], a["ws_bytes"], a["sync"], a["sync_bytes"], None)
    return rc, L.mvi_unet_last_error().decode()


def call_tok(L, a, stats, entry="mvi_groupnorm_tok2tok_forward"):
    rc = getattr(L, entry)(a["x"], a["y"], a["weight"], a["bias"], a["chan_bias"], stats, a["N"], a["frames"], a["C"], a["spatial"], a["groups"],
                           a["eps"], a["silu"], a["dtype"], a["ws"], a["ws_bytes"], None)
    return rc, L.mvi_unet_last_error().decode()


@pytest.mark.parametrize("stats", (None, STATS), ids=("inference", "stats"))
@pytest.mark.parametrize("call,ok,cases,empty", ((call_planes, PLANES_OK, PLANES_CASES, PLANES_EMPTY), (call_tok, TOK_OK, TOK_CASES, TOK_EMPTY)),
                         ids=("planes", "tok2tok"))
def test_error_table(L, call, ok, cases, empty, stats):
    for change, code, text in cases:
        assert call(L, {**ok, **change}, stats) == (code, text), change
    nothing = {k: None for k in ("x", "y", "weight", "bias", "chan_bias", "ws", "sync") if k in ok}
    for change in empty:                                          # an empty tensor is MVI_OK, also with every pointer NULL
        assert call(L, {**ok, **change}, stats)[0] == 0, change
        if change.get("layout", PLANES) == PLANES:                # (x == y == NULL is an alias to the other two layouts)
            assert call(L, {**ok, **change, **nothing}, None)[0] == 0, change


# ---- routing of the four public ops ---------------------------------------------------------------------------------------------------
class Fake:
    """What the ops ask of a CUDA tensor before they launch."""

    def __init__(self, shape, dtype=torch.bfloat16, grad=False, ptr=4096, contiguous=True):
        self.shape, self.dtype, self.requires_grad, self.is_cuda, self._ptr, self._contiguous = tuple(shape), dtype, grad, True, ptr, contiguous

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return self._contiguous

    def __getitem__(self, idx):
        return Fake(self.shape[len(idx):], self.dtype)


class Landing:
    """Where a call ended: ("launch", hip_ops function) or ("fn", layout, T); `.copied` once PyTorch's transposing copy followed."""

    def __init__(self, *where):
        self.where, self.copied = where, False

    def flatten(self, *a):
        self.copied = True
        return self

    transpose = flatten

    def contiguous(self):
        return self


def landing(call):
    try:
        r = call()
    except ops.HipPathError:
        return "HipPathError"
    return r.where + (("copied",) if r.copied else ())


@pytest.fixture
def routed(monkeypatch):
    monkeypatch.setattr(ops, "STRICT", True)                     # leaving the HIP path raises, whatever the reason
    for name in ("group_norm_silu", "group_norm_silu_tokens", "group_norm_silu_frames", "group_norm_silu_tok2tok"):
        monkeypatch.setattr(hip_ops, name, lambda *a, _n=name, **k: Landing("launch", _n))
    monkeypatch.setattr(ops._GroupNormFn, "apply", staticmethod(lambda x, w, b, cb, G, eps, silu, T, layout: Landing("fn", layout, T)))
    return monkeypatch


def _planes_pays(N, C, S, layout):
    return N * C * S >= ops.GROUPNORM_BACKWARD_MIN_ELEMENTS[layout]


def parent_planes_predicate(x, T, G, cb, layout):
    if not (ops.GROUPNORM_BACKWARD and x.dim() >= 2 and x.numel() > 0):
        return False
    N, C = x.shape[0], x.shape[1]
    S = x.numel() // (N * C)
    if cb is not None and tuple(cb.shape) != (N, C):
        return False
    return hip_ops.group_norm_backward_supported(N, C, S, G, T, x.dtype, layout) and _planes_pays(N, C, S, layout)


def parent_tok2tok_predicate(t, G, cb, frames):
    if not (ops.GROUPNORM_TOK2TOK_BACKWARD and t.dim() == 3 and t.numel() > 0 and frames >= 1):
        return False
    N, S, C = t.shape
    if cb is not None and tuple(cb.shape) != (N, C):
        return False
    if t.is_contiguous() and t.data_ptr() % 16 != 0:
        return False
    line = ops.GROUPNORM_TOK2TOK_BACKWARD_MIN_ELEMENTS
    return hip_ops.group_norm_tok2tok_backward_supported(N, C, S, G, frames, t.dtype) and line is not None and N * C * S >= line


def parent_group_norm(x, G, cb, grad):
    if not grad:
        return ("launch", "group_norm_silu")
    return ("fn", 0, 1) if parent_planes_predicate(x, 1, G, cb, 0) else "HipPathError"


def parent_group_norm_tokens(x, G, cb, grad):
    C, S = x.shape[1], x.numel() // (x.shape[0] * x.shape[1])
    if not grad:
        return ("launch", "group_norm_silu_tokens") if C % 8 == 0 and S % 8 == 0 else ("launch", "group_norm_silu", "copied")
    if C % 8 == 0 and S % 8 == 0 and x.data_ptr() % 16 == 0 and parent_planes_predicate(x, 1, G, cb, 2):
        return ("fn", 2, 1)
    return ("fn", 0, 1, "copied") if parent_planes_predicate(x, 1, G, cb, 0) else "HipPathError"


def parent_group_norm_frames(x, T, G, cb, stack3, grad):
    if not grad:
        return ("launch", "group_norm_silu_frames")
    layout = 1 if stack3 else 0
    return ("fn", layout, T) if x.shape[0] % T == 0 and parent_planes_predicate(x, T, G, cb, layout) else "HipPathError"


def parent_group_norm_tok2tok(t, G, cb, frames, grad):
    if not grad:
        return ("launch", "group_norm_silu_tok2tok")
    return ("fn", ops._GN_TOK2TOK, frames) if parent_tok2tok_predicate(t, G, cb, frames) else "HipPathError"


GRADS = ("none", "x", "weight")                                  # who requires grad
# (N, C, spatial, groups): small, odd S, C no multiple of 8, N no multiple of T = 2, and sizes on either side of the three default lines
PLANES_SHAPES = ((2, 64, (8, 8), 32), (2, 64, (5, 9), 32), (2, 60, (8, 8), 30), (3, 64, (8, 8), 32), (14, 320, (48, 64), 32),
                 (14, 1920, (24, 32), 32), (28, 320, (24, 32), 32), (2, 64, (), 32), (0, 64, (8, 8), 32))
# (N, S, C, groups): small, odd S, C no multiple of 8, more than 64 groups, three samples (no whole videos of 2), large, not 3-d
TOK_SHAPES = ((2, 64, 64, 32), (2, 45, 64, 32), (2, 64, 60, 30), (2, 16, 1280, 128), (3, 64, 64, 32), (4, 4096, 320, 32))
PLANES_LINES = (None, (0, 0, 0))                                 # None: the module's default (a line per layout; None is no value of it)
TOK_LINES = ("default", 0, 1 << 20)                             # the module's default is None: nothing routed


def _operands(shape, cbs, grad, dtype, **kw):
    x = Fake(shape, dtype, grad == "x", **kw)
    w = Fake((cbs[1],), torch.float32, grad == "weight")
    b = Fake((cbs[1],), torch.float32, grad == "weight")
    cb = {"none": None, "right": Fake(cbs, dtype), "wrong": Fake((cbs[0] + 1, cbs[1]), dtype)}
    return x, w, b, cb


@pytest.mark.parametrize("switch", (True, False))
@pytest.mark.parametrize("line", PLANES_LINES)
def test_routing_planes(routed, switch, line):
    routed.setattr(ops, "GROUPNORM_BACKWARD", switch)
    if line is not None:
        routed.setattr(ops, "GROUPNORM_BACKWARD_MIN_ELEMENTS", line)
    seen = set()
    for (N, C, sp, G), grad, dtype, ptr, which in itertools.product(PLANES_SHAPES, GRADS, (torch.bfloat16, torch.float32), (4096, 4104),
                                                                    ("none", "right", "wrong")):
        x, w, b, cbs = _operands((N, C, *sp), (N, C), grad, dtype, ptr=ptr)
        cb, g, case = cbs[which], grad != "none", (N, C, sp, G, grad, dtype, ptr, which)
        if N:                                                    # (group_norm_tokens reads x[0, 0])
            want = parent_group_norm_tokens(x, G, cb, g)
            assert landing(lambda: ops.group_norm_tokens(x, G, w, b, 1e-5, True, chan_bias=cb)) == want, ("group_norm_tokens",) + case
            seen.add(want)
        want = parent_group_norm(x, G, cb, g)
        assert landing(lambda: ops.group_norm(x, G, w, b, 1e-5, True, chan_bias=cb)) == want, ("group_norm",) + case
        seen.add(want)
        for T, stack3 in itertools.product((1, 2, 14), (False, True)):
            want = parent_group_norm_frames(x, T, G, cb, stack3, g)
            assert landing(lambda: ops.group_norm_frames(x, T, G, w, b, 1e-5, True, chan_bias=cb, stack3=stack3)) == want, \
                ("group_norm_frames", T, stack3) + case
            seen.add(want)
    every = {("launch", "group_norm_silu"), ("launch", "group_norm_silu_tokens"), ("launch", "group_norm_silu", "copied"),
             ("launch", "group_norm_silu_frames"), "HipPathError"}
    if switch:
        every |= {("fn", 0, 1), ("fn", 2, 1), ("fn", 0, 1, "copied"), ("fn", 0, 2), ("fn", 1, 2), ("fn", 1, 14), ("fn", 1, 1)}
    assert every <= seen, every - seen
    if not switch:
        assert not any(s[0] == "fn" for s in seen)


@pytest.mark.parametrize("switch", (True, False))
@pytest.mark.parametrize("line", TOK_LINES)
def test_routing_tok2tok(routed, switch, line):
    routed.setattr(ops, "GROUPNORM_TOK2TOK_BACKWARD", switch)
    if line != "default":
        routed.setattr(ops, "GROUPNORM_TOK2TOK_BACKWARD_MIN_ELEMENTS", line)
    assert ops.GROUPNORM_TOK2TOK_BACKWARD_MIN_ELEMENTS == (None if line == "default" else line)
    seen = set()
    tensors = ((4096, True), (4104, True), (4104, False))        # aligned; contiguous and misaligned: refused; not contiguous: not refused
    for (N, S, C, G), grad, dtype, (ptr, contig), which, frames in itertools.product(TOK_SHAPES, GRADS, (torch.bfloat16, torch.float32), tensors,
                                                                                    ("none", "right", "wrong"), (1, 2, 0)):
        t, w, b, cbs = _operands((N, S, C), (N, C), grad, dtype, ptr=ptr, contiguous=contig)
        cb = cbs[which]
        want = parent_group_norm_tok2tok(t, G, cb, frames, grad != "none")
        assert landing(lambda: ops.group_norm_tok2tok(t, G, w, b, 1e-5, True, chan_bias=cb, frames=frames)) == want, \
            (N, S, C, G, grad, dtype, ptr, contig, which, frames)
        assert ops.group_norm_tok2tok_hip_autograd(t, G, cb, frames) == parent_tok2tok_predicate(t, G, cb, frames)
        seen.add(want)
    t4 = Fake((2, 64, 8, 8), grad=True)                          # not token-major [N, S, C]
    assert not ops.group_norm_tok2tok_hip_autograd(t4, 32) and not parent_tok2tok_predicate(t4, 32, None, 1)
    every = {("launch", "group_norm_silu_tok2tok"), "HipPathError"}
    if switch and line != "default":
        every |= {("fn", ops._GN_TOK2TOK, 1), ("fn", ops._GN_TOK2TOK, 2)}
    assert every == seen, (every, seen)
    if switch and line == 0:                                     # the named refusals, with everything else in favour
        ok = Fake((2, 64, 64), grad=True)
        assert ops.group_norm_tok2tok_hip_autograd(ok, 32) and ops.group_norm_tok2tok_hip_autograd(Fake((2, 64, 64), ptr=4104, contiguous=False), 32)
        assert not ops.group_norm_tok2tok_hip_autograd(Fake((2, 64, 64), ptr=4104), 32)
        assert not ops.group_norm_tok2tok_hip_autograd(Fake((2, 16, 1280)), 128) and ops.group_norm_tok2tok_hip_autograd(Fake((2, 16, 1280)), 64)
        assert not ops.group_norm_tok2tok_hip_autograd(ok, 32, Fake((3, 64)))
        assert not ops.group_norm_tok2tok_hip_autograd(Fake((3, 64, 64)), 32, None, 2)

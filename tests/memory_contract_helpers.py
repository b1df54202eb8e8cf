"""The memory contract of the UNet op wrappers (multiview_inpaint_amd/svd/hip_ops.py), as a harness in plain PyTorch — it works on cpu
and cuda tensors alike (tests/test_memory_contract_cpu.py runs it on a toy module, tests/test_memory_contract_gpu.py on hip_ops).

Three rules are enforced on a call:
  1. every returned byte is written by this call;
  2. a returned byte depends on no byte the call did not write or was not given;
  3. nothing outside the outputs and the declared workspace bytes is written.

How: every allocation the wrappers make (their outputs, through a proxy of the name `torch` in the module's globals; the scratch, through
a replaced `_workspace` that hands out exactly the declared bytes) and every input (`place`) is a window in the middle of a larger buffer
filled with one `background` byte. The call runs once per background. Rules 1 and 2 hold when the returned tensors have the same bits
under every background and in an unpatched run (`verify`); rule 3 when every guard zone still holds its background afterwards (`check`).
An input must come back with the bits that were placed, unless the case declares it an output of an in-place op."""
import contextlib

import torch

GUARD = 64 << 10                                  # bytes on each side: a multiple of 256, the window keeps the allocator's alignment
BACKGROUNDS = (0x00, 0xFF, 0x7B, 0xFB)            # zeros; NaN (-1 as an integer); a large positive and a large negative finite value in
#                                                   fp32, bf16 and f16 alike — what a max or a min would swallow if it were NaN

_REGISTRY = []


class _Alloc:
    __slots__ = ("name", "buf", "offset", "nbytes", "background", "snapshot")

    def __init__(self, name, buf, offset, nbytes, background):
        self.name, self.buf, self.offset, self.nbytes, self.background, self.snapshot = name, buf, offset, nbytes, background, None

    def window(self):
        return self.buf[self.offset:self.offset + self.nbytes]


def reset():
    del _REGISTRY[:]


def _prod(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def _shape(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(int(v) for v in args[0])
    return tuple(int(v) for v in args)


def guarded(shape, dtype, device, background, name=None):
    """A contiguous tensor of `shape` and `dtype`: a view into the middle of a uint8 buffer with GUARD bytes on each side, the whole
    buffer (window included) filled with the one-byte `background`. Registered for check()."""
    shape = tuple(int(v) for v in shape)
    nbytes = _prod(shape) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((GUARD + nbytes + GUARD,), background, dtype=torch.uint8, device=device)
    a = _Alloc(name or f"alloc#{len(_REGISTRY)}", buf, GUARD, nbytes, background)
    a.name = f"{a.name} {dtype} {list(shape)}"
    _REGISTRY.append(a)
    return a.window().view(dtype).view(shape)


def place(t, background, name=None):
    """A contiguous copy of the input t in a guarded window: what lies past its end (and before its start) is `background`. check() also
    asserts that the window still holds the placed bits (declare_output lifts that for the argument of an in-place op)."""
    if t is None:
        return None
    src = t.detach().contiguous()
    p = guarded(src.shape, src.dtype, src.device, background, name or f"input#{len(_REGISTRY)}")
    p.copy_(src)
    _REGISTRY[-1].snapshot = _REGISTRY[-1].window().clone()
    return p


def declare_output(t):
    """The placed input t is the output of an in-place op: its window may change (its guards may not)."""
    a = _find(t)
    assert a is not None and a.snapshot is not None, "declare_output: not a placed input"
    a.snapshot = None


def _find(t):
    p = t.data_ptr()
    for a in _REGISTRY:
        base = a.buf.data_ptr() + a.offset
        if a.buf.device == t.device and base <= p < base + max(a.nbytes, 1):
            return a
    return None


def name_of(t):
    a = _find(t)
    return "an allocation outside the harness" if a is None else a.name


def _span(bad):
    idx = bad.nonzero().reshape(-1)
    return int(idx[0]), int(idx[-1]), int(idx.numel())


def check():
    """After torch.cuda.synchronize(): every guard zone of every registered buffer (outputs, workspace windows, inputs) still holds its
    background byte, and every placed input its placed bits. The failure names the allocation, the side, the first and last offset."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    for a in _REGISTRY:
        end = a.offset + a.nbytes
        for side, zone, origin in (("before", a.buf[:a.offset], -a.offset), ("after", a.buf[end:], a.nbytes)):
            bad = zone != a.background
            if bool(bad.any()):
                first, last, n = _span(bad)
                raise AssertionError(f"memory contract: {n} bytes written {side} {a.name} (background 0x{a.background:02X}): offsets "
                                     f"{origin + first} .. {origin + last} from the window's start, window of {a.nbytes} bytes")
        if a.snapshot is not None:
            bad = a.window() != a.snapshot
            if bool(bad.any()):
                first, last, n = _span(bad)
                raise AssertionError(f"memory contract: {a.name} was modified (background 0x{a.background:02X}): {n} bytes, offsets "
                                     f"{first} .. {last} of {a.nbytes}")


class _TorchProxy:
    """The name `torch` as the wrapped module sees it: every attribute is the real one, but empty / empty_like / empty_strided allocate
    guarded windows (zeros and everything else stay real)."""

    def __init__(self, background):
        self.__dict__["_bg"] = background

    def __getattr__(self, name):
        return getattr(torch, name)

    def _make(self, shape, dtype, device, what):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        return guarded(shape, dtype, torch.device("cpu" if device is None else device), self._bg, what)

    def empty(self, *size, dtype=None, device=None, **kw):
        assert not {k: v for k, v in kw.items() if v not in (None, False, torch.strided)}, f"torch.empty: unexpected {kw}"
        return self._make(_shape(size), dtype, device, f"empty#{len(_REGISTRY)}")

    def empty_like(self, t, dtype=None, device=None, **kw):
        assert t.is_contiguous(), "torch.empty_like of a non-contiguous tensor: the harness hands out contiguous windows"
        return self._make(t.shape, t.dtype if dtype is None else dtype, t.device if device is None else device, f"empty_like#{len(_REGISTRY)}")

    def empty_strided(self, size, stride, dtype=None, device=None, **kw):
        ref = torch.empty_strided(size, stride, dtype=dtype, device="meta")
        assert ref.is_contiguous(), "torch.empty_strided with gaps: the harness hands out contiguous windows"
        return self._make(size, dtype, device, f"empty_strided#{len(_REGISTRY)}")


def _hip_ops():
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


@contextlib.contextmanager
def contract(monkeypatch, background, module=None):
    """For its duration the module (hip_ops unless given) allocates through the proxy, and its `_workspace(dev, nbytes)` is a fresh guarded
    window of EXACTLY nbytes (no floor) filled with `background`. `_groupnorm_sync` is left alone: that buffer is zero before and after
    every launch by its own contract."""
    mod = _hip_ops() if module is None else module

    def workspace(dev, nbytes):
        return guarded((int(nbytes),), torch.uint8, dev, background, f"workspace#{len(_REGISTRY)} ({int(nbytes)} declared bytes)")

    with monkeypatch.context() as m:
        m.setitem(mod.__dict__, "torch", _TorchProxy(background))
        m.setitem(mod.__dict__, "_workspace", workspace)
        yield


def bits(t):
    """t's bytes as a flat uint8 tensor on the host (NaNs compare by bit pattern)."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _tensors(out):
    if torch.is_tensor(out) or out is None:
        return [out]
    return list(out)


def _same(what, a, b, name_a, name_b, alloc):
    assert (a is None) == (b is None), f"memory contract: {what} is None under {name_a} and not under {name_b}"
    if a is None:
        return
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ba, bb = bits(a), bits(b)
    if not torch.equal(ba, bb):
        first, last, n = _span(ba != bb)
        es = a.element_size()
        raise AssertionError(f"memory contract: {what} ({alloc}) has other bits under {name_b} than under {name_a}: {n} bytes differ, "
                             f"elements {first // es} .. {last // es} of {a.numel()} — an element this call did not write, or one that "
                             "depends on memory the call did not write or was not given")


def verify(monkeypatch, call, inputs, module=None, inplace=(), backgrounds=BACKGROUNDS, after=None, foreign=()):
    """call(*inputs) once unpatched, then once per background under contract() with the inputs placed under that background.
    Asserts rules 1 to 3 (module docstring) and that every input comes back as placed; inputs whose index is in `inplace` are outputs of an
    in-place op instead (each run gets its own copy). `after`, if given, runs after every contract run (further invariants). Every
    returned tensor must lie in an allocation of the harness — a call whose outputs bypass it would pass vacuously — but those whose index
    is in `foreign` (a library reduction of a guarded intermediate). -> the returned tensors of the unpatched run, as a list."""
    fresh = lambda: [t.clone() if i in inplace and t is not None else t for i, t in enumerate(inputs)]
    base = _tensors(call(*fresh()))
    for bg in backgrounds:
        reset()
        try:
            placed = [place(t, bg, f"input {i}") if torch.is_tensor(t) else t for i, t in enumerate(inputs)]
            for i in inplace:
                declare_output(placed[i])
            with contract(monkeypatch, bg, module):
                got = _tensors(call(*placed))
            check()
            assert len(got) == len(base)
            for k, v in enumerate(got):
                assert v is None or k in foreign or _find(v) is not None, f"memory contract: output {k} does not come from the harness's allocations"
            for k, (u, v) in enumerate(zip(base, got)):
                _same(f"output {k}", u, v, "the unpatched run", f"background 0x{bg:02X}", None if v is None else name_of(v))
            if after is not None:
                after()
        finally:
            reset()
    return base

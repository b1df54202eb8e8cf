"""Shared by tests/test_train_ops_refs_cpu.py and tests/test_train_ops_edges_gpu.py: plain references of the training-loop ops
declared in include/mvi_train_ops.h (window gather / scatter over a keep-mask, support bit masks, Adam in float64, the 3-NN mean
on an integer lattice, the photometric-loss inputs and their measured gradient tolerance) and the ctypes call helpers that drive
the C-ABI directly, so a test can hand the library misaligned views, NULL inputs, strided compact sides and oversized tables.

The references use nothing of the library and run on the CPU; the call helpers load it on first use."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

FLT_MAX = np.float32(3.4028234663852886e38)
SENTINEL = 0x5A5AA5A5                                                             # the word every copy destination is pre-filled with
SENTINEL_F = 1234.5                                                               # float sentinel next to the Adam views


def rand_words(shape, gen):
    """32-bit words over the full int32 range (NaN and Inf float payloads included)."""
    return torch.randint(-(1 << 31), 1 << 31, shape, generator=gen, dtype=torch.int64).to(torch.int32)


# ---- window gather / scatter -----------------------------------------------------------------------------------------
# The compact side of an entry is described like the C struct does: a flat word buffer, the word offset of row 0 inside it and the
# words between consecutive rows (`stride`); the full side is [P, w].

def window_rows(mask, first, capacity):
    """Rows of the window [first, first + capacity) of the kept-row list: n = max(0, min(capacity, n_keep - first))."""
    rows = torch.nonzero(mask.reshape(-1) != 0).reshape(-1)
    n = max(0, min(int(capacity), int(rows.numel()) - int(first)))
    return rows[first:first + n] if n > 0 else rows[:0]


def gather_window_ref(full, comp, mask, first, capacity, offset=0, stride=0):
    """comp (flat words) after out[j, :] = full[rows[first + j], :]; every other word of comp unchanged."""
    w = full.shape[1]
    stride = stride or w
    out = comp.clone()
    rows = window_rows(mask, first, capacity)
    n = rows.numel()
    if n:
        dst = (offset + torch.arange(n, device=out.device)[:, None] * stride + torch.arange(w, device=out.device)[None, :]).reshape(-1)
        out[dst] = full[rows].reshape(-1)
    return out


def scatter_window_ref(full, comp, mask, first, capacity, offset=0, stride=0):
    """full [P, w] after full[rows[first + j], :] = comp row j (comp None: zeros); every other row unchanged."""
    w = full.shape[1]
    stride = stride or w
    out = full.clone()
    rows = window_rows(mask, first, capacity)
    n = rows.numel()
    if n:
        if comp is None:
            out[rows] = 0
        else:
            src = (offset + torch.arange(n, device=out.device)[:, None] * stride + torch.arange(w, device=out.device)[None, :])
            out[rows] = comp[src.reshape(-1)].reshape(n, w)
    return out


# ---- support bit masks -----------------------------------------------------------------------------------------------

def pack_bits_ref(flags):
    """flags [P] uint8 (numpy) -> (P + 31) / 32 uint32 words, bit b of word w = flags[32 w + b] != 0, bits past P zero."""
    flags = np.asarray(flags, np.uint8)
    words = (flags.size + 31) // 32
    by = np.packbits(flags != 0, bitorder="little")
    by = np.concatenate([by, np.zeros(4 * words - by.size, np.uint8)])
    return by.view("<u4").astype(np.uint32)


def union_bits_ref(bits_all, P):
    """bits_all [n_ranks, words] uint32 (numpy) -> mask [P] uint8 of 0 / 1: the OR over the ranks, bits past P ignored."""
    r = np.bitwise_or.reduce(np.asarray(bits_all, np.uint32), axis=0)
    by = np.ascontiguousarray(r.astype("<u4")).view(np.uint8)
    return np.unpackbits(by, bitorder="little")[:P].astype(np.uint8)


# ---- Adam ------------------------------------------------------------------------------------------------------------

def adam_ref64(param, grads, lr, beta1=0.9, beta2=0.999, eps=1e-15, exp_avg=None, exp_avg_sq=None, first_step=1):
    """torch.optim.adam._single_tensor_adam (weight_decay 0, amsgrad off) restated in numpy float64, one step per entry of `grads`:
    exp_avg.lerp_(g, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2); denom = sqrt(exp_avg_sq) / sqrt(bc2) + eps;
    param.addcdiv_(exp_avg, denom, value=-lr / bc1). Returns (param, exp_avg, exp_avg_sq) as float64."""
    p = np.array(param, np.float64)
    m = np.zeros_like(p) if exp_avg is None else np.array(exp_avg, np.float64)
    v = np.zeros_like(p) if exp_avg_sq is None else np.array(exp_avg_sq, np.float64)
    for k, g in enumerate(grads):
        g = np.asarray(g, np.float64)
        step = first_step + k
        m = m + (g - m) * (1.0 - beta1)
        v = v * beta2 + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        denom = np.sqrt(v) / np.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
    return p, m, v


def sweep_grads(n, steps, seed):
    """Gradients log-uniform in [1e-30, 1e3] with random signs, fp32, one array per step."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        mag = 10.0 ** rng.uniform(-30.0, 3.0, size=n)
        out.append((mag * rng.choice([-1.0, 1.0], size=n)).astype(np.float32))
    return out


# ---- kNN on an integer lattice ---------------------------------------------------------------------------------------

def lattice_points(N, seed, copies=0):
    """N integer points in [-50, 50]^3 (fp32 holds them and every squared distance exactly); `copies` of them are one point."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(-50, 51, size=(N, 3)).astype(np.int64)
    if copies:
        idx = rng.choice(N, size=copies, replace=False)
        pts[idx] = pts[idx[0]]
    return pts


def knn3_lattice_ref(pts):
    """The fp32 value (d0 + d1 + d2) / 3 of the three smallest squared distances to OTHER points (by index), FLT_MAX terms when
    fewer than three exist. Distances are exact integers; the sum and the division are done in fp32 like the kernel's."""
    pts = np.asarray(pts, np.int64)
    N = pts.shape[0]
    d = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    assert d.max(initial=0) * 3 < (1 << 24)
    t = np.full((N, max(N, 4)), -1, np.int64)
    t[:, :N] = d
    t[np.arange(N), np.arange(N)] = -1                       # the point itself
    terms = np.empty((N, 3), np.float32)
    for i in range(N):
        others = np.sort(t[i][t[i] >= 0])[:3]
        terms[i] = FLT_MAX
        terms[i, :others.size] = others.astype(np.float32)
    with np.errstate(over="ignore"):
        s = (terms[:, 0] + terms[:, 1]).astype(np.float32) + terms[:, 2]
    return (s.astype(np.float32) / np.float32(3)).astype(np.float32)


# ---- photometric loss ------------------------------------------------------------------------------------------------
LOSS_LAMBDA = 0.2
LOSS_SIZES = [(37, 69), (36, 69), (37, 68), (53, 101), (16, 33)]     # (37, 69): exactly one block-uniform interior tile; (36, 69), (37, 68): none
LOSS_WEIGHTS = ["none", "binary", "half"]
LOSS_CASES = [(H, W, "random", wk) for H, W in LOSS_SIZES for wk in LOSS_WEIGHTS] + \
             [(53, 101, "flat", wk) for wk in LOSS_WEIGHTS]          # flat: 1.0 + 1e-3 noise, the cancellation of E[x^2] - mu^2
LOSS_TOL_CAP = 1e-4


def loss_inputs(H, W, kind, wkind):
    """(image, gt, weight or None) as fp32 numpy arrays, seeded by the case."""
    rng = np.random.default_rng(1000 * H + W + (7 if kind == "flat" else 0))
    if kind == "flat":
        gt = (1.0 + 1e-3 * rng.standard_normal((3, H, W))).astype(np.float32)
        img = (1.0 + 1e-3 * rng.standard_normal((3, H, W))).astype(np.float32)
    else:
        gt = rng.random((3, H, W)).astype(np.float32)
        img = np.clip(gt + 0.1 * rng.standard_normal((3, H, W)), 0.0, 1.0).astype(np.float32)
    u = rng.random((H, W))
    weight = {"none": None, "binary": (u > 0.3).astype(np.float32),
              "half": np.where(u < 0.25, 0.0, np.where(u < 0.6, 0.5, 1.0)).astype(np.float32)}[wkind]
    return img, gt, weight


@functools.lru_cache(maxsize=None)
def loss_oracle(H, W, kind, wkind):
    """oracle/loss_oracle.py (fp64) on the case's inputs: dict(loss, l1, ssim, grad). Computed once per case and not modified."""
    import loss_oracle as lo
    img, gt, weight = loss_inputs(H, W, kind, wkind)
    o = lo.photometric_loss(img, gt, LOSS_LAMBDA, weight)
    o["grad"].setflags(write=False)
    return o


def grad_ratio(got, ref):
    """max over elements of |got - ref| / max(|ref|, 1e-2 max|ref|)."""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), 1e-2 * np.abs(ref).max())).max())


@functools.lru_cache(maxsize=None)
def loss_fp32_ratios():
    """{case: grad_ratio of the suite's fp32 restatement (_torch_loss of tests/test_train_ops_gpu.py, CPU autograd) against the
    fp64 oracle}: what an fp32 evaluation of this formula costs on these inputs, the yardstick of the gradient tolerance."""
    from test_train_ops_gpu import _torch_loss
    out = {}
    for case in LOSS_CASES:
        img, gt, weight = loss_inputs(*case)
        x = torch.tensor(img).requires_grad_(True)
        _torch_loss(x, torch.tensor(gt), LOSS_LAMBDA, None if weight is None else torch.tensor(weight)).backward()
        out[case] = grad_ratio(x.grad.numpy(), loss_oracle(*case)["grad"])
    return out


def loss_grad_tolerance():
    """Four times the worst fp32-restatement ratio over LOSS_CASES, never above the project's 1e-4."""
    return min(4.0 * max(loss_fp32_ratios().values()), LOSS_TOL_CAP)


# ---- ctypes call helpers (GPU) ---------------------------------------------------------------------------------------

def lib():
    from multiview_inpaint_amd import _lib
    return _lib.lib()


def last_error():
    return lib().mvi_train_last_error().decode(errors="replace")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def compact_plan(mask_u8):
    """mvi_compact_plan on a uint8 mask: (workspace, count) — the count is the device word the plan wrote, behind the plan."""
    L, P = lib(), mask_u8.numel()
    nbytes = L.mvi_compact_workspace_bytes(P)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=mask_u8.device)
    cnt = ws[nbytes:nbytes + 4].view(torch.int32)
    rc = L.mvi_compact_plan(_ptr(mask_u8), P, _ptr(ws), nbytes, _ptr(cnt), _stream())
    assert rc == 0, last_error()
    return ws, cnt


def compact_table(entries):
    """entries: (in address or tensor or None, out address or tensor, width, packed_stride)."""
    from multiview_inpaint_amd import _lib
    tab = (_lib.CompactTensor * max(len(entries), 1))()
    addr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    for e, (src, dst, w, ps) in zip(tab, entries):
        e.in_, e.out, e.width, e.packed_stride = addr(src), addr(dst), w, ps
    return tab


def compact_gather(entries, P, n_keep, ws):
    return lib().mvi_compact_gather(compact_table(entries), len(entries), P, n_keep, _ptr(ws), _stream())


def compact_window(scatter, entries, P, cnt, first, capacity, ws):
    """mvi_compact_scatter_window / mvi_compact_gather_window; returns the library's return code."""
    L = lib()
    fn = L.mvi_compact_scatter_window if scatter else L.mvi_compact_gather_window
    return fn(compact_table(entries), len(entries), P, _ptr(cnt), first, capacity, _ptr(ws), _stream())


def pack_bits(flags, P, bits):
    return lib().mvi_support_pack_bits(_ptr(flags), P, _ptr(bits), _stream())


def union_bits(bits_all, n_ranks, P, mask):
    return lib().mvi_support_union_bits(_ptr(bits_all), n_ranks, P, _ptr(mask), _stream())


def adam_step(groups, step, beta1=0.9, beta2=0.999, eps=1e-15):
    """groups: (param, grad, exp_avg, exp_avg_sq, lr) of fp32 GPU tensors (views allowed); one mvi_adam_step call."""
    from multiview_inpaint_amd import _lib
    arr = (_lib.AdamGroup * max(len(groups), 1))()
    for k, (p, g, m, v, lr) in enumerate(groups):
        arr[k] = _lib.AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr)
    return lib().mvi_adam_step(arr, len(groups), beta1, beta2, eps, step, _stream())


def loss_fused(img, gt, weight, lam, upstream=1.0):
    """mvi_photometric_loss: (out3, grad)."""
    L = lib()
    H, W = img.shape[1:]
    out3, grad = torch.empty(3, device=img.device), torch.empty_like(img)
    ws = torch.empty(L.mvi_photometric_loss_workspace_bytes(H, W), dtype=torch.uint8, device=img.device)
    rc = L.mvi_photometric_loss(_ptr(img), _ptr(gt), _ptr(weight), H, W, lam, upstream, _ptr(out3), _ptr(grad), _ptr(ws), ws.numel(),
                                _stream())
    assert rc == 0, last_error()
    return out3, grad


def loss_pair(img, gt, weight, w_l1, w_ssim):
    """mvi_photometric_loss_stats, then mvi_photometric_loss_grad2 with the two device weights: (out3, grad)."""
    L = lib()
    H, W = img.shape[1:]
    out3, grad = torch.empty(3, device=img.device), torch.empty_like(img)
    ws = torch.empty(L.mvi_photometric_loss_workspace_bytes(H, W), dtype=torch.uint8, device=img.device)
    rc = L.mvi_photometric_loss_stats(_ptr(img), _ptr(gt), _ptr(weight), H, W, _ptr(out3), _ptr(ws), ws.numel(), _stream())
    assert rc == 0, last_error()
    w2 = torch.tensor([w_l1, w_ssim], dtype=torch.float32, device=img.device)
    rc = L.mvi_photometric_loss_grad2(_ptr(img), _ptr(gt), _ptr(weight), H, W, _ptr(w2), _ptr(grad), _ptr(ws), ws.numel(), _stream())
    assert rc == 0, last_error()
    return out3, grad

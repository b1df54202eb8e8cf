"""Exact-answer tests for the MFMA weight-gradient kernels (csrc/conv3x3_wgrad.hip with its stride-2 form, csrc/conv3t_wgrad.hip,
csrc/linear_wgrad.hip), the counterpart of tests/test_gemm_exact_gpu.py for the forward and dgrad kernels.

Data: x and dy integer-valued in {+-1, +-2, +-3} (exact_gemm_helpers.gen / signs / mags). Every product is an integer of magnitude <= 9
and every partial sum an integer far below 2^24 (at most 9 x 1089 rows here), so fp32 accumulation is exact in any order and any
split: the kernel's output has one right bit pattern, the fp64 formula of the existing helpers cast to fp32. The assertion is
torch.equal, for the default call and for split=False, in bf16 and f16. A dropped, doubled or misplaced slice, or a wrong slice stride
in the second launch that adds the partials, changes an integer.

Shapes: the smallest at which each path can go wrong (see the lists). Every listed shape but the first of each list is split by its
kernel's host policy; the first of each list is the smallest unsplit one, so that each kernel is held to the exact answer on both
routes without relying on split=False alone (asserted through the *_workspace_bytes functions)."""
import functools

import pytest
import torch

import conv3t_bwd_helpers as B3T
import conv_bwd_helpers as B
import exact_gemm_helpers as E
import linear_bwd_helpers as BL
import resample_bwd_helpers as R

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (N, H, W, C_in, C_out): one pixel, unsplit | two one-pixel images, S = 2: the eight outer taps are exactly 0 | two chunks inside one
# image: a tap's halo crosses the chunk and slice boundary; two C_out tiles
CONV3X3 = [(1, 1, 1, 64, 64), (2, 1, 1, 64, 64), (1, 13, 11, 64, 128)]
# (N, H, W, C_in, C_out), H x W the input: unsplit | S = 2 over two images | 72 positions, two chunks in one image
CONV3X3_S2 = [(1, 2, 2, 64, 64), (2, 2, 2, 64, 64), (1, 18, 14, 128, 64)]
# (B, T, S, C_in, C_out): unsplit | T = 1: only the centre tap is non-zero | two videos of two frames | a ragged second chunk of one pixel
CONV3T = [(1, 1, 1, 64, 64), (2, 1, 1, 64, 64), (2, 2, 1, 64, 64), (1, 3, 65, 64, 128)]
# (rows, K, N): one chunk, unsplit | a ragged chunk, S = 2 | S = 16, the XCD-grouped block order | a half-empty last K tile
LINEAR = [(64, 64, 64), (65, 64, 64), (1089, 64, 64), (1089, 192, 64)]


def _id(s):
    return "x".join(map(str, s))


def _hip_ops():
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


def _ints(g, *shape):
    """integers in {+-1, +-2, +-3}, fp64"""
    return E.signs(g, *shape) * E.mags(g, *shape)


def _check_sums(ref):
    assert torch.equal(ref, ref.round()) and ref.abs().max().item() < 2 ** 24
    return ref.float()


def test_every_kernel_has_a_split_and_an_unsplit_case():
    h = _hip_ops()
    for name, fn, shapes in (("conv3x3", h.conv3x3_wgrad_workspace_bytes, CONV3X3), ("conv3x3 s2", h.conv3x3_s2_wgrad_workspace_bytes, CONV3X3_S2),
                             ("conv3t", h.conv3t_wgrad_workspace_bytes, CONV3T), ("linear", h.linear_wgrad_workspace_bytes, LINEAR)):
        ws = [fn(*s) for s in shapes]
        print(f"{name}_wgrad workspace bytes: {dict(zip(map(_id, shapes), ws))}")
        assert ws[0] == 0 and all(b > 0 for b in ws[1:]), (name, ws)
    assert h.conv3x3_wgrad_workspace_bytes(2, 1, 1, 64, 64) == 2 * 64 * 64 * 9 * 4
    assert h.conv3t_wgrad_workspace_bytes(2, 2, 1, 64, 64) == 2 * 64 * 64 * 3 * 4
    assert h.linear_wgrad_workspace_bytes(65, 64, 64) == 2 * (64 * 64 + 64) * 4
    assert h.linear_wgrad_workspace_bytes(1089, 64, 64) == 16 * (64 * 64 + 64) * 4
    assert h.linear_wgrad_workspace_bytes(1089, 192, 64) == 16 * (64 * 192 + 64) * 4


@functools.lru_cache(maxsize=None)
def _conv3x3_case(shape, stride):
    """x [N, C_in, H, W] and dy [N, C_out, H / stride, W / stride] in fp64 and the fp64 formula's dweight as fp32."""
    N, H, W, Ci, Co = shape
    g = E.gen(31, stride, *shape)
    x, dy = _ints(g, N, Ci, H, W), _ints(g, N, Co, H // stride, W // stride)
    ref = B.wgrad_formula(x, dy) if stride == 1 else R.s2_wgrad_formula(x, dy)
    return x, dy, _check_sums(ref)


@pytest.mark.parametrize("tag", list(E.DTYPES))
@pytest.mark.parametrize("shape", CONV3X3, ids=_id)
def test_conv3x3_wgrad_is_exact(shape, tag):
    h = _hip_ops()
    N, H, W, Ci, Co = shape
    x, dy, want = _conv3x3_case(shape, 1)
    xd, dyd = B.tokens(x).to(E.DTYPES[tag]).to(DEV), B.tokens(dy).to(E.DTYPES[tag]).to(DEV)
    for split in (True, False):
        got = h.conv3x3_wgrad(xd, dyd, H, W, split=split).cpu()
        assert torch.equal(got, want), f"conv3x3_wgrad {_id(shape)} {tag} split={split}: {int((got != want).sum())} elements differ"
    if H == 1 and W == 1:                                        # a one-pixel image: only the centre tap sees a pixel
        outer = want.clone()
        outer[:, :, 1, 1] = 0
        assert not outer.any() and want[:, :, 1, 1].any()


@pytest.mark.parametrize("tag", list(E.DTYPES))
@pytest.mark.parametrize("shape", CONV3X3_S2, ids=_id)
def test_conv3x3_s2_wgrad_is_exact(shape, tag):
    h = _hip_ops()
    N, H, W, Ci, Co = shape
    x, dy, want = _conv3x3_case(shape, 2)
    xd, dyd = B.tokens(x).to(E.DTYPES[tag]).to(DEV), B.tokens(dy).to(E.DTYPES[tag]).to(DEV)
    for split in (True, False):
        got = h.conv3x3_s2_wgrad(xd, dyd, H, W, split=split).cpu()
        assert torch.equal(got, want), f"conv3x3_s2_wgrad {_id(shape)} {tag} split={split}: {int((got != want).sum())} elements differ"


@functools.lru_cache(maxsize=None)
def _conv3t_case(shape):
    Bv, T, S, Ci, Co = shape
    g = E.gen(32, *shape)
    x, dy = _ints(g, Bv * T, S, Ci), _ints(g, Bv * T, S, Co)
    return x, dy, _check_sums(B3T.wgrad_formula(x, dy, T))


@pytest.mark.parametrize("tag", list(E.DTYPES))
@pytest.mark.parametrize("shape", CONV3T, ids=_id)
def test_conv3t_wgrad_is_exact(shape, tag):
    h = _hip_ops()
    T = shape[1]
    x, dy, want = _conv3t_case(shape)
    xd, dyd = x.to(E.DTYPES[tag]).to(DEV), dy.to(E.DTYPES[tag]).to(DEV)
    for split in (True, False):
        got = h.conv3t_wgrad(xd, dyd, T, split=split).cpu()
        assert torch.equal(got, want), f"conv3t_wgrad {_id(shape)} {tag} split={split}: {int((got != want).sum())} elements differ"
    if T == 1:                                                   # one frame: the taps before and after it see nothing
        assert not want[:, :, 0].any() and not want[:, :, 2].any() and want[:, :, 1].any()


@functools.lru_cache(maxsize=None)
def _linear_case(shape, strided):
    """x [rows, K], dy [rows, N] in fp64; strided: x the first K columns of a [rows, K + 64] matrix and dy the middle third of a
    [rows, 3 N] one (linear_bwd_helpers.make_rows's layout). dweight and dbias of the fp64 formulas as fp32."""
    rows, K, N = shape
    g = E.gen(33, strided, *shape)
    if strided:
        x, dy = _ints(g, rows, K + 64)[:, :K], _ints(g, rows, 3 * N)[:, N:2 * N]
    else:
        x, dy = _ints(g, rows, K), _ints(g, rows, N)
    return x, dy, _check_sums(BL.dweight_formula(x, dy)), _check_sums(BL.dbias_formula(dy))


def _gpu_view(t, dtype):
    """t in `dtype` on the GPU with t's own strides (a column range of a wider matrix stays one)."""
    if t.is_contiguous():
        return t.to(dtype).to(DEV)
    base = torch.empty(t.untyped_storage().nbytes() // t.element_size(), dtype=t.dtype)
    base.set_(t.untyped_storage(), 0, base.shape)
    return base.to(dtype).to(DEV).as_strided(t.shape, t.stride(), t.storage_offset())


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("tag", list(E.DTYPES))
@pytest.mark.parametrize("shape", LINEAR, ids=_id)
def test_linear_wgrad_is_exact(shape, tag, strided):
    h = _hip_ops()
    x, dy, want_w, want_b = _linear_case(shape, strided)
    xd, dyd = _gpu_view(x, E.DTYPES[tag]), _gpu_view(dy, E.DTYPES[tag])
    assert xd.stride() == x.stride() and dyd.stride() == dy.stride() and torch.equal(dyd.cpu().double(), dy)
    for split in (True, False):
        for need_dbias in (True, False):
            dw, db = h.linear_wgrad(xd, dyd, need_dbias, split=split)
            what = f"linear_wgrad {_id(shape)} {tag}{' strided' if strided else ''} split={split} need_dbias={need_dbias}"
            assert torch.equal(dw.cpu(), want_w), f"{what}: {int((dw.cpu() != want_w).sum())} elements of dweight differ"
            if need_dbias:
                assert torch.equal(db.cpu(), want_b), f"{what}: {int((db.cpu() != want_b).sum())} elements of dbias differ"
            else:
                assert db is None

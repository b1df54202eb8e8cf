"""Bit-exact integer tests of the half-precision MFMA GEMM and convolution kernels (csrc/linear_n320.hip, csrc/ff_geglu.hip,
csrc/stem_conv.hip, forward and as the dgrad kernels of training), and one Gaussian case per plain kernel under a derived ELEMENTWISE
bound. The data, its preconditions, the fp64 references and the case lists are tests/exact_gemm_helpers.py's;
tests/test_gemm_exact_cpu.py shows on the CPU that the comparison used here (torch.equal against ref.to(dtype)) notices a dropped, a
doubled and a misplaced term, a leaking border tap, truncation on the store and a partial sum rounded to the storage type.

Where the rounding set is absent (the helper returns None) the case runs the parity set only: f16 launches without a bias at
K_total < 1280 (their sums stay inside the integers f16 holds exactly), and the bias-free stride-2 dgrad in f16 and at a 64-channel
contraction in bf16."""
import pytest
import torch

import exact_gemm_helpers as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAGS = list(E.DTYPES)
EXACT = ("parity", "rounding")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


def _dev(t, dtype):
    """fp64 holding numbers of `dtype` -> the device tensor (exact)."""
    if t is None:
        return None
    d = t.to(dtype)
    assert torch.equal(d.double(), t)
    return d.to(DEV)


def _bias(b):
    """The kernels take their bias in fp32 (hip_ops._f32): integers up to 2^24 pass unchanged."""
    return None if b is None else b.float().to(DEV)


def _strided(x, dtype, pad=64):
    """x [rows, K] as the first K columns of a [rows, K + pad] device matrix: a view with a longer row stride."""
    wide = torch.zeros(x.shape[0], x.shape[1] + pad, dtype=dtype)
    wide[:, :x.shape[1]] = x.to(dtype)
    v = wide.to(DEV)[:, :x.shape[1]]
    assert not v.is_contiguous() or x.shape[0] == 1
    return v


def _assert_equal(got, want, what):
    """torch.equal(got, want), with the pattern of the wrong elements in the message: which rows and columns, by how much."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    if torch.equal(got, want):
        return
    bad = (got.double() != want.double()) | torch.isnan(got.double())
    idx = bad.nonzero()
    diff = (got.double() - want.double())[bad]
    dims = [sorted(set(idx[:, d].tolist()))[:12] for d in range(idx.shape[1])]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; indices per axis (first 12) {dims}; "
                         f"got - want in [{diff.min().item()}, {diff.max().item()}], first {diff[:8].tolist()} at {idx[:8].tolist()}")


WORST = {}


def _check(case, got, what, dtype):
    """parity / rounding: one right bit pattern. gauss: the derived elementwise bound, no element excluded; prints the worst ratio."""
    if case.kind in EXACT:
        _assert_equal(got, case.want, what)
        return
    got = got.detach().double().cpu()
    assert got.shape == case.ref.shape and torch.isfinite(got).all(), what
    ratio = ((got - case.ref).abs() / case.bound).max().item()
    WORST[what] = ratio
    print(f"elementwise bound, {what}: worst |got - ref| / bound = {ratio:.3f} (K_total {case.K_total})")
    assert ratio <= 1.0, (what, ratio)


def _cases(kinds, tag, build, shapes):
    """(kind, shape, case) of every case that exists."""
    for kind in kinds:
        for shape in shapes:
            case = build(kind, tag, shape)
            assert case is not None or kind == "rounding", (kind, shape)     # (only the rounding set may be absent)
            if case is not None:
                yield kind, shape, case


# ---- the plain projections -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_linear_n320(ops, tag, kinds):
    """rows 1 / 255 / 256 / 257 / 513 x K = 128 / 192 / 256 / 704 (2 chunks, one ring, a wrap by one, an odd wrapping count) x N = 320 /
    640, bias on and off, x contiguous and as a strided view; K = 1280 at 257 rows."""
    dtype = E.DTYPES[tag]
    shapes = E.LINEAR_N320 if kinds == EXACT else E.LINEAR_N320_GAUSS
    for kind, (rows, K, N, wb, strided), c in _cases(kinds, tag, lambda k, t, s: E.linear_case(k, t, *s[:4]), shapes):
        assert ops.linear_n320_supported(K, N, dtype)
        xs = _strided(c.x, dtype) if strided else _dev(c.x, dtype)
        y = ops.linear_n320(xs, _dev(c.w, dtype), _bias(c.b))
        _check(c, y, f"linear_n320 {tag} {kind} rows {rows} K {K} N {N} bias {wb} strided {strided}", dtype)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_linear_k320(ops, tag, kinds):
    """K = 320 into N = 128 (the minimum), 192 (an odd number of 64-wide pairs) and 960 (the packed q | k | v width)."""
    dtype = E.DTYPES[tag]
    shapes = E.LINEAR_K320 if kinds == EXACT else E.LINEAR_K320_GAUSS
    for kind, (rows, N, wb, strided), c in _cases(kinds, tag, lambda k, t, s: E.linear_case(k, t, s[0], 320, s[1], s[2]), shapes):
        assert ops.linear_k320_supported(320, N, dtype)
        xs = _strided(c.x, dtype, 320) if strided else _dev(c.x, dtype)
        y = ops.linear_k320(xs, _dev(c.w, dtype), _bias(c.b))
        _check(c, y, f"linear_k320 {tag} {kind} rows {rows} N {N} bias {wb} strided {strided}", dtype)


# ---- the gated projections -------------------------------------------------------------------------------------------------------------

def _check_gates(c, y, what):
    """Equal where the gate is >= 0 ((v g).to(dtype), and 0 at g = 0); |got| <= 1e-20 where it is negative (the kernels return +-0, the
    true value is below 1e-14 |v g|)."""
    y = y.detach().cpu()
    assert y.shape == c.want.shape and y.dtype == c.want.dtype
    neg_mag = y[c.neg].double().abs()
    assert neg_mag.numel() and neg_mag.max().item() <= 1e-20, (what, neg_mag.max().item())
    _assert_equal(torch.where(c.neg, torch.zeros_like(y), y), c.want, what)


@pytest.mark.parametrize("tag", TAGS)
def test_ff_geglu(ops, tag):
    """K = 320, inner = 64 / 96 / 1280 (2 steps, 3 steps: the two accumulator sets end on the other one, the production width) at
    33 / 256 / 257 rows."""
    dtype = E.DTYPES[tag]
    for rows, inner in E.FF_GEGLU:
        c = E.geglu_case(tag, rows, 320, inner)
        assert ops.ff_geglu_supported(320, inner, dtype)
        y = ops.ff_geglu(_dev(c.x, dtype), _dev(c.w, dtype), _bias(c.b))
        _check_gates(c, y, f"ff_geglu {tag} rows {rows} inner {inner}")


@pytest.mark.parametrize("tag", TAGS)
def test_ff_geglu_n320(ops, tag):
    """K = 128 / 640, inner = 160 / 480 (one and three groups of 160 value + 160 gate columns) at 33 / 257 rows."""
    dtype = E.DTYPES[tag]
    for rows, K, inner in E.FF_GEGLU_N320:
        c = E.geglu_case(tag, rows, K, inner)
        assert ops.ff_geglu_n320_supported(K, inner, dtype)
        y = ops.ff_geglu_n320(_dev(c.x, dtype), _dev(c.w, dtype), _bias(c.b))
        _check_gates(c, y, f"ff_geglu_n320 {tag} rows {rows} K {K} inner {inner}")


@pytest.mark.parametrize("tag", TAGS)
def test_ff_geglu_n320_many_tiles_plain_and_persistent_grid(ops, tag, monkeypatch):
    """257 tiles — more than the chip has CUs — at K = 256 (four chunks: the persistent grid needs an even number >= 4, so at the K = 128
    of the smaller cases both settings would run the plain grid): MVI_N320_PERSIST = 0 and = 1 are both exact."""
    dtype = E.DTYPES[tag]
    rows, K, inner = E.FF_GEGLU_N320_MANY_TILES
    assert -(-rows // 256) * (inner // 160) > 256 and K // 64 >= 4 and (K // 64) % 2 == 0
    c = E.geglu_case(tag, rows, K, inner)
    x, w, b = _dev(c.x, dtype), _dev(c.w, dtype), _bias(c.b)
    for persist in ("0", "1"):
        monkeypatch.setenv("MVI_N320_PERSIST", persist)
        y = ops.ff_geglu_n320(x, w, b)
        torch.cuda.synchronize()
        _check_gates(c, y, f"ff_geglu_n320 {tag} rows {rows} K {K} inner {inner} MVI_N320_PERSIST={persist}")
    monkeypatch.delenv("MVI_N320_PERSIST")


# ---- the add + LayerNorm epilogue ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,tol", [("bf16", 1.0 / 128), ("f16", 1.0 / 1024)])
def test_linear_n320_add_layer_norm_residual_stream_is_exact(ops, tag, tol):
    """Integer x, W, bias, resid and row with every sum a number of the type: s and s_pre equal the fp64 sums bit for bit; y keeps the
    bar of the existing test (LayerNorm is not exact)."""
    dtype = E.DTYPES[tag]
    for rows, K, G, with_resid, ret_pre in E.LINEAR_LN:
        c = E.linear_ln_case(tag, rows, K, G, with_resid, ret_pre)
        what = f"linear_n320_add_layer_norm {tag} rows {rows} K {K} G {G} resid {with_resid} ret_pre {ret_pre}"
        y, s, s_pre = ops.linear_n320_add_layer_norm(_dev(c.x, dtype), _dev(c.w, dtype), _bias(c.b), c.lw.float().to(DEV), c.lb.float().to(DEV),
                                                     1e-5, resid=_dev(c.resid, dtype), row=_dev(c.row, dtype), ret_pre=ret_pre)
        _assert_equal(s, c.want_s, what + " s")
        if ret_pre:
            _assert_equal(s_pre, c.want_s_pre, what + " s_pre")
        else:
            assert s_pre is None
        err = (y.double().cpu() - c.y_ref).abs().max().item()
        assert err <= tol * max(1.0, c.y_ref.abs().max().item()), (what, err)


# ---- the 3x3 convolutions --------------------------------------------------------------------------------------------------------------

def _conv3x3_run(ops, c, dtype, N, H, W, C, Co, stride, up2, split):
    tok = E.tokens(c.x)
    out = ops.conv3x3_n320(_dev(tok, dtype), ops.conv3x3_n320_weight(_dev(c.w, dtype)), _bias(c.b), H, W, stride=stride, split=split, up2=up2)
    torch.cuda.synchronize()
    Ho, Wo = c.ref.shape[2], c.ref.shape[3]
    assert out.shape == (N, Ho * Wo, Co)
    return E.planes(out, Ho, Wo)


def _splits(N, H, W, C, Co, stride):
    from multiview_inpaint_amd import _lib
    return int(_lib.lib().mvi_conv3x3_n320_workspace_bytes(N, H, W, C, Co, stride)) > 0


# which split=True launches really split K (conv_ksplit in csrc/linear_n320.hip: fewer than 128 blocks and 9 C / 64 >= 16 chunks): every
# case at C >= 128 does; the C = 64 cases have 9 chunks and do NOT (named here, asserted below)
CONV3X3_SPLITS = {(1, 1, 1, 64): False, (3, 3, 5, 64): False, (2, 9, 16, 128): True, (1, 16, 17, 192): True}     # (at C_out 320 and 640)
CONV3X3_S2_SPLITS = {(1, 1, 1, 64, 320): False, (2, 7, 9, 128, 320): True, (1, 8, 6, 128, 640): True}


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("k_order", [0, 1])
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_conv3x3_n320_stride_1(ops, tag, k_order, kinds):
    """One pixel; rows that straddle image rows and images inside one wave; a ragged last block; C_out = 320 and 640; both packings of
    the contraction (mvi_conv3x3_n320_k_order); with and without the K split — and whether a split=True launch really split is asserted."""
    from multiview_inpaint_amd import _lib
    dtype = E.DTYPES[tag]
    L = _lib.lib()
    old = int(L.mvi_conv3x3_n320_k_order(-1))
    try:
        assert int(L.mvi_conv3x3_n320_k_order(k_order)) == k_order
        for kind, shape, c in _cases(kinds, tag, lambda k, t, s: E.conv3x3_case(k, t, *s), E.CONV3X3 if kinds == EXACT else E.CONV3X3_GAUSS):
            N, H, W, C, Co = shape
            assert ops.conv3x3_n320_supported(C, Co, dtype)
            for split in (False, True):
                if split:
                    assert _splits(N, H, W, C, Co, 1) == CONV3X3_SPLITS[shape[:4]], shape
                got = _conv3x3_run(ops, c, dtype, N, H, W, C, Co, 1, False, split)
                _check(c, got, f"conv3x3_n320 {tag} {kind} {shape} k_order {k_order} split {split}", dtype)
    finally:
        L.mvi_conv3x3_n320_k_order(old)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_conv3x3_n320_stride_2(ops, tag, kinds):
    """Odd and even image sizes, one pixel, the K split taken at C = 128 (asserted)."""
    dtype = E.DTYPES[tag]
    for kind, shape, c in _cases(kinds, tag, lambda k, t, s: E.conv3x3_case(k, t, *s, 2), E.CONV3X3_S2 if kinds == EXACT else E.CONV3X3_S2_GAUSS):
        N, H, W, C, Co = shape
        for split in (False, True):
            if split:
                assert _splits(N, H, W, C, Co, 2) == CONV3X3_S2_SPLITS[shape], shape
            got = _conv3x3_run(ops, c, dtype, N, H, W, C, Co, 2, False, split)
            _check(c, got, f"conv3x3_n320 stride 2 {tag} {kind} {shape} split {split}", dtype)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_conv3x3_up2_n320(ops, tag, kinds):
    """The convolution of the nearest-neighbour 2x upsampled image: one source pixel, and two 3 x 5 sources. This form is never K-split: the launch sets
    ksplit = 1 whatever workspace it is handed (conv_taps_n320 in csrc/linear_n320.hip), so split=True here does NOT split."""
    dtype = E.DTYPES[tag]
    for kind, shape, c in _cases(kinds, tag, lambda k, t, s: E.conv3x3_case(k, t, *s, 1, True), E.CONV3X3_UP2 if kinds == EXACT else E.CONV3X3_UP2_GAUSS):
        N, H, W, C, Co = shape
        got = _conv3x3_run(ops, c, dtype, N, H, W, C, Co, 1, True, True)
        _check(c, got, f"conv3x3_up2_n320 {tag} {kind} {shape}", dtype)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_conv3x3_s2_dgrad(ops, tag, kinds):
    """dx of the stride-2 convolution on the zero-stuffed source the kernel never builds, against F.conv_transpose2d in fp64: dy of
    2 x 2 and 6 x 10 pixels, contractions over 64 and 128 channels into 320 columns. K_total depends on the pixel's parity (1, 2 or 4
    taps), a multiple of C_out everywhere."""
    dtype = E.DTYPES[tag]
    shapes = E.CONV3X3_S2_DGRAD if kinds == EXACT else E.CONV3X3_S2_DGRAD_GAUSS
    for kind, shape, c in _cases(kinds, tag, lambda k, t, s: E.conv3x3_s2_dgrad_case(k, t, *s), shapes):
        N, h, w, Ci, Co = shape
        assert ops.conv3x3_s2_dgrad_supported(Ci, Co, dtype)
        wt = ops.conv3x3_n320_weight(ops.conv3x3_transposed_weight(_dev(c.w, dtype)))
        out = ops.conv3x3_s2_dgrad(_dev(E.tokens(c.dy), dtype), wt, 2 * h, 2 * w)
        torch.cuda.synchronize()
        assert out.shape == (N, 4 * h * w, Ci)
        _check(c, E.planes(out, 2 * h, 2 * w), f"conv3x3_s2_dgrad {tag} {kind} {shape}", dtype)


# ---- the frame convolution -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_conv3t_n320(ops, tag, kinds):
    """T = 1, 3, 4, 14; frames smaller and larger than a wave's 32 rows; first and last frames of two videos (nothing leaks across
    videos: with +-1 data a leaked frame moves every output of the frame). C_in = 384 and 640 split K — asserted: 3 C / 64 >= 16 chunks,
    the path the Gaussian tests of this kernel never reach."""
    from multiview_inpaint_amd import _lib
    dtype = E.DTYPES[tag]
    L = _lib.lib()
    for kind, shape, c in _cases(kinds, tag, lambda k, t, s: E.conv3t_case(k, t, *s), E.CONV3T if kinds == EXACT else E.CONV3T_GAUSS):
        B, T, S, C, Co = shape
        assert (int(L.mvi_conv3t_n320_workspace_bytes(B, T, S, C, Co)) > 0) == (C >= 384), shape
        for split in (False, True):
            out = ops.conv3t_n320(_dev(c.tok, dtype), ops.conv3t_n320_weight(_dev(c.w, dtype)), _bias(c.b), T, split=split)
            torch.cuda.synchronize()
            _check(c, out, f"conv3t_n320 {tag} {kind} {shape} split {split}", dtype)


# ---- the stem convolution --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kinds", [EXACT, ("gauss",)], ids=["exact", "gauss"])
def test_stem_conv3x3_without_silu(ops, tag, kinds):
    """7 -> 16, 16 -> 16, 20 -> 32, 32 -> 32, 8 -> 320 at stride 1 and 5 -> 32, 16 -> 32 at stride 2; one 4 x 64 tile, ragged tiles and
    borders (9 x 72, 5 x 136; 9 x 80, 5 x 144 at stride 2, which takes W % 16 == 0 only). The channel padding happens in the kernel. Odd
    C_in: an odd bias, see exact_gemm_helpers.stem_case."""
    dtype = E.DTYPES[tag]
    for kind, shape, c in _cases(kinds, tag, lambda k, t, s: E.stem_case(k, t, *s), E.STEM if kinds == EXACT else E.STEM_GAUSS):
        N, Ci, Co, H, W, stride = shape
        y = ops.stem_conv3x3_silu(_dev(c.x, dtype), _dev(c.w, dtype), _bias(c.b), silu=False, stride=stride)
        torch.cuda.synchronize()
        _check(c, y, f"stem_conv3x3 {tag} {kind} {shape}", dtype)


# ---- the dgrad entry points: the forward kernels on transposed weights -----------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_dgrad_entry_points_against_the_fp64_adjoint(ops, tag):
    """One parity case each: the weight transposition and packing (conv3x3_transposed_weight, conv3t_transposed_weight,
    stem_conv3x3_transposed_weight) bit for bit."""
    dtype = E.DTYPES[tag]
    for (rows, K, N), which in zip(E.LINEAR_DGRAD, ("k320", "n320")):           # forward x [rows, K] -> [rows, N]: dx = dy W
        c = E.linear_case("parity", tag, rows, N, K, False, 1)                  # x = dy [rows, N], w = W^T [K, N]
        assert ops.linear_dgrad_kernel(K, N, dtype) == which
        _check(c, ops.linear_dgrad(_dev(c.x, dtype), _dev(c.w, dtype)), f"linear_dgrad {tag} {(rows, K, N)} on {which}", dtype)
    N, H, W, Ci, Co = E.CONV3X3_DGRAD
    c = E.conv3x3_dgrad_case(tag, N, H, W, Ci, Co)
    wt = ops.conv3x3_n320_weight(ops.conv3x3_transposed_weight(_dev(c.w, dtype)))
    assert _splits(N, H, W, Co, Ci, 1)                                          # 9 * 128 / 64 = 18 chunks in one block: split=True splits
    for split in (False, True):
        out = ops.conv3x3_dgrad(_dev(E.tokens(c.dy), dtype), wt, H, W, split=split)
        _check(c, E.planes(out, H, W), f"conv3x3_dgrad {tag} {E.CONV3X3_DGRAD} split {split}", dtype)
    B, T, S, Ci, Co = E.CONV3T_DGRAD
    c = E.conv3t_dgrad_case(tag, B, T, S, Ci, Co)
    wt = ops.conv3t_n320_weight(ops.conv3t_transposed_weight(_dev(c.w, dtype)))
    from multiview_inpaint_amd import _lib
    assert int(_lib.lib().mvi_conv3t_n320_workspace_bytes(B, T, S, Co, Ci)) == 0      # 3 * 128 / 64 = 6 chunks: split=True does NOT split
    for split in (False, True):
        _check(c, ops.conv3t_dgrad(_dev(c.dy, dtype), wt, T, split=split), f"conv3t_dgrad {tag} {E.CONV3T_DGRAD} split {split}", dtype)
    for shape in E.STEM_DGRAD:
        c = E.stem_dgrad_case(tag, *shape)
        _check(c, ops.stem_conv3x3_dgrad(_dev(c.dz, dtype), _dev(c.w, dtype)), f"stem_conv3x3_dgrad {tag} {shape}", dtype)

"""Exact-answer tests of the split-operand first-stage convolutions (csrc/linear_n320.hip: mvi_conv3x3_split3_f32, mvi_conv3t_split3_f32,
mvi_conv3x3_s2_split3_f32 behind hip_ops.conv_split3 / conv_split3_s2) and of their operand producer (csrc/groupnorm_tokens.hip,
gt_apply_split_kernel<0|1|2> behind hip_ops.group_norm_split). The data, its preconditions, the fp64 references and the case lists are
tests/split3_exact_helpers.py's; tests/test_split3_exact_cpu.py shows on the CPU what the comparisons used here reject.

Convolutions: mixed-scale operands (hi of size 1, lo of size 2^-10) whose three kept terms x_hi . w_hi + x_hi . w_lo + x_lo . w_hi sum
exactly in fp32 in any order — torch.equal against the one right fp32 output; integer operands in the one-value modes "bf16" / "f16";
Gaussian operands under the derived elementwise bound 2 K_total 2^-24 sum|terms| against the three-term fp64 sum. Every batch also cut
to one image per launch; the stride-2 form also against the stride-1 answer at [1::2, 1::2]; stores past the padded rows through the
C ABI.

Producer: the plain split (num_groups = 0) of planted fp32 bit patterns against the split on the bit pattern (ties of both parities,
their neighbours, values that round into the next binade, +-0 — compared by value: torch.equal takes -0 for +0 —, lo a bf16
subnormal); the normalising form against the fp64 GroupNorm of tests/norm_exact_helpers.py, elementwise, hi a nearest bf16 number of
hi + lo on every element, the constant group bit for bit.

On an MI355X (profiles/split3_exact_gpu.txt, one line per launch): equality held on every case of the three entry points, both exact
sets — the matrix pipe's accumulate keeps terms of size 1 and 2^-10 below 2^24 units, up to 0.28 x 2^24 (unit, 9 x 512) and 0.46 x 2^24 (mags, 9 x 128) —,
whole and cut to one image per launch, in contraction order 1; the Gaussian cases stay below 0.004 of their bound (it is
K_total-fold wider than what the kernel loses); the producer's worst ratios are 0.85 (hi + lo), 0.999 (bf16) and 0.997 (f16),
rounding-limited, and |lo| reaches exactly half an ulp (the tie the nearest-number check allows)."""
import ctypes as C

import pytest
import torch

import exact_gemm_helpers as E
import norm_exact_helpers as NH
import split3_exact_helpers as S
import svd_helpers as SH

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
MODES = {"split3": BF16, "bf16": BF16, "f16": torch.float16}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    """MVI_STRICT for every test of this module: a GPU tensor that would leave the HIP path raises (svd/ops.py)."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)


@pytest.fixture(autouse=True)
def _nothing_runs_on_a_faulted_device():
    """A device fault is sticky: the run ends with the test that met it instead of launching the rest of the module on that device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is launched: {e}", returncode=3)


def _dev(t, dtype):
    """fp64 holding numbers of `dtype` -> the device tensor (exact)."""
    d = t.to(dtype)
    assert torch.equal(d.double(), t)
    return d.to(DEV)


def _assert_exact(got, want, what, rows_per_image):
    """torch.equal(got, want) on [rows, C_out] fp32, with the pattern of the wrong elements in the message: which rows, columns and
    images, and by how many units of 2^-10."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype)
    if torch.equal(got, want):
        return
    d = got.double() - want.double()
    bad = (d != 0) | torch.isnan(d)
    idx = bad.nonzero()
    first = lambda v: sorted(set(v.tolist()))[:12]
    units = d[bad] / S.U
    whole = bool((units == units.round()).all())
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; rows (first 12) {first(idx[:, 0])}, columns {first(idx[:, 1])}, "
                         f"images {first(idx[:, 0] // rows_per_image)}; got - want in units of 2^-10 in [{units.min().item()}, {units.max().item()}] "
                         f"({'whole units' if whole else 'NOT whole units'}), first {units[:8].tolist()} at {idx[:8].tolist()}")


def _x2(c):
    """(x_hi | x_lo) bf16 [input rows, 2 C], built on the CPU."""
    return _dev(torch.cat([c.xh.reshape(-1, c.C), c.xl.reshape(-1, c.C)], dim=1), BF16)


def _w3(ops, c):
    """split3_weight of the fp32 weight w_hi + w_lo — which has to be (w_hi | w_lo | w_hi) in the kernel's contraction order, padding
    rows zero, element for element (pack_w3 writes the layout out independently)."""
    group = int(ops._lib.lib().mvi_conv_split3_group(c.Co))
    w3 = ops.split3_weight(c.w32.to(DEV))
    want = S.pack_w3((c.wh, c.wl, c.wh), c.taps, ops.conv3x3_k_order(), group)
    assert w3.dtype == BF16 and w3.shape == want.shape and torch.equal(w3.cpu().double(), want), f"split3_weight {c.geom} {c.shape}"
    assert want.shape[0] % group == 0 and not want[c.Co:].any()
    return w3


def _w1(ops, c, mode):
    group = int(ops._lib.lib().mvi_conv_split3_group(c.Co))
    w1 = ops.split3_weight(c.w.float().to(DEV), mode)
    assert w1.dtype == MODES[mode] and torch.equal(w1.cpu().double(), S.pack_w3((c.w,), c.taps, ops.conv3x3_k_order(), group))
    return w1


def _run(ops, c, x, w, mode, **kw):
    n, a, b = c.dims
    if c.geom == "s2":
        out = ops.conv_split3_s2(x, w, n, a, b, c.Co, mode=mode, **kw)
    else:
        out = ops.conv_split3(x, w, n, a, b, c.Co, taps=c.taps, mode=mode, **kw)
    torch.cuda.synchronize()
    assert out.shape == (c.rows, c.Co) and out.dtype == torch.float32
    return out


def _launches(ops, c, x, w, mode):
    """(what, output) of the whole batch in one launch and, with more than one image / video, cut to one per launch."""
    n, a, b = c.dims
    yield "", _run(ops, c, x, w, mode)
    if n > 1:
        yield " cut to one image per launch", _run(ops, c, x, w, mode, _max_bytes=a * b * x.shape[1] * 2)


def _convolution(ops, geom, shape):
    """Every data set of one case: unit, mags (where it exists), gauss, and the integers in modes "bf16" and "f16"."""
    n, a, b, Cc, Co = shape
    Ho, Wo = S.out_hw(geom, a, b)
    per_image = (Ho * Wo) if geom != "conv3t" else a * b
    entry = {"conv9": "conv3x3_split3_f32", "conv3t": "conv3t_split3_f32", "s2": "conv3x3_s2_split3_f32"}[geom]
    for kind in S.KINDS:
        c = S.conv_case(geom, kind, shape)
        if c is None:
            assert kind == "mags" and (geom, shape) in S.MAGS_ABSENT
            SH.report(f"{entry} {shape} mags: absent (past 2^24 units), the unit set runs alone")
            continue
        x2, w3 = _x2(c), _w3(ops, c)
        for cut, got in _launches(ops, c, x2, w3, "split3"):
            what = f"{entry} {shape} {kind}{cut}"
            if kind in S.EXACT:
                _assert_exact(got, c.want, what, per_image)
                SH.report(f"{what}: torch.equal held (K_total {c.K_total}, sum|terms| up to {c.abs_ref.max().item() / S.U / 2 ** 24:.3f} x 2^24 units)")
            else:
                g = got.double().cpu()
                assert torch.isfinite(g).all(), what
                ratio = ((g - c.ref).abs() / c.bound).max().item()
                SH.report(f"{what}: worst |got - ref3| / bound = {ratio:.4f} (K_total {c.K_total})")
                assert ratio <= 1.0, (what, ratio)
        if geom == "s2" and kind in S.EXACT:
            # the same operands through the stride-1 answer: conv(pad(x, (0, 1, 0, 1)), stride 2) == conv(x, padding 1)[1::2, 1::2]
            full = S.conv_case("conv9", kind, shape)
            assert torch.equal(full.want.reshape(n, a, b, Co)[:, 1::2, 1::2].reshape(-1, Co), c.want)
            _assert_exact(_run(ops, full, x2, w3, "split3").view(n, a, b, Co)[:, 1::2, 1::2].reshape(-1, Co), c.want,
                          f"conv3x3_split3_f32 {shape} {kind} at [1::2, 1::2]", per_image)
    for mode in ("bf16", "f16"):
        c = S.int_case(geom, mode, shape)
        x, w = _dev(c.x.reshape(-1, Cc), MODES[mode]), _w1(ops, c, mode)
        for cut, got in _launches(ops, c, x, w, mode):
            what = f"{entry} {shape} integers in mode {mode}{cut}"
            _assert_exact(got, c.want, what, per_image)
            SH.report(f"{what}: torch.equal held")


@pytest.mark.parametrize("shape", S.CONV9, ids=str)
def test_conv3x3_split3(ops, shape):
    _convolution(ops, "conv9", shape)


@pytest.mark.parametrize("shape", S.CONV3T, ids=str)
def test_conv3t_split3(ops, shape):
    _convolution(ops, "conv3t", shape)


@pytest.mark.parametrize("shape", S.S2, ids=str)
def test_conv3x3_s2_split3(ops, shape):
    _convolution(ops, "s2", shape)


def test_which_contraction_order_ran(ops):
    """conv3x3_k_order() is part of every packed weight above (pack_w3 takes it): the order this process ran is reported, not flipped."""
    k = ops.conv3x3_k_order()
    assert k in (0, 1)
    SH.report(f"conv3x3_k_order() = {k} ({'[C / 64][9 taps][64 channels]' if k == 1 else 'tap-major'}) for every 3x3 case of this module")


@pytest.mark.parametrize("geom,shape", [("conv9", (3, 5, 7, 64, 128)), ("conv3t", (2, 2, 7, 64, 64)), ("s2", (2, 5, 7, 64, 128))], ids=str)
def test_nothing_is_stored_past_the_padded_rows(ops, geom, shape):
    """Through the C ABI: out has mvi_conv_split3_out_rows(rows) rows (whole 256-row blocks are stored) and 8 sentinel rows behind
    them. The sentinels are untouched, the first `rows` rows exact."""
    L = ops._lib.lib()
    c = S.conv_case(geom, "unit", shape)
    n, a, b = c.dims
    x2, w3 = _x2(c), _w3(ops, c)
    cap = int(L.mvi_conv_split3_out_rows(c.rows))
    assert cap >= c.rows and cap % 256 == 0
    out = torch.full((cap + 8, c.Co), 7.5, dtype=torch.float32, device=DEV)
    fn = {"conv9": L.mvi_conv3x3_split3_f32, "conv3t": L.mvi_conv3t_split3_f32, "s2": L.mvi_conv3x3_s2_split3_f32}[geom]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = fn(x2.data_ptr(), w3.data_ptr(), out.data_ptr(), n, a, b, c.C, c.Co, 3, 1, cap, st)            # terms 3, MVI_DT_BF16
    assert rc == 0, L.mvi_unet_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out[cap:] == 7.5).all()), f"{geom} {shape}: a sentinel row behind the {cap} padded rows was written"
    Ho, Wo = S.out_hw(geom, a, b)
    _assert_exact(out[:c.rows], c.want, f"{geom} {shape} through the C ABI", Ho * Wo if geom != "conv3t" else a * b)


# ---- the operand producer ------------------------------------------------------------------------------------------------------------------

def _block_rows(ops, Cc):
    """Rows one block of gt_apply_split_kernel covers: kGtPasses x gt_rows_per_pass(C / 4) = 8 x min(8, 512 / (C / 4)) (csrc/groupnorm_tok.h)
    — 64 at C = 64, 48 at C = 320 —, confirmed by the host function that sizes the statistics' partials with the same geometry."""
    rows = 8 * max(1, min(8, 512 // (Cc // 4)))
    assert rows == {64: 64, 320: 48}[Cc]
    L, dt = ops._lib.lib(), ops._DT[torch.float32]
    one = L.mvi_groupnorm_tok2tok_workspace_bytes(1, Cc, 1, 32, dt)
    assert one != 0 and L.mvi_groupnorm_tok2tok_workspace_bytes(1, Cc, rows, 32, dt) == one != L.mvi_groupnorm_tok2tok_workspace_bytes(1, Cc, rows + 1, 32, dt)
    return rows


@pytest.mark.parametrize("Cc", [64, 320])
def test_plain_split_of_planted_values(ops, Cc):
    """num_groups = 0, all three modes, one row, a block less one row and a block and a row: both halves against the split on the bit
    pattern (mode "f16": x.to(torch.float16)), by torch.equal."""
    rows = _block_rows(ops, Cc)
    for S_ in (1, rows - 1, rows + 1):
        v = S.probe_values(S.gen(45, S_, Cc), S_, Cc)
        hi, lo, _ = S.bit_split(v.double())
        assert torch.isfinite(hi).all()
        want = {"split3": torch.cat([hi, lo], dim=2).to(BF16), "bf16": hi.to(BF16), "f16": v.to(torch.float16)}
        for mode, w in want.items():
            got = ops.group_norm_split(v.to(DEV), 0, None, None, 0.0, False, mode=mode)
            torch.cuda.synchronize()
            got = got.cpu()
            assert got.dtype == w.dtype and got.shape == w.shape
            bad = (got != w) & ~(torch.isnan(got.float()) & torch.isnan(w.float()))
            what = f"group_norm_split plain {(1, S_, Cc)} mode {mode}"
            SH.report(f"{what}: torch.equal {'held' if not bad.any() else 'FAILED'}")
            if bad.any():
                i = bad.nonzero()[:8]
                src = v.view(torch.int32)[0][i[:, 1], i[:, 2] % Cc].tolist()
                raise AssertionError(f"{what}: {int(bad.sum())} elements differ; first at {i.tolist()}, inputs {[hex(s & 0xFFFFFFFF) for s in src]}, "
                                     f"got {got[bad][:8].tolist()}, want {w[bad][:8].tolist()}")
            assert torch.equal(got, w)


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("N,Cc,S_", NH.GN_ISSUE_SHAPES)
def test_group_norm_split_elementwise(ops, N, Cc, S_, frames):
    """The normalising form on norm_exact_helpers.gn_case("f32", ..) (N videos of `frames` frames), SiLU and chan_bias on and off. Modes
    1 / 2: |got - ref| <= cap + ulp(|ref| + cap) / 2 in bf16 / f16, cap = norm_cap's. Mode 0: |hi + lo - ref| <= cap + 2^-17 (|ref| + cap)
    — lo is an 8-bit rounding of a residue of at most half an ulp of hi, 2^-8 2^-9 of the value —, and hi is a nearest bf16 number of
    hi + lo on every element (|lo| <= half the bf16 spacing at hi + lo; a tie may fall either way: lo can round up onto the half ulp).
    Without SiLU the constant group has one right output: the split of bias[c]."""
    Nt = N * frames
    for silu in (True, False):
        for with_cb in (True, False):
            c = NH.gn_case("f32", Nt, Cc, S_, 32, frames, with_cb, silu)
            x = c.x.transpose(1, 2).contiguous().float().to(DEV)
            ref, cap, const = c.ref.transpose(1, 2), c.cap.transpose(1, 2), c.const.transpose(1, 2)
            par = lambda t: None if t is None else t.float().to(DEV)
            b_hi, b_lo, _ = S.bit_split(c.b)
            for mode, dt in MODES.items():
                what = f"group_norm_split {(Nt, S_, Cc)} frames={frames} silu={silu} cb={with_cb} mode {mode}"
                y = ops.group_norm_split(x, 32, par(c.w), par(c.b), c.eps, silu, chan_bias=par(c.cb), frames=frames, mode=mode)
                torch.cuda.synchronize()
                y = y.cpu()
                assert y.dtype == dt and torch.isfinite(y.float()).all(), what
                if mode == "split3":
                    hi, lo = y[..., :Cc].double(), y[..., Cc:].double()
                    s = hi + lo
                    bnd = cap + 2.0 ** -17 * (ref.abs() + cap)
                    ratio = ((s - ref).abs() / bnd).max().item()
                    near = (lo.abs() / (0.5 * E.ulp_of(s, BF16))).max().item()
                    SH.report(f"{what}: worst |hi + lo - ref| / bound = {ratio:.3f}; worst |lo| / half a bf16 ulp of hi + lo = {near:.3f}")
                    assert ratio <= 1.0 and near <= 1.0, (what, ratio, near)
                    want_const = (b_hi.expand_as(hi)[const], b_lo.expand_as(lo)[const])
                    got_const = (hi[const], lo[const])
                else:
                    bnd = NH.bound(ref, cap, dt)
                    ratio = ((y.double() - ref).abs() / bnd).max().item()
                    SH.report(f"{what}: worst |got - ref| / bound = {ratio:.3f}")
                    assert ratio <= 1.0, (what, ratio)
                    want_const = (c.b.to(dt).double().expand_as(ref)[const],)
                    got_const = (y.double()[const],)
                if not silu:
                    for g_, w_ in zip(got_const, want_const):
                        assert g_.numel() and torch.equal(g_, w_), (what, "constant group", int((g_ != w_).sum()), g_.numel())

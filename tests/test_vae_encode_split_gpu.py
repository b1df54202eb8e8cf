"""The first-stage ENCODER at fp32 accuracy on the bf16 matrix pipe (svd/vae_split.py encode; opt-in through
svd/vae.py encode_first_stage(mode="split3") / MVI_VAE_ENCODE=split3): the stride-2 split-operand convolution of Downsample
(mvi_conv3x3_s2_split3_f32), conv_in as an fp32 stem that writes token rows (mvi_conv3x3_small_cin_f32_tokens), the walk on a small
and on the full-size encoder, and the public entry. fp32 contract: 1e-4 relative, as tests/test_vae_gpu.py.
The max-norm bars here are on Gaussian data; the exact-answer tests of the three split-operand convolutions (one right fp32 bit pattern
per output, borders, padded column groups, the stride-2 origin) and of the split hi / lo producer are tests/test_split3_exact_gpu.py,
on the data of tests/split3_exact_helpers.py (tests/test_split3_exact_cpu.py shows what those comparisons reject)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import svd_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    """MVI_STRICT for every test of this module: a GPU tensor that would leave the HIP path raises (svd/ops.py)."""
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


def _down_ref(x_tok, w, N, Hh, W):
    """fp64 Downsample.conv of token-major x [N, H W, C] -> [N, Ho Wo, C_out]."""
    xp = F.pad(x_tok.double().view(N, Hh, W, -1).permute(0, 3, 1, 2), (0, 1, 0, 1))
    y = F.conv2d(xp, w.double(), stride=2)
    return y.permute(0, 2, 3, 1).reshape(N, y.shape[2] * y.shape[3], -1)


@pytest.mark.parametrize("N,Hh,W,Cc,Co", [(2, 24, 32, 128, 128), (3, 9, 15, 64, 320), (1, 40, 33, 256, 512), (2, 16, 16, 512, 256),
                                          (1, 2, 2, 64, 64), (5, 6, 10, 128, 256)])
def test_stride2_split_operand_convolution(ops, N, Hh, W, Cc, Co):
    """mvi_conv3x3_s2_split3_f32 behind hip_ops.conv_split3_s2: 3x3 / stride 2 over F.pad(x, (0, 1, 0, 1)) with split operands, rows =
    output pixels. Against fp64 on the same fp32 operands (3e-5, the bar of the stride-1 entry: the same arithmetic); bit-equal to the
    stride-1 entry sampled at [1::2, 1::2] (same contraction and chunk order per output pixel: anything else is a border or addressing
    error); bit-equal when cut to one image per launch; image 0 of the batch equals the call on image 0 alone; the one-value modes
    against fp64 on the rounded operands (5e-6)."""
    g = torch.Generator().manual_seed(N * 1000 + Hh * 10 + Cc + 9)
    x = torch.randn(N, Hh * W, Cc, generator=g) * torch.rand(1, 1, Cc, generator=g).mul(3).add(0.2)      # channels of different scales
    w = torch.randn(Co, Cc, 3, 3, generator=g) * (9 * Cc) ** -0.5
    Ho, Wo = (Hh - 2) // 2 + 1, (W - 2) // 2 + 1
    want = _down_ref(x, w, N, Hh, W)
    assert want.shape == (N, Ho * Wo, Co)
    xd = x.to(DEV)
    for mode, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        x1 = ops.group_norm_split(xd, 0, None, None, 0.0, False, mode=mode)
        g1 = ops.conv_split3_s2(x1.reshape(-1, Cc), ops.split3_weight(w.to(DEV), mode), N, Hh, W, Co, mode=mode).view(N, Ho * Wo, Co)
        e1 = rel(g1, _down_ref(x.to(dt), w.to(dt), N, Hh, W))
        print(f"stride-2 {mode}: {e1:.2e}")
        assert e1 < 5e-6, (mode, e1)
    x2 = ops.group_norm_split(xd, 0, None, None, 0.0, False).reshape(-1, 2 * Cc)
    w3 = ops.split3_weight(w.to(DEV))
    got = ops.conv_split3_s2(x2, w3, N, Hh, W, Co).view(N, Ho * Wo, Co)
    torch.cuda.synchronize()
    e = rel(got, want)
    print(f"stride-2 split3 {(N, Hh, W, Cc, Co)}: {e:.2e}")
    assert e < 3e-5, e
    full = ops.conv_split3(x2, w3, N, Hh, W, Co).view(N, Hh, W, Co)
    assert torch.equal(got, full[:, 1::2, 1::2].reshape(N, Ho * Wo, Co))
    if N > 1:
        cut = ops.conv_split3_s2(x2, w3, N, Hh, W, Co, _max_bytes=Hh * W * 4 * Cc).view(N, Ho * Wo, Co)
        assert torch.equal(cut, got)
    one = ops.conv_split3_s2(x2[:Hh * W].contiguous(), w3, 1, Hh, W, Co).view(Ho * Wo, Co)
    assert torch.equal(one, got[0])


def test_stride2_split_operand_convolution_rejects_bad_arguments(ops):
    """Every rejection of mvi_conv3x3_s2_split3_f32 is a negative status with a message, and nothing is launched: the output, filled
    with a sentinel, is untouched."""
    L = ops._lib.lib()
    N, Hh, W, Cc, Co = 1, 4, 6, 64, 64
    x2 = torch.zeros(N * Hh * W + 8, 2 * Cc, dtype=torch.bfloat16, device=DEV)
    w3 = ops.split3_weight(torch.zeros(Co, Cc, 3, 3, device=DEV))
    cap = int(L.mvi_conv_split3_out_rows(6))
    out = torch.full((cap + 8, Co), 7.5, dtype=torch.float32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    BF16, F16, F32 = 1, 2, 0

    def call(x=x2.data_ptr(), wgt=w3.data_ptr(), o=out.data_ptr(), H_=Hh, W_=W, C_=Cc, Co_=Co, terms=3, dtype=BF16, cap_=cap):
        return L.mvi_conv3x3_s2_split3_f32(x, wgt, o, N, H_, W_, C_, Co_, terms, dtype, cap_, st)
    assert call() == 0                                             # the arguments the rejections below vary are valid
    torch.cuda.synchronize()
    assert not bool((out[:6] == 7.5).any())
    out.fill_(7.5)
    bad = {"H < 2": dict(H_=1), "W < 2": dict(W_=1), "C % 64": dict(C_=96), "C_out % 16": dict(Co_=72), "terms 2": dict(terms=2),
           "split operands in f16": dict(terms=3, dtype=F16), "fp32 operands": dict(terms=1, dtype=F32), "short out": dict(cap_=cap - 1),
           "NULL x2": dict(x=None), "NULL weight": dict(wgt=None), "NULL out": dict(o=None), "misaligned x2": dict(x=x2.data_ptr() + 2),
           "misaligned weight": dict(wgt=w3.data_ptr() + 8), "misaligned out": dict(o=out.data_ptr() + 4)}
    for name, kw in bad.items():
        rc = call(**kw)
        msg = L.mvi_unet_last_error().decode()
        assert rc < 0 and "conv3x3_s2_split3_f32" in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())
    with pytest.raises(ValueError):
        ops.conv_split3_s2(x2[:Hh * W], w3, 1, 1, Hh * W, Co)


@pytest.mark.parametrize("N,Ci,Hh,W,Co", [(2, 3, 9, 15, 128), (1, 3, 64, 96, 128), (3, 4, 5, 7, 64), (1, 1, 2, 2, 128)])
def test_stem_writes_fp32_tokens(ops, N, Ci, Hh, W, Co):
    """mvi_conv3x3_small_cin_f32_tokens: conv2d(x, w, b, padding=1) of fp32 planes as token rows, exact fp32 FMA chains. Elementwise
    against fp64; the bound is derived, not measured: 9 C_in <= 27 products and the bias, each rounded once (the product inside an FMA
    not at all) -> |got - want| <= 28 * 2^-24 * (conv(|x|, |w|) + |b|)."""
    g = torch.Generator().manual_seed(N * 100 + Ci * 10 + Hh + Co)
    x = torch.randn(N, Ci, Hh, W, generator=g) * 1.5
    conv = torch.nn.Conv2d(Ci, Co, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5)
        conv.bias.copy_(torch.randn(Co, generator=g) * 0.3)
    wd, bd = conv.weight.detach().double(), conv.bias.detach().double()
    want = F.conv2d(x.double(), wd, bd, padding=1).permute(0, 2, 3, 1).reshape(N, Hh * W, Co)
    mag = F.conv2d(x.double().abs(), wd.abs(), bd.abs(), padding=1).permute(0, 2, 3, 1).reshape(N, Hh * W, Co)
    conv = conv.to(DEV)
    assert ops.conv_in_f32_tokens_supported(conv, x.to(DEV))
    got = ops.conv_in_f32_tokens(x.to(DEV), conv)
    torch.cuda.synchronize()
    assert got.shape == (N, Hh * W, Co) and got.dtype == torch.float32
    ratio = float(((got.double().cpu() - want).abs() / (28 * 2.0 ** -24 * mag)).max())
    print(f"stem {(N, Ci, Hh, W, Co)}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_stem_rejects_unsupported_channels(ops):
    L = ops._lib.lib()
    assert L.mvi_conv3x3_small_cin_f32_tokens_supported(3, 128) and L.mvi_conv3x3_small_cin_f32_tokens_supported(4, 64)
    assert not L.mvi_conv3x3_small_cin_f32_tokens_supported(5, 128) and not L.mvi_conv3x3_small_cin_f32_tokens_supported(3, 6)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for Ci, Co in ((5, 128), (3, 6)):
        x = torch.zeros(1, Ci, 4, 4, device=DEV)
        w = torch.zeros(Co, Ci, 3, 3, device=DEV)
        out = torch.full((16, Co), 7.5, device=DEV)
        rc = L.mvi_conv3x3_small_cin_f32_tokens(x.data_ptr(), w.data_ptr(), None, out.data_ptr(), 1, Ci, 4, 4, Co, st)
        assert rc < 0 and "conv3x3_small_cin_f32_tokens" in L.mvi_unet_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == 7.5).all())
        conv = torch.nn.Conv2d(Ci, Co, 3, padding=1).to(DEV)
        assert not ops.conv_in_f32_tokens_supported(conv, x)
        with pytest.raises(ValueError):
            ops.conv_in_f32_tokens(x, conv)


SMALL_ENC = dict(ch=64, ch_mult=[1, 2, 2], num_res_blocks=1, z_channels=4, double_z=True, in_channels=3, resolution=32,
                 attn_resolutions=[], out_ch=3)
SMALL_HW = (18, 30)                                  # levels 18x30 -> 9x15 -> 4x7: the second Downsample sees odd H and W; mid attention S = 28


@pytest.fixture(scope="module")
def small_encoder():
    """(encoder on the CPU, frames, its fp32 CPU moments) — computed once, shared, never modified."""
    from multiview_inpaint_amd.svd import vae
    enc = vae.Encoder(**SMALL_ENC).eval()
    enc.load_state_dict(H.seeded_state_dict(enc, 71), strict=True)
    x = H.vae_inputs(72, T=3, hw=SMALL_HW)
    with torch.no_grad():
        want = enc(x)
    return enc, x, want


def test_small_encoder_walk_matches_the_module(ops, small_encoder):
    """vae_split.encode against the SAME module run on the CPU in fp32: 1e-4, the module's contract."""
    import copy
    from multiview_inpaint_amd.svd import vae, vae_split
    enc_cpu, x, want = small_encoder
    enc = copy.deepcopy(enc_cpu).to(DEV)
    xd = x.to(DEV)
    assert want.shape == (3, 8, 4, 7)
    ops.PROFILE = []
    try:
        with torch.no_grad():
            assert vae_split.encoder_applies(enc, xd)
            got = vae_split.encode(enc, xd)
        torch.cuda.synchronize()
        kinds = set(k for k, *_ in ops.PROFILE)
    finally:
        ops.PROFILE = None
    e = rel(got, want)
    H.report(f"small encoder (ch 64, 3 frames of 18x30) on the split walk against the module on the CPU: relative max error {e:.2e} (bar 1e-4)")
    assert got.shape == want.shape and e < 1e-4, e
    assert {"conv_split3", "conv_split3_s2", "groupnorm_split", "conv_in_f32_tokens"} <= kinds, kinds
    with torch.no_grad():
        # outside the walk: the repository's small first stage (ch 32), and a CPU input
        small = vae.Encoder(**H.SMALL_VAE).eval().to(DEV)
        xs = H.vae_inputs(31).to(DEV)
        assert not vae_split.encoder_applies(small, xs)
        assert not vae_split.encoder_applies(enc_cpu, x)
        eng_small = vae.AutoencodingEngine(encoder_config=small, decoder_config=torch.nn.Identity())
        eng_cpu = vae.AutoencodingEngine(encoder_config=enc_cpu, decoder_config=torch.nn.Identity())
        for eng, inp in ((eng_small, xs), (eng_cpu, x)):
            with pytest.raises(ValueError):
                vae.encode_first_stage(eng, inp, mode="split3")
        assert not vae_split.encoder_applies(enc, xd.double())
    with torch.enable_grad():
        assert not vae_split.encoder_applies(enc, xd)


def test_full_size_encoder_walk_matches_the_reference(golden_dir, ops):
    """The full-size encoder (ch 128, ch_mult [1, 2, 4, 4]) on one 576x1024 frame through the split walk against the imported reference's
    fp32 CPU moments (tests/golden/vae_full.npz, weights seed 51, input seed 62 as tests/test_vae_gpu.py draws them): 1e-4; two runs
    give the same bits."""
    from multiview_inpaint_amd.svd import vae, vae_split
    G = np.load(os.path.join(golden_dir, "vae_full.npz"))
    enc = vae.Encoder(**H.FULL_VAE).eval()
    enc.load_state_dict(H.seeded_state_dict(enc, 51), strict=True)
    enc = enc.to(DEV)
    x = H.vae_inputs(62, T=1, hw=H.FULL_VAE_HW).to(DEV)
    with torch.no_grad():
        assert vae_split.encoder_applies(enc, x)
        m1 = vae_split.encode(enc, x)
        m2 = vae_split.encode(enc, x)
    torch.cuda.synchronize()
    e = rel(m1, G["enc_moments"])
    H.report(f"full-size encoder on the split walk (one 576x1024 frame): enc_moments relative max error {e:.2e} (bar 1e-4)")
    assert tuple(m1.shape) == tuple(G["enc_moments"].shape) and e < 1e-4, e
    assert torch.equal(m1, m2)


def test_encode_first_stage_split_mode_is_opt_in(ops, small_encoder, monkeypatch):
    """encode_first_stage(mode="split3") against the default route under the same seed (1e-4 of the largest latent); chunked ==
    unchunked on the moments, bit for bit per frame; the default route runs no split kernel, MVI_VAE_ENCODE=split3 does.
    Frames of 16x32 here (levels 16x32 -> 8x16 -> 4x8): the DEFAULT route is the yardstick of this test and has to stay on its HIP
    kernels under the strict fixture, and its token -> planes kernel takes S % 8 == 0 (S = 28 of the 18x30 frames above does not)."""
    import copy
    from multiview_inpaint_amd.svd import vae
    enc_cpu = small_encoder[0]
    eng = vae.AutoencodingEngine(encoder_config=copy.deepcopy(enc_cpu), decoder_config=torch.nn.Identity()).eval().to(DEV)
    x = H.vae_inputs(73, T=3, hw=(16, 32))
    xd = x.to(DEV)

    def run(**kw):
        torch.manual_seed(7)
        ops.PROFILE = []
        try:
            z = vae.encode_first_stage(eng, xd, **kw)
            torch.cuda.synchronize()
            return z, set(k for k, *_ in ops.PROFILE)
        finally:
            ops.PROFILE = None
    z0, kinds0 = run()
    z3, kinds3 = run(mode="split3")
    e = rel(z3, z0)
    H.report(f"encode_first_stage(mode='split3') against the default route, small encoder: relative max difference {e:.2e} (bar 1e-4)")
    assert z3.shape == z0.shape == (3, 4, 4, 8) and e < 1e-4, e
    assert not any(k.startswith("conv_split3") for k in kinds0), kinds0          # the default is unchanged
    assert {"conv_split3", "conv_split3_s2"} <= kinds3, kinds3
    m, _ = run(mode="split3", unregularized=True)
    mc, _ = run(mode="split3", unregularized=True, en_and_decode_n_samples_a_time=2)
    assert m.shape == (3, 8, 4, 8)
    for f in range(3):
        assert torch.equal(mc[f], m[f]), f
    monkeypatch.setattr(vae, "ENCODE_MODE", "split3")
    ze, kinds_env = run()
    assert {"conv_split3", "conv_split3_s2"} <= kinds_env and torch.equal(ze, z3)
    # the environment form falls back where the walk does not apply (a CPU input), the explicit form raised above
    torch.manual_seed(7)
    eng_cpu = vae.AutoencodingEngine(encoder_config=enc_cpu, decoder_config=torch.nn.Identity()).eval()
    assert vae.encode_first_stage(eng_cpu, x).shape == (3, 4, 4, 8)

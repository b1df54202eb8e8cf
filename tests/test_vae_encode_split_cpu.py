"""CPU side of the split-operand encoder (svd/vae_split.py encode): the pure geometry of hip_ops.conv_split3_s2 — output size of
Downsample.conv and the per-launch batch cut — and the identity the kernel's `origin` field rests on."""
import pytest
import torch
import torch.nn.functional as F

from multiview_inpaint_amd.svd import hip_ops

LIMIT = 0xFFFFFFFF                                   # the kernel's 32-bit byte offsets span the INPUT tensor of one launch


@pytest.mark.parametrize("Hh", range(2, 10))
@pytest.mark.parametrize("W", range(2, 10))
def test_output_size_is_that_of_the_padded_stride2_convolution(Hh, W):
    y = F.conv2d(F.pad(torch.zeros(1, 1, Hh, W), (0, 1, 0, 1)), torch.zeros(1, 1, 3, 3), stride=2)
    Ho, Wo, n = hip_ops.conv_split3_s2_plan(3, Hh, W, 256)
    assert (Ho, Wo) == tuple(y.shape[2:]) and n == 3
    # one image per launch when two do not fit, never fewer than one
    assert hip_ops.conv_split3_s2_plan(3, Hh, W, 256, max_bytes=Hh * W * 256)[2] == 1
    assert hip_ops.conv_split3_s2_plan(3, Hh, W, 256, max_bytes=2 * Hh * W * 256 + 1)[2] == 2
    assert hip_ops.conv_split3_s2_plan(3, Hh, W, 256, max_bytes=1)[2] == 1


def test_sizes_below_two_are_rejected():
    for Hh, W in ((1, 4), (4, 1), (0, 0)):
        with pytest.raises(ValueError):
            hip_ops.conv_split3_s2_plan(1, Hh, W, 256)


def test_origin_one_is_the_asymmetric_pad():
    """conv(pad(x, (0, 1, 0, 1)), stride 2) == conv(x, padding 1)[1::2, 1::2]: centres (2 y + 1, 2 x + 1), and the border tests of the
    padding-1 form are the pad's zero row and column — for even, odd and 2 x 2 sizes."""
    g = torch.Generator().manual_seed(3)
    for Hh, W in ((2, 2), (6, 8), (7, 9), (9, 4), (2, 5)):
        x, w = torch.randn(2, 3, Hh, W, generator=g).double(), torch.randn(4, 3, 3, 3, generator=g).double()
        a = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
        b = F.conv2d(x, w, padding=1)[:, :, 1::2, 1::2]
        assert a.shape == b.shape and torch.allclose(a, b, rtol=0, atol=1e-12)


def test_batch_cut_against_the_32_bit_limit_at_the_first_downsample_of_the_full_encoder():
    """The 576 x 1024 x 128-channel level as split bf16 (hi | lo): 512 bytes per pixel, 301 989 888 bytes per frame. A single frame is
    one launch. Every launch of any batch stays inside the limit and takes as many frames as fit.
    The issue asked for "a 14-frame batch must be cut" at this level; 14 frames are 4 227 858 432 bytes, which is BELOW 2^32 - 1 =
    4 294 967 295 (4.2 GB, but under 4 GiB), so the limit the kernel enforces allows them in one launch, as it does for the decoder's
    conv_split3 at the same level. The assertion below states what the limit implies: 14 frames fit, 15 do not."""
    Hh, W, row_bytes = 576, 1024, 2 * 128 * 2
    per = Hh * W * row_bytes
    assert per == 301_989_888
    Ho, Wo, n1 = hip_ops.conv_split3_s2_plan(1, Hh, W, row_bytes)
    assert (Ho, Wo, n1) == (288, 512, 1)
    for N in (1, 2, 14, 15, 16, 25, 28, 29):
        n = hip_ops.conv_split3_s2_plan(N, Hh, W, row_bytes)[2]
        assert 1 <= n <= N and n * per <= LIMIT and (n == N or (n + 1) * per > LIMIT), (N, n)
    assert 14 * per <= LIMIT < 15 * per
    assert hip_ops.conv_split3_s2_plan(14, Hh, W, row_bytes)[2] == 14
    assert hip_ops.conv_split3_s2_plan(15, Hh, W, row_bytes)[2] == 14         # a 15-frame batch IS cut: 14 + 1
    assert hip_ops.conv_split3_s2_plan(28, Hh, W, row_bytes)[2] == 14         # the sampling path's 14 + 14 frames: two launches
    with pytest.raises(ValueError):                                          # one image alone past the limit
        hip_ops.conv_split3_s2_plan(1, 4096, 4096, row_bytes)

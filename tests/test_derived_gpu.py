"""svd/derived.py through the sites that need the HIP library, in bf16: a parameter is replaced by ANOTHER parameter object on the same
storage (same address, version counter at 0 again — what the caching allocator does with a freed model's block) and the op must see
the new values: its result is bit-identical to the same op run with a fresh, unrelated parameter holding them."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)


def _randn(shape, seed, dtype=torch.bfloat16):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV, dtype)


def _check_replacement(run, shape, dtype=torch.bfloat16):
    """run(parameter) -> tensor. First values, then the storage overwritten and wrapped in a new parameter, then a fresh parameter."""
    buf, new = _randn(shape, 1, dtype), _randn(shape, 2, dtype)
    old = nn.Parameter(buf.data)
    with torch.no_grad():
        first = run(old).clone()
        assert torch.equal(run(old), first)
        buf.copy_(new)
        p2 = nn.Parameter(buf.data)
        assert p2 is not old and p2.data_ptr() == old.data_ptr() and p2._version == old._version
        got = run(p2)
        want = run(nn.Parameter(new.clone()))
    torch.cuda.synchronize()
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert not torch.equal(got, first)


def test_stem_conv_packed_weight():
    from multiview_inpaint_amd.svd import hip_ops
    x, bias = _randn((1, 4, 16, 16), 3), nn.Parameter(_randn((16,), 4))
    conv = nn.Conv2d(4, 16, 3, padding=1).to(DEV, torch.bfloat16)
    assert hip_ops.stem_conv3x3_supported(conv, x)
    _check_replacement(lambda w: hip_ops.stem_conv3x3_silu(x, w, bias), (16, 4, 3, 3))


def test_conv3x3_n320_tap_major_weight():
    from multiview_inpaint_amd.svd import hip_ops, layers
    tok = _randn((1, 16 * 16, 64), 5)
    assert hip_ops.conv3x3_n320_supported(64, 320, torch.bfloat16)
    _check_replacement(lambda w: hip_ops.conv3x3_n320(tok, layers._tap_major_weight(w), None, 16, 16), (320, 64, 3, 3))


def test_conv_split3_weight():
    from multiview_inpaint_amd.svd import hip_ops, vae_split
    N, T, S, C, Co = 3, 2, 40, 64, 64                       # the smallest (3,1,1) case of tests/test_vae_gpu.py, one rounded value per operand
    x1 = hip_ops.group_norm_split(_randn((N * T, S, C), 6, torch.float32), 0, None, None, 0.0, False, mode="bf16")
    _check_replacement(lambda w: hip_ops.conv_split3(x1.reshape(-1, C), vae_split._w3(w, "bf16"), N, T, S, Co, taps=3, mode="bf16"),
                       (Co, C, 3, 1, 1), torch.float32)


def test_group_norm_bf16_affine_parameters():
    from multiview_inpaint_amd.svd import ops
    x, bias = _randn((2, 64, 8, 8), 7), nn.Parameter(_randn((64,), 8))
    _check_replacement(lambda w: ops.group_norm(x, 32, w, bias, 1e-5, silu=True), (64,))

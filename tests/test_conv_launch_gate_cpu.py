"""hip_ops.conv_n320_launch_ok — the one "does csrc/linear_n320.hip take this convolution launch and fill the chip?" gate — against the
conditions its callers spelled out one by one before it existed, restated here in plain Python (`Parent`): the four ops.*_tokens_gates, the
no-grad branch of the four public ops (ops.conv3x3_tokens, conv3x3_down_tokens, conv3x3_up_tokens, conv3t_tokens) and
layers._conv_n320_shape_ok, on a grid that holds a K-split-only shape, a shape over the 32-bit byte-offset bound, a W over the
weight-gradient kernel's limit and odd H / W. mvi_conv3x3_n320_supported, the *_wgrad_supported functions and the *_workspace_bytes
functions are pure host functions of the shape and make no HIP call: no GPU.

The public ops are called with stand-ins for CUDA tensors (shape, dtype, is_cuda, requires_grad): with the launch itself replaced, a call
either reaches the kernel launch or, strict gates on, raises ops.HipPathError before its PyTorch expression — which is the gate's answer."""
import itertools
import types

import pytest
import torch

from multiview_inpaint_amd.svd import hip_ops, layers, ops

B16 = (torch.bfloat16, torch.float16)
BATCHES = (1, 2, 14, 28)
SIZES = ((1, 1), (3, 5), (4, 6), (6, 8), (12, 16), (18, 32), (48, 64), (72, 128), (2, 300), (576, 1024))
FRAME_SIZES = tuple(dict.fromkeys(SIZES + tuple((T, S) for T in (1, 14) for _, S in SIZES)))      # (T, S): SIZES, and T in {1, 14}
CHANNELS = ((64, 320), (320, 320), (640, 320), (320, 640), (1280, 1280), (2560, 1280), (320, 64), (96, 320), (320, 300))
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
MIN_BLOCKS = (0, 1, 128)
KSPLIT_ONLY = (1, 6, 8, 1280, 1280)            # the upsampling launch of this source: 4 blocks, and the stride-1 launch at 12x16 would K-split
OVER_32_BITS = (28, 576, 1024, 320, 320)       # 10.6 GB of byte offsets


@pytest.fixture(scope="module")
def L():
    from multiview_inpaint_amd import _lib
    return _lib.lib()                                            # raises if a declared symbol is missing


class Parent:
    """The conditions as the callers wrote them, `hip_ops.` read as `self.`; min_blocks stands for the module constant of each."""

    def __init__(self, L):
        self.L = L
        self.CONV3X3_WGRAD_MAX_W = 256

    def _dt(self, dtype):
        return {torch.bfloat16: 1, torch.float16: 2}[dtype]      # MVI_DT_BF16, MVI_DT_F16 (include/mvi_unet_ops.h)

    def conv3x3_n320_supported(self, C_in, C_out, dtype):
        return dtype in B16 and bool(self.L.mvi_conv3x3_n320_supported(int(C_in), int(C_out), self._dt(dtype)))

    def conv3x3_s2_dgrad_supported(self, C_in, C_out, dtype):
        return dtype in B16 and bool(self.L.mvi_conv3x3_s2_dgrad_supported(int(C_in), int(C_out), self._dt(dtype)))

    def conv3x3_wgrad_supported(self, C_in, C_out, dtype):
        return dtype in B16 and bool(self.L.mvi_conv3x3_wgrad_supported(int(C_in), int(C_out), self._dt(dtype)))

    def conv3x3_s2_wgrad_supported(self, C_in, C_out, dtype):
        return dtype in B16 and bool(self.L.mvi_conv3x3_s2_wgrad_supported(int(C_in), int(C_out), self._dt(dtype)))

    def conv3t_wgrad_supported(self, C_in, C_out, dtype):
        return dtype in B16 and bool(self.L.mvi_conv3t_wgrad_supported(int(C_in), int(C_out), self._dt(dtype)))

    def conv3x3_n320_fills_chip(self, N, H, W, C_in, C_out, min_blocks, stride=1):
        rows = N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        blocks = -(-rows // 256) * (C_out // 320)
        return blocks >= min_blocks or int(self.L.mvi_conv3x3_n320_workspace_bytes(N, H, W, C_in, C_out, stride)) > 0

    def conv3t_n320_fills_chip(self, B, T, S, C_in, C_out, min_blocks):
        blocks = -(-B * T * S // 256) * (C_out // 320)
        return blocks >= min_blocks or int(self.L.mvi_conv3t_n320_workspace_bytes(B, T, S, C_in, C_out)) > 0

    # ---- ops.*_tokens_gates ----
    def conv3x3_tokens_gates(self, N, H, W, C_in, C_out, dtype, min_blocks):
        rows = N * H * W
        return (dtype in (torch.bfloat16, torch.float16) and rows > 0
                and self.conv3x3_n320_supported(C_in, C_out, dtype) and self.conv3x3_n320_supported(C_out, C_in, dtype)
                and rows * max(C_in, C_out) * 2 < 2 ** 32
                and self.conv3x3_n320_fills_chip(N, H, W, C_in, C_out, min_blocks)
                and self.conv3x3_n320_fills_chip(N, H, W, C_out, C_in, min_blocks)
                and self.conv3x3_wgrad_supported(C_in, C_out, dtype) and W <= self.CONV3X3_WGRAD_MAX_W)

    def conv3x3_down_tokens_gates(self, N, H, W, C_in, C_out, dtype, min_blocks):
        rows = N * H * W
        return (dtype in (torch.bfloat16, torch.float16) and rows > 0 and H % 2 == 0 and W % 2 == 0
                and self.conv3x3_n320_supported(C_in, C_out, dtype) and self.conv3x3_s2_dgrad_supported(C_in, C_out, dtype)
                and rows * max(C_in, C_out) * 2 < 2 ** 32
                and self.conv3x3_n320_fills_chip(N, H, W, C_in, C_out, min_blocks, stride=2)
                and -(-rows // 256) * (C_in // 320) >= min_blocks
                and self.conv3x3_s2_wgrad_supported(C_in, C_out, dtype) and W <= self.CONV3X3_WGRAD_MAX_W)

    def conv3x3_up_tokens_gates(self, N, h, w, C_in, C_out, dtype, min_blocks):
        rows = N * 4 * h * w
        return (dtype in (torch.bfloat16, torch.float16) and rows > 0
                and self.conv3x3_n320_supported(C_in, C_out, dtype) and self.conv3x3_n320_supported(C_out, C_in, dtype)
                and rows * max(C_in, C_out) * 2 < 2 ** 32
                and -(-rows // 256) * (C_out // 320) >= min_blocks
                and self.conv3x3_n320_fills_chip(N, 2 * h, 2 * w, C_out, C_in, min_blocks))

    def conv3t_tokens_gates(self, B, T, S, C_in, C_out, dtype, min_blocks):
        rows = B * T * S
        return (dtype in (torch.bfloat16, torch.float16) and rows > 0
                and self.conv3x3_n320_supported(C_in, C_out, dtype) and self.conv3x3_n320_supported(C_out, C_in, dtype)
                and rows * max(C_in, C_out) * 2 < 2 ** 32
                and self.conv3t_n320_fills_chip(B, T, S, C_in, C_out, min_blocks)
                and self.conv3t_n320_fills_chip(B, T, S, C_out, C_in, min_blocks)
                and self.conv3t_wgrad_supported(C_in, C_out, dtype))

    # ---- the no-grad branch of the public ops (S = H W pixels per image; the tensors' dtypes agree) ----
    def conv3x3_tokens(self, N, H, W, C, Co, dtype, min_blocks):
        S = H * W
        return (self.conv3x3_n320_supported(C, Co, dtype) and N * S * C * 2 < 2 ** 32
                and self.conv3x3_n320_fills_chip(N, H, W, C, Co, min_blocks))

    def conv3x3_down_tokens(self, N, H, W, C, Co, dtype, min_blocks):
        S = H * W
        return (dtype in (torch.bfloat16, torch.float16) and N * S > 0 and self.conv3x3_n320_supported(C, Co, dtype)
                and N * S * C * 2 < 2 ** 32 and self.conv3x3_n320_fills_chip(N, H, W, C, Co, min_blocks, stride=2))

    def conv3x3_up_tokens(self, N, h, w, C, Co, dtype, min_blocks):
        S = h * w
        return (dtype in (torch.bfloat16, torch.float16) and N * S > 0 and self.conv3x3_n320_supported(C, Co, dtype)
                and 4 * N * S * C * 2 < 2 ** 32 and -(-4 * N * S // 256) * (Co // 320) >= min_blocks)

    def conv3t_tokens(self, B, T, S, C, Co, dtype, min_blocks):
        BT = B * T
        return (dtype in (torch.bfloat16, torch.float16) and BT * S > 0 and self.conv3x3_n320_supported(C, Co, dtype)
                and BT * S * C * 2 < 2 ** 32 and self.conv3t_n320_fills_chip(B, T, S, C, Co, min_blocks))

    # ---- layers._conv_n320_shape_ok(conv, N, C, Hi, Wi, dtype) ----
    def shape_ok(self, conv, N, C, Hi, Wi, dtype, min_blocks):
        return (C % 8 == 0 and self.conv3x3_n320_supported(C, conv.out_channels, dtype) and N * Hi * Wi * C * 2 < 2 ** 32
                and self.conv3x3_n320_fills_chip(N, Hi, Wi, C, conv.out_channels, min_blocks, stride=conv.stride[0]))


@pytest.fixture(scope="module")
def parent(L):
    return Parent(L)


def _grid(sizes=SIZES):
    return itertools.product(BATCHES, sizes, CHANNELS, DTYPES)


def _both(seen, what):
    assert seen == {True, False}, f"{what}: only {seen} on the grid"


@pytest.mark.parametrize("mb", MIN_BLOCKS)
def test_tokens_gates(parent, monkeypatch, mb):
    for name in ("CONV3X3_MIN_BLOCKS", "RESAMPLE_CONV_MIN_BLOCKS", "CONV3T_MIN_BLOCKS"):
        monkeypatch.setattr(ops, name, mb)
    for gate, sizes in (("conv3x3_tokens_gates", SIZES), ("conv3x3_down_tokens_gates", SIZES), ("conv3x3_up_tokens_gates", SIZES),
                        ("conv3t_tokens_gates", FRAME_SIZES)):
        seen = set()
        for N, (H, W), (Ci, Co), dt in _grid(sizes):
            want = bool(getattr(parent, gate)(N, H, W, Ci, Co, dt, mb))
            assert bool(getattr(ops, gate)(N, H, W, Ci, Co, dt)) == want, (gate, N, H, W, Ci, Co, dt, mb)
            seen.add(want)
        _both(seen, gate)


def _fake(shape, dtype):
    return types.SimpleNamespace(shape=tuple(shape), dtype=dtype, is_cuda=True, requires_grad=False)


LAUNCHED = object()


def _takes_kernel(call):
    """Did this call of a public op reach the launch (replaced) — or leave the HIP path at its gate?"""
    try:
        return call() is LAUNCHED
    except ops.HipPathError:
        return False


@pytest.mark.parametrize("mb", MIN_BLOCKS)
def test_no_grad_branches(parent, monkeypatch, mb):
    for name in ("CONV3X3_MIN_BLOCKS", "RESAMPLE_CONV_MIN_BLOCKS", "CONV3T_MIN_BLOCKS"):
        monkeypatch.setattr(ops, name, mb)
    monkeypatch.setattr(ops, "STRICT_GATES", True)
    monkeypatch.setattr(ops, "_conv_launch", lambda *a: LAUNCHED)
    calls = {
        "conv3x3_tokens": lambda N, H, W, C, Co, dt: ops.conv3x3_tokens(_fake((N, H * W, C), dt), _fake((Co, C, 3, 3), dt), H, W),
        "conv3x3_down_tokens": lambda N, H, W, C, Co, dt: ops.conv3x3_down_tokens(_fake((N, H * W, C), dt), _fake((Co, C, 3, 3), dt), None, H, W),
        "conv3x3_up_tokens": lambda N, H, W, C, Co, dt: ops.conv3x3_up_tokens(_fake((N, H * W, C), dt), _fake((Co, C, 3, 3), dt), None, H, W),
        "conv3t_tokens": lambda B, T, S, C, Co, dt: ops.conv3t_tokens(_fake((B * T, S, C), dt), _fake((Co, C, 3, 1, 1), dt), T),
    }
    for op, call in calls.items():
        seen = set()
        for N, (H, W), (Ci, Co), dt in _grid(FRAME_SIZES if op == "conv3t_tokens" else SIZES):
            want = bool(getattr(parent, op)(N, H, W, Ci, Co, dt, mb))
            assert _takes_kernel(lambda: call(N, H, W, Ci, Co, dt)) == want, (op, N, H, W, Ci, Co, dt, mb)
            seen.add(want)
        _both(seen, op)


@pytest.mark.parametrize("mb", MIN_BLOCKS)
def test_layers_shape_ok(parent, monkeypatch, mb):
    monkeypatch.setattr(layers, "CONV_N320_MIN_BLOCKS", mb)
    seen, seen_up = set(), set()
    for N, (H, W), (Ci, Co), dt in _grid():
        for stride in (1, 2):
            conv = types.SimpleNamespace(out_channels=Co, stride=(stride, stride))
            want = bool(parent.shape_ok(conv, N, Ci, H, W, dt, mb))
            assert bool(layers._conv_n320_shape_ok(conv, N, Ci, H, W, dt)) == want, (stride, N, H, W, Ci, Co, dt, mb)
            seen.add(want)
        # Upsample on tokens: it asked for the stride-1 launch at 2 H x 2 W and ran the upsampling launch of the H x W source
        conv = types.SimpleNamespace(out_channels=Co, stride=(1, 1))
        want = bool(parent.shape_ok(conv, N, Ci, 2 * H, 2 * W, dt, mb))
        assert bool(layers._conv_n320_shape_ok(conv, N, Ci, H, W, dt, form="up2", ksplit_counts=True)) == want, (N, H, W, Ci, Co, dt, mb)
        seen_up.add(want)
    _both(seen, "_conv_n320_shape_ok")
    _both(seen_up, "_conv_n320_shape_ok (Upsample)")


def test_named_cases(parent, L, monkeypatch):
    """The shapes the grid is built around, by name, at the shipped line of 128 blocks."""
    bf = torch.bfloat16
    for mod, name in ((ops, "CONV3X3_MIN_BLOCKS"), (ops, "RESAMPLE_CONV_MIN_BLOCKS"), (ops, "CONV3T_MIN_BLOCKS"), (layers, "CONV_N320_MIN_BLOCKS")):
        monkeypatch.setattr(mod, name, 128)
    monkeypatch.setattr(ops, "STRICT_GATES", True)
    monkeypatch.setattr(ops, "_conv_launch", lambda *a: LAUNCHED)
    N, h, w, C, Co = KSPLIT_ONLY
    assert -(-N * 4 * h * w // 256) * (Co // 320) == 4 and L.mvi_conv3x3_n320_workspace_bytes(N, 2 * h, 2 * w, C, Co, 1) > 0
    # the two upsampling gates disagree on it: layers.Upsample admits the K-split-only shape (and runs the unsplit launch), ops refuses
    conv = types.SimpleNamespace(out_channels=Co, stride=(1, 1))
    assert parent.shape_ok(conv, N, C, 2 * h, 2 * w, bf, 128)
    assert layers._conv_n320_shape_ok(conv, N, C, h, w, bf, form="up2", ksplit_counts=True)
    assert not parent.conv3x3_up_tokens(N, h, w, C, Co, bf, 128)
    assert not _takes_kernel(lambda: ops.conv3x3_up_tokens(_fake((N, h * w, C), bf), _fake((Co, C, 3, 3), bf), None, h, w))
    assert not hip_ops.conv_n320_launch_ok("up2", N, h, w, C, Co, bf, 128)
    assert hip_ops.conv_n320_launch_ok("s1", N, 2 * h, 2 * w, C, Co, bf, 128)          # (the stride-1 launch does split)
    # over the 32-bit bound: refused whatever the line; one batch less of the same image passes
    N, H, W, C, Co = OVER_32_BITS
    assert N * H * W * C * 2 > 0xFFFFFFFF
    for form in ("s1", "s2", "t3", "s2_dgrad"):
        assert not hip_ops.conv_n320_launch_ok(form, N, H, W, C, Co, bf, 0)
        assert hip_ops.conv_n320_launch_ok(form, 2, H, W, C, Co, bf, 0)
    assert not hip_ops.conv_n320_launch_ok("up2", N, H // 2, W // 2, C, Co, bf, 0)
    # W over the weight-gradient kernel's limit: the launches pass, the autograd gate does not
    assert hip_ops.conv_n320_launch_ok("s1", 14, 2, 300, 320, 320, bf, 0) and 300 > hip_ops.CONV3X3_WGRAD_MAX_W
    monkeypatch.setattr(ops, "CONV3X3_MIN_BLOCKS", 0)
    assert not ops.conv3x3_tokens_gates(14, 2, 300, 320, 320, bf) and ops.conv3x3_tokens_gates(14, 2, 256, 320, 320, bf)
    # odd H or W: the stride-2 forward takes it, its backward does not
    monkeypatch.setattr(ops, "RESAMPLE_CONV_MIN_BLOCKS", 0)
    assert hip_ops.conv_n320_launch_ok("s2", 14, 3, 5, 320, 320, bf, 0) and not ops.conv3x3_down_tokens_gates(14, 3, 5, 320, 320, bf)
    assert ops.conv3x3_down_tokens_gates(14, 4, 6, 320, 320, bf)
    # no rows, no launch — for every form
    for form in ("s1", "s2", "up2", "s2_dgrad", "t3"):
        assert not hip_ops.conv_n320_launch_ok(form, 0, 4, 6, 320, 320, bf, 0) and not hip_ops.conv_n320_launch_ok(form, 1, 4, 0, 320, 320, bf, 0)
    with pytest.raises(KeyError):
        hip_ops.conv_n320_launch_ok("s3", 1, 4, 6, 320, 320, bf, 0)

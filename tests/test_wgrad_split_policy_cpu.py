"""The split policies of the three MFMA weight-gradient files (csrc/conv3x3_wgrad.hip with its stride-2 form, csrc/conv3t_wgrad.hip,
csrc/linear_wgrad.hip), restated in plain Python from the formulas in the file headers and compared with what the library's
mvi_*_wgrad_workspace_bytes functions answer. Those functions are pure host functions of the shape and make no HIP call: no GPU.

The scheme ("Deterministic split-K of the weight gradients"): S = min(units, target / tiles, 64), below 2 means 1 (no
workspace); the projections round S down to whole groups of 8 above 8. S > 1 asks for S fp32 partials.
  conv3x3      units = N ceil(H (W + 2) / 160)             tiles = (C_in / 64)(C_out / 64)      target 512    9 C_out C_in floats
  conv3x3 s2   units = N ceil((H / 2)(W / 2 + 1) / 64)     the same                             target 512    the same
  conv3t       units = B ceil(S / 64)                      the same                             target 1024   3 C_out C_in floats
  linear       units = ceil(rows / 64)                     tiles = ceil(K / 128) ceil(N / 128)  target 512    N K + N floats, groups of 8"""
import itertools

import pytest

MAX_SPLIT = 64


def _ceil(a, b):
    return -(-a // b)


def split_count(units, tiles, target, group=1):
    s = min(units, target // tiles, MAX_SPLIT)
    if s > group:
        s -= s % group
    return 1 if s < 2 else s


def _channels_ok(*cs):
    return all(c > 0 and c % 64 == 0 for c in cs)


def conv3x3_bytes(N, H, W, Ci, Co):
    if not (_channels_ok(Ci, Co) and N > 0 and H >= 1 and 1 <= W <= 256):
        return 0
    s = split_count(N * _ceil(H * (W + 2), 160), (Ci // 64) * (Co // 64), 512)
    return s * Co * Ci * 9 * 4 if s > 1 else 0


def conv3x3_s2_bytes(N, H, W, Ci, Co):
    if not (_channels_ok(Ci, Co) and N > 0 and H >= 1 and 1 <= W <= 256 and H % 2 == 0 and W % 2 == 0):
        return 0
    s = split_count(N * _ceil((H // 2) * (W // 2 + 1), 64), (Ci // 64) * (Co // 64), 512)
    return s * Co * Ci * 9 * 4 if s > 1 else 0


def conv3t_bytes(B, T, S, Ci, Co):
    if not (_channels_ok(Ci, Co) and B > 0 and T >= 1 and S >= 1):
        return 0
    r = split_count(B * _ceil(S, 64), (Ci // 64) * (Co // 64), 1024)
    return r * Co * Ci * 3 * 4 if r > 1 else 0


def linear_bytes(rows, K, N):
    if not (_channels_ok(K, N) and rows > 0):
        return 0
    s = split_count(_ceil(rows, 64), _ceil(K, 128) * _ceil(N, 128), 512, group=8)
    return s * (N * K + N) * 4 if s > 1 else 0


@pytest.fixture(scope="module")
def L():
    from multiview_inpaint_amd import _lib
    return _lib.lib()                                            # raises if a declared symbol is missing


CHANNELS = [(64, 64), (64, 128), (320, 320), (640, 320), (1280, 1280), (2560, 1280)]
# the training shapes of tests/test_conv3x3_bwd_gpu.py, test_resample_conv_bwd_gpu.py, test_conv3t_bwd_gpu.py and test_linear_bwd_gpu.py
CONV3X3_TRAINING = [(N, H, W, Ci, Co) for N in (14, 28) for H, W, Ci, Co in
                    ((48, 64, 320, 320), (48, 64, 640, 320), (24, 32, 640, 640), (24, 32, 1280, 640), (12, 16, 1280, 1280),
                     (12, 16, 2560, 1280), (6, 8, 1280, 1280))]
CONV3X3_TESTED = [(2, 24, 32, 320, 320), (3, 9, 16, 64, 128), (1, 7, 5, 128, 64), (5, 1, 1, 64, 64), (1, 40, 33, 192, 320),
                  (2, 3, 96, 640, 320)]
S2_TRAINING = [(14, H, W, C, C) for H, W, C in ((72, 128, 320), (36, 64, 640), (18, 32, 1280))]
S2_TESTED = [(1, 2, 2, 64, 64), (5, 2, 2, 64, 64), (2, 6, 10, 128, 64), (1, 2, 256, 64, 64), (3, 18, 32, 320, 320), (1, 40, 34, 192, 320)]
CONV3T_TRAINING = [(B, 14, S, C, C) for B in (1, 2) for S, C in ((3072, 320), (768, 640), (192, 1280), (48, 1280))]
CONV3T_TESTED = [(1, 1, 5, 64, 64), (2, 2, 1, 64, 128), (2, 3, 45, 128, 64), (1, 14, 161, 64, 64), (2, 14, 333, 320, 320), (1, 4, 96, 640, 320)]
LINEAR_TRAINING = [(rows, K, N) for rows in (14 * 3072, 14 * 768, 14 * 192, 14 * 48, 258048) for K, N in
                   ((320, 320), (320, 960), (640, 640), (1280, 1280), (1280, 320), (320, 1280), (1024, 320))]
LINEAR_TESTED = [(300, 128, 320), (1, 64, 64), (257, 320, 960), (513, 1280, 320), (70001, 64, 128), (2600, 320, 960), (2600, 1280, 320)]


def test_anchors(L):
    """Derived by hand from the kernels' host code."""
    assert L.mvi_conv3x3_wgrad_workspace_bytes(2, 1, 1, 64, 64) == 294912 == conv3x3_bytes(2, 1, 1, 64, 64)           # S = 2
    assert L.mvi_conv3x3_wgrad_workspace_bytes(1, 1, 1, 64, 64) == 0 == conv3x3_bytes(1, 1, 1, 64, 64)
    assert L.mvi_conv3t_wgrad_workspace_bytes(2, 2, 1, 64, 64) == 98304 == conv3t_bytes(2, 2, 1, 64, 64)              # R = 2
    assert L.mvi_linear_wgrad_workspace_bytes(1089, 64, 64) == 16 * (64 * 64 + 64) * 4 == 266240 == linear_bytes(1089, 64, 64)  # 18 -> 16
    assert L.mvi_linear_wgrad_workspace_bytes(65, 64, 64) == 2 * 4160 * 4 == 33280 == linear_bytes(65, 64, 64)


def test_conv3x3_policy(L):
    grid = [(N, H, W, Ci, Co) for N, H, W in itertools.product((1, 2, 3, 5, 14), (1, 2, 3, 7, 13, 24), (1, 2, 5, 11, 16, 64, 255, 256))
            for Ci, Co in CHANNELS]
    split = 0
    for s in grid + CONV3X3_TRAINING + CONV3X3_TESTED:
        want = conv3x3_bytes(*s)
        assert L.mvi_conv3x3_wgrad_workspace_bytes(*s) == want, s
        split += want > 0
    assert 0 < split < len(grid)
    for s in ((0, 8, 8, 64, 64), (2, 8, 8, 96, 64), (2, 8, 8, 64, 32), (2, 8, 257, 64, 64), (2, 0, 8, 64, 64), (2, 8, 0, 64, 64), (-1, 8, 8, 64, 64)):
        assert L.mvi_conv3x3_wgrad_workspace_bytes(*s) == 0 == conv3x3_bytes(*s), s


def test_conv3x3_s2_policy(L):
    grid = [(N, H, W, Ci, Co) for N, H, W in itertools.product((1, 2, 3, 5, 14), (2, 4, 6, 18, 40), (2, 4, 10, 14, 32, 128, 254, 256))
            for Ci, Co in CHANNELS]
    split = 0
    for s in grid + S2_TRAINING + S2_TESTED:
        want = conv3x3_s2_bytes(*s)
        assert L.mvi_conv3x3_s2_wgrad_workspace_bytes(*s) == want, s
        split += want > 0
    assert 0 < split < len(grid)
    for s in ((0, 8, 8, 64, 64), (2, 7, 8, 64, 64), (2, 8, 7, 64, 64), (2, 1, 1, 64, 64), (2, 8, 8, 96, 64), (2, 8, 8, 64, 100), (2, 8, 257, 64, 64),
              (2, 8, 258, 64, 64)):
        assert L.mvi_conv3x3_s2_wgrad_workspace_bytes(*s) == 0 == conv3x3_s2_bytes(*s), s


def test_conv3t_policy(L):
    grid = [(B, T, S, Ci, Co) for B, T, S in itertools.product((1, 2, 3, 5), (1, 2, 3, 14), (1, 5, 63, 64, 65, 128, 129, 333, 3072))
            for Ci, Co in CHANNELS]
    split = 0
    for s in grid + CONV3T_TRAINING + CONV3T_TESTED:
        want = conv3t_bytes(*s)
        assert L.mvi_conv3t_wgrad_workspace_bytes(*s) == want, s
        split += want > 0
    assert 0 < split < len(grid)
    for s in ((0, 14, 64, 64, 64), (2, 0, 64, 64, 64), (2, 14, 0, 64, 64), (2, 14, 64, 96, 64), (2, 14, 64, 64, 72)):
        assert L.mvi_conv3t_wgrad_workspace_bytes(*s) == 0 == conv3t_bytes(*s), s


def test_linear_policy(L):
    grid = [(rows, K, N) for rows in (1, 63, 64, 65, 128, 129, 300, 512, 513, 576, 577, 1024, 1089, 4096, 4097, 70001)
            for K, N in CHANNELS + [(192, 64), (64, 192), (960, 320), (3840, 1280)]]
    split, counts = 0, set()
    for s in grid + LINEAR_TRAINING + LINEAR_TESTED:
        want = linear_bytes(*s)
        assert L.mvi_linear_wgrad_workspace_bytes(*s) == want, s
        split += want > 0
        counts.add(want // ((s[1] * s[2] + s[2]) * 4))
    assert 0 < split < len(grid)
    # 0 (unsplit), fewer than 8 slices as they come, whole groups of 8 above
    assert all(c == 0 or 2 <= c <= 8 or c % 8 == 0 for c in counts) and {0, 2, 8, 16, 64} <= counts, sorted(counts)
    for s in ((0, 64, 64), (300, 96, 64), (300, 64, 100), (300, 0, 64), (-5, 64, 64)):
        assert L.mvi_linear_wgrad_workspace_bytes(*s) == 0 == linear_bytes(*s), s

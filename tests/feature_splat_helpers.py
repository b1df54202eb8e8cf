"""Reference, scenes and bars for the feature splat (raster.splat_features: out[c, p] = sum_i alpha_i(p) T_i(p) F[i, c]).

The reference needs no oracle code of its own: the CPU oracle's forward with colors_precomp = F[:, 3k : 3k + 3] on a zero
background IS sum alpha T F, three channels per call (tests/test_feature_splat_cpu.py pins it as the adjoint of the lift's
reference, tests/mask_lift_helpers.py).

The image bar is the colour bar of tests/test_raster_gpu.py::_check_forward: |got - ref| <= 1e-4 max(|ref|, floor) with
floor = max(1, max |F|) on every pixel the oracle's margins do not mark colour-marginal, offending pixels overall within the
flip allowance of the composited pairs, and the scene's marginal share below MAX_MARGINAL."""
import numpy as np

from mask_lift_helpers import MAX_MARGINAL, marginal_share
from raster_aux_helpers import flip_allowance, viol, zero_bg_params


def oracle_splat(ro, cam, sc, F):
    """(params, forward dict of the first call, [C,H,W] float64) of the oracle for features F [P, C]."""
    F = np.asarray(F, np.float32)
    if F.ndim == 1:
        F = F[:, None]
    P, Cn = F.shape
    p0 = zero_bg_params(ro, cam, sc)
    planes, first = [], None
    for c0 in range(0, Cn, 3):
        chunk = F[:, c0:c0 + 3]
        cp = np.zeros((P, 3), np.float32)
        cp[:, :chunk.shape[1]] = chunk
        f = ro.forward(p0, sc["means3D"], sc["opacities"], colors_precomp=cp, scales=sc["scales"], rotations=sc["rotations"])
        first = f if first is None else first
        planes.append(f["color"][:chunk.shape[1]].astype(np.float64))
    return p0, first, np.concatenate(planes, 0)


def signed_features(P, C, seed=21):
    """Signed float features: normal draws, every third row scaled by 3 so that the floor of the bar is not 1."""
    F = np.random.default_rng(seed).normal(size=(P, C)).astype(np.float32)
    F[::3] *= 3.0
    return F


def check_image(name, got, ref, ro, p0, f, floor):
    """The image bar. got, ref [C,H,W]; floor = max(1, max |F|). Returns the number of offending pixels."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    share = marginal_share(ro, p0, f)
    assert share < MAX_MARGINAL, ("margin too wide: the test would excuse too many pixels", share)
    colour_marginal = (ro.margins(p0, f) & 1) != 0
    bad, worst = viol(got, ref, floor)
    bad = bad.any(0)
    allow = flip_allowance(int(f["n_contrib"].sum()))
    print(f"image {name}: shape {ref.shape}, floor {floor:.3g}, worst ratio to the bar {worst:.3f}, pixels outside it "
          f"{int(bad.sum())} (allowed {allow}), marginal share {share:.4f}")
    assert not (bad & ~colour_marginal).any(), (name, "off on a pixel with no marginal decision", worst)
    assert int(bad.sum()) <= allow, (name, int(bad.sum()), allow)
    return int(bad.sum())


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return float((a & b).sum()) / max(1, int((a | b).sum()))

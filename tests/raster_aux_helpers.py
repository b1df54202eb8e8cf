"""Reference and bars for the rasterizer's aux outputs (expected depth = sum z alpha T, alpha = 1 - T_final).

The reference needs no oracle code of its own: both CPU oracles render arbitrary per-Gaussian colours, and with
colors_precomp = (z, 1, 0) and a zero background channel 0 of the oracle's colour IS the expected depth and channel 1 IS
alpha. Its backward for the upstream image (gD, gA, 0) returns the geometry gradients directly plus dL/dcolors[:, 0] = dL/dz,
and z = [m, 1] . V[:, 2] takes that to the positions: dL/dmeans3D += dL/dz * V[0:3, 2].

The bars are those of tests/test_raster_gpu.py, copied: the elementwise bar, the flip allowance and _grad_check."""
import numpy as np

RTOL = 1e-4
GRAD_FLOOR = 1e-2          # gradient floor as a fraction of the array's largest |value| (tests/test_raster_gpu.py)
PURE_REL_MIN_FRACTION = 0.985
GEOMETRY_KEYS = ("means3D", "means2D", "opacities", "scales", "rotations", "cov3D_precomp")


def flip_allowance(n_pairs):
    """Pixels allowed to differ because a decision flipped: 2 + 1e-7 per evaluated (pixel, Gaussian) pair."""
    return 2 + int(1e-7 * n_pairs)


def viol(got, ref, floor):
    """Elementwise bar: boolean array of violations of |got - ref| <= RTOL * max(|ref|, floor), and the worst ratio."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = RTOL * np.maximum(np.abs(ref), floor)
    d = np.abs(got - ref)
    return d > tol, (float((d / tol).max()) if d.size else 0.0)


def grad_check(name, got, ref, n_flips_allowed, pure_min=None):
    """tests/test_raster_gpu.py:_grad_check: rows with any element outside the elementwise bar are counted against the flip
    allowance, nothing may be off by more than 1e-2 of the array's scale, and the fraction of the non-zero reference elements
    that meet the pure relative bar is asserted too."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() + 1e-30
    bad, worst = viol(got, ref, GRAD_FLOOR * scale)
    rows = bad.reshape(bad.shape[0], -1).any(1).sum() if bad.ndim > 1 else bad.sum()
    nz = ref != 0
    rel = np.abs(got - ref)[nz] / np.abs(ref[nz]) if nz.any() else np.zeros(1)
    frac_pure = float((rel <= RTOL).mean())
    q50, q99 = (float(np.quantile(rel, q)) for q in (0.5, 0.99))
    print(f"grad {name}: shape {tuple(ref.shape)} non-zero refs {int(nz.sum())}; pure relative 1e-4 met by {frac_pure:.5f}; "
          f"relative error median {q50:.2e}, p99 {q99:.2e}, worst {float(rel.max()):.2e}; with the floor: worst ratio to the bar "
          f"{worst:.3f}, rows outside it {int(rows)} (allowed {2 * n_flips_allowed})")
    assert rows <= 2 * n_flips_allowed, (name, int(rows), worst)
    assert np.abs(got - ref).max() <= 1e-2 * scale, (name, float(np.abs(got - ref).max() / scale))
    assert frac_pure >= (PURE_REL_MIN_FRACTION if pure_min is None else pure_min), (name, frac_pure)
    return worst


def same_to_summation_order(a, b, tol=2e-5):
    """Two GPU evaluations of the same sums (float atomics in a different order): max |a - b| relative to the scale."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30)) <= tol


def zero_bg_params(ro, cam, sc, scale_modifier=1.0):
    from raster_helpers import oracle_params
    return oracle_params(ro, cam, sc, np.zeros(3, np.float32), scale_modifier=scale_modifier)


def depth_colours(z):
    """colors_precomp = (z, 1, 0)."""
    z = np.asarray(z, np.float32).reshape(-1)
    return np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)


def aux_forward(ro, cam, sc, z, cov_kw):
    """(params, oracle forward dict): f["color"][0] = expected depth, f["color"][1] = alpha. cov_kw: scales + rotations or
    cov3D_precomp (numpy)."""
    p0 = zero_bg_params(ro, cam, sc)
    f = ro.forward(p0, sc["means3D"], sc["opacities"], colors_precomp=depth_colours(z), **cov_kw)
    return p0, f


def aux_backward(ro, cam, sc, p0, f_aux, z, gD, gA, cov_kw):
    """Reference gradients of sum(gD * expected_depth + gA * alpha): dict over GEOMETRY_KEYS (None where not an input) plus
    "dz" [P]."""
    H, W = cam["H"], cam["W"]
    g_img = np.zeros((3, H, W), np.float32)
    if gD is not None:
        g_img[0] = np.asarray(gD, np.float32).reshape(H, W)
    if gA is not None:
        g_img[1] = np.asarray(gA, np.float32).reshape(H, W)
    b = ro.backward(p0, f_aux, g_img, sc["means3D"], colors_precomp=depth_colours(z), **cov_kw)
    dz = b["colors_precomp"][:, 0].astype(np.float64)
    V = np.asarray(cam["viewmatrix"], np.float64).reshape(4, 4)
    out = {k: (None if b[k] is None else b[k].astype(np.float64)) for k in GEOMETRY_KEYS}
    out["means3D"] = out["means3D"] + dz[:, None] * V[0:3, 2][None, :]
    out["dz"] = dz
    return out


def add_grads(a, b, keys):
    """Sum of two reference gradient dicts over `keys` (None stays None; a key missing from b counts as zero)."""
    out = dict(a)
    for k in keys:
        if a.get(k) is not None and b.get(k) is not None:
            out[k] = np.asarray(a[k], np.float64) + np.asarray(b[k], np.float64)
    return out

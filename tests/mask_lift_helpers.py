"""Reference, scenes and bars for mask lifting (raster.lift_weights: total_i = sum alpha T, hit_i,c = sum alpha T w_c).

The reference needs no oracle code of its own: with colors_precomp as the colour input, the CPU oracle's colour gradient for the
upstream image g is dL/dcolors_precomp[i, c] = sum_p alpha_i(p) T_i(p) g_c(p) over the pairs its forward composited. So with
g = (w_0, w_1, w_2) it is the hits, and with a channel of ones it is the total; more than three channels take several backward
calls on the same forward (tests/test_mask_lift_cpu.py pins this against autograd in fp64).

The bars are those the colour gradient is held to (tests/raster_aux_helpers.py): grad_check on the [P, 1 + C] array, with the
flip allowance of the evaluated pairs, and the share of pixels with a marginal decision below MAX_MARGINAL."""
import math

import numpy as np

from multiview_inpaint_amd import synthetic as syn
from raster_aux_helpers import flip_allowance, grad_check, zero_bg_params
from raster_helpers import small_scene

MAX_MARGINAL = 5e-3


def long_list_scene():
    """The long-list scene of tests/test_raster_aux_gpu.py, rebuilt: 3000 small Gaussians on 48 x 40, nearly transparent left
    of the image centre and nearly opaque right of it; tile lists of several staging batches, n_contrib in the hundreds."""
    cam, sc, bg = small_scene(3, N=3000, W=48, H=40, deg=1, pose=True, log_scale=np.log(0.04))
    rng = np.random.default_rng(3)
    V = np.asarray(cam["viewmatrix"], np.float32).reshape(4, 4)
    vx = sc["means3D"] @ V[0:3, 0] + V[3, 0]
    lo, hi = rng.uniform(0.004, 0.03, 3000), rng.uniform(0.6, 0.99, 3000)
    sc["opacities"] = np.where(vx < 0, lo, hi).astype(np.float32).reshape(sc["opacities"].shape)
    return cam, sc, bg


def oracle_forward(ro, cam, sc):
    """(params, forward dict) of the oracle with zero precomputed colours on a zero background."""
    p0 = zero_bg_params(ro, cam, sc)
    cp = np.zeros((sc["means3D"].shape[0], 3), np.float32)
    f = ro.forward(p0, sc["means3D"], sc["opacities"], colors_precomp=cp, scales=sc["scales"], rotations=sc["rotations"])
    return p0, f


def oracle_lift(ro, cam, sc, weights=None, fwd=None):
    """(params, forward dict, acc [P, 1 + C] float64): column 0 the totals, column 1 + c the hits of weights[c] ([C,H,W])."""
    p0, f = oracle_forward(ro, cam, sc) if fwd is None else fwd
    H, W, P = cam["H"], cam["W"], sc["means3D"].shape[0]
    planes = [np.ones((H, W), np.float32)]
    if weights is not None:
        planes += [np.asarray(w, np.float32).reshape(H, W) for w in weights]
    cp = np.zeros((P, 3), np.float32)
    cols = []
    for i in range(0, len(planes), 3):
        chunk = planes[i:i + 3]
        g = np.zeros((3, H, W), np.float32)
        g[:len(chunk)] = np.stack(chunk)
        b = ro.backward(p0, f, g, sc["means3D"], colors_precomp=cp, scales=sc["scales"], rotations=sc["rotations"])
        cols.append(b["colors_precomp"][:, :len(chunk)].astype(np.float64))
    return p0, f, np.concatenate(cols, 1)


def marginal_share(ro, p0, f):
    return float(((ro.margins(p0, f) & 1) != 0).mean())


def check_acc(name, got, ref, ro, p0, f, pure_min=None):
    """The bars: marginal-pixel share of the scene, then grad_check with the flip allowance of its evaluated pairs."""
    share = marginal_share(ro, p0, f)
    assert share < MAX_MARGINAL, ("margin too wide: the test would excuse too many pixels", share)
    allow = flip_allowance(int(f["n_contrib"].sum()))
    return grad_check(name, np.asarray(got, np.float64), ref, allow, pure_min=pure_min)


def weight_images(kind, H, W, seed=5):
    """Weight images of the GPU cases: C = 0 (None), a binary mask, three signed float channels, eight channels (a mix)."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        return None
    if kind == 1:
        return (rng.random((1, H, W)) < 0.4).astype(np.float32)
    if kind == 3:
        return rng.normal(size=(3, H, W)).astype(np.float32)
    if kind == 2:
        return np.stack([(rng.random((H, W)) < 0.5).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32)])
    if kind == 8:
        w = rng.normal(size=(8, H, W)).astype(np.float32)
        w[::2] = (w[::2] > 0.3).astype(np.float32)               # even channels binary, odd channels signed floats
        return w
    raise ValueError(kind)


# ---- object in front of a wall and a floor, four views (the end-to-end case) ---------------------------------------------------

OBJ_N, BG_N, OBJ_W, OBJ_H, OBJ_YAWS = 300, 1500, 96, 80, (-0.7, -0.25, 0.25, 0.7)


def orbit_camera(yaw, W=OBJ_W, H=OBJ_H, radius=3.0, fov_deg=50.0):
    """Camera on the circle of `radius` at height 0 around the origin, looking at the origin (x right, y down, z forward;
    yaw 0 stands at z = -radius)."""
    c = np.array([radius * math.sin(yaw), 0.0, -radius * math.cos(yaw)])
    fwd = -c / np.linalg.norm(c)
    right = np.array([math.cos(yaw), 0.0, math.sin(yaw)])
    down = np.array([0.0, 1.0, 0.0])
    R = np.stack([right, down, fwd], 1)                           # camera-to-world
    return syn.make_camera(W, H, fov_deg, R, -R.T @ c)


def object_scene():
    """300 object Gaussians in a ball of radius 0.35 at the origin, 1500 background Gaussians on a wall (z = 2.5) and a floor
    (y = 0.8); NumPy default_rng(7), draws in the order of this text. Returns (sc, is_object [P] bool)."""
    rng = np.random.default_rng(7)
    d = rng.normal(size=(OBJ_N, 3))
    obj = d / np.linalg.norm(d, axis=1, keepdims=True) * (0.35 * rng.random(OBJ_N) ** (1.0 / 3.0))[:, None]
    h = BG_N // 2
    wall = np.stack([rng.uniform(-3, 3, h), rng.uniform(-2.5, 0.8, h), np.full(h, 2.5)], 1)
    floor = np.stack([rng.uniform(-3, 3, h), np.full(h, 0.8), rng.uniform(-2.5, 2.5, h)], 1)
    P = OBJ_N + BG_N
    means = np.concatenate([obj, wall, floor]).astype(np.float32)
    scales = np.exp(rng.normal(math.log(0.06), 0.3, (P, 3)))
    scales[OBJ_N:] *= 2.5
    q = rng.normal(size=(P, 4))
    rotations = q / np.linalg.norm(q, axis=1, keepdims=True)
    opacities = rng.uniform(0.5, 0.95, (P, 1))
    sc = dict(means3D=means, scales=scales.astype(np.float32), rotations=rotations.astype(np.float32),
              opacities=opacities.astype(np.float32), shs=np.zeros((P, 1, 3), np.float32), sh_degree=0)
    is_obj = np.arange(P) < OBJ_N
    return sc, is_obj


def object_reference(ro):
    """Oracle side of the end-to-end case: per view the camera, the mask (alpha > 0.5 of the object rendered alone) and the
    oracle's forward; the summed oracle acc [P, 2]. Returns dict(sc, is_obj, cams, masks, fwds, acc)."""
    sc, is_obj = object_scene()
    alone = {k: (v[:OBJ_N] if k != "sh_degree" else v) for k, v in sc.items()}
    cams, masks, fwds, acc = [], [], [], 0.0
    for yaw in OBJ_YAWS:
        cam = orbit_camera(yaw)
        _, fa = oracle_forward(ro, cam, alone)
        mask = ((1.0 - fa["final_T"]) > 0.5).astype(np.float32)
        p0, f, a = oracle_lift(ro, cam, sc, mask[None])
        cams.append(cam); masks.append(mask); fwds.append((p0, f))
        acc = acc + a
    return dict(sc=sc, is_obj=is_obj, cams=cams, masks=masks, fwds=fwds, acc=acc)

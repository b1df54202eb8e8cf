"""The render backward's entry loop (csrc/raster_render.hip, render_backward_kernel) against oracle/raster_oracle.c at the
shapes where its staging and its decisions can go wrong.

A staged entry is one record of three float4 in one LDS array (centre + t2 + id, conic + opacity, colour), read at the top of
the iteration that evaluates it; the per-entry accumulator row is addressed as 36 x entry + a per-lane constant; an active
pixel is decided on o G (>= 1/255, power <= 0, position below the pixel's n_contrib) and alpha = min(0.99, o G) is formed
from the selected value. What can break: a record read with the wrong offset or from the wrong round, the accumulator row of
another entry, a wave with no live pixel, lanes outside the image, a decision at the edge of a threshold, and an
accumulator or a record that is not rewritten by the next staging round.

The bar is the one of tests/test_render_backward_reduce_gpu.py: |got - ref| <= 1e-4 max(|ref|, 1e-2 max|ref|) for every
element of every gradient array, no element excluded."""
import numpy as np
import pytest
import torch

from raster_helpers import oracle_params, small_scene

pytestmark = pytest.mark.gpu
RTOL, GRAD_FLOOR = 1e-4, 1e-2
TILE = 16


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


@pytest.fixture(scope="module")
def ro():
    from oracle import raster_oracle
    return raster_oracle


def _settings(R, cam, bg, deg):
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor(bg, device="cuda"), scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device="cuda"),
        projmatrix=torch.tensor(cam["projmatrix"], device="cuda"), sh_degree=deg, campos=torch.tensor(cam["campos"], device="cuda"),
        prefiltered=False)


def _gpu_backward(R, cam, bg, deg, g_img, means3D, opacities, **geom):
    """One forward + backward on the GPU. geom: shs plus scales + rotations or cov3D_precomp (numpy). Returns (gradients as
    numpy, RasterState)."""
    rs = _settings(R, cam, bg, deg)
    m = torch.tensor(means3D, device="cuda")
    gkw = {k: torch.tensor(v, device="cuda") for k, v in geom.items()}
    _, _, _, st = R.rasterize_forward(rs, m, torch.tensor(opacities, device="cuda"), **gkw)
    g = R.rasterize_backward(rs, st, torch.tensor(g_img, device="cuda"), m, **gkw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items() if v is not None}, st


def _worst(got, ref, keys):
    worst = {}
    for k in keys:
        a, b = got[k].astype(np.float64), np.asarray(ref[k], np.float64)
        assert a.shape == b.shape, k
        assert np.abs(b).max() > 0, k
        tol = RTOL * np.maximum(np.abs(b), GRAD_FLOOR * np.abs(b).max())
        worst[k] = float((np.abs(a - b) / tol).max())
    return worst


def _tile_max_contrib(n_contrib):
    H, W = n_contrib.shape
    return [int(n_contrib[y:y + TILE, x:x + TILE].max()) for y in range(0, H, TILE) for x in range(0, W, TILE)]


SH_KEYS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
# (W, H, N, log scale, opacity factor, sh degrees)
#   16x8          the tile's second wave lies wholly outside the image (wave_last = 0): one live wave stages, reads and adds
#   17x9          two tiles: the second has one pixel column inside, and the second wave of both one pixel row (in0 without in1);
#   17x17         four tiles, three of them with one pixel column or row inside: lanes whose n_contrib is 0 beside live ones
#   32x32_rounds  image-sized splats at 0.05 x opacity: lists and replayed lists beyond 256 entries, three staging rounds or
#                 more (asserted): the accumulator and the staged records are rewritten every round
#   40x36         degree 3 with deferred colours, the combination the benchmark runs
SHAPES = {"16x8": (16, 8, 40, np.log(0.15), 1.0, (0, 3)), "17x9": (17, 9, 60, np.log(0.15), 1.0, (0,)),
          "17x17": (17, 17, 60, np.log(0.15), 1.0, (0,)),
          "32x32_rounds": (32, 32, 400, np.log(0.6), 0.05, (0,)), "40x36": (40, 36, 80, np.log(0.15), 1.0, (3,))}
CASES = [(s, d) for s, v in SHAPES.items() for d in v[5]]


@pytest.mark.parametrize("shape,deg", CASES, ids=[f"{s}-deg{d}" for s, d in CASES])
def test_entry_loop_against_oracle(R, ro, shape, deg):
    W, H, N, log_scale, opacity, _ = SHAPES[shape]
    cam, sc, bg = small_scene(11 + deg, N=N, W=W, H=H, deg=deg, log_scale=log_scale)
    sc["opacities"] = (sc["opacities"] * opacity).astype(np.float32)
    p = oracle_params(ro, cam, sc, bg)
    okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    if shape == "32x32_rounds":
        per_tile = _tile_max_contrib(f["n_contrib"])
        print("32x32: max n_contrib per tile", per_tile)
        assert max(per_tile) > 256, "the case no longer needs three staging rounds"
    if shape == "40x36":
        from multiview_inpaint_amd import _lib
        assert _lib.lib().mvi_raster_color_mode(-1) == 1, "colours are not deferred"
    g_img = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    got, _ = _gpu_backward(R, cam, bg, deg, g_img, sc["means3D"], sc["opacities"], **okw)
    worst = _worst(got, ref, SH_KEYS)
    print(f"{shape} deg {deg}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- alpha decision edges ------------------------------------------------------------------------------------------------
# 16x16 image, one tile. Camera: identity pose, 90 degree field of view (tan = 1, focal length 8 pixels). A Gaussian at
# (ndc_x z, ndc_y z, z) with z a power of two >= 2 projects with no rounding at all (p_w = 1 / (z + 1e-7f) = 1 / z), so with
# ndc = (2 pixel + 1) / 16 - 1 its centre IS the pixel centre: dx = dy = 0, power = 0 and G = 1 there, exactly. The 3-D
# covariance is given (cov3D_precomp) as diag(s, s, 0): the Jacobian's third column meets zeros only, and the 2-D covariance
# is ((8 / z)^2 s + 0.3) I, an isotropic conic.
K_ALPHA_MIN = np.float32(1.0) / np.float32(255.0)
EDGE = {  # name: (pixel x, pixel y, z, 3-D covariance (xx, xy, yy), opacity)
    "up": (3, 3, 2.0, (0.05, 0.0, 0.05), np.nextafter(K_ALPHA_MIN, np.float32(1.0))),       # active at its centre pixel only
    "down": (11, 4, 4.0, (0.2, 0.0, 0.2), np.nextafter(K_ALPHA_MIN, np.float32(0.0))),       # never active
    # 2-D covariance (-0.8, 2; 2, -0.8): conic (0.238, 0.595; 0.595, 0.238), positive diagonal, dominant off-diagonal term,
    # indefinite. power = -0.119 (dx^2 + dy^2) - 0.595 dx dy is positive wherever dx dy < 0 is large enough
    "indefinite": (8, 9, 8.0, (-1.1, 2.0, -1.1), np.float32(0.8)),
    "one": (5, 11, 16.0, (3.2, 0.0, 3.2), np.float32(1.0)),                                   # o G = 1 at the centre: clamps to 0.99
    "wide": (8, 8, 32.0, (320.0, 0.0, 320.0), np.float32(0.5)),                               # something behind every pixel
}


def _edge_scene():
    from multiview_inpaint_amd import synthetic as syn
    cam = syn.make_camera(16, 16, 90.0)
    names = list(EDGE)
    means, cov, op = [], [], []
    for n in names:
        px, py, z, (cxx, cxy, cyy), o = EDGE[n]
        means.append((((2 * px + 1) / 16.0 - 1.0) * z, ((2 * py + 1) / 16.0 - 1.0) * z, z))
        cov.append((cxx, cxy, 0.0, cyy, 0.0, 0.0))
        op.append(o)
    rng = np.random.default_rng(5)
    shs = rng.normal(0, 1.0, (len(names), 1, 3)).astype(np.float32)
    return cam, names, np.array(means, np.float32), np.array(cov, np.float32), np.array(op, np.float32).reshape(-1, 1), shs


def test_alpha_decision_edges(R, ro):
    cam, names, means3D, cov3D, opacities, shs = _edge_scene()
    bg = np.array([0.3, 0.1, 0.7], np.float32)
    N = len(names)
    p = ro.make_params(N, 0, 1, 16, 16, cam["tanfovx"], cam["tanfovy"], 1.0, cam["viewmatrix"], cam["projmatrix"], cam["campos"], bg)
    okw = dict(shs=shs, cov3D_precomp=cov3D)
    f = ro.forward(p, means3D, opacities, **okw)
    # the construction: centres on pixel centres, exactly; isotropic conics where the covariance is isotropic
    want_xy = np.array([EDGE[n][:2] for n in names], np.float32)
    assert np.array_equal(f["xy"], want_xy), f["xy"]
    co = f["conic_opacity"]
    for i, n in enumerate(names):
        if n != "indefinite":
            assert co[i, 0] == co[i, 2] and co[i, 1] == 0.0, (n, co[i])
    yy, xx = np.mgrid[0:16, 0:16].astype(np.float32)

    def power(i):
        dx, dy = want_xy[i, 0] - xx, want_xy[i, 1] - yy
        return -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
    i_up, i_down, i_ind, i_one = (names.index(n) for n in ("up", "down", "indefinite", "one"))
    a_up = co[i_up, 3] * np.exp(power(i_up))
    assert int((a_up >= K_ALPHA_MIN).sum()) == 1 and a_up[3, 3] >= K_ALPHA_MIN          # active at its centre pixel only
    assert not (co[i_down, 3] * np.exp(np.minimum(power(i_down), 0.0)) >= K_ALPHA_MIN).any()   # never active
    p_ind = power(i_ind)
    assert (p_ind > 0).sum() > 20 and (p_ind < -0.1).sum() > 20, "the indefinite conic must have pixels on both sides"
    assert co[i_one, 3] * np.exp(power(i_one))[11, 5] == 1.0                             # o G = 1: alpha is the clamp

    g_img = np.random.default_rng(3).normal(size=(3, 16, 16)).astype(np.float32)
    ref = ro.backward(p, f, g_img, means3D, **okw)
    got, st = _gpu_backward(R, cam, bg, 0, g_img, means3D, opacities, **okw)
    assert np.array_equal(st.tensor("means2D", (N, 2), torch.float32).cpu().numpy(), want_xy)
    keys = ("means3D", "means2D", "opacities", "shs", "cov3D_precomp")
    worst = _worst(got, ref, keys)
    print("alpha edges: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    touched = st.tensor("grad_support", (N,), torch.uint8).cpu().numpy()
    for k in keys:
        assert not got[k][i_down].any(), (k, got[k][i_down])       # exactly zero, every component
        assert not np.asarray(ref[k])[i_down].any(), k
    assert touched[i_down] == 0 and touched[i_up] == 1 and touched[i_one] == 1 and touched[i_ind] == 1, touched


def test_one_tile_is_deterministic(R, ro):
    """16x16, one tile, N = 300, lists beyond 128 entries: every Gaussian receives exactly one row atomic onto a zeroed row, and
    the two waves' LDS adds into one accumulator element commute, so two runs agree in every bit of every gradient."""
    W = H = 16
    cam, sc, bg = small_scene(17, N=300, W=W, H=H, deg=0, log_scale=np.log(0.6))
    sc["opacities"] = (sc["opacities"] * 0.05).astype(np.float32)
    p = oracle_params(ro, cam, sc, bg)
    okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    r = f["ranges"].astype(np.int64)
    assert r.shape[0] == 1 and r[0, 1] - r[0, 0] > 128 and int(f["n_contrib"].max()) > 128, (r, int(f["n_contrib"].max()))
    g_img = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    a, _ = _gpu_backward(R, cam, bg, 0, g_img, sc["means3D"], sc["opacities"], **okw)
    b, _ = _gpu_backward(R, cam, bg, 0, g_img, sc["means3D"], sc["opacities"], **okw)
    for k in SH_KEYS:
        assert np.abs(a[k]).max() > 0, k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (k, int((a[k] != b[k]).sum()))
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    worst = _worst(a, ref, SH_KEYS)
    print("one tile, N = 300: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst

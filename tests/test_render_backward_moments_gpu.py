"""The render backward's moments (csrc/raster_render.hip, render_backward_kernel): a lane owns two pixels with the same x and
adjacent y and adds them BEFORE it multiplies by what they share,
    s = W0 + W1,  m_x = s dx,  m_xx = m_x dx,  m_y = W0 dy0 + W1 dy1,  m_xy = m_y dx,  m_yy = fma(W1 dy1, dy1, (W0 dy0) dy0),
and the colour moments as one product and one fma. What can break: a pixel's weight meeting the other pixel's dy, a product
that is exact only while dy or dx is 0, the fma's operand order. The cases put a Gaussian exactly on the lane's upper pixel
centre (dy = (0, -1)), on the lower one (dy = (1, 0)), exactly between them (dy = (0.5, -0.5)), each at dx = 0 for the lanes of
its column and at dx != 0 in every lane; what they hold to the oracle is dL/dmean2D and the three conic gradients. Two small
random scenes (17x17, 16x8) cover the lanes of which only one pixel, or none, lies inside the image.

The bar is the one of tests/test_render_backward_reduce_gpu.py against oracle/raster_oracle.c: |got - ref| <= 1e-4 max(|ref|,
1e-2 max|ref|) for every element of every gradient array, no element excluded."""
import numpy as np
import pytest
import torch

from raster_helpers import oracle_params, small_scene

pytestmark = pytest.mark.gpu
RTOL, GRAD_FLOOR = 1e-4, 1e-2


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


@pytest.fixture(scope="module")
def ro():
    from oracle import raster_oracle
    return raster_oracle


# ---- the kernel -------------------------------------------------------------------------------------------------------------
def _settings(R, cam, bg, deg):
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor(bg, device="cuda"), scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device="cuda"),
        projmatrix=torch.tensor(cam["projmatrix"], device="cuda"), sh_degree=deg, campos=torch.tensor(cam["campos"], device="cuda"),
        prefiltered=False)


def _gpu_backward(R, cam, bg, deg, g_img, means3D, opacities, **geom):
    rs = _settings(R, cam, bg, deg)
    m = torch.tensor(means3D, device="cuda")
    gkw = {k: torch.tensor(v, device="cuda") for k, v in geom.items()}
    _, _, _, st = R.rasterize_forward(rs, m, torch.tensor(opacities, device="cuda"), **gkw)
    g = R.rasterize_backward(rs, st, torch.tensor(g_img, device="cuda"), m, **gkw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items() if v is not None}


def _worst(got, ref, keys):
    worst = {}
    for k in keys:
        a, b = got[k].astype(np.float64), np.asarray(ref[k], np.float64)
        assert a.shape == b.shape, k
        assert np.abs(b).max() > 0, k
        tol = RTOL * np.maximum(np.abs(b), GRAD_FLOOR * np.abs(b).max())
        worst[k] = float((np.abs(a - b) / tol).max())
    return worst


SH_KEYS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
# (W, H, N): a lane's sum over its two pixels where only ONE of them is inside the image, and where none is.
#   17x17   four tiles, three with one pixel column or row inside: in the tiles of the second tile row a lane's upper pixel (y = 16)
#           is inside and its lower (y = 17) is not, and it must enter every moment as exactly nothing (contributors on row 16 asserted)
#   16x8    the tile's second wave lies wholly outside the image
EDGE_SHAPES = {"17x17": (17, 17, 60), "16x8": (16, 8, 40)}


@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
def test_one_pixel_of_the_lane_outside_the_image(R, ro, shape):
    W, H, N = EDGE_SHAPES[shape]
    cam, sc, bg = small_scene(23, N=N, W=W, H=H, deg=0, log_scale=np.log(0.15))
    p = oracle_params(ro, cam, sc, bg)
    okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    if shape == "17x17":
        assert int(f["n_contrib"][16, :].min()) > 0 and int(f["n_contrib"][:, 16].min()) > 0, "row / column 16 has no contributor"
    g_img = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    got = _gpu_backward(R, cam, bg, 0, g_img, sc["means3D"], sc["opacities"], **okw)
    worst = _worst(got, ref, SH_KEYS)
    print(f"{shape}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- hand-placed Gaussians ----------------------------------------------------------------------------------------------------
# 16x16 image, one tile; identity pose, 90 degree field of view (focal length 8 pixels). A Gaussian at (ndc_x z, ndc_y z, z)
# with z a power of two projects without rounding, so with ndc = (2 pixel + 1) / 16 - 1 its centre is at `pixel` exactly
# (half-integer pixels included). cov3D_precomp = diag(s, s, 0): the 2-D covariance is ((8 / z)^2 s + 0.3) I.
def _placed(ro, items):
    """items: (pixel x, pixel y, z, s, opacity) -> camera, oracle params, means3D, cov3D, opacities, shs"""
    from multiview_inpaint_amd import synthetic as syn
    cam = syn.make_camera(16, 16, 90.0)
    means = np.array([(((2 * px + 1) / 16.0 - 1.0) * z, ((2 * py + 1) / 16.0 - 1.0) * z, z) for px, py, z, _, _ in items], np.float32)
    cov = np.array([(s, 0.0, 0.0, s, 0.0, 0.0) for _, _, _, s, _ in items], np.float32)
    op = np.array([o for *_, o in items], np.float32).reshape(-1, 1)
    shs = np.random.default_rng(5).normal(0, 1.0, (len(items), 1, 3)).astype(np.float32)
    bg = np.array([0.3, 0.1, 0.7], np.float32)
    p = ro.make_params(len(items), 0, 1, 16, 16, cam["tanfovx"], cam["tanfovy"], 1.0, cam["viewmatrix"], cam["projmatrix"],
                       cam["campos"], bg)
    return cam, bg, p, means, cov, op, shs


PLACED_KEYS = ("means3D", "means2D", "opacities", "shs", "cov3D_precomp")


# the factored moments: a lane owns pixels (x, 2 k) and (x, 2 k + 1). Centre on the upper pixel (dy = (0, -1)), on the lower
# (dy = (1, 0)), exactly between (dy = (0.5, -0.5)); dx = 0 for the lanes of its column, and a centre at x + 0.5 has dx != 0 in
# every lane. One Gaussian per scene: the floor of the bar is that Gaussian's own largest gradient.
FACTOR = {"upper": (5.0, 6.0), "lower": (5.0, 7.0), "between": (5.0, 6.5),
          "upper_dx": (5.5, 6.0), "lower_dx": (5.5, 7.0), "between_dx": (5.5, 6.5)}


@pytest.mark.parametrize("case", list(FACTOR))
def test_factored_moments_at_pixel_centres(R, ro, case):
    px, py = FACTOR[case]
    cam, bg, p, means3D, cov3D, opacities, shs = _placed(ro, [(px, py, 8.0, 2.0, 0.8)])
    okw = dict(shs=shs, cov3D_precomp=cov3D)
    f = ro.forward(p, means3D, opacities, **okw)
    assert np.array_equal(f["xy"], np.array([[px, py]], np.float32)), f["xy"]
    co = f["conic_opacity"][0]
    assert co[0] == co[2] and co[1] == 0.0, co
    g_img = np.random.default_rng(3).normal(size=(3, 16, 16)).astype(np.float32)
    ref = ro.backward(p, f, g_img, means3D, **okw)
    got = _gpu_backward(R, cam, bg, 0, g_img, means3D, opacities, **okw)
    worst = _worst(got, ref, PLACED_KEYS)             # means2D and cov3D_precomp carry dL/dmean2D and the three conic gradients
    print(f"{case}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_one_tile_is_deterministic(R, ro):
    """16x16, one tile, N = 300, lists beyond 128 entries: an accumulator row receives one add per wave and entry, two addends
    onto zero commute, and every Gaussian gets one row atomic: with the factored moments two runs still agree in every bit."""
    W = H = 16
    cam, sc, bg = small_scene(17, N=300, W=W, H=H, deg=0, log_scale=np.log(0.6))
    sc["opacities"] = (sc["opacities"] * 0.05).astype(np.float32)
    p = oracle_params(ro, cam, sc, bg)
    okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    r = f["ranges"].astype(np.int64)
    assert r.shape[0] == 1 and r[0, 1] - r[0, 0] > 128 and int(f["n_contrib"].max()) > 128, (r, int(f["n_contrib"].max()))
    g_img = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    a = _gpu_backward(R, cam, bg, 0, g_img, sc["means3D"], sc["opacities"], **okw)
    b = _gpu_backward(R, cam, bg, 0, g_img, sc["means3D"], sc["opacities"], **okw)
    for k in SH_KEYS:
        assert np.abs(a[k]).max() > 0, k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (k, int((a[k] != b[k]).sum()))
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    worst = _worst(a, ref, SH_KEYS)
    print("one tile, N = 300: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst

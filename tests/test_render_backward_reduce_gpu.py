"""The render backward's per-Gaussian moment sums: wave_sum9 (csrc/raster_render.hip) on its own through the diagnostics
entry mvi_raster_dev_wave_sum9, and the kernel that uses it against the CPU oracle at the shapes where the reduction and
its accumulator can go wrong.

The nine moments of an entry are summed over the 64 lanes of a wave in registers (a halving butterfly: DPP adds, then the
gfx950 lane swaps) and nine owner lanes add the totals into the block's LDS accumulator. What can break: a lane routed to
the wrong moment or dropped (the exact tests), the rounding of the tree (the float test), lanes that contribute nothing
(pixels outside the image, a whole wave outside it), both waves adding into one accumulator row, and the accumulator
being reused by the next staging round."""
import ctypes as C

import numpy as np
import pytest
import torch

from raster_helpers import oracle_params, small_scene

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)


def _wave_sum9(x):
    """x [n_waves, 9, 64] float32 (numpy) -> [n_waves, 9] through the device function."""
    from multiview_inpaint_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert x.dtype == np.float32 and x.shape[1:] == (9, 64)
    d_in = torch.tensor(x, device="cuda").contiguous()
    d_out = torch.full((x.shape[0], 9), float("nan"), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().mvi_raster_dev_wave_sum9(C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), x.shape[0], None),
               "mvi_raster_dev_wave_sum9")
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_wave_sum9_exact_integers():
    """in[w][m][l] = (l + 1)(m + 1) + 64 w: every partial sum is an integer below 2^24, so any summation order is exact and
    the result must EQUAL the numpy sum. A lane added into the wrong moment, twice or not at all changes a sum."""
    w, m, l = np.meshgrid(np.arange(5), np.arange(9), np.arange(64), indexing="ij")
    x = ((l + 1) * (m + 1) + 64 * w).astype(np.float32)
    want = x.astype(np.float64).sum(2)
    assert want.max() < 2 ** 24
    got = _wave_sum9(x)
    assert np.array_equal(got, want.astype(np.float32)), (got, want)


def test_wave_sum9_single_lane_each_position():
    """One non-zero lane, at each of the 64 positions for each of the nine moments (576 waves, one launch): the value must
    arrive in its own moment's total and nowhere else."""
    x = np.zeros((9 * 64, 9, 64), np.float32)
    want = np.zeros((9 * 64, 9), np.float32)
    for m in range(9):
        for l in range(64):
            w = m * 64 + l
            x[w, m, l] = want[w, m] = float(w + 1)
    got = _wave_sum9(x)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(w) // 64, int(w) % 64, int(m), float(got[w, m])) for w, m in bad[:8]]   # (moment, lane, output, value)


def test_wave_sum9_floats():
    """Seeded normal inputs against the float64 sum: |got - ref| <= 64 eps32 sum|x| per output. A pairwise tree over 64 values
    is six roundings deep, each at most eps32 / 2 of a partial sum that is at most sum|x|: 3 eps32 sum|x|, inside the bar."""
    x = np.random.default_rng(20).normal(size=(7, 9, 64)).astype(np.float32)
    x[1] *= 1e4
    x[2] *= 1e-4
    ref = x.astype(np.float64).sum(2)
    bound = 64.0 * EPS32 * np.abs(x.astype(np.float64)).sum(2)
    got = _wave_sum9(x).astype(np.float64)
    err = np.abs(got - ref)
    print("wave_sum9 floats: worst |got - ref| / (eps32 sum|x|) =", float((err / (EPS32 * np.abs(x.astype(np.float64)).sum(2))).max()))
    assert (err <= bound).all(), float((err / bound).max())


# ---- the kernel against oracle/raster_oracle.c -------------------------------------------------------------------------
RTOL, GRAD_FLOOR = 1e-4, 1e-2
# (W, H, N, log scale, opacity factor): 16x8 = the second wave of the only tile is wholly outside the image; 17x9 = partial
# columns and rows, lanes that contribute zeros; 40x36 / N = 80 = the small scene of raster_helpers; 32x32 / N = 400 with
# splats about as large as the image and faint opacities = tile lists AND replayed lists longer than 128 entries, so the
# backward stages two rounds and clears and refills its accumulator (asserted below).
SHAPES = {"16x8": (16, 8, 80, np.log(0.15), 1.0), "17x9": (17, 9, 80, np.log(0.15), 1.0), "40x36": (40, 36, 80, np.log(0.15), 1.0),
          "32x32_two_rounds": (32, 32, 400, np.log(0.6), 0.05)}


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


@pytest.fixture(scope="module")
def ro():
    from oracle import raster_oracle
    return raster_oracle


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_against_oracle(R, ro, shape, deg):
    """Every gradient element within |got - ref| <= 1e-4 max(|ref|, 1e-2 max|ref|) of the oracle's, no element excluded (the
    elementwise rule of tests/test_raster_gpu.py::test_backward_parity_small, without its allowance for flipped decisions)."""
    W, H, N, log_scale, opacity = SHAPES[shape]
    cam, sc, bg = small_scene(11 + deg, N=N, W=W, H=H, deg=deg, log_scale=log_scale)
    sc["opacities"] = (sc["opacities"] * opacity).astype(np.float32)
    p = oracle_params(ro, cam, sc, bg)
    okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    if shape == "32x32_two_rounds":
        r = f["ranges"].astype(np.int64)
        assert (r[:, 1] - r[:, 0]).max() > 128 and int(f["n_contrib"].max()) > 128, "the case no longer needs two staging rounds"
    g_img = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    b = ro.backward(p, f, g_img, sc["means3D"], **okw)
    t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}
    rs = R.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.tensor(bg, device="cuda"),
        scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device="cuda"),
        projmatrix=torch.tensor(cam["projmatrix"], device="cuda"), sh_degree=deg, campos=torch.tensor(cam["campos"], device="cuda"),
        prefiltered=False)
    gkw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    color, radii, depth, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
    g = R.rasterize_backward(rs, st, torch.tensor(g_img, device="cuda"), t["means3D"], **gkw)
    torch.cuda.synchronize()
    worst = {}
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        got, ref = g[k].cpu().numpy().astype(np.float64), np.asarray(b[k], np.float64)
        assert got.shape == ref.shape, k
        assert np.abs(ref).max() > 0, k
        tol = RTOL * np.maximum(np.abs(ref), GRAD_FLOOR * np.abs(ref).max())
        worst[k] = float((np.abs(got - ref) / tol).max())
    print(f"{shape} deg {deg}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst

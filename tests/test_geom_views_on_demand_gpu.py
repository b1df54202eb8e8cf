"""The views `depths`, `cov3D_a`, `cov3D_b` and `tiles_touched` of a forward: no kernel of the default path reads them, the
forward does not write them, and RasterState.tensor() has them filled by mvi_raster_materialize_geom_views from the forward's
own inputs. 96 x 64, P around a wave (64) and a depth-sort tile (2048), with scale / rotation input, cov3D_precomp input, raw
parameters and binning version 1 (whose forward still writes tiles_touched itself).

Bars: bit-equal with oracle/raster_oracle.c on the visible set, as tests/test_raster_gpu.py::_check_forward compares the same
views; a backward behind a read within |got - ref| <= 1e-4 max(|ref|, 1e-2 max|ref|) of the oracle's, the rule of
tests/test_binning_loads_gpu.py::test_backward_after_reading_tile_ids (raw parameters: against the backward without a read,
for the reason given in the test)."""
import numpy as np
import pytest
import torch

from multiview_inpaint_amd import synthetic as syn
from raster_helpers import oracle_params

pytestmark = pytest.mark.gpu
RTOL, GRAD_FLOOR = 1e-4, 1e-2
BG = np.array([0.3, 0.1, 0.7], np.float32)
W, H, DEG = 96, 64, 1


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


@pytest.fixture(scope="module")
def ro():
    from oracle import raster_oracle
    return raster_oracle


def _settings(R, cam):
    d = "cuda"
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.tensor(BG, device=d),
        scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device=d), projmatrix=torch.tensor(cam["projmatrix"], device=d),
        sh_degree=DEG, campos=torch.tensor(cam["campos"], device=d), prefiltered=False)


def _scene(P, seed=50):
    cam = syn.make_camera(W, H, 50.0)
    sc = syn.make_scene(P, cam, DEG, seed=seed, log_scale_mean=np.log(0.05), zmin=1.0, zmax=6.0)
    m = sc["means3D"].copy()
    m[:, :2] *= 0.8                                    # P = 1 is inside the image
    if P > 8:
        m[P // 2::7, 2] *= -1.0                        # and some Gaussians are behind the camera: their views stay unwritten
    sc["means3D"] = m
    return cam, sc


def _views(st):
    P = st.P
    return dict(depths=st.tensor("depths", (P,), torch.float32).cpu().numpy().view(np.uint32),
                cov3D_a=st.tensor("cov3D_a", (P, 4), torch.float32).cpu().numpy().view(np.uint32),
                cov3D_b=st.tensor("cov3D_b", (P, 2), torch.float32).cpu().numpy().view(np.uint32),
                tiles_touched=st.tensor("tiles_touched", (P,), torch.int32).cpu().numpy().view(np.uint32))


def _bar(tag, got, ref, names):
    worst = {}
    for k, r in names:
        a, b = got[k].cpu().numpy().astype(np.float64), np.asarray(ref[r], np.float64).reshape(got[k].shape)
        assert np.abs(b).max() > 0, k
        tol = RTOL * np.maximum(np.abs(b), GRAD_FLOOR * np.abs(b).max())
        worst[k] = float((np.abs(a - b) / tol).max())
    print(f"{tag}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


@pytest.mark.parametrize("variant", ["scale_rot", "cov3D_precomp", "raw", "binning_v1"])
@pytest.mark.parametrize("P", [1, 63, 65, 2049])
def test_views_equal_the_oracle_and_a_read_does_not_disturb_the_backward(R, ro, P, variant):
    from multiview_inpaint_amd import _lib
    L = _lib.lib()
    cam, sc = _scene(P)
    t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}
    rs = _settings(R, cam)
    raw = None
    if variant == "raw":
        # raw parameters whose activations (the kernels' own expressions: train_ops.activate_gaussians) the oracle is then fed with
        from multiview_inpaint_amd import train_ops as T
        gen = torch.Generator("cuda").manual_seed(1)
        raw = dict(xyz=t["means3D"], dc=t["shs"][:, :1].contiguous(), rest=t["shs"][:, 1:].contiguous(),
                   o=torch.logit(t["opacities"].clamp(1e-4, 1 - 1e-4)), s=torch.log(t["scales"]),
                   q=t["rotations"] * (0.5 + torch.rand(P, 1, device="cuda", generator=gen)))
        scales, rots, opac, shs = T.activate_gaussians(raw["s"], raw["q"], raw["o"], raw["dc"], raw["rest"])
        sc = dict(sc, scales=scales.cpu().numpy(), rotations=rots.cpu().numpy(), opacities=opac.cpu().numpy().reshape(P, 1),
                  shs=shs.cpu().numpy())
    p = oracle_params(ro, cam, sc, BG)
    okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    gkw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    if variant == "cov3D_precomp":
        c6 = f["cov3D"].copy()
        okw = dict(shs=sc["shs"], cov3D_precomp=c6)
        gkw = dict(shs=t["shs"], cov3D_precomp=torch.tensor(c6, device="cuda"))
        f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    g_img = np.random.default_rng(7).normal(size=(3, H, W)).astype(np.float32)
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    gi = torch.tensor(g_img, device="cuda")
    vis = f["radii"] > 0
    assert vis.any()

    def forward():
        if variant == "raw":
            return R.rasterize_forward_raw(rs, raw["xyz"], raw["dc"], raw["rest"], raw["o"], raw["s"], raw["q"])
        prev = L.mvi_raster_binning_version(1 if variant == "binning_v1" else 0)
        try:
            return R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
        finally:
            L.mvi_raster_binning_version(prev)

    def backward(st):
        if variant == "raw":
            g = R.rasterize_backward_raw(rs, st, gi, raw["xyz"], raw["dc"], raw["rest"], raw["o"], raw["s"], raw["q"])
            return g, ()
        g = R.rasterize_backward(rs, st, gi, t["means3D"], **gkw)
        return g, tuple((k, k) for k in ("means3D", "means2D", "opacities", "shs") +
                        (("cov3D_precomp",) if variant == "cov3D_precomp" else ("scales", "rotations")))

    _, radii, _, st = forward()
    assert np.array_equal(radii.cpu().numpy(), f["radii"]) and st.D == f["num_rendered"]
    v1 = _views(st)
    v2 = _views(st)
    for k in v1:
        assert np.array_equal(v1[k], v2[k]), f"{k}: two reads differ"
    assert np.array_equal(v1["tiles_touched"], f["tiles_touched"])
    assert np.array_equal(v1["depths"][vis], f["depths"].view(np.uint32)[vis])
    cov = np.concatenate([v1["cov3D_a"], v1["cov3D_b"]], 1)
    if variant != "raw":
        assert np.array_equal(cov[vis], f["cov3D"].view(np.uint32)[vis])
    else:
        # the forward normalises the quaternion without fused multiply-adds and the activation kernel that fed the oracle with
        # them: the two unit quaternions differ by an ulp per component, R = R(q) by a few, and an element of (R S)(R S)^T is
        # three products of such entries: within 32 eps32 of the row's largest element
        cf, rf = cov.view(np.float32).astype(np.float64)[vis], f["cov3D"].astype(np.float64)[vis]
        assert (np.abs(cf - rf) <= 32 * np.finfo(np.float32).eps * np.abs(rf).max(1, keepdims=True)).all()
    if variant == "cov3D_precomp":
        vz = sc["means3D"].astype(np.float64) @ cam["viewmatrix"][:3, 2].astype(np.float64) + float(cam["viewmatrix"][3, 2])
        front = vz > 0.2 + 1e-4                       # the forward's near-plane cull, away from its rounding
        assert front.sum() >= vis.sum() and np.array_equal(cov[front], c6.view(np.uint32)[front]), "the view is not the input"
    # the backward behind the reads, and one on a fresh forward that nobody read: both at the oracle's bar
    g_read, names = backward(st)
    _, _, _, st0 = forward()
    g_plain, _ = backward(st0)
    torch.cuda.synchronize()
    if names:
        _bar(f"{variant} P {P} after a read", g_read, ref, names)
        _bar(f"{variant} P {P} no read", g_plain, ref, names)
    if variant == "raw":
        # No oracle bar in raw mode. That bar rests on per-Gaussian floats that are bit-equal on both sides, and the quaternion
        # the kernels normalise themselves is an ulp away from any the CPU could be handed (see above); the conic of an
        # elongated Gaussian amplifies that ulp past 1e-4 (measured at P = 2049: up to 4.9 bars, with or without a read).
        # tests/test_raster_gpu.py holds the raw path to the standard one. Here: the backward behind a read against the
        # backward nobody read before, which differ by the order of the float atomics only (that file's 2e-5 of the scale).
        for k in ("xyz", "means2D", "opacity", "scaling", "rotation", "features_dc", "features_rest"):
            a, b = g_read[k].cpu().numpy().astype(np.float64), g_plain[k].cpu().numpy().astype(np.float64)
            assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 2e-5 * np.abs(b).max(), k
    # a read AFTER the backward gives the same views
    v3 = _views(st)
    for k in v1:
        assert np.array_equal(v1[k], v3[k]), f"{k}: changed by the backward"


@pytest.mark.parametrize("version", [2, 1])
def test_everything_culled(R, version):
    """Nothing in front of the camera (D = 0): the views read, and tiles_touched is zero for every Gaussian."""
    from multiview_inpaint_amd import _lib
    L = _lib.lib()
    P = 500
    cam, sc = _scene(P, seed=51)
    m = sc["means3D"].copy()
    m[:, 2] = -np.abs(m[:, 2])
    t = {k: torch.tensor(v, device="cuda") for k, v in dict(sc, means3D=m).items() if k != "sh_degree"}
    prev = L.mvi_raster_binning_version(version)
    try:
        _, radii, _, st = R.rasterize_forward(_settings(R, cam), t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"],
                                              rotations=t["rotations"])
    finally:
        L.mvi_raster_binning_version(prev)
    v = _views(st)
    assert st.D == 0 and int((radii != 0).sum()) == 0
    assert v["tiles_touched"].shape == (P,) and not v["tiles_touched"].any()
    assert v["depths"].shape == (P,) and v["cov3D_a"].shape == (P, 4) and v["cov3D_b"].shape == (P, 2)

"""The per-Gaussian chain rule of the default backward (csrc/raster_preprocess.hip, preprocess_backward_sparse_kernel) with the
compaction of the support flags inside it, and with cov3D derived again from scale and rotation instead of read back.

A one-wave block owns 1024 consecutive flags (16 per lane), compacts the indices of its touched Gaussians into LDS and takes
them from there in rounds of 64. What can break: a lane's 16 flags straddling the end of the scene, the last block holding one
flag, a block with no flag set, a block whose list needs more than one round (more than 64 touched) up to all 1024, an index
written to the wrong list slot (a Gaussian skipped or done twice), and the paths the kernel takes for its inputs: SH degree 0
and 3, scale / rotation or cov3D_precomp, rows at 4-byte alignment. Every case compares the sparse kernel with the dense one
on the same state, and with oracle/raster_oracle.c under the elementwise rule of tests/test_render_backward_reduce_gpu.py
(|got - ref| <= 1e-4 max(|ref|, 1e-2 max|ref|), no element excluded).

The scenes keep the number of Gaussians that contribute to a pixel small (footprints of a few pixels, or few Gaussians). The
oracle bar is met by the render backward, which feeds this kernel, only there: both sides carry a pixel's transmittance as an
fp32 product over its contributors with exponentials that differ by an ulp, and the accumulation rows are sums of as many
terms. Measured, with the parent's kernels exactly as with these: 4097 splats of ~30 pixels each on 48 x 32 give 1.11 bars
on dL/dscales, 1024 splats that all cover a 16 x 16 image 2.5 bars on dL/dmeans3D, 70 image-sized splats with rotation
gradients that cancel over the image 1.19 bars on dL/drotations; the scenes below at most 0.56 bars."""
import ctypes as C

import numpy as np
import pytest
import torch

from multiview_inpaint_amd import synthetic as syn
from raster_helpers import oracle_params, small_scene
from test_raster_gpu import _same_to_summation_order

pytestmark = pytest.mark.gpu
RTOL, GRAD_FLOOR = 1e-4, 1e-2
BG = np.array([0.3, 0.1, 0.7], np.float32)


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


@pytest.fixture(scope="module")
def ro():
    from oracle import raster_oracle
    return raster_oracle


def _settings(R, cam, deg):
    d = "cuda"
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.tensor(BG, device=d),
        scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device=d), projmatrix=torch.tensor(cam["projmatrix"], device=d),
        sh_degree=deg, campos=torch.tensor(cam["campos"], device=d), prefiltered=False)


def _scene(P, W, H, deg, seed, log_scale, opacity=1.0):
    cam = syn.make_camera(W, H, 50.0)
    sc = syn.make_scene(P, cam, deg, seed=seed, log_scale_mean=log_scale, zmin=1.0, zmax=6.0)
    m = sc["means3D"].copy()
    m[:, :2] *= 0.8                                    # every centre inside the image: P = 1 is visible
    sc["means3D"] = m
    sc["opacities"] = (sc["opacities"] * opacity).astype(np.float32)
    return cam, sc


def _to_dev(sc):
    return {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}


def _inputs(ro, cam, sc, mode):
    """(oracle keywords, GPU keywords) for scale / rotation input or the same covariances handed in as cov3D_precomp."""
    t = _to_dev(sc)
    if mode == "cov":
        p = oracle_params(ro, cam, sc, BG)
        c6 = ro.forward(p, sc["means3D"], sc["opacities"], shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"],
                        render=False)["cov3D"].copy()
        return dict(shs=sc["shs"], cov3D_precomp=c6), dict(shs=t["shs"], cov3D_precomp=torch.tensor(c6, device="cuda")), t
    return (dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"]),
            dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"]), t)


def _names(mode):
    return ("means3D", "means2D", "opacities", "shs") + (("cov3D_precomp",) if mode == "cov" else ("scales", "rotations"))


def _oracle_bar(tag, g, ref, names):
    worst = {}
    for k in names:
        got, want = g[k].cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
        assert got.shape == want.shape and np.abs(want).max() > 0, k
        tol = RTOL * np.maximum(np.abs(want), GRAD_FLOOR * np.abs(want).max())
        worst[k] = float((np.abs(got - want) / tol).max())
    print(f"{tag}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


def _sparse_dense_oracle(R, ro, cam, sc, deg, mode, g_img, tag):
    """Sparse and dense backward on one state, both against each other and against the oracle. Returns the support flags."""
    from multiview_inpaint_amd import _lib
    L = _lib.lib()
    okw, gkw, t = _inputs(ro, cam, sc, mode)
    p = oracle_params(ro, cam, sc, BG)
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    rs = _settings(R, cam, deg)
    P = sc["means3D"].shape[0]
    _, radii, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
    gi = torch.tensor(g_img, device="cuda")
    prev = L.mvi_raster_backward_mode(0)
    try:
        sparse = R.rasterize_backward(rs, st, gi, t["means3D"], **gkw)
        support = st.tensor("grad_support", (P,), torch.uint8).bool()
        L.mvi_raster_backward_mode(1)
        dense = R.rasterize_backward(rs, st, gi, t["means3D"], **gkw)
    finally:
        L.mvi_raster_backward_mode(prev)
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy(), f["radii"])
    assert int(support.sum()) <= int((radii > 0).sum())
    names = _names(mode)
    for k in names:
        a, b = sparse[k], dense[k]
        assert a.shape == b.shape, k
        assert _same_to_summation_order(a.cpu().numpy(), b.cpu().numpy()), (tag, "sparse vs dense", k)
        assert (a.reshape(P, -1)[~support] == 0).all() and (b.reshape(P, -1)[~support] == 0).all(), (tag, k)
    _oracle_bar(tag + " sparse", sparse, ref, names)
    _oracle_bar(tag + " dense", dense, ref, names)
    return support, radii


@pytest.mark.parametrize("mode", ["sr", "cov"])
@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 4097])
def test_scene_ends_around_a_block_of_flags(R, ro, P, deg, mode):
    """48 x 32. The scene ends one flag short of a block's 1024, at it, one past it (a last block that holds ONE flag), and
    at 4097 = four full blocks and one flag; P = 1 is a single lane of a single block. Splats below a pixel (the footprint is
    the low-pass filter's: about a dozen pixels) at a third of the usual opacity: nearly every Gaussian is touched."""
    cam, sc = _scene(P, 48, 32, deg, seed=40 + deg, log_scale=np.log(0.01), opacity=0.3)
    g_img = np.random.default_rng(3).normal(size=(3, 32, 48)).astype(np.float32)
    support, radii = _sparse_dense_oracle(R, ro, cam, sc, deg, mode, g_img, f"P {P} deg {deg} {mode}")
    assert int(support.sum()) > 0
    if P > 1000:
        per_block = np.add.reduceat(support.cpu().numpy().astype(np.int64), np.arange(0, P, 1024))
        assert per_block.max() > 64, "no block needs a second round"


def test_every_gaussian_touched_image_sized_splats(R, ro):
    """70 faint splats about as large as the 32 x 32 image (the generator and scale of the two-round case of
    tests/test_render_backward_reduce_gpu.py), one opacity for all: above the 1/255 below which an entry is skipped, and
    0.95^70 = 0.03 keeps every pixel above the 1e-4 at which it stops. Every Gaussian receives a gradient: two rounds of one
    block, the second with 6 lanes."""
    cam, sc, _ = small_scene(14, N=70, W=32, H=32, deg=3, log_scale=np.log(0.6))
    sc["opacities"] = np.full_like(sc["opacities"], 0.05)
    g_img = np.random.default_rng(3).normal(size=(3, 32, 32)).astype(np.float32)
    support, _ = _sparse_dense_oracle(R, ro, cam, sc, 3, "sr", g_img, "70 image-sized")
    assert bool(support.all()), int(support.sum())


def test_every_flag_of_a_block_set(R, ro):
    """1024 half-pixel splats on a 32 x 32 grid, 4 pixels apart in a 128 x 128 image, opacity 0.5: nobody is occluded, every
    flag of the one block is set: 64 x 16 list entries, 16 full rounds."""
    n, W, H = 32, 128, 128
    cam = syn.make_camera(W, H, 50.0)
    sc = syn.make_scene(n * n, cam, 3, seed=44, log_scale_mean=np.log(0.012), zmin=1.0, zmax=6.0)
    u = ((np.arange(n) + 0.5) / n * 2 - 1) * 0.95
    gx, gy = np.meshgrid(u, u)
    sc["means3D"] = np.stack([gx.ravel() * 3.0 * cam["tanfovx"], gy.ravel() * 3.0 * cam["tanfovy"], np.full(n * n, 3.0)], 1).astype(np.float32)
    sc["opacities"] = np.full_like(sc["opacities"], 0.5)
    g_img = np.random.default_rng(4).normal(size=(3, H, W)).astype(np.float32)
    support, _ = _sparse_dense_oracle(R, ro, cam, sc, 3, "sr", g_img, "1024 on a grid")
    assert bool(support.all()), int(support.sum())


def test_zero_upstream_gradient_leaves_an_empty_support(R):
    """dL/dcolour = 0: no flag is set, no block finds work, and every output is exactly zero (the render backward zeroed it)."""
    P = 1025
    cam, sc = _scene(P, 48, 32, 3, seed=45, log_scale=np.log(0.05))
    t = _to_dev(sc)
    rs = _settings(R, cam, 3)
    gkw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    _, radii, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
    out = {k: torch.full(s, float("nan"), device="cuda") for k, s in
           (("means3D", (P, 3)), ("means2D", (P, 3)), ("opacities", (P, 1)), ("shs", (P, 16, 3)), ("scales", (P, 3)), ("rotations", (P, 4)))}
    g = R.rasterize_backward(rs, st, torch.zeros(3, 32, 48, device="cuda"), t["means3D"], out=out, **gkw)
    torch.cuda.synchronize()
    assert int((radii > 0).sum()) > 100
    assert int(st.tensor("grad_support", (P,), torch.uint8).sum()) == 0
    for k in out:
        assert g[k].data_ptr() == out[k].data_ptr() and bool((g[k] == 0).all()), k


def test_hand_placed_support_at_block_edges(R, ro):
    """P = 2049, every Gaussian behind the camera except indices 0, 1023, 1024 and P - 1, which sit side by side in the image:
    the first and the last flag of the first block, the first flag of the second, and a third block that holds one flag."""
    P, W, H, deg = 2049, 64, 32, 3
    cam, sc = _scene(P, W, H, deg, seed=46, log_scale=np.log(0.05))
    m = sc["means3D"].copy()
    m[:, 2] = -np.abs(m[:, 2])
    keep = [0, 1023, 1024, P - 1]
    for j, i in enumerate(keep):
        m[i] = [(-0.6 + 0.4 * j) * 3.0 * cam["tanfovx"], 0.0, 3.0]
    sc["means3D"] = m
    sc["scales"][keep] = 0.08
    sc["opacities"][keep] = 0.5
    g_img = np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32)
    support, radii = _sparse_dense_oracle(R, ro, cam, sc, deg, "sr", g_img, "hand placed")
    assert torch.nonzero(radii > 0).flatten().tolist() == keep
    assert torch.nonzero(support).flatten().tolist() == keep


def test_rows_at_4_byte_alignment(R):
    """Every caller array of the chain rule one float into a larger buffer (16-byte accesses at dword alignment, rotations per
    word): against the same call with aligned arrays, to summation order."""
    P, W, H, deg = 1025, 48, 32, 3
    cam, sc = _scene(P, W, H, deg, seed=47, log_scale=np.log(0.05), opacity=0.3)
    t = _to_dev(sc)
    rs = _settings(R, cam, deg)
    g_img = torch.randn(3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(3))

    def off(shape, src=None):
        n = int(np.prod(shape))
        v = torch.zeros(n + 1, device="cuda")[1:].view(*shape)
        if src is not None:
            v.copy_(src)
        assert v.data_ptr() % 16 == 4
        return v
    res = []
    for shifted in (False, True):
        kw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
        out = None
        if shifted:
            kw = dict(shs=off((P, 16, 3), t["shs"]), scales=off((P, 3), t["scales"]), rotations=off((P, 4), t["rotations"]))
            out = dict(means3D=off((P, 3)), means2D=off((P, 3)), opacities=off((P, 1)), shs=off((P, 16, 3)), scales=off((P, 3)),
                       rotations=off((P, 4)))
        _, _, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **kw)
        res.append(R.rasterize_backward(rs, st, g_img, t["means3D"], out=out, **kw))
    torch.cuda.synchronize()
    assert int((res[0]["shs"].abs().sum(dim=(1, 2)) > 0).sum()) > 64
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        assert _same_to_summation_order(res[1][k].cpu().numpy(), res[0][k].cpu().numpy()), k


@pytest.mark.parametrize("mode", ["sr", "cov"])
def test_range_entry_from_a_row_that_is_no_multiple_of_64(R, ro, mode):
    """mvi_raster_backward_geom_range over [100, 100 + 777) of 1025 Gaussians (the dense kernel, with cov3D derived again at
    rows moved by `first`): the rows of the range against the oracle and the one-call backward, every other row untouched."""
    from multiview_inpaint_amd import _lib
    from multiview_inpaint_amd.raster import _Frame, _ptr
    L = _lib.lib()
    P, W, H, deg, first, n = 1025, 48, 32, 3, 100, 777
    cam, sc = _scene(P, W, H, deg, seed=48, log_scale=np.log(0.01), opacity=0.3)
    okw, gkw, t = _inputs(ro, cam, sc, mode)
    p = oracle_params(ro, cam, sc, BG)
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    g_img = np.random.default_rng(6).normal(size=(3, H, W)).astype(np.float32)
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    rs = _settings(R, cam, deg)
    gi = torch.tensor(g_img, device="cuda")
    _, _, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
    one = R.rasterize_backward(rs, st, gi, t["means3D"], **gkw)
    fr = _Frame(rs)
    rows = torch.empty(P, 16, device="cuda")
    SENT = 123.0
    shapes = dict(means3D=(P, 3), means2D=(P, 3), opacities=(P, 1), shs=(P, 16, 3), colors=(P, 3), scales=(P, 3), rotations=(P, 4),
                  cov3D_precomp=(P, 6))
    o = {k: torch.full(s, SENT, device="cuda") for k, s in shapes.items()}
    cov = mode == "cov"
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.mvi_raster_backward_render(C.byref(fr.c), P, st.D, _ptr(st.radii), _ptr(st.geom), _ptr(st.binning), _ptr(st.image),
                                            _ptr(gi), _ptr(rows), None, 1, 0, stream), "backward_render")
    _lib.check(L.mvi_raster_backward_geom_range(
        C.byref(fr.c), P, 16, first, n, _ptr(t["means3D"]), _ptr(t["shs"]), None, _ptr(gkw.get("scales")), _ptr(gkw.get("rotations")),
        _ptr(gkw.get("cov3D_precomp")), _ptr(st.radii), _ptr(st.geom), _ptr(rows), _ptr(o["means3D"]), _ptr(o["means2D"]),
        _ptr(o["opacities"]), _ptr(o["shs"]), _ptr(o["colors"]), None if cov else _ptr(o["scales"]), None if cov else _ptr(o["rotations"]),
        _ptr(o["cov3D_precomp"]) if cov else None, stream), "backward_geom_range")
    torch.cuda.synchronize()
    names = _names(mode)
    inside = np.zeros(P, bool)
    inside[first:first + n] = True
    worst = {}
    for k in names:
        got, want, whole = o[k].cpu().numpy(), np.asarray(ref[k], np.float64), one[k].cpu().numpy()
        assert (got[~inside] == SENT).all(), (k, "a row outside the range was written")
        assert _same_to_summation_order(got[inside], whole[inside]), k
        tol = RTOL * np.maximum(np.abs(want), GRAD_FLOOR * np.abs(want).max())
        worst[k] = float((np.abs(got.astype(np.float64) - want) / tol)[inside].max())
    print(f"range {mode}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst

"""GPU tests of the feature splat (raster.splat_features / GaussianRasterizer.splat / mask_lift.project_selection /
mask_lift.propagate_masks): out[c, p] = sum_i alpha_i(p) T_i(p) F[i, c] against the CPU oracle's colors_precomp forward on a zero
background (tests/feature_splat_helpers.py; pinned as the adjoint of the lift's reference in tests/test_feature_splat_cpu.py),
bit for bit against the project's own colour render, and its autograd against the lift. Bar: the colour bar of
tests/test_raster_gpu.py (feature_splat_helpers.check_image)."""
import math

import numpy as np
import pytest
import torch

from multiview_inpaint_amd import synthetic as syn
from feature_splat_helpers import check_image, iou, oracle_splat, signed_features
from mask_lift_helpers import (OBJ_N, long_list_scene, marginal_share, object_reference, oracle_forward, orbit_camera,
                               weight_images, MAX_MARGINAL)
from raster_aux_helpers import same_to_summation_order, viol
from raster_helpers import small_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


@pytest.fixture(scope="module")
def ro():
    from oracle import raster_oracle
    return raster_oracle


def _dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def _settings(R, cam, deg=0):
    d = "cuda"
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.zeros(3, device=d), scale_modifier=1.0,
        viewmatrix=torch.tensor(cam["viewmatrix"], device=d), projmatrix=torch.tensor(cam["projmatrix"], device=d),
        sh_degree=deg, campos=torch.tensor(cam["campos"], device=d), prefiltered=False)


def _forward(R, cam, sc, colours="sh", **kw):
    """A forward of the scene on the GPU with a zero background: (settings, state, input tensors, radii, colour image).
    colours: "sh" (deferred SH colours) | "precomp"."""
    rs = _settings(R, cam, sc["sh_degree"])
    t = {k: _dev(sc[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    if colours == "sh":
        t["shs"] = _dev(sc["shs"])
        ckw = dict(shs=t["shs"])
    else:
        t["colors_precomp"] = _dev(np.abs(np.random.default_rng(9).normal(0.5, 0.3, (sc["means3D"].shape[0], 3))))
        ckw = dict(colors_precomp=t["colors_precomp"])
    color, radii, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], scales=t["scales"], rotations=t["rotations"],
                                              **ckw, **kw)
    return rs, st, t, radii, color


def _n_contrib(st):
    return st.tensor("n_contrib", (st.H, st.W), torch.int32)


_refs = {}


def _reference(ro, key, scene, C):
    """The oracle's splat of the scene's 8 signed feature columns, computed once; the cases take its leading C planes (the
    channels are independent sums)."""
    if key not in _refs:
        cam, sc = scene()
        F = signed_features(sc["means3D"].shape[0], 8)
        _refs[key] = (cam, sc, F) + oracle_splat(ro, cam, sc, F)
    cam, sc, F, p0, f, img = _refs[key]
    return cam, sc, F[:, :C], p0, f, img[:C]


@pytest.mark.parametrize("channels", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("seed,pose,W,H", [(0, True, 40, 36), (12, False, 40, 36), (0, True, 17, 9)])
def test_small_scenes_against_the_oracle(R, ro, seed, pose, W, H, channels):
    """40 x 36: partial tiles on both edges. 17 x 9: the second tile is one pixel wide and two of a tile's four waves have no
    pixel at all. C = 1, 3, 4, 5, 8: both sides of the four-float boundary of a staged entry's features, and a full launch."""
    cam, sc, F, p0, f, ref = _reference(ro, (seed, pose, W, H), lambda: small_scene(seed, N=80, W=W, H=H, deg=1, pose=pose)[:2],
                                        channels)
    _, st, _, radii, _ = _forward(R, cam, sc)
    out = R.splat_features(st, _dev(F))
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy(), f["radii"])
    assert out.shape == (channels, H, W) and out.dtype == torch.float32 and out.is_contiguous()
    assert (f["n_contrib"] > 0).sum() > 40 and np.abs(ref).max() > 0.5
    check_image(f"C={channels}", out.cpu().numpy(), ref, ro, p0, f, max(1.0, float(np.abs(F).max())))


@pytest.mark.parametrize("channels", [2, 8])
def test_tile_lists_longer_than_a_staging_round(R, ro, channels):
    cam, sc, F, p0, f, ref = _reference(ro, "long_list", lambda: long_list_scene()[:2], channels)
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 256 and (f["n_contrib"] > 128).any(), (int(lens), int(f["n_contrib"].max()))   # several 256-entry rounds
    assert (f["final_T"] < 1e-3).any() and (f["n_contrib"] > 0)[f["final_T"] > 0.5].any(), "no mix of saturated and thin pixels"
    _, st, _, _, _ = _forward(R, cam, sc)
    out = R.splat_features(st, _dev(F))
    check_image(f"long lists C={channels}", out.cpu().numpy(), ref, ro, p0, f, max(1.0, float(np.abs(F).max())))


def test_empty_tiles_and_untouched_pixels_are_written_as_zeros(R, ro):
    """10 small Gaussians on 96 x 64: most tiles have an empty range and most pixels composite nothing; `out` arrives full of
    NaN and must come back fully written."""
    cam, sc, _ = small_scene(5, N=10, W=96, H=64, deg=1, pose=True, log_scale=math.log(0.02))
    F = signed_features(10, 3)
    p0, f, ref = oracle_splat(ro, cam, sc, F)
    empty = int((f["ranges"][:, 1] == f["ranges"][:, 0]).sum())
    assert f["ranges"].shape[0] == 24 and empty >= 5 and 0 < int((f["n_contrib"] > 0).sum()) < 0.2 * 96 * 64, empty
    _, st, _, _, _ = _forward(R, cam, sc)
    buf = torch.full((3, 64, 96), float("nan"), device="cuda")
    out = R.splat_features(st, _dev(F), out=buf)
    assert out.data_ptr() == buf.data_ptr() and bool(torch.isfinite(buf).all())
    nc = _n_contrib(st)
    assert int((nc == 0).sum()) > 0.8 * 96 * 64 and bool((buf[:, nc == 0] == 0).all())
    check_image("empty space", buf.cpu().numpy(), ref, ro, p0, f, max(1.0, float(np.abs(F).max())))


@pytest.mark.parametrize("scene", ["long_list", "17x9"])
def test_the_splat_of_a_forwards_colours_is_its_colour_image_bit_for_bit(R, scene):
    """One fma(F, alpha T, acc) per channel and composited entry in list order is what render_forward_kernel does: on a zero
    background the two images have the same bits, with precomputed colours and with SH colours (after resolve_colors)."""
    cam, sc = long_list_scene()[:2] if scene == "long_list" else small_scene(0, N=80, W=17, H=9, deg=1, pose=True)[:2]
    P = sc["means3D"].shape[0]
    _, st, t, _, color = _forward(R, cam, sc, colours="precomp")
    assert float(color.max()) > 0.2
    assert torch.equal(R.splat_features(st, t["colors_precomp"]), color)
    _, st, t, _, color = _forward(R, cam, sc, colours="sh")
    st.resolve_colors()
    rgb = st.tensor("rgbd", (P, 4), torch.float32)[:, :3]
    rgb = torch.where(torch.isfinite(rgb), rgb, torch.zeros_like(rgb))    # a culled Gaussian's record is never written or read
    assert float(color.max()) > 0.2
    assert torch.equal(R.splat_features(st, rgb), color)


def test_exact_equalities(R):
    cam, sc = long_list_scene()[:2]
    P, H, W = sc["means3D"].shape[0], cam["H"], cam["W"]
    _, st, _, _, _ = _forward(R, cam, sc)
    F = _dev(signed_features(P, 11))
    o8 = R.splat_features(st, F[:, :8].contiguous())
    assert float(o8.abs().max()) > 0.5
    # two calls give the same bits (no atomics)
    assert torch.equal(R.splat_features(st, F[:, :8].contiguous()), o8)
    # channels are independent: a column alone gives the plane it gives among eight
    for c in (0, 3, 4, 7):
        one = R.splat_features(st, F[:, c].contiguous())
        assert one.shape == (1, H, W) and torch.equal(one[0], o8[c]), c
    # [P] is [P, 1]
    assert torch.equal(R.splat_features(st, F[:, 2:3].contiguous()), R.splat_features(st, F[:, 2].contiguous()))
    # a strided view is read in place: the lift's rows (64-byte rows, base 4 bytes off) and a column range of F
    acc = R.lift_weights(st, _dev(weight_images(3, H, W)))
    view = acc[:, 1:4]
    assert view.stride() == (16, 1) and view.data_ptr() % 16 == 4
    assert torch.equal(R.splat_features(st, view), R.splat_features(st, view.contiguous()))
    assert torch.equal(R.splat_features(st, F[:, :8]), o8) and torch.equal(R.splat_features(st, F[:, 1:6]), o8[1:6])
    # a column-major tensor is made contiguous
    assert torch.equal(R.splat_features(st, F[:, :8].T.contiguous().T), o8)
    # more than eight channels: chunks of eight over the same state
    o11 = R.splat_features(st, F)
    assert o11.shape == (11, H, W) and torch.equal(o11[:8], o8) and torch.equal(o11[8:], R.splat_features(st, F[:, 8:].contiguous()))


@pytest.mark.parametrize("scene", ["small", "long_list"])
def test_a_channel_of_ones_is_the_alpha_image(R, scene):
    """sum alpha T = 1 - prod (1 - alpha): against 1 - final_T of the state and against `alpha` of an aux forward, on every
    pixel (two GPU evaluations of the same decisions: nothing is excused)."""
    cam, sc = long_list_scene()[:2] if scene == "long_list" else small_scene(0, N=80, W=40, H=36, deg=1, pose=True)[:2]
    P, H, W = sc["means3D"].shape[0], cam["H"], cam["W"]
    ones = torch.ones(P, device="cuda")
    _, st, _, _, _ = _forward(R, cam, sc)
    a = R.splat_features(st, ones)
    ft = st.tensor("final_T", (H, W), torch.float32)
    bad, worst = viol(a[0].cpu().numpy(), (1.0 - ft).cpu().numpy(), 1.0)
    print(f"ones vs 1 - final_T: worst ratio to the bar {worst:.3f}")
    assert not bad.any() and float(a.max()) > 0.9
    _, st2, _, _, _ = _forward(R, cam, sc, aux=True)
    a2 = R.splat_features(st2, ones)
    bad, worst = viol(a2.cpu().numpy(), st2.alpha.cpu().numpy(), 1.0)
    print(f"ones vs aux alpha: worst ratio to the bar {worst:.3f}")
    assert not bad.any() and torch.equal(a2, a)


def _one_tile():
    return small_scene(2, N=40, W=16, H=16, deg=1, pose=False)[:2]


def test_the_splat_leaves_the_forward_state_alone(R):
    """forward(prepare_backward=True) -> splat -> backward equals forward -> backward bit for bit, with equal support flags, and
    the splat gives the same image before and after that backward (the one-tile scene of the lift's test: the backward's float
    atomics have one order)."""
    cam, sc = _one_tile()
    F = _dev(signed_features(40, 5))
    gC = torch.randn(3, 16, 16, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    out, imgs, support = [], [], []
    for splat in (False, True):
        rs, st, t, radii, _ = _forward(R, cam, sc, prepare_backward=True)
        if splat:
            imgs.append(R.splat_features(st, F))
        out.append(R.rasterize_backward(rs, st, gC, t["means3D"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"]))
        if splat:
            imgs.append(R.splat_features(st, F))
        support.append(st.tensor("grad_support", (40,), torch.uint8))
    assert int((radii > 0).sum()) > 10 and float(out[0]["means3D"].abs().max()) > 0 and float(imgs[0].abs().max()) > 0
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(out[0][k], out[1][k]), k
    assert torch.equal(imgs[0], imgs[1])
    assert torch.equal(support[0], support[1]) and int(support[0].sum()) > 10
    # the aux forward's state serves as well, and the stateless form is the same computation
    rs, st, t, _, _ = _forward(R, cam, sc, aux=True)
    assert torch.equal(R.splat_features(st, F), imgs[0])
    a = R.GaussianRasterizer(rs).splat(F, t["means3D"], t["opacities"], scales=t["scales"], rotations=t["rotations"])
    assert torch.equal(a, imgs[0])


def test_autograd_the_backward_is_the_lift(R):
    cam, sc = _one_tile()
    rs, st, t, _, _ = _forward(R, cam, sc)
    gen = torch.Generator("cuda").manual_seed(6)
    # one tile: every row of the lift is added to once per slot, so the lift's float atomics have one order
    F = _dev(signed_features(40, 3)).requires_grad_()
    G = torch.randn(3, 16, 16, device="cuda", generator=gen)
    out = R.splat_features(st, F)
    assert out.requires_grad and torch.equal(out.detach(), R.splat_features(st, F.detach()))
    out.backward(G)
    want = R.lift_weights(st, G)[:, 1:]
    assert F.grad.shape == (40, 3) and float(want.abs().max()) > 0 and torch.equal(F.grad, want)
    # [P] features get a [P] gradient
    f1 = _dev(signed_features(40, 1)[:, 0]).requires_grad_()
    R.splat_features(st, f1).backward(G[:1])
    assert f1.grad.shape == (40,) and torch.equal(f1.grad, R.lift_weights(st, G[:1])[:, 1])
    # 11 channels: the backward chunks 8 + 3
    F11 = _dev(signed_features(40, 11)).requires_grad_()
    G11 = torch.randn(11, 16, 16, device="cuda", generator=gen)
    R.splat_features(st, F11).backward(G11)
    assert F11.grad.shape == (40, 11)
    assert torch.equal(F11.grad[:, :8], R.lift_weights(st, G11[:8])[:, 1:]) and torch.equal(F11.grad[:, 8:], R.lift_weights(st, G11[8:])[:, 1:])
    # out= cannot take part in a differentiable call; without grad mode it can
    with pytest.raises(ValueError, match="out="):
        R.splat_features(st, F, out=torch.empty(3, 16, 16, device="cuda"))
    with torch.no_grad():
        buf = torch.empty(3, 16, 16, device="cuda")
        assert R.splat_features(st, F, out=buf) is buf and not buf.requires_grad
    # the stateless form is differentiable in the features only
    m3 = t["means3D"].clone().requires_grad_()
    F2 = _dev(signed_features(40, 3)).requires_grad_()
    img = R.GaussianRasterizer(rs).splat(F2, m3, t["opacities"], scales=t["scales"], rotations=t["rotations"])
    img.backward(G)
    assert m3.grad is None and torch.equal(F2.grad, want)


def test_autograd_on_long_lists(R):
    cam, sc = long_list_scene()[:2]
    P, H, W = sc["means3D"].shape[0], cam["H"], cam["W"]
    _, st, _, _, _ = _forward(R, cam, sc)
    F = _dev(signed_features(P, 8)).requires_grad_()
    G = _dev(weight_images(8, H, W))
    R.splat_features(st, F).backward(G)
    want = R.lift_weights(st, G)[:, 1:]
    assert float(want.abs().max()) > 1.0
    assert same_to_summation_order(F.grad.cpu().numpy(), want.cpu().numpy())


def test_degenerate_inputs_and_errors(R):
    cam = syn.make_camera(48, 32, 60.0)
    rast = R.GaussianRasterizer(_settings(R, cam))
    z = lambda *s: torch.zeros(*s, device="cuda")
    # P = 0
    a = rast.splat(z(0, 3), z(0, 3), z(0, 1), scales=z(0, 3), rotations=z(0, 4))
    assert a.shape == (3, 32, 48) and bool((a == 0).all())
    # every Gaussian behind the camera: num_rendered = 0
    N = 16
    means = z(N, 3)
    means[:, 2] = torch.linspace(-3, 0.2, N)
    kw = dict(scales=torch.full((N, 3), 0.1, device="cuda"), rotations=torch.tensor([[1.0, 0, 0, 0]], device="cuda").repeat(N, 1))
    op = torch.full((N, 1), 0.9, device="cuda")
    a = rast.splat(torch.rand(N, 11, device="cuda"), means, op, **kw)
    assert a.shape == (11, 32, 48) and bool((a == 0).all())
    _, _, _, st0 = R.rasterize_forward(rast.raster_settings, means, op, colors_precomp=z(N, 3), **kw)
    assert st0.D == 0
    buf = torch.full((2, 32, 48), float("nan"), device="cuda")
    assert R.splat_features(st0, torch.rand(N, 2, device="cuda"), out=buf) is buf and bool((buf == 0).all())
    # Python-side argument errors
    means[:, 2] += 4.0
    _, _, _, st = R.rasterize_forward(rast.raster_settings, means, op, colors_precomp=z(N, 3), **kw)
    assert st.D > 0
    with pytest.raises(ValueError, match="features must be"):
        R.splat_features(st, z(N + 1, 3))
    with pytest.raises(ValueError, match="features must be"):
        R.splat_features(st, z(N, 3, 1))
    with pytest.raises(ValueError, match="features must be"):
        R.splat_features(st, z(N, 0))
    with pytest.raises(TypeError, match="float32"):
        R.splat_features(st, z(N, 3).double())
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.splat_features(st, torch.zeros(N, 3))
    for bad in (z(3, 48, 32), z(2, 32, 48), z(3, 32, 48).double(), torch.zeros(3, 32, 48), z(3, 32, 96)[:, :, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            R.splat_features(st, z(N, 3), out=bad)
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        rast.splat(z(N, 3), means, op)
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        rast.splat(z(N, 3), means, op, cov3D_precomp=z(N, 6), **kw)


@pytest.fixture(scope="module")
def objects(ro):
    """The object scene of the lift's end-to-end case, its oracle selection, and per destination view (two orbit cameras that
    are no source view; yaw 1.0 lies outside the sources' range) the oracle's soft mask of that selection and the mask of the
    object rendered alone."""
    ref = object_reference(ro)
    sc, acc = ref["sc"], ref["acc"]
    sel = (acc[:, 0] > 0) & (acc[:, 1] > 0.5 * acc[:, 0])
    alone = {k: (v[:OBJ_N] if k != "sh_degree" else v) for k, v in sc.items()}
    dst = []
    for yaw in (0.45, 1.0):
        cam = orbit_camera(yaw)
        p0, f, soft = oracle_splat(ro, cam, sc, sel.astype(np.float32))
        _, fa = oracle_forward(ro, cam, alone)
        dst.append(dict(cam=cam, p0=p0, f=f, soft=soft, alone=(1.0 - fa["final_T"]) > 0.5))
    ref.update(sel=sel, dst=dst)
    return ref


def test_masks_in_some_views_to_masks_in_any_view_end_to_end(R, ro, objects):
    from multiview_inpaint_amd import mask_lift
    sc, is_obj, sel_ref, acc_ref = objects["sc"], objects["is_obj"], objects["sel"], objects["acc"]
    t = {k: _dev(sc[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    geo = dict(scales=t["scales"], rotations=t["rotations"])
    # conditions on the inputs, on the oracle alone
    assert int(sel_ref[is_obj].sum()) == 296 and int(sel_ref[~is_obj].sum()) == 0
    for d in objects["dst"]:
        band = np.abs(d["soft"][0] - 0.5) <= 1e-3
        d["band"] = band
        assert int(band.sum()) <= 3
        assert d["alone"].sum() > 100 and iou(d["soft"][0] > 0.5, d["alone"]) >= 0.9, iou(d["soft"][0] > 0.5, d["alone"])
    dst_rs = [_settings(R, d["cam"]) for d in objects["dst"]]
    # the GPU's projection of the oracle's selection against the oracle's soft mask
    masks = mask_lift.project_selection(torch.tensor(sel_ref, device="cuda"), dst_rs, t["means3D"], t["opacities"], **geo)
    assert len(masks) == 2
    for d, m in zip(objects["dst"], masks):
        assert m.shape == (1, d["cam"]["H"], d["cam"]["W"]) and m.dtype == torch.float32
        check_image("soft mask", m.cpu().numpy(), d["soft"], ro, d["p0"], d["f"], 1.0)
        compared = ~d["band"] & ((ro.margins(d["p0"], d["f"]) & 1) == 0)
        assert np.array_equal((m[0] > 0.5).cpu().numpy()[compared], (d["soft"][0] > 0.5)[compared])
    # float weights and a [P, K] selection: column k is the [P] call on column k
    two = torch.stack([torch.tensor(sel_ref, device="cuda").float(), 0.25 * torch.ones(len(sel_ref), device="cuda")], 1)
    m2 = mask_lift.project_selection(two, dst_rs[:1], t["means3D"], t["opacities"], **geo)[0]
    assert m2.shape == (2, 80, 96) and torch.equal(m2[:1], masks[0])
    # the whole way in one call
    src = [(_settings(R, cam), _dev(m)) for cam, m in zip(objects["cams"], objects["masks"])]
    res = mask_lift.propagate_masks(src, dst_rs, t["means3D"], t["opacities"], **geo)
    assert isinstance(res, tuple) and len(res) == 2
    selection, pm = res
    assert selection.dtype == torch.bool and selection.shape == (len(sel_ref),) and len(pm) == 2
    again = mask_lift.project_selection(selection, dst_rs, t["means3D"], t["opacities"], **geo)
    assert all(torch.equal(a, b) for a, b in zip(pm, again))
    sel2 = mask_lift.select(mask_lift.lift_views(src, t["means3D"], t["opacities"], **geo))
    ratio = acc_ref[:, 1] / np.maximum(acc_ref[:, 0], 1e-30)
    decided = (np.abs(ratio - 0.5) > 1e-3) & (acc_ref[:, 0] > 1e-4)        # the rows the lift's end-to-end test compares
    assert np.array_equal(selection.cpu().numpy()[decided], sel2.cpu().numpy()[decided])
    assert np.array_equal(selection.cpu().numpy()[decided], sel_ref[decided])
    for d, m in zip(objects["dst"], pm):
        assert iou((m[0] > 0.5).cpu().numpy(), d["alone"]) >= 0.9
    # normalize: the share of the pixel's composited weight that the selection owns
    norm = mask_lift.project_selection(selection, dst_rs, t["means3D"], t["opacities"], normalize=True, **geo)
    for d, rs, soft, n in zip(objects["dst"], dst_rs, pm, norm):
        assert n.shape == soft.shape and float(n.min()) >= 0.0 and float(n.max()) <= 1.0 and float(n.max()) > 0.9
        alpha = R.GaussianRasterizer(rs).splat(torch.ones(len(sel_ref), device="cuda"), t["means3D"], t["opacities"], **geo)[0]
        pos = alpha > 0
        assert int(pos.sum()) > 1000 and torch.equal(n[0][pos], soft[0][pos] / alpha[pos])
        _, st, _, _, _ = _forward(R, d["cam"], sc)
        nc = _n_contrib(st)
        assert bool((n[0][nc == 0] == 0).all()) and bool((n[0][~pos] == 0).all())

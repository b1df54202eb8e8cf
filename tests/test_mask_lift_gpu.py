"""GPU tests of mask lifting (raster.lift_weights / GaussianRasterizer.lift / mask_lift): per-Gaussian blend weights
total_i = sum alpha T and hit_i,c = sum alpha T w_c against the CPU oracle's colour gradient with colors_precomp
(tests/mask_lift_helpers.py; pinned against autograd in tests/test_mask_lift_cpu.py). Bars: those the colour gradient is held
to (raster_aux_helpers.grad_check, the flip allowance, the marginal-pixel share)."""
import os

import numpy as np
import pytest
import torch

from multiview_inpaint_amd import synthetic as syn
from mask_lift_helpers import (check_acc, long_list_scene, marginal_share, object_reference, oracle_forward, oracle_lift,
                               weight_images, MAX_MARGINAL)
from raster_aux_helpers import flip_allowance, grad_check, same_to_summation_order
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
    """A forward of the scene on the GPU: (settings, state, input tensors). colours: "sh" (deferred SH colours) | "precomp"."""
    rs = _settings(R, cam, sc["sh_degree"])
    t = {k: _dev(sc[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    if colours == "sh":
        t["shs"] = _dev(sc["shs"])
        ckw = dict(shs=t["shs"])
    else:
        t["colors_precomp"] = _dev(np.abs(np.random.default_rng(9).normal(0.5, 0.3, (sc["means3D"].shape[0], 3))))
        ckw = dict(colors_precomp=t["colors_precomp"])
    _, radii, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], scales=t["scales"], rotations=t["rotations"], **ckw, **kw)
    return rs, st, t, radii


_scenes = {}


def _small(ro, seed, pose, W, H):
    """The scene and its oracle forward, computed once for the cases that share it."""
    key = (seed, pose, W, H)
    if key not in _scenes:
        cam, sc, _ = small_scene(seed, N=80, W=W, H=H, deg=1, pose=pose)
        _scenes[key] = (cam, sc, oracle_forward(ro, cam, sc))
    return _scenes[key]


@pytest.mark.parametrize("channels", [0, 1, 3, 8])
@pytest.mark.parametrize("seed,pose,W,H", [(0, True, 40, 36), (12, False, 40, 36), (0, True, 17, 9)])
def test_small_scenes_against_the_oracle(R, ro, seed, pose, W, H, channels):
    """40 x 36: partial tiles on both edges. 17 x 9: the second tile is one pixel wide and the tile's second wave has one row.
    C = 0 (totals only), a binary mask, three signed float channels, and eight channels (the nine-value wave sum is full)."""
    cam, sc, fwd = _small(ro, seed, pose, W, H)
    w = weight_images(channels, H, W)
    p0, f, ref = oracle_lift(ro, cam, sc, w, fwd=fwd)
    _, st, _, radii = _forward(R, cam, sc)
    acc = R.lift_weights(st, None if w is None else _dev(w))
    torch.cuda.synchronize()
    assert np.array_equal(radii.cpu().numpy(), f["radii"])
    assert acc.shape == (80, 1 + channels) and acc.dtype == torch.float32 and ref.shape == acc.shape
    assert (ref[:, 0] > 0).sum() > 40
    check_acc(f"acc C={channels}", acc.cpu().numpy(), ref, ro, p0, f)
    if channels == 1:                                                      # [H, W] is C = 1
        a2 = R.lift_weights(st, _dev(w[0]))
        assert a2.shape == (80, 2) and same_to_summation_order(a2.cpu().numpy(), acc.cpu().numpy())


@pytest.fixture(scope="module")
def long_list(ro):
    cam, sc, _ = long_list_scene()
    w = weight_images(2, cam["H"], cam["W"])
    return (cam, sc, w) + oracle_lift(ro, cam, sc, w)


def test_tile_lists_longer_than_a_staging_batch(R, ro, long_list):
    cam, sc, w, p0, f, ref = long_list
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 256 and (f["n_contrib"] > 128).any(), (int(lens), int(f["n_contrib"].max()))   # several 128-entry rounds
    assert (f["final_T"] < 1e-3).any() and (f["n_contrib"] > 0)[f["final_T"] > 0.5].any(), "no mix of saturated and thin pixels"
    _, st, _, _ = _forward(R, cam, sc)
    acc = R.lift_weights(st, _dev(w))
    check_acc("acc long lists", acc.cpu().numpy(), ref, ro, p0, f)


def test_equals_the_colour_gradient_of_the_projects_own_backward(R, long_list):
    """The route a user had before: colors_precomp forward, full backward with the weight image as grad_color, read
    dL/dcolors_precomp."""
    cam, sc = long_list[:2]
    w = _dev(weight_images(3, cam["H"], cam["W"]))
    rs, st, t, _ = _forward(R, cam, sc, colours="precomp", prepare_backward=True)
    acc = R.lift_weights(st, w)
    g = R.rasterize_backward(rs, st, w, t["means3D"], colors_precomp=t["colors_precomp"], scales=t["scales"], rotations=t["rotations"])
    n_pairs = int(st.tensor("n_contrib", (cam["H"], cam["W"]), torch.int32).sum())
    assert n_pairs > 100_000
    grad_check("hits vs dL/dcolors_precomp", acc[:, 1:4].cpu().numpy(), g["colors_precomp"].cpu().numpy(), flip_allowance(n_pairs))


@pytest.fixture(scope="module")
def objects(ro):
    return object_reference(ro)


def _object_inputs(ref):
    sc = ref["sc"]
    return {k: _dev(sc[k]) for k in ("means3D", "opacities", "scales", "rotations")}


def test_accumulation_and_row_layout(R, objects):
    sc, cams, masks = objects["sc"], objects["cams"], objects["masks"]
    P = sc["means3D"].shape[0]
    (_, st0, _, radii0), (_, st1, _, _) = (_forward(R, cams[v], sc) for v in (0, 3))
    w0, w1 = _dev(masks[0]), _dev(masks[3])
    r0, r1 = R.lift_weights(st0, w0), R.lift_weights(st1, w1)
    assert r0.shape == (P, 2) and r0.stride() == (16, 1)                   # a view of 64-byte rows
    assert not same_to_summation_order(r0.cpu().numpy(), r1.cpu().numpy(), 1e-2), "the two views should differ"
    # two views into one acc = the sum of the two results
    acc = R.lift_weights(st0, w0)
    both = R.lift_weights(st1, w1, acc=acc)
    assert both.data_ptr() == acc.data_ptr() and both.shape == acc.shape
    assert same_to_summation_order(both.cpu().numpy(), (r0 + r1).cpu().numpy())
    # acc is added into, never zeroed; culled Gaussians and the slots behind 1 + C keep their bits
    wide = torch.ones(P, 16, device="cuda")
    out = R.lift_weights(st0, w0, acc=wide[:, :2])
    assert same_to_summation_order(out.cpu().numpy(), (1.0 + r0).cpu().numpy())
    culled = radii0 == 0
    assert 100 < int(culled.sum()) < P - 100
    assert torch.equal(out[culled], torch.ones_like(out[culled])) and bool((out[~culled][:, 0] > 1.0).any())
    assert torch.equal(wide[:, 2:], torch.ones(P, 14, device="cuda"))
    # a tight [P, 1 + C] acc works too
    tight = R.lift_weights(st0, w0, acc=torch.zeros(P, 2, device="cuda"))
    assert tight.is_contiguous() and same_to_summation_order(tight.cpu().numpy(), r0.cpu().numpy())
    # a zero weight image: hits exactly 0, totals as before
    z = R.lift_weights(st0, torch.zeros_like(w0))
    assert bool((z[:, 1] == 0).all()) and int((z[:, 0] > 0).sum()) > 300
    assert same_to_summation_order(z[:, 0].cpu().numpy(), r0[:, 0].cpu().numpy())
    with pytest.raises(ValueError, match="acc must be"):
        R.lift_weights(st0, w0, acc=torch.zeros(P, 3, device="cuda"))
    with pytest.raises(ValueError, match="acc must be"):
        R.lift_weights(st0, w0, acc=torch.zeros(2, P, device="cuda").T)


def test_the_lift_leaves_the_forward_state_alone(R):
    """forward(prepare_backward=True) -> lift -> backward equals forward -> backward bit for bit, and the lift gives the same acc
    before and after that backward. One 16 x 16 tile, so that every row is added to once per slot and two runs of the float
    atomics cannot differ in their order."""
    cam, sc, _ = small_scene(2, N=40, W=16, H=16, deg=1, pose=False)
    w = _dev(weight_images(3, 16, 16))
    gC = torch.randn(3, 16, 16, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    out, accs, support = [], [], []
    for lift in (False, True):
        rs, st, t, radii = _forward(R, cam, sc, prepare_backward=True)
        if lift:
            accs.append(R.lift_weights(st, w))
        out.append(R.rasterize_backward(rs, st, gC, t["means3D"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"]))
        if lift:
            accs.append(R.lift_weights(st, w))
        support.append(st.tensor("grad_support", (40,), torch.uint8))
    assert int((radii > 0).sum()) > 10 and float(out[0]["means3D"].abs().max()) > 0 and float(accs[0][:, 0].max()) > 0
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(out[0][k], out[1][k]), k
    assert torch.equal(accs[0], accs[1])
    assert torch.equal(support[0], support[1]) and int(support[0].sum()) > 10
    # the aux forward's state serves as well, and the stateless form is the same computation
    rs, st, t, _ = _forward(R, cam, sc, aux=True)
    assert torch.equal(R.lift_weights(st, w), accs[0])
    a = R.GaussianRasterizer(rs).lift(w, t["means3D"], t["opacities"], scales=t["scales"], rotations=t["rotations"])
    assert torch.equal(a, accs[0])


def test_degenerate_inputs(R, ro):
    cam = syn.make_camera(48, 32, 60.0)
    rast = R.GaussianRasterizer(_settings(R, cam))
    z = lambda *s: torch.zeros(*s, device="cuda")
    w = torch.rand(2, 32, 48, device="cuda")
    # P = 0
    a = rast.lift(w, z(0, 3), z(0, 1), scales=z(0, 3), rotations=z(0, 4))
    assert a.shape == (0, 3)
    # every Gaussian behind the camera: num_rendered = 0
    N = 16
    means = z(N, 3)
    means[:, 2] = torch.linspace(-3, 0.2, N)
    kw = dict(scales=torch.full((N, 3), 0.1, device="cuda"), rotations=torch.tensor([[1.0, 0, 0, 0]], device="cuda").repeat(N, 1))
    op = torch.full((N, 1), 0.9, device="cuda")
    a = rast.lift(w, means, op, **kw)
    assert a.shape == (N, 3) and bool((a == 0).all())
    assert bool((rast.lift(None, means, op, **kw) == 0).all())
    # Python-side argument errors
    means[:, 2] += 4.0
    _, _, _, st = R.rasterize_forward(rast.raster_settings, means, op, colors_precomp=z(N, 3), **kw)
    assert st.D > 0
    with pytest.raises(ValueError, match="weights must be"):
        R.lift_weights(st, z(2, 48, 32))
    with pytest.raises(ValueError, match="weights must be"):
        R.lift_weights(st, z(1, 2, 32, 48))
    with pytest.raises(ValueError, match="at most 8"):
        R.lift_weights(st, z(9, 32, 48))
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.lift_weights(st, torch.zeros(2, 32, 48))
    with pytest.raises(TypeError, match="float32"):
        R.lift_weights(st, z(2, 32, 48).bool())
    # GaussianRasterizer.lift is rasterize_forward + lift_weights
    cam, sc, fwd = _small(ro, 0, True, 40, 36)
    _, st, t, _ = _forward(R, cam, sc)
    w = _dev(weight_images(3, 36, 40))
    a = R.GaussianRasterizer(_settings(R, cam, 1)).lift(w, t["means3D"], t["opacities"], scales=t["scales"], rotations=t["rotations"])
    assert same_to_summation_order(a.cpu().numpy(), R.lift_weights(st, w).cpu().numpy())
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        rast.lift(None, means, op)


def test_object_and_background_four_views_end_to_end(R, ro, objects, tmp_path):
    """300 object Gaussians in front of 1500 on a wall and a floor, four views, each view's mask = alpha > 0.5 of the object
    rendered alone. The oracle selects 296 of the 300 object Gaussians (3 are never seen, 1 is below the ratio) and no background
    Gaussian; its object ratios have their 1 % quantile at 0.52, the background's largest ratio is 0.32."""
    from multiview_inpaint_amd import gaussian_io, mask_lift
    sc, is_obj, ref = objects["sc"], objects["is_obj"], objects["acc"]
    P = sc["means3D"].shape[0]
    t = _object_inputs(objects)
    views = [(_settings(R, cam), _dev(m)) for cam, m in zip(objects["cams"], objects["masks"])]
    acc = mask_lift.lift_views(views, t["means3D"], t["opacities"], scales=t["scales"], rotations=t["rotations"])
    assert acc.shape == (P, 2)
    pairs = 0
    for p0, f in objects["fwds"]:
        assert marginal_share(ro, p0, f) < MAX_MARGINAL
        pairs += int(f["n_contrib"].sum())
    grad_check("acc over four views", acc.cpu().numpy(), ref, flip_allowance(pairs))
    # the oracle's own selection
    sel_ref = (ref[:, 0] > 0) & (ref[:, 1] > 0.5 * ref[:, 0])
    assert int(sel_ref[is_obj].sum()) == 296 and int(sel_ref[~is_obj].sum()) == 0
    sel = mask_lift.select(acc, ratio=0.5, min_total=0.0)
    sel_np = sel.cpu().numpy()
    ratio = ref[:, 1] / np.maximum(ref[:, 0], 1e-30)
    decided = (np.abs(ratio - 0.5) > 1e-3) & (ref[:, 0] > 1e-4)            # a condition on the rows compared, not a tolerance
    assert int(((np.abs(ratio - 0.5) <= 1e-3) & (ref[:, 0] > 1e-4)).sum()) <= 5      # the band holds a handful of rows at most
    assert np.array_equal(sel_np[decided], sel_ref[decided])
    assert int(sel_np[~is_obj].sum()) == 0 and int(sel_np[is_obj].sum()) >= 285
    # the same through a PLY: the stored parameters are the raw ones
    raw = dict(xyz=t["means3D"], f_dc=torch.zeros(P, 1, 3, device="cuda"), f_rest=torch.zeros(P, 0, 3, device="cuda"),
               opacity=torch.logit(t["opacities"]), scaling=torch.log(t["scales"]), rotation=t["rotations"] * 1.5)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    gaussian_io.save_ply(src, raw["xyz"], raw["f_dc"], raw["f_rest"], raw["opacity"], raw["scaling"], raw["rotation"])
    kept, total = mask_lift.delete_by_masks(src, dst, views, ratio=0.5, min_total=0.0)
    assert total == P and kept == P - int(sel_np.sum())
    back = gaussian_io.load_ply(dst, 0)
    assert np.array_equal(back["xyz"], sc["means3D"][~sel_np])
    assert np.array_equal(back["opacity"], raw["opacity"].cpu().numpy()[~sel_np])


def test_mid_size_100k_800(R, ro):
    """The 100k Gaussians / 800 x 800 scene of test_raster_aux_gpu.test_mid_size_100k_800, C = 2."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cam = syn.make_camera(800, 800, 50.0)
    sc = syn.make_scene(100_000, cam, 3, seed=0)
    w = weight_images(2, 800, 800)
    ro.set_threads(max(1, min(16, avail)))
    try:
        p0, f, ref = oracle_lift(ro, cam, sc, w)
        share = marginal_share(ro, p0, f)
    finally:
        ro.set_threads(1)
    assert share < MAX_MARGINAL
    _, st, _, _ = _forward(R, cam, sc)
    acc = R.lift_weights(st, _dev(w))
    grad_check("acc 100k", acc.cpu().numpy(), ref, flip_allowance(int(f["n_contrib"].sum())))

"""GPU tests of the rasterizer's differentiable aux outputs: expected_depth = sum z alpha T and alpha = 1 - T_final, forward
and backward, against the CPU oracle rendering the colours (z, 1, 0) on a zero background (tests/raster_aux_helpers.py; the
composition itself is pinned against autograd in tests/test_raster_aux_cpu.py). Bars: those of tests/test_raster_gpu.py."""
import os

import numpy as np
import pytest
import torch

from multiview_inpaint_amd import synthetic as syn
from raster_aux_helpers import (GEOMETRY_KEYS, add_grads, aux_backward, aux_forward, flip_allowance, grad_check,
                                same_to_summation_order, viol)
from raster_helpers import oracle_params, small_scene

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


def _settings(R, cam, bg, deg):
    d = "cuda"
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor(bg, device=d), scale_modifier=1.0,
        viewmatrix=torch.tensor(cam["viewmatrix"], device=d), projmatrix=torch.tensor(cam["projmatrix"], device=d),
        sh_degree=deg, campos=torch.tensor(cam["campos"], device=d), prefiltered=False)


def _dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def _inputs(ro, cam, sc, bg, mode):
    """(oracle kwargs, GPU kwargs) of the two input forms: SH + scales / rotations, or colors_precomp + cov3D_precomp."""
    if mode == "precomp":
        p = oracle_params(ro, cam, sc, bg)
        f0 = ro.forward(p, sc["means3D"], sc["opacities"], shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"], render=False)
        c6 = f0["cov3D"].copy()
        cp = np.abs(np.random.default_rng(9).normal(0.5, 0.3, (p.P, 3))).astype(np.float32)
        return dict(colors_precomp=cp, cov3D_precomp=c6), dict(colors_precomp=_dev(cp), cov3D_precomp=_dev(c6))
    return (dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"]),
            dict(shs=_dev(sc["shs"]), scales=_dev(sc["scales"]), rotations=_dev(sc["rotations"])))


def _cov_kw(okw):
    return {k: v for k, v in okw.items() if k in ("scales", "rotations", "cov3D_precomp")}


def _forward_and_check(R, ro, cam, sc, bg, mode="sh", max_marginal=5e-3):
    """One aux forward against the oracle. Returns everything the backward tests need."""
    deg = sc["sh_degree"]
    okw, gkw = _inputs(ro, cam, sc, bg, mode)
    rs = _settings(R, cam, bg, deg)
    m3, op = _dev(sc["means3D"]), _dev(sc["opacities"])
    color, radii, depth, st = R.rasterize_forward(rs, m3, op, prepare_backward=True, aux=True, **gkw)
    c0, r0, d0, st0 = R.rasterize_forward(rs, m3, op, **gkw)
    torch.cuda.synchronize()
    H, W, P = cam["H"], cam["W"], st.P
    # colour, radii and the median depth are those of the plain forward, bit for bit; the plain state carries no aux outputs
    assert torch.equal(color, c0) and torch.equal(radii, r0) and torch.equal(depth, d0)
    assert st0.expected_depth is None and st0.alpha is None
    assert st.expected_depth.shape == (1, H, W) and st.alpha.shape == (1, H, W)
    ft = st.tensor("final_T", (H, W), torch.float32)
    assert torch.equal(st.alpha[0], 1.0 - ft), "alpha is not 1 - final_T bit for bit"
    z = st.tensor("depths", (P,), torch.float32).cpu().numpy()
    p0, f = aux_forward(ro, cam, sc, z, _cov_kw(okw))
    assert np.array_equal(radii.cpu().numpy(), f["radii"])
    assert np.array_equal(z[f["radii"] > 0], f["depths"][f["radii"] > 0])
    mm = ro.margins(p0, f)
    marginal = (mm & 1) != 0
    assert marginal.mean() < max_marginal, "margin too wide: the test would excuse too many pixels"
    allow = flip_allowance(int(f["n_contrib"].sum()))
    ed, al = st.expected_depth[0].cpu().numpy(), st.alpha[0].cpu().numpy()
    bad_d, worst_d = viol(ed, f["color"][0], 1.0)
    bad_a, worst_a = viol(al, f["color"][1], 1.0)
    print(f"expected depth: worst ratio to the 1e-4 bar {worst_d:.3f}; alpha: {worst_a:.3f}; marginal pixels {int(marginal.sum())}, "
          f"differing {int((bad_d | bad_a).sum())} (allowed {allow})")
    assert not (bad_d & ~marginal).any(), ("expected depth off on a pixel with no marginal decision", worst_d)
    assert not (bad_a & ~marginal).any(), ("alpha off on a pixel with no marginal decision", worst_a)
    assert int((bad_d | bad_a).sum()) <= allow
    assert (ed[f["n_contrib"] == 0] == 0).all() and (al[f["n_contrib"] == 0] == 0).all()
    return dict(rs=rs, st=st, m3=m3, op=op, okw=okw, gkw=gkw, p0=p0, f_aux=f, z=z, allow=allow, mode=mode)


def _reference(ro, cam, sc, bg, ctx, g_color, gD, gA):
    """Oracle colour backward (if g_color is given) + composed aux backward."""
    cov = _cov_kw(ctx["okw"])
    ref = aux_backward(ro, cam, sc, ctx["p0"], ctx["f_aux"], ctx["z"], gD, gA, cov)
    P = ctx["st"].P
    colour_key = "shs" if "shs" in ctx["okw"] else "colors_precomp"
    ref[colour_key] = np.zeros((P,) + ctx["okw"][colour_key].shape[1:], np.float64)
    if g_color is not None:
        p = oracle_params(ro, cam, sc, bg)
        fc = ro.forward(p, sc["means3D"], sc["opacities"], **ctx["okw"])
        bc = ro.backward(p, fc, g_color, sc["means3D"], **ctx["okw"])
        ref = add_grads(ref, bc, GEOMETRY_KEYS + (colour_key,))
    return ref


def _check_grads(g, ref, allow, pure_min=None):
    for k in GEOMETRY_KEYS + ("shs", "colors_precomp"):
        if ref.get(k) is None:
            assert g.get(k) is None, k
            continue
        grad_check(k, g[k].cpu().numpy(), ref[k], allow, pure_min=pure_min)


@pytest.mark.parametrize("seed,deg,pose", [(0, 3, True), (1, 3, True), (11, 1, True), (12, 2, False)])
def test_forward_small(R, ro, seed, deg, pose):
    """40 x 36 is not a multiple of the tile: partial tiles on both edges."""
    cam, sc, bg = small_scene(seed, deg=deg, pose=pose)
    _forward_and_check(R, ro, cam, sc, bg)


def _long_list_scene():
    cam, sc, bg = small_scene(3, N=3000, W=48, H=40, deg=1, pose=True, log_scale=np.log(0.04))
    rng = np.random.default_rng(3)
    # a mix of opacities: nearly transparent Gaussians left of the image centre, nearly opaque ones right of it
    V = np.asarray(cam["viewmatrix"], np.float32).reshape(4, 4)
    vx = sc["means3D"] @ V[0:3, 0] + V[3, 0]
    lo, hi = rng.uniform(0.004, 0.03, 3000), rng.uniform(0.6, 0.99, 3000)
    sc["opacities"] = np.where(vx < 0, lo, hi).astype(np.float32).reshape(sc["opacities"].shape)
    return cam, sc, bg


def test_forward_with_tile_lists_longer_than_a_staging_batch(R, ro):
    cam, sc, bg = _long_list_scene()
    ctx = _forward_and_check(R, ro, cam, sc, bg)
    f = ctx["f_aux"]
    lens = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).max()
    assert lens > 256, int(lens)                                           # more than one 256-entry round of the forward
    assert (f["final_T"] < 1e-3).any() and (f["n_contrib"] > 0)[f["final_T"] > 0.5].any(), "no mix of saturated and thin pixels"
    assert (f["n_contrib"] > 128).any()                                    # and more than one 128-entry round of the backward


@pytest.mark.parametrize("mode", ["sh", "precomp"])
@pytest.mark.parametrize("case", ["depth", "alpha", "joint"])
def test_backward_small(R, ro, case, mode):
    cam, sc, bg = small_scene(0, deg=3)
    ctx = _forward_and_check(R, ro, cam, sc, bg, mode)
    rng = np.random.default_rng(5)
    H, W = cam["H"], cam["W"]
    gD = rng.normal(size=(1, H, W)).astype(np.float32) if case in ("depth", "joint") else None
    gA = rng.normal(size=(1, H, W)).astype(np.float32) if case in ("alpha", "joint") else None
    gC = rng.normal(size=(3, H, W)).astype(np.float32) if case == "joint" else None
    g = R.rasterize_backward(ctx["rs"], ctx["st"], _dev(gC) if gC is not None else torch.zeros(3, H, W, device="cuda"), ctx["m3"],
                             grad_expected_depth=None if gD is None else _dev(gD), grad_alpha=None if gA is None else _dev(gA),
                             **ctx["gkw"])
    torch.cuda.synchronize()
    _check_grads(g, _reference(ro, cam, sc, bg, ctx, gC, gD, gA), ctx["allow"])


def test_backward_with_tile_lists_longer_than_a_staging_batch(R, ro):
    cam, sc, bg = _long_list_scene()
    ctx = _forward_and_check(R, ro, cam, sc, bg)
    rng = np.random.default_rng(6)
    H, W = cam["H"], cam["W"]
    gD, gA, gC = (rng.normal(size=(c, H, W)).astype(np.float32) for c in (1, 1, 3))
    g = R.rasterize_backward(ctx["rs"], ctx["st"], _dev(gC), ctx["m3"], grad_expected_depth=_dev(gD), grad_alpha=_dev(gA), **ctx["gkw"])
    torch.cuda.synchronize()
    _check_grads(g, _reference(ro, cam, sc, bg, ctx, gC, gD, gA), ctx["allow"])


def test_a_gaussian_with_a_depth_gradient_only(R, ro):
    """One Gaussian, gD != 0 on the pixels it covers, zero colour gradient: only the aux kernel adds to its row, so its
    position gradient exists only if that kernel marks the gradient support and fills slot 9."""
    cam, sc0, bg = small_scene(0, deg=0)
    p = oracle_params(ro, cam, sc0, bg)
    f0 = ro.forward(p, sc0["means3D"], sc0["opacities"], shs=sc0["shs"], scales=sc0["scales"], rotations=sc0["rotations"])
    counts = np.bincount(f0["point_list"], minlength=p.P) * (f0["radii"] > 0)
    k = int(np.argmax(counts))
    sc = {key: (v[k:k + 1].copy() if key != "sh_degree" else v) for key, v in sc0.items()}
    sc["opacities"][:] = 0.8
    ctx = _forward_and_check(R, ro, cam, sc, bg)
    covered = ctx["f_aux"]["n_contrib"] > 0
    assert covered.sum() > 4
    H, W = cam["H"], cam["W"]
    gD = np.where(covered, 1.0 + np.random.default_rng(1).random((H, W)), 0.0).astype(np.float32)[None]
    g = R.rasterize_backward(ctx["rs"], ctx["st"], torch.zeros(3, H, W, device="cuda"), ctx["m3"], grad_expected_depth=_dev(gD),
                             **ctx["gkw"])
    sup = ctx["st"].tensor("grad_support", (1,), torch.uint8)
    torch.cuda.synchronize()
    assert int(sup[0]) == 1
    ref = _reference(ro, cam, sc, bg, ctx, None, gD, None)
    assert np.abs(ref["dz"]).max() > 0 and float(g["means3D"].abs().max()) > 0
    assert (g["shs"] == 0).all()
    _check_grads(g, ref, ctx["allow"])


def test_raw_path_equals_activations_plus_standard_path(R):
    from multiview_inpaint_amd import train_ops as T
    cam, sc, bg = small_scene(21, N=1500, W=160, H=112, deg=3, log_scale=np.log(0.05))
    t = {k: _dev(v) for k, v in sc.items() if k != "sh_degree"}
    P = t["shs"].shape[0]
    gen = torch.Generator("cuda").manual_seed(1)
    raw = dict(xyz=t["means3D"], dc=t["shs"][:, :1].contiguous(), rest=t["shs"][:, 1:].contiguous(),
               o=torch.logit(t["opacities"].clamp(1e-4, 1 - 1e-4)), s=torch.log(t["scales"]),
               q=t["rotations"] * (0.5 + torch.rand(P, 1, device="cuda", generator=gen)))
    rast = R.GaussianRasterizer(_settings(R, cam, bg, 3))
    gC = torch.randn(3, cam["H"], cam["W"], device="cuda", generator=gen)
    gD, gA = (torch.randn(1, cam["H"], cam["W"], device="cuda", generator=gen) for _ in range(2))

    def run(raw_mode):
        p = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
        m2d = torch.zeros(P, 3, device="cuda", requires_grad=True)
        if raw_mode:
            o = rast.forward_raw_aux(p["xyz"], m2d, p["dc"], p["rest"], p["o"], p["s"], p["q"])
        else:
            scales, rots, opac, shs = T.activate_gaussians(p["s"], p["q"], p["o"], p["dc"], p["rest"])
            o = rast.forward_aux(means3D=p["xyz"], means2D=m2d, shs=shs, opacities=opac, scales=scales, rotations=rots)
        assert isinstance(o, R.RasterAuxOutput) and not o.depth.requires_grad and o.expected_depth.requires_grad and o.alpha.requires_grad
        ((o.color * gC).sum() + (o.expected_depth * gD).sum() + (o.alpha * gA).sum()).backward()
        return o, {**{k: v.grad for k, v in p.items()}, "m2d": m2d.grad}

    o0, g0 = run(False)
    o1, g1 = run(True)
    assert torch.equal(o0.radii, o1.radii) and int((o0.radii > 0).sum()) > P // 3
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)                                            # the forward has no atomics: identical
    # the depth part of the position gradient is there: colour-only gradients differ from these by far more than the bar
    p = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    c, _, _ = rast.forward_raw(p["xyz"], torch.zeros(P, 3, device="cuda"), p["dc"], p["rest"], p["o"], p["s"], p["q"])
    (c * gC).sum().backward()
    assert not same_to_summation_order(p["xyz"].grad.cpu().numpy(), g1["xyz"].cpu().numpy(), 1e-3)
    for k in g0:
        assert g1[k] is not None and g1[k].shape == g0[k].shape, k
        assert same_to_summation_order(g1[k].cpu().numpy(), g0[k].cpu().numpy()), k


def test_autograd_end_to_end(R, ro):
    cam, sc, bg = small_scene(1, deg=3)
    ctx = _forward_and_check(R, ro, cam, sc, bg)
    leaves = {k: _dev(sc[k]).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    m2d = torch.zeros(ctx["st"].P, 3, device="cuda", requires_grad=True)
    gen = torch.Generator("cuda").manual_seed(2)
    H, W = cam["H"], cam["W"]
    target, gt = 3.0 * torch.rand(1, H, W, device="cuda", generator=gen), torch.rand(3, H, W, device="cuda", generator=gen)

    def loss_of(color, ed, alpha):
        return (ed / alpha.clamp_min(1e-3) - target).abs().mean() + alpha.mean() + (color - gt).abs().mean()
    o = R.GaussianRasterizer(ctx["rs"]).forward_aux(means3D=leaves["means3D"], means2D=m2d, shs=leaves["shs"],
                                                    opacities=leaves["opacities"], scales=leaves["scales"],
                                                    rotations=leaves["rotations"])
    assert len(o) == 5 and not o.depth.requires_grad
    loss_of(o.color, o.expected_depth, o.alpha).backward()
    # the upstream image gradients of the same loss, by torch on detached copies of the three images
    imgs = [t.detach().clone().requires_grad_(True) for t in (o.color, o.expected_depth, o.alpha)]
    gC, gD, gA = (t.cpu().numpy() for t in torch.autograd.grad(loss_of(*imgs), imgs))
    ref = _reference(ro, cam, sc, bg, ctx, gC, gD, gA)
    g = {k: v.grad for k, v in leaves.items()}
    g["means2D"] = m2d.grad
    for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        assert g[k] is not None and g[k].shape == (leaves[k].shape if k in leaves else m2d.shape), k
        grad_check(k, g[k].cpu().numpy(), ref[k], ctx["allow"])


def test_mid_size_100k_800(R, ro):
    """The 100k Gaussians / 800 x 800 scene of test_bringup_config_100k_800: forward and the joint backward."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cam = syn.make_camera(800, 800, 50.0)
    sc = syn.make_scene(100_000, cam, 3, seed=0)
    bg = np.zeros(3, np.float32)
    rng = np.random.default_rng(0)
    gD, gA, gC = (rng.normal(size=(c, 800, 800)).astype(np.float32) for c in (1, 1, 3))
    ro.set_threads(max(1, min(16, avail)))
    try:
        ctx = _forward_and_check(R, ro, cam, sc, bg)
        ref = _reference(ro, cam, sc, bg, ctx, gC, gD, gA)
    finally:
        ro.set_threads(1)
    g = R.rasterize_backward(ctx["rs"], ctx["st"], _dev(gC), ctx["m3"], grad_expected_depth=_dev(gD), grad_alpha=_dev(gA), **ctx["gkw"])
    _check_grads(g, ref, ctx["allow"])


def test_degenerate_cases(R):
    cam = syn.make_camera(48, 32, 60.0)
    bg = np.array([0.2, 0.4, 0.6], np.float32)
    rast = R.GaussianRasterizer(_settings(R, cam, bg, 0))
    z = lambda *s: torch.zeros(*s, device="cuda")
    # P = 0
    m = z(0, 3).requires_grad_(True)
    o = rast.forward_aux(means3D=m, means2D=z(0, 3), shs=z(0, 1, 3), opacities=z(0, 1), scales=z(0, 3), rotations=z(0, 4))
    assert (o.expected_depth == 0).all() and (o.alpha == 0).all() and (o.depth == 15.0).all()
    (o.expected_depth.sum() + o.alpha.sum() + o.color.sum()).backward()
    assert m.grad.shape == (0, 3)
    # every Gaussian behind the camera: num_rendered = 0
    N = 16
    means = z(N, 3)
    means[:, 2] = torch.linspace(-3, 0.2, N)
    means.requires_grad_(True)
    op = torch.full((N, 1), 0.9, device="cuda", requires_grad=True)
    o = rast.forward_aux(means3D=means, means2D=z(N, 3), shs=torch.ones(N, 1, 3, device="cuda"), opacities=op,
                         scales=torch.full((N, 3), 0.1, device="cuda"), rotations=torch.tensor([[1.0, 0, 0, 0]], device="cuda").repeat(N, 1))
    assert (o.radii == 0).all() and (o.expected_depth == 0).all() and (o.alpha == 0).all()
    ((o.expected_depth * 2).sum() + o.alpha.sum() + o.color.sum()).backward()
    torch.cuda.synchronize()
    assert (means.grad == 0).all() and (op.grad == 0).all()


def test_no_aux_gradients_is_the_plain_backward_bit_for_bit(R):
    """Both aux gradients None: nothing is launched and the rows go the way they always went. One 16 x 16 tile, so that every
    accumulation row is added to once per slot and two runs of the float atomics cannot differ in their order."""
    cam, sc, bg = small_scene(2, N=40, W=16, H=16, deg=1, pose=False)
    rs = _settings(R, cam, bg, 1)
    kw = dict(shs=_dev(sc["shs"]), scales=_dev(sc["scales"]), rotations=_dev(sc["rotations"]))
    m3, op = _dev(sc["means3D"]), _dev(sc["opacities"])
    gC = torch.randn(3, 16, 16, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    out = []
    for aux, extra in ((False, {}), (True, dict(grad_expected_depth=None, grad_alpha=None)), (True, {})):
        _, radii, _, st = R.rasterize_forward(rs, m3, op, prepare_backward=True, aux=aux, **kw)
        out.append(R.rasterize_backward(rs, st, gC, m3, **extra, **kw))
    assert int((radii > 0).sum()) > 10 and float(out[0]["means3D"].abs().max()) > 0
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(out[0][k], out[1][k]) and torch.equal(out[0][k], out[2][k]), k


def test_patched_render_adds_the_aux_keys_only_when_asked(monkeypatch):
    import test_patch_render_gpu as PR
    from multiview_inpaint_amd.dropin import patch_gs_simp
    cam, sc, bg = small_scene(34, N=500, W=64, H=48, deg=1, pose=True, log_scale=np.log(0.05))
    camera, bg_t = PR.Camera(cam), torch.tensor(bg, device="cuda")
    patched = patch_gs_simp._make_render(PR.standin_render, PR.Model)
    monkeypatch.delenv("MVI_RENDER_AUX", raising=False)
    pc = PR.Model(sc, 1, 1)
    base = patched(camera, pc, PR.Pipe(), bg_t)
    assert list(base.keys()) == ["render", "depth", "viewspace_points", "visibility_filter", "radii"]
    monkeypatch.setenv("MVI_RENDER_AUX", "1")
    pkg = patched(camera, pc, PR.Pipe(), bg_t)
    assert list(pkg.keys()) == list(base.keys()) + ["expected_depth", "alpha"]
    assert pkg["expected_depth"].requires_grad and pkg["alpha"].requires_grad and not pkg["depth"].requires_grad
    assert torch.equal(pkg["render"], base["render"]) and torch.equal(pkg["depth"], base["depth"]) and torch.equal(pkg["radii"], base["radii"])
    (pkg["expected_depth"].sum() + pkg["alpha"].sum()).backward()
    assert float(pc._xyz.grad.abs().max()) > 0 and float(pc._opacity.grad.abs().max()) > 0
    assert pkg["viewspace_points"].grad is not None

"""Aux outputs of the rasterizer (expected depth, alpha), the parts that need no GPU: the reference construction the GPU tests
compare against is pinned against torch.autograd in fp64, and the three C entry points are bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from oracle import raster_torch as rt
from raster_aux_helpers import aux_backward, aux_forward
from raster_helpers import rel_err, small_scene


@pytest.mark.parametrize("seed,deg,pose", [(0, 3, True), (12, 1, False)])
def test_composed_reference_equals_autograd_through_the_torch_oracle(seed, deg, pose):
    """colors_precomp = (z, 1, 0), bg = 0 through oracle/raster_oracle.c, plus dL/dz * V[0:3, 2] on the positions, against
    autograd through oracle/raster_torch.render with the colours (tz, 1, 0) built differentiably from means3D: every input
    gradient, at the bar test_oracle_raster.py holds the C oracle to (2e-4 of the array's scale: its own fp32 error)."""
    cam, sc, bg = small_scene(seed, N=80, W=40, H=36, deg=deg, pose=pose)
    rng = np.random.default_rng(seed + 100)
    gD = rng.normal(size=(cam["H"], cam["W"])).astype(np.float32)
    gA = rng.normal(size=(cam["H"], cam["W"])).astype(np.float32)
    cov_kw = dict(scales=sc["scales"], rotations=sc["rotations"])
    # z: the per-Gaussian view depth of the C oracle's own forward (what the GPU forward reproduces bit for bit)
    z = ro.forward(ro.make_params(80, deg, sc["shs"].shape[1], cam["W"], cam["H"], cam["tanfovx"], cam["tanfovy"], 1.0,
                                  cam["viewmatrix"], cam["projmatrix"], cam["campos"], bg),
                   sc["means3D"], sc["opacities"], shs=sc["shs"], render=False, **cov_kw)["depths"]
    p0, f = aux_forward(ro, cam, sc, z, cov_kw)
    ref = aux_backward(ro, cam, sc, p0, f, z, gD, gA, cov_kw)

    dt = torch.float64
    t = {k: torch.tensor(np.asarray(sc[k], np.float64), requires_grad=True) for k in ("means3D", "opacities", "scales", "rotations")}
    m2d = torch.zeros(80, 3, dtype=dt, requires_grad=True)
    V = torch.tensor(np.asarray(cam["viewmatrix"], np.float64).reshape(4, 4))
    tz = t["means3D"] @ V[0:3, 2] + V[3, 2]
    cols = torch.stack([tz, torch.ones_like(tz), torch.zeros_like(tz)], 1)
    col, _, radii, aux = rt.render(cam, np.zeros(3), deg, t["means3D"], m2d, t["opacities"], colors_precomp=cols,
                                   scales=t["scales"], rotations=t["rotations"])
    assert np.array_equal(f["radii"], radii.numpy()) and (f["radii"] > 0).sum() > 20
    assert rel_err(f["color"][0], col[0].detach().numpy()) < 1e-5          # expected depth
    assert rel_err(f["color"][1], col[1].detach().numpy()) < 1e-5          # alpha
    assert rel_err(f["color"][1], 1.0 - aux["final_T"].detach().numpy()) < 1e-5
    (col[0] * torch.tensor(gD, dtype=dt) + col[1] * torch.tensor(gA, dtype=dt)).sum().backward()
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert rel_err(ref[k], t[k].grad.numpy()) < 2e-4, k
    assert rel_err(ref["means2D"], m2d.grad.numpy()) < 2e-4
    # the position gradient really has a depth part: without it the composition is off by far more than the bar
    assert rel_err(ref["means3D"] - ref["dz"][:, None] * V[0:3, 2].numpy()[None], t["means3D"].grad.numpy()) > 1e-2


def test_the_three_entry_points_are_bound_and_there_is_no_cpu_path():
    from multiview_inpaint_amd import _lib, raster as R
    L = _lib.lib()
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    S = C.POINTER(_lib.RasterSettings)
    want = {"mvi_raster_forward_render_aux": [S, i32, i64, vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp],
            "mvi_raster_backward_render_aux": [S, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp],
            "mvi_raster_backward_depth_to_means": [S, i32, vp, vp, vp]}
    header = open(_lib.INCLUDE_DIR + "/mvi_raster.h").read()
    for name, argtypes in want.items():
        assert name in _lib.declared_symbols() and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        decl = header[header.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(argtypes), name     # as many parameters as the header declares
    # argument errors come back as errors, not as launches: a NULL settings struct, and NULL aux outputs
    assert L.mvi_raster_backward_depth_to_means(None, 0, None, None, None) == -1
    assert L.mvi_raster_backward_render_aux(None, 0, 0, None, None, None, None, None, None, None, None) == -1
    cam, sc, bg = small_scene(0, N=8, W=16, H=16, deg=0)
    rs = R.GaussianRasterizationSettings(
        image_height=16, image_width=16, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.tensor(bg), scale_modifier=1.0,
        viewmatrix=torch.tensor(cam["viewmatrix"]), projmatrix=torch.tensor(cam["projmatrix"]), sh_degree=0,
        campos=torch.tensor(cam["campos"]), prefiltered=False)
    t = {k: torch.tensor(v) for k, v in sc.items() if k != "sh_degree"}
    rast = R.GaussianRasterizer(rs)
    kw = dict(means3D=t["means3D"], means2D=torch.zeros(8, 3), shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
              rotations=t["rotations"])
    with pytest.raises(RuntimeError, match="no CPU path") as e0:
        rast(**kw)
    with pytest.raises(RuntimeError, match="no CPU path") as e1:
        rast.forward_aux(**kw)
    assert str(e0.value) == str(e1.value)
    assert R.RasterAuxOutput._fields == ("color", "radii", "depth", "expected_depth", "alpha")
    assert len(R.GaussianRasterizationSettings._fields) == 11
    # the view-parallel forms are out of scope and say so
    for fn, n in ((R.rasterize_backward_split, 8), (R.rasterize_backward_ranged, 8)):
        with pytest.raises(NotImplementedError, match="grad_expected_depth"):
            fn(*([None] * n), grad_alpha=torch.zeros(1))
    with pytest.raises(NotImplementedError, match="grad_expected_depth"):
        R.rasterize_backward_raw(*([None] * 9), sh_grad="factor", grad_expected_depth=torch.zeros(1))

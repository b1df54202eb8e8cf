"""Box-region kernels (csrc/box_region.hip) against the reference's own outputs (tests/golden/box_region/, written by
tools/gen_golden_box_region.py from gs-simp/utils/bounding.py on the seeded inputs of box_region_helpers.py).

Hit decisions (cond, t_ind, inside, mask) are exact outside the generator's margin set; t and the hit points are within
1e-6 relative + 1e-6 absolute on hits; the adversarial rays match exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_region_helpers as H
from multiview_inpaint_amd import box_region as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mesh(kind):
    return B.BoxMesh.from_obj(H.mesh_path(kind), device=DEV)


def _close(got, want):
    return np.abs(got.astype(np.float64) - want) <= 1e-6 * np.abs(want) + 1e-6


@pytest.mark.parametrize("kind", sorted(H.MESHES))
def test_intersect_matches_the_reference(kind):
    mesh = _mesh(kind)
    g = np.load(H.golden_path(f"rays_{kind}.npz"))
    for name, (o, d) in H.ray_sets(mesh.f_v.cpu().numpy(), H.RAY_SEEDS[kind]).items():
        n = o.shape[0]
        p, t, i, c = B.intersect(mesh, torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV))
        assert (p.shape, t.shape, i.shape, c.shape) == ((n, 3), (n, 1), (n, 1), (n, 1))
        assert (p.dtype, t.dtype, i.dtype, c.dtype) == (torch.float32, torch.float32, torch.int64, torch.bool)
        p, t, i, c = p.cpu().numpy(), t.cpu().numpy()[:, 0], i.cpu().numpy()[:, 0], c.cpu().numpy()[:, 0]
        wc = H.unpack(g[f"{name}_cond"], n)
        wt, wi, wp = g[f"{name}_int_t"], g[f"{name}_t_ind"].astype(np.int64), g[f"{name}_int_p"]
        if name == "adversarial":
            assert np.array_equal(c, wc) and np.array_equal(i, wi), name
            assert np.array_equal(t, wt) and np.array_equal(p, wp), name
            continue
        ok = ~H.unpack(g[f"{name}_margin"], n)
        assert np.array_equal(c[ok], wc[ok]), f"{kind}/{name}: cond differs on {int((c != wc)[ok].sum())} rays"
        assert np.array_equal(i[ok], wi[ok]), f"{kind}/{name}: t_ind differs on {int((i != wi)[ok].sum())} rays"
        hit = ok & wc & c
        assert _close(t[hit], wt[hit]).all(), f"{kind}/{name}: int_t"
        assert _close(p[hit], wp[hit]).all(), f"{kind}/{name}: int_p"
        assert not t[~c].any() and not p[~c].any()
        assert wc.sum() > 0


def test_points_inside_at_1_5m_points():
    mesh = _mesh("del")
    g = np.load(H.golden_path("points_del.npz"))
    xyz = H.del_points(mesh.f_v.cpu().numpy(), H.N_POINTS, H.POINTS_SEED)
    got = B.points_inside(mesh, torch.from_numpy(xyz).to(DEV))
    assert got.dtype == torch.bool and got.shape == (H.N_POINTS,)
    got = got.cpu().numpy()
    want, ok = H.unpack(g["inside"], H.N_POINTS), ~H.unpack(g["margin"], H.N_POINTS)
    assert np.array_equal(got[ok], want[ok]), f"inside differs on {int((got != want)[ok].sum())} points"
    assert 0 < want.sum() < H.N_POINTS


def _mask_inputs(name):
    kind, V, Hh, Ww, seed = H.MASK_SETS[name]
    f_v = np.load(H.golden_path(f"mesh_{kind}.npz"))["f_v"]
    c2w, fovx, fovy = H.cameras(f_v, V, Hh, Ww, seed)
    return kind, c2w, fovx, fovy, H.depth_maps(f_v, V, Hh, Ww, seed + 100), H.renders(V, Hh, Ww, seed + 200)


@pytest.mark.parametrize("name", sorted(H.MASK_SETS))
def test_view_masks_match_the_reference(name):
    kind, c2w, fovx, fovy, depth, render = _mask_inputs(name)
    V, _, Hh, Ww = depth.shape
    g = np.load(H.golden_path(f"masks_{name}.npz"))
    out = B.view_masks(_mesh(kind), torch.from_numpy(c2w).to(DEV), fovx, fovy, torch.from_numpy(depth).to(DEV),
                       render=torch.from_numpy(render).to(DEV), disparity=True)
    mask = out["mask"].cpu().numpy()
    assert mask.shape == (V, 1, Hh, Ww) and set(np.unique(mask)) <= {0.0, 1.0}
    want = H.unpack(g["mask"], mask.size).reshape(mask.shape)
    ok = ~H.unpack(g["margin"], mask.size).reshape(mask.shape)
    got = mask != 0
    assert np.array_equal(got[ok], want[ok]), f"mask differs on {int((got != want)[ok].sum())} pixels"
    m = want.astype(np.float32)
    same = np.broadcast_to(got == want, render.shape)
    exp = render * (np.float32(1) - m) + m                                  # gen_seq.py:52
    assert np.array_equal(out["masked"].cpu().numpy()[same], exp[same])
    assert np.array_equal(out["disparity"].cpu().numpy(), np.float32(1) / np.maximum(depth, np.float32(1e-3)))


def test_view_masks_batched_equals_single_views():
    kind, c2w, fovx, fovy, depth, render = _mask_inputs("seq")
    mesh = _mesh(kind)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    allv = B.view_masks(mesh, t(c2w), fovx, fovy, t(depth), render=t(render), disparity=True)
    for k in range(depth.shape[0]):
        one = B.view_masks(mesh, t(c2w[k:k + 1]), [fovx[k]], [fovy[k]], t(depth[k:k + 1]), render=t(render[k:k + 1]), disparity=True)
        for key in ("mask", "masked", "disparity"):
            assert torch.equal(allv[key][k:k + 1], one[key]), (k, key)


def test_patched_torchmesh_intersect_on_cuda_rays():
    from multiview_inpaint_amd.dropin import patch_gs_simp

    class StandIn:
        def __init__(self, f_v):
            self.f_v = f_v

        def intersect(self, rayo, rayd, bs=10000):
            raise AssertionError("CUDA rays must not reach the reference method")

    StandIn.intersect = patch_gs_simp._make_intersect(StandIn.intersect)
    g = np.load(H.golden_path("rays_add.npz"))
    mesh = StandIn(torch.from_numpy(np.load(H.golden_path("mesh_add.npz"))["f_v"]).to(DEV))
    o, d = H.ray_sets(mesh.f_v.cpu().numpy(), H.RAY_SEEDS["add"])["random"]
    n = o.shape[0]
    p, t, i, c = mesh.intersect(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), bs=10000)
    assert (p.shape, t.shape, i.shape, c.shape) == ((n, 3), (n, 1), (n, 1), (n, 1))
    assert (p.dtype, t.dtype, i.dtype, c.dtype) == (torch.float32, torch.float32, torch.int64, torch.bool)
    ok = ~H.unpack(g["random_margin"], n)
    wc = H.unpack(g["random_cond"], n)
    assert np.array_equal(c.cpu().numpy()[:, 0][ok], wc[ok])
    assert np.array_equal(i.cpu().numpy()[:, 0][ok], g["random_t_ind"].astype(np.int64)[ok])
    hit = ok & wc
    assert _close(t.cpu().numpy()[:, 0][hit], g["random_int_t"][hit]).all()


def test_delete_cli_keeps_the_reference_rows(tmp_path):
    from multiview_inpaint_amd import gaussian_io
    f_v = np.load(H.golden_path("mesh_del.npz"))["f_v"]
    g = H.ply_gaussians(f_v, H.N_PLY, H.PLY_SEED)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    gaussian_io.save_ply(src, g["xyz"], g["features_dc"], g["features_rest"], g["opacity"], g["scaling"], g["rotation"])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "multiview_inpaint_amd.box_region", "delete", "--mesh", H.mesh_path("del"),
                        "--ply", src, "--out", dst], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    keep = H.unpack(np.load(H.golden_path("points_del.npz"))["ply_keep"], H.N_PLY)
    assert 0 < keep.sum() < H.N_PLY
    out = gaussian_io.load_ply(dst, 0)
    for k, v in g.items():
        assert out[k].shape == v[keep].shape and np.array_equal(out[k], v[keep]), k
    assert open(dst, "rb").read().split(b"end_header")[0] == open(src, "rb").read().split(b"end_header")[0].replace(
        f"element vertex {H.N_PLY}".encode(), f"element vertex {int(keep.sum())}".encode())


def test_bad_input_raises():
    mesh = _mesh("add")
    o = torch.zeros(10, 3, device=DEV)
    with pytest.raises(TypeError):
        B.intersect(mesh, o.double(), o.double())
    with pytest.raises(RuntimeError):
        B.intersect(mesh, o.cpu(), o.cpu())
    with pytest.raises(ValueError):
        B.intersect(B.BoxMesh(None, None, torch.zeros(0, 3, 3, device=DEV), None, None, None), o, o)
    with pytest.raises(ValueError):
        B.points_inside(B.BoxMesh(None, None, torch.zeros(0, 3, 3, device=DEV), None, None, None), o)
    c2w = torch.eye(4, device=DEV).expand(2, 4, 4).contiguous()
    with pytest.raises(ValueError):
        B.view_masks(mesh, c2w, 0.8, 0.8, torch.ones(3, 1, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        B.view_masks(mesh, c2w, [0.8, 0.8, 0.8], 0.8, torch.ones(2, 1, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        B.view_masks(mesh, c2w, 0.8, 0.8, torch.ones(2, 1, 8, 8, device=DEV), render=torch.ones(3, 3, 8, 8, device=DEV))

"""Generates tests/golden/box_region/ from the reference itself, on the CPU of a development machine that has the reference
tree (never on the GPU box, never by the tests):

    python tools/gen_golden_box_region.py /path/to/MultiView_Inpaint

It imports gs-simp/utils/bounding.py (numpy + torch only) and loads gs-simp/scene/helpers.py by file path (scene/__init__
needs plyfile), and writes DATA only: the three box .obj files as shipped (the 10 008-vertex one gzip-compressed), the reference-parsed mesh arrays, and the
reference's outputs on the seeded inputs of tests/box_region_helpers.py — intersect results per ray set, `inside` bits of
del.py's rule at 1.5 M points, the kept rows of the delete CLI's scene, and gen_seq.py's masks of a 3-view 512 x 384 sequence
and of one 1920 x 1080 view.

Ray counts avoid n % 10000 == 3 and every mesh has F = 12 != 3: the reference's torch.cross without `dim` crosses over the
FIRST axis of length 3 of its [n, F, 3] operands, which is wrong exactly for a chunk of 3 rays or a 3-face mesh; the HIP
kernels implement the last-axis product the code intends, and the fixtures stay clear of the cases where the two differ.

Margin flags (fp64, bit per ray / point / pixel): the rays whose hit decisions sit within rounding distance of a threshold,
where the tests compare only t values. A ray is at the margin when, for any face, |u|, |v|, |1 - u| or |1 - u - v| < 1e-5
(barycentric edges), 0 <= t < 1e-6 (origin on the surface), or |a| < 1e-6 with |s . h| < 1e-5 (near-parallel face that
could pass the u test; with |s . h| >= 1e-5 the fp32 u = (s . h) / (a + 1e-8) is far outside [0, 1] whichever way a rounds,
so an exactly parallel face — a = 0, as the faces along x of an axis-aligned box are for del.py's +-x rays — is no margin;
nor is a face whose h = d x e2 is exactly zero, d parallel to an edge: its fp32 h, a and u are exact zeros too, and it is
invalid both ways).
A mask pixel is also at the margin when |t - depth| <= 1e-5 depth. Under 1 % of each random set may be at the margin
(asserted here).
"""
import gzip
import importlib.util
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import box_region_helpers as H  # noqa: E402


def _load_reference(ref_root):
    gs = os.path.join(ref_root, "gs-simp")
    sys.path.insert(0, gs)
    from utils import bounding                                     # noqa: E402
    spec = importlib.util.spec_from_file_location("ref_scene_helpers", os.path.join(gs, "scene", "helpers.py"))
    helpers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(helpers)
    return gs, bounding, helpers


def ray_margin(o, d, f_v, chunk=200_000):
    """fp64 margin flags of rays o, d [n,3] against f_v [F,3,3] (see the module docstring)."""
    o, d, fv = o.astype(np.float64), d.astype(np.float64), f_v.astype(np.float64)
    v0, e1, e2 = fv[:, 0], fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]
    out = np.zeros(o.shape[0], bool)
    for s0 in range(0, o.shape[0], chunk):
        oc, dc = o[s0:s0 + chunk, None, :], d[s0:s0 + chunk]
        dc = (dc / np.maximum(np.linalg.norm(dc, axis=-1, keepdims=True), 1e-12))[:, None, :]
        h = np.cross(dc, e2[None])
        a = (e1[None] * h).sum(-1)
        s = oc - v0[None]
        sh = (s * h).sum(-1)
        q = np.cross(s, e1[None])
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v, t = sh / a, (dc * q).sum(-1) / a, (e2[None] * q).sum(-1) / a
            m = (np.abs(u) < 1e-5) | (np.abs(v) < 1e-5) | (np.abs(1 - u) < 1e-5) | (np.abs(1 - u - v) < 1e-5)
            m |= (t >= 0) & (t < 1e-6) & (u >= 0) & (v >= 0) & (u + v <= 1)
        m |= (np.abs(a) < 1e-6) & (np.abs(sh) < 1e-5) & (np.abs(h).max(-1) > 0)
        out[s0:s0 + chunk] = m.any(-1)
    return out


def ref_intersect(mesh, o, d):
    with torch.no_grad():
        p, t, i, c = mesh.intersect(torch.from_numpy(o), torch.from_numpy(d))
    return p.numpy(), t.numpy()[:, 0], i.numpy()[:, 0], c.numpy()[:, 0]


class _View:
    """The attributes scene/helpers.py get_rays reads from a Camera."""

    def __init__(self, c2w, fovx, fovy, H_, W_):
        self.camera_to_world = torch.from_numpy(c2w)
        self.FoVx, self.FoVy, self.image_height, self.image_width, self.data_device = float(fovx), float(fovy), H_, W_, "cpu"


def ref_masks(mesh, helpers, f_v, c2w, fovx, fovy, depth):
    V, _, Hh, Ww = depth.shape
    masks, margins = np.zeros((V, Hh, Ww), bool), np.zeros((V, Hh, Ww), bool)
    for k in range(V):
        ro, rd = helpers.get_rays(_View(c2w[k], fovx[k], fovy[k], Hh, Ww))
        with torch.no_grad():
            _, t, _, _ = mesh.intersect(ro, rd)
        t = t.view(Hh, Ww)[None]
        dep = torch.from_numpy(depth[k])
        masks[k] = ((t > 0.) & ((t < dep) | (dep == 15.)))[0].numpy()                 # gen_seq.py:49
        tn, dn = t[0].numpy().astype(np.float64), depth[k, 0].astype(np.float64)
        margins[k] = ray_margin(ro.numpy(), rd.numpy(), f_v).reshape(Hh, Ww) | ((tn > 0) & (np.abs(tn - dn) <= 1e-5 * dn))
    return masks, margins


def _assert_margin(name, m):
    frac = float(m.mean())
    print(f"  {name}: {int(m.sum())} of {m.size} at the margin ({100 * frac:.3f} %)")
    assert frac < 0.01, f"{name}: {100 * frac:.2f} % at the margin"


def main(ref_root):
    gs, bounding, helpers = _load_reference(ref_root)
    os.makedirs(H.GOLDEN, exist_ok=True)
    meshes = {}
    for kind, fn in H.MESHES.items():
        src = os.path.join(gs, "bds", "del" if kind == "del" else "add", fn.replace(".gz", ""))
        if fn.endswith(".gz"):
            with open(src, "rb") as f, open(H.stored_mesh_path(kind), "wb") as raw, \
                    gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as z:
                z.write(f.read())
        else:
            shutil.copyfile(src, H.stored_mesh_path(kind))
        m = bounding.torchMesh(src)
        meshes[kind] = m
        np.savez_compressed(H.golden_path(f"mesh_{kind}.npz"), **{k: getattr(m, k).numpy() for k in
                                                                  ("v", "f", "f_v", "axes", "origin", "center")})
        f_v = m.f_v.numpy()
        assert f_v.shape[0] != 3
        out = {}
        for name, (o, d) in H.ray_sets(f_v, H.RAY_SEEDS[kind]).items():
            assert o.shape[0] % 10000 != 3
            p, t, i, c = ref_intersect(m, o, d)
            mg = ray_margin(o, d, f_v)
            if name != "adversarial":
                _assert_margin(f"{kind}/{name}", mg)
            out.update({f"{name}_int_p": p, f"{name}_int_t": t, f"{name}_t_ind": i.astype(np.int8),
                        f"{name}_cond": np.packbits(c), f"{name}_margin": np.packbits(mg)})
            print(f"  {kind}/{name}: {int(c.sum())} of {c.size} hit")
        np.savez_compressed(H.golden_path(f"rays_{kind}.npz"), **out)
    # del.py:104-108 at 1.5 M points, against the `del` box
    m, f_v = meshes["del"], meshes["del"].f_v.numpy()
    xyz = H.del_points(f_v, H.N_POINTS, H.POINTS_SEED)
    n = xyz.shape[0]
    pos_d = np.tile(np.array([[1., 0., 0.]], np.float32), (n, 1))
    _, pos_t, _, _ = ref_intersect(m, xyz, pos_d)
    _, neg_t, _, _ = ref_intersect(m, xyz, -pos_d)
    inside = (pos_t > 0.) & (neg_t > 0.)
    mg = ray_margin(xyz, pos_d, f_v) | ray_margin(xyz, -pos_d, f_v)
    _assert_margin("points", mg)
    print(f"  points: {int(inside.sum())} of {n} inside")
    g = H.ply_gaussians(f_v, H.N_PLY, H.PLY_SEED)
    pd = np.tile(np.array([[1., 0., 0.]], np.float32), (H.N_PLY, 1))
    keep = ~((ref_intersect(m, g["xyz"], pd)[1] > 0.) & (ref_intersect(m, g["xyz"], -pd)[1] > 0.))
    ply_mg = ray_margin(g["xyz"], pd, f_v) | ray_margin(g["xyz"], -pd, f_v)
    assert not ply_mg.any(), "the delete scene must have no margin point (its rows are compared bit for bit)"
    np.savez_compressed(H.golden_path("points_del.npz"), inside=np.packbits(inside), margin=np.packbits(mg),
                        ply_keep=np.packbits(keep))
    # gen_seq.py:46-52: a 3-view sequence at 512 x 384 (the `add` box) and one 1920 x 1080 view (the 10 008-vertex box)
    for name, (kind, V, Hh, Ww, seed) in H.MASK_SETS.items():
        f_v = meshes[kind].f_v.numpy()
        c2w, fovx, fovy = H.cameras(f_v, V, Hh, Ww, seed)
        depth = H.depth_maps(f_v, V, Hh, Ww, seed + 100)
        masks, margins = ref_masks(meshes[kind], helpers, f_v, c2w, fovx, fovy, depth)
        _assert_margin(f"masks_{name}", margins)
        print(f"  masks_{name}: {int(masks.sum())} of {masks.size} pixels masked")
        np.savez_compressed(H.golden_path(f"masks_{name}.npz"), mask=np.packbits(masks), margin=np.packbits(margins))
    for fn in sorted(os.listdir(H.GOLDEN)):
        sz = os.path.getsize(H.golden_path(fn))
        print(f"  {fn}: {sz} bytes")
        assert sz < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MVI_REFERENCE_ROOT", ""))

"""Box-region masks on the GPU: rays against the hand-made bounding-box mesh of the inpainting pipeline.

Reference: gs-simp/utils/bounding.py (torchMesh: the OBJ reader :5-46, intersect :62-121), the inpaint masks of
gs-simp/gen_seq.py:46-52, the point deletion of gs-simp/del.py:104-111 and the disparity of render_depth.py:37. The ray-face
rule, its fp32 operation order and the one deliberate difference (the cross product over the LAST axis) are documented in
include/mvi_box_region.h; every op here is one HIP launch (csrc/box_region.hip) and takes CUDA tensors only — there is no
CPU path.

    python -m multiview_inpaint_amd.box_region delete --mesh BOX.obj --ply IN.ply --out OUT.ply

is del.py's product for one scene: the Gaussians inside the box are dropped, every attribute of the others is kept.
"""
import argparse
import ctypes as C
import math
import sys

import numpy as np
import torch

from . import _lib


def _check(rc, what):
    if rc != 0:
        msg = _lib.lib().mvi_box_region_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class BoxMesh:
    """The box mesh as torchMesh holds it: v [nv,3] fp32, f [F,3] int32, f_v [F,3,3] fp32, axes [3,3], origin [1,3],
    center [1,3] (fp32), on `device`."""

    def __init__(self, v, f, f_v, axes, origin, center):
        self.v, self.f, self.f_v, self.axes, self.origin, self.center = v, f, f_v, axes, origin, center

    @classmethod
    def from_obj(cls, path, inverse=True, device="cuda"):
        """bounding.py:5-46: `v x y z` lines (mapped to (x, -z, y) when `inverse`), each quad `f v1 v2 v3 v4` split into the
        triangles (v1, v2, v3), (v1, v3, v4); the box frame comes from the first quad (p1, p2, p3 = its first three corners)
        and from the LAST later quad that shares the edge (p2, p3) with it (p4, p5 by the reference's four cases):
        axes = [v[p3] - v[p2], v[p1] - v[p2], v[p5] - v[p4]], origin = v[p2], center = origin + sum(axes / 2)."""
        verts, faces = [], []
        p1 = p2 = p3 = p4 = p5 = None
        with open(path) as fh:
            fh.readline()                                   # the reference skips the first line as the file header
            for line in fh:
                if line[:2] == "f ":
                    idx = [int(tok.split("/")[0]) - 1 for tok in line.split(" ")[1:]]
                    if len(idx) != 4:
                        raise ValueError(f"{path}: only quad faces are supported, got {line.strip()!r}")
                    v1, v2, v3, v4 = idx
                    faces += [[v1, v2, v3], [v1, v3, v4]]
                    if p1 is None:
                        p1, p2, p3 = v1, v2, v3
                    elif v2 in (p2, p3) and v3 in (p2, p3):
                        p4, p5 = v3, v4
                    elif v1 in (p2, p3) and v2 in (p2, p3):
                        p4, p5 = v2, v3
                    elif v3 in (p2, p3) and v4 in (p2, p3):
                        p4, p5 = v3, v2
                    elif v1 in (p2, p3) and v4 in (p2, p3):
                        p4, p5 = v1, v2
                elif line[:2] == "v ":
                    x = [float(tok) for tok in line.split(" ")[1:]]
                    verts.append([x[0], -x[2], x[1]] if inverse else [x[0], x[1], x[2]])
        if not faces:
            raise ValueError(f"{path}: no faces")
        if p4 is None:
            raise ValueError(f"{path}: no quad shares an edge with the first one; the box frame is undefined")
        v = np.array(verts, dtype=np.float64)
        f = np.array(faces, dtype=np.int64)
        f_v = torch.from_numpy(v[f]).float()
        axes = torch.from_numpy(np.array([v[p3] - v[p2], v[p1] - v[p2], v[p5] - v[p4]])).float()
        origin = torch.from_numpy(np.array([v[p2]])).float()
        center = origin + torch.sum(axes * 0.5, dim=0, keepdim=True)       # (on the CPU, as the reference's own sum)
        return cls(torch.from_numpy(v).float().to(device), torch.from_numpy(f).int().to(device), f_v.to(device),
                   axes.to(device), origin.to(device), center.to(device))


def _faces(mesh, dev):
    f_v = getattr(mesh, "f_v", None)
    if not torch.is_tensor(f_v) or f_v.dtype != torch.float32 or f_v.ndim != 3 or tuple(f_v.shape[1:]) != (3, 3):
        raise TypeError("mesh.f_v: a float32 [F,3,3] tensor expected")
    if f_v.shape[0] < 1:
        raise ValueError("mesh.f_v: the mesh has no faces (F = 0)")
    if f_v.device != dev:
        raise ValueError(f"mesh.f_v is on {f_v.device}, the rays on {dev}")
    return f_v.contiguous()


def _cuda_f32(t, name, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name}: a CUDA tensor expected; there is no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: float32 expected, got {t.dtype}")
    if shape is not None and (t.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape))):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple('*' if s is None else s for s in shape)}")
    return t.contiguous()


def intersect(mesh, rayo, rayd):
    """torchMesh.intersect (bounding.py:101-121) in one launch: rays rayo, rayd [n,3] (CUDA fp32; rayd need not be unit) ->
    (int_p [n,3], int_t [n,1], t_ind [n,1] int64, cond [n,1] bool); int_t = int_p = 0 where the ray misses."""
    rayo = _cuda_f32(rayo, "rayo", (None, 3))
    rayd = _cuda_f32(rayd, "rayd", (rayo.shape[0], 3))
    dev = rayo.device
    if rayd.device != dev:
        raise ValueError("rayo and rayd on different devices")
    f_v = _faces(mesh, dev)
    n = rayo.shape[0]
    int_p = torch.empty((n, 3), device=dev, dtype=torch.float32)
    int_t = torch.empty((n, 1), device=dev, dtype=torch.float32)
    t_ind = torch.empty((n, 1), device=dev, dtype=torch.int64)
    cond = torch.empty((n, 1), device=dev, dtype=torch.uint8)
    if n:
        with torch.cuda.device(dev):
            _check(_lib.lib().mvi_mesh_intersect(_p(rayo), _p(rayd), n, _p(f_v), f_v.shape[0], _p(int_p), _p(int_t), _p(t_ind),
                                                 _p(cond), _stream(dev)), "mvi_mesh_intersect")
    return int_p, int_t, t_ind, cond.view(torch.bool)


def points_inside(mesh, xyz):
    """del.py:104-108: bool [N], True where the rays from xyz [N,3] (CUDA fp32) along +x and -x both hit the mesh."""
    xyz = _cuda_f32(xyz, "xyz", (None, 3))
    dev = xyz.device
    f_v = _faces(mesh, dev)
    out = torch.empty((xyz.shape[0],), device=dev, dtype=torch.uint8)
    if xyz.shape[0]:
        with torch.cuda.device(dev):
            _check(_lib.lib().mvi_mesh_points_inside(_p(xyz), xyz.shape[0], _p(f_v), f_v.shape[0], _p(out), _stream(dev)),
                   "mvi_mesh_points_inside")
    return out.view(torch.bool)


def _per_view(x, V, name):
    vals = x.detach().cpu().double().reshape(-1).tolist() if torch.is_tensor(x) else (
        [float(x)] if np.isscalar(x) else [float(a) for a in x])
    if len(vals) == 1:
        vals = vals * V
    if len(vals) != V:
        raise ValueError(f"{name}: {len(vals)} values for {V} views")
    return vals


def view_masks(mesh, c2w, fovx, fovy, depth, render=None, disparity=False):
    """gen_seq.py:46-52 (and render_depth.py:37) for V views of one size in one launch. c2w [V,4,4] camera-to-world
    (Camera.camera_to_world), fovx / fovy: one value or V values (radians), depth [V,1,H,W], render [V,3,H,W] (optional);
    all tensors CUDA fp32. Returns {"mask": [V,1,H,W] 0/1 floats, "masked": render * (1 - mask) + mask (with render),
    "disparity": 1 / max(depth, 1e-3) (with disparity=True)}. The per-pixel rays are those of scene/helpers.py get_rays."""
    depth = _cuda_f32(depth, "depth", (None, 1, None, None))
    V, _, H, W = depth.shape
    dev = depth.device
    c2w = _cuda_f32(c2w, "c2w", (V, 4, 4))
    if c2w.device != dev:
        raise ValueError("c2w and depth on different devices")
    if render is not None:
        render = _cuda_f32(render, "render", (V, 3, H, W))
        if render.device != dev:
            raise ValueError("render and depth on different devices")
    f_v = _faces(mesh, dev)
    # fov2focal (gs-simp/utils/graphics_utils.py) in double, then fp32 like the reference's tensor / python-float division
    fx = torch.tensor([W / (2 * math.tan(a / 2)) for a in _per_view(fovx, V, "fovx")], dtype=torch.float32, device=dev)
    fy = torch.tensor([H / (2 * math.tan(a / 2)) for a in _per_view(fovy, V, "fovy")], dtype=torch.float32, device=dev)
    out = {"mask": torch.empty((V, 1, H, W), device=dev, dtype=torch.float32)}
    if render is not None:
        out["masked"] = torch.empty((V, 3, H, W), device=dev, dtype=torch.float32)
    if disparity:
        out["disparity"] = torch.empty((V, 1, H, W), device=dev, dtype=torch.float32)
    opt = lambda k: _p(out[k]) if k in out else None
    if V * H * W:
        with torch.cuda.device(dev):
            _check(_lib.lib().mvi_mesh_view_masks(_p(c2w), _p(fx), _p(fy), V, H, W, _p(f_v), f_v.shape[0], _p(depth),
                                                  _p(render) if render is not None else None, _p(out["mask"]), opt("masked"),
                                                  opt("disparity"), _stream(dev)), "mvi_mesh_view_masks")
    return out


def _ply_sh_degree(path):
    """The SH degree of a Gaussian PLY from its header: 3 ((D + 1)^2 - 1) f_rest properties."""
    n_rest = 0
    with open(path, "rb") as fh:
        for raw in fh:
            tok = raw.decode("ascii", "replace").split()
            if tok[:1] == ["end_header"]:
                break
            if tok[:1] == ["property"] and tok[-1].startswith("f_rest_"):
                n_rest += 1
    D = round(math.sqrt(n_rest / 3 + 1)) - 1
    if 3 * ((D + 1) ** 2 - 1) != n_rest:
        raise ValueError(f"{path}: {n_rest} f_rest properties match no SH degree")
    return D


def delete_inside(mesh_path, ply_in, ply_out, device="cuda"):
    """del.py for one scene: drops the Gaussians of ply_in inside the box of mesh_path, writes the rest to ply_out.
    Returns (kept, total)."""
    from . import gaussian_io, train_ops
    mesh = BoxMesh.from_obj(mesh_path, device=device)
    g = gaussian_io.load_ply(ply_in, _ply_sh_degree(ply_in))
    P = g["xyz"].shape[0]
    names = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation")
    ts = [torch.from_numpy(g[k]).to(device) for k in names]
    keep = ~points_inside(mesh, ts[0])
    rows = train_ops.compact_rows(keep, [t.reshape(P, int(np.prod(t.shape[1:]))) for t in ts])
    out = [r.reshape((r.shape[0],) + t.shape[1:]) for r, t in zip(rows, ts)]
    gaussian_io.save_ply(ply_out, *out)
    return out[0].shape[0], P


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m multiview_inpaint_amd.box_region")
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("delete", help="drop the Gaussians inside a box mesh (gs-simp/del.py)")
    d.add_argument("--mesh", required=True, help="box .obj (bds/del/<scene>.obj)")
    d.add_argument("--ply", required=True, help="input point_cloud.ply")
    d.add_argument("--out", required=True, help="output .ply")
    a = ap.parse_args(argv)
    kept, total = delete_inside(a.mesh, a.ply, a.out)
    print(f"[multiview_inpaint_amd] kept {kept} of {total} Gaussians ({total - kept} inside the box) -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

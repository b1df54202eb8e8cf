"""Box-region kernels on the GPU, one JSON line: device-event times (median of --reps after --warmup) of

  * view_masks on one 1920 x 1080 view and on a 14-view 512 x 384 sequence (with render -> masked), and
  * points_inside at 1.5 M points,

each beside a chunked PyTorch restatement of the reference rule (gs-simp/utils/bounding.py, bs = 10 000, last-axis cross
product) on the same GPU, written for timing only. Bounds from shapes: view_masks moves 32 B per pixel (depth and render in,
mask and masked out) and evaluates ~35 fp32 operations per ray and face; points_inside reads 12 B and writes 1 B per point
and evaluates two rays per point. The fraction of the roofline is the larger bound over the measured time.

    python tools/bench_box_region.py [--warmup 5] [--reps 20] [--out profiles/box_region_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import box_region_helpers as H  # noqa: E402
from multiview_inpaint_amd import box_region as B  # noqa: E402

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_VECTOR_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: peak FP32 (vector)
FLOPS_PER_RAY_FACE = 35


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def torch_intersect(f_v, rayo, rayd, bs=10000):
    """bounding.py:62-121 restated (cross over dim=-1), for timing."""
    eps = 1e-8
    rayd = torch.nn.functional.normalize(rayd, p=2, dim=-1)
    e1, e2 = f_v[:, 1] - f_v[:, 0], f_v[:, 2] - f_v[:, 0]
    ts = []
    for st in range(0, rayo.shape[0], bs):
        o, d = rayo[st:st + bs], rayd[st:st + bs]
        n, F = o.shape[0], f_v.shape[0]
        E1, E2, D = e1[None].repeat(n, 1, 1), e2[None].repeat(n, 1, 1), d[:, None].repeat(1, F, 1)
        h = torch.cross(D, E2, dim=-1)
        a = (E1 * h).sum(-1)
        f = 1. / (a + eps)
        s = o[:, None] - f_v[None, :, 0]
        u = f * (s * h).sum(-1)
        q = torch.cross(s, E1, dim=-1)
        v = f * (D * q).sum(-1)
        t = f * (E2 * q).sum(-1)
        bad = ((a > -eps) & (a < eps)) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1) | (t < eps)
        mx, _ = t.max(-1, keepdim=True)
        it, _ = torch.where(bad, mx + 1, t).min(-1, keepdim=True)
        c = (mx + 1 - it) > 0
        ts.append(torch.where(c, it, torch.zeros_like(it)))
    return torch.cat(ts)


def torch_view_masks(f_v, c2w, fx, fy, depth, render):
    V, _, Hh, Ww = depth.shape
    dev = depth.device
    j, i = torch.meshgrid(torch.arange(Hh, device=dev, dtype=torch.float32) + 0.5,
                          torch.arange(Ww, device=dev, dtype=torch.float32) + 0.5, indexing="ij")
    outs = []
    for k in range(V):
        dirs = torch.stack(((i - Ww // 2) / fx[k], (j - Hh // 2) / fy[k], torch.ones_like(i)), -1).reshape(-1, 3)
        rd = dirs @ c2w[k, :3, :3].T
        ro = c2w[k, :3, 3].expand_as(rd)
        t = torch_intersect(f_v, ro, rd).view(1, Hh, Ww)
        m = ((t > 0) & ((t < depth[k]) | (depth[k] == 15.))).float()
        outs.append((m, render[k] * (1. - m) + m))
    return outs


def mask_case(kind, V, Hh, Ww, seed, warmup, reps):
    mesh = B.BoxMesh.from_obj(H.mesh_path(kind), device="cuda")
    f_v = mesh.f_v.cpu().numpy()
    c2w, fovx, fovy = H.cameras(f_v, V, Hh, Ww, seed)
    t = lambda a: torch.from_numpy(a).cuda()
    c2w_d, depth, render = t(c2w), t(H.depth_maps(f_v, V, Hh, Ww, seed + 100)), t(H.renders(V, Hh, Ww, seed + 200))
    us = timed(lambda: B.view_masks(mesh, c2w_d, fovx, fovy, depth, render=render), warmup, reps)
    fx = [Ww / (2 * np.tan(a / 2)) for a in fovx]
    fy = [Hh / (2 * np.tan(a / 2)) for a in fovy]
    us_t = timed(lambda: torch_view_masks(mesh.f_v, c2w_d, fx, fy, depth, render), 2, max(3, reps // 4))
    px, F = V * Hh * Ww, mesh.f_v.shape[0]
    hbm_us = 32.0 * px / (HBM_PEAK_GBS * 1e3)
    valu_us = FLOPS_PER_RAY_FACE * F * px / (FP32_VECTOR_PEAK_TFLOPS * 1e6)
    bound = max(hbm_us, valu_us)
    return dict(views=V, height=Hh, width=Ww, faces=F, us=round(us, 2), torch_chunked_us=round(us_t, 1),
                speedup=round(us_t / us, 1), hbm_bound_us=round(hbm_us, 2), valu_bound_us=round(valu_us, 2),
                binds="hbm" if hbm_us >= valu_us else "valu", fraction_of_roofline=round(bound / us, 3),
                hbm_fraction=round(hbm_us / us, 3), gpix_per_s=round(px / us / 1e3, 2))


def points_case(warmup, reps):
    mesh = B.BoxMesh.from_obj(H.mesh_path("del"), device="cuda")
    xyz = torch.from_numpy(H.del_points(mesh.f_v.cpu().numpy(), H.N_POINTS, H.POINTS_SEED)).cuda()
    us = timed(lambda: B.points_inside(mesh, xyz), warmup, reps)
    pos = torch.tensor([[1., 0., 0.]], device="cuda").repeat(H.N_POINTS, 1)

    def ref():
        a = torch_intersect(mesh.f_v, xyz, pos)
        b = torch_intersect(mesh.f_v, xyz, -pos)
        return ((a > 0) & (b > 0))[..., 0]
    us_t = timed(ref, 1, 3)
    F = mesh.f_v.shape[0]
    hbm_us = 13.0 * H.N_POINTS / (HBM_PEAK_GBS * 1e3)
    valu_us = 2 * FLOPS_PER_RAY_FACE * F * H.N_POINTS / (FP32_VECTOR_PEAK_TFLOPS * 1e6)
    return dict(points=H.N_POINTS, faces=F, us=round(us, 2), torch_chunked_us=round(us_t, 1), speedup=round(us_t / us, 1),
                hbm_bound_us=round(hbm_us, 2), valu_bound_us=round(valu_us, 2), binds="hbm" if hbm_us >= valu_us else "valu",
                fraction_of_roofline=round(max(hbm_us, valu_us) / us, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_region needs a GPU")
    res = {"metric": "box_region", "device": torch.cuda.get_device_name(0),
           "view_masks_1080p": mask_case("big", 1, H.HD_H, H.HD_W, 22, a.warmup, a.reps),
           "view_masks_seq14_512x384": mask_case("add", 14, H.SEQ_H, H.SEQ_W, 21, a.warmup, a.reps),
           "points_inside_1p5m": points_case(a.warmup, a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Seeded inputs of the box-region tests (tests/test_box_region_*.py) and of their golden generator
(tools/gen_golden_box_region.py): rays, points, cameras, depth maps and renders are regenerated from seeds here, so the
fixtures under tests/golden/box_region/ hold outputs only. numpy only; every array is float32 unless stated."""
import gzip
import math
import os
import tempfile

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_region")
# the shipped boxes: one of gen_seq.py's `add` boxes, one of del.py's `del` boxes, one `add` box whose .obj lists 10 008 vertices
# (10 000 of them used by no face); that one is kept gzip-compressed, byte for byte, and unpacked on first use
MESHES = {"add": "garden_cake.obj", "del": "garden.obj", "big": "counter_bread.obj.gz"}
SEQ_VIEWS, SEQ_H, SEQ_W = 3, 512, 384          # gen_seq's sequence size (Camera.update_attr: 384 wide, 512 high)
HD_H, HD_W = 1080, 1920
N_POINTS = 1_500_000                           # del.py on a 1.5 M-Gaussian scene
N_PLY = 20_011                                 # the delete CLI's seeded scene (n % 10000 != 3)
RAY_SEEDS = {"add": 100, "del": 101, "big": 102}
POINTS_SEED, PLY_SEED = 7, 13
# mask sets: name -> (mesh, views, H, W, seed of the cameras; the depth maps use seed + 100, the renders seed + 200)
MASK_SETS = {"seq": ("add", SEQ_VIEWS, SEQ_H, SEQ_W, 21), "hd": ("big", 1, HD_H, HD_W, 22)}
DEPTH_SENTINEL = 15.0                          # the renderer's empty-pixel depth that gen_seq.py:49 tests for


_UNPACKED = {}


def stored_mesh_path(kind):
    return os.path.join(GOLDEN, MESHES[kind])


def mesh_path(kind):
    """A readable .obj of the box `kind` (a compressed fixture is unpacked once per process into a temporary directory)."""
    src = stored_mesh_path(kind)
    if not src.endswith(".gz"):
        return src
    if kind not in _UNPACKED:
        dst = os.path.join(tempfile.mkdtemp(prefix="mvi_box_"), os.path.basename(src)[:-3])
        with gzip.open(src, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
        _UNPACKED[kind] = dst
    return _UNPACKED[kind]


def golden_path(name):
    return os.path.join(GOLDEN, name)


def bounds(f_v):
    p = f_v.reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    return lo, hi, (lo + hi) / 2, float(np.linalg.norm(hi - lo))


def ray_sets(f_v, seed):
    """{name: (o [n,3], d [n,3])}: the random and targeted sets (margin-checked) and the adversarial rays (exact)."""
    rng = np.random.default_rng(seed)
    lo, hi, c, diag = bounds(f_v)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    sets = {}
    n = 20_011
    o = c + (rng.random((n, 3)) - 0.5) * (hi - lo) * 3.0                # around and inside the box
    sets["random"] = (f32(o), f32(rng.normal(size=(n, 3))))
    n = 6_007
    tri = rng.integers(0, f_v.shape[0], n)
    w = rng.dirichlet((2.0, 2.0, 2.0), n)
    target = np.einsum("nk,nkc->nc", w, f_v[tri].astype(np.float64))    # points well inside the faces
    o = c + rng.normal(size=(n, 3)) * diag * 1.5
    sets["face_aimed"] = (f32(o), f32((target - o) * rng.uniform(0.2, 5.0, (n, 1))))
    n = 5_001
    o = c + (rng.random((n, 3)) - 0.5) * (hi - lo) * 1.6
    d = np.zeros((n, 3))
    d[:, 0] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    sets["pm_x"] = (f32(o), f32(d))
    v0 = f_v[0, 0].astype(np.float64)
    e1 = (f_v[0, 1] - f_v[0, 0]).astype(np.float64)
    out = c + (v0 - c) * 2.0
    far = np.array([c[0], c[1], c[2] + 3e7])                            # exact in fp32 but for z: the ray meets the box
    adv_o = [c, c + (hi - lo) * 2.0, out, far, c]
    adv_d = [np.zeros(3), np.zeros(3), e1, np.array([0.0, 0.0, -1.0]), np.array([0.0, 0.0, 1e-30])]
    sets["adversarial"] = (f32(adv_o), f32(adv_d))
    return sets


def del_points(f_v, n, seed):
    """A del-style cloud: half of it Gaussian around the box (a fair share inside), half uniform over a larger scene."""
    rng = np.random.default_rng(seed)
    lo, hi, c, diag = bounds(f_v)
    k = n // 2
    a = c + rng.normal(size=(k, 3)) * (hi - lo) * 0.6
    b = c + (rng.random((n - k, 3)) - 0.5) * diag * 4.0
    p = np.concatenate([a, b])[rng.permutation(n)]
    return np.ascontiguousarray(p, dtype=np.float32)


def cameras(f_v, V, H, W, seed):
    """V cameras looking at the box from around it: c2w [V,4,4] (camera-to-world, x right, y down, z forward — the
    convention of Camera.camera_to_world), fovx, fovy [V] (radians, float64)."""
    rng = np.random.default_rng(seed)
    lo, hi, c, diag = bounds(f_v)
    c2w = np.zeros((V, 4, 4))
    fovx = rng.uniform(0.6, 1.1, V)
    fovy = 2 * np.arctan(np.tan(fovx / 2) * H / W)
    for k in range(V):
        az, el = rng.uniform(0, 2 * math.pi), rng.uniform(-0.5, 0.8)
        pos = c + diag * rng.uniform(1.2, 2.0) * np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), math.sin(el)])
        fwd = c + rng.normal(size=3) * diag * 0.1 - pos
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        c2w[k, :3, 0], c2w[k, :3, 1], c2w[k, :3, 2], c2w[k, :3, 3], c2w[k, 3, 3] = right, down, fwd, pos, 1.0
    return np.ascontiguousarray(c2w, dtype=np.float32), fovx, fovy


def depth_maps(f_v, V, H, W, seed):
    """[V,1,H,W]: a smooth field around the camera-to-box distance (so t < depth flips inside the box's footprint), with
    rectangles of the 15.0 sentinel."""
    rng = np.random.default_rng(seed)
    lo, hi, c, diag = bounds(f_v)
    y, x = np.mgrid[0:H, 0:W] / max(H, W)
    out = np.empty((V, 1, H, W))
    for k in range(V):
        f = np.zeros((H, W))
        for _ in range(4):
            kx, ky, ph = rng.uniform(2, 9), rng.uniform(2, 9), rng.uniform(0, 2 * math.pi)
            f += np.sin(kx * x + ky * y + ph)
        f = diag * (1.6 + 0.35 * f / 4)
        for _ in range(3):
            h0, w0 = rng.integers(0, H - H // 4), rng.integers(0, W - W // 4)
            f[h0:h0 + rng.integers(H // 16, H // 4), w0:w0 + rng.integers(W // 16, W // 4)] = DEPTH_SENTINEL
        out[k, 0] = f
    return np.ascontiguousarray(out, dtype=np.float32)


def renders(V, H, W, seed):
    return np.random.default_rng(seed).random((V, 3, H, W), dtype=np.float32)


def ply_gaussians(f_v, n, seed):
    """An SH-degree-0 Gaussian scene (the only kind del.py reads) in the model layouts of gaussian_io.load_ply."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(xyz=del_points(f_v, n, seed), features_dc=f32(rng.normal(size=(n, 1, 3))), features_rest=np.zeros((n, 0, 3), np.float32),
                opacity=f32(rng.normal(size=(n, 1))), scaling=f32(rng.normal(size=(n, 3)) - 4), rotation=f32(rng.normal(size=(n, 4))))


def unpack(bits, n):
    return np.unpackbits(bits, count=n).astype(bool)

"""Binning version 2 (csrc/raster_binning2.hip) where its loads are clamped instead of branched around, and the tile ids that
are derived from the tile ranges on demand (mvi_raster_materialize_tile_ids) instead of being stored by pass 2.

Every kernel of the binning loads its items through an index clamped into the array and drops what a lane past the end
loaded, so the lanes that matter sit at the ends: the last lane, wave, depth-sort tile (2048 keys) and pass-1 block (2048
Gaussians) of a scene, an empty chunk whose first segment is the segment total (an empty LAST tile column), blocks that see
only culled Gaussians, and a scene with no pair at all. Each case compares version 2 with version 1 bit for bit (D, radii,
point list, tile ids, ranges), checks the binning properties and that two runs of version 2 agree. sh_degree 0 throughout."""
import numpy as np
import pytest
import torch

from multiview_inpaint_amd import synthetic as syn
from raster_helpers import oracle_params, small_scene

pytestmark = pytest.mark.gpu

CHUNK2, CAP_SMALL = 1536, 7168      # kEx2Chunk, kEx2SmallCap (csrc/raster_common.h)


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


def _settings(R, cam, bg=None):
    d = "cuda"
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.zeros(3, device=d) if bg is None else torch.tensor(bg, device=d), scale_modifier=1.0,
        viewmatrix=torch.tensor(cam["viewmatrix"], device=d), projmatrix=torch.tensor(cam["projmatrix"], device=d),
        sh_degree=0, campos=torch.tensor(cam["campos"], device=d), prefiltered=False)


def _tiles(cam):
    return (cam["W"] + 15) // 16, (cam["H"] + 15) // 16


def _binning(R, cam, t, version):
    from multiview_inpaint_amd import _lib
    L = _lib.lib()
    prev = L.mvi_raster_binning_version(version)
    try:
        gx, gy = _tiles(cam)
        _, radii, _, st = R.rasterize_forward(_settings(R, cam), t["means3D"], t["opacities"], shs=t["shs"],
                                              scales=t["scales"], rotations=t["rotations"])
        out = dict(D=st.D, radii=radii.clone(), plist=st.tensor("point_list", (st.D,), torch.int32).clone(),
                   tids=st.tensor("tile_ids_sorted", (st.D,), torch.int32).clone(),
                   ranges=st.tensor("ranges", (gx * gy, 2), torch.int32).clone())
        torch.cuda.synchronize()
        return out, st
    finally:
        L.mvi_raster_binning_version(prev)


def _properties(st, radii, cam):
    P, D = st.P, st.D
    gx, gy = _tiles(cam)
    plist = st.tensor("point_list", (D,), torch.int32).long()
    tt = st.tensor("tiles_touched", (P,), torch.int32).long()
    depths = st.tensor("depths", (P,), torch.float32)
    tids = st.tensor("tile_ids_sorted", (D,), torch.int32).long()
    keys = (tids << 32) | (depths[plist].view(torch.int32).long() & 0xFFFFFFFF)
    assert (keys[1:] >= keys[:-1]).all()                                   # sorted by (tile, depth bits)
    assert D == int(tt.sum()) and ((radii > 0) == (tt > 0)).all()
    assert torch.equal(torch.bincount(plist, minlength=P), tt)
    same = keys[1:] == keys[:-1]
    assert (plist[1:][same] > plist[:-1][same]).all()                      # stable: ties in Gaussian order
    ranges = st.tensor("ranges", (gx * gy, 2), torch.int32).long()
    cnt = torch.bincount(keys >> 32, minlength=gx * gy)
    assert torch.equal(ranges[:, 1] - ranges[:, 0], cnt)
    nz = cnt > 0
    assert torch.equal(ranges[nz, 0], (torch.cumsum(cnt, 0) - cnt)[nz])   # a tile's pairs start where the earlier tiles' end


def _check(R, cam, sc):
    """Version 2 twice and version 1 once on one scene; returns version 2's outputs."""
    t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}
    a, st2 = _binning(R, cam, t, 2)
    a2, _ = _binning(R, cam, t, 2)
    b, _ = _binning(R, cam, t, 1)
    assert a["D"] == b["D"] == a2["D"]
    for k in ("radii", "plist", "tids", "ranges"):
        assert torch.equal(a[k], b[k]), f"{k}: version 2 differs from version 1"
        assert torch.equal(a[k], a2[k]), f"{k}: two runs of version 2 differ"
    if a["D"]:
        _properties(st2, a["radii"], cam)
    return a, st2


@pytest.mark.parametrize("P", [1, 63, 65, 2047, 2048, 2049, 4097, 262_145, 2_097_153])
def test_scene_ends_inside_a_lane_wave_tile_block(R, P):
    """96 x 64: the scene ends one short of, at and one past a wave (64), a depth-sort tile and a pass-1 block (2048).
    P = 262 145 is the first at which version 1's row of block sums (one per 256 Gaussians) has a second 1024-value scan
    round, of one element; P = 2 097 153 the same for version 2's column table (one entry per 2048 Gaussians)."""
    cam = syn.make_camera(96, 64, 50.0)
    sc = syn.make_scene(P, cam, 0, seed=31, log_scale_mean=np.log(0.05))
    a, _ = _check(R, cam, sc)
    if P >= 63:
        assert a["D"] > 0, "the case bins nothing"


def test_empty_outer_tile_columns(R):
    """About 400 Gaussians in the middle third of a 320 x 64 image (20 tile columns): the outer columns, the LAST one
    included, are empty, and the last column's one empty chunk starts at the segment total."""
    cam = syn.make_camera(320, 64, 50.0)
    sc = syn.make_scene(400, cam, 0, seed=32)
    m = sc["means3D"].copy()
    m[:, 0] *= 0.3                                  # the camera sits at the origin and looks along z: x is image x
    sc["means3D"] = m
    a, _ = _check(R, cam, sc)
    gx, gy = _tiles(cam)
    per_col = (a["ranges"][:, 1] - a["ranges"][:, 0]).reshape(gy, gx).sum(0).cpu().numpy()
    assert a["D"] > 0 and per_col[gx - 1] == 0 and per_col[0] == 0, per_col
    assert (per_col[:5] == 0).all() and (per_col[-5:] == 0).all() and per_col[gx // 2] > 0, per_col


def test_far_half_behind_the_camera(R):
    """P = 3000, the second half of the Gaussians behind the camera: the tail of the depth order is culled keys, the last
    depth-sort tile and pass-1 block see only empty rectangles."""
    cam = syn.make_camera(96, 64, 50.0)
    sc = syn.make_scene(3000, cam, 0, seed=33, log_scale_mean=np.log(0.05))
    m = sc["means3D"].copy()
    m[1500:, 2] *= -1.0
    sc["means3D"] = m
    a, _ = _check(R, cam, sc)
    assert a["D"] > 0 and int((a["radii"][1500:] > 0).sum()) == 0 and int((a["radii"][:1500] > 0).sum()) > 0


def test_every_gaussian_culled(R):
    """Nothing in front of the camera: D = 0, every range (0, 0), and reading the tile ids of no pair works."""
    cam = syn.make_camera(96, 64, 50.0)
    sc = syn.make_scene(500, cam, 0, seed=34)
    m = sc["means3D"].copy()
    m[:, 2] *= -1.0
    sc["means3D"] = m
    a, st = _check(R, cam, sc)
    assert a["D"] == 0 and a["tids"].numel() == 0 and a["plist"].numel() == 0
    assert int(a["ranges"].abs().sum()) == 0 and int((a["radii"] != 0).sum()) == 0
    assert st.tensor("tile_ids_sorted", (0,), torch.int32).numel() == 0


@pytest.mark.parametrize("H", [1296, 2064])
def test_tall_instantiations(R, H):
    """16 x 1296 (81 tile rows: the 128-bin kernel) and 16 x 2064 (129 rows: the 256-bin kernel), 50 Gaussians."""
    cam = syn.make_camera(16, H, 50.0)
    sc = syn.make_scene(50, cam, 0, seed=35, log_scale_mean=np.log(0.1))
    a, _ = _check(R, cam, sc)
    assert a["D"] > 0


def test_chunk_overflows_the_small_image(R):
    """80 tile rows, splats as large as the image: a chunk's pairs do not fit the 7168-entry image of the small
    instantiation and leave in groups of rounds. 48 x 1280 = 3 tile columns; with at most 1536 visible Gaussians every column
    is ONE chunk, whose pair count is the column's: asserted to exceed the image."""
    cam = syn.make_camera(48, 1280, 50.0)
    sc = syn.make_scene(150, cam, 0, seed=36, log_scale_mean=np.log(0.4))
    a, _ = _check(R, cam, sc)
    gx, gy = _tiles(cam)
    assert gy == 80 and int((a["radii"] > 0).sum()) <= CHUNK2
    per_col = (a["ranges"][:, 1] - a["ranges"][:, 0]).reshape(gy, gx).sum(0).cpu().numpy()
    print("pairs per column (= per chunk):", per_col, "image entries:", CAP_SMALL)
    assert per_col.max() > CAP_SMALL, "total > CAP no longer holds: the case does not take the overflow path"


# ---- tile ids on demand --------------------------------------------------------------------------------------------------
def test_tile_ids_read_twice_and_nothing_else_moves(R):
    cam = syn.make_camera(96, 64, 50.0)
    sc = syn.make_scene(2049, cam, 0, seed=37, log_scale_mean=np.log(0.05))
    t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}
    _, _, _, st = R.rasterize_forward(_settings(R, cam), t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"],
                                      rotations=t["rotations"])
    gx, gy = _tiles(cam)
    D = st.D
    assert D > 0
    plist0 = st.tensor("point_list", (D,), torch.int32).clone()
    ranges0 = st.tensor("ranges", (gx * gy, 2), torch.int32).clone()
    t1 = st.tensor("tile_ids_sorted", (D,), torch.int32).clone()
    t2 = st.tensor("tile_ids_sorted", (D,), torch.int32).clone()
    assert torch.equal(t1, t2)
    assert torch.equal(plist0, st.tensor("point_list", (D,), torch.int32))
    assert torch.equal(ranges0, st.tensor("ranges", (gx * gy, 2), torch.int32))
    r = ranges0.long()
    want = torch.repeat_interleave(torch.arange(gx * gy, device="cuda"), r[:, 1] - r[:, 0])
    assert torch.equal(t1.long(), want)             # ranges are in tile order: pair i belongs to the tile whose range holds i


RTOL, GRAD_FLOOR = 1e-4, 1e-2                       # the elementwise rule of tests/test_render_backward_reduce_gpu.py


def test_backward_after_reading_tile_ids(R):
    """A backward behind the call that derives the tile ids against oracle/raster_oracle.c, within the tolerance a backward
    without the call is held to (|got - ref| <= 1e-4 max(|ref|, 1e-2 max|ref|)); both are run."""
    from oracle import raster_oracle as ro
    W, H, N = 40, 36, 80
    cam, sc, bg = small_scene(11, N=N, W=W, H=H, deg=0, log_scale=np.log(0.15))
    p = oracle_params(ro, cam, sc, bg)
    okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
    g_img = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
    ref = ro.backward(p, f, g_img, sc["means3D"], **okw)
    t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}
    rs = _settings(R, cam, bg)
    gkw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    for read_ids in (False, True):
        _, _, _, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
        if read_ids:
            tids = st.tensor("tile_ids_sorted", (st.D,), torch.int32).cpu().numpy().astype(np.uint64)
            assert np.array_equal(tids, f["keys_sorted"] >> np.uint64(32))
        g = R.rasterize_backward(rs, st, torch.tensor(g_img, device="cuda"), t["means3D"], **gkw)
        torch.cuda.synchronize()
        worst = {}
        for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
            got, want = g[k].cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
            assert got.shape == want.shape and np.abs(want).max() > 0, k
            tol = RTOL * np.maximum(np.abs(want), GRAD_FLOOR * np.abs(want).max())
            worst[k] = float((np.abs(got - want) / tol).max())
        print(f"tile ids read: {read_ids}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
        assert all(v <= 1.0 for v in worst.values()), (read_ids, worst)

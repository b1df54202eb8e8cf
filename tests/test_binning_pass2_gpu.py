"""Pass 2 of binning version 2 (csrc/raster_binning2.hip, expand_scatter_kernel) at the boundaries of its instantiations:
images of at most 80 tile rows take the small-LDS kernel (NB 80, 1536-segment chunks, a 7168-entry image), taller ones the
128- and 256-bin kernels. Version 2 against version 1 bit for bit (point list, tile ids, ranges), the binning properties, and
the same inputs twice giving the same outputs."""
import numpy as np
import pytest
import torch

from multiview_inpaint_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


def _settings(R, cam):
    d = "cuda"
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.zeros(3, device=d), scale_modifier=1.0,
        viewmatrix=torch.tensor(cam["viewmatrix"], device=d), projmatrix=torch.tensor(cam["projmatrix"], device=d),
        sh_degree=0, campos=torch.tensor(cam["campos"], device=d), prefiltered=False)


def _binning(R, cam, t, version):
    from multiview_inpaint_amd import _lib
    L = _lib.lib()
    prev = L.mvi_raster_binning_version(version)
    try:
        W, H = cam["W"], cam["H"]
        _, radii, _, st = R.rasterize_forward(_settings(R, cam), t["means3D"], t["opacities"], shs=t["shs"],
                                              scales=t["scales"], rotations=t["rotations"])
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        out = dict(D=st.D, radii=radii.clone(), plist=st.tensor("point_list", (st.D,), torch.int32).clone(),
                   tids=st.tensor("tile_ids_sorted", (st.D,), torch.int32).clone(),
                   ranges=st.tensor("ranges", (tiles, 2), torch.int32).clone())
        torch.cuda.synchronize()
        return out, st
    finally:
        L.mvi_raster_binning_version(prev)


def _properties(st, radii, W, H):
    P, D = st.P, st.D
    plist = st.tensor("point_list", (D,), torch.int32).long()
    tt = st.tensor("tiles_touched", (P,), torch.int32).long()
    depths = st.tensor("depths", (P,), torch.float32)
    tids = st.tensor("tile_ids_sorted", (D,), torch.int32).long()
    keys = (tids << 32) | (depths[plist].view(torch.int32).long() & 0xFFFFFFFF)
    assert (keys[1:] >= keys[:-1]).all()
    assert D == int(tt.sum()) and ((radii > 0) == (tt > 0)).all()
    assert torch.equal(torch.bincount(plist, minlength=P), tt)
    same = keys[1:] == keys[:-1]
    assert (plist[1:][same] > plist[:-1][same]).all()
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    ranges = st.tensor("ranges", (tiles, 2), torch.int32).long()
    cnt = torch.bincount(keys >> 32, minlength=tiles)
    assert torch.equal(ranges[:, 1] - ranges[:, 0], cnt)


@pytest.mark.parametrize("N,W,H,log_scale,squeeze", [
    (300_000, 1024, 1280, None, None),          # 80 tile rows: the small kernel with every bin in use
    (300_000, 1024, 1281, None, None),          # 81 tile rows: the 128-bin kernel
    (20_000, 640, 1280, np.log(0.4), None),     # huge footprints at 80 rows: chunks overflow the 7168-entry image
    (50_000, 1280, 1280, None, "row"),          # every Gaussian in one tile row: one bin holds every entry of the chunk
    (1_536 * 5 + 7, 320, 1276, np.log(0.3), None),   # whole chunks plus a few segments, a ragged last tile row
    (3, 16, 1280, np.log(0.3), None)])          # one tile column, 80 rows, a handful of Gaussians
def test_pass2_instantiations_equal_version_1(R, N, W, H, log_scale, squeeze):
    cam = syn.make_camera(W, H, 50.0)
    kw = {} if log_scale is None else dict(log_scale_mean=log_scale)
    sc = syn.make_scene(N, cam, 0, seed=21, **kw)
    if squeeze == "row":
        m = sc["means3D"].copy()
        m[:, 1] *= 0.004
        sc["means3D"] = m
    t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}
    a, st2 = _binning(R, cam, t, 2)
    a2, _ = _binning(R, cam, t, 2)
    b, _ = _binning(R, cam, t, 1)
    assert a["D"] == b["D"] == a2["D"]
    for k in ("radii", "plist", "tids", "ranges"):
        assert torch.equal(a[k], b[k]), f"{k}: version 2 differs from version 1"
        assert torch.equal(a[k], a2[k]), f"{k}: two runs of version 2 differ"
    if a["D"]:
        a, st2 = _binning(R, cam, t, 2)
        _properties(st2, a["radii"], W, H)

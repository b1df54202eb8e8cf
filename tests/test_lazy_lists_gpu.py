"""Tile lists expanded on demand (include/mvi_raster.h, mvi_raster_list_expansion; csrc/raster_render.hip, LAZY;
csrc/raster_render_shared.h, lazy_list_step). Under mode 1 pass 2 of the binning stops behind its row scan, whose last block
writes the tile ranges; the render kernel finds the entries of a round by walking the column segments of its tile column
that cover its tile row and stores the Gaussians of the rounds it staged into the point list; mark_front finds the leading
entries of its sampled tiles by the same walk. Mode 0 is the pass-2 scatter that writes every list in full.

What can break: an entry dropped or taken twice where a sub-step of the walk holds entries of two rounds; a column whose first
segment is odd (the walk reads two segments per 4-byte word); a long stretch of a column without an entry of the row; a round
that ends with the column; ranges that differ from the scatter's; a stored prefix shorter than what the backward, the aux
backward, the splat and the lift replay; a materialised list that is not the scatter's.

Every comparison of integers and of forward outputs is bit for bit. Gradients and lift sums behind a lazy forward are held
against those behind an eager forward of the same inputs: bit for bit where every Gaussian lies in one tile (no sum depends
on an order), elsewhere |lazy - eager| <= 1e-4 max(|eager|, 1e-2 max|eager|), the bar of tests/test_render_backward_reduce_gpu.py."""
import numpy as np
import pytest
import torch

from raster_helpers import oracle_params, small_scene

pytestmark = pytest.mark.gpu
RTOL, GRAD_FLOOR = 1e-4, 1e-2                           # tests/test_render_backward_reduce_gpu.py


@pytest.fixture(scope="module")
def R():
    from multiview_inpaint_amd import raster
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return raster


@pytest.fixture(scope="module")
def ro():
    from oracle import raster_oracle
    return raster_oracle


@pytest.fixture()
def select():
    """select(mode) / select.binning(version); what the test found is put back afterwards."""
    from multiview_inpaint_amd import _lib
    L = _lib.lib()
    start, version = L.mvi_raster_list_expansion(-1), L.mvi_raster_binning_version(0)

    def mode(v):
        assert L.mvi_raster_list_expansion(v) in (0, 1)
        assert L.mvi_raster_list_expansion(-1) == v
    mode.binning = lambda v: L.mvi_raster_binning_version(v)
    yield mode
    L.mvi_raster_list_expansion(start)
    L.mvi_raster_binning_version(version)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
# Hand-placed, 144 x 80 = 9 x 5 tiles. Identity pose, 90 degree vertical field of view: the focal length is H / 2 = 40 pixels on
# both axes. A group is K isotropic Gaussians (cov3D_precomp = diag(s, s, 0): 2-D variance (40 / z)^2 s + 0.3) on one pixel
# position, at depths z0 + i dz: the depth order is the order of z. Variance 3.6 -> radius ceil(3 * 1.9) = 6 px; around pixel
# 7.75 of a tile that is the one tile, around (7.75, 15.75) the tile and the one below. Variance 175 -> radius 40 px: around
# (103.75, 40) the rectangle is columns 3..8 x rows 0..4.
#   column 0   4515 segments (more than two steps of 2048), every one a single row. Row 0 holds the first 8 and the last 6 of
#              them, the 4501 between lie in rows 1..4: the walk of tile (0, 0) crosses two whole steps without an entry.
#              Opacity 0.01: no tile of the column saturates (a pixel two off the centre keeps T = 0.9935^1126 = 6e-4), so
#              tile (0, 0) is walked to the column's end and the tiles below through the five rounds of their 1125 or 1126 entries.
#   column 1   starts at segment 4515, an odd number. 600 single-row segments in row 2 (three rounds, never saturated:
#              0.99^600 = 2.4e-3), 20 segments over rows 3..4; rows 0 and 1 are empty tiles.
#   column 2   empty.
#   columns 3..8   40 segments over all five rows each; column 8 holds nothing else: every segment covers every row.
#   columns 4..7   300 segments over rows 0..3 in front of everything (variance 60 -> radius 24 px around (103.75, 39.75),
#              opacity 0.9): every pixel of tile (2, 6) sees alpha >= 0.33 and saturates within its first round, the second
#              round of its 340 entries is never looked at. Column 4 also holds 50 single-row segments in row 1.
W144, H80 = 144, 80
GROUPS = [  # K, px, py, variance, opacity, z0, dz
    (8, 7.75, 7.75, 3.6, 0.01, 2.0, 1e-4),
    (4501, 7.75, None, 3.6, 0.01, 2.01, 1e-5),          # py: rows 1..4 in turn
    (6, 7.75, 7.75, 3.6, 0.01, 2.1, 1e-4),
    (600, 23.75, 39.75, 3.6, 0.01, 2.2, 1e-4),
    (20, 23.75, 63.75, 3.6, 0.3, 2.3, 1e-4),
    (50, 71.75, 23.75, 3.6, 0.9, 1.5, 1e-3),
    (40, 103.75, 40.0, 175.0, 0.05, 3.0, 1e-3),
    (300, 103.75, 39.75, 60.0, 0.9, 1.0, 1e-3),
]
# every Gaussian in ONE tile (the bit-exact partner): the single-row groups only
GROUPS_ONE_TILE = [g for g in GROUPS if g[3] < 10 and g[2] != 63.75]


def _placed_scene(groups):
    from multiview_inpaint_amd import synthetic as syn
    W, H = W144, H80
    cam = syn.make_camera(W, H, 90.0)
    px, py, z, var, op = [], [], [], [], []
    for K, x, y, v, o, z0, dz in groups:
        i = np.arange(K)
        px.append(np.full(K, x)); py.append(np.full(K, y) if y is not None else 16.0 * (1 + i % 4) + 7.75)
        z.append(z0 + dz * i); var.append(np.full(K, v)); op.append(np.full(K, o))
    px, py, z, var, op = (np.concatenate(a) for a in (px, py, z, var, op))
    s = (var - 0.3) * (z / (H / 2)) ** 2
    means = np.stack([((2 * px + 1) / W - 1.0) * cam["tanfovx"] * z, ((2 * py + 1) / H - 1.0) * cam["tanfovy"] * z, z], 1).astype(np.float32)
    cov = np.stack([s, 0 * s, 0 * s, s, 0 * s, 0 * s], 1).astype(np.float32)
    n = len(z)
    shs = np.random.default_rng(5).normal(0, 1.0, (n, 1, 3)).astype(np.float32)
    bg = np.array([0.3, 0.1, 0.7], np.float32)
    return dict(cam=cam, bg=bg, deg=0, means3D=means, opacities=op.astype(np.float32)[:, None], shs=shs, cov3D_precomp=cov)


def _random_scene(W, H):
    cam, sc, bg = small_scene(14, N={17: 80, 48: 300, 80: 700}[W], W=W, H=H, deg=3)
    return dict(cam=cam, bg=bg, deg=3, means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"],
                rotations=sc["rotations"])


_SCENES = {}


def _scene(name):
    """name -> (scene, device tensors), built once"""
    if name not in _SCENES:
        sc = {"placed": lambda: _placed_scene(GROUPS), "one_tile": lambda: _placed_scene(GROUPS_ONE_TILE)}.get(
            name, lambda: _random_scene(*map(int, name.split("x"))))()
        t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k not in ("cam", "bg", "deg")}
        _SCENES[name] = (sc, t)
    return _SCENES[name]


_ORACLE = {}


def _oracle(ro, name):
    """the oracle's forward of a scene, run once"""
    if name not in _ORACLE:
        sc, _ = _scene(name)
        cam = sc["cam"]
        p = ro.make_params(sc["means3D"].shape[0], sc["deg"], sc["shs"].shape[1], cam["W"], cam["H"], cam["tanfovx"], cam["tanfovy"],
                           1.0, cam["viewmatrix"], cam["projmatrix"], cam["campos"], sc["bg"])
        kw = {k: sc[k] for k in ("shs", "scales", "rotations", "cov3D_precomp") if k in sc}
        _ORACLE[name] = ro.forward(p, sc["means3D"], sc["opacities"], **kw)
    return _ORACLE[name]


SCENES = ["17x17", "48x32", "80x48", "placed"]


def _settings(R, sc):
    cam = sc["cam"]
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor(sc["bg"], device="cuda"), scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device="cuda"),
        projmatrix=torch.tensor(cam["projmatrix"], device="cuda"), sh_degree=sc["deg"],
        campos=torch.tensor(cam["campos"], device="cuda"), prefiltered=False)


def _poison():
    """The allocator hands a new forward the blocks an earlier one freed: a list left there by an eager forward of the same
    scene would pass for the prefix a lazy forward has to store. Fill what is cached with 0xFF first."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    x = torch.full((96 << 20,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    del x


def _forward(R, name, **kw):
    sc, t = _scene(name)
    rs = _settings(R, sc)
    gkw = {k: t[k] for k in ("shs", "scales", "rotations", "cov3D_precomp") if k in t}
    color, radii, depth, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw, **kw)
    torch.cuda.synchronize()
    return rs, st, t, gkw, color, depth


def _forward_outputs(st, color, depth):
    """everything the forward leaves that does not depend on the expansion mode, as integer tensors (bit patterns)"""
    tiles = ((st.W + 15) // 16) * ((st.H + 15) // 16)
    bits = lambda x: x.contiguous().view(torch.int32).clone()
    return dict(color=bits(color), depth=bits(depth), final_T=st.tensor("final_T", (st.H, st.W), torch.int32),
                n_contrib=st.tensor("n_contrib", (st.H, st.W), torch.int32), ranges=st.tensor("ranges", (tiles, 2), torch.int32),
                radii=st.radii.clone(), rgbd=st.tensor("rgbd", (st.P, 4), torch.int32), clamped=st.tensor("clamped", (st.P,), torch.uint8),
                front=st.tensor("front", (st.P,), torch.uint8), D=torch.tensor([st.D]))


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def _tile_max(st):
    """[tiles] largest n_contrib of every tile"""
    gx, gy = (st.W + 15) // 16, (st.H + 15) // 16
    nc = np.zeros((gy * 16, gx * 16), np.int64)
    nc[:st.H, :st.W] = st.tensor("n_contrib", (st.H, st.W), torch.int32).cpu().numpy().view(np.uint32)
    return nc.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_lazy_forward_equals_eager(R, select, name):
    select(0)
    _, st, _, _, color, depth = _forward(R, name)
    eager = _forward_outputs(st, color, depth)
    del st
    _poison()
    select(1)
    _, st, _, _, color, depth = _forward(R, name)
    lazy = _forward_outputs(st, color, depth)
    assert int(eager["front"].sum()) > 0 and int(eager["n_contrib"].max()) > 0
    _assert_same(eager, lazy, name)


def test_placed_scene_is_what_it_claims(R, ro, select):
    """The cases the hand-placed scene was built for, read from the oracle's forward and from a lazy forward's n_contrib."""
    f = _oracle(ro, "placed")
    gx = W144 // 16
    length = (f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]).reshape(-1, gx)
    assert length[:, 0].tolist() == [14, 1126, 1125, 1125, 1125]                    # the long sparse column: 4515 segments
    assert length[:, 1].tolist() == [0, 0, 600, 20, 20] and (length[:, 2] == 0).all()  # empty tiles, two rows, the empty column
    assert length[:, 4].tolist() == [340, 390, 340, 340, 40] and length[2, 6] == 340 and (length[:, 8] == 40).all()
    touched = f["tiles_touched"]
    assert set(np.unique(touched).tolist()) == {1, 2, 16, 30}                        # one row, two rows, four rows x 4, all rows x 6
    assert int(touched[:4515].sum()) == 4515 and int(touched[:4515].max()) == 1       # column 1 starts at an odd segment
    select(1)
    st = _forward(R, "placed")[1]
    tmax = _tile_max(st).reshape(-1, gx)
    assert tmax[0, 0] == 14 and tmax[2, 1] == 600 and tmax[1, 0] == 1126             # never saturated: walked to the end
    assert 0 < tmax[2, 6] <= 256                                                     # saturated in the first of two rounds


@pytest.mark.parametrize("name", SCENES)
def test_stored_prefix_and_materialised_list(R, ro, select, name):
    f = _oracle(ro, name)
    want = torch.tensor(f["point_list"].astype(np.int64))
    _poison()
    select(1)
    st = _forward(R, name)[1]
    assert st.D == f["num_rendered"] and st.D > 0
    tiles = ((st.W + 15) // 16) * ((st.H + 15) // 16)
    ranges = st.tensor("ranges", (tiles, 2), torch.int32).cpu().numpy().view(np.uint32)
    assert np.array_equal(ranges, f["ranges"])
    left = st.tensor("point_list", (st.D,), torch.int32, _derive=False).cpu().long() & 0xFFFFFFFF
    tmax = _tile_max(st)
    for t in range(tiles):
        r0, n = int(ranges[t, 0]), int(tmax[t])
        assert n <= int(ranges[t, 1]) - r0
        assert torch.equal(left[r0:r0 + n], want[r0:r0 + n]), (name, "tile", t, "stored prefix", n)
    for again in range(2):
        whole = st.tensor("point_list", (st.D,), torch.int32).cpu().long() & 0xFFFFFFFF
        assert torch.equal(whole, want), (name, "materialised", again, int((whole != want).sum()))
    assert np.array_equal(st.tensor("ranges", (tiles, 2), torch.int32).cpu().numpy().view(np.uint32), f["ranges"])


def test_alternating_modes(R, select):
    """Three forwards in a row whose scratch comes from the blocks the one before freed: lazy, eager, lazy."""
    select(0)
    _, st, _, _, color, depth = _forward(R, "placed")
    want = _forward_outputs(st, color, depth)
    del st
    for m in (1, 0, 1):
        select(m)
        _, st, _, _, color, depth = _forward(R, "placed")
        _assert_same(want, _forward_outputs(st, color, depth), f"mode {m}")
        del st


def test_binning_version_1_stays_eager(R, ro, select):
    """Version 1 under mode 1: the forward writes the whole list itself (read without materialising), and the same outputs."""
    f = _oracle(ro, "48x32")
    select(0)
    _, st, _, _, color, depth = _forward(R, "48x32")
    want = _forward_outputs(st, color, depth)
    del st
    _poison()
    select(1)
    select.binning(1)
    _, st, _, _, color, depth = _forward(R, "48x32")
    left = st.tensor("point_list", (st.D,), torch.int32, _derive=False).cpu().numpy().view(np.uint32)
    assert np.array_equal(left, f["point_list"])
    _assert_same(want, _forward_outputs(st, color, depth), "version 1")
    st.materialize_point_list()                                                       # a no-op there
    assert np.array_equal(st.tensor("point_list", (st.D,), torch.int32).cpu().numpy().view(np.uint32), f["point_list"])


# ---- what replays the list --------------------------------------------------------------------------------------------------------
def _consumers(R, name, seed=3):
    """backward with the aux gradients, splat and lift behind an aux forward of the scene"""
    rs, st, t, gkw, color, depth = _forward(R, name, aux=True, prepare_backward=True)
    rng = np.random.default_rng(seed)
    g_img = torch.tensor(rng.normal(size=(3, st.H, st.W)).astype(np.float32), device="cuda")
    g_d = torch.tensor(rng.normal(size=(1, st.H, st.W)).astype(np.float32), device="cuda")
    g_a = torch.tensor(rng.normal(size=(1, st.H, st.W)).astype(np.float32), device="cuda")
    feats = torch.tensor(rng.normal(size=(st.P, 3)).astype(np.float32), device="cuda")
    wts = torch.tensor(rng.uniform(size=(2, st.H, st.W)).astype(np.float32), device="cuda")

    def run():
        g = R.rasterize_backward(rs, st, g_img, t["means3D"], **gkw, grad_expected_depth=g_d, grad_alpha=g_a)
        out = {"grad_" + k: v.clone() for k, v in g.items() if v is not None}
        out["grad_support"] = st.tensor("grad_support", (st.P,), torch.uint8)
        g = R.rasterize_backward(rs, st, g_img, t["means3D"], **gkw)                  # the colour backward alone
        out.update({"color_grad_" + k: v.clone() for k, v in g.items() if v is not None})
        out["splat"] = R.splat_features(st, feats).clone()
        out["lift"] = R.lift_weights(st, wts).clone()
        torch.cuda.synchronize()
        return out
    return st, run


def _assert_within_bar(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        if ref[k].dtype != torch.float32 or k == "splat":                             # flags; the splat has no atomics
            assert torch.equal(got[k], ref[k]), (what, k)
            continue
        a, b = got[k].double(), ref[k].double()
        assert float(b.abs().max()) > 0, (what, k)
        tol = RTOL * torch.maximum(b.abs(), GRAD_FLOOR * b.abs().max())
        worst = float(((a - b).abs() / tol).max())
        assert worst <= 1.0, (what, k, worst)


def _assert_same_bits(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        x, y = (v.view(torch.int32) if v.dtype == torch.float32 else v for v in (got[k], ref[k]))
        assert torch.equal(x, y), (what, k, int((x != y).sum()))


@pytest.mark.parametrize("name", SCENES + ["one_tile"])
def test_consumers_behind_a_lazy_forward(R, select, name):
    select(0)
    st, run = _consumers(R, name)
    eager = run()
    del st, run
    _poison()
    select(1)
    st, run = _consumers(R, name)
    check = _assert_same_bits if name == "one_tile" else _assert_within_bar
    if name == "one_tile":
        assert (st.tensor("tiles_touched", (st.P,), torch.int32) == 1).all(), "a Gaussian's rectangle is not one tile"
    check(run(), eager, f"{name}: stored prefix")
    st.materialize_point_list()
    check(run(), eager, f"{name}: materialised list")

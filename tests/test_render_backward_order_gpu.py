"""The render backward's tile order (csrc/raster_render.hip; include/mvi_raster.h, mvi_raster_backward_order). The forward
records every tile's work class, min(15, largest n_contrib of the tile // 32), in one queue per (XCD band, class); under order 1
the i-th workgroup of a band takes the i-th tile of the band's queues read from class 15 down, under order 0 the band's i-th
tile. What can break: a tile queued twice, not at all, in another band or another class; counts that are not zero when a
forward starts (a scratch that held another image's queues); a block that takes a tile nobody queued; a backward that reads
queues no forward filled. The tile order itself only permutes float atomics: on a scene whose Gaussians each lie in ONE tile
every gradient is bit-identical under both orders, and against oracle/raster_oracle.c both orders are held to the bar of
tests/test_render_backward_reduce_gpu.py, no element excluded."""
import numpy as np
import pytest
import torch

from raster_helpers import oracle_params, small_scene

pytestmark = pytest.mark.gpu
RTOL, GRAD_FLOOR = 1e-4, 1e-2                           # tests/test_render_backward_reduce_gpu.py
BANDS, CLASSES, CLASS_WIDTH = 8, 16, 32


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
def order():
    """order(v) selects the backward's tile order; the selection the test found is put back afterwards."""
    from multiview_inpaint_amd import _lib
    L = _lib.lib()
    start = L.mvi_raster_backward_order(-1)

    def select(v):
        assert L.mvi_raster_backward_order(v) in (0, 1)
        assert L.mvi_raster_backward_order(-1) == v
    yield select
    L.mvi_raster_backward_order(start)


def _settings(R, cam, bg, deg):
    return R.GaussianRasterizationSettings(
        image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor(bg, device="cuda"), scale_modifier=1.0, viewmatrix=torch.tensor(cam["viewmatrix"], device="cuda"),
        projmatrix=torch.tensor(cam["projmatrix"], device="cuda"), sh_degree=deg, campos=torch.tensor(cam["campos"], device="cuda"),
        prefiltered=False)


def _tile_max_n_contrib(st):
    """[tiles] largest n_contrib of every 16x16 tile, from the state's n_contrib view"""
    W, H = st.W, st.H
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nc = np.zeros((gy * 16, gx * 16), np.int64)
    nc[:H, :W] = st.tensor("n_contrib", (H, W), torch.int32).cpu().numpy().view(np.uint32)
    return nc.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)


def _check_queue(st):
    """Per band: the counts sum to the band's size, the queues read from class 15 down are a permutation of the band's tiles,
    and every tile sits in the class of its largest n_contrib. Returns (tile -> class, tile -> largest n_contrib)."""
    torch.cuda.synchronize()
    tiles = ((st.W + 15) // 16) * ((st.H + 15) // 16)
    q, r = divmod(tiles, BANDS)
    stride = (tiles + BANDS - 1) // BANDS + 1
    count = st.tensor("tile_class_count", (BANDS, CLASSES), torch.int32).cpu().numpy()
    queue = st.tensor("tile_class_queue", (BANDS, CLASSES, stride), torch.int32).cpu().numpy()
    tile_max = _tile_max_n_contrib(st)
    want_class = np.minimum(CLASSES - 1, tile_max // CLASS_WIDTH)
    got_class = np.full(tiles, -1, np.int64)
    for x in range(BANDS):
        first, size = x * q + min(x, r), q + (1 if x < r else 0)          # xcd_band_tile: band x is tiles [first, first + size)
        assert (count[x] >= 0).all() and int(count[x].sum()) == size, (x, count[x].tolist(), size)
        seq = np.concatenate([queue[x, c, :count[x, c]] for c in range(CLASSES - 1, -1, -1)])
        assert sorted(seq.tolist()) == list(range(first, first + size)), (x, seq.tolist())
        for c in range(CLASSES):
            got_class[queue[x, c, :count[x, c]]] = c
    assert np.array_equal(got_class, want_class), (got_class.tolist(), want_class.tolist())
    return got_class, tile_max


# ---- hand-placed Gaussians, each inside ONE tile ---------------------------------------------------------------------------------
# Identity pose, 90 degree vertical field of view: the focal length is H / 2 pixels on both axes. K faint isotropic Gaussians
# sit on the centre of a tile with a 2-D variance of 3.6 px^2 (cov3D_precomp = diag(s, s, 0), variance (H / 2 / z)^2 s + 0.3):
# radius ceil(3 * 1.9) = 6 px around pixel 7.75 of the tile, so the tile rectangle is the one tile, and all K reach the centre
# pixels (alpha = opacity there), so the tile's largest n_contrib is K while T stays above the 1e-4 cut-off (0.99^530 = 5e-3).
W144, H80 = 144, 80
# tile -> K. 45 tiles in bands of 6, 6, 6, 6, 6, 5, 5, 5: tiles 20, 21, 22 share band 3 (classes 6, 1, 2 there, and three empty
# tiles); tile 44 holds more than 512 entries, class 530 // 32 = 16 clamped to 15; every tile not named is empty.
PLACED = {0: 10, 3: 40, 7: 70, 13: 100, 20: 200, 21: 33, 22: 64, 31: 95, 44: 530}


def _placed_scene(ro):
    from multiview_inpaint_amd import synthetic as syn
    W, H = W144, H80
    gx = W // 16
    cam = syn.make_camera(W, H, 90.0)
    px, py, z = [], [], []
    for t, K in PLACED.items():
        i = np.arange(K)
        px.append(np.full(K, (t % gx) * 16 + 7.75)); py.append(np.full(K, (t // gx) * 16 + 7.75)); z.append(2.0 + 0.001 * i + 0.0001 * t)
    px, py, z = np.concatenate(px), np.concatenate(py), np.concatenate(z)
    s = (3.6 - 0.3) * (z / (H / 2)) ** 2
    means = np.stack([((2 * px + 1) / W - 1.0) * cam["tanfovx"] * z, ((2 * py + 1) / H - 1.0) * cam["tanfovy"] * z, z], 1).astype(np.float32)
    cov = np.stack([s, 0 * s, 0 * s, s, 0 * s, 0 * s], 1).astype(np.float32)
    n = len(z)
    shs = np.random.default_rng(5).normal(0, 1.0, (n, 1, 3)).astype(np.float32)
    op = np.full((n, 1), 0.01, np.float32)
    bg = np.array([0.3, 0.1, 0.7], np.float32)
    return cam, bg, means, cov, op, shs


def _forward_placed(R, ro):
    cam, bg, means, cov, op, shs = _placed_scene(ro)
    rs = _settings(R, cam, bg, 0)
    t = dict(means3D=torch.tensor(means, device="cuda"), opacities=torch.tensor(op, device="cuda"))
    gkw = dict(shs=torch.tensor(shs, device="cuda"), cov3D_precomp=torch.tensor(cov, device="cuda"))
    color, radii, depth, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
    return rs, st, t, gkw


def _forward_small(R, W, H, seed=14, N=80):
    cam, sc, bg = small_scene(seed, N=N, W=W, H=H, deg=3)
    rs = _settings(R, cam, bg, 3)
    t = {k: torch.tensor(v, device="cuda") for k, v in sc.items() if k != "sh_degree"}
    gkw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    color, radii, depth, st = R.rasterize_forward(rs, t["means3D"], t["opacities"], **gkw)
    return rs, st, t, gkw, (cam, sc, bg)


def _check_placed_queue(st):
    got_class, tile_max = _check_queue(st)
    assert {t: int(tile_max[t]) for t in PLACED} == PLACED, "a placed tile's largest n_contrib is not its number of Gaussians"
    assert int(tile_max[44]) > 512 and got_class[44] == CLASSES - 1 and 530 // CLASS_WIDTH > CLASSES - 1      # the clamp
    empty = [t for t in range(45) if t not in PLACED]
    assert (tile_max[empty] == 0).all() and (got_class[empty] == 0).all()
    assert len(set(got_class.tolist())) >= 4


# 17x17: 4 tiles, bands 4..7 empty, partial tiles; 48x32: 6 tiles; 80x48: 15 tiles, q = 1, r = 7; 144x80: 45 tiles, q = 5, r = 5
@pytest.mark.parametrize("W,H", [(17, 17), (48, 32), (80, 48)])
def test_queue_is_a_permutation(R, W, H):
    rs, st, t, gkw, _ = _forward_small(R, W, H)
    _check_queue(st)


def test_queue_is_a_permutation_placed(R, ro):
    rs, st, t, gkw = _forward_placed(R, ro)
    _check_placed_queue(st)


def test_stale_state(R, ro):
    """Three forwards in a row in one process: the second and third start from scratch memory that may hold the queues and the
    counts of the one before, for another image size."""
    st = _forward_placed(R, ro)[1]
    _check_placed_queue(st)
    del st
    st = _forward_small(R, 48, 32)[1]
    _check_queue(st)
    del st
    st = _forward_placed(R, ro)[1]
    _check_placed_queue(st)


def _backward(R, rs, st, t, gkw, g_img):
    g = R.rasterize_backward(rs, st, g_img, t["means3D"], **gkw)
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in g.items() if v is not None}
    out["grad_support"] = st.tensor("grad_support", (st.P,), torch.uint8)
    return out


def _assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = (v.view(torch.int32) if v.dtype == torch.float32 else v for v in (a[k], b[k]))
        assert torch.equal(x, y), (what, k, int((x != y).sum()))
        if a[k].dtype == torch.float32:
            assert torch.equal(a[k] == 0, b[k] == 0), (what, k, "zero rows")


def test_bit_exact_partner(R, ro, order):
    """Every Gaussian of the placed scene lies in one tile (asserted), so its accumulation row receives ONE atomic per moment
    and its LDS sums two addends: no sum depends on an order. Order 0, order 1 and order 1 again on the same forward state:
    every gradient array, its zero rows and grad_support bit-identical."""
    rs, st, t, gkw = _forward_placed(R, ro)
    touched = st.tensor("tiles_touched", (st.P,), torch.int32).cpu().numpy()
    assert (touched == 1).all(), "a Gaussian's rectangle is not one tile"
    _check_placed_queue(st)
    g_img = torch.tensor(np.random.default_rng(3).normal(size=(3, H80, W144)).astype(np.float32), device="cuda")
    order(0)
    plain = _backward(R, rs, st, t, gkw, g_img)
    order(1)
    first = _backward(R, rs, st, t, gkw, g_img)
    second = _backward(R, rs, st, t, gkw, g_img)
    assert int(plain["grad_support"].sum()) == st.P and float(plain["means2D"].abs().max()) > 0
    _assert_same_bits(plain, first, "order 0 against order 1")
    _assert_same_bits(first, second, "order 1 twice")


# ---- against the oracle -------------------------------------------------------------------------------------------------------
def _hold_to_oracle(g, ref, what):
    worst = {}
    for k in ("means3D", "means2D", "opacities", "shs", "scales", "rotations"):
        got, want = g[k].cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
        assert got.shape == want.shape, k
        assert np.abs(want).max() > 0, k
        tol = RTOL * np.maximum(np.abs(want), GRAD_FLOOR * np.abs(want).max())
        worst[k] = float((np.abs(got - want) / tol).max())
    print(f"{what}: worst |got - ref| / bar per array:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (what, worst)


_ORACLE = {}


def _oracle_case(R, ro, W, H):
    """(forward state and inputs, oracle gradients, image gradient) of small_scene at W x H, degree 3; the oracle runs once"""
    from multiview_inpaint_amd import _lib
    assert _lib.lib().mvi_raster_color_mode(-1) == 1, "deferred colours are the default"
    rs, st, t, gkw, (cam, sc, bg) = _forward_small(R, W, H, seed=14, N=300 if W > 100 else 80)
    if (W, H) not in _ORACLE:
        p = oracle_params(ro, cam, sc, bg)
        okw = dict(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
        f = ro.forward(p, sc["means3D"], sc["opacities"], **okw)
        g_img = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
        _ORACLE[(W, H)] = (ro.backward(p, f, g_img, sc["means3D"], **okw), g_img)
    ref, g_img = _ORACLE[(W, H)]
    return rs, st, t, gkw, ref, torch.tensor(g_img, device="cuda")


@pytest.mark.parametrize("W,H", [(144, 80), (17, 17)])
def test_backward_against_oracle(R, ro, order, W, H):
    """|got - ref| <= 1e-4 max(|ref|, 1e-2 max|ref|) on every gradient element, under the plain order first (the scene must
    meet the bar there), then heaviest first on the same forward state."""
    rs, st, t, gkw, ref, g_img = _oracle_case(R, ro, W, H)
    _check_queue(st)
    order(0)
    _hold_to_oracle(_backward(R, rs, st, t, gkw, g_img), ref, f"{W}x{H} order 0")
    order(1)
    _hold_to_oracle(_backward(R, rs, st, t, gkw, g_img), ref, f"{W}x{H} order 1")


def test_no_queue_falls_back(R, ro, order):
    """A state whose image scratch no forward of this process rendered into: the forward's scratch copied to another address
    (inside a larger buffer, off the allocator's 512-byte grid, so no earlier state ever lived there), its counts and queues
    overwritten with 0xFF. Under order 1 the backward must take the plain order: it meets the oracle's bar, and a block that
    read the overwritten queues would have been clamped onto the last tile."""
    rs, st, t, gkw, ref, g_img = _oracle_case(R, ro, 144, 80)
    torch.cuda.synchronize()
    v = st.views()
    n = st.image.numel()
    big = torch.empty(n + 512, dtype=torch.uint8, device="cuda")
    copy = big[256:256 + n]
    assert copy.data_ptr() % 512 == 256
    copy.copy_(st.image)
    lo = v.tile_class_count - st.image.data_ptr()
    stride = (45 + BANDS - 1) // BANDS + 1
    copy[lo:lo + 4 * BANDS * CLASSES * (1 + stride)] = 0xFF
    assert v.tile_class_queue - v.tile_class_count == 4 * BANDS * CLASSES
    st.image = copy
    order(1)
    _hold_to_oracle(_backward(R, rs, st, t, gkw, g_img), ref, "144x80 order 1, no queue")

"""Feature splat, the parts that need no GPU: the C entry is bound and checks its arguments on the host; the reference the GPU
tests compare against (the CPU oracle's colors_precomp forward, tests/feature_splat_helpers.py) is the adjoint of the lift's
reference (tests/mask_lift_helpers.py); the argument checks and the normalisation of mask_lift.project_selection."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from feature_splat_helpers import oracle_splat
from mask_lift_helpers import long_list_scene, oracle_lift
from raster_helpers import rel_err, small_scene


def test_the_entry_point_is_bound_and_there_is_no_cpu_path():
    from multiview_inpaint_amd import _lib, raster as R
    L = _lib.lib()                                               # raises if a declared symbol is missing
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = [C.POINTER(_lib.RasterSettings), i32, i64, vp, vp, vp, vp, i32, i32, vp, vp]
    name = "mvi_raster_splat_features"
    assert name in _lib.declared_symbols() and hasattr(L, name)
    fn = getattr(L, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == want
    header = open(_lib.INCLUDE_DIR + "/mvi_raster.h").read()
    decl = header[header.index("int " + name + "("):]
    assert decl[:decl.index(";")].count(",") + 1 == len(want)             # as many parameters as the header declares
    # argument checks run on the host: without settings the entry reports an error and touches no device
    assert fn(None, 0, 0, None, None, None, None, 1, 1, None, None) == -1
    assert b"settings is NULL" in L.mvi_raster_last_error()
    # channels outside 1..8, a row shorter than the channels, no features, no state: errors before anything is launched (the
    # four settings pointers are only checked for NULL on the host)
    s = _lib.RasterSettings()
    s.image_height = s.image_width = 16
    s.tanfovx = s.tanfovy = s.scale_modifier = 1.0
    s.bg = s.viewmatrix = s.projmatrix = s.campos = 64
    for channels, stride, features, what in ((9, 16, 64, b"channels"), (0, 16, 64, b"channels"), (-1, 16, 64, b"channels"),
                                             (3, 2, 64, b"feat_stride"), (2, 16, None, b"features is NULL"),
                                             (2, 16, 64, b"NULL geom/binning/image/out")):
        assert fn(C.byref(s), 4, 7, None, None, None, features, channels, stride, None, None) == -1, what
        assert what in L.mvi_raster_last_error(), (what, L.mvi_raster_last_error())
    for geom, binning, image, out in ((None, 64, 64, 64), (64, None, 64, 64), (64, 64, None, 64), (64, 64, 64, None)):
        assert fn(C.byref(s), 4, 7, geom, binning, image, 64, 2, 16, out, None) == -1
        assert b"NULL geom/binning/image/out" in L.mvi_raster_last_error()
    # P == 0, num_rendered == 0 and an empty image: 0, nothing launched (no device pointer is valid here)
    assert fn(C.byref(s), 0, 7, 64, 64, 64, 64, 2, 16, 64, None) == 0
    assert fn(C.byref(s), 4, 0, 64, 64, 64, 64, 2, 16, 64, None) == 0
    s.image_width = 0
    assert fn(C.byref(s), 4, 7, 64, 64, 64, 64, 2, 16, 64, None) == 0
    assert R.SPLAT_MAX_CHANNELS == 8
    st = R.RasterState()
    st.P, st.D, st.W, st.H, st.geom = 4, 7, 16, 16, torch.empty(0, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.splat_features(st, torch.zeros(4, 3))


_SCENES = {"small": lambda: small_scene(0, N=80, W=40, H=36, deg=1, pose=True)[:2],
           "small_17x9": lambda: small_scene(0, N=80, W=17, H=9, deg=1, pose=True)[:2],
           "long_list": lambda: long_list_scene()[:2]}


@pytest.mark.parametrize("scene", list(_SCENES))
def test_the_reference_is_the_adjoint_of_the_lifts_reference(scene):
    """<splat(F), G> = <F, lift(G)[:, 1:]> with non-negative F [P,8] and G [8,H,W] (no cancellation: the two sides are sums of
    the same non-negative products alpha T F G in another order): 1e-6 relative. The oracle shows 5.1e-8, 7.0e-9 and 6.4e-9 here."""
    cam, sc = _SCENES[scene]()
    P, H, W = sc["means3D"].shape[0], cam["H"], cam["W"]
    rng = np.random.default_rng(31)
    F = rng.random((P, 8)).astype(np.float32)
    G = rng.random((8, H, W)).astype(np.float32)
    _, f, img = oracle_splat(ro, cam, sc, F)
    _, _, acc = oracle_lift(ro, cam, sc, G)
    assert img.shape == (8, H, W) and acc.shape == (P, 9) and int(f["n_contrib"].sum()) > 50
    lhs, rhs = float((img * G.astype(np.float64)).sum()), float((F.astype(np.float64) * acc[:, 1:]).sum())
    print(f"{scene}: <splat F, G> = {lhs:.6f}, <F, lift G> = {rhs:.6f}, relative difference {abs(lhs - rhs) / rhs:.2e}")
    assert rhs > 1.0 and abs(lhs - rhs) <= 1e-6 * rhs
    # a channel of ones is the alpha image
    _, _, ones = oracle_splat(ro, cam, sc, np.ones((P, 1), np.float32))
    assert rel_err(ones[0], 1.0 - f["final_T"].astype(np.float64)) < 1e-6


def test_eight_channels_equal_three_chunked_calls():
    cam, sc = _SCENES["small"]()
    F = np.random.default_rng(32).normal(size=(80, 8)).astype(np.float32)
    _, _, img = oracle_splat(ro, cam, sc, F)
    for c0, c1 in ((0, 3), (3, 6), (6, 8)):
        _, _, part = oracle_splat(ro, cam, sc, F[:, c0:c1])
        assert part.shape == (c1 - c0, cam["H"], cam["W"]) and rel_err(img[c0:c1], part) < 1e-6
    _, _, one = oracle_splat(ro, cam, sc, F[:, 4])                        # [P] is C = 1
    assert one.shape == (1, cam["H"], cam["W"]) and rel_err(img[4:5], one) < 1e-6


def test_normalize_soft_masks():
    from multiview_inpaint_amd import mask_lift
    soft = torch.tensor([[[0.0, 0.25, 0.5], [0.3, 0.0, 1e-3]],
                         [[0.0, 0.75, 0.0], [0.0, 0.0, 0.0]]])
    alpha = torch.tensor([[0.0, 1.0, 0.5], [0.3, 0.0, 2e-3]])
    n = mask_lift.normalize_soft_masks(soft, alpha)
    want = torch.tensor([[[0.0, 0.25, 1.0], [1.0, 0.0, 0.5]],
                         [[0.0, 0.75, 0.0], [0.0, 0.0, 0.0]]])
    assert n.shape == soft.shape and torch.equal(n, want)
    assert bool(torch.isfinite(n).all()) and float(n.min()) >= 0.0 and float(n.max()) <= 1.0
    with pytest.raises(ValueError):
        mask_lift.normalize_soft_masks(soft, alpha[None])
    with pytest.raises(ValueError):
        mask_lift.normalize_soft_masks(soft[0], alpha)


def test_project_selection_checks_its_arguments_before_it_needs_a_device():
    from multiview_inpaint_amd import mask_lift
    means, op = torch.zeros(5, 3), torch.ones(5, 1)
    kw = dict(scales=torch.ones(5, 3), rotations=torch.ones(5, 4))
    with pytest.raises(ValueError, match="selection must be"):
        mask_lift.project_selection(torch.zeros(5, 2, 2), [], means, op, **kw)
    with pytest.raises(ValueError, match="selection must be"):
        mask_lift.project_selection([True] * 5, [], means, op, **kw)
    with pytest.raises(ValueError, match="selection must be"):
        mask_lift.project_selection(torch.zeros(5, 0), [], means, op, **kw)
    with pytest.raises(TypeError, match="bool or floating"):
        mask_lift.project_selection(torch.zeros(5, dtype=torch.int64), [], means, op, **kw)
    with pytest.raises(ValueError, match="4 rows for 5"):
        mask_lift.project_selection(torch.zeros(4, dtype=torch.bool), [], means, op, **kw)
    assert mask_lift.project_selection(torch.zeros(5, dtype=torch.bool), [], means, op, **kw) == []      # no views: no masks
    with pytest.raises(ValueError, match="no views"):
        mask_lift.propagate_masks([], [], means, op, **kw)
    m, K = mask_lift._selection_features(torch.tensor([True, False, True]), normalize=True)
    assert K == 1 and m.dtype == torch.float32 and m.tolist() == [[1.0, 1.0], [0.0, 1.0], [1.0, 1.0]]
    m, K = mask_lift._selection_features(torch.tensor([[0.5, 2.0]], dtype=torch.float64), normalize=False)
    assert K == 2 and m.dtype == torch.float32 and m.tolist() == [[0.5, 2.0]]

"""Host side of the on-demand geometry views: RasterState.tensor() has exactly `depths`, `cov3D_a`, `cov3D_b` and
`tiles_touched` filled before it copies (mvi_raster_materialize_geom_views) and no other view, and the library exports the
entry with the arguments the wrapper passes. No GPU."""
import types

import torch

from multiview_inpaint_amd import _lib, raster

ON_DEMAND = {"depths", "cov3D_a", "cov3D_b", "tiles_touched"}


def test_tensor_materialises_the_four_views_and_no_other(monkeypatch):
    names = [n for n, _ in _lib.RasterViews._fields_ if n != "tile_id_bytes"]
    assert ON_DEMAND <= set(names) and set(raster.RasterState.ON_DEMAND_GEOM_VIEWS) == ON_DEMAND
    calls = []
    monkeypatch.setattr(raster.RasterState, "materialize_geom_views", lambda self: calls.append("fill"))
    monkeypatch.setattr(raster.RasterState, "views",
                        lambda self: types.SimpleNamespace(tile_id_bytes=2, **{n: 0 for n in names}))
    st = raster.RasterState()
    st.P, st.D, st.W, st.H = 4, 0, 16, 16
    st.geom, st.binning, st.image = torch.empty(0, dtype=torch.uint8), None, None
    for n in names:
        calls.clear()
        out = st.tensor(n, (0,), torch.float32)                  # an empty copy: nothing is read from the (absent) scratch
        assert out.numel() == 0
        assert calls == (["fill"] if n in ON_DEMAND else []), (n, calls)
    calls.clear()
    st.tensor("depths", (0,), torch.float32, _derive=False)
    assert calls == []


def test_library_exports_the_materialiser():
    assert "mvi_raster_materialize_geom_views" in _lib.declared_symbols()
    L = _lib.lib()                                               # raises if a declared symbol is missing
    fn = L.mvi_raster_materialize_geom_views
    assert fn.restype is not None and len(fn.argtypes) == 9
    # argument checks run on the host: without settings the entry reports an error and touches no device
    assert fn(None, 0, None, None, None, None, None, None, None) == -1
    assert b"settings is NULL" in L.mvi_raster_last_error()

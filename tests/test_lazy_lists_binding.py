"""Host side of the tile-list expansion selector (include/mvi_raster.h, mvi_raster_list_expansion) and of the point-list
materialiser: the binding answers the query, selects both modes, refuses any other value without changing the selection,
MVI_RASTER_LAZY_LISTS sets the selection a fresh process starts with, RasterState.tensor("point_list") has the list
materialised before it copies, and the materialiser checks its arguments on the host. No GPU: nothing is launched."""
import os
import subprocess
import sys
import types

import torch

from multiview_inpaint_amd import _lib, raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_expansion_selector():
    assert "mvi_raster_list_expansion" in _lib.declared_symbols()
    L = _lib.lib()                                               # raises if a declared symbol is missing
    start = L.mvi_raster_list_expansion(-1)
    assert start in (0, 1)
    try:
        for mode in (0, 1, 1, 0):
            prev = L.mvi_raster_list_expansion(-1)
            assert L.mvi_raster_list_expansion(mode) == prev         # returns the previous selection
            assert L.mvi_raster_list_expansion(-1) == mode
        for keep in (0, 1):
            L.mvi_raster_list_expansion(keep)
            for bad in (2, 3, -2, 15, 1 << 20):
                assert L.mvi_raster_list_expansion(bad) == -1, bad   # MVI_EINVAL
                assert b"list expansion" in L.mvi_raster_last_error()
                assert L.mvi_raster_list_expansion(-1) == keep, "a refused value changed the selection"
    finally:
        L.mvi_raster_list_expansion(start)
    assert L.mvi_raster_list_expansion(-1) == start


def _fresh_process_mode(value):
    env = {k: v for k, v in os.environ.items() if k != "MVI_RASTER_LAZY_LISTS"}
    if value is not None:
        env["MVI_RASTER_LAZY_LISTS"] = value
    code = "from multiview_inpaint_amd import _lib; print(_lib.lib().mvi_raster_list_expansion(-1))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    return int(out.strip().splitlines()[-1])


def test_list_expansion_environment():
    """The variable is read once, when the library is loaded: "0" and "1" select, anything else leaves the built-in default."""
    default = _fresh_process_mode(None)
    assert default in (0, 1)
    assert _fresh_process_mode("0") == 0
    assert _fresh_process_mode("1") == 1
    for junk in ("2", "10", ""):
        assert _fresh_process_mode(junk) == default, junk


def test_tensor_materialises_the_point_list(monkeypatch):
    names = [n for n, _ in _lib.RasterViews._fields_ if n != "tile_id_bytes"]
    assert "point_list" in names and "front" in names
    calls = []
    monkeypatch.setattr(raster.RasterState, "materialize_point_list", lambda self: calls.append("list"))
    monkeypatch.setattr(raster.RasterState, "materialize_geom_views", lambda self: None)
    monkeypatch.setattr(raster.RasterState, "views",
                        lambda self: types.SimpleNamespace(tile_id_bytes=2, **{n: 0 for n in names}))
    st = raster.RasterState()
    st.P, st.D, st.W, st.H = 4, 0, 16, 16
    st.geom, st.binning, st.image = torch.empty(0, dtype=torch.uint8), None, None
    for n in names:
        calls.clear()
        assert st.tensor(n, (0,), torch.int32).numel() == 0
        assert calls == (["list"] if n == "point_list" else []), (n, calls)
    calls.clear()
    st.tensor("point_list", (0,), torch.int32, _derive=False)
    assert calls == []


def test_materialiser_checks_its_arguments():
    assert "mvi_raster_materialize_point_list" in _lib.declared_symbols()
    L = _lib.lib()
    fn = L.mvi_raster_materialize_point_list
    assert len(fn.argtypes) == 8
    assert fn(4, 0, 16, 16, None, None, None, None) == 0          # no pairs: nothing to write, no scratch needed
    assert fn(0, 5, 16, 16, None, None, None, None) == 0
    assert fn(4, 5, 16, 16, None, None, None, None) == -1
    assert b"NULL scratch" in L.mvi_raster_last_error()
    assert fn(4, -1, 16, 16, None, None, None, None) == -1
    assert fn(4, 1 << 33, 16, 16, None, None, None, None) == -1
    st = raster.RasterState()                                    # a state without pairs never calls the library
    st.P, st.D, st.W, st.H, st.geom, st.binning, st.image = 4, 0, 16, 16, None, None, None
    st.materialize_point_list()

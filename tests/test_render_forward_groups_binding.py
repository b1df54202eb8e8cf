"""Host side of the forward render kernel's group selector (include/mvi_raster.h, mvi_raster_forward_group): the binding answers
the query, selects every built instantiation, refuses a size that is not built without changing the selection, and 0 puts the
default back. No GPU: nothing is launched."""
from multiview_inpaint_amd import _lib

BUILT, DEFAULT = (1, 4), 4


def test_forward_group_selector():
    assert "mvi_raster_forward_group" in _lib.declared_symbols()
    L = _lib.lib()                                               # raises if a declared symbol is missing
    start = L.mvi_raster_forward_group(-1)
    assert start in BUILT
    try:
        assert L.mvi_raster_forward_group(0) == start and L.mvi_raster_forward_group(-1) == DEFAULT
        for g in BUILT:
            prev = L.mvi_raster_forward_group(-1)
            assert L.mvi_raster_forward_group(g) == prev             # returns the previous selection
            assert L.mvi_raster_forward_group(-1) == g
        keep = L.mvi_raster_forward_group(-1)
        for bad in (2, 3, 5, 6, 7, 8, 16, 64, -2, 1 << 20):
            assert L.mvi_raster_forward_group(bad) == -1, bad        # MVI_EINVAL
            assert b"forward group" in L.mvi_raster_last_error()
            assert L.mvi_raster_forward_group(-1) == keep, "a refused size changed the selection"
        assert L.mvi_raster_forward_group(0) == keep and L.mvi_raster_forward_group(-1) == DEFAULT
    finally:
        L.mvi_raster_forward_group(start)
    assert L.mvi_raster_forward_group(-1) == start

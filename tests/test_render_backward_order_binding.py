"""Host side of the render backward's tile-order selector (include/mvi_raster.h, mvi_raster_backward_order): the binding answers
the query, selects both orders, refuses any other value without changing the selection, and MVI_RASTER_BACKWARD_ORDER sets the
selection a fresh process starts with. No GPU: nothing is launched."""
import os
import subprocess
import sys

from multiview_inpaint_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_order_selector():
    assert "mvi_raster_backward_order" in _lib.declared_symbols()
    L = _lib.lib()                                               # raises if a declared symbol is missing
    start = L.mvi_raster_backward_order(-1)
    assert start in (0, 1)
    try:
        for order in (0, 1, 1, 0):
            prev = L.mvi_raster_backward_order(-1)
            assert L.mvi_raster_backward_order(order) == prev        # returns the previous selection
            assert L.mvi_raster_backward_order(-1) == order
        for keep in (0, 1):
            L.mvi_raster_backward_order(keep)
            for bad in (2, 3, -2, 15, 1 << 20):
                assert L.mvi_raster_backward_order(bad) == -1, bad   # MVI_EINVAL
                assert b"backward order" in L.mvi_raster_last_error()
                assert L.mvi_raster_backward_order(-1) == keep, "a refused value changed the selection"
    finally:
        L.mvi_raster_backward_order(start)
    assert L.mvi_raster_backward_order(-1) == start


def _fresh_process_order(value):
    env = {k: v for k, v in os.environ.items() if k != "MVI_RASTER_BACKWARD_ORDER"}
    if value is not None:
        env["MVI_RASTER_BACKWARD_ORDER"] = value
    code = "from multiview_inpaint_amd import _lib; print(_lib.lib().mvi_raster_backward_order(-1))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    return int(out.strip().splitlines()[-1])


def test_backward_order_environment():
    """The variable is read once, when the library is loaded: "0" and "1" select, anything else leaves the built-in default."""
    default = _fresh_process_order(None)
    assert default in (0, 1)
    assert _fresh_process_order("0") == 0
    assert _fresh_process_order("1") == 1
    for junk in ("2", "10"):
        assert _fresh_process_order(junk) == default, junk

"""A toy module shaped like multiview_inpaint_amd/svd/hip_ops.py — a global `torch`, a grow-only `_workspace`, wrappers that allocate their
outputs with torch.empty — in plain torch on the CPU, with the faults tests/test_memory_contract_cpu.py plants (fault=None: the correct
op). An access past the end of a tensor lands in whatever memory follows it: `_beyond` reaches it where the storage has room (under the
harness: the guard zone) and otherwise does nothing, as an unnoticed overrun would."""
import torch

_ws = {}
TILE = 4


def _workspace(dev, nbytes):
    """Grow-only scratch with a floor, never cleared after its creation (hip_ops._workspace)."""
    w = _ws.get("cpu")
    if w is None or w.numel() < nbytes:
        w = torch.zeros(max(nbytes, 1 << 12), dtype=torch.uint8)
        _ws["cpu"] = w
    return w


def _beyond(t, extra):
    """The flat view of contiguous t extended by `extra` elements past its end, or None where the storage ends with t."""
    n = t.numel()
    if t.untyped_storage().nbytes() < (t.storage_offset() + n + extra) * t.element_size():
        return None
    return torch.as_strided(t, (n + extra,), (1,), t.storage_offset())


def scale_rows(x, fault=None):
    """2 x of x [R, C], a tile of TILE rows at a time."""
    R, C = x.shape
    out = torch.empty_like(x)
    for r0 in range(0, R, TILE):
        r1 = min(R, r0 + TILE)
        if fault == "ragged_row" and r1 - r0 < TILE:
            r0 += 1                                              # the first row of the ragged last tile is never stored
        if fault == "last_element" and r1 == R:
            out[r0:r1 - 1] = 2.0 * x[r0:r1 - 1]
            out[r1 - 1, :-1] = 2.0 * x[r1 - 1, :-1]              # the last lane's store is masked off
        else:
            out[r0:r1] = 2.0 * x[r0:r1]
    if fault == "out_overrun":
        wide = _beyond(out, 1)
        if wide is not None:
            wide[-1] = 1.0
    if fault == "input_overread":
        wide = _beyond(x, 1)
        if wide is not None:
            out.view(-1)[-1] += 0.0 * wide[-1]                   # a lane past the end, "masked" by a multiply: NaN comes through
    if fault == "modifies_input":
        x[0, 0] = -x[0, 0] - 1.0
    return out


def _partials(x, slots, declared_slots):
    R, C = x.shape
    used = min(slots, -(-R // TILE))
    ws = _workspace(x.device, declared_slots(used) * C * 4)
    return ws, used


def col_sums(x, slots=4, fault=None):
    """Column sums of x [R, C] through per-chunk partial rows in the workspace: chunk i of the `used` chunks sums rows i, i + used, ..."""
    R, C = x.shape
    ws, used = _partials(x, slots, (lambda u: u) if fault != "stale_sum" else (lambda u: slots))
    part = ws[:ws.numel() // (C * 4) * C * 4].view(torch.float32).view(-1, C)
    for i in range(used):
        part[i] = x[i::used].sum(0)
    if fault == "ws_overrun":
        wide = _beyond(ws[:used * C * 4].view(torch.float32), 1)
        if wide is not None:
            wide[-1] = 3.0
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    out.copy_(part[:slots if fault == "stale_sum" else used].sum(0))
    return out


def col_max(x, slots=4, fault=None):
    """Column maxima of x [R, C] the same way; the merge drops NaN like v_max_f32 (torch.fmax)."""
    R, C = x.shape
    ws, used = _partials(x, slots, (lambda u: u) if fault != "stale_max" else (lambda u: slots))
    part = ws[:ws.numel() // (C * 4) * C * 4].view(torch.float32).view(-1, C)
    for i in range(used):
        part[i] = x[i::used].max(0).values
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    m = part[0].clone()
    for i in range(1, slots if fault == "stale_max" else used):
        m = torch.fmax(m, part[i])
    out.copy_(m)
    return out

"""The memory-contract harness (tests/memory_contract_helpers.py) catches what it claims to, shown on the CPU with a toy module shaped like
hip_ops (tests/memory_contract_toy.py): the correct ops pass, each of eight planted faults fails with a message that names the
allocation. And the coverage guard: every launching mvi_* entry hip_ops.py calls is named by a case of tests/memory_contract_cases.py,
the table tests/test_memory_contract_gpu.py runs."""
import os
import re

import pytest
import torch

import memory_contract_cases as T
import memory_contract_helpers as M
import memory_contract_toy as toy

R, C = 6, 5                                       # six rows: a full tile of four and a ragged one of two; two of four workspace slots used


def _x(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, C, generator=g) + 3.0   # positive column maxima: a zero slot does not move them


def _verify(monkeypatch, fn, backgrounds=M.BACKGROUNDS, **kw):
    return M.verify(monkeypatch, lambda x: fn(x, **kw), [_x()], module=toy, backgrounds=backgrounds)


def test_guarded_window_sits_between_two_guards_of_the_background():
    M.reset()
    t = M.guarded((3, 5), torch.float32, "cpu", 0x7B, "probe")
    a = M._REGISTRY[-1]
    assert t.is_contiguous() and t.shape == (3, 5) and t.dtype == torch.float32 and M.GUARD % 256 == 0
    assert a.buf.numel() == 2 * M.GUARD + 60 and a.offset == M.GUARD and bool((a.buf == 0x7B).all())
    assert t.data_ptr() == a.buf.data_ptr() + M.GUARD
    assert bool((t > 1e30).all())                                      # 0x7B7B7B7B: large, positive, finite
    for dt, big in ((torch.float32, 1e30), (torch.bfloat16, 1e30), (torch.float16, 5e4)):
        assert bool(torch.isnan(M.guarded((4,), dt, "cpu", 0xFF)).all())
        assert bool((M.guarded((4,), dt, "cpu", 0x7B) > big).all()) and bool((M.guarded((4,), dt, "cpu", 0xFB) < -big).all())
    assert bool((M.guarded((4,), torch.int32, "cpu", 0xFF) == -1).all())
    M.check()
    M.reset()


def test_correct_toy_ops_pass(monkeypatch):
    x = _x()
    (y,) = _verify(monkeypatch, toy.scale_rows)
    assert torch.equal(y, 2.0 * x)
    (s,) = _verify(monkeypatch, toy.col_sums)
    assert torch.allclose(s, x.sum(0))
    (m,) = _verify(monkeypatch, toy.col_max)
    assert torch.equal(m, x.max(0).values)
    assert toy.torch is torch and toy._workspace.__module__ == toy.__name__      # the patches are gone


@pytest.mark.parametrize("fn,fault,message", [
    (toy.scale_rows, "last_element", r"output 0 \(empty_like#\d+ torch.float32 \[6, 5\]\) has other bits .* elements 29 \.\. 29 of 30"),
    (toy.scale_rows, "ragged_row", r"output 0 \(empty_like#\d+ torch.float32 \[6, 5\]\) has other bits .* elements 20 \.\. 24 of 30"),
    (toy.col_sums, "stale_sum", r"output 0 \(empty#\d+ torch.float32 \[5\]\) has other bits under background 0xFF"),
    (toy.scale_rows, "out_overrun", r"bytes written after empty_like#\d+ torch.float32 \[6, 5\] .* offsets 12[0-3] \.\. 123 from the window's start"),
    (toy.col_sums, "ws_overrun", r"bytes written after workspace#\d+ \(40 declared bytes\) torch.uint8 \[40\] .* offsets 4[0-3] \.\. 43"),
    (toy.scale_rows, "input_overread", r"output 0 \(empty_like#\d+ torch.float32 \[6, 5\]\) has other bits under background 0xFF .* elements 29 \.\. 29"),
    (toy.scale_rows, "modifies_input", r"input 0 torch.float32 \[6, 5\] was modified .* offsets 0 \.\. 3 of 120"),
], ids=["last_element", "ragged_row", "stale_sum", "out_overrun", "ws_overrun", "input_overread", "modifies_input"])
def test_planted_fault_is_caught(monkeypatch, fn, fault, message):
    """Faults 1, 2, 3, 5, 6, 7, 8 of the list: an unwritten last element; an unwritten interior row of the ragged tile; a sum over
    workspace slots nobody wrote in this call; a store past the output; a store past the declared workspace bytes; a read past an input
    that reaches the result; a modified input."""
    with pytest.raises(AssertionError, match=message):
        _verify(monkeypatch, fn, fault=fault)
    assert toy.torch is torch                                          # restored after a failure too
    M.check()                                                          # and the registry is empty again


def test_max_over_an_unwritten_slot_is_caught_by_the_large_positive_background_only(monkeypatch):
    """Fault 4: zeros and a large negative value lose against the written maxima, NaN is dropped by the merge (torch.fmax, as
    v_max_f32 does) — only 0x7B shows the slot."""
    _verify(monkeypatch, toy.col_max, backgrounds=(0x00, 0xFF, 0xFB), fault="stale_max")
    with pytest.raises(AssertionError, match=r"output 0 \(empty#\d+ torch.float32 \[5\]\) has other bits under background 0x7B"):
        _verify(monkeypatch, toy.col_max, fault="stale_max")


def test_in_place_argument_is_declared_an_output(monkeypatch):
    def negate_(x):
        x.neg_()
        return x
    x = _x()
    with pytest.raises(AssertionError, match="input 0 .* was modified"):
        M.verify(monkeypatch, negate_, [x.clone()], module=toy, backgrounds=(0x00,))
    (y,) = M.verify(monkeypatch, negate_, [x], module=toy, inplace=(0,))
    assert torch.equal(y, -x) and torch.equal(x, _x())                 # each run had its own copy


def test_host_helpers_of_hip_ops_behave_under_the_proxy(monkeypatch):
    """The functions of hip_ops that make no launch give the same answers while the module's `torch` is the proxy and `_workspace` the
    guarded one; nothing is left patched."""
    from multiview_inpaint_amd.svd import hip_ops
    g = torch.Generator().manual_seed(3)
    w4, w5 = torch.randn(6, 4, 3, 3, generator=g), torch.randn(6, 4, 3, 1, 1, generator=g)
    v = torch.randn(7, 9, generator=g)
    real_ws = hip_ops._workspace

    def answers():
        return [hip_ops.conv3x3_transposed_weight(w4), hip_ops.conv3t_transposed_weight(w5), hip_ops.stem_conv3x3_transposed_weight(w4),
                hip_ops.conv3t_n320_weight(w5), *hip_ops.split_hi_lo(v), torch.tensor(hip_ops.conv_split3_s2_plan(3, 8, 6, 256))]
    plain = answers()
    for bg in M.BACKGROUNDS:
        with M.contract(monkeypatch, bg):
            assert hip_ops.torch is not torch and hip_ops.torch.float32 is torch.float32 and hip_ops.torch.cuda is torch.cuda
            assert hip_ops.GN_TOKENS == 2 and hip_ops.linear_dgrad_kernel.__module__ == hip_ops.__name__
            for a, b in zip(plain, answers()):
                assert torch.equal(a, b)
            ws = hip_ops._workspace(torch.device("cpu"), 24)
            assert ws.numel() == 24 and ws.dtype == torch.uint8 and bool((ws == bg).all())        # exactly the declared bytes, no floor
            z = hip_ops.torch.zeros(3)
            assert M._find(z) is None and not z.any()                                              # zeros stays real
            e = hip_ops.torch.empty(2, 3, dtype=torch.float16, device="cpu")
            assert M._find(e) is not None and e.shape == (2, 3) and bool((M.bits(e) == bg).all())
        assert hip_ops.torch is torch and hip_ops._workspace is real_ws
        M.check()
        M.reset()


# ---- the coverage guard -----------------------------------------------------------------------------------------------------------------------

HOST_ONLY = (r"_supported$", r"_workspace_bytes$", r"_bytes$", r"_out_rows$", r"_kernel_kind$", r"_kernel_variant$", r"_k_order$", r"_set_walk$",
             r"^mvi_conv_split3_group$", r"_blocks_per_group$", r"^mvi_unet_last_error$")
EXCLUDED = {}                                     # launching entry -> why no case names it; at most three


def _entries_hip_ops_calls():
    """Every mvi_* name hip_ops.py reaches through the library handle: L.mvi_x / _lib.lib().mvi_x, and the names it keeps as strings
    for getattr (the GroupNorm backward families)."""
    import multiview_inpaint_amd.svd as svd
    src = open(os.path.join(os.path.dirname(svd.__file__), "hip_ops.py")).read()
    return set(re.findall(r"(?:\bL|lib\(\))\.(mvi_\w+)", src)) | set(re.findall(r"\"(mvi_\w+)\"", src))


def test_every_launching_entry_of_hip_ops_has_a_case():
    called = _entries_hip_ops_calls()
    assert len(called) > 90 and "mvi_groupnorm_backward" in called and "mvi_rows_fused_gnstats" in called
    launching = {e for e in called if not any(re.search(p, e) for p in HOST_ONLY)}
    assert len(launching) >= 60, sorted(launching)
    assert len(EXCLUDED) <= 3 and all(isinstance(v, str) and v for v in EXCLUDED.values()) and set(EXCLUDED) <= launching
    missing = sorted(launching - T.COVERED - set(EXCLUDED))
    assert not missing, f"launching entries of hip_ops.py without a memory-contract case: {missing}"
    unknown = sorted(T.COVERED - launching)
    assert not unknown, f"the case table names entries hip_ops.py does not launch: {unknown}"


def test_the_case_table_is_well_formed():
    ids = [c.id for c in T.CASES]
    assert len(set(ids)) == len(ids)
    per_entry = {}
    for c in T.CASES:
        assert c.entries and set(c.tags) <= set(T.ALL) and callable(c.build), c.id
        for e in c.entries:
            per_entry.setdefault(e, []).append(c.id)
    assert all(len(v) >= 1 for v in per_entry.values())

"""Poisoned-buffer and canary tests for every UNet op wrapper of multiview_inpaint_amd/svd/hip_ops.py (the harness:
tests/memory_contract_helpers.py; the cases: tests/memory_contract_cases.py; what the harness catches: tests/test_memory_contract_cpu.py).

Per case: the wrapper runs once unpatched, then once per background byte (0x00, 0xFF = NaN, 0x7B / 0xFB = a large finite value of either
sign) with every output, every workspace window — exactly the declared bytes, no floor — and every input inside guard zones of that byte.
Asserted: every returned tensor has the bits of the unpatched run under all four backgrounds (an element the kernel did not store, a
reduce over a slot nobody wrote, a read past an input that reaches the result would differ); no guard byte changed (nothing is written
outside the outputs, the declared workspace and the inputs); every input holds the bits that were placed (the in-place ops declare their
argument an output); after a GroupNorm every word of the cluster counters is zero, the sticky timeout word included. The unpatched
result is then held once to the op's fp64 or exact reference with the bar of the op's own suite."""
import time

import pytest
import torch

import memory_contract_cases as T
import memory_contract_helpers as M

pytestmark = pytest.mark.gpu

SLOWEST = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops


@pytest.fixture(autouse=True)
def _nothing_runs_on_a_faulted_device():
    """A device fault is sticky: the run ends with the test that met it instead of launching the rest of the module on that device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is launched: {e}", returncode=3)


def _groupnorm_counters_are_zero(ops):
    torch.cuda.synchronize()
    for key, buf in ops._gn_sync.items():
        words = buf.view(torch.int32)
        assert int(words.ne(0).sum()) == 0, f"cluster GroupNorm counters of {key}: {int(words.ne(0).sum())} non-zero words (flag {int(words[2 * 65536])})"


@pytest.mark.parametrize("case,tag", T.PARAMS, ids=[f"{c.id}-{tag}" for c, tag in T.PARAMS])
def test_memory_contract(ops, monkeypatch, case, tag):
    t0 = time.perf_counter()
    b = case.build(ops, tag)
    torch.cuda.synchronize()
    after = (lambda: _groupnorm_counters_are_zero(ops)) if b.gn else None
    outs = M.verify(monkeypatch, b.call, b.inputs, inplace=b.inplace, after=after, foreign=b.foreign)
    assert any(o is not None for o in outs), case.id
    b.ref(outs)
    torch.cuda.synchronize()
    SLOWEST[f"{case.id}-{tag}"] = time.perf_counter() - t0


def test_report_the_slowest_cases():
    worst = sorted(SLOWEST.items(), key=lambda kv: -kv[1])[:5]
    print(f"memory contract: {len(SLOWEST)} cases in {sum(SLOWEST.values()):.1f} s; slowest: " + ", ".join(f"{k} {v:.2f} s" for k, v in worst))
    assert all(v < 10.0 for _, v in worst), worst

"""CPU side of the Add+LayerNorm backward's parity chain: the fp64 formula of tests/layernorm_bwd_helpers.py against fp64 autograd of
the unfused expression (1e-12) on every tensor fixture and every combination of absent h / row / gs / gs_pre, the fixtures' bits, and
the completeness of the recorded reference errors. No GPU."""
import itertools
import os

import numpy as np
import pytest
import torch

import layernorm_bwd_helpers as L

FIXTURES = [(case, tag) for case in L.TENSOR_CASES for tag in L.DTYPES]
IDS = [L.case_name(c, t) for c, t in FIXTURES]
COMBOS = list(itertools.product((True, False), repeat=4))          # h, row, gs, gsp present


@pytest.mark.parametrize("case,tag", FIXTURES, ids=IDS)
def test_formula_matches_fp64_autograd_of_the_unfused_expression(case, tag):
    inp0, _ = L.load_fixture(case, tag)
    worst = 0.0
    for has_h, has_row, has_gs, has_gsp in COMBOS:
        inp = dict(inp0)
        if not has_h:
            inp["h"] = None
        if not has_row:
            inp["row"] = None
        if not has_gs:
            inp["gs"] = None
        if not has_gsp:
            inp["gsp"] = None
        G = case.G if has_row else 0
        auto = L.autograd_unfused(inp, torch.float64)
        s64 = L.stream(*(None if inp[k] is None else inp[k].double() for k in ("x", "h", "row")))
        f = L.formula(s64, inp["w"], inp["gy"], inp["gs"], inp["gsp"], G)
        # the gradient of s_pre reaches x always and h when there is one; without h, s_pre IS x: its gradient and x's are one
        pairs = [(f["dx"], auto["dx"]), (f["dweight"], auto["dweight"]), (f["dbias"], auto["dbias"])]
        if has_h:
            pairs.append((f["dx"], auto["dh"]))
        if has_row:
            pairs.append((f["drow"], auto["drow"]))
        for got, ref in pairs:
            worst = max(worst, L.errors(got, ref)[0])
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("case,tag", FIXTURES, ids=IDS)
def test_fixtures_reload_to_the_same_bits(case, tag):
    inp, out = L.load_fixture(case, tag)
    again = L.make_inputs(case, L.DTYPES[tag])
    for k, v in again.items():
        assert (v is None) == (inp[k] is None), k
        if v is not None:
            assert np.array_equal(L.bits(v), L.bits(inp[k])), k
    f = L.truth(inp, case)
    for n in L.OUTPUTS:
        assert L.errors(f[n], out[n])[0] <= 1e-13, n               # (the order of an fp64 sum may differ between machines)


def test_every_gpu_case_has_its_own_recorded_reference_error():
    table = L.ref_errors()
    for case in L.GPU_CASES:
        for tag in L.DTYPES:
            e = table[L.case_name(case, tag)]
            want = [n for n in L.OUTPUTS if n != "drow" or case.G]
            for n in want:
                assert e[n + "_max"] > 0 and e[n + "_rms"] > 0, (case.name, tag, n)
    assert all(os.path.exists(os.path.join(L.GOLDEN, L.case_name(c, t) + ".npz")) for c, t in FIXTURES)


def test_default_routing_lines():
    """ops.add_layer_norm_backward_pays as profiles/layernorm_bwd_bench.json set it: from 28 x 2304 x 640 elements, not f16 "add", not
    fp32, nothing at the training latent's shapes."""
    from multiview_inpaint_amd.svd import ops
    bf, f16 = torch.bfloat16, torch.float16
    for variant in ("plain", "add", "row"):
        assert ops.add_layer_norm_backward_pays(28 * 9216, 320, bf, variant) and ops.add_layer_norm_backward_pays(28 * 2304, 640, bf, variant)
        assert not ops.add_layer_norm_backward_pays(28 * 576, 1280, bf, variant) and not ops.add_layer_norm_backward_pays(14 * 3072, 320, bf, variant)
        assert not ops.add_layer_norm_backward_pays(28 * 9216, 320, torch.float32, variant)
    assert ops.add_layer_norm_backward_pays(28 * 2304, 640, f16, "row") and ops.add_layer_norm_backward_pays(28 * 9216, 320, f16, "plain")
    assert not ops.add_layer_norm_backward_pays(28 * 9216, 320, f16, "add")

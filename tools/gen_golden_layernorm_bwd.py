"""Fixtures of the Add+LayerNorm backward (tests/golden/layernorm_bwd/), generated in the BUILD container from the imported reference:

    python tools/gen_golden_layernorm_bwd.py

The reference's transformer blocks chain `x = layer(norm(x)) + x` (sgm/modules/attention.py:544-572) with nn.LayerNorm as
BasicTransformerBlock builds it; here that module and `+` run under autograd on the CPU, in fp64 on inputs rounded to bf16 / f16 and
again in that 16-bit type (parameters in the activation type: a plain nn module under `.to(dtype)`): the reference's OWN error per
output (dx, dweight, dbias, drow), max-norm and rms, against the fp64 formula of tests/layernorm_bwd_helpers.py evaluated on the
forward's rounded residual stream. Every case the GPU tests run gets its own entry in ref_errors.json; the small cases also store
tensors (<case>_<type>.npz: inputs as bits, fp64 outputs). Arrays and numbers, no program text.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import layernorm_bwd_helpers as H  # noqa: E402
import ref_import  # noqa: E402


def run(LayerNorm, inp, dtype):
    """The reference's module and adds under autograd in `dtype`: dict dx, dh, dweight, dbias, drow."""
    R, C = inp["x"].shape
    norm = LayerNorm(C)
    assert norm.elementwise_affine and abs(norm.eps - H.EPS) < 1e-12
    with torch.no_grad():
        norm.weight.copy_(inp["w"].float())
        norm.bias.copy_(inp["b"].float())
    norm = norm.to(dtype)
    leaf = {k: (None if inp[k] is None else inp[k].detach().to(dtype).requires_grad_()) for k in ("x", "h", "row")}
    s_pre = leaf["x"] if leaf["h"] is None else leaf["h"] + leaf["x"]
    s = s_pre
    if leaf["row"] is not None:
        G = leaf["row"].shape[0]
        s = (s_pre.reshape(G, R // G, C) + leaf["row"][:, None, :]).reshape(R, C)
    y = norm(s)
    outs, grads = [y], [inp["gy"].to(dtype)]
    if inp["gs"] is not None:
        outs.append(s); grads.append(inp["gs"].to(dtype))
    if inp["gsp"] is not None:
        outs.append(s_pre); grads.append(inp["gsp"].to(dtype))
    torch.autograd.backward(outs, grads)
    gr = lambda t: None if t is None else t.grad
    return dict(dx=gr(leaf["x"]), dh=gr(leaf["h"]), dweight=norm.weight.grad, dbias=norm.bias.grad, drow=gr(leaf["row"]))


def one_case(LayerNorm, case, tag):
    dtype = H.DTYPES[tag]
    inp = H.make_inputs(case, dtype)
    r64 = run(LayerNorm, inp, torch.float64)
    f64 = H.formula(H.stream(*(None if inp[k] is None else inp[k].double() for k in ("x", "h", "row"))), inp["w"], inp["gy"], inp["gs"],
                    inp["gsp"], case.G)
    agree = max(H.errors(f64[n], r64[n])[0] for n in H.OUTPUTS if f64[n] is not None)
    assert agree < 1e-12, agree
    r16 = run(LayerNorm, inp, dtype)
    f = H.truth(inp, case)
    err = {}
    for n in H.OUTPUTS:
        if f[n] is not None:
            err[n + "_max"], err[n + "_rms"] = H.errors(r16[n], f[n])
    print(f"{H.case_name(case, tag)}: formula vs reference fp64 {agree:.1e}; reference's own error " +
          ", ".join(f"{n} {err[n + '_max']:.2e} / {err[n + '_rms']:.2e}" for n in H.OUTPUTS if n + "_max" in err), flush=True)
    return inp, f, err


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref_import.import_reference()
    from sgm.modules import attention
    LayerNorm = attention.nn.LayerNorm
    os.makedirs(H.GOLDEN, exist_ok=True)
    table = {}
    for case in H.GPU_CASES:
        for tag in H.DTYPES:
            inp, f, err = one_case(LayerNorm, case, tag)
            table[H.case_name(case, tag)] = err
            if case in H.TENSOR_CASES:
                arrays = {k: H.bits(v) for k, v in inp.items() if v is not None}
                arrays.update({"out_" + n: f[n].numpy() for n in H.OUTPUTS if f[n] is not None})
                np.savez_compressed(os.path.join(H.GOLDEN, H.case_name(case, tag) + ".npz"), **arrays)
    with open(os.path.join(H.GOLDEN, "ref_errors.json"), "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

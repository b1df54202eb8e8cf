"""Fixtures of the GEGLU backward (tests/golden/geglu_bwd/), generated in the BUILD container from the imported reference:

    python tools/gen_golden_geglu_bwd.py

The reference's GEGLU (sgm/modules/attention.py:87-95) is run under autograd in fp64 on seeded inputs rounded to bf16 / f16 — y, dx,
dweight, dbias — and again in that 16-bit type on the CPU: the reference's OWN error in the type, per gradient, as max-norm and rms
relative error. Small cases store tensors (<case>.npz, the fp64 results as fp64); the K = 320 shapes the GPU tests draw themselves
(same seeded inputs, tests/geglu_bwd_helpers.py) store the six error numbers only (ref_errors.json). Arrays and numbers, no program text.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import geglu_bwd_helpers as G  # noqa: E402
import ref_import  # noqa: E402


def run(GEGLU, dtype, x, w, b, dy):
    K, inner = x.shape[1], w.shape[0] // 2
    m = GEGLU(K, inner)
    with torch.no_grad():
        m.proj.weight.copy_(w.float())
        m.proj.bias.copy_(b.float())
    m = m.to(dtype)
    xa = x.to(dtype).requires_grad_()
    y = m(xa)
    y.backward(dy.to(dtype))
    return y.detach(), xa.grad, m.proj.weight.grad, m.proj.bias.grad


def one_case(GEGLU, case, tag):
    dtype = G.DTYPES[tag]
    x, w, b, dy = G.make_inputs(case, dtype)
    ref64 = run(GEGLU, torch.float64, x, w, b, dy)
    ref16 = run(GEGLU, dtype, x, w, b, dy)
    # the written-out formula against the reference's own fp64 autograd (what tests/test_geglu_bwd_cpu.py re-checks from the files)
    agree = max(G.errors(f, r)[0] for f, r in zip(G.formula(x, w, b, dy), ref64))
    err = {}
    for name, r16, r64 in zip(G.OUTPUTS, ref16[1:], ref64[1:]):
        err[name + "_max"], err[name + "_rms"] = G.errors(r16, r64)
    print(f"{G.case_name(case, tag)}: formula vs reference fp64 {agree:.1e}; reference's own error (max / rms) "
          + ", ".join(f"{n} {err[n + '_max']:.2e} / {err[n + '_rms']:.2e}" for n in G.OUTPUTS), flush=True)
    return (x, w, b, dy), ref64, err


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref_import.import_reference()
    from sgm.modules.attention import GEGLU
    os.makedirs(G.GOLDEN, exist_ok=True)
    for case in G.TENSOR_CASES:
        for tag in G.DTYPES:
            (x, w, b, dy), (y, dx, dw, db), err = one_case(GEGLU, case, tag)
            np.savez_compressed(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz"), x=G.bits(x), weight=G.bits(w), bias=G.bits(b),
                                dy=G.bits(dy), y=y.numpy(), dx=dx.numpy(), dweight=dw.numpy(), dbias=db.numpy(),
                                ref_err=np.array([err[f] for f in G.ERROR_FIELDS], dtype=np.float64))
    table = {}
    for case in G.ERROR_CASES:
        for tag in G.DTYPES:
            table[G.case_name(case, tag)] = one_case(GEGLU, case, tag)[-1]
    with open(os.path.join(G.GOLDEN, "ref_errors.json"), "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

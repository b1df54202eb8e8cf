"""Fixtures of the GroupNorm(+SiLU) backward (tests/golden/groupnorm_bwd/), generated in the BUILD container from the imported reference:

    python tools/gen_golden_groupnorm_bwd.py

The reference's own modules — `normalization(C)` + `nn.SiLU()` as `ResBlock.out_layers[:2]` uses them with `h + emb_out` in front
(openaimodel.py:341-353), the same on `b c t h w` for the temporal ResBlock (video_model.py:71-75), and `Normalize` (attention.py:125-128,
eps 1e-6, no SiLU) — run under autograd in fp64 on inputs rounded to bf16 / f16, and again in that 16-bit type on the CPU: the reference's
OWN error per output (y, dx, dweight, dbias, demb), max-norm and rms. In fp64 GroupNorm32 is entered through nn.GroupNorm.forward: its own
forward casts to fp32 first (util.py:274-276), which is the 16-bit recipe, not the oracle. Parameters stay fp32 in the 16-bit run, as
under the reference's autocast. Small cases store tensors (<case>.npz), training shapes the error numbers only (ref_errors.json). Arrays
and numbers, no program text.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import groupnorm_bwd_helpers as G  # noqa: E402
import ref_import  # noqa: E402


def run(mods, case, dtype, x, emb, dy, weight, bias):
    normalization, Normalize = mods
    norm = normalization(case.C) if case.silu else Normalize(case.C)
    assert norm.num_groups == G.GROUPS and abs(norm.eps - case.eps) < 1e-12
    with torch.no_grad():
        norm.weight.copy_(weight)
        norm.bias.copy_(bias)
    fp64 = dtype == torch.float64
    if fp64:
        norm = norm.double()
    elif not case.silu:
        norm = norm.to(dtype)                              # plain nn.GroupNorm: parameters in the activation type
    fwd = (lambda t: nn.GroupNorm.forward(norm, t)) if fp64 else norm
    x = x.to(dtype).requires_grad_()
    e = None if emb is None else emb.to(dtype).requires_grad_()
    N, C, H, W = x.shape
    T = case.T
    h = x.reshape(N // T, T, C, H, W).transpose(1, 2)      # (b t) c h w -> b c t h w
    if e is not None:
        h = h + e.reshape(N // T, T, C).transpose(1, 2)[..., None, None]      # b t c -> b c t 1 1
    if T == 1:
        h = h.reshape(N, C, H, W)
    y = fwd(h)
    if case.silu:
        y = nn.SiLU()(y)
    if T > 1:
        y = y.transpose(1, 2).reshape(N, C, H, W)
    y.backward(dy.to(dtype))
    return dict(y=y.detach(), dx=x.grad, dweight=norm.weight.grad, dbias=norm.bias.grad, demb=None if e is None else e.grad)


def one_case(mods, case, tag):
    dtype = G.DTYPES[tag]
    x, emb, dy, weight, bias = G.make_inputs(case, dtype)
    r64 = run(mods, case, torch.float64, x, emb, dy, weight, bias)
    r16 = run(mods, case, dtype, x, emb, dy, weight, bias)
    f = G.formula(x, emb, dy, weight, bias, case.T, case.silu, case.eps)
    agree = max(G.errors(f[n], r64[n])[0] for n in G.OUTPUTS if r64[n] is not None)
    err = {}
    for n in G.OUTPUTS:
        if r64[n] is not None:
            err[n + "_max"], err[n + "_rms"] = G.errors(r16[n], r64[n])
    print(f"{G.case_name(case, tag)}: formula vs reference fp64 {agree:.1e}; reference's own error " +
          ", ".join(f"{n} {err[n + '_max']:.2e} / {err[n + '_rms']:.2e}" for n in G.OUTPUTS if n + "_max" in err), flush=True)
    assert agree < 1e-11
    return (x, emb, dy, weight, bias), r64, err


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref_import.import_reference()
    from sgm.modules.attention import Normalize
    from sgm.modules.diffusionmodules.util import normalization
    mods = (normalization, Normalize)
    os.makedirs(G.GOLDEN, exist_ok=True)
    for case in G.TENSOR_CASES:
        for tag in G.DTYPES:
            (x, emb, dy, weight, bias), r64, err = one_case(mods, case, tag)
            arrays = dict(x=G.bits(x), dy=G.bits(dy), weight=weight.numpy(), bias=bias.numpy(),
                          ref_err=np.array([[err.get(n + "_max", np.nan), err.get(n + "_rms", np.nan)] for n in G.OUTPUTS]))
            if emb is not None:
                arrays["emb"] = emb.numpy()
            arrays.update({n: r64[n].numpy() for n in G.OUTPUTS if r64[n] is not None})
            np.savez_compressed(os.path.join(G.GOLDEN, G.case_name(case, tag) + ".npz"), **arrays)
    table = {}
    for case in G.ERROR_CASES:
        for tag in G.DTYPES:
            table[G.case_name(case, tag)] = one_case(mods, case, tag)[-1]
    with open(os.path.join(G.GOLDEN, "ref_errors.json"), "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

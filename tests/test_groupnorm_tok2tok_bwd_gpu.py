"""GPU parity of the token-major GroupNorm(+SiLU) under autograd: ops.group_norm_tok2tok through ops._GroupNormFn
(csrc/groupnorm_tokens.hip's forward with the statistics kept, csrc/groupnorm_bwd.hip's gn_bwd_tok_reduce_kernel / gn_bwd_tok_apply_kernel)
and the ResBlock middle that stays token-major behind layers.RESBLOCK_CONV_BWD.

Parity chain: the reference's modules under fp64 autograd -> the fp64 formula of tests/groupnorm_bwd_helpers.py
(tests/test_groupnorm_bwd_cpu.py, 1e-12) -> ops.group_norm_tok2tok's CPU path (tests/test_groupnorm_tok2tok_bwd_cpu.py, 1e-12) -> the
kernels (here). The token-major inputs are the transposes of the planes tensors of the fixtures / of G.make_inputs. Bars, 16-bit: the
error against fp64 as a multiple of the reference's OWN error in that type for the same output (fixture, or
tests/golden/groupnorm_bwd/ref_errors.json through G.ref_error_for): rms <= 1.6 x, max norm <= 2.0 x, the project's bars for 16-bit
gradient kernels. fp32 I/O: 1e-4 relative max norm per output. Every test runs with ops.STRICT = True and the speed decision
ops.group_norm_tok2tok_backward_pays lifted (the routing and module tests say where they differ)."""
import functools

import pytest
import torch

import groupnorm_bwd_helpers as G
import svd_helpers as H
from test_groupnorm_bwd_cpu import load_fixture

pytestmark = pytest.mark.gpu

RMS_BAR = 1.6
MAX_BAR = 2.0
FP32_BAR = 1e-4
DEV = "cuda"
ALL_DTYPES = dict(G.DTYPES, fp32=torch.float32)
# the shapes of tools/bench_groupnorm_tok2tok_bwd.py: (H, W, C) of the ResBlock middles of the training latent
BENCH_LEVELS = ((48, 64, 320), (24, 32, 640), (12, 16, 1280), (6, 8, 1280))


@pytest.fixture(autouse=True)
def _strict_hip_path(monkeypatch):
    from multiview_inpaint_amd.svd import layers, ops as dev_ops
    monkeypatch.setattr(dev_ops, "STRICT", True)
    monkeypatch.setattr(dev_ops, "GROUPNORM_TOK2TOK_BACKWARD", True)
    monkeypatch.setattr(dev_ops, "GROUPNORM_TOK2TOK_BACKWARD_MIN_ELEMENTS", 0)        # the speed decision, lifted
    monkeypatch.setattr(layers, "RESBLOCK_CONV_BWD", layers.RESBLOCK_CONV_BWD)         # (the module test sets it; restored here)


def _ops():
    from multiview_inpaint_amd.svd import hip_ops, ops
    return ops, hip_ops


def _tok(t):
    """planes [N, C, *spatial] -> token-major [N, S, C]"""
    return t.flatten(2).transpose(1, 2).contiguous()


def _check(name, n, got, ref, tag, r):
    e_max, e_rms = G.errors(got.detach().cpu(), ref)
    if tag == "fp32":
        H.report(f"{name} {n}: max {e_max:.2e}, rms {e_rms:.2e} (fp32 I/O)")
        return e_max <= FP32_BAR, (name, n, e_max, e_rms)
    r_max, r_rms = r[n + "_max"], r[n + "_rms"]
    H.report(f"{name} {n}: max {e_max:.2e} = {e_max / r_max:.2f} x, rms {e_rms:.2e} = {e_rms / r_rms:.2f} x the reference's own error")
    return e_max <= MAX_BAR * r_max and e_rms <= RMS_BAR * r_rms, (name, n, e_max, r_max, e_rms, r_rms)


def _assert_all(results):
    bad = [info for ok, info in results if not ok]
    assert not bad, bad


def _run(case, x, emb, dy, weight, bias, emb_grad=True, params_grad=True):
    """The case through ops.group_norm_tok2tok under autograd on the transposed tensors: (y, dict of gradients), y and dx token-major."""
    ops, _ = _ops()
    ta = _tok(x).to(DEV).requires_grad_()
    wa, ba = weight.to(DEV).requires_grad_(params_grad), bias.to(DEV).requires_grad_(params_grad)
    ea = None if emb is None else emb.to(DEV).requires_grad_(emb_grad)
    y = ops.group_norm_tok2tok(ta, G.GROUPS, wa, ba, case.eps, silu=case.silu, chan_bias=ea, frames=case.T)
    y.backward(_tok(dy).to(DEV))
    return y.detach(), dict(dx=ta.grad, dweight=wa.grad, dbias=ba.grad, demb=None if ea is None else ea.grad)


def _no_grad_y(case, x, emb, weight, bias):
    ops, _ = _ops()
    with torch.no_grad():
        return ops.group_norm_tok2tok(_tok(x).to(DEV), G.GROUPS, weight.to(DEV), bias.to(DEV), case.eps, silu=case.silu,
                                      chan_bias=None if emb is None else emb.to(DEV), frames=case.T)


def _parity(name, case, tag, inputs, ref, r):
    """y and the four gradients against `ref` (planes, fp64) at the bars; y under autograd = the no-grad y and a second backward = the
    first, bit for bit. Returns the gradients."""
    x, emb, dy, weight, bias = inputs
    y, grads = _run(case, x, emb, dy, weight, bias)
    assert torch.equal(y, _no_grad_y(case, x, emb, weight, bias)), "y under autograd must be the inference y, bit for bit"
    _, grads2 = _run(case, x, emb, dy, weight, bias)
    assert all(torch.equal(grads[n], grads2[n]) for n in grads if grads[n] is not None), "two backward runs must match bit for bit"
    results = [_check(name, "y", y.float(), _tok(ref["y"]), tag, r), _check(name, "dx", grads["dx"].float(), _tok(ref["dx"]), tag, r)]
    for n in ("dweight", "dbias", "demb"):
        if ref[n] is not None:
            results.append(_check(name, n, grads[n].float(), ref[n], tag, r))
    _assert_all(results)
    return grads


FIXTURES = [(case, tag) for case in G.TENSOR_CASES for tag in G.DTYPES]


@pytest.mark.parametrize("case,tag", FIXTURES, ids=[G.case_name(c, t) for c, t in FIXTURES])
def test_fixture_within_the_reference_own_error(case, tag):
    """Every fixture (odd_s45: a tail of tokens, C/G = 2; cg3: groups cross a vector; temporal_t2: frames = 2; normalize: no SiLU, no
    chan_bias, eps 1e-6; offset: cancellation) transposed, through ops.group_norm_tok2tok under autograd with frames = case.T, against the
    fixture's fp64 tensors at 1.6 x (rms) / 2.0 x (max) of the reference's own error in the fixture."""
    Z, x, emb, dy, weight, bias = load_fixture(case, tag)
    r = {n + s: float(Z["ref_err"][i][j]) for i, n in enumerate(G.OUTPUTS) for j, s in enumerate(("_max", "_rms"))}
    ref = {n: torch.from_numpy(Z[n]) if n in Z.files else None for n in G.OUTPUTS}
    _parity(G.case_name(case, tag), case, tag, (x, emb, dy, weight, bias), ref, r)


@functools.lru_cache(maxsize=2)
def _oracle(case, tag):
    """Seeded inputs and the fp64 formula on them, computed once per (case, dtype) and left unchanged."""
    inputs = G.make_inputs(case, ALL_DTYPES[tag])
    return inputs, G.formula(*inputs, case.T, case.silu, case.eps)


def _reduce_tile(C, tag):
    """Tokens per block of gn_bwd_tok_reduce_kernel / gn_bwd_tok_apply_kernel: 8 passes of rp rows, rp = 512 / (C / vector) clamped to
    [1, 8] (csrc/groupnorm_tok.h) — 64 tokens for C = 320 in bf16 (40 vectors per row), 48 in fp32 (80 vectors)."""
    vpr = C // (4 if tag == "fp32" else 8)
    return 8 * max(1, min(8, 512 // vpr))


def _edge_cases(tag):
    return [G.Case("edge_tile_plus_one", 1, 320, 1, _reduce_tile(320, tag) + 1, 1, True, True, 1e-5, True),     # one token past a tile
            G.Case("edge_s7", 2, 320, 1, 7, 1, True, True, 1e-5, True),                                        # S below one tile
            G.Case("edge_widest_6x8", 28, 2560, 6, 8, 1, True, True, 1e-5, True),                              # the widest row
            G.Case("edge_two_videos_t14", 28, 1280, 4, 4, 14, True, True, 1e-5, True)]                         # two 14-frame videos


@pytest.mark.parametrize("tag", ["bf16", "fp32"])
@pytest.mark.parametrize("index", range(4), ids=["tile_plus_one", "s7", "widest_6x8", "two_videos_t14"])
def test_edges_of_the_tiling(index, tag):
    """The edges of the token tiling against the fp64 formula evaluated on the spot; for each also: chan_bias present but not requiring
    grad gives demb None and the other three gradients the same bits."""
    assert (_reduce_tile(320, "bf16"), _reduce_tile(320, "fp32")) == (64, 48)
    case = _edge_cases(tag)[index]
    inputs, ref = _oracle(case, tag)
    r = None if tag == "fp32" else G.ref_error_for(case, tag)
    grads = _parity(G.case_name(case, tag), case, tag, inputs, ref, r)
    _, g3 = _run(case, *inputs, emb_grad=False)
    assert g3["demb"] is None and all(torch.equal(g3[n], grads[n]) for n in ("dx", "dweight", "dbias"))


def test_frozen_parameters_skip_the_parameter_launch():
    """weight / bias frozen: PROFILE holds groupnorm_tok2tok_bwd and no groupnorm_tok2tok_bwd_params, dx has the bits of the trainable
    run; trainable: the _params kind."""
    _, hip_ops = _ops()
    case = _edge_cases("bf16")[1]
    inputs, _ = _oracle(case, "bf16")
    hip_ops.PROFILE = []
    try:
        _, frozen = _run(case, *inputs, params_grad=False)
        kinds_frozen = [p[0] for p in hip_ops.PROFILE]
        del hip_ops.PROFILE[:]
        _, full = _run(case, *inputs)
        kinds_full = [p[0] for p in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = None
    assert kinds_frozen == ["groupnorm_tok2tok_stats_fwd", "groupnorm_tok2tok_bwd"], kinds_frozen
    assert kinds_full == ["groupnorm_tok2tok_stats_fwd", "groupnorm_tok2tok_bwd_params"], kinds_full
    assert frozen["dweight"] is None and frozen["dbias"] is None
    assert torch.equal(frozen["dx"], full["dx"]) and torch.equal(frozen["demb"], full["demb"])


TRAINING = {c.name: c for c in G.ERROR_CASES}
SHAPES = [(TRAINING[n], tag) for n in ("n2_c320_48x64", "n2_c640_24x32", "n2_c2560_6x8", "t14_c1280_12x16") for tag in ALL_DTYPES]


@pytest.mark.parametrize("case,tag", SHAPES, ids=[G.case_name(c, t) for c, t in SHAPES])
def test_training_shapes_against_the_fp64_formula(case, tag):
    """The training shapes (the temporal one with frames = 14), transposed, against the fp64 formula evaluated on this machine's CPU."""
    inputs, ref = _oracle(case, tag)
    r = None if tag == "fp32" else G.ref_error_for(case, tag)
    _parity(G.case_name(case, tag), case, tag, inputs, ref, r)


def test_routing_and_strict_mode():
    """The switch off, or a shape the gate refuses (C = 36 with 4 groups in bf16: no multiple of the vector): HipPathError under strict
    mode; with strict lifted the PyTorch route runs and FALLBACKS holds ("group_norm_tok2tok", "requires grad"). The speed decision
    answers a bool for every shape of the bench list."""
    ops, hip_ops = _ops()
    g = torch.Generator().manual_seed(3)

    def call(C, groups):
        t = torch.randn(2, 48, C, generator=g).to(torch.bfloat16).to(DEV).requires_grad_()
        w, b = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
        y = ops.group_norm_tok2tok(t, groups, w, b, 1e-5, silu=True)
        y.sum().backward()
        return t.grad

    def both_checks(C, groups):
        ops.STRICT = True
        with pytest.raises(ops.HipPathError):
            call(C, groups)
        ops.STRICT = False                                           # (restored by the module's fixture)
        del ops.FALLBACKS[:]
        assert call(C, groups).shape == (2, 48, C)
        assert ("group_norm_tok2tok", "requires grad") in ops.FALLBACKS, ops.FALLBACKS

    assert hip_ops.group_norm_tok2tok_backward_supported(2, 64, 48, 32, 1, torch.bfloat16)
    ops.STRICT = True
    del ops.FALLBACKS[:]
    call(64, 32)                                                     # switch on: the HIP route, no fallback
    assert not ops.FALLBACKS, ops.FALLBACKS
    ops.GROUPNORM_TOK2TOK_BACKWARD = False
    both_checks(64, 32)
    ops.GROUPNORM_TOK2TOK_BACKWARD = True
    assert not hip_ops.group_norm_tok2tok_backward_supported(2, 36, 48, 4, 1, torch.bfloat16)
    both_checks(36, 4)
    for N in (14, 28):
        for h, w, C in BENCH_LEVELS:
            for dt in (torch.bfloat16, torch.float16):
                assert isinstance(ops.group_norm_tok2tok_backward_pays(N, C, h * w, 1, dt), bool)


def _seed_params(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.copy_((1.0 if n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
            p.copy_(p.to(torch.bfloat16).to(p.dtype))


@pytest.mark.parametrize("channels", [320, 640])
def test_resblock_middle_against_the_parent_route(channels, monkeypatch):
    """layers.ResBlock(channels, 1280, 0.0, out_channels=320), bf16, under checkpoint(use_reentrant=False) with RESBLOCK_CONV_BWD on and
    the speed decisions lifted, at the smallest batch of 48x64 frames at which layers._conv_bwd_path_ok holds (found from the gates; 14
    if none below holds): input and parameter gradients against the fp64 CPU module. Yardstick: the same block in the same process with
    GROUPNORM_TOK2TOK_BACKWARD off — the parent's middle, transposing copy + ops.group_norm_tokens — against the same fp64 result; the
    new middle's error per tensor is at most 1.6 x (rms) / 2.0 x (max) of it. ops.STRICT = False for both (the skip adds still record
    fallbacks). The new route's PROFILE holds one groupnorm_tok2tok_bwd* per backward and its FALLBACKS no group_norm_tok2tok entry;
    checked with every parameter trainable and frozen with only x requiring grad."""
    from torch.utils.checkpoint import checkpoint
    from multiview_inpaint_amd.svd import layers
    ops, hip_ops = _ops()
    dt = torch.bfloat16
    monkeypatch.setattr(ops, "conv3x3_backward_pays", lambda *a: True)
    monkeypatch.setattr(ops, "group_norm_backward_pays", lambda *a, **k: True)
    ops.STRICT = False                                               # (restored by the module's fixture)
    layers.RESBLOCK_CONV_BWD = True

    def make():
        m = layers.ResBlock(channels, 1280, 0.0, out_channels=320)
        _seed_params(m, 23)
        return m
    probe = make().to(DEV, dt)

    def path_ok(n):
        return layers._conv_bwd_path_ok(probe, torch.empty(n, channels, 48, 64, device=DEV, dtype=dt).requires_grad_(),
                                        torch.empty(n, 1280, device=DEV, dtype=dt))
    N = next((n for n in range(1, 14) if path_ok(n)), 14)
    H.report(f"ResBlock {channels} -> 320, 48x64 bf16: smallest batch on the conv-backward route = {N}")
    assert path_ok(N)
    del probe
    g = torch.Generator().manual_seed(29)
    x = torch.randn(N, channels, 48, 64, generator=g).to(dt)
    emb = torch.randn(N, 1280, generator=g).to(dt)
    dy = torch.randn(N, 320, 48, 64, generator=g).to(dt)
    m64 = make().double()
    x64 = x.double().requires_grad_()
    m64(x64, emb.double()).backward(dy.double())
    ref = {"x": x64.grad, **{n: p.grad for n, p in m64.named_parameters() if p.grad is not None}}

    def gpu_run(trainable=True):
        m = make().to(DEV, dt).requires_grad_(trainable)
        xg = x.to(DEV).requires_grad_()
        del ops.FALLBACKS[:]
        hip_ops.PROFILE = []
        try:
            checkpoint(m, xg, emb.to(DEV), use_reentrant=False).backward(dy.to(DEV))
            kinds = [p[0] for p in hip_ops.PROFILE]
        finally:
            hip_ops.PROFILE = None
        return {"x": xg.grad, **{n: p.grad for n, p in m.named_parameters() if p.grad is not None}}, kinds, list(ops.FALLBACKS)

    new, kinds, fallbacks = gpu_run()
    assert kinds.count("groupnorm_tok2tok_bwd_params") == 1 and kinds.count("groupnorm_tok2tok_bwd") == 0, kinds
    assert not [f for f in fallbacks if f[0] == "group_norm_tok2tok"], fallbacks
    frozen, kinds_f, fallbacks_f = gpu_run(trainable=False)
    assert kinds_f.count("groupnorm_tok2tok_bwd") == 1 and kinds_f.count("groupnorm_tok2tok_bwd_params") == 0, kinds_f
    assert not [f for f in fallbacks_f if f[0] == "group_norm_tok2tok"], fallbacks_f
    ops.GROUPNORM_TOK2TOK_BACKWARD = False                           # the parent's middle
    old, old_kinds, _ = gpu_run()
    old_frozen, _, _ = gpu_run(trainable=False)
    ops.GROUPNORM_TOK2TOK_BACKWARD = True
    assert not [k for k in old_kinds if k.startswith("groupnorm_tok2tok")], old_kinds
    assert set(new) == set(old) and set(new) <= set(ref), (set(new) ^ set(old), set(new) - set(ref))
    bad = []
    for name in list(new) + ["frozen x"]:
        got, yard, key = (frozen["x"], old_frozen["x"], "x") if name == "frozen x" else (new[name], old[name], name)
        o_max, o_rms = G.errors(yard.cpu(), ref[key])
        e_max, e_rms = G.errors(got.cpu(), ref[key])
        H.report(f"ResBlock {channels} {N}x48x64 bf16 d{name}: max {e_max:.2e} = {e_max / o_max:.2f} x, rms {e_rms:.2e} = "
                 f"{e_rms / o_rms:.2f} x the parent middle's own error")
        if not (e_max <= MAX_BAR * o_max and e_rms <= RMS_BAR * o_rms):
            bad.append((name, e_max, o_max, e_rms, o_rms))
    assert not bad, bad

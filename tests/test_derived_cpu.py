"""svd/derived.py — the one rule for values cached per parameter — alone (a hit, an in-place update, ANOTHER parameter object at the
same address and version, a changed `extra`, eviction when a source dies) and through the sites that work without a GPU: after a
parameter is replaced by another object on the same storage, each site returns what a fresh, unrelated parameter holding the new values
gives, exactly. No GPU."""
import gc

import pytest
import torch
import torch.nn as nn

from multiview_inpaint_amd.svd import derived as D


class Recycled:
    """Two nn.Parameter objects on ONE storage, each with its own version counter at 0 — what the caching allocator produces on the GPU
    when a freed model's block is handed to the next model: `old` holds the first values; replace() overwrites the storage through the
    buffer (no version bump on `old`) and returns (the new parameter on that storage, a fresh unrelated parameter with the same values)."""

    def __init__(self, shape, dtype=torch.float32, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.buf = torch.randn(shape, generator=g).to(dtype)
        self.new = torch.randn(shape, generator=g).to(dtype)
        self.old = nn.Parameter(self.buf.data)

    def replace(self):
        self.buf.copy_(self.new)
        p2 = nn.Parameter(self.buf.data)
        assert p2 is not self.old and p2.data_ptr() == self.old.data_ptr() and p2._version == self.old._version == 0
        return p2, nn.Parameter(self.new.clone())


def _counting(fn):
    calls = []

    def build(*a):
        calls.append(1)
        return fn(*a)
    return build, calls


@pytest.mark.parametrize("single", [False, True], ids=["derived", "derived1"])
def test_helper_hit_update_recycled_address_extra_and_eviction(single):
    gc.collect()
    size0 = len(D._table)
    r = Recycled((5, 3))
    p = r.old
    if single:
        build, calls = _counting(lambda s: s.detach() * 2)
        get = lambda s, extra=(): D.derived1("t", s, build, extra)
    else:
        q = nn.Parameter(torch.ones(3))
        build, calls = _counting(lambda: cur[0].detach() * 2 + q.detach())
        get = lambda s, extra=(): D.derived("t", (s, q), build, extra)
    cur = [p]
    v = get(p)
    assert get(p) is v and len(calls) == 1                              # 1: a hit is the identical object
    p2, _ = r.replace()
    cur[0] = p2
    v3 = get(p2)
    assert v3 is not v and len(calls) == 2                             # 3: another object at the same address and version rebuilds
    assert torch.equal(v3, p2.detach() * 2 + (0 if single else 1)) and not torch.equal(v3, v)
    with torch.no_grad():
        p2.add_(1)
    v2 = get(p2)
    assert v2 is not v3 and len(calls) == 3 and get(p2) is v2          # 2: an in-place update rebuilds
    assert get(p2, extra=1) is not v2 and len(calls) == 4              # 4: a changed extra rebuilds
    assert len(D._table) > size0
    del p, p2, cur, r, get, build                                       # 5: the entries leave with their sources
    gc.collect()
    assert len(D._table) == size0


def test_table_holds_no_source():
    import weakref
    p = nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))
    D.derived1("t", p, lambda s: s.detach().float())
    D.derived("t2", (p,), lambda: 0)
    ref = weakref.ref(p)
    del p
    gc.collect()
    assert ref() is None


def test_signature_holds_only_for_the_same_live_unchanged_sources():
    r = Recycled((4,))
    other = nn.Parameter(torch.zeros(2))
    sig = D.Signature([r.old, other], extra=(False, False))
    assert sig.holds([r.old, other], (False, False))
    assert not sig.holds([r.old, other], (False, True)) and not sig.holds([r.old], (False, False))
    p2, _ = r.replace()
    assert not sig.holds([p2, other], (False, False))
    with torch.no_grad():
        other.mul_(2)
    assert not sig.holds([r.old, other], (False, False))


# ---- the sites ------------------------------------------------------------------------------------------------------------------

def _site_f32(p):
    from multiview_inpaint_amd.svd import hip_ops
    return hip_ops._f32(p)


def _site_sum_param(p):
    from multiview_inpaint_amd.svd import layers
    return layers._sum_param(_FIXED_BIAS, p)


def _site_channels_last(p):
    from multiview_inpaint_amd.svd import layers
    w = layers._channels_last_weight(p)
    assert w.is_contiguous(memory_format=torch.channels_last)
    return w


_FIXED_BIAS = nn.Parameter(torch.arange(6, dtype=torch.float32))
_CONV3 = nn.Conv3d(2, 3, (3, 1, 1), padding=(1, 0, 0))
_X3 = torch.randn(4, 6, 5, 5, generator=torch.Generator().manual_seed(5))


def _site_temporal_conv3_stacked(p):
    from multiview_inpaint_amd.svd import layers
    _CONV3.weight = p
    with torch.no_grad():
        return layers.temporal_conv3_stacked(_X3, _CONV3)


_ATTN = []


def _site_packed_qkv(p):
    from multiview_inpaint_amd.svd.transformer import CrossAttention
    if not _ATTN:
        torch.manual_seed(1)
        _ATTN.append(CrossAttention(query_dim=8, heads=2, dim_head=4))
    m = _ATTN[0]
    m.to_q.weight = p
    w, folded = m._packed_qkv_weight()
    assert not folded and torch.equal(w[8:], torch.cat([m.to_k.weight, m.to_v.weight]).detach())
    return w


_SVT = []


def _site_frame_embedding_mlp(p):
    from multiview_inpaint_amd.svd.transformer import SpatialVideoTransformer
    if not _SVT:
        torch.manual_seed(2)
        _SVT.append(SpatialVideoTransformer(32, 2, 16, use_linear=True, context_dim=8, use_spatial_context=True).eval())
    m = _SVT[0]
    m.time_pos_embed[2].weight = p
    with torch.no_grad():
        return m._frame_embedding_mlp(3, 2, torch.device("cpu"))


SITES = [
    (_site_f32, (6,), torch.bfloat16),
    (_site_sum_param, (6,), torch.float32),
    (_site_channels_last, (4, 3, 3, 3), torch.float32),
    (_site_temporal_conv3_stacked, (3, 2, 3, 1, 1), torch.float32),
    (_site_packed_qkv, (8, 8), torch.float32),
    (_site_frame_embedding_mlp, (32, 128), torch.float32),
]


@pytest.mark.parametrize("site,shape,dtype", SITES, ids=[s[0].__name__[6:] for s in SITES])
def test_site_sees_a_parameter_replaced_at_the_same_address(site, shape, dtype):
    r = Recycled(shape, dtype, seed=11)
    first = site(r.old).clone()
    assert torch.equal(site(r.old), first)
    p2, fresh = r.replace()
    got = site(p2)
    want = site(fresh)
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(got, first)
